"""The event scenes (tests/event_scenes.py) and their exact classifier against the CPU oracle alone.

On every CLEAR predicate the oracle's colliding / goal_reached / listed goals equal the classifier's verdict; reward, done and the
event reasons of every scene and step follow the precedence table; every family keeps its share of CLEAR and BAND target
predicates; the scenes hit the lanes, planes, plane chunks, queue positions and steps they were built for.
"""
import collections

import numpy as np
import pytest

import event_scenes as ES

_built = {}


def _scenes(O, n_goals):
    if n_goals not in _built:
        _built[n_goals] = ES.build_scenes(O, n_goals)
    return _built[n_goals]


@pytest.mark.parametrize("n_goals,auto_reset,dyn", [(5, True, False), (5, False, False), (1, True, False), (6, False, False), (5, True, True)])
def test_oracle_agrees_with_the_classifier_and_the_table(oracle, n_goals, auto_reset, dyn):
    O = oracle
    recs, hulls, scenes, _ = _scenes(O, n_goals)
    assert 2048 <= len(scenes) <= 4096 and len(scenes) % 64
    ref = ES.run_oracle(O, recs, scenes, 10, 2, n_goals, auto_reset, dyn=dyn)
    cls = ES.classify_run(O, hulls, scenes, ref)
    bad = []
    for k in range(ES.K):
        pk = ref["peek"][k]
        for e, s in enumerate(scenes):
            v = cls[k][e]
            if v.colliding[1] and v.colliding[0] != (pk[e, 9] != 0):
                bad.append((k, s.tag, "colliding", v.hull, pk[e, 9]))
            if v.reached[1] and v.reached[0] != (pk[e, 10] != 0):
                bad.append((k, s.tag, "goal_reached", v.goal, pk[e, 10]))
            if v.listed[1] and v.listed[0] != int(pk[e, 13]):
                bad.append((k, s.tag, "listed goals", v.listed, pk[e, 13]))
    assert not bad, (len(bad), bad[:8])
    # the table, from the oracle's own predicates: its reward and done bit for bit, its cumulative reward
    rew, done, ev, cum = ES.expected(ref, False, auto_reset)
    np.testing.assert_array_equal(rew, ref["rew"])
    np.testing.assert_array_equal(done, ref["done"])
    np.testing.assert_array_equal(cum, ref["after"][-1][:, 12])
    fixed = ES.expected(ref, True, auto_reset)
    col_only = ((ev & ES.EV_COLLIDING) != 0) & ((ev & ES.EV_GOAL_REACHED) == 0)
    assert col_only.sum() > 100 and (fixed[0][col_only] == -1.0).all() and np.array_equal(fixed[0][~col_only], rew[~col_only])
    assert np.array_equal(fixed[1], done) and np.array_equal(fixed[2], ev)
    # every event reason occurs, alone and with others
    seen = collections.Counter(ev[0].tolist())
    for bit in (ES.EV_COLLIDING, ES.EV_GOAL_REACHED, ES.EV_OUT_OF_BOUNDS, ES.EV_MAX_STEPS, ES.EV_NO_GOALS_LEFT):
        alone = seen[bit] > 0
        if bit == ES.EV_GOAL_REACHED and n_goals == 1:  # (the one goal reached leaves none)
            alone = True
        assert alone and sum(n for f, n in seen.items() if f & bit and f != bit) > 0, (bit, seen)
    count = ES.count_targets(scenes, cls, ref)
    print({f: (count[(f, True)], count[(f, False)]) for f in ES.FAMILIES}, "(clear, band) target predicates per family")
    ES.check_conditions(count)


@pytest.mark.parametrize("dyn", [False, True])
def test_precedence_combinations(oracle, dyn):
    """every combination of (colliding, goal reached, out of bounds, step limit, no goals left) that the geometry allows: no goals
    left without a goal reached needs an empty list from the start, everything else is free"""
    recs, hulls, scenes, _ = _scenes(oracle, 5)
    ref = ES.run_oracle(oracle, recs, scenes, 10, 2, 5, False, dyn=dyn, steps=1)
    pk = ref["peek"][0]
    got = set()
    for e, s in enumerate(scenes):
        if s.family != "precedence" or s.meta.get("kind") != "combo":
            continue
        c, o, lim, tag = s.meta["want"]
        p = pk[e]
        real = (p[9] != 0, p[10] != 0, p[0] < 0, p[7] >= ES.MAX_STEPS, p[8] == 0)
        assert real == (bool(c), tag.startswith("reached"), bool(o), bool(lim), "none" in tag), (s.tag, real)
        got.add(real)
    assert len(got) == 2 * 2 * 2 * 4  # (colliding, out, limit) x (not reached / reached) x (goals left / none left)


@pytest.mark.parametrize("n_goals", [1, 5, 6])
def test_scenes_hit_what_they_were_built_for(oracle, n_goals):
    O = oracle
    recs, hulls, scenes, info = _scenes(O, n_goals)
    ship = ES.Ship(O)
    fam = collections.defaultdict(list)
    for e, s in enumerate(scenes):
        fam[s.family].append((e, s))
    assert set(fam) == set(ES.FAMILIES)
    # the interleaved part fills whole waves and mixes the families in every one of them
    assert info["mixed"] % 64 == 0
    for w in range(info["mixed"] // 64):
        assert len({s.family for s in scenes[64 * w: 64 * w + 64]}) >= 6, w

    def planes_in_front(h, sv):
        """the bank planes of h that have all five ship vertices strictly in front (stage 1's separating axes)"""
        return [j for j in range(h.count) if all(h.n[j][0] * (x - h.v[j][0]) + h.n[j][1] * (y - h.v[j][1]) > 0 for x, y in sv)]

    def ship_planes_in_front(h, pose, sv):
        """the ship planes that have every hull vertex strictly in front (stage 2's second fold)"""
        out = []
        for i in range(5):
            n = ES._rot(ship.ln[i], pose[2])
            if all(n[0] * (x - sv[i][0]) + n[1] * (y - sv[i][1]) > 0 for x, y in h.v):
                out.append(i)
        return out

    # sat_bank_axis: plane j alone separates a scene built 1e-9 or more outside; no plane does 1e-9 or more inside; every plane
    # index of hulls of 3, 4, 5, 8, 9, 12 planes on both hulls, both sides of the chunks of four, all five ship vertices
    seen = collections.defaultdict(set)
    for _, s in fam["sat_bank_axis"]:
        h = hulls[s.rec][s.meta["s"]]
        sv, bb = ship.world(*s.pose)
        front = planes_in_front(h, sv)
        if s.meta["off"] >= 1e-9:
            assert front == [s.meta["plane"]], (s.tag, front)
            assert bb[0] <= h.bb[2] and h.bb[0] <= bb[2], s.tag  # past the x-extent reject: the SAT decides
        elif s.meta["off"] <= -1e-9:
            assert front == [] and ship_planes_in_front(h, s.pose, sv) == [], (s.tag, front)
        seen[(s.meta["s"], h.count)].add(s.meta["plane"])
        seen["verts"].add(s.meta["vert"])
        seen["chunk", s.meta["s"]].add((s.meta["plane"] // 4, h.count % 4 != 0))
    for sd in (0, 1):
        for cnt in (3, 4, 5, 8, 9, 12):
            assert seen[(sd, cnt)] == set(range(cnt)), (sd, cnt)
        assert {(0, True), (1, True), (2, True), (0, False), (1, False), (2, False)} <= seen["chunk", sd]
    assert seen["verts"] == set(range(5))
    # sat_ship_axis (and serve's decisive scene): no bank plane separates, ship plane i alone does when 1e-9 or more outside
    seen = collections.defaultdict(set)
    for _, s in fam["sat_ship_axis"] + [x for x in fam["serve"] if x[1].meta["served"]]:
        h = hulls[s.rec][s.meta["s"]]
        sv, _ = ship.world(*s.pose)
        assert planes_in_front(h, sv) == [], s.tag
        sp = ship_planes_in_front(h, s.pose, sv)
        assert sp == ([s.meta["edge"]] if s.meta["off"] >= 1e-9 else []) or abs(s.meta["off"]) < 1e-9, (s.tag, sp)
        if s.family == "sat_ship_axis":
            seen["edges"].add(s.meta["edge"])
            seen[h.count].add(s.meta["q"])
    assert seen["edges"] == set(range(5))
    for cnt in (3, 4, 5, 8, 9, 12):
        assert {0, cnt - 1} <= seen[cnt], cnt
    assert 11 in seen[12]  # lanes 55 .. 59 of stage 2
    # sat_vertex_vertex: the two vertices at the offset from each other; nothing separates when 1e-9 or more inside
    for _, s in fam["sat_vertex_vertex"]:
        h = hulls[s.rec][s.meta["s"]]
        sv, _ = ship.world(*s.pose)
        v, q = sv[s.meta["vert"]], h.v[s.meta["q"]]
        d = np.hypot(v[0] - q[0], v[1] - q[1])
        if s.meta["off"] >= 0:
            assert abs(d - s.meta["off"]) < 1e-11, (s.tag, d)
        if s.meta["off"] <= -1e-9:
            assert planes_in_front(h, sv) == [] and ship_planes_in_front(h, s.pose, sv) == [], s.tag
    # sat_contain: ship inside, both hulls, and the small hull inside the ship's box
    kinds = collections.Counter(s.meta["kind"] for _, s in fam["sat_contain"])
    assert kinds["inside"] >= 10 and kinds["both"] >= 6 and kinds["in_box"] >= 28, kinds
    for _, s in fam["sat_contain"]:
        if s.meta["kind"] == "in_box":
            h = hulls[s.rec][s.meta["s"]]
            _, bb = ship.world(*s.pose)
            assert bb[0] < h.bb[0] and h.bb[2] < bb[2] and bb[1] < h.bb[1] and h.bb[3] < bb[3], s.tag
    # reject: the extents meet exactly where they were meant to
    eq = collections.Counter()
    for _, s in fam["reject"]:
        h = hulls[s.rec][s.meta["s"]]
        _, bb = ship.world(*s.pose)
        if s.meta["kind"] == "x_eq_y_far":
            eq["x", bb[0] == h.bb[2] or bb[2] == h.bb[0]] += 1
            assert bb[1] > h.bb[3] + 20 or bb[3] < h.bb[1] - 20, s.tag
        elif s.meta["kind"] == "y_eq_x_far":
            eq["y", bb[1] == h.bb[3]] += 1
            assert bb[0] > h.bb[2] + 20 or bb[2] < h.bb[0] - 20, s.tag
    assert eq["x", True] >= 20 and eq["x", False] >= 20 and eq["y", True] >= 8 and eq["y", False] >= 8, eq
    # serve: 1, 2, 63 and 64 served lanes per wave, lanes 0, 31, 32, 63 alone; the last wave is partly filled
    sets = []
    for tag, e0 in info["serve_waves"]:
        w = scenes[e0:e0 + 64]
        assert e0 % 64 == 0 and all(s.family == "serve" and s.meta["lane"] == i for i, s in enumerate(w))
        sets.append(sorted(i for i, s in enumerate(w) if s.meta["served"]))
        for s in w:  # a far lane is dropped by the x-extent reject on both hulls, a served one passes it on its hull
            _, bb = ship.world(*s.pose)
            near = [bb[0] <= h.bb[2] and h.bb[0] <= bb[2] for h in hulls[s.rec]]
            assert near == ([True, False] if s.meta["served"] else [False, False]), s.tag
    assert sets[:5] == [[0], [31], [32], [63], [31, 32]] and len(sets[5]) == 63 and len(sets[6]) == 64
    last = scenes[info["serve_last"]:]
    for s in last:
        _, bb = ship.world(*s.pose)
        assert (bb[0] <= hulls[s.rec][0].bb[2]) == s.meta["served"] and bb[2] < hulls[s.rec][1].bb[0], s.tag
    assert info["serve_last"] % 64 == 0 and 0 < len(last) < 64 and [i for i, s in enumerate(last) if s.meta["served"]] == [0, 31, 32, 36]
    # goal_queue: the pair counts per wave, and the reached pair at its queue position, pass and slot
    counts, singles = {}, set()
    for tag, e0 in info["gq_waves"]:
        w = scenes[e0:e0 + 64]
        assert e0 % 64 == 0 and all(s.family == "goal_queue" for s in w)
        order = ES.queue_order(list(enumerate(w)), n_goals, ship)
        if tag.startswith("single"):
            pos = int(tag.split()[1])
            lane, g = order[pos]
            assert len(order) == 25 and w[lane].meta.get("pos") == pos and w[lane].meta["g"] == g, (tag, order)
            assert sum(1 for s in w if s.meta["kind"] == "single") == 1
            in_pass = order[12 * (pos // 12): 12 * (pos // 12) + 12]
            assert len({ln for ln, _ in in_pass}) == len(in_pass)  # the pass straddles lanes: every pair another lane's
            singles.add((pos // 12, pos % 12))
        else:
            counts[tag] = len(order)
    assert counts == {"count 0": 0, "count 1": 1, "count 11": 11, "count 12": 12, "count 13": 13, "count 24": 24, "count 25": 25, "all": 64 * n_goals}
    assert singles == {(p // 12, p % 12) for p in range(25)}
    # goal_dist: every region of every edge and vertex; the box reject at equality on its four sides
    kinds = collections.Counter((s.meta["kind"], s.meta.get("feat")) for _, s in fam["goal_dist"])
    for i in range(5):
        for kind in ("edge", "vertex", "extension"):
            assert kinds[(kind, i)] == len(ES.OFFSETS), (kind, i)
        assert kinds[("on_vertex", i)] == 1 and kinds[("inside", i)] >= 2
    sides = collections.Counter()
    for _, s in fam["goal_dist"]:
        if s.meta["kind"] == "box":
            c, (_, bb) = ES.CLUSTER[s.meta["g"]], ship.world(*s.pose)
            sides[(c[0] - ES.GOAL_R == bb[2], bb[0] == c[0] + ES.GOAL_R, c[1] - ES.GOAL_R == bb[3], bb[1] == c[1] + ES.GOAL_R)] += 1
    assert all(sides[tuple(i == j for j in range(4))] >= 2 * len({0, n_goals - 1}) for i in range(4)), sides
    # bounds, limit, approach, exact
    xs = {(s.pose[0], np.signbit(s.pose[0])) for _, s in fam["bounds"]} | {(s.pose[1], np.signbit(s.pose[1])) for _, s in fam["bounds"]}
    for v in (0.0, -0.0, -5e-324, 5e-324, 600.0, np.nextafter(600.0, np.inf), np.nextafter(600.0, 0.0)):
        assert (v, np.signbit(v)) in xs, v
    assert {s.steps0 for _, s in fam["limit"] if s.target} == {ES.MAX_STEPS - d for d in range(6)}
    assert {(s.meta["kind"], s.meta["step"]) for _, s in fam["approach"] if "step" in s.meta} == {(kd, k) for kd in ("bank", "goal", "bound") for k in range(ES.K)}
    for _, s in fam["exact"]:
        assert s.pose[2] == 0.0
        for h in hulls[s.rec]:
            assert all(abs(nx) + abs(ny) == 1.0 and nx * ny == 0.0 for nx, ny in h.n), s.tag  # unit normals without rounding
    assert all(abs(nx) + abs(ny) == 1.0 for nx, ny in ship.ln[:3])


def test_approach_crosses_in_its_step(oracle):
    """a moving scene's target predicate turns at the step it was built for: false before it, true after it"""
    recs, hulls, scenes, _ = _scenes(oracle, 5)
    ref = ES.run_oracle(oracle, recs, scenes, 10, 2, 5, False)
    cls = ES.classify_run(oracle, hulls, scenes, ref)
    n = 0
    for e, s in enumerate(scenes):
        if s.family != "approach" or "step" not in s.meta:
            continue
        for k in range(ES.K):
            tp = ES.target_pred(s, cls[k][e])
            if tp is None:  # the goal has gone
                assert s.meta["kind"] == "goal" and k > s.meta["step"]
                continue
            if k != s.meta["step"]:
                assert tp == (k > s.meta["step"], True), (s.tag, k, tp)
                n += 1
            elif abs(s.meta["off"]) >= 1e-9:
                assert tp == (s.meta["off"] < 0, True), (s.tag, k, tp)
    assert n > 200


def test_exact_family_is_the_closed_set_verdict(oracle):
    """touching collides, one ulp apart does not, one ulp inside does: the oracle on the exact family"""
    recs, hulls, scenes, _ = _scenes(oracle, 5)
    ref = ES.run_oracle(oracle, recs, scenes, 10, 2, 5, False, steps=1)
    seen = collections.Counter()
    for e, s in enumerate(scenes):
        if s.family == "exact":
            col = ref["peek"][0][e, 9] != 0
            seen[(s.meta["ulp"], col)] += 1
    assert seen[(0, True)] == 12 and seen[(0, False)] == 0 and seen[(-1, False)] + seen[(1, False)] == 12 and seen[(-1, True)] + seen[(1, True)] == 12, seen
