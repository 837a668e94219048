"""CPU checks of the config-4 oracle hooks (poke_goal, the arbiter census) and of the scene generator tests/dyn_scenes.py."""
import collections

import numpy as np

import dyn_scenes as DS


def _batch(O, scenes):
    polys, goals = DS.bank_arrays(len(DS.RECORDS))
    ob = O.Batch(len(scenes), DS.oracle_cfg(O), polys, goals, map_ids=np.array([s.rec for s in scenes], dtype=np.int32))
    ob.reset()
    return ob


def test_poke_goal_is_a_body_reset_there(oracle):
    """A poked goal moves exactly as one the record had placed there: same bodies, arbiters and outputs over 20 steps."""
    O = oracle
    s = DS.Scene("gap", "t", "open", {}, {0: (70.0, 200.0, 3.0, -1.0), 1: (81.0, 203.0)})
    a = _batch(O, [s])
    DS.poke(O, a, 0, *s.pokes[0][1:])
    # the same bodies from the record: goal positions are the record's, velocities poked (v_bias, w stay zero)
    polys, goals = DS.bank_arrays(len(DS.RECORDS))
    goals[s.rec, 0] = (70.0, 200.0); goals[s.rec, 1] = (81.0, 203.0)
    b = O.Batch(1, DS.oracle_cfg(O), polys, goals, map_ids=np.array([s.rec], dtype=np.int32))
    b.reset()
    for k in range(3):
        b.poke_traffic(0, k, *s.pokes[0][1][k])
    b.poke_goal(0, 0, 70.0, 200.0, 3.0, -1.0)
    act = np.full(1, DS.ACTION, dtype=np.int32)
    for k in range(20):
        oa, ra, da = a.step(act)
        ob_, rb, db = b.step(act)
        np.testing.assert_array_equal(a.peek_dyn(0)["goals"], b.peek_dyn(0)["goals"])
        np.testing.assert_array_equal(a.peek_dyn(0)["traffic"], b.peek_dyn(0)["traffic"])
        assert a.census(0) == b.census(0)
        np.testing.assert_array_equal(ra, rb)
    assert a.peek_dyn(0)["goals"][0, 0] != 70.0                  # it did move


def test_census_matches_the_solver_list_and_ageing(oracle):
    """The census list is last_arbiters long, in canonical order; arbiters age 1, 2 as CACHED and are gone at 3; a touched
    arbiter has age 0 and is FIRST (new or back from CACHED) or NORMAL."""
    O = oracle
    scenes = [s for s in DS.persist_scenes() if "goal-bank away" in s.tag]
    r = DS.run_oracle(O, scenes, len(DS.RECORDS), 12)
    for k, cen in enumerate(r["census"]):
        for e, c in enumerate(cen):
            assert len(c["list"]) == r["dyn"][k][e]["arbiters"]
            for a, b, cnt, st in c["list"]:
                assert cnt >= 1 and st in (1, 2)
            for (i, j), a in c["arbs"].items():
                assert i < j and a["state"] in (1, 2, 4) and 0 <= a["age"] < 3
                assert (a["state"] == 4) == (a["age"] > 0)
    # the goal-bank contact: away j steps from step 2, back at 2 + j: ages 1..min(j, 2), then FIRST again (j <= 2: the same
    # arbiter, warm-started; j >= 3: a new one)
    for e, s in enumerate(scenes):
        j = int(s.tag.split()[2])
        ages = [c["arbs"].get((0, 2), {}).get("age") for c in (r["census"][k][e] for k in range(12))]
        assert ages[:2] == [0, 0], (s.tag, ages)
        assert ages[2: 2 + j] == [1, 2, None, None][:j], (s.tag, ages)
        assert r["census"][2 + j][e]["arbs"][(0, 2)]["state"] == 1, s.tag
        if j <= 2:  # warm start: the cached impulse is carried over (circle contacts: hash 0 == 0)
            assert r["census"][1][e]["arbs"][(0, 2)]["jn"][0] >= 0.0


def test_scene_generator_coverage(oracle):
    """Deterministic; every family; solver-list lengths 0..9 and above 12; an EPA hull above 7; CircleToCircle at dist 0; the
    interleaved record holds every length class; envs with >= 5 cached and >= 5 ageing arbiters in one step."""
    O = oracle
    a, b = DS.build_scenes(O), DS.build_scenes(O)
    assert [s.tag for s in a] == [s.tag for s in b]
    assert all(np.array_equal(p[1], q[1]) for s, t in zip(a, b) for p, q in zip(s.pokes, t.pokes))
    fam = collections.Counter(s.family for s in a)
    assert set(fam) == set(DS.FAMILIES), fam
    r = DS.run_oracle(O, a, len(DS.RECORDS), 8)
    cen = r["census"]
    lens = collections.Counter(len(c["list"]) for step in cen for c in step)
    assert all(lens[m] > 0 for m in range(10)) and max(lens) > 12, sorted(lens.items())
    assert max(c["epa_hull"] for step in cen for c in step) > 7
    assert sum(c["c2c_zero"] for step in cen for c in step) > 0
    n_cached = [max(sum(a_["state"] == 4 for a_ in c["arbs"].values()) for c in step) for step in cen]
    n_aging = [max(sum(a_["state"] == 4 and a_["age"] == 1 for a_ in c["arbs"].values()) for c in step) for step in cen]
    assert max(n_cached) >= 5 and max(n_aging) >= 5, (n_cached, n_aging)
    open_lens = {len(cen[0][e]["list"]) for e, s in enumerate(a) if s.rec == DS.REC["open"]}
    assert {0, 1, 2}.issubset(open_lens) and max(open_lens) > 8
    print("solver-list lengths over 8 steps:", " ".join("%d:%d" % kv for kv in sorted(lens.items())))
