"""Config-4 contact scenes at the edges of the full cpSpaceStep (dyn_step_kernel), and their oracle run.

A scene is one env: a bank record, the three traffic ships' poses and velocities, the five goal bodies, a constant player action
(1: the rudder only, so the player stays at the spawn point) and a list of pokes (step, ships, goals): the bodies are written
before that step, as a test writes the F_TRAFFIC / F_GOAL_BODIES columns.  Everything is deterministic from one seed.

Families (FAMILIES):
  pile      goals and ships stacked on one spot against a bank, sized by the oracle's solver-list length N (0 .. 36 on the open
            record's one bank; up to 44 on the pinch record, where both banks overlap under the stack)
  gap       every pair type (goal-bank, goal-goal, ship-bank, goal-ship, ship-ship, player-ship) at signed gaps 0, +-1e-9 x the
            coordinate scale and +-1e-3, angle 0, zero velocity (every operation on both sides is the same IEEE operation); the
            player-ship gaps run out past the step kernel's dyn_reach2 reject radius; a tilted ship on a bank edge keeps one of
            its two clipped contacts
  deep      a goal centre inside a bank and inside a ship, two coincident goal centres (n = (1, 0)), coincident bounding-box
            centres (zero GJK axis), overlapping parallel ship edges (two contacts, clip clamps), ships deep in 12-plane banks
            (EPA hulls of more than 7 entries).  The GJK / EPA iteration caps (30) are not reached: on these shapes (a circle or
            a 5-gon against at most a 12-gon) GJK ends in a handful of steps and EPA's hull stops growing once it holds the
            Minkowski difference's vertices, at most 17.
  ties      ships at angle 0 and pi against the axis-aligned bank edges at their corners and against each other
  persist   a contact separated for 1, 2, 3 and 4 steps, then back (CACHED -> FIRST with a contact-hash warm start, or dropped);
            a two-contact ship arbiter tilted to one contact; stacks of 5 .. 9 arbiters all separated in one step
  removal   the player reaches a goal in the step the goal touches a ship or another goal
  dup       copies of pile / gap scenes parked for one step and poked one step after their twins: the memo answers them
"""
import math

import numpy as np

W = H = 600.0
SCALE = 600.0
EPS = 1e-9 * SCALE
ACTION = 1
FAMILIES = ("pile", "gap", "deep", "ties", "persist", "removal", "dup")
GOAL_R = 5.0
# ship k's hull: models.py:6 SHIP_TEMPLATE scaled by add_default_traffic's (width, height)
TEMPLATE = ((0, 0), (0, 10), (5, 15), (10, 10), (10, 0))
SHIP_SCALE = ((1.0, 1.0), (1.5, 2.0), (1.0, 3.0))
PLAYER = (300.0, 25.0)  # spawn; its hull is the template x (2, 3): x 300..320, y 25..70, tip (310, 70)
PARK_SHIPS = ((200.0, 530.0), (250.0, 525.0), (300.0, 520.0))
PARK_GOALS = tuple((350.0 + 20.0 * g, 580.0) for g in range(5))


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _ngon(cx, cy, rx, ry, k, phase):
    return [(cx + rx * math.cos(phase + 2 * math.pi * i / k), cy + ry * math.sin(phase + 2 * math.pi * i / k)) for i in range(k)]


def pad12(pts):
    """A convex polygon of k <= 12 vertices as the 12 points a bank record holds: the rest are interior points (hulled away)."""
    pts = [tuple(map(float, p)) for p in pts]
    cx = sum(p[0] for p in pts) / len(pts)
    cy = sum(p[1] for p in pts) / len(pts)
    out = list(pts)
    i = 0
    while len(out) < 12:
        p = pts[i % len(pts)]
        f = 0.15 + 0.1 * (i // len(pts))
        out.append((cx + f * (p[0] - cx) + 0.37 * (i + 1), cy + f * (p[1] - cy) - 0.29 * (i + 1)))
        i += 1
    return np.array(out, dtype=np.float64)


# record 0 holds every family interleaved; 1 and 2 are homogeneous pile blocks; 3 holds the 12-plane banks
RECORDS = (
    ("open", _rect(0, 0, 60, 600), _rect(540, 0, 600, 600)),
    ("open_pile", _rect(0, 0, 60, 600), _rect(540, 0, 600, 600)),
    ("pinch", _rect(0, 300, 310, 420), _rect(290, 300, 600, 420)),
    ("twelve", _ngon(110, 300, 75, 190, 12, 0.1), _ngon(490, 300, 75, 190, 12, 0.35)),
)
REC = {name: i for i, (name, _, _) in enumerate(RECORDS)}


def bank_arrays(n_records):
    """(polys [n][2][12][2], goals [n][5][2]) of a bank of n_records >= len(RECORDS): the scene records first, then copies of the
    open record nobody is reset to (a bank of more than 64 records runs the per-lane-planes kernel)."""
    polys, goals = [], []
    for i in range(n_records):
        _, left, right = RECORDS[i] if i < len(RECORDS) else RECORDS[0]
        polys.append(np.stack([pad12(left), pad12(right)]))
        goals.append(np.array(PARK_GOALS))
    return np.stack(polys), np.stack(goals)


class Scene:
    def __init__(self, family, tag, rec, ships, goals, pokes=()):
        self.family, self.tag, self.rec = family, tag, REC[rec]
        # pokes: (step, ships [3][6] x y angle vx vy w, goals [5][4] x y vx vy); step 0 = right after the reset
        self.pokes = [(0, _ships(ships), _goals(goals))] + [(s, _ships(sh), _goals(go)) for s, sh, go in pokes]


def _ships(over):
    out = np.zeros((3, 6))
    for k in range(3):
        out[k, :2] = PARK_SHIPS[k]
    for k, v in (over or {}).items():
        v = list(v) + [0.0] * (6 - len(v))
        out[k] = v
    return out


def _goals(over):
    out = np.zeros((5, 4))
    for g in range(5):
        out[g, :2] = PARK_GOALS[g]
    for g, v in (over or {}).items():
        v = list(v) + [0.0] * (4 - len(v))
        out[g] = v
    return out


# ------------------------------------------------------------------------------------------------------------- families
GAPS = (-1e-3, -EPS, 0.0, EPS, 1e-3)


def gap_scenes():
    out = []
    for i, y in enumerate((150.0, 230.0, 380.0)):
        for gp in GAPS:
            t = "y%d gap %g" % (y, gp)
            out.append(Scene("gap", "goal-bank0 " + t, "open", {}, {0: (60.0 + GOAL_R + gp, y)}))
            out.append(Scene("gap", "goal-bank1 " + t, "open", {}, {1: (540.0 - GOAL_R - gp, y)}))
            out.append(Scene("gap", "goal-goal " + t, "open", {}, {0: (200.0, y), 1: (200.0 + 2 * GOAL_R + gp, y)}))
            out.append(Scene("gap", "goal-goal-v " + t, "open", {}, {2: (220.0, y), 3: (220.0, y + 2 * GOAL_R + gp)}))
            out.append(Scene("gap", "ship-bank0 " + t, "open", {0: (60.0 + gp, y)}, {}))
            out.append(Scene("gap", "ship-bank1 " + t, "open", {2: (540.0 - 10.0 - gp, y)}, {}))
            # goal left of ship 1's left edge (x = 300, y 300..320), below its bottom edge
            out.append(Scene("gap", "goal-ship " + t, "open", {1: (300.0, y)}, {0: (300.0 - GOAL_R - gp, y + 8.0)}))
            out.append(Scene("gap", "goal-ship-bottom " + t, "open", {1: (300.0, y)}, {4: (305.0, y - GOAL_R - gp)}))
            # ship 0's right edge (x + 10, y .. y + 10) against ship 1's left edge: parallel, two clipped contacts
            out.append(Scene("gap", "ship-ship " + t, "open", {0: (200.0, y), 1: (210.0 + gp, y)}, {}))
            out.append(Scene("gap", "ship-ship-2 " + t, "open", {1: (400.0, y), 2: (415.0 + gp, y + 5.0)}, {}))
        # a ship tilted on the bank edge: one of the two clipped contacts is kept (margins 0.05)
        for a in (0.01, -0.01):
            x = 60.05 if a > 0 else 59.95 + 0.1
            out.append(Scene("gap", "ship-bank0 one-of-two a=%g y%d" % (a, y), "open", {0: (x, y, a)}, {}))
    # the player (x 300..320, y 25..55 at its right edge) against ship 0 on its right: the step kernel's collide_ship, and its
    # dyn_reach2 reject radius at larger gaps
    for gp in GAPS + (0.5, 2.0, 10.0, 25.0, 40.0, 60.0, 90.0):
        out.append(Scene("gap", "player-ship gap %g" % gp, "open", {0: (320.0 + gp, 30.0)}, {}))
        out.append(Scene("gap", "player-ship-left gap %g" % gp, "open", {2: (300.0 - 10.0 - gp, 20.0)}, {}))
    return out


def deep_scenes():
    out = []
    for y in (150.0, 260.0):
        out.append(Scene("deep", "goal in bank0 y%d" % y, "open", {}, {0: (30.0, y)}))
        out.append(Scene("deep", "goal centre on bank edge y%d" % y, "open", {}, {0: (60.0, y)}))
        out.append(Scene("deep", "goal in ship1 y%d" % y, "open", {1: (300.0, y)}, {0: (307.0, y + 12.0)}))
        out.append(Scene("deep", "coincident goals y%d" % y, "open", {}, {0: (200.0, y), 1: (200.0, y)}))
        out.append(Scene("deep", "coincident goals x3 y%d" % y, "open", {}, {2: (240.0, y), 3: (240.0, y), 4: (240.0, y)}))
        # ship 1's box centre (307.5, y + 15): a goal there, and ship 0 with the same box centre
        out.append(Scene("deep", "bb centres goal-ship y%d" % y, "open", {1: (300.0, y)}, {0: (307.5, y + 15.0)}))
        out.append(Scene("deep", "bb centres ship-ship y%d" % y, "open", {0: (302.5, y + 7.5), 1: (300.0, y)}, {}))
        out.append(Scene("deep", "parallel overlap y%d" % y, "open", {0: (200.0, y), 1: (209.5, y)}, {}))
        out.append(Scene("deep", "parallel overlap offset y%d" % y, "open", {0: (200.0, y + 4.0), 1: (209.0, y)}, {}))
    # ship 2 (10 x 45) and ship 1 driven into the 12-plane banks at several depths
    for d in (2.0, 8.0, 20.0, 40.0, 70.0, 100.0):
        out.append(Scene("deep", "ship2 in twelve-left d=%g" % d, "twelve", {2: (185.0 - d, 278.0)}, {}))
        out.append(Scene("deep", "ship1 in twelve-right d=%g" % d, "twelve", {1: (415.0 + d - 15.0, 285.0, 0.3)}, {}))
        out.append(Scene("deep", "ship0 in twelve-left tilted d=%g" % d, "twelve", {0: (185.0 - d, 300.0, -0.7)}, {}))
    return out


def tie_scenes():
    out = []
    for gp in (-1e-3, 0.0, 1e-3):
        # angle 0: ship 0's left edge on bank 0's edge at the corner (60, 0) and (60, 600) ends; ship 2 against bank 1's corner
        out.append(Scene("ties", "ship0 corner-lo gap %g" % gp, "open", {0: (60.0 + gp, -5.0)}, {}))
        out.append(Scene("ties", "ship0 corner-hi gap %g" % gp, "open", {0: (60.0 + gp, 590.0)}, {}))
        out.append(Scene("ties", "ship2 corner-lo gap %g" % gp, "open", {2: (530.0 - gp, -20.0)}, {}))
        out.append(Scene("ties", "ships 0-1 flush tops gap %g" % gp, "open", {0: (200.0, 300.0), 1: (210.0 + gp, 300.0)}, {}))
    for gp in (-1e-3, 1e-3):  # angle pi: the rotation is not exact, clear margins only
        out.append(Scene("ties", "ship0 pi on bank0 gap %g" % gp, "open", {0: (70.0 + gp, 215.0, math.pi)}, {}))
        out.append(Scene("ties", "ship1 pi vs ship0 gap %g" % gp, "open", {0: (200.0, 300.0), 1: (225.0 + gp, 320.0, math.pi)}, {}))
        out.append(Scene("ties", "ship2 pi corner gap %g" % gp, "open", {2: (550.0 - gp, 20.0, math.pi)}, {}))
    return out


def persist_scenes():
    out = []
    touch = 60.0 + GOAL_R - 0.05      # 0.05 deep: inside the slop, the goal stays at rest
    for j in (1, 2, 3, 4):
        for y in (150.0, 300.0):
            away = {0: (80.0, y)}
            back = {0: (touch, y)}
            out.append(Scene("persist", "goal-bank away %d y%d" % (j, y), "open", {}, back, [(2, {}, away), (2 + j, {}, back)]))
            # a ship flat on the bank (two contacts), lifted away and put back
            out.append(Scene("persist", "ship-bank away %d y%d" % (j, y), "open", {0: (59.95, y)}, {},
                             [(2, {0: (70.0, y)}, {}), (2 + j, {0: (59.95, y)}, {})]))
    for y in (150.0, 300.0):
        # two contacts, then tilted to one that keeps one of the two hashes
        out.append(Scene("persist", "ship two->one contact y%d" % y, "open", {0: (59.95, y)}, {}, [(2, {0: (60.05, y, 0.01)}, {})]))
        out.append(Scene("persist", "ship two->one contact (b) y%d" % y, "open", {0: (59.95, y)}, {}, [(2, {0: (59.95 + 0.1, y, -0.01)}, {})]))
    # 5 .. 9 arbiters (goals on the bank and on each other) all separated in one step, and brought back after 2
    for m in (3, 4, 5):
        for y in (150.0, 300.0):
            stack = {g: (touch, y + 9.95 * g) for g in range(m)}
            apart = {g: (200.0 + 20.0 * g, y) for g in range(m)}
            out.append(Scene("persist", "stack %d apart y%d" % (m, y), "open", {}, stack, [(2, {}, apart), (4, {}, stack)]))
            ships = {0: (59.95, y + 60.0), 1: (59.95, y + 80.0)}
            out.append(Scene("persist", "stack %d + ships apart y%d" % (m, y), "open", ships, stack,
                             [(2, {0: (150.0, y + 60.0), 1: (170.0, y + 90.0)}, apart)]))
    return out


def removal_scenes():
    out = []
    # the player's tip is (310, 70): a goal at (310, 74) touches it
    out.append(Scene("removal", "goal+goal", "open", {}, {0: (310.0, 74.0), 1: (310.0, 83.5)}))
    out.append(Scene("removal", "goal+goal (later index)", "open", {}, {3: (310.0, 74.0), 1: (310.0, 83.5)}))
    out.append(Scene("removal", "goal+ship", "open", {0: (314.5, 72.0)}, {0: (310.0, 74.0)}))
    out.append(Scene("removal", "goal+ship+goal", "open", {0: (314.5, 72.0)}, {0: (310.0, 74.0), 2: (305.0, 82.5)}))
    out.append(Scene("removal", "two goals reached", "open", {}, {0: (306.0, 73.0), 4: (314.0, 73.0)}))
    return out


def pile_candidates(rng, n):
    """Random stacks: a random subset of the goals and ships on one spot with jitter (angle 0 for half of them)."""
    out = []
    for i in range(n):
        rec = ("open", "open_pile", "pinch")[i % 3]
        cx, cy = (62.0, 150.0 + 250.0 * rng.rand()) if rec != "pinch" else (300.0 + rng.uniform(-6, 6), 360.0)
        ng = rng.randint(0, 6)
        ns = rng.randint(0, 4)
        gs = rng.permutation(5)[:ng]
        ks = rng.permutation(3)[:ns]
        rot = i % 2 == 1
        j = rng.uniform(2.0, 7.0)
        goals = {int(g): (cx + rng.uniform(-j, j), cy + rng.uniform(-j, j)) for g in gs}
        ships = {int(k): (cx - 6.0 + rng.uniform(-j, j), cy - 12.0 + rng.uniform(-j, j), rng.uniform(-0.6, 0.6) if rot else 0.0) for k in ks}
        out.append(Scene("pile", "pile %s #%d" % (rec, i), rec, ships, goals))
    return out


# ------------------------------------------------------------------------------------------------------------ oracle runs
def oracle_cfg(O):
    return O.default_config(n_traffic=3)


def run_oracle(O, scenes, n_records, K, cfg=None, census=True, n_threads=16):
    """Step the scenes K times in an oracle batch on a bank of n_records, auto-reset on.  Returns per step the outputs, the
    bodies, the goal masks, and (census=True) the arbiter census of every env."""
    n = len(scenes)
    polys, goals = bank_arrays(n_records)
    ob = O.Batch(n, cfg if cfg is not None else oracle_cfg(O), polys, goals, map_ids=np.array([s.rec for s in scenes], dtype=np.int32))
    out = {"obs0": ob.reset(), "obs": [], "rew": [], "done": [], "peek": [], "dyn": [], "census": [], "poked": []}
    act = np.full(n, ACTION, dtype=np.int32)
    alive = np.ones(n, dtype=bool)  # no done yet: pokes apply
    for k in range(K):
        poked = np.zeros(n, dtype=bool)
        for e, s in enumerate(scenes):
            if not alive[e]:
                continue
            for step, ships, gls in s.pokes:
                if step != k:
                    continue
                poke(O, ob, e, ships, gls)
                poked[e] = True
        out["poked"].append(poked)
        o, r, d = ob.step(act, auto_reset=True, n_threads=n_threads)
        out["obs"].append(o); out["rew"].append(r); out["done"].append(d.copy())
        out["peek"].append(ob.peek_all())
        out["dyn"].append([ob.peek_dyn(e) for e in range(n)])
        if census:
            out["census"].append([ob.census(e) for e in range(n)])
        alive &= d == 0
    out["batch"] = ob
    return out


def poke(O, ob, e, ships, gls):
    mask = int(ob.peek_dyn(e)["in_space"])
    for k in range(3):
        ob.poke_traffic(e, k, *ships[k])
    for g in range(5):
        if mask >> g & 1:
            ob.poke_goal(e, g, *gls[g])


def list_lengths(O, scenes, n_records):
    r = run_oracle(O, scenes, n_records, 1)
    return np.array([len(c["list"]) for c in r["census"][0]])


def build_scenes(O, seed=20261016):
    """Every family, interleaved so that each wave mixes list lengths; the pile block sized by the oracle's list length."""
    rng = np.random.RandomState(seed)
    fixed = gap_scenes() + deep_scenes() + tie_scenes() + persist_scenes() + removal_scenes()
    cands = pile_candidates(rng, 2400)
    n_list = list_lengths(O, cands, len(RECORDS))
    piles, per = [], {}
    for s, m in zip(cands, n_list):  # at most 40 scenes per list length (all of the rare long ones)
        if per.get(m, 0) < 40:
            per[m] = per.get(m, 0) + 1
            s.n_list = int(m)
            piles.append(s)
    mixed = [s for s in piles if RECORDS[s.rec][0] == "open"]
    blocks = [s for s in piles if RECORDS[s.rec][0] != "open"]
    # interleave: every run of 8 envs on the open record holds fixed scenes and piles of every length class
    mixed.sort(key=lambda s: s.n_list)
    lo = [s for s in mixed if s.n_list <= 2]
    mid = [s for s in mixed if 3 <= s.n_list <= 8]
    hi = [s for s in mixed if s.n_list > 8]
    out, pools = [], [fixed, lo, mid, hi]
    idx = [0, 0, 0, 0]
    while any(idx[i] < len(p) for i, p in enumerate(pools)):
        for i, p in enumerate(pools):
            take = 2 if i else 3
            out.extend(p[idx[i]: idx[i] + take])
            idx[i] += take
    out.extend(blocks)
    # twins: copies of some scenes that stay parked one step and are poked one step later
    twins = [s for s in out if s.family in ("gap", "pile")][:120:2]
    for s in twins:
        d = Scene("dup", "dup of " + s.tag, RECORDS[s.rec][0], {}, {})
        d.pokes = [(0, _ships({}), _goals({}))] + [(st + 1, sh, go) for st, sh, go in s.pokes]
        d.twin = s
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ oracle census -> HIP rows
def pair_id(i, j):
    """The HIP arbiter row (include/shipsim.h SSG_F_DYN_LIVE) of oracle slot pair i < j (0, 1 banks, 2..6 goals, 8..10 ships)."""
    if i < 2:
        return 9 + 2 * (j - 2) + i if j < 7 else 2 * (j - 8) + i
    if i < 7:
        h = i - 2
        return 39 + (j - 2) * (j - 3) // 2 + h if j < 7 else 21 + 3 * h + (j - 8)
    return 6 + (i - 8) + (j - 8) - 1


def census_rows(census):
    """One step's census of n envs as the HIP columns hold them: live [n] u64, meta [n][54] (state | age << 3 | count << 5),
    hash [n][9], impulses [n][54][4] (jn0, jn1, jt0, jt1; contact 1 zero when one contact)."""
    n = len(census)
    live = np.zeros(n, dtype=np.uint64)
    meta = np.zeros((n, 54), dtype=np.uint32)
    hh = np.zeros((n, 9), dtype=np.uint32)
    acc = np.zeros((n, 54, 4))
    for e, c in enumerate(census):
        for (i, j), a in c["arbs"].items():
            p = pair_id(i, j)
            live[e] |= np.uint64(1) << np.uint64(p)
            meta[e, p] = a["state"] | a["age"] << 3 | a["count"] << 5
            two = a["count"] > 1
            if p < 9:
                hh[e, p] = a["hash"][0] | ((a["hash"][1] if two else 0) << 16)
            acc[e, p] = (a["jn"][0], a["jn"][1] if two else 0.0, a["jt"][0], a["jt"][1] if two else 0.0)
    return live, meta, hh, acc


def goal_pair_mask(gmask):
    """[n] u64: the pair ids that involve a goal NOT in gmask (their arbiters leave with the goal at the next full step)."""
    out = np.zeros(len(gmask), dtype=np.uint64)
    for e, m in enumerate(gmask):
        v = 0
        for g in range(5):
            if m >> g & 1:
                continue
            for i in range(11):
                if i != 2 + g and i != 7:
                    v |= 1 << pair_id(min(i, 2 + g), max(i, 2 + g))
        out[e] = v
    return out
