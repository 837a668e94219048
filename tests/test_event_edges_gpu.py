"""The step kernel's events (collide_ship, collide_goal, determine_reward, is_done) at their decision boundaries, against the
oracle and the exact classifier.

One handle holds every scene of tests/event_scenes.py, one per env: the families interleaved inside every wave, then the waves
that goal_queue and serve own, then a last, partly filled wave.  The scene is written into the F_X, F_Y, F_ANGLE, F_VX, F_VY,
F_W, F_GOAL_MASK and F_STEP_COUNT columns (config 4: also the parked traffic and the goal_dist scenes' goal bodies through
F_TRAFFIC / F_GOAL_BODIES, then wake_dynamics()) and into the oracle worlds; then every env takes K = 4 steps of action 1, in three modes: (a) four step_tensor
calls, (b) rollout_tensor in overwrite mode, (c) rollout_tensor with trajectory=True; (b) and (c) with and without auto-reset.

Per row of every step: reward, done and all five SSG_EV_* bits are bit for bit the precedence table's on the oracle's own
predicates (CLEAR and BAND scenes alike); on CLEAR predicates the flags equal the classifier's verdict directly; the pose, rudder
and nearest-goal columns of the newest frame are within 1e-9 of the oracle's, the older frames too in mode (c) from step 1 on;
F_GOAL_MASK, F_STEP_COUNT, F_CUM_REWARD and F_MAP_ID (the next episode's record) after the launch are the oracle's.  The six
layouts (SSG_BLOCK 64 / 128 / 256 x bank staged / gathered) and the three modes give identical bits.
"""
import os

import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import event_scenes as ES
from step_rows import EVENT_ROWS

pytestmark = pytest.mark.gpu

# n_beams x history x fix_collision_reward x n_goals x n_ships (tests/step_rows.py), thinned: one beam count from each compiled beam
# group and both BASELINE counts, history 1 .. 3, both reward rules, n_goals 1, 5 and 6; the rows with n_ships = 4 are config 4 (the
# DYN instantiation) at 6, 10, 12 and 16 beams
ROWS = EVENT_ROWS
LAYOUTS = (("64", False), ("128", False), ("256", False), ("64", True), ("128", True), ("256", True))
K = ES.K
_cache = {}


def _scenes(O, n_goals):
    if n_goals not in _cache:
        _cache[n_goals] = ES.build_scenes(O, n_goals)
    return _cache[n_goals]


def _reference(O, row, auto_reset):
    """the oracle run of a row, its classification and the table's outputs, as arrays [K, n]"""
    nb, hist, fix, ng, n_ships = row
    recs, hulls, scenes, _ = _scenes(O, ng)
    ref = ES.run_oracle(O, recs, scenes, nb, hist, ng, auto_reset, dyn=n_ships > 1)
    cls = ES.classify_run(O, hulls, scenes, ref)
    ref["rew_t"], ref["done_t"], ref["ev_t"], ref["cum_t"] = ES.expected(ref, fix, auto_reset)
    if not fix:
        assert np.array_equal(ref["rew_t"], ref["rew"])
    assert np.array_equal(ref["done_t"], ref["done"])
    for name, get in (("col", lambda v: v.colliding), ("goal", lambda v: v.reached)):
        ref[name] = np.array([[get(v)[0] for v in step] for step in cls])
        ref[name + "_clear"] = np.array([[get(v)[1] for v in step] for step in cls])
    ref["listed"] = np.array([[v.listed[0] for v in step] for step in cls])
    ref["listed_clear"] = np.array([[v.listed[1] for v in step] for step in cls])
    ref["count"] = ES.count_targets(scenes, cls, ref)
    return ref


class Handle:
    def __init__(self, torch, N, row, scenes, recs, blk, in_global, auto_reset):
        from ship_sim_gym_amd import config as cfgmod, worldgen
        from ship_sim_gym_amd.vec_env import ShipVecEnv
        nb, hist, fix, ng, n_ships = row
        self.torch, self.N, self.scenes, self.ng, self.dyn = torch, N, scenes, ng, n_ships > 1

        class EC(cfgmod.EnvConfig):
            HISTORY_SIZE = hist
            MAX_STEPS = ES.MAX_STEPS

        polys, goals = ES.bank_arrays(recs)
        keep = cfgmod.N_GOALS
        cfgmod.N_GOALS = ng
        os.environ["SSG_BLOCK"] = blk
        try:
            bank = np.stack([worldgen.build_record(p[0], p[1], g, (ES.W / 2, 25.0)) for p, g in zip(polys, goals)])
            self.vec = ShipVecEnv(len(scenes), env_config=EC, n_beams=nb, bank=bank, bank_in_global=in_global, auto_reset=auto_reset,
                                  fix_collision_reward=fix, n_ships=n_ships)
        finally:
            del os.environ["SSG_BLOCK"]
            cfgmod.N_GOALS = keep
        assert self.vec.cfg.n_goals == ng
        self.geo = self.vec.launch_geometry()
        dev = self.vec.device
        n = len(scenes)
        self.ids = torch.tensor([s.rec for s in scenes], dtype=torch.int32, device=dev)
        self.state = torch.tensor([(ES.dyn_pose(s) if self.dyn else s.pose) + s.vel for s in scenes], dtype=torch.float64, device=dev)
        self.bodies = [(e, g, x, y) for e, s in enumerate(scenes) for g, x, y in ES.dyn_goal_bodies(s, ng)] if self.dyn else []
        self.mask = torch.tensor([s.mask for s in scenes], dtype=torch.uint8, device=dev)
        self.steps0 = torch.tensor([s.steps0 for s in scenes], dtype=torch.int32, device=dev)
        self.act = torch.full((K, n), ES.ACTION, dtype=torch.int32, device=dev)

    def start(self):
        """reset onto the scenes' records and write the scenes; returns the reset observation"""
        torch, N, vec = self.torch, self.N, self.vec
        obs0 = vec.reset_tensor(map_ids=self.ids).cpu().numpy().copy()
        for col, f in enumerate((N.F_X, N.F_Y, N.F_ANGLE, N.F_VX, N.F_VY, N.F_W)):
            vec.field(f)[:] = self.state[:, col]
        vec.field(N.F_STEP_COUNT)[:] = self.steps0
        gm = vec.field(N.F_GOAL_MASK)
        gm[:] = (gm & 0xC0) | self.mask
        if self.dyn:  # config 4: the traffic parked; the shifted scenes' listed goals written as bodies
            T, G = vec.field(N.F_TRAFFIC), vec.field(N.F_GOAL_BODIES)
            for k in range(3):
                T[9 * k: 9 * k + 9] = 0.0
                T[9 * k + 0] = ES.PARK_SHIPS[k][0]
                T[9 * k + 1] = ES.PARK_SHIPS[k][1]
            g = G.cpu().numpy().copy()
            for e, j, x, y in self.bodies:
                g[8 * j: 8 * j + 8, e] = (x, y, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
            G.copy_(torch.from_numpy(g).to(vec.device))
            vec.wake_dynamics()
        return obs0

    def fields(self):
        N, vec = self.N, self.vec
        return {"mask": (vec.field(N.F_GOAL_MASK) & 0x3F).cpu().numpy().copy(), "steps": vec.field(N.F_STEP_COUNT).cpu().numpy().copy(),
                "cum": vec.field(N.F_CUM_REWARD).cpu().numpy().copy(), "map": vec.field(N.F_MAP_ID).cpu().numpy().copy()}

    def run(self, mode):
        """{'obs' [K or 1, n, D], 'rew', 'done', 'flags', 'fields'}: mode a / c every step, mode b the last step"""
        vec = self.vec
        out = {"obs0": self.start()}
        if mode == "a":
            steps = []
            for k in range(K):
                steps.append([x.cpu().numpy().copy() for x in vec.step_tensor(self.act[k])])
            res = [np.stack([s[i] for s in steps]) for i in range(4)]
        elif mode == "b":
            res = [x.cpu().numpy().copy()[None] for x in vec.rollout_tensor(self.act)]
        else:
            res = [x.cpu().numpy().copy() for x in vec.rollout_tensor(self.act, trajectory=True)]
        out["obs"], out["rew"], out["done"], out["flags"] = res
        out["fields"] = self.fields()
        return out


def _check(N, row, scenes, ref, g, mode, where, auto_reset):
    """one run against the oracle, the table and the classifier"""
    nb, hist, fix, ng, n_ships = row
    F = 6 + nb
    ks = list(range(K)) if mode != "b" else [K - 1]

    def tags(bad):
        return [(ks[i], scenes[e].family, scenes[e].tag) for i, e in zip(*np.nonzero(bad))][:8]

    np.testing.assert_array_equal(g["obs0"], ref["obs0"], err_msg=where)
    for name, want in (("rew", ref["rew_t"]), ("done", ref["done_t"]), ("flags", ref["ev_t"])):
        bad = g[name] != want[ks]
        assert not bad.any(), (where, name, int(bad.sum()), tags(bad), g[name][bad][:8], want[ks][bad][:8])
    # on clear predicates: the classifier's verdict directly
    for bit, name in ((N.EV_COLLIDING, "col"), (N.EV_GOAL_REACHED, "goal")):
        bad = (((g["flags"] & bit) != 0) != ref[name][ks]) & ref[name + "_clear"][ks]
        assert not bad.any(), (where, name, "against the classifier", tags(bad))
    # the state after the launch
    after = ref["after"][-1]
    for name, want in (("mask", after[:, 13]), ("steps", after[:, 7]), ("cum", ref["cum_t"]), ("map", after[:, 11])):
        bad = g["fields"][name] != want
        assert not bad.any(), (where, "F_" + name, [(scenes[e].tag, g["fields"][name][e], want[e]) for e in np.nonzero(bad)[0][:8]])
    if not auto_reset:
        ok = ref["listed_clear"].all(axis=0)
        lst = ref["listed"][-1]
        assert np.array_equal(g["fields"]["mask"][ok], lst[ok]), (where, "listed goals against the classifier")
    # the newest frame's pose, rudder and nearest-goal columns; in mode (c) the older frames too, from step 1 on
    for i, k in enumerate(ks):
        for fr in range(hist):
            if fr < hist - 1 and (mode != "c" or k == 0):
                continue
            err = np.abs(g["obs"][i][:, fr * F: fr * F + 6] - ref["obs"][k][:, fr * F: fr * F + 6]).max(axis=1)
            bad = ~(err <= 1e-9)
            assert not bad.any(), (where, "obs frame %d step %d" % (fr, k), [(scenes[e].tag, err[e]) for e in np.nonzero(bad)[0][:8]])


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "beams%d-hist%d-fix%d-goals%d-ships%d" % r)
def test_events_at_their_decision_boundaries(torch_cuda, oracle, native, row):
    torch, O, N = torch_cuda, oracle, native
    nb, hist, fix, ng, n_ships = row
    recs, _, scenes, _ = _scenes(O, ng)
    n = len(scenes)
    assert 2048 <= n <= 4096 and n % 64
    refs = {False: _reference(O, row, False), True: _reference(O, row, True)}
    count = refs[False]["count"]
    print("%r: (clear, band) target predicates per family: %s" % (row, " ".join("%s %d/%d" % (f, count[(f, True)], count[(f, False)])
                                                                                 for f in ES.FAMILIES)), flush=True)
    for auto in (False, True):
        ES.check_conditions(refs[auto]["count"])
        # all five done reasons occur in the row (config 4 too), and with five goals or more all 32 combinations of them
        ev0 = refs[auto]["ev_t"][0]
        assert all((ev0 & bit).any() for bit in (1, 2, 4, 8, 16)), row
        combos = {int(ev0[e]) for e, s in enumerate(scenes) if s.family == "precedence" and s.meta.get("kind") == "combo"}
        assert ng < 5 or combos == set(range(32)), (row, sorted(combos))
    first = {}
    for blk, in_global in LAYOUTS:
        runs = {}
        for auto in (False, True):
            h = Handle(torch, N, row, scenes, recs, blk, in_global, auto)
            epw, staged, _ = h.geo
            where = "%r SSG_BLOCK=%s epw=%d global=%d staged=%d auto_reset=%d" % (row, blk, epw, in_global, staged, auto)
            # (no 256-env workgroups above 12 beams; config 4's step kernel is built for 64 and 256)
            assert epw == int(blk) or (nb > 12 and epw < int(blk)) or (n_ships > 1 and blk == "128" and epw == 64), where
            assert staged == (not in_global), where  # the records are few enough to stage at every size
            for mode in (("a", "b", "c") if not auto else ("b", "c")):
                g = h.run(mode)
                _check(N, row, scenes, refs[auto], g, mode, where + " mode " + mode, auto)
                runs[(auto, mode)] = g
            h.vec.close()
        # the three modes: identical bits for reward, done, flags and observation rows
        for auto in (False, True):
            c = runs[(auto, "c")]
            for key in ("obs", "rew", "done", "flags"):
                assert np.array_equal(runs[(auto, "b")][key][0], c[key][K - 1]), (row, blk, in_global, auto, "b != c", key)
                if not auto:
                    assert np.array_equal(runs[(auto, "a")][key], c[key]), (row, blk, in_global, "a != c", key)
            for key in ("mask", "steps", "cum", "map"):
                assert np.array_equal(runs[(auto, "b")]["fields"][key], c["fields"][key]), (row, blk, in_global, auto, key)
        # the six layouts: identical bits
        for am, g in runs.items():
            if am not in first:
                first[am] = g
                continue
            for key in ("obs", "rew", "done", "flags"):
                assert np.array_equal(first[am][key], g[key]), (row, blk, in_global, am, key)
        print("%r SSG_BLOCK=%s global=%d ok" % (row, blk, in_global), flush=True)
