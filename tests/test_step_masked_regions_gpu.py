"""The step kernel where a wave's lanes part ways: execution-masked reset regions and rebased output addresses.

The kernel moves a reset env's registers under the execution mask (a wave without a reset env skips the region), stores its
observation rows through a wave-uniform base plus per-lane byte offsets, and predicates the lidar pair queue's stores.  What can
go wrong there depends on WHICH lanes of a wave take a branch in a step, and on the row / tile / workgroup an offset belongs to —
not on the batch size.  So the scenes are two small batches built from tests/event_scenes.py's records and scene type:

  S256  256 envs = the four tiles of one 256-env workgroup.   S300  300 envs = four tiles and a ragged fifth wave of 44 lanes.

Every (wave, step) of a K = 4 launch is given a set of lanes that are reset in that step (the step limit: steps0 = MAX_STEPS - 1 - k),
and one of lanes that reach a goal (a ship at rest on the goal cluster; or a ship reset a step earlier onto a record with a goal at
the spawn point, which it reaches in the next step — that is how a goal is reached in the LAST step of a fused launch, where the
observer's speculative rows have to be patched):  none, lane 0 only, lane 63 only, two lanes, 63 lanes, all 64 — at the first, a
middle and the last step.  The other ships spin next to the right bank with neighbouring lanes half a turn apart, so that a beam's
hit / miss alternates from lane to lane and from step to step (both arms of the sticky merge), and the actions mix thrust, rudder
left and rudder right inside every wave in every step.  The designed patterns are asserted on the oracle's run before anything is
compared with it.

Layouts SSG_BLOCK 64 / 128 / 256, bank staged and bank_in_global (above 12 beams there are no 256-env workgroups: the layout runs
at the size the library folds it to); every beam count 1 .. 16 at history 1 and 2, history 3 at 1, 4, 7, 12 and 16 beams
(tests/step_rows.py: the beam count selects how a row is written — the column tile or the pair writer, their remainders, the
split and speculative rows); auto-reset on and off.  Per layout: a fused K = 4 trajectory launch, and four single-step (K = 1)
launches of a second handle.  Reward, done and flags are the oracle's (the precedence table on its predicates) bit for bit,
observation rows within the suite's 1e-9, and every fused slot is bitwise equal to the single-step launch — the pattern of
test_every_workgroup_layout_against_the_oracle.
"""
import math
import os

import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import event_scenes as ES
from lidar_scenes import layouts
from step_rows import LANE_ROWS

pytestmark = pytest.mark.gpu

K = 4
NG = 5
LAYOUTS = (("64", False), ("128", False), ("256", False), ("64", True), ("128", True), ("256", True))
SPIN_W = 2.0 * math.pi / 1.4   # with damping 0.4 the angle is back after two steps: a beam's hit / miss alternates step by step
SPIN_AT = (340.0, 300.0)       # 65 in front of the right bank of banks3_12 (lidar range 100), out of reach of the left one
SPAWN_GOALS = [[310.0, 45.0], [250.0, 40.0]]  # inside the hull of a ship at the spawn point (300, 25); the next nearest
ALL, NONE = frozenset(range(64)), frozenset()


def _records():
    """0 banks (next: 1) | 1 goal at the spawn point | 2 banks (next: 3) | 3 banks | 4 cluster (next: 5) | 5 banks"""
    _, bl, br = layouts()[0]
    far = ES.FAR_GOALS[:NG]
    spawn_goal = SPAWN_GOALS + far[2:]
    cluster = [list(c) for c in ES.CLUSTER[:NG]]
    return [("banks", bl, br, far), ("spawn_goal", bl, br, spawn_goal), ("banks2", bl, br, far), ("banks3", bl, br, far),
            ("cluster", bl, br, cluster), ("banks5", bl, br, far)]


def _spinner(e, rec, steps0=0):
    lane = e % 64
    a0 = -math.pi / 2 if lane % 2 == 0 else math.pi / 2  # even lanes face the bank first, odd lanes face away
    return ES.Scene("approach", "spinner", rec, (SPIN_AT[0], SPIN_AT[1] + (lane % 5), a0), None, vel=(0.0, 0.0, SPIN_W), mask=31, steps0=steps0)


def _on_cluster(e):
    """at rest on the goal cluster: goals 0 and 1 are reached at once; even lanes list {0, 2} (the nearest goal moves from 0 to 2),
    odd lanes all five"""
    return ES.Scene("goal_queue", "on the cluster", 4, ES.P0, None, mask=(1 | 4) if e % 2 == 0 else 31)


def _build(plan, n):
    """plan[wave] = {"reset": {step: lanes}, "goal0": lanes at rest on the cluster, "via_spawn": reset steps whose lanes sit on
    record 0 (-> the record with a goal at the spawn point)}.  Returns (scenes, want_reset [K][n], want_goal [K][n])."""
    scenes, want_reset, want_goal = [], np.zeros((K, n), dtype=bool), np.zeros((K, n), dtype=bool)
    for e in range(n):
        w, lane = divmod(e, 64)
        p = plan[w]
        if lane in p.get("goal0", NONE):
            scenes.append(_on_cluster(e))
            want_goal[0, e] = True
            continue
        step = next((k for k, lanes in p.get("reset", {}).items() if lane in lanes), None)
        via = step is not None and step in p.get("via_spawn", ())
        scenes.append(_spinner(e, 0 if via else 2, 0 if step is None else ES.MAX_STEPS - 1 - step))
        if step is not None:
            want_reset[step, e] = True
            if via and step + 1 < K:
                want_goal[step + 1, e] = True
    return scenes, want_reset, want_goal


PLAN_256 = {0: {"reset": {0: {0}, 1: {63}, 2: {30, 31}}},
            1: {"reset": {0: ALL}},
            2: {"reset": {1: {17}, 3: ALL - {17}}},
            3: {"reset": {2: ALL - {0}, 3: {0}}}}
PLAN_300 = {0: {"reset": {1: ALL}, "via_spawn": (1,)},                                    # all 64 reach a goal in step 2
            1: {"goal0": {0}, "reset": {0: {8, 9}, 3: {63}}},
            2: {"goal0": ALL - {63}},
            3: {"goal0": {63}, "reset": {2: {20, 41}}, "via_spawn": (2,)},                 # two lanes reach a goal in the LAST step
            4: {"goal0": set(range(44))}}                                                  # the ragged wave: every lane
SETS = {256: PLAN_256, 300: PLAN_300}


def _actions(scenes):
    """[K][n]: the spinners thrust / turn the rudder left / right, all three inside a wave in every step; a ship on the cluster
    only turns its rudder (it stays at rest where its goals were placed)"""
    e = np.arange(len(scenes))
    on_cluster = np.array([s.rec == 4 for s in scenes])
    return np.stack([np.where(on_cluster, 1 + (e + k) % 2, (e + 2 * k + e // 7) % 3).astype(np.int32) for k in range(K)])


def _run_oracle(O, recs, scenes, nb, hist, auto_reset, acts):
    """event_scenes.run_oracle with per-env actions (its keys)"""
    polys, goals = ES.bank_arrays(recs)
    n = len(scenes)
    ob = O.Batch(n, ES.oracle_config(O, nb, hist, NG), polys, goals, map_ids=np.array([s.rec for s in scenes], dtype=np.int32))
    out = {"obs0": ob.reset(), "obs": [], "rew": [], "done": [], "peek": []}
    for e, s in enumerate(scenes):
        ob.poke_state(e, *(s.pose + s.vel))
        ob.poke_episode(e, s.mask, s.steps0)
    for k in range(K):
        o, r, d = ob.step(acts[k], auto_reset=False, n_threads=8)
        out["peek"].append(ob.peek_all())
        if auto_reset:
            o = ob.auto_reset_done()
        out["obs"].append(o); out["rew"].append(r); out["done"].append(d.copy())
    for key in ("obs", "rew", "done", "peek"):
        out[key] = np.stack(out[key])
    out["rew_t"], out["done_t"], out["ev_t"], _ = ES.expected(out, False, auto_reset)
    assert np.array_equal(out["rew_t"], out["rew"]) and np.array_equal(out["done_t"], out["done"])
    return out


def _check_design(n, scenes, want_reset, want_goal, ref, acts, nb):
    """the oracle's run shows the designed lane patterns"""
    done, goal = ref["done"] != 0, (ref["ev_t"] & ES.EV_GOAL_REACHED) != 0
    assert np.array_equal(goal, want_goal), [(k, e) for k, e in zip(*np.nonzero(goal != want_goal))][:8]
    # (an env on the cluster is done when it lists no further goal; every other done is the designed step limit)
    on_cluster = np.array([s.rec == 4 for s in scenes])
    assert np.array_equal(done[:, ~on_cluster], want_reset[:, ~on_cluster]), "reset lanes"
    assert not (ref["ev_t"][:, ~on_cluster] & (ES.EV_COLLIDING | ES.EV_OUT_OF_BOUNDS)).any()
    waves_of_spinners = 0
    for w in range((n + 63) // 64):
        a = acts[:, 64 * w: 64 * w + 64][:, ~on_cluster[64 * w: 64 * w + 64]]
        if a.shape[1] >= 32:
            waves_of_spinners += 1
            assert all({0, 1, 2} <= set(a[k].tolist()) for k in range(K)), "thrust on in some lanes of a wave and off in others"
    assert waves_of_spinners >= 3
    # sticky merge: a spinner's reading changes in a step (a hit) or stays (a miss).  Both in successive steps of one lane, and
    # in neighbouring lanes in the same step
    F = 6 + nb
    rd = np.concatenate([ref["obs0"][None, :, -nb:], ref["obs"][:, :, -nb:]])  # [K + 1][n][nb] newest frame's readings
    hit = rd[1:] != rd[:-1]
    spin = np.array([s.tag == "spinner" for s in scenes]) & ~want_reset.any(axis=0)
    flips = (hit[1:] != hit[:-1]) & spin[None, :, None]
    nb_pairs = [e for e in range(0, n - 1) if spin[e] and spin[e + 1] and e // 64 == (e + 1) // 64]
    across = sum(int((hit[:, e] != hit[:, e + 1]).any()) for e in nb_pairs)
    assert flips.sum() >= 20 and across >= 8, (int(flips.sum()), across, F)


class Handle:
    def __init__(self, torch, N, nb, hist, scenes, recs, blk, in_global, auto_reset):
        from ship_sim_gym_amd import config as cfgmod, worldgen
        from ship_sim_gym_amd.vec_env import ShipVecEnv

        class EC(cfgmod.EnvConfig):
            HISTORY_SIZE = hist
            MAX_STEPS = ES.MAX_STEPS

        assert cfgmod.N_GOALS == NG
        polys, goals = ES.bank_arrays(recs)
        os.environ["SSG_BLOCK"] = blk
        try:
            bank = np.stack([worldgen.build_record(p[0], p[1], g, (ES.W / 2, 25.0)) for p, g in zip(polys, goals)])
            self.vec = ShipVecEnv(len(scenes), env_config=EC, n_beams=nb, bank=bank, bank_in_global=in_global, auto_reset=auto_reset)
        finally:
            del os.environ["SSG_BLOCK"]
        self.torch, self.N = torch, N
        dev = self.vec.device
        self.ids = torch.tensor([s.rec for s in scenes], dtype=torch.int32, device=dev)
        self.state = torch.tensor([s.pose + s.vel for s in scenes], dtype=torch.float64, device=dev)
        self.mask = torch.tensor([s.mask for s in scenes], dtype=torch.uint8, device=dev)
        self.steps0 = torch.tensor([s.steps0 for s in scenes], dtype=torch.int32, device=dev)

    def start(self):
        N, vec = self.N, self.vec
        obs0 = vec.reset_tensor(map_ids=self.ids).cpu().numpy().copy()
        for col, f in enumerate((N.F_X, N.F_Y, N.F_ANGLE, N.F_VX, N.F_VY, N.F_W)):
            vec.field(f)[:] = self.state[:, col]
        vec.field(N.F_STEP_COUNT)[:] = self.steps0
        gm = vec.field(N.F_GOAL_MASK)
        gm[:] = (gm & 0xC0) | self.mask
        return obs0

    def fused(self, acts):
        return [x.cpu().numpy().copy() for x in self.vec.rollout_tensor(acts, trajectory=True)]

    def single(self, acts):
        steps = [[x.cpu().numpy().copy() for x in self.vec.step_tensor(acts[k])] for k in range(K)]
        return [np.stack([s[i] for s in steps]) for i in range(4)]


@pytest.mark.parametrize("nb,hist", LANE_ROWS, ids=lambda v: str(v))
def test_lane_patterns_of_resets_goals_hits_and_thrust(torch_cuda, oracle, native, nb, hist):
    torch, O, N = torch_cuda, oracle, native
    recs = _records()
    for n, plan in SETS.items():
        scenes, want_reset, want_goal = _build(plan, n)
        acts = _actions(scenes)
        refs = {auto: _run_oracle(O, recs, scenes, nb, hist, auto, acts) for auto in (True, False)}
        _check_design(n, scenes, want_reset, want_goal, refs[True], acts, nb)
        first = {}
        for blk, in_global in LAYOUTS:
            for auto in (True, False):
                ref = refs[auto]
                where = "n=%d beams=%d history=%d SSG_BLOCK=%s global=%d auto_reset=%d" % (n, nb, hist, blk, in_global, auto)
                a = Handle(torch, N, nb, hist, scenes, recs, blk, in_global, auto)
                b = Handle(torch, N, nb, hist, scenes, recs, blk, in_global, auto)
                epw = a.vec.launch_geometry()[0]
                assert epw == int(blk) or (nb > 12 and epw < int(blk)), where  # (no 256-env workgroups above 12 beams)
                dacts = torch.tensor(acts, dtype=torch.int32, device=a.vec.device)
                np.testing.assert_array_equal(a.start(), ref["obs0"], err_msg=where)
                b.start()
                fo, fr, fd, ff = a.fused(dacts)
                so, sr, sd, sf = b.single(dacts)
                a.vec.close(); b.vec.close()
                for name, got, want in (("reward", fr, ref["rew_t"]), ("done", fd, ref["done_t"]), ("flags", ff, ref["ev_t"])):
                    bad = got != want
                    assert not bad.any(), (where, name, [(k, e, scenes[e].tag) for k, e in zip(*np.nonzero(bad))][:8])
                err = np.abs(fo - ref["obs"])
                # (the frames that predate the scene write, hist - 1 - k of them at step k: the kernel rebuilds the newest of them
                # from the state columns the scene was written into, the oracle holds the reset's frame — the scene's own doing;
                # every frame of a step taken after the write is compared)
                for k in range(min(K, hist - 1)):
                    err[k, :, :(6 + nb) * (hist - 1 - k)] = 0.0
                assert (err <= 1e-9).all(), (where, "obs", float(err.max()), [(k, e, j) for k, e, j in zip(*np.nonzero(~(err <= 1e-9)))][:8])
                # every fused slot: bitwise the single-step (K = 1) launch
                for name, f, s in (("obs", fo, so), ("reward", fr, sr), ("done", fd, sd), ("flags", ff, sf)):
                    assert np.array_equal(f, s), (where, "fused != single steps", name, [tuple(i) for i in np.argwhere(f != s)[:8]])
                # the six layouts: identical bits
                if auto not in first:
                    first[auto] = fo
                assert np.array_equal(first[auto], fo), (where, "layouts differ")
