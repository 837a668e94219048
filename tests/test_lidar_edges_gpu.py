"""The step kernel's lidar (lidar_query / lidar_pass) at its decision boundaries, against the oracle and the exact classifier.

One handle holds every scene of tests/lidar_scenes.py, one per env, families interleaved inside every wave: beams through hull
vertices, parallel to edges, ending on edges, origins on planes (the need_exact pass) and inside hulls or on bank corners, two
hulls on one beam, hulls of 3..12 planes, beam ends at a hull's x extent (the cull) and sticky readings.  The pose is written
into the F_X / F_Y / F_ANGLE columns (velocities zero) and into the oracle worlds, then every env steps twice.

Per beam: a CLEAR beam (every deciding predicate of cpPolyShapeSegmentQuery holds by >= 1e-12 x the coordinate scale) reads
what the oracle reads within 1e-9; a BAND beam reads one of the classifier's candidates, never anything else, never -0.0.
Reward, done and the event flags are bit-exact with the oracle; staged and gathered bank and the three workgroup sizes give
identical bits; the default and the EXACT path agree on every clear beam.

Two tests share the run and the comparison (_gpu_run, _check_row): the first holds the rows with the EXACT path beside the
default one, the second one case per remaining beam count, so that every step_kernel instantiation 1 .. 16 reads these scenes
(tests/step_rows.py).
"""
import collections
import os

import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import lidar_scenes as LS
from step_rows import LIDAR_MORE_ROWS, LIDAR_ROWS

pytestmark = pytest.mark.gpu

# tests/step_rows.py.  ROWS: n_beams x history x exact_lidar, thinned: both histories on both paths, and the EXACT path
# (SSG_FLAG_EXACT_LIDAR is built for 8 and 10 beams) beside the default one at its beam counts.  MORE_ROWS: n_beams x history, the
# other beam counts on the default path, one test case each.  Every row runs on all six bank / workgroup layouts.
ROWS, MORE_ROWS = LIDAR_ROWS, LIDAR_MORE_ROWS
LAYOUTS = (("64", False), ("128", False), ("256", False), ("64", True), ("128", True), ("256", True))


def _gpu_run(torch, native, lay, scenes, nb, hist, exact, blk, in_global):
    from ship_sim_gym_amd import config as cfgmod, worldgen
    from ship_sim_gym_amd.vec_env import ShipVecEnv

    class EC(cfgmod.EnvConfig):
        HISTORY_SIZE = hist

    polys, goals = LS.bank_arrays(lay)
    bank = np.stack([worldgen.build_record(p[0], p[1], g, (LS.W / 2, 25.0)) for p, g in zip(polys, goals)])
    os.environ["SSG_BLOCK"] = blk
    try:
        vec = ShipVecEnv(len(scenes), env_config=EC, n_beams=nb, bank=bank, bank_in_global=in_global, exact_lidar=exact,
                         auto_reset=False)
    finally:
        del os.environ["SSG_BLOCK"]
    geo = vec.launch_geometry()
    assert geo[0] == int(blk) or (nb > 12 and geo[0] < int(blk)), (blk, geo)  # (no 256-env workgroups above 12 beams)
    assert not (in_global and geo[1])
    dev = vec.device
    ids = torch.tensor([s.rec for s in scenes], dtype=torch.int32, device=dev)
    out = {"obs0": vec.reset_tensor(map_ids=ids).cpu().numpy().copy(), "staged": geo[1], "epw": geo[0]}
    act = torch.full((len(scenes),), LS.ACTION, dtype=torch.int32, device=dev)
    rew, done, flags = [], [], []
    for k, attr in ((1, "pose1"), (2, "pose2")):
        pose = torch.tensor([getattr(s, attr) for s in scenes], dtype=torch.float64, device=dev)
        vec.field(native.F_X)[:] = pose[:, 0]
        vec.field(native.F_Y)[:] = pose[:, 1]
        vec.field(native.F_ANGLE)[:] = pose[:, 2]
        for f in (native.F_VX, native.F_VY, native.F_W):
            vec.field(f)[:] = 0.0
        o, r, d, fl = vec.step_tensor(act)
        out["obs%d" % k] = o.cpu().numpy().copy()
        rew.append(r.cpu().numpy().copy()); done.append(d.cpu().numpy().copy()); flags.append(fl.cpu().numpy().copy())
    vec.close()
    out["rew"], out["done"], out["flags"] = np.stack(rew), np.stack(done), np.stack(flags)
    return out


def _check_row(torch, oracle, native, nb, hist, exact, report):
    """one (n_beams, history, exact_lidar) row on all six layouts against the oracle and the classifier; returns the first
    layout's step-1 observation and the step-1 clear mask"""
    lay, hulls, scenes = LS.build_scenes(oracle, nb)
    n = len(scenes)
    assert 2048 <= n <= 4096
    cls = LS.classify_scenes(oracle, lay, hulls, scenes, nb)
    ref = LS.run_oracle(oracle, lay, scenes, nb, hist)
    rl = [LS.lidar_cols(ref["obs1"], nb, hist), LS.lidar_cols(ref["obs2"], nb, hist)]
    clear_mask = np.array([[[c for c, _ in cls[e][k]] for e in range(n)] for k in (0, 1)])
    first = None
    for blk, in_global in LAYOUTS:
        g = _gpu_run(torch, native, lay, scenes, nb, hist, exact, blk, in_global)
        where = "n_beams=%d history=%d exact=%d SSG_BLOCK=%s epw=%d global=%d staged=%d" % (nb, hist, exact, blk, g["epw"], in_global,
                                                                                         g["staged"])
        np.testing.assert_array_equal(g["obs0"], ref["obs0"], err_msg=where)
        np.testing.assert_array_equal(g["rew"], ref["rew"], err_msg="reward: " + where)
        np.testing.assert_array_equal(g["done"], ref["done"], err_msg="done: " + where)
        np.testing.assert_array_equal((g["flags"] & native.EV_COLLIDING) != 0, ref["flags"][..., 0] != 0, err_msg=where)
        np.testing.assert_array_equal((g["flags"] & native.EV_GOAL_REACHED) != 0, ref["flags"][..., 1] != 0, err_msg=where)
        count, bad = collections.Counter(), []
        for k in (0, 1):
            gl = LS.lidar_cols(g["obs%d" % (k + 1)], nb, hist)
            gp = np.full((n, nb), -1.0) if k == 0 else LS.lidar_cols(g["obs1"], nb, hist)
            # the rest of the new frame: as the oracle's (the kernel rebuilds the previous frame's pose from the state
            # columns the test has just written, the oracle keeps the frame it emitted: not compared)
            F, hh = 6 + nb, hist - 1
            np.testing.assert_allclose(g["obs%d" % (k + 1)][:, hh * F:hh * F + 6], ref["obs%d" % (k + 1)][:, hh * F:hh * F + 6],
                                       rtol=0, atol=1e-9, err_msg=where)
            for e, s in enumerate(scenes):
                for i, (clear, cands) in enumerate(cls[e][k]):
                    r = gl[e, i]
                    # (a clear miss keeps the reading of step 1.  Where that beam was a BAND beam in step 1 and the kernel took
                    # another of its candidates than the oracle did — both checked there — the oracle's step-2 reading is the
                    # oracle's own step-1 choice, not this beam's reading: the kernel's own, bit for bit, is all there is to ask.
                    # It happens where a beam of the sticky scenes' hit pose ends on the hull at the very end of its range: at
                    # 3, 6, 9, 12 and 15 beams)
                    kept_band = k == 1 and cands == [None] and not cls[e][0][i][0] and not abs(gp[e, i] - rl[0][e, i]) <= 1e-9
                    if clear and not kept_band:
                        ok = abs(r - rl[k][e, i]) <= 1e-9 and LS.accepts(cands, r, gp[e, i])
                    else:
                        ok = LS.accepts(cands, r, gp[e, i])
                    if not ok:
                        bad.append((s.tag, "step %d beam %d" % (k + 1, i), "clear" if clear else "band", cands, r, rl[k][e, i]))
                    if i == s.beam:
                        count[(s.family, clear)] += 1
        assert not bad, (where, len(bad), bad[:8])
        print(where, "ok", flush=True)
        report.append("%s: %s" % (where, " ".join("%s %d/%d" % (f, count[(f, True)], count[(f, False)]) for f in LS.FAMILIES)))
        for f in LS.FAMILIES:
            assert count[(f, True)] >= 10 and count[(f, False)] >= 10, (where, f)
        # the staged and the gathered bank and the three workgroup sizes: identical bits
        if first is None:
            first = g
        else:
            for key in ("obs1", "obs2", "rew", "done", "flags"):
                assert np.array_equal(first[key], g[key]), (key, where)
    return first["obs1"], clear_mask[0]


def test_lidar_at_its_decision_boundaries(torch_cuda, oracle, native):
    torch = torch_cuda
    clear_reads = {}  # n_beams -> {exact_lidar: step-1 readings}
    report = []
    for nb, hist, exact in ROWS:
        obs1, clear1 = _check_row(torch, oracle, native, nb, hist, exact, report)
        clear_reads.setdefault(nb, {})[exact] = (obs1, hist, clear1)
    # the default and the EXACT path agree on every clear beam (the same scenes at the same n_beams, either history)
    assert sorted(nb for nb, by in clear_reads.items() if len(by) == 2) == [8, 10]
    for nb, by in clear_reads.items():
        if len(by) < 2:
            continue
        (oa, ha, ma), (ob, hb, _) = by[False], by[True]
        la, lb = LS.lidar_cols(oa, nb, ha), LS.lidar_cols(ob, nb, hb)
        assert np.max(np.abs(la - lb)[ma], initial=0.0) <= 1e-9, nb
    print("\n".join(["clear/band target beams per family:"] + report))


@pytest.mark.parametrize("nb,hist", MORE_ROWS, ids=lambda v: str(v))
def test_lidar_at_the_other_beam_counts(torch_cuda, oracle, native, nb, hist):
    """the same scenes, classifier and per-beam assertions on the default path at the beam counts ROWS leaves out: each one is
    another step_kernel instantiation (how the beams are dealt to the two lidar waves, the queue entries' wave-local beam index,
    every tile's LDS layout, the observer's transposition through the lidar result buffer)"""
    report = []
    _check_row(torch_cuda, oracle, native, nb, hist, False, report)
    print("\n".join(["clear/band target beams per family:"] + report))
