"""The body role's integrator, bit for bit: action decode, thrust, cpBodyUpdatePosition, cpBodyUpdateVelocity.

The chain's contract is that every product and sum rounds where Chipmunk's does (-ffp-contract=off, shipsim_kernels.hip); the
parity suites hold the player's columns to 1e-9 only, so one a * b + c fused in one instantiation would pass them.  Here the
columns F_X, F_Y, F_ANGLE, F_VX, F_VY, F_W, F_RUDDER and bit 7 of F_GOAL_MASK are compared BITWISE with body_scenes.restate_step,
at dt = 0.1, 1.0, 3.0000000000000004 and 4.0 (GameConfig.SPEED 1, 10, 30, 40): at dt = 1 a fused x + vx * dt rounds like the
unfused one, at the others it does not (at 4.0 the product is exact, but damp = 0.4^4 is not).

test_coast_and_rudder_lattice   K = 40 steps, as single launches and as one fused launch, on all six layouts.  Lanes that only
    turn the rudder carry velocities of both signs from 1e-300 to 1e3, +-0.0 and subnormals — no sincos in their chain — with
    rudder sequences that reach +-rudder_max, push against the clamp, come back and cross 0.  Every eighth lane never touches the
    rudder: it thrusts, at angle 0 and through the centre of gravity, where the rotation is (0, 1) exactly and the torque zero, so
    the restatement covers it too; its bit 7 stays clear and its rudder 0.  Every step of the single launches and of the fused
    trajectory's newest frame (x, y, rudder, angle) equals the restatement; fused equals single in every column.

test_one_step_from_a_written_state   K = 1 from a state written after a four-step prelude that leaves every rudder value of the
    lattice with bit 7 set, and rudder 0 with bit 7 clear (px = px0); thrust points (0, 0) and (10, 22.5).  Lanes thrust or turn
    (both arms of every select inside every wave, asserted on the inputs), at fixture angles whose sin and cos exceed 2^-30, with
    w, vx, vy non-zero.  x, y, angle, rudder and bit 7 equal the restatement outright; (vx, vy, w) equal, as ONE triple, the
    restatement at one of the nine (sin, cos) in {correctly rounded, +-1 ulp}^2 — sincos_body's contract at these angles.  The same
    envs are within 1e-5 of the oracle, which ties the restatement's px0 / bit-7 rule to the reference's (models.py:109,146).
"""
import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import body_scenes as BS
import sincos_args as A
from helpers import oracle_cfg

pytestmark = pytest.mark.gpu

ATOL = 1e-5  # the suite's parity tolerance (tests/test_parity_gpu.py)
COLS = ("x", "y", "a", "vx", "vy", "w")


def _assert_equal(got, want, where):
    for name in COLS:
        bad = ~BS.same_bits(got[name], want[name])
        assert not bad.any(), (where, name, int(bad.sum()), [(int(e), float(got[name][e]).hex(), float(want[name][e]).hex()) for e in np.nonzero(bad)[0][:6]])
    assert np.array_equal(got["rudder"], want["rudder"]), (where, "rudder")
    assert np.array_equal(got["bit7"], want["bit7"]), (where, "bit 7")


@pytest.mark.parametrize("speed", BS.SPEEDS)
def test_coast_and_rudder_lattice(torch_cuda, native, monkeypatch, speed):
    torch, N = torch_cuda, native
    cols, act, untouched = BS.coast_lanes()
    n = cols.shape[1]
    # the inputs: the designed rudder histories, from the actions alone
    walk = np.zeros(n, dtype=np.int64)
    hist = []
    for k in range(BS.K):
        walk = np.clip(walk + np.where(act[k] == 1, -5, np.where(act[k] == 2, 5, 0)), -10, 10)
        hist.append(walk.copy())
    hist = np.stack(hist)
    assert ((hist[:-1] == 10) & (act[1:] == 2)).sum() > 100 and ((hist[:-1] == -10) & (act[1:] == 1)).sum() > 100  # the clamp is pushed against ...
    assert ((hist[:-1] == 10) & (hist[1:] == 5)).any() and ((hist[:-1] == -10) & (hist[1:] == -5)).any()  # ... and left again
    assert ((hist[:-1] == -5) & (hist[1:] == 0)).any() and ((hist[:-1] == 5) & (hist[1:] == 0)).any()     # 0 is crossed both ways
    assert untouched.sum() >= 40 and np.all(hist[:, untouched] == 0)
    for w0 in range(0, n, 64):  # every wave: thrusting and turning lanes, both turns
        a0 = act[0, w0: w0 + 64]
        assert {0, 1, 2} <= set(a0.tolist())
    rot = (np.zeros(n), np.ones(n))
    final = None
    for li, (blk, in_global) in enumerate(BS.LAYOUTS):
        nb = BS.BEAMS[li % len(BS.BEAMS)]
        vec = BS.make_vec(monkeypatch, n, n_beams=nb, blk=blk, in_global=in_global, speed=speed)
        where = "SPEED %d dt %r beams %d SSG_BLOCK=%s global=%d" % (speed, vec.cfg.dt, nb, blk, in_global)
        kk = BS.constants(vec)
        ids = torch.zeros(n, dtype=torch.int32, device=vec.device)
        acts = torch.from_numpy(act).to(vec.device)
        F = 6 + nb
        new = (vec.cfg.history - 1) * F
        # single launches
        vec.reset_tensor(map_ids=ids)
        BS.write_pose(torch, N, vec, cols)
        st = BS.read_state(N, vec)
        assert not st["bit7"].any() and not st["rudder"].any()
        want = [st]
        for k in range(BS.K):
            obs = vec.step_tensor(acts[k])[0].cpu().numpy()
            want.append(BS.restate_step(want[-1], act[k], kk, *rot))
            got = BS.read_state(N, vec)
            _assert_equal(got, want[-1], where + " single step %d" % k)
            assert np.all(got["a"][untouched] == 0.0) and not got["bit7"][untouched].any()
            for c, name in ((0, "x"), (1, "y"), (3, "a")):
                assert np.all(BS.same_bits(obs[:, new + c], got[name])), (where, "observation row", name, k)
            assert np.array_equal(obs[:, new + 2], got["rudder"].astype(np.float64))
        single = got
        # one fused launch
        vec.reset_tensor(map_ids=ids)
        BS.write_pose(torch, N, vec, cols)
        traj = vec.rollout_tensor(acts, trajectory=True)[0].cpu().numpy()
        fused = BS.read_state(N, vec)
        _assert_equal(fused, single, where + " fused != single")
        for k in range(BS.K):
            for c, name in ((0, "x"), (1, "y"), (3, "a")):
                assert np.all(BS.same_bits(traj[k][:, new + c], want[k + 1][name])), (where, "fused trajectory", name, k)
            assert np.array_equal(traj[k][:, new + 2], want[k + 1]["rudder"].astype(np.float64)), (where, "fused trajectory rudder", k)
        if final is None:
            final = fused
        _assert_equal(fused, final, where + " != the first layout")
        vec.close()


@pytest.mark.parametrize("point", ((0.0, 0.0), (10.0, 22.5)), ids=("px0_0", "px0_bb_centre"))
@pytest.mark.parametrize("speed", BS.SPEEDS)
def test_one_step_from_a_written_state(torch_cuda, oracle, native, monkeypatch, speed, point):
    torch, O, N = torch_cuda, oracle, native
    fix = A.load()
    cols, prelude, act, combo, which = BS.step_lanes(fix)
    n = cols.shape[1]
    rud0, bit0 = np.array(BS.PRELUDE_RUDDER)[combo], combo != 5
    # both arms of every select inside every wave: bit 7 (px = -rudder / px0), thrust or not, turn left / right, the clamp's two
    # sides hit (rudder at +-max pushed further) and not hit, and every rudder value under the thrust
    for w0 in range(0, n, 64):
        s = slice(w0, w0 + 64)
        assert bit0[s].any() and (~bit0[s]).any() and {0, 1, 2} <= set(act[s].tolist())
        assert ((rud0[s] == -10) & (act[s] == 1)).any() and ((rud0[s] == 10) & (act[s] == 2)).any()
        assert ((rud0[s] == -10) & (act[s] == 2)).any() and ((rud0[s] == 10) & (act[s] == 1)).any()
        assert {(r, b) for r, b, t in zip(rud0[s].tolist(), bit0[s].tolist(), act[s].tolist()) if t == 0} == {(-10, True), (-5, True), (0, True), (5, True), (10, True), (0, False)}
    assert np.all(cols[3:] != 0.0)
    # the oracle's run
    vec = BS.make_vec(monkeypatch, n, n_beams=10, speed=speed, thrust_px0=point[0], thrust_py0=point[1])
    ob = O.Batch(n, oracle_cfg(O, vec), vec.bank_polys, vec.bank_goals, map_ids=np.zeros(n, dtype=np.int32))
    ob.reset()
    for k in range(4):
        ob.step(prelude[k], auto_reset=False, n_threads=8)
    for e in range(n):
        ob.poke_state(e, *cols[:, e])
    ob.step(act, auto_reset=False, n_threads=8)
    pk = ob.peek_all()
    vec.close()
    # the restatement at the nine candidate rotations
    s_hi, c_hi = fix["sin_hi"][which], fix["cos_hi"][which]
    cands = [(s, c) for s in (np.nextafter(s_hi, -np.inf), s_hi, np.nextafter(s_hi, np.inf))
             for c in (np.nextafter(c_hi, -np.inf), c_hi, np.nextafter(c_hi, np.inf))]
    first = None
    for li, (blk, in_global) in enumerate(BS.LAYOUTS):
        nb = BS.BEAMS[(li + 1) % len(BS.BEAMS)]
        vec = BS.make_vec(monkeypatch, n, n_beams=nb, blk=blk, in_global=in_global, speed=speed, thrust_px0=point[0], thrust_py0=point[1])
        where = "SPEED %d point %r beams %d SSG_BLOCK=%s global=%d" % (speed, point, nb, blk, in_global)
        kk = BS.constants(vec)
        vec.reset_tensor(map_ids=torch.zeros(n, dtype=torch.int32, device=vec.device))
        vec.rollout_tensor(torch.from_numpy(prelude).to(vec.device))
        BS.write_pose(torch, N, vec, cols)
        st = BS.read_state(N, vec)
        assert np.array_equal(st["rudder"], rud0) and np.array_equal(st["bit7"], bit0), where
        for i, name in enumerate(COLS):
            assert np.all(BS.same_bits(st[name], cols[i])), (where, "written", name)
        vec.step_tensor(torch.from_numpy(act).to(vec.device))
        got = BS.read_state(N, vec)
        wants = [BS.restate_step(st, act, kk, s, c) for s, c in cands]
        for name in ("x", "y", "a"):
            assert np.all(BS.same_bits(got[name], wants[4][name])), (where, name)
        assert np.array_equal(got["rudder"], wants[4]["rudder"]) and np.array_equal(got["bit7"], wants[4]["bit7"]), where
        match = np.stack([BS.same_bits(got["vx"], w["vx"]) & BS.same_bits(got["vy"], w["vy"]) & BS.same_bits(got["w"], w["w"]) for w in wants])
        bad = ~match.any(axis=0)
        assert not bad.any(), (where, "no candidate rotation gives the device's (vx, vy, w)", int(bad.sum()),
                               [(int(e), int(act[e]), int(rud0[e]), bool(bit0[e]), float(cols[2, e]),
                                 [(float(got[c][e]).hex(), float(wants[4][c][e]).hex()) for c in ("vx", "vy", "w")]) for e in np.nonzero(bad)[0][:4]])
        assert np.all(match[:, act != 0])  # (a lane that turns reads no rotation)
        # the reference's rule for the thrust point, through the oracle
        for c, name in enumerate(COLS[:2] + ("vx", "vy", "a", "w")):
            err = np.abs(got[name] - pk[:, c])
            assert np.all(err <= ATOL), (where, "oracle", name, float(err.max()))
        assert np.array_equal(got["rudder"], pk[:, 6].astype(np.int32)), where
        if first is None:
            first = got
        _assert_equal(got, first, where + " != the first layout")
        vec.close()
    print("SPEED %d point %r: candidates used %s" % (speed, point, match[:, act == 0].sum(axis=1).tolist()), flush=True)
