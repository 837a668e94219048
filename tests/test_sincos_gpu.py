"""The bits the step kernel's own sincos returns, read out through the thrust, against the exact fixture and the host build.

No entry point returns a body's rotation, but the thrust does.  With dt = 1 (GameConfig.SPEED = 10), force_y = 1 and
ship_m_inv = 1 a ship at rest that takes action 0 ends the step with

    F_VX = (0 * damp) + ((-sin a * 1) * 1) * 1 = -sin a        F_VY = (0 * damp) + ((cos a * 1) * 1) * 1 = cos a

without a rounding (handle_discrete_action and cpBodyUpdateVelocity in shipsim_kernels.hip), and keeps its position and angle.
One env per argument of tests/golden/ref_sincos.npz, at body_scenes.CLEAR where no rotation of the hull meets anything.  The two
config fields reach ssg_create through a monkeypatched _native.default_config: the production constructor, untouched.

  (a) one step_tensor of action 0: the rotation role 0 computes at launch start (sincos_call);
  (b) a fused rollout_tensor of the actions (1, 0): step 1 only turns the rudder, the angle stays, and step 2's thrust reads the
      rotation the body role's in-loop sincos_call left in the pose slot;
  (c) as (a) on an n_ships = 4 handle after wake_dynamics(): the DYN instantiation (workgroups of 64 and 256).

(a) and (b) run on the six layouts of the edge suites (SSG_BLOCK 64 / 128 / 256, bank staged and in global memory), each with
one beam count from every compiled beam group.  Asserted per run: position and angle unchanged bit for bit, F_W zero in (a) and
(c); the contract of tests/test_sincos.py against the exact values for |a| <= 2^18 and 2^-50 absolute for the library's path
beyond; sin odd and cos even bit for bit; (0) -> (0, 1); every layout, beam count and launch shape gives the same bits; and, where
the host program of tests/test_sincos.py can be built, the device's bits ARE the host's for every |a| <= 2^18 — no instantiation
contracts or reorders the routine.  (A sin of +0.0 and -0.0 read the same through 0 * damp + (-sin a); the host test pins that sign.)

Not covered, (d) of the plan: wake_dynamics() recomputes the traffic ships' rotation columns (DC_TROT) with the same sincos_body,
but field() exposes no id for those columns (F_TRAFFIC ends at the nine body columns per ship), so they are left out.
"""
import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import body_scenes as BS
import sincos_args as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return A.load()


@pytest.fixture(scope="module")
def host_bits(fix, tmp_path_factory):
    """(sin, cos) of the host build of the committed header, or None where it cannot be built"""
    exe = A.build_host(tmp_path_factory.mktemp("sincos_host"))
    return A.run_host(exe, fix["a"]) if exe is not None else None


def _read_out(torch, N, vec, a, mode):
    n = len(a)
    vec.reset_tensor(map_ids=torch.zeros(n, dtype=torch.int32, device=vec.device))
    cols = np.zeros((6, n))
    cols[0], cols[1], cols[2] = BS.CLEAR[0], BS.CLEAR[1], a
    BS.write_pose(torch, N, vec, cols)
    if mode == "b":
        act = torch.zeros((2, n), dtype=torch.int32, device=vec.device)
        act[0] = 1
        vec.rollout_tensor(act)
    else:
        vec.step_tensor(torch.zeros(n, dtype=torch.int32, device=vec.device))
    return BS.read_state(N, vec)


def _check(fix, st, where, host, at_rest):
    a = fix["a"]
    own, z = np.abs(a) <= A.LIMIT, a == 0.0
    assert np.all(BS.same_bits(st["x"], np.full(len(a), BS.CLEAR[0]))) and np.all(BS.same_bits(st["y"], np.full(len(a), BS.CLEAR[1]))), where
    assert np.all(BS.same_bits(st["a"], a) | z) and np.all(st["a"][z] == 0.0), where
    if at_rest:  # thrust through the centre of gravity, (px0, py0) = (0, 0): no torque
        assert np.all(st["w"] == 0.0), where
    sn, cs = 0.0 - st["vx"], st["vy"]
    for name, got in (("sin", sn), ("cos", cs)):
        hi, lo = fix[name + "_hi"], fix[name + "_lo"]
        err = np.abs(A.error(got, hi, lo))
        bad = own & ~(err <= A.bound(a, hi, lo))
        assert not bad.any(), (where, name, int(bad.sum()), [(float(a[i]), float(got[i]), float(hi[i]), float(err[i])) for i in np.nonzero(bad)[0][:8]])
        assert np.all(err[~own] <= 2.0 ** -50), (where, name, "library path", float(err[~own].max()))
    assert np.all(sn[z] == 0.0) and np.all(BS.same_bits(cs[z], np.ones(2))), where
    j = A.mirror_index(a)
    assert np.all(BS.same_bits(sn[j], -sn)[~z]), (where, "sin is not odd")
    assert np.all(BS.same_bits(cs[j], cs)), (where, "cos is not even")
    if host is not None:
        for name, got, h in (("sin", sn, host[0]), ("cos", cs, host[1])):
            bad = own & ~BS.same_bits(got, h + 0.0)  # (+ 0.0: the read-out's -0.0 -> +0.0)
            assert not bad.any(), (where, name, "device bits != host bits", int(bad.sum()),
                                   [(float(a[i]), float(got[i]).hex(), float(h[i]).hex()) for i in np.nonzero(bad)[0][:8]])
    return sn, cs


def test_step_kernel_sincos_bits(torch_cuda, native, monkeypatch, fix, host_bits):
    torch, N = torch_cuda, native
    a = fix["a"]
    n = len(a)
    assert n % 64 and n > 256  # more than one workgroup at every size, a ragged last wave
    first = None
    for nb in BS.BEAMS:
        for blk, in_global in BS.LAYOUTS:
            vec = BS.make_vec(monkeypatch, n, n_beams=nb, blk=blk, in_global=in_global, force_y=1.0, ship_m_inv=1.0)
            epw, staged, _ = vec.launch_geometry()
            where = "beams %d SSG_BLOCK=%s epw=%d global=%d" % (nb, blk, epw, in_global)
            assert (epw == int(blk) or (nb > 12 and epw < int(blk))) and staged == (not in_global), where
            assert vec.cfg.dt == 1.0 and vec.cfg.thrust_px0 == 0.0 and vec.cfg.thrust_py0 == 0.0
            for mode in ("a", "b"):
                st = _read_out(torch, N, vec, a, mode)
                got = _check(fix, st, where + " mode " + mode, host_bits, at_rest=mode == "a")
                if first is None:
                    first = got
                    own = np.abs(a) <= A.LIMIT
                    for line in A.report(a, fix, got[0], got[1], own):
                        print("device " + line, flush=True)
                    print("device bits == host bits: %s" % ("yes" if host_bits is not None else "host program not built"), flush=True)
                assert np.all(BS.same_bits(first[0], got[0])) and np.all(BS.same_bits(first[1], got[1])), (where, mode, "other bits than the first run")
            vec.close()


@pytest.mark.parametrize("blk", ("64", "256"))
def test_config4_sincos_bits(torch_cuda, native, monkeypatch, fix, host_bits, blk):
    torch, N = torch_cuda, native
    a = fix["a"]
    vec = BS.make_vec(monkeypatch, len(a), n_beams=10, blk=blk, n_ships=4, force_y=1.0, ship_m_inv=1.0)
    epw, _, _ = vec.launch_geometry()
    assert epw == int(blk)
    _check(fix, _read_out(torch, N, vec, a, "a"), "config 4 SSG_BLOCK=%s" % blk, host_bits, at_rest=True)
    vec.close()
