"""The time-out bootstrap without a device: the numpy restatement of ssg_ppo_gae_boot against a case worked by hand and against the
plain GAE, the time-out predicate over every flags byte, what ssg_set_timeout_boot refuses, and the binding's exports."""
import ctypes as C

import numpy as np
import pytest

from ship_sim_gym_amd import ppo

f32 = np.float32
NEW_SYMBOLS = ("ssg_set_timeout_boot", "ssg_get_timeout_boot", "ssg_timeout_values", "ssg_pop_timeout_values", "ssg_ppo_gae_boot",
               "ssg_pop_gae_boot")


def test_reference_on_a_three_step_case_worked_by_hand():
    """Two envs, three steps.  Env 0 times out at t = 1 (done, boot = V(terminal observation) = 2.0); env 1 truly ends at t = 0 (done,
    boot = +0).  Every line below is the issue's walk written out by hand in f32, product by product."""
    g, gl = f32(0.5), f32(0.5 * 0.5)
    rew = np.array([[1.0, -1.0], [0.25, 0.5], [2.0, 3.0]])
    done = np.array([[0, 1], [1, 0], [0, 0]], dtype=np.uint8)
    val = np.array([[0.5, 1.5], [1.0, -0.5], [0.75, 0.25]], dtype=f32)
    last = np.array([4.0, -2.0], dtype=f32)
    boot = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 0.0]], dtype=f32)
    # env 0
    d2 = (f32(2.0) + g * f32(4.0)) - f32(0.75)              # t = 2, not done: the target is last_val
    a2 = d2
    d1 = (f32(0.25) + g * f32(2.0)) - f32(1.0)              # t = 1, the time-out: the target is boot, not val[2]
    a1 = d1 + (gl * f32(0.0)) * a2                          # ... and the lambda chain is cut
    d0 = (f32(1.0) + g * f32(1.0)) - f32(0.5)               # t = 0, not done: the target is val[1]
    a0 = d0 + (gl * f32(1.0)) * a1
    # env 1
    e2 = (f32(3.0) + g * f32(-2.0)) - f32(0.25)
    b2 = e2
    e1 = (f32(0.5) + g * f32(0.25)) - f32(-0.5)
    b1 = e1 + (gl * f32(1.0)) * b2
    e0 = (f32(-1.0) + g * f32(0.0)) - f32(1.5)              # t = 0, the true terminal: the target is +0
    b0 = e0 + (gl * f32(0.0)) * b1
    want = np.array([[a0, b0], [a1, b1], [a2, b2]], dtype=f32)
    assert (a1, b0) == (f32(0.25), f32(-2.5))               # the two done samples, in plain numbers
    adv, ret, stats = ppo.gae_boot_reference(rew, done, val, last, boot, gamma=0.5, lam=0.5)
    assert adv.dtype == f32 and ret.dtype == f32 and stats.dtype == f32
    np.testing.assert_array_equal(adv, want)
    np.testing.assert_array_equal(ret, want + val)
    # without the bootstrap the time-out's advantage is what a return of 0 gives
    plain, _, _ = ppo.gae_boot_reference(rew, done, val, last, np.zeros_like(boot), gamma=0.5, lam=0.5)
    assert plain[1, 0] == (f32(0.25) + g * f32(0.0)) - f32(1.0) and plain[1, 0] != adv[1, 0]
    np.testing.assert_array_equal(plain[:, 1], adv[:, 1])   # (env 1 has no time-out: nothing changes)
    a64 = want.astype(np.float64).reshape(-1)
    mean = a64.sum() / 6.0
    std = np.sqrt(((a64 - mean) ** 2).sum() / 5.0)
    assert abs(float(stats[0]) - mean) <= 1e-6 and abs(float(stats[1]) - (std + 1e-8)) <= 1e-6
    assert stats[2] == f32(1.0) / stats[1] and stats[3] == 0.0


@pytest.mark.parametrize("K,n,gamma,lam", [(5, 300, 0.99, 0.95), (1, 2, 0.9, 1.0), (7, 257, 1.0, 0.0)])
def test_reference_with_zero_boot_is_the_plain_gae(K, n, gamma, lam):
    """boot == +0 everywhere: adv and ret are bit for bit the trainer's GAE loop (tests/ppo_reference.torch_gae, what ssg_ppo_gae
    reproduces), and the statistics are its mean and unbiased std."""
    import torch
    from ppo_reference import torch_gae
    rng = np.random.RandomState(K * 1000 + n)
    rew = rng.randn(K, n)
    done = (rng.rand(K, n) < 0.3).astype(np.uint8)
    val, last = rng.randn(K, n).astype(f32), rng.randn(n).astype(f32)
    adv, ret, stats = ppo.gae_boot_reference(rew, done, val, last, np.zeros((K, n), dtype=f32), gamma=gamma, lam=lam)
    b = {"rew": torch.from_numpy(rew), "done": torch.from_numpy(done), "val": torch.from_numpy(val), "last_val": torch.from_numpy(last)}
    tadv, tret = torch_gae(torch, b, gamma, lam)
    np.testing.assert_array_equal(adv, tadv.numpy())
    np.testing.assert_array_equal(ret, tret.numpy())
    a64 = adv.astype(np.float64)
    assert abs(float(stats[0]) - a64.mean()) <= 1e-6 * max(1.0, abs(a64.mean()))
    assert abs(float(stats[1]) - (a64.std(ddof=1) + 1e-8)) <= 1e-5 * a64.std(ddof=1)
    # and a boot that is non-zero only where done is 0 changes nothing: the select reads it at done samples alone
    noise = np.where(done != 0, f32(0), rng.randn(K, n).astype(f32))
    adv2, ret2, stats2 = ppo.gae_boot_reference(rew, done, val, last, noise, gamma=gamma, lam=lam)
    np.testing.assert_array_equal(adv2, adv)
    np.testing.assert_array_equal(ret2, ret)
    np.testing.assert_array_equal(stats2, stats)


def test_timeout_predicate_over_all_flag_combinations():
    """Sample (k, e) is a time-out when the clock's bit is set and no true terminal's is; SSG_EV_GOAL_REACHED does not matter."""
    from ship_sim_gym_amd import _native as N
    assert (N.EV_COLLIDING, N.EV_GOAL_REACHED, N.EV_OUT_OF_BOUNDS, N.EV_MAX_STEPS, N.EV_NO_GOALS_LEFT) == (1, 2, 4, 8, 16)
    want = []
    for f in range(32):
        collided, goal, out, clock, no_goals = (bool(f >> i & 1) for i in range(5))
        want.append(clock and not (collided or out or no_goals))
        assert bool(N.is_timeout(f)) == want[-1], f
    assert [f for f in range(32) if want[f]] == [8, 10]                     # the clock alone, or with a goal reached on the last step
    np.testing.assert_array_equal(N.is_timeout(np.arange(32, dtype=np.uint8)), np.array(want))


def _handle(native, **kw):
    c = native.default_config()
    c.n_envs, c.flags = 64, native.FLAG_AUTO_RESET
    for k, v in kw.items():
        setattr(c, k, v)
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _record(native, rows=4, term=0x10000, boot=0x20000):
    r = native.TimeoutBootRecord()
    r.struct_size, r.rows, r.dev_term_obs_KND, r.dev_boot_KN = C.sizeof(native.TimeoutBootRecord), rows, term, boot
    return r


def test_record_refusals_that_need_no_device(native):
    """ssg_set_timeout_boot is host only: it refuses what ssg_set_terminal_obs refuses and a malformed record, keeps the previous
    binding when it refuses, and NULL unbinds."""
    L = native.lib()
    got = native.TimeoutBootRecord()
    assert L.ssg_set_timeout_boot(None, None) == -1 and L.ssg_get_timeout_boot(None, C.byref(got)) == -1
    for kw, code, text in (({"history": 3}, -4, b"history > 2"), ({"flags": 0}, -1, b"SSG_FLAG_AUTO_RESET")):
        h = _handle(native, **kw)
        rec = _record(native)
        assert L.ssg_set_timeout_boot(h, C.byref(rec)) == code and text in L.ssg_last_error(h)
        native.check(L.ssg_get_timeout_boot(h, C.byref(got)), h)
        assert got.struct_size == 0 and got.rows == 0 and not got.dev_term_obs_KND and not got.dev_boot_KN
        assert L.ssg_set_timeout_boot(h, None) == 0                         # NULL always passes
        L.ssg_destroy(h)
    for hist in (1, 2):
        h = _handle(native, history=hist)
        native.check(L.ssg_get_timeout_boot(h, C.byref(got)), h)
        assert got.struct_size == 0                                         # nothing bound at first
        good = _record(native, rows=7)
        native.check(L.ssg_set_timeout_boot(h, C.byref(good)), h)
        bad = [_record(native, rows=0), _record(native, rows=-3), _record(native, term=None), _record(native, boot=None), _record(native)]
        bad[-1].struct_size -= 4
        for rec in bad:
            assert L.ssg_set_timeout_boot(h, C.byref(rec)) == -1 and b"ssg_set_timeout_boot" in L.ssg_last_error(h)
            native.check(L.ssg_get_timeout_boot(h, C.byref(got)), h)
            assert (got.struct_size, got.rows, got.dev_term_obs_KND, got.dev_boot_KN) == (C.sizeof(native.TimeoutBootRecord), 7, 0x10000,
                                                                                         0x20000)  # the previous binding is kept
        # a caller's own ssg_set_terminal_obs binding and this record do not touch each other
        assert L.ssg_set_terminal_obs(h, C.c_void_p(0x3000)) == 0
        native.check(L.ssg_get_timeout_boot(h, C.byref(got)), h)
        assert got.rows == 7
        native.check(L.ssg_set_timeout_boot(h, None), h)
        native.check(L.ssg_get_timeout_boot(h, C.byref(got)), h)
        assert got.struct_size == 0 and got.rows == 0
        # the entry points that launch refuse an unbound handle before they look at a device
        pol = native.Policy()
        assert L.ssg_timeout_values(h, C.byref(pol), 1, None, None, None, 64, None) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)
        hp = native.PpoHparams()
        assert L.ssg_ppo_gae_boot(h, C.byref(hp), 1, 64, None, None, None, None, None, None, None, None, 0, None) == -3
        L.ssg_destroy(h)


def test_binding_exports_every_new_symbol(native):
    L = native.lib()
    for name in NEW_SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert C.sizeof(native.TimeoutBootRecord) == 24
    import inspect
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    assert "rows" in inspect.signature(ShipVecEnv.set_timeout_bootstrap).parameters
    assert "return_filter" in inspect.signature(ppo.NativePPO.gae).parameters and "return_filter" in inspect.signature(PopulationPPO.gae).parameters


def test_trainers_take_the_flag_and_the_torch_update_refuses_it():
    """--timeout-bootstrap is off by default; train/ppo_torch.py takes it with --mode native --update native only."""
    from gpu_support import load_script
    single, pbt = load_script("train/ppo_torch.py"), load_script("train/pbt_native.py")
    assert single.parse_args([]).timeout_bootstrap is False and pbt.parse_args([]).timeout_bootstrap is False
    assert single.parse_args(["--mode", "native", "--update", "native", "--timeout-bootstrap"]).timeout_bootstrap is True
    assert pbt.parse_args(["--timeout-bootstrap"]).timeout_bootstrap is True
    for argv in (["--timeout-bootstrap"], ["--mode", "native", "--timeout-bootstrap"], ["--mode", "eager", "--timeout-bootstrap"]):
        with pytest.raises(SystemExit):
            single.parse_args(argv)
    import inspect
    for mod in (single, pbt):
        assert inspect.signature(mod.train).parameters["timeout_bootstrap"].default is False
