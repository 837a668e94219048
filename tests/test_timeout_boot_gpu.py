"""The time-out bootstrap on the device: the one launch that turns a rollout's flags and terminal observations into values
(ssg_timeout_values / ssg_pop_timeout_values), the rollout that feeds it, GAE that reads it (ssg_ppo_gae_boot / ssg_pop_gae_boot), what
is refused, and one update end to end.  Every comparison of values is bitwise.  Shapes: N = 200 (three waves of 64 and a tail of 8 for
the policy kernels), N = 300 (256 + 44 for the GAE block), hidden 16 and 32, history 1 and 2 with 4 beams (D = 10, 20)."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, env_config, same_columns, torch_cuda  # noqa: F401
from population_harness import cols
from ppo_reference import actor_critic_policy, split_policy

pytestmark = pytest.mark.gpu

BEAMS = 4
SLICES = [8, 64, 100, 28]


def _env(n, history, max_steps=None, base=0, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    env = ShipVecEnv(n, n_maps=4, n_beams=BEAMS, env_config=env_config(history, max_steps), env_id_base=base, **kw)
    assert env.states_history == history * (6 + BEAMS)
    return env


def _policy(torch, D, H, layers, split, seed=0):
    return (split_policy if split else actor_critic_policy)(torch, D, H=H, layers=layers, seed=seed)[1]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _synthetic_flags(torch, N_):
    """u8 [3, 200].  Full waves (e < 192): row k holds (e + 11 k) % 32, so every full wave of every row holds each of the 32 flag
    combinations twice — but for wave 1 of row 2, where the two time-out combinations are replaced by true terminals that carry the clock
    bit too (9, 11): a full wave without a time-out lane, the early exit.  The tail wave has 8 lanes in 3 rows, 24 entries, so it cannot
    hold all 32: it holds the 16 combinations with the clock bit (row 0: 8..15, both time-outs among true terminals; row 1: 24..31, the
    clock with no goals left) and, in row 2, eight without it — a tail wave that leaves early."""
    e = torch.arange(200)
    f = torch.stack([(e + 11 * k) % 32 for k in range(3)])
    w1 = f[2, 64:128]
    w1[w1 == 8] = 9
    w1[w1 == 10] = 11
    f[0, 192:] = torch.arange(8, 16)
    f[1, 192:] = torch.arange(24, 32)
    f[2, 192:] = torch.tensor([0, 1, 2, 3, 4, 5, 16, 17])
    for k in range(3):
        for w in range(3):
            if (k, w) != (2, 1):
                assert set(f[k, 64 * w: 64 * w + 64].tolist()) == set(range(32))
    assert not N_.is_timeout(f[2, 64:128]).any() and not N_.is_timeout(f[2, 192:]).any()
    assert N_.is_timeout(f[0, 192:]).sum() == 2 and not N_.is_timeout(f[1, 192:]).any()
    return f.to(torch.uint8).to(DEV).contiguous()


def _synthetic_rows(torch, flags, D, N_, seed):
    """f64 [K, N, D]: observation-like rows (U(0, 600), a tenth of them the reset row's -1) where a time-out sits, NaN elsewhere."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    K, n = flags.shape
    rows = torch.rand((K, n, D), generator=g, device=DEV, dtype=torch.float64) * 600.0
    rows[torch.rand((K, n, D), generator=g, device=DEV) < 0.1] = -1.0
    rows[~N_.is_timeout(flags)] = float("nan")
    return rows.contiguous()


def _values_by_acting(torch, env2, act, flags, rows, N_):
    """The expectation of test 1: row by row, the rows written over a second env's obs tensor and `act` (policy_act / population_act)
    asked for its value; +0.0 where the sample is no time-out."""
    want = torch.zeros(flags.shape, dtype=torch.float32, device=DEV)
    for k in range(flags.shape[0]):
        env2.obs.copy_(rows[k])
        v = act()[2]
        want[k] = torch.where(N_.is_timeout(flags[k]), v, torch.zeros_like(v))
    return want


CASES = {
    # name: (history, hidden, layers, separate value, observation filter, population: None / "equal" / "sliced")
    "shared-1": (1, 16, 1, False, False, None),
    "shared-2": (2, 32, 2, False, False, None),
    "split-1": (1, 32, 1, True, False, None),
    "split-2": (2, 16, 2, True, False, None),
    "filter-shared-2": (2, 16, 2, False, True, None),
    "filter-split-1": (1, 32, 1, True, True, None),
    "pop-equal": (2, 16, 2, False, False, "equal"),
    "pop-equal-split-filter": (1, 32, 2, True, True, "equal"),
    "pop-sliced": (2, 32, 1, False, False, "sliced"),
    "pop-sliced-split-filter": (1, 16, 2, True, True, "sliced"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_alone_on_synthetic_flags(torch_cuda, case):
    """ssg_timeout_values / ssg_pop_timeout_values on a [3, 200] flags array with every flag combination: a non-time-out gives exactly
    +0.0f (the bit pattern; its observation row is NaN, so a product instead of a select would show), a time-out the bits of policy_act's
    value for that row on a second env.  A population's members are, on unequal slices, also the single-policy call on their shard.  A
    bound observation filter is read and left as it is."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N_
    from ship_sim_gym_amd.obs_filter import ObsFilter
    from ship_sim_gym_amd.population import NativePopulation
    history, H, layers, split, filt, pop_kind = CASES[case]
    env, env2 = _env(200, history), _env(200, history)
    D = env.states_history
    flags = _synthetic_flags(torch, N_)
    rows = _synthetic_rows(torch, flags, D, N_, seed=len(case))
    timeout = N_.is_timeout(flags)
    P = 4 if pop_kind else 1
    sizes = SLICES if pop_kind == "sliced" else [200 // P] * P
    members = [_policy(torch, D, H, layers, split, seed=m) for m in range(P)]
    shard_members = [_policy(torch, D, H, layers, split, seed=m) for m in range(P)]
    who = NativePopulation(members) if pop_kind else members[0]
    if pop_kind == "sliced":
        env.set_population_slices(sizes)
        env2.set_population_slices(sizes)
    flt = None
    if filt:  # a state that is neither empty nor the fixed scale: merged from observation-like rows, per member
        flt = ObsFilter(env, n_members=P, clip=5.0, update=True)
        g = torch.Generator(device=DEV).manual_seed(7)
        flt.update((torch.rand((200, D), generator=g, device=DEV, dtype=torch.float64) * 600.0).contiguous())
        env.set_obs_filter(flt)
        env2.set_obs_filter(flt.frozen(env2))
        state0 = flt.state.clone()
    env.reset_tensor()
    env2.reset_tensor()
    out = torch.full((3, 200), float("nan"), dtype=torch.float32, device=DEV)  # every entry is written by every call
    got = env.timeout_values(who, flags, rows, out=out)
    act = (lambda: env2.population_act(who, seed=3, step=0)) if pop_kind else (lambda: env2.policy_act(who, seed=3, step=0))
    want = _values_by_acting(torch, env2, act, flags, rows, N_)
    assert int(timeout.sum()) > 0 and not bool(torch.isnan(want).any())
    assert bool((_bits(got)[~timeout] == 0).all()), "a non-time-out must be +0.0f, bit for bit"
    assert torch.equal(_bits(got), _bits(want))
    assert float(got[timeout].abs().min()) > 0.0                             # (the values are real ones)
    if filt:
        assert torch.equal(flt.state, state0), "the launch must not update the filter"
    if pop_kind == "sliced":  # each member: the single-policy call on a shard handle of its own
        for m, n_m in enumerate(sizes):
            sh = _env(n_m, history, base=sum(sizes[:m]))
            if filt:
                f1 = ObsFilter(sh, n_members=1, clip=5.0, update=False, _state=flt.state[m: m + 1])
                sh.set_obs_filter(f1)
            sh.reset_tensor()
            one = sh.timeout_values(shard_members[m], cols(flags, m, sizes).contiguous(), cols(rows, m, sizes).contiguous())
            assert torch.equal(_bits(one), _bits(cols(got, m, sizes))), m
            sh.close()
    env.close()
    env2.close()


def _stepwise_boot(torch, env, env2, who, K, seed, step0, pop):
    """The rollout restated step by step on `env` (terminal observations enabled): policy_act, step_tensor, and per step the value of
    the terminal rows as in test 1, on env2.  Returns (the rollout's dict, boot f32 [K, N])."""
    from ship_sim_gym_amd import _native as N_
    act = env.population_act if pop else env.policy_act
    act2 = env2.population_act if pop else env2.policy_act
    keys = ("obs", "act", "logp", "val", "rew", "done", "flags")
    rows = {k: [] for k in keys}
    boot = []
    for k in range(K):
        a, lp, v, x = act(who, seed=seed, step=step0 + k)
        _, r, d, f = env.step_tensor(a)
        for name, t in zip(keys, (x, a, lp, v, r.clone(), d.clone(), f.clone())):
            rows[name].append(t)
        env2.obs.copy_(env.term_obs)  # (rows of envs that were not reset: whatever they hold; the select drops them)
        tv = act2(who, seed=0, step=0)[2]
        boot.append(torch.where(N_.is_timeout(f), tv, torch.zeros_like(tv)))
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["last_val"] = act(who, seed=seed, step=step0 + K)[2]
    return out, torch.stack(boot)


@pytest.mark.parametrize("K,pop", [(12, False), (1, False), (12, True)], ids=["K12", "K1", "K12-population"])
def test_rollout_with_the_record_bound(torch_cuda, K, pop):
    """MAX_STEPS = 5: in a rollout of 12 steps the clock expires at rows 4 and 9 (max_steps < K); K = 1 is the one step on which it
    expires.  With the record bound every output of the rollout and the env state are bitwise those of an identically seeded env with
    nothing bound; boot is the step-by-step restatement; a caller's own set_terminal_obs binding serves again afterwards."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N_
    from ship_sim_gym_amd.population import NativePopulation
    history = 2 if K == 12 else 1
    a, b, c, c2 = (_env(200, history, max_steps=5) for _ in range(4))
    D = a.states_history
    make = (lambda: NativePopulation([_policy(torch, D, 16, 2, False, seed=m) for m in range(4)])) if pop else (lambda: _policy(torch, D, 32, 1, True))
    who = make()
    roll = (lambda e, k, **kw: e.rollout_population(who, k, **kw)) if pop else (lambda e, k, **kw: e.rollout_policy(who, k, **kw))
    for e in (a, b, c, c2):
        e.reset_tensor()
    a.enable_terminal_obs(True)           # the caller's own binding, ahead of the record
    c.enable_terminal_obs(True)
    a.set_timeout_bootstrap(True, rows=2)  # (fewer rows than K = 12: the buffers grow)
    pre = 0
    if K == 1:  # four steps first, so that the one step of the rollout is the fifth of every episode still running
        pre = 4
        for e in (a, b):
            roll(e, pre, seed=11, step0=0)
        for k in range(pre):
            c.step_tensor(c.policy_act(who, seed=11, step=k)[0])
    ba = roll(a, K, seed=11, step0=pre)
    bb = roll(b, K, seed=11, step0=pre)
    assert a.timeout_bootstrap >= K and b.timeout_bootstrap == 0 and "boot" not in bb
    for k in ("obs", "act", "logp", "val", "rew", "done", "flags", "last_val"):
        assert ba[k].dtype == bb[k].dtype and torch.equal(ba[k], bb[k]), k
    assert torch.equal(a.obs, b.obs) and same_columns(torch, a, b)
    bc, boot = _stepwise_boot(torch, c, c2, who, K, 11, pre, pop)
    for k in ("obs", "act", "logp", "val", "rew", "done", "flags", "last_val"):
        assert torch.equal(ba[k], bc[k]), k
    timeout = N_.is_timeout(ba["flags"])
    n_timeout, n_terminal = int(timeout.sum()), int((ba["done"] != 0).sum()) - int(timeout.sum())
    print("K = %d: %d time-out samples, %d true terminals" % (K, n_timeout, n_terminal))
    assert n_timeout > 0
    assert bool(((ba["done"] != 0) | ~timeout).all())                        # a time-out is a done sample
    if K == 12:
        assert int(timeout[4].sum()) > 0 and int(timeout[9].sum()) > 0   # (an env that truly ended early times out on a later row)
        assert not bool(timeout[:4].any())
    assert ba["boot"].dtype == torch.float32 and tuple(ba["boot"].shape) == (K, 200)
    assert bool((_bits(ba["boot"])[~timeout] == 0).all())
    assert torch.equal(_bits(ba["boot"]), _bits(boot))
    assert float(ba["boot"][timeout].abs().min()) > 0.0
    # the caller's own terminal-observation binding is in place again: three more steps in lockstep with c (the clock expires once more)
    dones = 0
    act = a.population_act if pop else a.policy_act
    for k in range(K + pre, K + pre + 5):
        a.term_obs.fill_(float("nan"))
        c.term_obs.fill_(float("nan"))
        acts = act(who, seed=11, step=k)[0]
        _, _, d, _ = a.step_tensor(acts)
        c.step_tensor(acts)
        dones += int(d.sum())
        assert torch.equal(torch.isnan(a.term_obs), torch.isnan(c.term_obs))
        assert torch.equal(torch.nan_to_num(a.term_obs), torch.nan_to_num(c.term_obs))
        assert bool((torch.isnan(a.term_obs).all(dim=1) == (d == 0)).all())   # written for exactly the envs the step reset
    assert dones > 0
    for e in (a, b, c, c2):
        e.close()


def _gae_batch(torch, K, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    done = (torch.rand((K, n), generator=g, device=DEV) < 0.2).to(torch.uint8)
    boot = torch.randn((K, n), generator=g, device=DEV)
    boot = torch.where((done != 0) & (torch.rand((K, n), generator=g, device=DEV) < 0.6), boot, torch.zeros_like(boot))
    assert int((boot != 0).sum()) > 0 and int(((done != 0) & (boot == 0)).sum()) > 0
    return dict(rew=torch.randn((K, n), generator=g, device=DEV, dtype=torch.float64), done=done.contiguous(),
                val=torch.randn((K, n), generator=g, device=DEV), last_val=torch.randn((n,), generator=g, device=DEV),
                boot=boot.contiguous())


def _reference(ppo_mod, b, gamma, lam, rew="rew", boot=None):
    h = {k: v.cpu().numpy() for k, v in b.items() if k in (rew, "done", "val", "last_val", "boot")}
    return ppo_mod.gae_boot_reference(h[rew], h["done"], h["val"], h["last_val"], h["boot"] if boot is None else boot, gamma, lam)


def _same(torch, t, ref):
    return np.array_equal(t.cpu().numpy().view(np.int32), np.ascontiguousarray(ref).view(np.int32))


@pytest.fixture(scope="module")
def gae_env(torch_cuda):
    env = _env(300, 1)
    env.reset_tensor()
    yield env
    env.close()


def test_gae_boot_is_the_reference_and_zero_boot_is_the_plain_gae(torch_cuda, gae_env):
    """K = 5, N = 300 (a full block of 256 and one of 44): adv, ret and the statistics are bitwise gae_boot_reference's; with an
    all-zero boot they are bitwise ssg_ppo_gae's."""
    torch = torch_cuda
    from ship_sim_gym_amd import ppo as ppo_mod
    pol = _policy(torch, gae_env.states_history, 16, 1, False)
    ppo = ppo_mod.NativePPO(pol, gae_env)
    for gamma, lam in ((0.99, 0.95), (0.9, 1.0)):
        b = _gae_batch(torch, 5, 300, seed=5)
        adv, ret = ppo.gae(b, gamma, lam)
        stats = ppo.adv_stats().clone()
        radv, rret, rstats = _reference(ppo_mod, b, gamma, lam)
        assert _same(torch, adv, radv) and _same(torch, ret, rret) and _same(torch, stats, rstats[:3])
        plain = {k: v for k, v in b.items() if k != "boot"}
        padv, pret = ppo.gae(plain, gamma, lam)
        pstats = ppo.adv_stats().clone()
        assert not torch.equal(padv, adv)                                    # the bootstrap changes the time-outs' targets
        zero = dict(plain, boot=torch.zeros_like(b["boot"]))
        zadv, zret = ppo.gae(zero, gamma, lam)
        assert torch.equal(_bits(zadv), _bits(padv)) and torch.equal(_bits(zret), _bits(pret))
        assert torch.equal(_bits(ppo.adv_stats()), _bits(pstats))


def test_gae_boot_with_a_return_filter_takes_the_normalised_reward_and_the_raw_boot(torch_cuda, gae_env):
    torch = torch_cuda
    from ship_sim_gym_amd import ppo as ppo_mod
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    pol = _policy(torch, gae_env.states_history, 16, 1, False)
    ppo = ppo_mod.NativePPO(pol, gae_env)
    b = _gae_batch(torch, 5, 300, seed=6)
    raw = b["rew"].clone()
    adv, ret = ppo.gae(b, 0.99, 0.95, return_filter=ReturnFilter(gae_env, gamma=0.99))
    assert torch.equal(b["rew"], raw) and not torch.equal(b["rew_norm"], raw)
    radv, rret, rstats = _reference(ppo_mod, b, 0.99, 0.95, rew="rew_norm")
    assert _same(torch, adv, radv) and _same(torch, ret, rret) and _same(torch, ppo.adv_stats(), rstats[:3])


@pytest.mark.parametrize("sizes", [[75, 75, 75, 75], [8, 264, 20, 8]], ids=["equal", "sliced"])
def test_population_gae_boot_is_each_members_single_call(torch_cuda, sizes):
    """Per-member gammas and lambdas, on equal slices and on unequal ones (a member of 264 envs: two blocks): each member's adv, ret and
    statistics are bitwise ssg_ppo_gae_boot's on its shard of the batch, and the reference's."""
    torch = torch_cuda
    from ship_sim_gym_amd import ppo as ppo_mod
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    env = _env(300, 1)
    env.reset_tensor()
    D = env.states_history
    if len(set(sizes)) > 1:
        env.set_population_slices(sizes)
    pop = NativePopulation([_policy(torch, D, 16, 1, False, seed=m) for m in range(4)])
    gammas, lams = [0.99, 0.9, 0.95, 0.999], [0.95, 1.0, 0.8, 0.9]
    pp = PopulationPPO(pop, env, gamma=gammas, lam=lams)
    b = _gae_batch(torch, 5, 300, seed=8)
    adv, ret = pp.gae(b)
    stats = pp.workspace[:64].view(torch.float32).view(4, 4).clone()
    one = ppo_mod.NativePPO(_policy(torch, D, 16, 1, False), env)
    for m in range(4):
        sb = {k: cols(v, m, sizes).contiguous() for k, v in b.items() if k in ("rew", "done", "val", "last_val", "boot")}
        sadv, sret = one.gae(sb, gammas[m], lams[m])
        assert torch.equal(_bits(cols(adv, m, sizes)), _bits(sadv)) and torch.equal(_bits(cols(ret, m, sizes)), _bits(sret)), m
        assert torch.equal(_bits(stats[m, :3]), _bits(one.adv_stats())), m
        radv, rret, rstats = _reference(ppo_mod, sb, gammas[m], lams[m])
        assert _same(torch, sadv, radv) and _same(torch, sret, rret) and _same(torch, stats[m, :3], rstats[:3]), m
    env.close()


def _raw_rollout(env, pol, K, flags=True):
    """ssg_rollout_policy itself, on buffers of K rows filled with a sentinel: (the status, the buffers)."""
    import torch
    from ship_sim_gym_amd import _native as N_
    out, p = env._rollout_buffers(K, None, "raw")
    for k in ("val", "logp", "last_val"):
        out[k].fill_(-7.0)
    rec = pol.to_native()
    rc = N_.lib().ssg_rollout_policy(env._h, C.byref(rec), K, None, 1, 0, C.c_void_p(env.obs.data_ptr()), p["act"], p["logp"], p["val"], p["obs"],
                                     p["rew"], p["done"], p["flags"] if flags else None, p["last_val"], env.num_envs, env._stream())
    torch.cuda.synchronize()
    return rc, out


def test_refusals_launch_nothing_and_keep_the_binding(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N_
    from ship_sim_gym_amd._native import ShipSimError
    # the handles ssg_set_terminal_obs refuses
    for kw, text in ((dict(history=3), "history > 2"), (dict(history=1, auto_reset=False), "SSG_FLAG_AUTO_RESET")):
        history = kw.pop("history")
        e = _env(200, history, **kw)
        with pytest.raises(ShipSimError, match=text):
            e.set_timeout_bootstrap(True, rows=4)
        assert e.timeout_bootstrap == 0
        e.close()
    env, twin = _env(200, 1, max_steps=5), _env(200, 1, max_steps=5)
    pol = _policy(torch, env.states_history, 16, 1, False)
    env.reset_tensor()
    twin.reset_tensor()
    env.set_timeout_bootstrap(True, rows=4)
    boot0 = env._timeout_boot["boot"]
    boot0.fill_(-7.0)

    def untouched(out):
        assert bool((out["val"] == -7.0).all()) and bool((out["last_val"] == -7.0).all()) and bool((boot0 == -7.0).all())
        assert same_columns(torch, env, twin) and torch.equal(env.obs, twin.obs)
        assert env.timeout_bootstrap == 4

    rc, out = _raw_rollout(env, pol, 5)                                      # K > rows
    assert rc == -1 and "rows" in N_.lib().ssg_last_error(env._h).decode()
    untouched(out)
    rc, out = _raw_rollout(env, pol, 4, flags=False)                         # NULL flags
    assert rc == -1 and "dev_flags_KN" in N_.lib().ssg_last_error(env._h).decode()
    untouched(out)
    # a capturing stream
    bufs, _ = env._rollout_buffers(2, None, "capture")
    bufs["boot"] = boot0
    bufs["val"].fill_(-7.0)
    bufs["last_val"].fill_(-7.0)
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    refused = False
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            env.rollout_policy(pol, 2, seed=1, out=bufs)
        except ShipSimError as ex:
            refused = "capturing" in str(ex)
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert refused
    untouched(bufs)
    # ... and with the same arguments outside a capture the rollout runs, as it does on the twin with nothing bound
    ok = env.rollout_policy(pol, 4, seed=1)
    ref = twin.rollout_policy(pol, 4, seed=1)
    assert torch.equal(ok["val"], ref["val"]) and tuple(ok["boot"].shape) == (4, 200) and same_columns(torch, env, twin)
    env.set_timeout_bootstrap(False)
    assert env.timeout_bootstrap == 0 and "boot" not in env.rollout_policy(pol, 2, seed=2)
    env.close()
    twin.close()


def test_two_updates_end_to_end(torch_cuda):
    """NativePPO for two updates at N = 200, K = 12, MAX_STEPS = 5, with the bootstrap on and off (off: what the parent computes): the
    parameters stay finite, and they differ — the time-outs' targets enter the update."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    params = {}
    for on in (False, True):
        env = _env(200, 2, max_steps=5)
        env.reset_tensor()
        pol = _policy(torch, env.states_history, 32, 2, True)
        ppo = NativePPO(pol, env, perm_seed=3)
        if on:
            env.set_timeout_bootstrap(True)
        for u in range(2):
            batch = env.rollout_policy(pol, 12, seed=21, step0=12 * u)
            assert ("boot" in batch) == on
            ppo.gae(batch, 0.99, 0.95)
            ppo.update(batch, None, 2, 4)
        torch.cuda.synchronize()
        params[on] = pol.params.clone()
        env.close()
    assert bool(torch.isfinite(params[True]).all()) and bool(torch.isfinite(params[False]).all())
    assert not torch.equal(params[True], params[False])


def test_trainers_run_with_the_flag_and_change_nothing_where_no_clock_expires(torch_cuda):
    """Both trainers with timeout_bootstrap on (in process, small): they run, and since no episode reaches the default MAX_STEPS =
    1 000 in 16 steps, boot is +0 everywhere and the trained parameters are bit for bit the flag-off run's.  The torch update refuses."""
    torch = torch_cuda
    from gpu_support import load_script
    quiet = lambda *a, **k: None  # noqa: E731
    single, pbt = load_script("train/ppo_torch.py"), load_script("train/pbt_native.py")
    runs = {}
    for on in (False, True):
        _, d = single.train(envs=256, updates=2, horizon=8, mode="native", update="native", timeout_bootstrap=on, return_details=True, log=quiet)
        _, p = pbt.train(members=3, envs_per_member=64, updates=2, horizon=8, perturb_every=1, timeout_bootstrap=on, return_details=True,
                         log=quiet)
        runs[on] = (torch.cat([t.reshape(-1) for t in d["params"]]), p["params"])
    for a, b in zip(runs[False], runs[True]):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    with pytest.raises(ValueError, match="timeout_bootstrap"):
        single.train(envs=64, updates=1, horizon=4, mode="native", update="torch", timeout_bootstrap=True, log=quiet)
