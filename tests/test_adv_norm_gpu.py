"""GPU checks of per-minibatch advantage normalisation (ssg_ppo_set_adv_norm, SSG_ADV_NORM_MINIBATCH; NativePPO / PopulationPPO with
adv_norm="minibatch"; --adv-norm of the trainers): the statistics bit for bit against the numpy restatement of the two launches, the
gradient kernel wired to them bit for bit, gradients and whole updates against f64 autograd with the per-minibatch rule, batch mode left
alone, populations bit for bit against NativePPO on each member's shard, the member-count refusal, and the trainers."""
import numpy as np
import pytest

from gpu_support import DEV, load_script, vec
from gpu_support import torch_cuda  # noqa: F401
from population_harness import age, cached, member_hparams as _hp, perms_per_member, shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy, check_per_tensor, minibatch, plain_loss, ref_grad, split_policy, synthetic_batch, \
    synthetic_batch_logp_noise

pytestmark = pytest.mark.gpu

EPS = 1e-8
EXT_TERMS = dict(vf_clip=0.05, kl_coef=1.0, max_grad_norm=0.5)

_ENVS, _SYNTH = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    _SYNTH.clear()


def _env(D, n=64):
    """One small handle per obs_dim (the PPO calls take their own K and N)."""
    if (D, n) not in _ENVS:
        _ENVS[(D, n)] = vec(n, D)
    return _ENVS[(D, n)]


def _default_env(n):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    if ("default", n) not in _ENVS:
        _ENVS[("default", n)] = ShipVecEnv(n, n_maps=64)
    return _ENVS[("default", n)]


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the statistics, bitwise against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
K1, N1 = 16, 4125


def _stats_setup(torch):
    """(pol, ppo, batch) at D = 7, H = 16, one layer, over a synthetic batch of 66 000 samples; computed once."""
    if "stats" not in _SYNTH:
        from ship_sim_gym_amd.ppo import NativePPO
        _, pol = actor_critic_policy(torch, 7, 16, 1, "tanh", 3, seed=1)
        ppo = NativePPO(pol, _env(7), adv_norm="minibatch")
        b = synthetic_batch_logp_noise(torch, pol, K1, N1, 5)
        ppo.gae(b)
        _SYNTH["stats"] = (pol, ppo, b)
    return _SYNTH["stats"]


def _check_stats(torch, ppo, b, idx):
    from ship_sim_gym_amd.ppo import minibatch_adv_reference
    n = b["adv"].numel()
    ppo.minibatch_adv_stats().fill_(float("nan"))                            # every entry of the row must be written,
    ppo.minibatch_adv_partials().fill_(float("nan"))                         # and every partial that is read
    ppo.grad(b, idx)
    got, part = ppo.minibatch_adv_stats().clone(), ppo.minibatch_adv_partials().clone()
    valid = (idx >= 0) & (idx < n)
    gathered = b["adv"].reshape(-1)[idx.clamp(0, n - 1)]
    want, want_part = minibatch_adv_reference(gathered.cpu().numpy(), valid.cpu().numpy(), EPS, partials=True)
    assert got.shape == (1, 4) and got.dtype == torch.float32 and part.shape == (1, 64, 3) and part.dtype == torch.float64
    assert np.array_equal(_bits(got[0]), want.view(np.uint32)), (idx.numel(), got.tolist(), want.tolist())
    # the f64 partials, bit for bit: they show the ORDER of the sums, which the f32 row seldom does
    B = min(64, -(-idx.numel() // 1024))
    assert want_part.shape == (B, 3) and want_part[:, 2].sum() == int(valid.sum())
    assert np.array_equal(part[0, :B].cpu().numpy().view(np.uint64), want_part.view(np.uint64)), (idx.numel(), B)
    assert bool(torch.isnan(part[0, B:]).all())                               # workgroups past B wrote nothing
    return got[0]


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 1024, 1025, 4097, 65600])
def test_statistics_are_bitwise_the_restatement(torch_cuda, M):
    """One and several partials (1 024 -> 1, 1 025 -> 2, 4 097 -> 5 workgroups), the cap of 64 workgroups with a second round
    (65 600 = 4 x 16 384 + 64), tails that are no multiple of 64 or 256."""
    torch = torch_cuda
    assert K1 * N1 == 66000
    pol, ppo, b = _stats_setup(torch)
    g = torch.Generator(device=DEV).manual_seed(M)
    row = _check_stats(torch, ppo, b, torch.randperm(K1 * N1, device=DEV, generator=g)[:M])
    if M == 1:
        assert row.tolist()[1:] == [np.float32(EPS), np.float32(1.0) / np.float32(EPS), 0.0]    # one sample: var = 0


def test_statistics_skip_indices_out_of_range(torch_cuda):
    torch = torch_cuda
    pol, ppo, b = _stats_setup(torch)
    n, M = K1 * N1, 4097
    g = torch.Generator(device=DEV).manual_seed(77)
    idx = torch.randperm(n, device=DEV, generator=g)[:M].clone()
    bad = torch.rand(M, device=DEV, generator=g) < 0.05
    beyond = torch.rand(M, device=DEV, generator=g) < 0.5
    idx[bad & beyond] += n                                                   # past the batch
    idx[bad & ~beyond] = -1 - idx[bad & ~beyond]                             # negative
    assert 100 < int(bad.sum()) < 350 and int((idx < 0).sum()) > 0 and int((idx >= n).sum()) > 0
    inside = _check_stats(torch, ppo, b, idx)
    everything = _check_stats(torch, ppo, b, idx.clamp(0, n - 1))
    assert not torch.equal(inside, everything)                               # the skipped samples would have counted
    none = _check_stats(torch, ppo, b, torch.full((300,), n, device=DEV, dtype=torch.int64))
    assert none.tolist() == [0.0, 1.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the wiring: the gradient kernel reads exactly those four floats
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [65, 1025])
@pytest.mark.parametrize("split", [False, True], ids=["shared", "split"])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_gradient_reads_the_minibatch_statistics_bitwise(torch_cuda, ext, split, M):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    D, H, L, A = 22, 32, 2, 3
    _, pol = (split_policy if split else actor_critic_policy)(torch, D, H, L, "tanh", A, seed=3)
    b = synthetic_batch(torch, pol, 8, 500, 9)
    if not ext:
        del b["logp_all"]
    terms = EXT_TERMS if ext else {}
    env = _env(D)
    g = torch.Generator(device=DEV).manual_seed(M)
    idx = torch.randperm(4000, device=DEV, generator=g)[:M]
    mine = NativePPO(pol, env, adv_norm="minibatch", **terms)
    mine.gae(b)
    g_mb, s_mb = mine.grad(b, idx, stats=True)
    row = mine.minibatch_adv_stats()[0].clone()
    assert env.adv_norm() == (1, 1)
    batch = NativePPO(pol, env, **terms)
    batch.gae(b)
    assert torch.equal(batch.adv_stats(), mine.adv_stats()) and not torch.equal(batch.adv_stats(), row[:3])
    g_b, _ = batch.grad(b, idx, stats=True)
    assert env.adv_norm() == (0, 0) and not torch.equal(g_b, g_mb)           # batch mode normalises otherwise
    batch.workspace[:16].view(torch.float32).copy_(row)                      # ... until its workspace holds the minibatch's four floats
    g_w, s_w = batch.grad(b, idx, stats=True)
    assert torch.equal(g_w, g_mb) and torch.equal(s_w, s_mb) and s_mb.numel() == (8 if ext else 4)
    assert bool(torch.isfinite(g_mb).all()) and float(g_mb.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. against autograd
# ------------------------------------------------------------------------------------------------------------------------------------
def _minibatch_advn(torch, adv, idx, dtype):
    """The whole batch's advantages normalised by minibatch idx's own torch mean / unbiased std, in dtype (one sample: std 0)."""
    a = adv.reshape(-1).to(dtype)
    sub = a[idx]
    std = sub.std() if idx.numel() > 1 else sub.new_zeros(())
    return (a - sub.mean()) / (std + EPS)


@pytest.mark.parametrize("H,L,act,A", [(16, 1, "relu", 2), (64, 2, "tanh", 3), (128, 2, "relu", 4)])
def test_grad_matches_autograd_with_the_minibatch_rule(torch_cuda, H, L, act, A):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    D = 22
    _, pol = actor_critic_policy(torch, D, H, L, act, A, seed=H + L + A)
    b = synthetic_batch_logp_noise(torch, pol, 8, 500, H)
    ppo = NativePPO(pol, _env(D), adv_norm="minibatch")
    ppo.gae(b)
    g = torch.Generator(device=DEV).manual_seed(5)
    perm = torch.randperm(4000, device=DEV, generator=g)
    for M in (2, 63, 65, 3000):
        idx = perm[:M]
        mine, st = ppo.grad(b, idx, stats=True)
        assert torch.equal(mine, ppo.grad(b, idx)), M
        r64, _ = ref_grad(torch, pol, b, idx, _minibatch_advn(torch, b["adv"], idx, torch.float64), torch.float64)
        r32, terms32 = ref_grad(torch, pol, b, idx, _minibatch_advn(torch, b["adv"], idx, torch.float32), torch.float32)
        check_per_tensor(torch, pol, mine, r64, r32, (H, L, act, A, M), verbose=True)
        for got, want in zip(st.tolist(), terms32):
            assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, (M, st.tolist(), terms32)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. whole updates
# ------------------------------------------------------------------------------------------------------------------------------------
def _ref_update(torch, pol, b, perm, minibatches, dtype):
    """ppo_reference.ref_update's loop with the per-minibatch rule: (parameters, Adam's exp_avg, exp_avg_sq)."""
    p = pol.params.detach().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=3e-4)
    for row in perm:
        for idx in row.chunk(minibatches):
            advn = _minibatch_advn(torch, b["adv"], idx, dtype)
            loss = plain_loss(torch, p, pol.offsets, pol.n_hidden_layers, pol.activation, *minibatch(torch, pol, b, idx, advn, dtype))[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


@pytest.mark.parametrize("K,envs,minibatches,chunks", [(8, 125, 3, [334, 334, 332]), (2, 5, 6, [2, 2, 2, 2, 2]), (1, 7, 3, [3, 3, 1])])
def test_whole_update_against_f64_and_run_to_run(torch_cuda, K, envs, minibatches, chunks):
    """The last chunk of the third case is ONE sample: its normalised advantage is 0 (var = 0), in the reference too."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    epochs = 2
    env = _default_env(envs)
    _, pol = actor_critic_policy(torch, env.states_history, 64, 2, "tanh", 3, seed=K + envs)
    env.reset_tensor()
    b = dict(env.rollout_policy(pol, K, seed=envs))
    n = K * envs
    g = torch.Generator(device=DEV).manual_seed(minibatches)
    perm = torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(epochs)])
    assert [len(c) for c in perm[0].chunk(minibatches)] == chunks
    p0 = pol.params.detach().clone()
    P = p0.numel()
    runs = []
    for _ in range(2):
        pol.params.copy_(p0)
        ppo = NativePPO(pol, env, adv_norm="minibatch")
        ppo.gae(b)
        st = ppo.update(b, perm, epochs, minibatches, stats=True)
        assert st.shape == (epochs * len(chunks), 4) and bool(torch.isfinite(st).all()) and ppo.step == epochs * len(chunks)
        runs.append((pol.params.detach().clone(), ppo.adam_mv.clone(), st.clone(), ppo.minibatch_adv_stats().clone()))
    for x, y in zip(*runs):
        assert torch.equal(x, y)                                             # identical bits run to run
    mine, mv, _, last = runs[0]
    # the scratch holds the LAST minibatch's statistics
    from ship_sim_gym_amd.ppo import minibatch_adv_reference
    idx = perm[-1].chunk(minibatches)[-1]
    want = minibatch_adv_reference(b["adv"].reshape(-1)[idx].cpu().numpy(), np.ones(idx.numel(), dtype=bool), EPS)
    assert np.array_equal(_bits(last[0]), want.view(np.uint32))
    pol.params.copy_(p0)
    r64, m64, v64 = _ref_update(torch, pol, b, perm, minibatches, torch.float64)
    r32, m32, v32 = _ref_update(torch, pol, b, perm, minibatches, torch.float32)
    check_per_tensor(torch, pol, mine, r64, r32, ("update", n, minibatches), verbose=True)
    check_per_tensor(torch, pol, mv[:P], m64, m32, ("exp_avg", n, minibatches), verbose=True)
    check_per_tensor(torch, pol, mv[P:], v64, v32, ("exp_avg_sq", n, minibatches), verbose=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. off is off
# ------------------------------------------------------------------------------------------------------------------------------------
def test_batch_mode_is_untouched_by_a_minibatch_mode_neighbour(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    n_env, K = 125, 8
    fresh, used = ShipVecEnv(n_env, n_maps=64), ShipVecEnv(n_env, n_maps=64)
    try:
        _, pol_a = actor_critic_policy(torch, fresh.states_history, 64, 2, "tanh", 3, seed=4)
        _, pol_b = actor_critic_policy(torch, fresh.states_history, 64, 2, "tanh", 3, seed=4)
        _, pol_s = actor_critic_policy(torch, fresh.states_history, 64, 2, "tanh", 3, seed=4)      # the scratch copy
        assert torch.equal(pol_a.params, pol_b.params)
        fresh.reset_tensor()
        b = dict(fresh.rollout_policy(pol_a, K, seed=3))
        g = torch.Generator(device=DEV).manual_seed(2)
        perm = torch.stack([torch.randperm(K * n_env, device=DEV, generator=g) for _ in range(2)])
        plain = NativePPO(pol_a, fresh)                                      # a handle that never bound anything
        plain.gae(b)
        s_a = plain.update(b, perm, 2, 3, stats=True)
        assert fresh.adv_norm() == (N.ADV_NORM_BATCH, 0)
        neighbour = NativePPO(pol_s, used, adv_norm="minibatch")
        neighbour.gae(b)
        batch_stats = neighbour.adv_stats().clone()
        s_n = neighbour.update(b, perm, 2, 3, stats=True)
        assert used.adv_norm() == (N.ADV_NORM_MINIBATCH, 1)
        assert torch.equal(neighbour.adv_stats(), batch_stats)               # the batch statistics survive a minibatch-mode update
        assert torch.equal(batch_stats, plain.adv_stats())
        assert not torch.equal(pol_s.params, pol_a.params) and not torch.equal(s_n, s_a)           # (the mode does change the update)
        used.set_adv_norm(N.ADV_NORM_BATCH)
        assert used.adv_norm() == (N.ADV_NORM_BATCH, 0)
        after = NativePPO(pol_b, used)
        after.gae(b)
        s_b = after.update(b, perm, 2, 3, stats=True)
        assert torch.equal(pol_a.params, pol_b.params) and torch.equal(plain.adam_mv, after.adam_mv) and torch.equal(s_a, s_b)
        # two trainers on one env: each call binds its own mode
        neighbour.grad(b, perm[0, :65])
        assert used.adv_norm() == (N.ADV_NORM_MINIBATCH, 1)
        after.grad(b, perm[0, :65])
        assert used.adv_norm() == (N.ADV_NORM_BATCH, 0)
    finally:
        fresh.close()
        used.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. populations: every member is NativePPO(adv_norm="minibatch") on its shard, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
K6 = 8
EXT4 = {"vf_clip": [10.0, 0.05, 0.0, 0.2], "max_grad_norm": [0.0, 0.03, 0.0, 0.5], "kl_coef": [1.0, 0.0, 0.0, 0.5],
        "kl_target": [1e-4, 0.0, 0.0, 10.0]}     # RLlib's loss; PPO2's; everything off; everything on


def _pop_setup(torch, sizes):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    sizes = list(sizes)
    sliced = len(set(sizes)) > 1

    def make_env(n, base):
        env = ShipVecEnv(n, n_maps=64, env_id_base=base)
        if sliced and n == sum(sizes):
            env.set_population_slices(sizes)
        return env

    def make():
        P = len(sizes)
        setup = shard_rollouts(torch, make_env, lambda D: [actor_critic_policy(torch, D, seed=100 + m)[1] for m in range(P)], sizes, K6, 7)
        env, pop, b, shards, refs, sbs = setup
        age(torch, b, sbs, sizes, pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(sum(sizes)), True)
        return setup
    return cached(tuple(sizes), make)


def _check_population(torch, sizes, ext, epochs, minibatches):
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    env, pop, b, shards, refs, sbs = _pop_setup(torch, sizes)
    P = len(sizes)
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    hp = _hp(P)
    ep = epochs if isinstance(epochs, list) else [epochs] * P
    mbs = minibatches if isinstance(minibatches, list) else [minibatches] * P
    samples = [K6 * s for s in sizes]
    steps = [e * chunk_split(s, c)[1] for e, c, s in zip(ep, mbs, samples)]
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, adv_norm="minibatch", **hp, **ext)
        ppo.gae(b)
        batch_stats = ppo.adv_stats().clone()
        g = torch.Generator(device=DEV).manual_seed(11)
        if len(set(sizes)) > 1:
            perm = perms_per_member(torch, g, max(ep), samples)
        else:
            perm = stacked_perms(torch, g, P, max(ep), samples[0])
        st = ppo.update(b, perm, epochs, minibatches, stats=True)
        assert env.adv_norm() == (1, P) and st.shape[:2] == (P, max(steps)) and bool(torch.isfinite(st).all())
        assert torch.equal(ppo.adv_stats(), batch_stats)
        rows = ppo.minibatch_adv_stats().clone()
        assert rows.shape == (P, 4) and bool(torch.isfinite(rows).all())
        for m in range(P):
            ref = NativePPO(refs[m], shards[m], lr=hp["lr"][m], betas=(hp["beta1"][m], 0.999), clip=hp["clip"][m], ent_coef=hp["ent_coef"][m],
                            adv_norm="minibatch", **{k: v[m] for k, v in ext.items()})
            ref.gae(sbs[m], 0.99, hp["lam"][m])
            r_st = ref.update(sbs[m], perm[m][:ep[m]].contiguous(), ep[m], mbs[m], stats=True)
            assert r_st.shape[0] == steps[m], m
            assert torch.equal(pop.params[m], refs[m].params), (m, "params")
            assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (m, "moments")
            assert torch.equal(st[m, :steps[m], :r_st.shape[1]], r_st), (m, "stats")
            # the member's row is its OWN last minibatch's, also when later launches of the call served other members only
            assert torch.equal(rows[m], ref.minibatch_adv_stats()[0]), (m, rows[m].tolist(), ref.minibatch_adv_stats().tolist())
            assert torch.equal(ppo.kl_coef[m:m + 1], ref.kl_coef), (m, "coefficient")
        assert not torch.equal(pop.params, saved[0])
        return ppo
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)


def test_population_update_is_each_members_own(torch_cuda):
    ppo = _check_population(torch_cuda, [64] * 4, {}, 2, 4)                   # ssg_pop_update
    assert not ppo.extended() and not ppo.diverged()


def test_population_ext_update_is_each_members_own(torch_cuda):
    assert _check_population(torch_cuda, [64] * 4, EXT4, 2, 4).extended()     # ssg_pop_update_ext


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_population_on_schedules_keeps_idle_members_rows(torch_cuda, ext):
    """512 samples per member; steps 1 / 6 / 15 / 32: member 0 is idle from the second launch on, member 3 alone in the last 17."""
    ppo = _check_population(torch_cuda, [64] * 4, EXT4 if ext else {}, [1, 2, 3, 4], [1, 3, 5, 8])
    assert ppo.member_steps == [1, 6, 15, 32]


def test_population_on_unequal_slices_is_each_members_own(torch_cuda):
    ppo = _check_population(torch_cuda, [64, 128, 192, 256], {}, 2, 4)
    assert ppo.member_steps == [8, 8, 8, 8]


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. more members than the bound scratch serves
# ------------------------------------------------------------------------------------------------------------------------------------
def test_member_count_above_the_bound_one_is_refused_and_nothing_runs(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import adv_norm_scratch
    env, pop, b, shards, refs, sbs = _pop_setup(torch, [64] * 4)
    b = dict(b)
    ppo = PopulationPPO(pop, env, adv_norm="minibatch")
    ppo.gae(b)
    small = adv_norm_scratch(2, pop.device)
    ppo._bind_adv_norm = lambda: env.set_adv_norm(N.ADV_NORM_MINIBATCH, small, 2)   # a scratch for two members under a call for four
    perm = stacked_perms(torch, torch.Generator(device=DEV).manual_seed(1), 4, 4, K6 * 64)
    before = pop.params.clone(), ppo.adam_mv.clone()
    try:
        for epochs, minibatches in ((2, 4), ([1, 2, 3, 4], [1, 3, 5, 8])):    # ssg_pop_update, ssg_pop_update_sched
            with pytest.raises(N.ShipSimError, match="n_members"):
                ppo.update(b, perm[:, :2].contiguous() if epochs == 2 else perm, epochs, minibatches)
            torch.cuda.synchronize()
            assert torch.equal(pop.params, before[0]) and torch.equal(ppo.adam_mv, before[1]) and ppo.member_steps == [0] * 4
        assert env.adv_norm() == (N.ADV_NORM_MINIBATCH, 2)
        del ppo._bind_adv_norm                                               # its own scratch again: the same call runs
        ppo.update(b, perm[:, :2].contiguous(), 2, 4)
        assert not torch.equal(pop.params, before[0])
    finally:
        pop.params.copy_(before[0])
        env.set_adv_norm(N.ADV_NORM_BATCH)


# ------------------------------------------------------------------------------------------------------------------------------------
# 8. the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update", ["native", "torch"])
def test_ppo_torch_trains_with_minibatch_normalisation(torch_cuda, update):
    torch = torch_cuda
    mod = load_script("train/ppo_torch.py")
    kw = dict(envs=256, updates=1, horizon=8, mode="native", update=update, return_details=True, log=lambda s: None)
    _, det = mod.train(adv_norm="minibatch", **kw)
    assert all(bool(torch.isfinite(p).all()) for p in det["params"])
    _, base = mod.train(**kw)
    assert any(not torch.equal(p, q) for p, q in zip(det["params"], base["params"]))            # the flag reaches the update
