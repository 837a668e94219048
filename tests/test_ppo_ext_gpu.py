"""GPU checks of the extended PPO update (ship_sim_gym_amd/ppo.py; ssg_ppo_dist, ssg_ppo_grad_ext, ssg_ppo_update_ext): with every term
off it is the existing path bit for bit; ssg_ppo_dist reproduces the rollout's logp; the gradient of the loss with the value clip and
the KL penalty against an f64 autograd reference over every branch; gradient-norm clipping against clip_grad_norm_ + Adam; a whole
update with the three terms on against the f64 reference of the same update, the coefficient's adaptation bitwise, and run to run."""
import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _policy, check_per_tensor as _check_per_tensor, kl_adapt as _adapt, \
    ref_grad as _ref_grad, ref_update

pytestmark = pytest.mark.gpu

VF_CLIP, KL_COEF = 0.05, 1.0
TERMS = dict(vf_clip=VF_CLIP, kl_coef=KL_COEF)


def _vec(n):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64)


_BATCHES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_cached_envs():
    yield
    for entry in _BATCHES.values():
        entry[0].close()
    _BATCHES.clear()


def _batch_for(torch, H, L, act, A, n=500, K=8):
    """(env, pol, b, advn) for a shape, computed once per module: a rollout, GAE, then the acting policy made an OLDER one so that
    every branch of the extended loss occurs — logp_all_old = log_softmax(logp_all + 0.5*randn) with logp gathered from it, and
    v_old = val + U(-0.2, 0.2) against vf_clip = 0.05."""
    key = (H, L, act, A, n, K)
    if key in _BATCHES:
        return _BATCHES[key]
    from ship_sim_gym_amd.ppo import NativePPO
    seed = H + L + A
    env = _vec(n)
    _, pol = _policy(torch, env.states_history, H, L, act, A, seed=seed)
    env.reset_tensor()
    b = dict(env.rollout_policy(pol, K, seed=seed + 7))
    ppo = NativePPO(pol, env)
    ppo.gae(b)
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    la = ppo.dist(b)
    old = torch.log_softmax(la[..., :A] + 0.5 * torch.randn(la[..., :A].shape, generator=g, device="cuda:0"), -1)
    b["logp_all"] = torch.zeros_like(la)
    b["logp_all"][..., :A] = old
    b["logp"] = old.gather(-1, b["act"].long().unsqueeze(-1)).squeeze(-1).contiguous()
    b["val"] = (b["val"] + (torch.rand(b["val"].shape, generator=g, device="cuda:0") - 0.5) * 0.4).contiguous()
    st = ppo.adv_stats().clone()
    advn = (b["adv"].reshape(-1) - st[0]) / st[1]
    _BATCHES[key] = (env, pol, b, advn, st)
    return _BATCHES[key]


def _ppo(torch, pol, env, st, n, M, **kw):
    """A fresh NativePPO whose workspace holds the advantage statistics st (what gae() left for the batch)."""
    from ship_sim_gym_amd.ppo import NativePPO
    ppo = NativePPO(pol, env, **kw)
    ppo._ws(n, M)
    ppo.workspace[:12].view(torch.float32).copy_(st)
    return ppo


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. off is the existing path
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,L,act,A", [(64, 2, "tanh", 3), (16, 1, "relu", 2)])
def test_everything_off_is_the_existing_path_bitwise(torch_cuda, H, L, act, A):
    torch = torch_cuda
    env, pol, b, advn, st = _batch_for(torch, H, L, act, A)
    n = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    perm = torch.stack([torch.randperm(n, device="cuda:0", generator=g) for _ in range(2)])
    p0 = pol.params.detach().clone()
    try:
        plain, ext = _ppo(torch, pol, env, st, n, n), _ppo(torch, pol, env, st, n, n)
        ext.force_ext = True
        assert not plain.extended() and ext.extended()
        for M in (1, 65, 3000):
            g0, s0 = plain.grad(b, perm[0, :M], stats=True)
            g1, s1 = ext.grad(b, perm[0, :M], stats=True)
            assert s0.shape == (4,) and s1.shape == (8,)
            assert torch.equal(g0, g1) and torch.equal(s0, s1[:4]), M
            assert s1[4:].tolist() == [0.0, 0.0, 0.0, 0.0]
        s0 = plain.update(b, perm, 2, 4, stats=True)
        after = pol.params.detach().clone()
        pol.params.copy_(p0)
        s1 = ext.update(b, perm, 2, 4, stats=True)
        assert s0.shape == (8, 4) and s1.shape == (8, 8)
        assert torch.equal(pol.params, after) and torch.equal(plain.adam_mv, ext.adam_mv) and torch.equal(s0, s1[:, :4])
        assert plain.step == ext.step == 8 and float(ext.kl_coef) == 0.0
    finally:
        pol.params.copy_(p0)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. ssg_ppo_dist
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_dist_reproduces_the_rollouts_logp_bitwise(torch_cuda, n, A):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec(n)
    _, pol = _policy(torch, env.states_history, 64, 2, "tanh", A, seed=n + A)
    env.reset_tensor()
    b = dict(env.rollout_policy(pol, 3, seed=n))
    la = NativePPO(pol, env).dist(b)
    assert la.shape == (3, n, 4) and la.dtype == torch.float32 and b["logp_all"] is la
    assert torch.equal(la.gather(-1, b["act"].long().unsqueeze(-1)).squeeze(-1), b["logp"])
    assert bool((la[..., A:] == 0).all())
    assert float(torch.logsumexp(la[..., :A].double(), -1).abs().max()) <= 1e-6
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the gradient against f64 autograd
# ------------------------------------------------------------------------------------------------------------------------------------
def _grad_case(torch, H, L, act, A, n, K, sizes, need_branches):
    env, pol, b, advn, st = _batch_for(torch, H, L, act, A, n, K)
    total = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    perm = torch.randperm(total, device="cuda:0", generator=g)
    ppo = _ppo(torch, pol, env, st, total, max(sizes), vf_clip=VF_CLIP, kl_coef=KL_COEF, max_grad_norm=0.5)
    for M in sizes:
        idx = perm[:M]
        mine, stats = ppo.grad(b, idx, stats=True)
        again = ppo.grad(b, idx)
        assert torch.equal(mine, again), M                              # bitwise run to run
        r64, terms64, (dv, l1, l2) = _ref_grad(torch, pol, b, idx, advn, torch.float64, **TERMS)
        r32, terms32, _ = _ref_grad(torch, pol, b, idx, advn, torch.float32, **TERMS)
        if M in need_branches:  # on the f64 reference: every branch of the value clip and of its max occurs, and the KL term is alive
            below, inside, above = dv < -VF_CLIP, dv.abs() <= VF_CLIP, dv > VF_CLIP
            assert int(below.sum()) > 0 and int(inside.sum()) > 0 and int(above.sum()) > 0
            clipped = below | above
            assert int((clipped & (l1 > l2)).sum()) > 0 and int((clipped & (l2 > l1)).sum()) > 0
            assert terms64[4] > 0.0
        _check_per_tensor(torch, pol, mine, r64, r32, (H, L, act, A, M))
        got = stats.tolist()
        print("M=%d stats %s f32 reference %s norm %.9g" % (M, got, terms32, float(r32.norm())))
        for k in range(5):                                              # pg, VL, entropy, clip fraction, KL
            assert abs(got[k] - terms32[k]) <= 1e-5 * abs(terms32[k]) + 1e-6, (k, got, terms32)
        want_norm = float(r32.norm())
        assert abs(got[5] - want_norm) <= 1e-5 * abs(want_norm) + 1e-6, (got[5], want_norm)
        assert got[6] == KL_COEF and got[7] == 0.0


@pytest.mark.parametrize("H,L,act,A", [(16, 1, "relu", 2), (64, 2, "tanh", 3), (128, 2, "relu", 4)])
def test_ext_grad_matches_f64_autograd(torch_cuda, H, L, act, A):
    _grad_case(torch_cuda, H, L, act, A, 500, 8, [1, 63, 65, 3000], {3000})


def test_ext_grad_over_more_than_512_tiles(torch_cuda):
    """33 000 samples are 516 tiles: more than the 512 workgroups, so workgroups take a second tile."""
    _grad_case(torch_cuda, 64, 2, "tanh", 3, 4125, 8, [33000], {33000})


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. gradient-norm clipping
# ------------------------------------------------------------------------------------------------------------------------------------
def test_grad_norm_clip_is_clip_grad_norm_then_adam(torch_cuda):
    torch = torch_cuda
    env, pol, b, advn, st = _batch_for(torch, 64, 2, "tanh", 3)
    n = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(9)
    perm = torch.randperm(n, device="cuda:0", generator=g).unsqueeze(0)
    p0 = pol.params.detach().clone()
    kw = dict(vf_clip=VF_CLIP, kl_coef=KL_COEF)
    try:
        # the norm of the unclipped gradient (stats[5] of a run whose bound is out of reach)
        norm = float(_ppo(torch, pol, env, st, n, n, max_grad_norm=1e30, **kw).grad(b, perm[0], stats=True)[1][5])
        assert norm > 0.0
        free = _ppo(torch, pol, env, st, n, n, **kw)
        s_free = free.update(b, perm, 1, 1, stats=True)
        p_free = pol.params.detach().clone()
        assert float(s_free[0, 5]) == 0.0
        pol.params.copy_(p0)
        loose = _ppo(torch, pol, env, st, n, n, max_grad_norm=2 * norm, **kw)
        s_loose = loose.update(b, perm, 1, 1, stats=True)
        assert torch.equal(pol.params, p_free) and torch.equal(loose.adam_mv, free.adam_mv)     # coef = 1: bitwise the unclipped update
        assert torch.equal(s_loose[0, :5], s_free[0, :5]) and float(s_loose[0, 5]) == norm
        pol.params.copy_(p0)
        tight = _ppo(torch, pol, env, st, n, n, max_grad_norm=0.5 * norm, **kw)
        s_tight = tight.update(b, perm, 1, 1, stats=True)
        assert float(s_tight[0, 5]) == norm
        mine = pol.params.detach().clone()
        pol.params.copy_(p0)
        r64 = ref_update(torch, pol, b, advn, perm, 1, torch.float64, max_grad_norm=0.5 * norm, **TERMS)[0]
        r32 = ref_update(torch, pol, b, advn, perm, 1, torch.float32, max_grad_norm=0.5 * norm, **TERMS)[0]
        _check_per_tensor(torch, pol, mine, r64, r32, "clipped step")
        # the moments hold the CLIPPED gradient: m = 0.1 * g * coef after the first step
        g_raw = _ppo(torch, pol, env, st, n, n, **kw).grad(b, perm[0])
        coef = np.float32(min(1.0, np.float32(0.5 * norm) / (np.float32(norm) + np.float32(1e-6))))
        assert 0.49 < float(coef) < 0.51
        torch.testing.assert_close(tight.adam_mv[: mine.numel()], g_raw * float(coef) * 0.1, rtol=1e-5, atol=1e-9)
    finally:
        pol.params.copy_(p0)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. a whole update with the three terms on
# ------------------------------------------------------------------------------------------------------------------------------------
def _ref_update(torch, pol, b, advn, perm, epochs, minibatches, dtype, max_norm, kl_coef, kl_target):
    """(parameters, the adapted coefficient, the last epoch's mean KL) of the reference update with the three terms on."""
    p, _, kls = ref_update(torch, pol, b, advn, perm[:epochs], minibatches, dtype, max_grad_norm=max_norm, vf_clip=VF_CLIP, kl_coef=kl_coef)
    kls = kls[-(len(kls) // epochs):]
    mean = sum(kls) / len(kls)
    if kl_target > 0:
        kl_coef = kl_coef * 1.5 if mean > 2 * kl_target else (kl_coef * 0.5 if mean < 0.5 * kl_target else kl_coef)
    return p, kl_coef, mean


def test_whole_ext_update_against_f64_adapts_the_coefficient_and_repeats(torch_cuda):
    """The targets here are a factor of 4 from the mean KL; tests/test_kl_adapt_gpu.py puts them AT the decision's boundaries."""
    torch = torch_cuda
    env, pol, b, advn, st = _batch_for(torch, 64, 2, "tanh", 3, n=2048, K=8)
    n = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(11)
    perm = torch.stack([torch.randperm(n, device="cuda:0", generator=g) for _ in range(2)])
    p0 = pol.params.detach().clone()
    # (this batch's minibatch gradients have norms of 0.02 .. 0.09: a bound of 0.05 clips some steps and leaves others alone)
    max_norm = 0.05
    kw = dict(vf_clip=VF_CLIP, max_grad_norm=max_norm, kl_coef=KL_COEF)
    try:
        # a first run without adaptation: the mean KL of the last epoch, from which the two targets are derived
        probe = _ppo(torch, pol, env, st, n, n // 4, **kw)
        s_probe = probe.update(b, perm, 2, 4, stats=True)
        assert s_probe.shape == (8, 8) and bool(torch.isfinite(s_probe).all()) and float(probe.kl_coef) == KL_COEF
        mean_kl = float(s_probe[-4:, 4].mean())
        print("mean KL of the last epoch: %.9g; gradient norms %s" % (mean_kl, s_probe[:, 5].tolist()))
        assert mean_kl > 0.0 and bool((s_probe[:, 5] > max_norm).any()) and bool((s_probe[:, 5] < max_norm).any())
        first = pol.params.detach().clone()
        for target, factor in ((mean_kl / 4.0, 1.5), (mean_kl * 4.0, 0.5)):  # lands above 2*target, then below 0.5*target
            pol.params.copy_(p0)
            r64, c64, m64 = _ref_update(torch, pol, b, advn, perm, 2, 4, torch.float64, max_norm, KL_COEF, target)
            r32, c32, _ = _ref_update(torch, pol, b, advn, perm, 2, 4, torch.float32, max_norm, KL_COEF, target)
            ppo = _ppo(torch, pol, env, st, n, n // 4, kl_target=target, **kw)
            stats = ppo.update(b, perm, 2, 4, stats=True)
            assert torch.equal(stats, s_probe) and torch.equal(pol.params, first)   # the target changes nothing but the coefficient
            assert bool((stats[:, 6] == KL_COEF).all())                      # the coefficient every minibatch USED
            want = _adapt(KL_COEF, stats[-4:, 4].cpu().numpy(), target)
            got = ppo.kl_coef.cpu().numpy()[0]
            assert got.dtype == np.float32 and got == want == np.float32(KL_COEF * factor), (got, want, factor)
            _check_per_tensor(torch, pol, pol.params.detach(), r64, r32, "ext update")
            assert c64 == c32 == float(got) and abs(m64 - mean_kl) <= 1e-4 * mean_kl
            # a second update uses the adapted coefficient
            s2 = ppo.update(b, perm[:1], 1, 4, stats=True)
            assert bool((s2[:, 6] == float(got)).all())
    finally:
        pol.params.copy_(p0)


@pytest.mark.parametrize("K,envs,minibatches,chunks", [(8, 125, 3, 3), (2, 5, 6, 5)])
def test_whole_ext_update_at_uneven_chunkings(torch_cuda, K, envs, minibatches, chunks):
    """The shapes of the plain path's test_update_uneven_chunks_and_continuity with the three terms on: a last chunk shorter than the
    others (334, 334, 332), then fewer chunks than asked (5 of 2 samples).  Stats rows, Adam steps and the adaptation count CHUNKS.
    (The target is a factor of 4 from the mean KL; tests/test_kl_adapt_gpu.py has these chunkings AT the decision's boundaries.)"""
    torch = torch_cuda
    epochs = 2
    env, pol, b, advn, st = _batch_for(torch, 64, 2, "tanh", 3, n=envs, K=K)
    n = b["act"].numel()
    assert n == K * envs and len(torch.arange(n).chunk(minibatches)) == chunks
    g = torch.Generator(device="cuda:0").manual_seed(minibatches)
    perm = torch.stack([torch.randperm(n, device="cuda:0", generator=g) for _ in range(epochs)])
    assert [len(c) for c in perm[0].chunk(minibatches)] == [-(-n // minibatches)] * (chunks - 1) + [n - (chunks - 1) * -(-n // minibatches)]
    p0 = pol.params.detach().clone()
    max_norm = 0.05
    kw = dict(vf_clip=VF_CLIP, max_grad_norm=max_norm, kl_coef=KL_COEF)
    M = -(-n // minibatches)
    try:
        # a first run without adaptation: the mean KL of the last epoch, a quarter of which is a target the coefficient grows at
        probe = _ppo(torch, pol, env, st, n, M, **kw)
        s_probe = probe.update(b, perm, epochs, minibatches, stats=True)
        assert s_probe.shape == (epochs * chunks, 8) and bool(torch.isfinite(s_probe).all()) and float(probe.kl_coef) == KL_COEF
        mean_kl = float(s_probe[-chunks:, 4].mean())
        print("mean KL of the last epoch: %.9g; gradient norms %s" % (mean_kl, s_probe[:, 5].tolist()))
        assert mean_kl > 0.0
        target = mean_kl / 4.0
        pol.params.copy_(p0)
        r64, c64, m64 = _ref_update(torch, pol, b, advn, perm, epochs, minibatches, torch.float64, max_norm, KL_COEF, target)
        r32, c32, _ = _ref_update(torch, pol, b, advn, perm, epochs, minibatches, torch.float32, max_norm, KL_COEF, target)
        ppo = _ppo(torch, pol, env, st, n, M, kl_target=target, **kw)
        stats = ppo.update(b, perm, epochs, minibatches, stats=True)
        assert stats.shape == (epochs * chunks, 8) and torch.equal(stats, s_probe)
        assert ppo.step == epochs * chunks
        assert bool((stats[:, 6] == KL_COEF).all()) and bool((stats[:, 5] > 0).all()) and bool((stats[:, 7] == 0).all())
        want = _adapt(KL_COEF, stats[-chunks:, 4].cpu().numpy(), target)
        got = ppo.kl_coef.cpu().numpy()[0]
        assert got.dtype == np.float32 and got == want == np.float32(KL_COEF * 1.5), (got, want)
        _check_per_tensor(torch, pol, pol.params.detach(), r64, r32, ("ext update", n, minibatches))
        assert c64 == c32 == float(got) and abs(m64 - mean_kl) <= 1e-4 * mean_kl
    finally:
        pol.params.copy_(p0)
