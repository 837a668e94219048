"""GPU checks of the device PPO update (ssg_ppo_*) and the policy forward (ssg_policy_act / ssg_rollout_policy) over the domain the
API accepts, not only the shapes train/ppo_torch.py uses: obs_dim 7..176 (not multiples of 4 or 16, past 64, the maximum), hidden
widths whose tile count is not a multiple of the 4 waves, minibatches from 1 sample to several tiles per workgroup (duplicates
included), a workspace full of NaN, non-default hyper-parameters, GAE at odd shapes and discounts, uneven torch.chunk splits over
two consecutive updates, and Adam's moments against torch for betas on both sides of lerp's 0.5 switch.

The batches are synthetic (every extreme under control): obs f32 [K, N, D] mixes rows at the real scale (obs / 600), reset rows
(obs = -1) and ~5 % of rows scaled x50 (tanh saturates to exactly +-1 in f32); logp_old = the current policy's logp + U(-0.4, 0.4),
so that ratios are clipped on both sides and min() ties inside the range.  References are torch autograd in f64 (and f32, for the
bound) on the same packed parameters; the acceptance rule is check_per_tensor's: max|mine - f64| <= 4 max|torch f32 - f64| +
1e-6 max|f64| per packed tensor."""
import itertools

import numpy as np
import pytest

from gpu_support import DEV, HIST_BEAMS, check_near_rows, env_config as _env_config, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, assert_same_rollout, check_per_tensor, forward, ref_grad, ref_update, stepwise_rollout, \
    synthetic_batch_logp_noise as _synthetic, torch_gae

pytestmark = pytest.mark.gpu


def _vec(n, history, n_beams, n_maps=4):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=n_maps, n_beams=n_beams, env_config=_env_config(history))


@pytest.fixture(scope="module")
def envs(torch_cuda):
    """One 64-env handle per obs_dim (check_policy ties obs_dim to the handle; the PPO calls take their own K, N)."""
    made = {}

    def get(D):
        if D not in made:
            made[D] = _vec(64, *HIST_BEAMS[D])
            assert made[D].states_history == D
        return made[D]
    yield get
    for e in made.values():
        e.close()


def _ppo(torch, env, H, L, act, A, seed=0, **kw):
    from ship_sim_gym_amd.ppo import NativePPO
    _, pol = actor_critic_policy(torch, env.states_history, H, L, act, A, seed=seed)
    return pol, NativePPO(pol, env, **kw)


def _prepare(torch, pol, ppo, K, N, seed):
    """A synthetic batch after ppo.gae (the gradient reads the workspace statistics gae left), and its normalised advantages."""
    b = _synthetic(torch, pol, K, N, seed)
    ppo.gae(b)
    st = ppo.adv_stats()
    return b, (b["adv"].reshape(-1) - st[0]) / st[1]


def _check_grad(torch, pol, ppo, b, advn, idx, what, coefs=(0.2, 0.5, 0.01)):
    """grad() against f64 / f32 autograd (per packed tensor), its stats against f32, and bitwise run to run."""
    mine, st = ppo.grad(b, idx, stats=True)
    assert torch.equal(mine, ppo.grad(b, idx)), what
    kw = dict(zip(("clip", "vf_coef", "ent_coef"), coefs))
    r64, _ = ref_grad(torch, pol, b, idx, advn, torch.float64, **kw)
    r32, terms32 = ref_grad(torch, pol, b, idx, advn, torch.float32, **kw)
    check_per_tensor(torch, pol, mine, r64, r32, what)
    for got, want in zip(st.tolist(), terms32):
        assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, (what, st.tolist(), terms32)
    return mine, st


# ------------------------------------------------------------------------------------------------------------------------------------
# the gradient over (D, H, L, A, activation)
# ------------------------------------------------------------------------------------------------------------------------------------
def _shape_cases():
    """A covering design: every D meets every H; each (L, act, A) meets an odd H/16 (idle waves); (176, 128, L=2) is in."""
    combos = list(itertools.product((1, 2), ("tanh", "relu"), (2, 3, 4)))
    cases, odd = [], 0
    for i, (D, H) in enumerate(itertools.product(sorted(HIST_BEAMS), (16, 48, 80, 112, 128))):
        if (H // 16) % 2:
            L, act, A = combos[odd % len(combos)]
            odd += 1
        else:
            L, act, A = combos[(5 * i) % len(combos)]
        if (D, H) == (176, 128):
            L = 2                                              # the largest LDS footprint: 151 048 bytes
        cases.append((D, H, L, A, act))
    seen = {(L, act, A) for D, H, L, A, act in cases if (H // 16) % 2}
    assert seen == set(combos) and (176, 128, 2) in {c[:3] for c in cases}
    assert {(D, H) for D, H, *_ in cases} == set(itertools.product(HIST_BEAMS, (16, 48, 80, 112, 128)))
    return cases


SHAPES = _shape_cases()


def test_grad_shape_sweep(torch_cuda, envs):
    torch = torch_cuda
    for j, (D, H, L, A, act) in enumerate(SHAPES):
        pol, ppo = _ppo(torch, envs(D), H, L, act, A, seed=j)
        b, advn = _prepare(torch, pol, ppo, 4, 800, seed=100 + j)
        perm = torch.randperm(3200, device=DEV, generator=torch.Generator(device=DEV).manual_seed(j))
        _check_grad(torch, pol, ppo, b, advn, perm[:2500], (D, H, L, A, act))


def test_grad_on_real_rollouts_at_the_extreme_widths(torch_cuda):
    """D = 7 and D = 176 through the real data flow: rollout_policy, gae, grad."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    for D, H, L, A, act in ((7, 48, 2, 3, "tanh"), (176, 128, 2, 4, "relu")):
        env = _vec(1000, *HIST_BEAMS[D])
        _, pol = actor_critic_policy(torch, D, H, L, act, A, seed=D)
        env.reset_tensor()
        b = dict(env.rollout_policy(pol, 6, seed=D))
        ppo = NativePPO(pol, env)
        ppo.gae(b)
        g = torch.Generator(device=DEV).manual_seed(D)
        b["logp"] = (b["logp"] + (torch.rand(b["logp"].shape, generator=g, device=DEV) - 0.5) * 0.8).contiguous()
        st = ppo.adv_stats()
        advn = (b["adv"].reshape(-1) - st[0]) / st[1]
        _check_grad(torch, pol, ppo, b, advn, torch.randperm(6000, device=DEV, generator=g)[:4000], ("rollout", D, H))
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# minibatch sizes, duplicates, the workspace
# ------------------------------------------------------------------------------------------------------------------------------------
MB_SIZES = (1, 2, 63, 64, 65, 32768, 32769, 100003)


def test_grad_minibatch_sizes_and_duplicates(torch_cuda, envs):
    """One partial tile, an exact tile, a grid of exactly 512, 513 tiles (workgroup 0 takes two: the read-modify-write path) and 3-4
    tiles per workgroup; indices drawn with replacement, and all equal to the last sample (each occurrence counts once)."""
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(27), 80, 2, "tanh", 3, seed=27)
    b, advn = _prepare(torch, pol, ppo, 8, 16384, seed=27)
    n = b["act"].numel()
    g = torch.Generator(device=DEV).manual_seed(1)
    perm = torch.randperm(n, device=DEV, generator=g)
    for M in MB_SIZES:
        _check_grad(torch, pol, ppo, b, advn, perm[:M], ("distinct", M))
    for M in (65, 32769, 100003):
        _check_grad(torch, pol, ppo, b, advn, torch.randint(0, n, (M,), device=DEV, generator=g), ("with replacement", M))
    for M in (1, 64, 65, 32769):
        _check_grad(torch, pol, ppo, b, advn, torch.full((M,), n - 1, dtype=torch.int64, device=DEV), ("all the last sample", M))


@pytest.mark.parametrize("D,H,L,A,act", [(44, 48, 1, 2, "relu"), (27, 80, 2, 3, "tanh")])
def test_grad_ignores_what_the_workspace_held(torch_cuda, envs, D, H, L, A, act):
    """Every slot entry is written before it is read: a workspace of NaN bytes past the statistics gives the same bits."""
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(D), H, L, act, A, seed=D)
    b, _ = _prepare(torch, pol, ppo, 8, 8192, seed=D)
    idx = torch.randperm(65536, device=DEV, generator=torch.Generator(device=DEV).manual_seed(D))[:40000]
    ppo.grad(b, idx)                                           # (grows the workspace to its size for M = 40 000)
    ppo.workspace[256:].zero_()
    clean, st_clean = ppo.grad(b, idx, stats=True)
    ppo.workspace[256:].fill_(0xFF)
    dirty, st_dirty = ppo.grad(b, idx, stats=True)
    assert bool(torch.isfinite(clean).all()) and torch.equal(clean, dirty) and torch.equal(st_clean, st_dirty)


# ------------------------------------------------------------------------------------------------------------------------------------
# hyper-parameters
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip,vf_coef,ent_coef,adv_eps", [(0.05, 0.0, 0.1, 1e-8), (0.5, 2.0, 0.0, 0.5), (0.2, 0.5, 0.01, 1e-8)])
def test_grad_hyperparameters_reach_the_kernel(torch_cuda, envs, clip, vf_coef, ent_coef, adv_eps):
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(22), 48, 2, "tanh", 4, seed=22, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, adv_eps=adv_eps)
    b, advn = _prepare(torch, pol, ppo, 4, 2000, seed=22)
    flat = b["adv"].reshape(-1).double()
    st = ppo.adv_stats().double()
    assert abs(float(st[1]) - (float(flat.std()) + adv_eps)) <= 1e-6 * (float(flat.std()) + adv_eps)
    idx = torch.randperm(8000, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))[:5000]
    _check_grad(torch, pol, ppo, b, advn, idx, (clip, vf_coef, ent_coef, adv_eps), (clip, vf_coef, ent_coef))


# ------------------------------------------------------------------------------------------------------------------------------------
# GAE
# ------------------------------------------------------------------------------------------------------------------------------------
GAE_SHAPES = ((1, 2), (2, 1), (1, 256), (3, 257), (64, 255), (7, 65537))
GAE_DISCOUNTS = ((0.99, 0.95), (0.999, 1.0), (0.5, 0.0), (1.0, 1.0))
DONE_PATTERNS = ("none", "all", "last row", "random")


def _check_adv_stats(torch, ppo, adv, adv_eps=1e-8):
    """adv_stats() against an f64 two-pass mean and unbiased std of the kernel's own advantages."""
    a = adv.reshape(-1).double()
    mean64 = float(a.mean())
    std64 = float(((a - mean64) ** 2).sum() / (a.numel() - 1)) ** 0.5
    mean, stdp, inv = (float(v) for v in ppo.adv_stats().double())
    assert abs(mean - mean64) <= 1e-6 * (abs(mean64) + std64), (mean, mean64, std64)
    assert abs((stdp - adv_eps) - std64) <= 1e-6 * (std64 + adv_eps), (stdp, std64)
    assert abs(inv * stdp - 1.0) <= 2.0 ** -22


def test_gae_domain(torch_cuda, envs):
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(7), 16, 1, "tanh", 2)
    g = torch.Generator(device=DEV).manual_seed(0)
    for (K, N), (gamma, lam), pattern in itertools.product(GAE_SHAPES, GAE_DISCOUNTS, DONE_PATTERNS):
        done = torch.zeros((K, N), dtype=torch.uint8, device=DEV)
        if pattern == "all":
            done.fill_(1)
        elif pattern == "last row":
            done[-1] = 1
        elif pattern == "random":
            done = (torch.rand((K, N), generator=g, device=DEV) < 0.2).to(torch.uint8)
        b = dict(rew=torch.randn((K, N), generator=g, device=DEV, dtype=torch.float64), done=done,
                 val=torch.randn((K, N), generator=g, device=DEV), last_val=torch.randn((N,), generator=g, device=DEV))
        adv, ret = ppo.gae(b, gamma, lam)
        ref_adv, ref_ret = torch_gae(torch, b, gamma, lam)
        tag = (K, N, gamma, lam, pattern)
        assert torch.equal(adv, ref_adv) and torch.equal(ret, ref_ret), tag
        _check_adv_stats(torch, ppo, adv)
    # mean / std ~ 1e3: the single-pass variance (sum of squares minus sum * mean, in f64)
    K, N = 16, 4096
    b = dict(rew=1000.0 + torch.randn((K, N), generator=g, device=DEV, dtype=torch.float64),
             done=torch.ones((K, N), dtype=torch.uint8, device=DEV), val=torch.zeros((K, N), device=DEV),
             last_val=torch.zeros((N,), device=DEV))
    adv, ret = ppo.gae(b)
    ref_adv, ref_ret = torch_gae(torch, b)
    assert torch.equal(adv, ref_adv) and torch.equal(ret, ref_ret)
    assert 900.0 < float(adv.double().mean()) / float(adv.double().std()) < 1100.0
    _check_adv_stats(torch, ppo, adv)


# ------------------------------------------------------------------------------------------------------------------------------------
# whole updates: uneven chunks, two calls in a row
# ------------------------------------------------------------------------------------------------------------------------------------
UPDATE_HP = dict(lr=1e-3, betas=(0.3, 0.95), eps=1e-6)


@pytest.mark.parametrize("K,N,minibatches,chunks", [(8, 125, 3, 3), (8, 125, 6, 6), (2, 5, 6, 5)])
def test_update_uneven_chunks_and_continuity(torch_cuda, envs, K, N, minibatches, chunks):
    torch = torch_cuda
    n = K * N
    assert len(torch.arange(n).chunk(minibatches)) == chunks
    pol, ppo = _ppo(torch, envs(88), 48, 1, "relu", 3, seed=n + minibatches, **UPDATE_HP)
    b, advn = _prepare(torch, pol, ppo, K, N, seed=88)
    g = torch.Generator(device=DEV).manual_seed(minibatches)
    perms = [torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(2)]) for _ in range(2)]
    r64, s64, _ = ref_update(torch, pol, b, advn, perms, minibatches, torch.float64, adam=UPDATE_HP)
    r32, s32, _ = ref_update(torch, pol, b, advn, perms, minibatches, torch.float32, adam=UPDATE_HP)
    for perm in perms:
        st = ppo.update(b, perm, 2, minibatches, stats=True)
        assert st.shape == (2 * chunks, 4) and bool(torch.isfinite(st).all())
    check_per_tensor(torch, pol, pol.params, r64, r32, ("update", n, minibatches))
    assert ppo.step == int(s64["step"]) == 2 * 2 * chunks
    # the moments: within 1e-5 of their max, plus 4x the torch f32 update's own distance from f64 (Adam's normalised steps let
    # the f32 and f64 trajectories part by a few 1e-5 over 12-20 steps)
    P = ppo.n_params
    for mine, name in ((ppo.adam_mv[:P], "exp_avg"), (ppo.adam_mv[P:], "exp_avg_sq")):
        for k, (o, s) in pol.offsets.items():
            e = int(np.prod(s))
            want, t32 = s64[name][o: o + e].double(), s32[name][o: o + e].double()
            e_mine, e_t32 = float((mine[o: o + e].double() - want).abs().max()), float((t32 - want).abs().max())
            assert e_mine <= 4 * e_t32 + 1e-5 * float(want.abs().max()), (name, k, e_mine, e_t32)


# ------------------------------------------------------------------------------------------------------------------------------------
# Adam's moments
# ------------------------------------------------------------------------------------------------------------------------------------
def _ulp(torch, t):
    t = t.abs().float()
    return (torch.nextafter(t, torch.full_like(t, float("inf"))) - t).double()


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.99), (0.3, 0.9), (0.0, 0.999)])
def test_adam_moments_match_torch(torch_cuda, envs, betas):
    """20 steps with gradients over 1e-8 .. 1e3 (zeros, sign flips).  After every step m (v) is within 2 ulp of max(|m_prev|, |g|)
    (max(b2 v_prev, (1 - b2) g^2)) of torch.optim.Adam(foreach=True) stepped from the same state; the parameters follow a free-running
    torch.optim.Adam to rtol 1e-6 / atol 1e-7; with b1 = 0, m is g bitwise."""
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(7), 128, 2, "tanh", 4, lr=1e-3, betas=betas)
    P = ppo.n_params
    free = pol.params.detach().clone().requires_grad_(True)
    opt_free = torch.optim.Adam([free], lr=1e-3, betas=betas, foreach=True)
    sync = pol.params.detach().clone().requires_grad_(True)
    opt_sync = torch.optim.Adam([sync], lr=1e-3, betas=betas, foreach=True)
    g = torch.Generator(device=DEV).manual_seed(int(betas[0] * 10))
    for step in range(20):
        mag = torch.pow(10.0, torch.rand(P, generator=g, device=DEV) * 11.0 - 8.0)
        sign = torch.where(torch.rand(P, generator=g, device=DEV) < 0.5, -1.0, 1.0)
        grad = torch.where(torch.rand(P, generator=g, device=DEV) < 0.1, torch.zeros_like(mag), mag * sign)
        m_prev, v_prev = ppo.adam_mv[:P].clone(), ppo.adam_mv[P:].clone()
        if step:
            st = opt_sync.state[sync]
            st["exp_avg"].copy_(m_prev)
            st["exp_avg_sq"].copy_(v_prev)
            with torch.no_grad():
                sync.copy_(pol.params)
        ppo.adam_step(grad)
        for p, opt in ((free, opt_free), (sync, opt_sync)):
            p.grad = grad.clone()
            opt.step()
        m, v = ppo.adam_mv[:P], ppo.adam_mv[P:]
        st = opt_sync.state[sync]
        bm = 2 * _ulp(torch, torch.maximum(m_prev.abs(), grad.abs()))
        bv = 2 * _ulp(torch, torch.maximum(betas[1] * v_prev, (1 - betas[1]) * grad * grad))
        dm, dv = (m.double() - st["exp_avg"].double()).abs(), (v.double() - st["exp_avg_sq"].double()).abs()
        assert bool((dm <= bm).all()), (betas, step, "m", float((dm - bm).max()), int((dm > bm).sum()))
        assert bool((dv <= bv).all()), (betas, step, "v", float((dv - bv).max()), int((dv > bv).sum()))
        torch.testing.assert_close(pol.params, sync.detach(), rtol=1e-6, atol=1e-7)
        if betas[0] == 0.0:
            assert torch.equal(m, grad), (step, int((m != grad).sum()))
    torch.testing.assert_close(pol.params, free.detach(), rtol=1e-6, atol=1e-7)


def test_update_moment_with_beta1_zero_is_the_gradient(torch_cuda, envs):
    """ssg_ppo_update goes through the same Adam: with b1 = 0 the first moment after a one-minibatch update is that gradient, bitwise."""
    torch = torch_cuda
    pol, ppo = _ppo(torch, envs(27), 80, 2, "tanh", 3, seed=5, lr=1e-3, betas=(0.0, 0.999))
    b, _ = _prepare(torch, pol, ppo, 4, 1000, seed=5)
    g = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(3):
        perm = torch.randperm(4000, device=DEV, generator=g).unsqueeze(0)
        grad = ppo.grad(b, perm[0])
        ppo.update(b, perm, 1, 1)
        assert torch.equal(ppo.adam_mv[:ppo.n_params], grad)


# ------------------------------------------------------------------------------------------------------------------------------------
# the policy forward
# ------------------------------------------------------------------------------------------------------------------------------------
def _forward64(torch, pol, x):
    """The forward restated in f64 on the f32 parameters: (logp_all [N, A], value [N])."""
    logits, v = forward(torch, pol.params.detach().double(), pol.offsets, pol.n_hidden_layers, pol.activation, x.double())
    return torch.log_softmax(logits, -1), v


@pytest.mark.parametrize("history,n_beams", [(1, 1), (1, 16), (4, 16), (8, 16)])
def test_policy_forward_domain(torch_cuda, history, n_beams):
    """policy_act with caller uniforms at 1, 65 and 1000 envs (tail workgroups) against the f64 forward.  The bound is checked over the
    rows of the three handles together: max|mine - f64| <= 4 max|torch f32 - f64| + 1e-6 max|f64| for value and logp."""
    torch = torch_cuda
    hs = []
    for n in (1, 65, 1000):
        env = _vec(n, history, n_beams, n_maps=16)
        env.reset_tensor()
        acts = env.random_actions(history, 0, 2 * history + 3)
        for k in range(acts.shape[0]):
            env.step_tensor(acts[k])
        hs.append(env)
    D = hs[0].states_history
    obs = [e.obs.clone() for e in hs]
    us = [torch.rand(e.num_envs, generator=torch.Generator(device=DEV).manual_seed(e.num_envs), device=DEV) for e in hs]
    for j, (H, L, act, A) in enumerate(itertools.product((16, 48, 112), (1, 2), ("tanh", "relu"), (2, 4))):
        _, pol = actor_critic_policy(torch, D, H, L, act, A, seed=j)
        tag = (history, n_beams, H, L, act, A)
        rows = {k: [] for k in ("lp", "v", "lp64", "v64", "lp32", "v32")}
        near_total, near_err = 0, []
        for env, o, u in zip(hs, obs, us):
            a, logp, val, x = env.policy_act(pol, uniforms=u)
            assert torch.equal(x, (o / pol.obs_scale).float()), tag
            lp64_all, v64 = _forward64(torch, pol, x)
            _, logits32, v32 = pol.forward_reference(o)
            cdf = lp64_all.exp().cumsum(-1)
            near = (u.double().unsqueeze(-1) - cdf[:, :-1]).abs().min(dim=-1).values < 1e-5
            near_total += int(near.sum())
            ok = ~near
            ar = (u.double().unsqueeze(-1) > cdf[:, :-1]).sum(-1)
            assert torch.equal(a.long()[ok], ar[ok]), tag
            near_err.append(check_near_rows(torch, near, u, cdf, a, logp, lp64_all))   # near rows: an adjacent action, and ITS logp (below)
            al = a.long().unsqueeze(-1)
            rows["lp"].append(logp[ok]); rows["v"].append(val)
            rows["lp64"].append(lp64_all.gather(-1, al).squeeze(-1)[ok]); rows["v64"].append(v64)
            rows["lp32"].append(torch.log_softmax(logits32, -1).gather(-1, al).squeeze(-1)[ok]); rows["v32"].append(v32)
        assert near_total <= 3, tag
        cat = {k: torch.cat(v).double() for k, v in rows.items()}
        for q in ("lp", "v"):
            e_mine = float((cat[q] - cat[q + "64"]).abs().max())
            e_t32 = float((cat[q + "32"] - cat[q + "64"]).abs().max())
            assert e_mine <= 4 * e_t32 + 1e-6 * float(cat[q + "64"].abs().max()), (tag, q, e_mine, e_t32)
            if q == "lp":                                                       # the same bound, from the other rows, on the near rows
                e_near = torch.cat(near_err)
                assert e_near.numel() == near_total and bool((e_near <= 4 * e_t32 + 1e-6 * float(cat["lp64"].abs().max())).all()), (tag, e_near.tolist())
    for e, o in zip(hs, obs):
        assert torch.equal(e.obs, o)
        e.close()


@pytest.mark.parametrize("history,n_beams", [(1, 1), (8, 16)])
def test_fused_rollout_equals_stepwise_at_the_extreme_widths(torch_cuda, history, n_beams):
    torch = torch_cuda
    a, b = _vec(65, history, n_beams, n_maps=16), _vec(65, history, n_beams, n_maps=16)
    a.reset_tensor(); b.reset_tensor()
    _, pol = actor_critic_policy(torch, a.states_history, 48, 2, "tanh", 4, seed=history)
    fused = a.rollout_policy(pol, 12, seed=9, step0=3)
    step = stepwise_rollout(b, pol, 12, 9, 3)
    assert_same_rollout(torch, fused, step, (history, n_beams))
    assert torch.equal(a.obs, b.obs)
    a.close(); b.close()
