"""GPU checks of the PPO loss's per-sample decisions AT their boundaries (ppo_grad_body in csrc/shipsim_ppo.hip, and the gradient-norm
clip behind it): min(s1, s2) and the ratio clamp at lo and hi, max(l1, l2) and the value clamp at +-vf_clip, the clip fraction, the KL
term, and coef = min(1, max_grad_norm / (norm + 1e-6f)) at coef == 1.  tests/loss_edges.py has the idea (zero head weights and M = 1 make
one sample's dl[j], dv and loss terms readable; the ratio is read off the device and the f64 autograd reference evaluated ON it), the
tables and the references; tests/test_loss_edges.py shows on the host that every defect these tests are there for fails a named case.

Per-sample bound: |mine - ref| <= 1e-5 * S + 1e-30, S = the sum of the magnitudes of the component's addends (a wrong decision is
0.5 S or more).  Measured on the MI355X over every case (6 208 per body), both body kinds, L = 1 and 2, H = 16 and 48: the largest
|mine - ref| / S is 5.47e-07, the same in all four (test_every_case_against_the_reference prints it); no case failed, so every decision
is as include/shipsim.h states it."""
import numpy as np
import pytest

import loss_edges as E
from gpu_support import DEV, torch_cuda, vec  # noqa: F401
from ppo_reference import actor_critic_policy, check_per_tensor, split_policy, synthetic_batch

pytestmark = pytest.mark.gpu

D = 7
TABLE_KEYS = [(2, 0), (2, 1), (3, 0), (3, 2), (4, 0), (4, 3)]      # (n_actions, the acted action): the first and the last
# (body, layers, width, whether the cases without an extended term go through the _ext entry points): H = 48 is three column tiles and
# an idle wave; the plain and the _ext kernels are separate instantiations of the same loss code
COMBOS = [("shared", 1, 16, False), ("shared", 2, 48, True), ("split", 1, 48, True), ("split", 2, 16, False)]
TRUNK = ("W0", "b0", "W1", "b1", "V0", "c0", "V1", "c1")


@pytest.fixture(scope="module")
def envs(torch_cuda):
    """One 64-env handle per obs_dim."""
    made = {}

    def get(d):
        if d not in made:
            made[d] = vec(64, d)
        return made[d]
    yield get
    _RUNS.clear()
    for e in made.values():
        e.close()


_TABLES, _RUNS = {}, {}


def _table(A, act):
    if (A, act) not in _TABLES:
        _TABLES[A, act] = E.with_twins(E.table(A, act))
    return _TABLES[A, act]


def _policy(torch, mode, H, L, A, seed, d=D):
    """A policy whose head weights are zero: logits == bpi and value == bv whatever the trunk computes."""
    _, pol = (actor_critic_policy if mode == "shared" else split_policy)(torch, d, H, L, "tanh", A, seed=seed)
    assert pol.separate_value == (mode == "split")
    for k in ("Wpi", "Wv"):
        o, s = pol.offsets[k]
        pol.params[o: o + int(np.prod(s))].zero_()
    return pol


def _batch(torch, cases, seed, adv=None):
    """The cases as the rows of a [1, n] batch; the observations are uniform noise (the trunk's output reaches no head)."""
    n = len(cases)
    col = lambda f, dt: torch.tensor([f(c) for c in cases], dtype=dt, device=DEV).reshape(1, n).contiguous()  # noqa: E731
    g = torch.Generator(device=DEV).manual_seed(seed)
    return dict(obs=torch.rand((1, n, D), generator=g, device=DEV), act=col(lambda c: c.act, torch.int32), logp=col(lambda c: c.logp, torch.float32),
                adv=col((lambda c: c.adv) if adv is None else (lambda c: adv), torch.float32), ret=col(lambda c: c.ret, torch.float32),
                val=col(lambda c: c.val, torch.float32),
                logp_all=torch.tensor(np.array([c.lpo for c in cases], dtype=np.float32), device=DEV).reshape(1, n, 4).contiguous())


def _plant(torch, ppo, n, M, st=(0.0, 1.0, 1.0, 0.0)):
    """Size the workspace and plant the advantage statistics (mean, std + eps, its inverse, 0): (0, 1, 1, 0) makes An = adv exactly."""
    ppo._ws(n, M)
    st = torch.as_tensor(st, dtype=torch.float32, device=DEV)
    ppo.workspace[:4 * st.numel()].view(torch.float32).copy_(st)
    return ppo


def _trainer(torch, pol, env, cfg, n, ext=False, M=128, **kw):
    from ship_sim_gym_amd.ppo import NativePPO
    ppo = NativePPO(pol, env, clip=cfg.clip, vf_coef=cfg.vf_coef, ent_coef=cfg.ent_coef, vf_clip=cfg.vf_clip, kl_coef=cfg.kl_coef, **kw)
    ppo.force_ext = ext
    return _plant(torch, ppo, n + 8, M)


def _params_of(torch, pol, cases):
    """[n, P]: the policy's parameters with every case's head biases."""
    (ob, _), (ov, _) = pol.offsets["bpi"], pol.offsets["bv"]
    allp = pol.params.detach().clone().repeat(len(cases), 1)
    allp[:, ob: ob + cases[0].A] = torch.tensor([c.bpi for c in cases], dtype=torch.float32, device=DEV)
    allp[:, ov] = torch.tensor([c.bv for c in cases], dtype=torch.float32, device=DEV)
    return allp


def _run(torch, env, pol, cases, b, ext, trainers, again=7):
    """One M = 1 grad(stats=True) per case under its own configuration and head biases: (gradients f32 [n, P], the stats rows as a
    list, whether every `again`-th call gave the same bits when repeated)."""
    n, P = len(cases), pol.params.numel()
    base, allp = pol.params.detach().clone(), _params_of(torch, pol, cases)
    G, S = torch.empty((n, P), dtype=torch.float32, device=DEV), torch.full((n, 8), float("nan"), dtype=torch.float32, device=DEV)
    idx, same = torch.arange(n, device=DEV), torch.ones((), dtype=torch.bool, device=DEV)
    try:
        for i, c in enumerate(cases):
            if c.cfg not in trainers:
                trainers[c.cfg] = _trainer(torch, pol, env, c.cfg, n, ext)
            pol.params.copy_(allp[i])
            g, st = trainers[c.cfg].grad(b, idx[i: i + 1], stats=True)
            G[i], S[i, : st.numel()] = g, st
            if i % again == 0:
                g2, st2 = trainers[c.cfg].grad(b, idx[i: i + 1], stats=True)
                same &= (g2.view(torch.int32) == g.view(torch.int32)).all() & (st2.view(torch.int32) == st.view(torch.int32)).all()
    finally:
        pol.params.copy_(base)
    S = S.cpu().numpy()
    return G.cpu().numpy(), [row[~np.isnan(row)] if np.isnan(row[4:]).all() else row for row in S], bool(same)


def _result(torch, envs, mode, L, H, ext, A, act):
    """The whole table of (A, act) through one policy, observed, completed with its rung cases and judged: a record, kept per module."""
    key = (mode, L, H, ext, A, act)
    if key in _RUNS:
        return _RUNS[key]
    env, pol = envs(D), _policy(torch, mode, H, L, A, seed=H + L + A)
    P = pol.params.numel()
    assert P == sum(int(np.prod(s)) for _, s in pol.offsets.values()) and pol.offsets["bpi"][1] == (A,) and pol.offsets["bv"][1] == (1,)
    first, trainers = _table(A, act), {}
    b0 = _batch(torch, first, seed=A)
    G0, S0, same0 = _run(torch, env, pol, first, b0, ext, trainers)
    cases, r, missing, disagree = E.complete(first, [s[0] for s in S0])
    rec = dict(env=env, pol=pol, first=first, b0=b0, S0=S0, trainers=trainers, cases=cases, r=r, missing=missing, disagree=disagree)
    if not missing:
        extra = cases[len(first):]
        G1, S1, same1 = _run(torch, env, pol, extra, _batch(torch, extra, seed=A + 1), ext, trainers, again=1)
        rec.update(G=np.concatenate([G0, G1]), S=S0 + S1, same=same0 and same1, ref=E.reference(torch, cases, r))
    _RUNS[key] = rec
    return rec


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the per-sample derivative and terms at every case
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,L,H,ext", COMBOS)
def test_every_case_against_the_reference(torch_cuda, envs, mode, L, H, ext):
    torch = torch_cuda
    worst = 0.0
    for A, act in TABLE_KEYS:
        rec = _result(torch, envs, mode, L, H, ext, A, act)
        assert not rec["missing"] and not rec["disagree"], (A, act, rec["missing"], rec["disagree"][:3])
        cases, r, G, S, ref, pol = (rec[k] for k in ("cases", "r", "G", "S", "ref", "pol"))
        assert rec["same"], (A, act)                                             # the same call twice: the same bits
        (ob, _), (ov, _) = pol.offsets["bpi"], pol.offsets["bv"]
        assert G.shape == (len(cases), pol.params.numel()) and np.isfinite(G).all()
        fails, w = E.judge(cases, r, ref, G[:, ob: ob + A], G[:, ov], S)
        worst = max(worst, w)
        assert not fails, (mode, L, H, A, act, len(fails), fails[:4])
        for k in TRUNK:                                                          # zero head weights: nothing reaches the trunk
            if k in pol.offsets:
                o, s = pol.offsets[k]
                assert not G[:, o: o + int(np.prod(s))].any(), (A, act, k)
        (ow, sw), (owv, swv) = pol.offsets["Wpi"], pol.offsets["Wv"]            # dl[j] * h[k] and dv * h[k], |h| <= 1 under tanh
        assert (np.abs(G[:, ow: ow + A * H].reshape(-1, A, H)) <= np.abs(G[:, ob: ob + A])[:, :, None]).all()
        assert (np.abs(G[:, owv: owv + H]) <= np.abs(G[:, ov])[:, None]).all()
        for c, st in zip(cases, S):
            wide = ext or c.cfg.vf_clip > 0 or c.cfg.kl_coef > 0
            assert len(st) == (8 if wide else 4) and np.isfinite(st).all(), c.name
            if wide:                                                             # no norm (the clip is off), the coefficient in use, 0
                assert st[5] == 0.0 and st[6] == np.float32(max(c.cfg.kl_coef, 0.0)) and st[7] == 0.0, (c.name, st)
    print("largest |mine - ref| / S over %s L=%d H=%d: %.3e" % (mode, L, H, worst))
    assert worst <= E.BOUND_REL


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the ladders' conditions
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["lo", "hi"])
@pytest.mark.parametrize("clip", E.CLIPS)
def test_the_ladder_reaches_the_bound_and_its_neighbours(torch_cuda, envs, clip, which):
    """Per clip and bound: the observed ratios hold bound-, bound and bound+, and wherever An = +1 and An = -1 both reveal the ratio
    (lo < r < hi) they reveal the same float."""
    lo, hi, _ = E.bounds32(clip)
    for A, act in ((2, 0), (3, 2), (4, 3)):
        rec = _result(torch_cuda, envs, "shared", 1, 16, False, A, act)
        rungs = {}
        for c, s in zip(rec["first"], rec["S0"]):
            if c.ladder is not None and c.ladder[:2] == (clip, which):
                rungs.setdefault(c.ladder[2], {})[c.adv] = np.float32(s[0])
        assert len(rungs) == 2 * E.LADDER_RUNGS + 1, (A, act)
        seen, both = set(), 0
        for k, tw in sorted(rungs.items()):
            a, b = np.float32(-tw[1.0]), tw[-1.0]                               # min(r, hi) and max(r, lo)
            assert a <= hi and b >= lo
            if a < hi and b > lo:
                both += 1
                assert a == b, (A, act, k, a, b)
            seen.add(float(a if a < hi else b))
        want = {float(t) for t in E.rung_targets(clip, which).values()}
        print("clip %g %s A=%d: %d distinct ratios over %d rungs, %d read through both signs" % (clip, which, A, len(seen), len(rungs), both))
        assert want <= seen, (A, act, sorted(want - seen))
        assert both > 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. padding rows and out-of-range indices
# ------------------------------------------------------------------------------------------------------------------------------------
PADDING_CASES = ("ladder/clip0.2/hi/k=+0/An=+1", "ratio/clip0.2/far=1/An=+1", "ratio/clip0.3/far=2/An=-1", "dist/low20/r=0.7992/An=-1",
                 "dist/low120/r=1.2012/An=+1", "value/c0.05/d=c+/tie_clamped", "value/c0.0625/d=c/tie_inside/ret=0", "value/c0.5/d=far-/l1>l2",
                 "kl/unnormalised_half", "kl/garbage_padding", "kl/old_logp_-100")


def test_an_out_of_range_index_is_a_zero_sample_and_a_second_tile_adds_up(torch_cuda, envs):
    """idx = [i, n + 5] (M = 2) is exactly half of case i's M = 1 gradient and loss means (halving is exact); idx = [i] * 65 (a second
    tile holding one row) is within the bound of the single-sample reference."""
    torch = torch_cuda
    rec = _result(torch, envs, "shared", 2, 48, True, 3, 2)
    assert not rec["missing"]
    pol, b, first, ref = rec["pol"], rec["b0"], rec["first"], rec["ref"]
    n, names = len(first), [c.name for c in first]
    (ob, _), (ov, _) = pol.offsets["bpi"], pol.offsets["bv"]
    base, allp = pol.params.detach().clone(), _params_of(torch, pol, first)
    try:
        for name in PADDING_CASES:
            i = names.index(name)
            ppo = rec["trainers"][first[i].cfg]
            pol.params.copy_(allp[i])
            g1, s1 = ppo.grad(b, torch.tensor([i], device=DEV), stats=True)
            g2, s2 = ppo.grad(b, torch.tensor([i, n + 5], device=DEV), stats=True)
            assert torch.equal(g1.cpu(), torch.tensor(rec["G"][i], dtype=torch.float32)), name
            assert torch.equal((g1 * 0.5).view(torch.int32), g2.view(torch.int32)), name
            assert torch.equal((s1[:5] * 0.5).view(torch.int32), s2[:5].view(torch.int32)) and torch.equal(s1[5:], s2[5:]), (name, s1, s2)
            g65, s65 = ppo.grad(b, torch.full((65,), i, device=DEV), stats=True)
            mine = g65.double().cpu().numpy()
            ok, rel = E.within_bound(np.append(mine[ob: ob + 3], mine[ov]), np.append(ref["dz"][i], ref["dv"][i]),
                                     np.append(ref["Sz"][i], ref["Sv"][i]))
            assert ok.all(), (name, rel)
            assert float(s65[3]) == float(s1[3]) and abs(float(s65[1]) - float(s1[1])) <= 1e-5 * abs(float(s1[1])), (name, s65, s1)
    finally:
        pol.params.copy_(base)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. every case in one minibatch
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,mode,L,H", [(2, "shared", 1, 16), (3, "split", 2, 48), (4, "shared", 2, 48)])
def test_the_whole_table_in_one_minibatch(torch_cuda, envs, A, mode, L, H):
    """The batch rows of a whole table under ONE parameter set (the 0.95 distribution, v = 0) and ONE configuration (every term on): grad
    over M = n against the pinned-ratio reference of the same minibatch in f64, under check_per_tensor's rule with the same reference in
    f32.  The ratios are read first, two M = 1 calls per sample."""
    torch = torch_cuda
    env, pol, cases = envs(D), _policy(torch, mode, H, L, A, seed=11 * A), _table(A, 0)
    n = len(cases)
    assert n % 64 != 0 and n > 512
    (ob, _), (ov, _) = pol.offsets["bpi"], pol.offsets["bv"]
    pol.params[ob: ob + A] = torch.tensor(E.distributions(A, 0)["p95"], dtype=torch.float32, device=DEV)
    pol.params[ov] = 0.0
    lo, hi, _ = E.bounds32(0.2)
    idx = torch.arange(n, device=DEV)
    reveal = []
    for adv in (1.0, -1.0):
        b, ppo = _batch(torch, cases, seed=A, adv=adv), _trainer(torch, pol, env, E.ratio_cfg(0.2), n)
        reveal.append(torch.stack([ppo.grad(b, idx[i: i + 1], stats=True)[1][0] for i in range(n)]).cpu().numpy())
    a, bb = -reveal[0], reveal[1]                                               # min(r, hi), max(r, lo)
    both = (a < hi) & (bb > lo)
    assert (a[both] == bb[both]).all() and both.any() and (a[~both] >= hi).any() and (bb[~both] <= lo).any()
    r = np.where(a < hi, a, bb).astype(np.float32)
    b = _batch(torch, cases, seed=A)
    ppo = _trainer(torch, pol, env, E.GROUP_CFG, n, M=n)
    mine, st = ppo.grad(b, idx, stats=True)
    assert torch.equal(mine, ppo.grad(b, idx))
    x = b["obs"].reshape(n, D)
    ref = [E.pinned_minibatch_grad(torch, pol.params, pol.offsets, L, "tanh", x, cases, r, E.GROUP_CFG, dt) for dt in (torch.float64, torch.float32)]
    check_per_tensor(torch, pol, mine, ref[0], ref[1], ("table", A, mode, L, H), verbose=True)
    cf = np.mean([float(E.clip_fraction_bit(x, 0.2)) for x in r])
    assert abs(float(st[3]) - cf) <= 1e-6 and bool(torch.isfinite(st).all()), (st, cf)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the gradient-norm clip at coef == 1
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,H,L,A,P", [(7, 16, 1, 2, 179), (22, 16, 1, 2, 419), (176, 128, 2, 4, None)])
def test_the_norm_clip_at_its_boundary(torch_cuda, envs, d, H, L, A, P):
    """betas = (0, 0.999): Adam's first moment after one step is the gradient it applied, bit for bit.  P = 179 is one partial sum of
    squares with a tail (ceil((P + 8) / 256) of them), 419 two, the largest accepted shape 156."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    f32 = np.float32
    env = envs(d)
    _, pol = actor_critic_policy(torch, d, H, L, "tanh", A, seed=d)
    n_par = pol.params.numel()
    assert P is None or n_par == P
    b = synthetic_batch(torch, pol, 8, 125, seed=d)
    first = NativePPO(pol, env)
    first.gae(b)
    st = first.adv_stats().clone()
    n = 1000
    perm = torch.randperm(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(d)).unsqueeze(0)
    p0 = pol.params.detach().clone()
    kw = dict(vf_clip=0.05, kl_coef=1.0, betas=(0.0, 0.999))

    def trainer(mgn, **more):
        return _plant(torch, NativePPO(pol, env, max_grad_norm=mgn, **dict(kw, **more)), n, n, st)

    def update(mgn, batch=b, **more):
        pol.params.copy_(p0)
        ppo = trainer(mgn, **more)
        s = ppo.update(batch, perm, 1, 1, stats=True)
        assert s.shape == (1, 8)
        return s[0].cpu().numpy(), ppo.adam_mv[:n_par].clone(), pol.params.detach().clone()

    try:
        g, s_g = trainer(1e30).grad(b, perm[0], stats=True)
        norm = f32(s_g[5].item())
        exact = float(g.double().pow(2).sum().sqrt())
        print("P=%d norm %.9g, sqrt(sum g^2) in f64 %.17g" % (n_par, norm, exact))
        assert norm > 0 and abs(float(norm) - exact) <= float(np.spacing(norm))
        s_free, m_free, p_free = update(0.0)
        assert s_free[5] == 0.0 and torch.equal(m_free, g) and not torch.equal(p_free, p0)
        m0 = f32(norm + f32(1e-6))
        below, above = np.nextafter(m0, f32(0.0)), np.nextafter(m0, f32(np.inf))
        for mgn in (m0, above):                                                 # coef == 1: the unclipped update, bit for bit
            assert E.clip_coef(mgn, norm) == 1.0
            s, m, p = update(float(mgn))
            assert s[5] == norm and torch.equal(m, g) and torch.equal(p, p_free), mgn
            assert np.array_equal(s[:5], s_free[:5])
        for mgn in (below, norm):                                               # whatever the restatement says (below m0: coef < 1)
            coef = E.clip_coef(mgn, norm)
            s, m, p = update(float(mgn))
            assert s[5] == norm
            print("max_grad_norm %.9g: coef %.9g" % (mgn, coef))
            if mgn == below:
                assert coef < 1.0
            if coef < 1.0:
                assert torch.equal(m, g * float(coef)) and bool((m != g).any()), mgn
            else:
                assert torch.equal(m, g) and torch.equal(p, p_free), mgn
        # a zero gradient: norm 0, coef = min(1, max_grad_norm / 1e-6f), nothing moves
        zero = dict(b, adv=torch.zeros_like(b["adv"]))
        for mgn in (1.0, 1e-7, 1e-30):
            pol.params.copy_(p0)
            ppo = _plant(torch, NativePPO(pol, env, max_grad_norm=mgn, vf_coef=0.0, ent_coef=0.0, vf_clip=0.05, betas=(0.0, 0.999)), n, n)
            s = ppo.update(zero, perm, 1, 1, stats=True)[0]
            assert bool(torch.isfinite(s).all()) and float(s[5]) == 0.0, (mgn, s)
            assert not bool(ppo.adam_mv.any()) and torch.equal(pol.params, p0), mgn
    finally:
        pol.params.copy_(p0)
