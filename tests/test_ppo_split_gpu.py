"""GPU checks of the PPO gradient and update with a separate value network (SSG_POLICY_SEPARATE_VALUE; ssg_ppo_grad / ssg_ppo_update and
their _ext forms).  The gradient against f64 autograd of a separate-tower reference under the project's bound (per packed tensor:
max|mine - f64| <= 4 max|torch f32 - f64| + 1e-6 max|f64|; loss terms as tests/test_ppo_native_gpu.py compares them), for the plain
loss and for the extended one with the value clip, the KL penalty and the gradient-norm clip on; the exact decomposition against the
shared policy (identical towers, vf_coef = 0); whole updates against the f64 update, run to run, ext-all-off against plain, and the
rollout seeing both towers' new weights; refusals of other flag bits.

Batches are synthetic (ppo_reference.synthetic_batch) on 64-env handles, one per obs_dim: the PPO calls take their own K, N.  Indices are
drawn with replacement (they repeat), and the workspace past the advantage statistics is filled with NaN bytes before every gradient."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, torch_cuda, vec  # noqa: F401
from ppo_reference import check_per_tensor, nan_fill, ref_grad, ref_update, shared_over_pi_tower, split_policy, synthetic_batch

pytestmark = pytest.mark.gpu

K, N = 4, 100                      # 400 samples per batch
MB = (1, 63, 65, 200)              # one sample, a tile less one, a tile plus one, several tiles
# (D, H, L, A, act): every D, H, L, A and activation of the issue's list, every H with both L, every A with both activations; the last
# is the largest LDS footprint (D = 176, H = 128, L = 2, with EXT)
SHAPES = [(7, 16, 1, 2, "tanh"), (22, 16, 2, 3, "relu"), (22, 48, 1, 4, "relu"), (7, 48, 2, 2, "relu"), (7, 128, 1, 3, "tanh"),
          (22, 128, 2, 4, "tanh"), (176, 128, 2, 3, "tanh")]
EXT_ON = dict(vf_clip=0.05, kl_coef=1.0, max_grad_norm=0.5)


@pytest.fixture(scope="module")
def envs(torch_cuda):
    made = {}

    def get(D):
        if D not in made:
            made[D] = vec(64, D)
        return made[D]
    yield get
    for e in made.values():
        e.close()


def _ppo(torch, pol, env, b, max_m, **kw):
    """A NativePPO whose workspace is sized for minibatches of max_m, after gae on b; returns it and the normalised advantages."""
    from ship_sim_gym_amd.ppo import NativePPO
    ppo = NativePPO(pol, env, **kw)
    ppo._ws(b["act"].numel(), max_m)
    ppo.gae(b)
    st = ppo.adv_stats()
    return ppo, (b["adv"].reshape(-1) - st[0]) / st[1]


def _check_grad(torch, pol, ppo, b, advn, idx, what, ext):
    nan_fill(ppo)
    mine, st = ppo.grad(b, idx, stats=True)
    nan_fill(ppo)
    assert torch.equal(mine, ppo.grad(b, idx)), what                       # bitwise run to run
    assert bool(torch.isfinite(mine).all()) and bool(torch.isfinite(st).all()), what
    kw = dict(vf_clip=EXT_ON["vf_clip"], kl_coef=EXT_ON["kl_coef"]) if ext else {}
    r64 = ref_grad(torch, pol, b, idx, advn, torch.float64, **kw)[0]
    r32, terms32 = ref_grad(torch, pol, b, idx, advn, torch.float32, **kw)[:2]
    check_per_tensor(torch, pol, mine, r64, r32, what, verbose=True)
    got = st.tolist()
    print("%s stats %s torch f32 %s" % (what, got, terms32))
    for k in range(5 if ext else 4):                                       # pg, VL, entropy, clip fraction[, KL]
        assert abs(got[k] - terms32[k]) <= 1e-5 * abs(terms32[k]) + 1e-6, (what, k, got, terms32)
    if ext:
        want_norm = float(r32.norm())
        assert abs(got[5] - want_norm) <= 1e-5 * abs(want_norm) + 1e-6, (what, got[5], want_norm)
        assert got[6] == EXT_ON["kl_coef"] and got[7] == 0.0
    return mine


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("D,H,L,A,act", SHAPES)
def test_grad_matches_f64_autograd(torch_cuda, envs, D, H, L, A, act, ext):
    torch = torch_cuda
    _, pol = split_policy(torch, D, H, L, act, A, seed=D + H + L + A)
    b = synthetic_batch(torch, pol, K, N, seed=D + H)
    ppo, advn = _ppo(torch, pol, envs(D), b, max(MB), **(EXT_ON if ext else {}))
    assert ppo.extended() == ext and set(pol.offsets) >= {"V0", "c0"}
    g = torch.Generator(device=DEV).manual_seed(H + A)
    for M in MB:
        idx = torch.randint(0, K * N, (M,), device=DEV, generator=g)
        if M > 1:
            idx[M // 2] = idx[0]                                           # a repeated index, whatever the draw
        _check_grad(torch, pol, ppo, b, advn, idx, (D, H, L, A, act, M, "ext" if ext else "plain"), ext)


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_grad_when_a_workgroup_takes_a_second_tile(torch_cuda, envs, ext):
    """M = 32 769 = 512 tiles + 1 sample: workgroup 0 takes a second tile (the slots' read-modify-write path), in both tower passes."""
    torch = torch_cuda
    _, pol = split_policy(torch, 7, 16, 2, "tanh", 3, seed=5)
    b = synthetic_batch(torch, pol, K, N, seed=5)
    ppo, advn = _ppo(torch, pol, envs(7), b, 32769, **(EXT_ON if ext else {}))
    idx = torch.randint(0, K * N, (32769,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    _check_grad(torch, pol, ppo, b, advn, idx, ("second tile", "ext" if ext else "plain"), ext)


PI_NAMES = ("W0", "b0", "W1", "b1", "Wpi", "bpi")
VF_NAMES = ("V0", "c0", "V1", "c1", "Wv", "bv")


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("D,H,L,A,act", [(7, 16, 1, 2, "tanh"), (22, 48, 2, 3, "relu"), (22, 128, 2, 4, "tanh"), (176, 128, 2, 3, "relu")])
def test_grad_decomposes_exactly(torch_cuda, envs, D, H, L, A, act, ext):
    """Identical towers, vf_coef = 0: the pi tower's and pi head's entries are the shared policy's entries at vf_coef = 0 on the same
    minibatch (== : a zero of either sign is a zero), and the vf tower's and vf head's entries are all zero."""
    torch = torch_cuda
    net, split = split_policy(torch, D, H, L, act, A, seed=D + H, same_towers=True)
    shared = shared_over_pi_tower(torch, net, split)
    b = synthetic_batch(torch, split, K, N, seed=D + L)
    kw = dict(vf_coef=0.0, **(dict(vf_clip=0.05, kl_coef=1.0) if ext else {}))
    ppo_s, _ = _ppo(torch, split, envs(D), b, 32769, **kw)
    ppo_h, _ = _ppo(torch, shared, envs(D), b, 32769, **kw)
    g = torch.Generator(device=DEV).manual_seed(D)
    for M in MB + ((32769,) if D == 7 else ()):
        idx = torch.randint(0, K * N, (M,), device=DEV, generator=g)
        nan_fill(ppo_s)
        nan_fill(ppo_h)
        gs, st_s = ppo_s.grad(b, idx, stats=True)
        gh, st_h = ppo_h.grad(b, idx, stats=True)
        assert bool(torch.isfinite(gs).all()) and float(gh.abs().max()) > 0
        for name in PI_NAMES:
            if name in split.offsets:
                (o1, s), (o2, _) = split.offsets[name], shared.offsets[name]
                n = int(np.prod(s))
                assert bool((gs[o1: o1 + n] == gh[o2: o2 + n]).all()), (M, name)
        for name in VF_NAMES:
            if name in split.offsets:
                o, s = split.offsets[name]
                assert bool((gs[o: o + int(np.prod(s))] == 0).all()), (M, name)
        assert torch.equal(st_s, st_h), M                                   # the loss sums keep their meaning and order


UPDATE_HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("D,H,L,A,act", [(22, 48, 2, 3, "tanh"), (7, 16, 1, 4, "relu")])
def test_whole_update_against_f64_and_run_to_run(torch_cuda, envs, D, H, L, A, act, ext):
    """2 epochs x 3 minibatches: 400 samples chunk into 134, 134, 132.  Parameters per packed tensor under the project's bound, the
    moments under tests/test_ppo_domain_gpu.py's (4x torch f32's own distance from f64 + 1e-5 of their max), and bitwise run to run."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    n = K * N
    assert [len(c) for c in torch.arange(n).chunk(3)] == [134, 134, 132]
    _, pol = split_policy(torch, D, H, L, act, A, seed=D * H)
    b = synthetic_batch(torch, pol, K, N, seed=D * 3)
    kw = dict(UPDATE_HP, **(EXT_ON if ext else {}))
    ppo, advn = _ppo(torch, pol, envs(D), b, 134, **kw)
    g = torch.Generator(device=DEV).manual_seed(11)
    perm = torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(2)])
    p0, stats = pol.params.detach().clone(), ppo.adv_stats().clone()
    mgn = EXT_ON["max_grad_norm"] if ext else 0.0
    terms = dict(vf_clip=EXT_ON["vf_clip"], kl_coef=EXT_ON["kl_coef"]) if ext else {}
    r64, s64, _ = ref_update(torch, pol, b, advn, perm, 3, torch.float64, adam=UPDATE_HP, max_grad_norm=mgn, **terms)
    r32, s32, _ = ref_update(torch, pol, b, advn, perm, 3, torch.float32, adam=UPDATE_HP, max_grad_norm=mgn, **terms)
    nan_fill(ppo)
    st = ppo.update(dict(b), perm, 2, 3, stats=True)
    assert st.shape == (6, 8 if ext else 4) and bool(torch.isfinite(st).all()) and ppo.step == 6 == int(s64["step"])
    first, first_mv = pol.params.detach().clone(), ppo.adam_mv.clone()
    check_per_tensor(torch, pol, first, r64, r32, ("update", D, H, L, A, act, ext), verbose=True)
    P = ppo.n_params
    for mine, name in ((ppo.adam_mv[:P], "exp_avg"), (ppo.adam_mv[P:], "exp_avg_sq")):
        for k, (o, s) in pol.offsets.items():
            e = int(np.prod(s))
            want, t32 = s64[name][o: o + e].double(), s32[name][o: o + e].double()
            e_mine, e_t32 = float((mine[o: o + e].double() - want).abs().max()), float((t32 - want).abs().max())
            print("%s %s: |mine - f64| %.3e  |torch f32 - f64| %.3e  max %.3e" % (name, k, e_mine, e_t32, float(want.abs().max())))
            assert e_mine <= 4 * e_t32 + 1e-5 * float(want.abs().max()), (name, k, e_mine, e_t32)
    # both towers moved
    o = pol.offsets
    assert not torch.equal(first[: o["V0"][0]], p0[: o["V0"][0]]) and not torch.equal(first[o["V0"][0]:], p0[o["V0"][0]:])
    # again from the same start: the same bits
    pol.params.copy_(p0)
    ppo2 = NativePPO(pol, envs(D), **kw)
    ppo2._ws(n, 134)
    ppo2.workspace[:12].view(torch.float32).copy_(stats)
    nan_fill(ppo2)
    st2 = ppo2.update(dict(b), perm, 2, 3, stats=True)
    assert torch.equal(pol.params, first) and torch.equal(ppo2.adam_mv, first_mv) and torch.equal(st2, st)


@pytest.mark.parametrize("D,H,L,A,act", [(22, 48, 2, 3, "tanh"), (7, 128, 1, 2, "relu")])
def test_ext_with_every_term_off_is_the_plain_update_bitwise(torch_cuda, envs, D, H, L, A, act):
    torch = torch_cuda
    n = K * N
    _, pol = split_policy(torch, D, H, L, act, A, seed=H)
    b = synthetic_batch(torch, pol, K, N, seed=H)
    plain, _ = _ppo(torch, pol, envs(D), b, 200)
    ext, _ = _ppo(torch, pol, envs(D), b, 200)
    ext.force_ext = True
    assert not plain.extended() and ext.extended()
    g = torch.Generator(device=DEV).manual_seed(5)
    perm = torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(2)])
    p0 = pol.params.detach().clone()
    for M in MB:
        g0, s0 = plain.grad(b, perm[0, :M], stats=True)
        g1, s1 = ext.grad(b, perm[0, :M], stats=True)
        assert torch.equal(g0, g1) and torch.equal(s0, s1[:4]) and s1[4:].tolist() == [0.0, 0.0, 0.0, 0.0], M
    s0 = plain.update(dict(b), perm, 2, 3, stats=True)
    after = pol.params.detach().clone()
    pol.params.copy_(p0)
    s1 = ext.update(dict(b), perm, 2, 3, stats=True)
    assert torch.equal(pol.params, after) and torch.equal(plain.adam_mv, ext.adam_mv) and torch.equal(s0, s1[:, :4])
    assert not torch.equal(after, p0)


def test_rollout_sees_the_new_weights_of_both_towers(torch_cuda):
    """An update whose pi gradients are exactly zero (equal advantages, no entropy term) and whose vf gradients are not: the next
    rollout acts bit for bit as before and values differently; then an ordinary update moves the actions' log-probabilities too."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    n, D, Kr = 100, 22, 3
    env = vec(n, D)
    _, pol = split_policy(torch, D, 48, 2, "tanh", 3, seed=1)
    U = torch.rand((Kr, n), generator=torch.Generator(device=DEV).manual_seed(4), device=DEV)
    env.reset_tensor()
    r0 = {k: v.clone() for k, v in env.rollout_policy(pol, Kr, uniforms=U).items()}
    b = dict(r0)
    b["rew"], b["done"] = torch.zeros_like(r0["rew"]), torch.zeros_like(r0["done"])
    b["val"], b["last_val"] = torch.zeros_like(r0["val"]), torch.zeros_like(r0["last_val"])
    ppo = NativePPO(pol, env, ent_coef=0.0, lr=1e-2)
    adv, ret = ppo.gae(b)
    assert float(adv.abs().max()) == 0.0 and float(ret.abs().max()) == 0.0
    p0 = pol.params.clone()
    perm = torch.stack([torch.randperm(Kr * n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(e)) for e in range(2)])
    ppo.update(b, perm, 2, 3)
    vf0 = pol.offsets["V0"][0]
    assert torch.equal(pol.params[:vf0], p0[:vf0]) and not torch.equal(pol.params[vf0:], p0[vf0:])
    assert bool((ppo.adam_mv[:vf0] == 0).all())
    env.reset_tensor()
    r1 = {k: v.clone() for k, v in env.rollout_policy(pol, Kr, uniforms=U).items()}
    for k in ("obs", "act", "logp", "rew", "done", "flags"):
        assert torch.equal(r1[k], r0[k]), k
    assert not torch.equal(r1["val"], r0["val"]) and not torch.equal(r1["last_val"], r0["last_val"])
    assert float((r1["val"] - r0["val"]).abs().max()) > 1e-4
    # an ordinary update moves the pi tower as well
    ppo2 = NativePPO(pol, env, lr=1e-2)
    b2 = dict(r1)
    ppo2.gae(b2)
    ppo2.update(b2, perm, 2, 3)
    env.reset_tensor()
    r2 = env.rollout_policy(pol, Kr, uniforms=U)
    assert not torch.equal(r2["logp"][0], r1["logp"][0]) and not torch.equal(r2["val"][0], r1["val"][0])
    env.close()


BAD_FLAGS = (0x200, 0x102, 0x100 | 0xff, 0x300, 2, -1)


def test_bad_flag_bits_are_refused_and_launch_nothing(torch_cuda, envs):
    """ssg_ppo_grad, ssg_ppo_adam, ssg_ppo_update, ssg_ppo_grad_ext and ssg_ppo_update_ext, on pre-filled outputs."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as Nat
    D, n = 22, K * N
    env = envs(D)
    _, pol = split_policy(torch, D, 48, 2, "tanh", 3)
    b = synthetic_batch(torch, pol, K, N, seed=1)
    ppo, _ = _ppo(torch, pol, env, b, 200, **EXT_ON)
    ext = ppo._ext(b, n)
    idx = torch.arange(200, device=DEV)
    perm = torch.stack([torch.randperm(n, device=DEV) for _ in range(2)])
    grad = torch.full((ppo.n_params,), 7.0, device=DEV)
    stats = torch.full((6, 8), 7.0, device=DEV)
    torch.cuda.synchronize()
    p0, mv0, ws0, kl0 = pol.params.clone(), ppo.adam_mv.clone(), ppo.workspace.clone(), ppo.kl_coef.clone()
    L, P, h, stream = Nat.lib(), (lambda t: C.c_void_p(t.data_ptr())), env._h, ppo._stream()
    samples = [P(b[k]) for k in ("obs", "act", "logp", "adv", "ret")]
    ws, nb = ppo._ws_ptr()

    def calls(p):
        return [L.ssg_ppo_grad(h, C.byref(p), C.byref(ppo.hp), n, *samples, P(idx), 200, P(grad), P(stats), ws, nb, stream),
                L.ssg_ppo_adam(h, C.byref(p), C.byref(ppo.hp), P(grad), P(ppo.adam_mv), 1, stream),
                L.ssg_ppo_update(h, C.byref(p), C.byref(ppo.hp), n, *samples, P(perm), 2, 3, P(ppo.adam_mv), 0, P(stats), ws, nb, stream),
                L.ssg_ppo_grad_ext(h, C.byref(p), C.byref(ppo.hp), C.byref(ext), n, *samples, P(idx), 200, P(grad), P(stats), ws, nb, stream),
                L.ssg_ppo_update_ext(h, C.byref(p), C.byref(ppo.hp), C.byref(ext), n, *samples, P(perm), 2, 3, P(ppo.adam_mv), 0, P(stats),
                                     ws, nb, stream)]

    for flag in BAD_FLAGS:
        p = pol.to_native()
        p.activation = flag
        assert calls(p) == [-1] * 5, hex(flag)
    torch.cuda.synchronize()
    assert torch.equal(pol.params, p0) and torch.equal(ppo.adam_mv, mv0) and torch.equal(ppo.workspace, ws0) and torch.equal(ppo.kl_coef, kl0)
    assert bool((grad == 7).all()) and bool((stats == 7).all())
    # the good record is served by every one of them
    assert calls(pol.to_native()) == [0] * 5
    torch.cuda.synchronize()
    assert not bool((grad == 7).any()) and not torch.equal(pol.params, p0)
