"""GPU checks of a population of separate-value-network policies (SSG_POLICY_SEPARATE_VALUE in ssg_population.activation; ssg_pop_*).
The reference of every check is the single-policy path on the member's slice alone — NativePolicy row m on a shard
``ShipVecEnv(n, env_id_base=m*n)``, NativePPO's update — and every comparison is torch.equal.  P = 3 members x n = 100 envs: a full
wave plus a tail per member."""
import ctypes as C

import pytest

from gpu_support import DEV, load_script, vec
from gpu_support import torch_cuda  # noqa: F401
from population_harness import age, cached, cols, shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy, split_module, split_policy

pytestmark = pytest.mark.gpu

P, N_ENVS, K = 3, 100, 4
SIZES = [N_ENVS] * P
# per member: RLlib's loss, PPO2's loss, everything off
EXT = {"vf_clip": [10.0, 0.05, 0.0], "max_grad_norm": [0.0, 0.03, 0.0], "kl_coef": [1.0, 0.0, 0.0], "kl_target": [1e-4, 0.0, 0.0]}
SHAPES = [(22, 48, 2, 3, "tanh"), (7, 16, 1, 4, "relu")]


def _members(torch, D, H, L, A, act, seed=100):
    return [split_policy(torch, D, H, L, act, A, seed=seed + m)[1] for m in range(P)]


def _setup(torch, shape):
    """One population rollout and the P shard rollouts (asserted equal, bootstrap value and ssg_pop_dist rows included); then, in
    both, the acting policy is made an older one: the same noise on the log-distribution and on the value prediction."""
    def make():
        D, H, L, A, act = shape
        setup = shard_rollouts(torch, lambda n, base: vec(n, D, base=base), lambda D: _members(torch, D, H, L, A, act), SIZES, K, 7)
        env, pop, b, shards, refs, sbs = setup
        assert pop.separate_value and pop.to_native().activation & 0x100
        age(torch, b, sbs, SIZES, A, b["logp_all"], torch.Generator(device=DEV).manual_seed(3), True)
        return setup
    return cached(shape, make)


@pytest.mark.parametrize("shape", SHAPES)
def test_rollout_and_dist_are_bitwise_each_members_own(torch_cuda, shape):
    """(the comparisons run inside the setup; here also the single forward)"""
    torch = torch_cuda
    env, pop, b, shards, refs, sbs = _setup(torch, shape)
    u = torch.rand(P * N_ENVS, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV)
    got = env.population_act(pop, uniforms=u)
    for m in range(P):
        want = shards[m].policy_act(refs[m], uniforms=u[m * N_ENVS:(m + 1) * N_ENVS].contiguous())
        for g, w in zip(got, want):
            assert torch.equal(g[m * N_ENVS:(m + 1) * N_ENVS], w), m


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("shape", SHAPES)
def test_gae_and_update_are_bitwise_each_members_own(torch_cuda, shape, ext):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env, pop, b, shards, refs, sbs = _setup(torch, shape)
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    lrs, lams = [1e-3, 5e-4, 1e-4], [0.9, 0.95, 1.0]
    terms = EXT if ext else {}
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, lr=lrs, lam=lams, **terms)
        assert ppo.extended() == ext and ppo.n_params == refs[0].params.numel()
        ppo._ws(K * N_ENVS, 134)                                           # (its final size, so that the NaN fill below stays)
        adv, ret = ppo.gae(b)
        stats = ppo.adv_stats().clone()
        ref_ppos = []
        for m in range(P):
            ref = NativePPO(refs[m], shards[m], lr=lrs[m], **{k: v[m] for k, v in terms.items()})
            r_adv, r_ret = ref.gae(sbs[m], 0.99, lams[m])
            assert torch.equal(cols(adv, m, SIZES), r_adv) and torch.equal(cols(ret, m, SIZES), r_ret), m
            assert torch.equal(stats[m], ref.adv_stats()), m
            ref_ppos.append(ref)
        samples = K * N_ENVS
        g = torch.Generator(device=DEV).manual_seed(11)
        for round_ in range(2):                                            # 3 minibatches: chunks of 134, 134, 132; the second continues
            perm = stacked_perms(torch, g, P, 2, samples)
            ppo.workspace[4096:].fill_(0xFF)                               # NaN bytes past the members' advantage statistics
            st = ppo.update(b, perm, 2, 3, stats=True)
            assert st.shape == (P, 6, 8 if ext else 4) and bool(torch.isfinite(st).all())
            for m in range(P):
                r_st = ref_ppos[m].update(sbs[m], perm[m], 2, 3, stats=True)
                assert torch.equal(pop.params[m], refs[m].params), (round_, m, "params")
                assert torch.equal(ppo.adam_mv[m], ref_ppos[m].adam_mv), (round_, m, "moments")
                assert torch.equal(st[m, :, :r_st.shape[1]], r_st), (round_, m, "stats")
                if ext:
                    assert torch.equal(ppo.kl_coef[m:m + 1], ref_ppos[m].kl_coef), (round_, m, "coefficient")
            if ext:
                assert bool((st[2, :, 4:] == 0).all()) and bool((st[0, :, 4] > 0).all()) and bool((st[1, :, 5] > 0).all())
        assert not torch.equal(pop.params, saved[0])
        vf0 = pop.offsets["V0"][0]
        assert not torch.equal(pop.params[:, vf0:], saved[0][:, vf0:]) and not torch.equal(pop.params[:, :vf0], saved[0][:, :vf0])
    finally:
        pop.params.copy_(saved[0])
        for r, p0 in zip(refs, saved[1]):
            r.params.copy_(p0)


def test_exploit_copies_the_longer_rows_and_load_into_round_trips(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    D, H, L, A, act = 22, 48, 2, 3, "tanh"
    env = vec(4 * 16, D)
    nets = [split_module(torch, D, H, L, act, A, seed=m) for m in range(4)]
    scale = torch.full((D,), 600.0, dtype=torch.float64, device=DEV)
    pop = NativePopulation.from_actor_critics(nets, scale)
    Lp = pop.n_params
    assert pop.separate_value and Lp == 2 * (H * D + H + H * H + H) + A * H + A + H + 1
    ppo = PopulationPPO(pop, env)
    ppo.adam_mv.copy_(torch.randn(ppo.adam_mv.shape, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV))
    p0, mv0 = pop.params.clone(), ppo.adam_mv.clone()
    ppo.exploit([0, 3, 2, 3])                                               # 1 <- 3, the whole row: both towers, both moment rows
    assert torch.equal(pop.params[1], p0[3]) and torch.equal(ppo.adam_mv[1], mv0[3])
    for m in (0, 2, 3):
        assert torch.equal(pop.params[m], p0[m]) and torch.equal(ppo.adam_mv[m], mv0[m])
    # load_into: row m into a separate-tower module; from_layers over its tensors gives the row back
    others = [split_module(torch, D, H, L, act, A, seed=50 + m) for m in range(4)]
    pop.load_into(others)
    for m, net in enumerate(others):
        assert torch.equal(NativePolicy.from_actor_critic(net, scale).params, pop.params[m]), m
        assert torch.equal(torch.cat([q.detach().flatten() for q in net.vf_body.parameters()]),
                           pop.params[m, pop.offsets["V0"][0]: pop.offsets["Wv"][0]])

    def triple(net):
        pair = lambda lin: (lin.weight.detach().clone(), lin.bias.detach().clone())  # noqa: E731
        return ([pair(l) for l in list(net.pi_body)[0::2]], pair(net.pi), pair(net.v), [pair(l) for l in list(net.vf_body)[0::2]])
    again = NativePopulation.from_layers([triple(net) for net in others], scale, activation=act)
    assert again.separate_value and torch.equal(again.params, pop.params)
    # one architecture per population
    with pytest.raises(ValueError, match="member 1"):
        NativePopulation([pop.member(0), actor_critic_policy(torch, D, H, L, act, A)[1]])
    env.close()


BAD_FLAGS = (0x200, 0x102, 0x100 | 0xff, 0x300, 2, -1)


def test_bad_flag_bits_are_refused_and_launch_nothing(torch_cuda):
    """Every ssg_pop_* entry point that takes the population record, on pre-filled outputs."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as Nat
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _setup(torch, SHAPES[0])
    D, n = pop.obs_dim, P * N_ENVS
    ppo = PopulationPPO(pop, env, **EXT)
    b = dict(b)
    ppo.gae(b)
    ppo._ws(K * N_ENVS, 134)
    samples = K * N_ENVS
    perm = torch.stack([torch.stack([torch.randperm(samples, device=DEV) for _ in range(2)]) for _ in range(P)])
    table = ppo._table(6)
    ext, ext_table = ppo._ext(b, K, n)
    f = lambda shape, dt=torch.float32: torch.full(shape, 7, dtype=dt, device=DEV)  # noqa: E731
    out = {"act": f((K, n), torch.int32), "logp": f((K, n)), "val": f((K, n)), "x": f((K, n, D)), "rew": f((K, n), torch.float64),
           "done": f((K, n), torch.uint8), "flags": f((K, n), torch.uint8), "last": f((n,)), "logp_all": f((K, n, 4)),
           "adv": f((K, n)), "ret": f((K, n)), "stats": f((P, 6, 8))}
    torch.cuda.synchronize()
    state0, obs0, p0, mv0, ws0 = env.state.clone(), env.obs.clone(), pop.params.clone(), ppo.adam_mv.clone(), ppo.workspace.clone()
    L, Pt, h, stream = Nat.lib(), (lambda t: C.c_void_p(t.data_ptr())), env._h, ppo._stream()
    batch = [Pt(b[k]) for k in ("obs", "act", "logp", "adv", "ret")]
    ws, nb = Pt(ppo.workspace), ppo.workspace.numel()
    src = (C.c_int32 * P)(0, 0, 2)

    def calls(p):
        return [L.ssg_pop_act(h, C.byref(p), Pt(env.obs), None, 0, 0, Pt(out["act"]), Pt(out["logp"]), Pt(out["val"]), Pt(out["x"]), stream),
                L.ssg_pop_rollout(h, C.byref(p), K, None, 0, 0, Pt(env.obs), Pt(out["act"]), Pt(out["logp"]), Pt(out["val"]), Pt(out["x"]),
                                  Pt(out["rew"]), Pt(out["done"]), Pt(out["flags"]), Pt(out["last"]), n, stream),
                L.ssg_pop_gae(h, C.byref(p), Pt(table), K, Pt(b["rew"]), Pt(b["done"]), Pt(b["val"]), Pt(b["last_val"]), Pt(out["adv"]),
                              Pt(out["ret"]), ws, nb, stream),
                L.ssg_pop_update(h, C.byref(p), Pt(table), 6, K, *batch, Pt(perm), 2, 3, Pt(ppo.adam_mv), Pt(out["stats"]), ws, nb, stream),
                L.ssg_pop_dist(h, C.byref(p), K, Pt(b["obs"]), Pt(out["logp_all"]), stream),
                L.ssg_pop_update_ext(h, C.byref(p), C.byref(ext), Pt(table), 6, K, *batch, Pt(perm), 2, 3, Pt(ppo.adam_mv), Pt(out["stats"]),
                                     ws, nb, stream),
                L.ssg_pop_exploit(h, C.byref(p), src, Pt(ppo.adam_mv), stream)]

    nbytes = C.c_size_t(12345)
    for flag in BAD_FLAGS:
        p = pop.to_native()
        p.activation = flag
        assert calls(p) == [-1] * 7, hex(flag)
        assert L.ssg_pop_workspace_nbytes(C.byref(p), samples, 134, C.byref(nbytes)) == -1 and nbytes.value == 12345
    torch.cuda.synchronize()
    assert torch.equal(env.state, state0) and torch.equal(env.obs, obs0) and torch.equal(pop.params, p0)
    assert torch.equal(ppo.adam_mv, mv0) and torch.equal(ppo.workspace, ws0)
    for k, t in out.items():
        assert bool((t == 7).all()), k


def test_pbt_trainer_with_separate_value_networks(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/pbt_native.py")
    hist, det = mod.train(members=4, envs_per_member=64, updates=2, horizon=8, perturb_every=1, seed=0, log=lambda s: None,
                          return_details=True, kl_coeff=1.0, max_grad_norm=0.5, separate_value=True)
    assert len(hist) == 2 and det["params"].shape[0] == 4 and bool(torch.isfinite(det["params"]).all())
    net = det["nets"][0]
    assert [n for n, _ in net.named_children()] == ["pi_body", "pi", "vf_body", "v"]
    assert det["params"].shape[1] == sum(q.numel() for q in net.parameters())
    assert torch.equal(torch.cat([q.detach().flatten() for q in net.parameters()]), det["params"][0])
