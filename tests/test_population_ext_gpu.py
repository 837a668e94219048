"""GPU checks of the extended update for a population (ssg_pop_dist, ssg_pop_update_ext; PopulationPPO's vf_clip / max_grad_norm /
kl_coef / kl_target).  The reference of every check is the single-policy path: member m's update is NativePPO's with that member's
settings on a ``ShipVecEnv(n, n_maps=64, env_id_base=m*n)`` shard, and every comparison is torch.equal."""
import importlib.util
import os

import pytest

from helpers import actor_critic_policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ROLLOUT_KEYS = ("obs", "act", "logp", "val", "rew", "done", "flags")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _vec(n, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64, env_id_base=base)


def _members(torch, D, P, seed=100):
    return [actor_critic_policy(torch, D, seed=seed + m)[1] for m in range(P)]


def _cols(t, m, n):
    return t[:, m * n:(m + 1) * n]


# P = 3: the reference's RLlib loss, PPO2's loss with its own clip range, and a member with everything off
P, N_ENVS, K = 3, 100, 4                        # 100 envs per member: a tail workgroup per member
EXT = {"vf_clip": [10.0, 0.05, 0.0], "max_grad_norm": [0.0, 0.03, 0.0], "kl_coef": [1.0, 0.0, 0.0], "kl_target": [1e-4, 0.0, 0.0]}


@pytest.fixture(scope="module")
def setup(torch_cuda):
    """One population rollout and the P shard rollouts (asserted equal); then, in both, the acting policy is made an older one:
    the same noise on the log-distribution and on the value prediction."""
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec(P * N_ENVS)
    D = env.states_history
    pop, refs = NativePopulation(_members(torch, D, P)), _members(torch, D, P)
    env.reset_tensor()
    b = dict(env.rollout_population(pop, K, seed=7))
    ppo = PopulationPPO(pop, env)
    la = ppo.dist(b).clone()
    g = torch.Generator(device=DEV).manual_seed(3)
    A = pop.n_actions
    noise = 0.3 * torch.randn((K, P * N_ENVS, A), generator=g, device=DEV)
    vnoise = (torch.rand((K, P * N_ENVS), generator=g, device=DEV) - 0.5) * 0.4
    shards, sbs = [], []
    for m in range(P):
        sh = _vec(N_ENVS, base=m * N_ENVS)
        sh.reset_tensor()
        sb = dict(sh.rollout_policy(refs[m], K, seed=7))
        for k in ROLLOUT_KEYS:
            assert torch.equal(_cols(b[k], m, N_ENVS), sb[k]), (m, k)
        # ssg_pop_dist's rows are ssg_ppo_dist's per member, and both reproduce the rollout's logp
        sla = NativePPO(refs[m], sh).dist(sb)
        assert torch.equal(_cols(la, m, N_ENVS), sla), m
        assert torch.equal(sla.gather(-1, sb["act"].long().unsqueeze(-1)).squeeze(-1), sb["logp"]), m
        shards.append(sh)
        sbs.append(sb)
    assert bool((la[..., A:] == 0).all())
    old = torch.zeros_like(la)
    old[..., :A] = torch.log_softmax(la[..., :A] + noise, -1)
    b["logp_all"] = old
    b["logp"] = old.gather(-1, b["act"].long().unsqueeze(-1)).squeeze(-1).contiguous()
    b["val"] = (b["val"] + vnoise).contiguous()
    for m in range(P):
        for k in ("logp_all", "logp", "val"):
            sbs[m][k] = _cols(b[k], m, N_ENVS).contiguous()
    yield env, pop, b, shards, refs, sbs
    env.close()
    for sh in shards:
        sh.close()


def test_population_ext_update_is_bitwise_each_members_own(torch_cuda, setup):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env, pop, b, shards, refs, sbs = setup
    lrs = [1e-3, 5e-4, 1e-4]
    ppo = PopulationPPO(pop, env, lr=lrs, **EXT)
    assert ppo.extended() and ppo.kl_coef.tolist() == EXT["kl_coef"]
    ppo.gae(b)
    samples = K * N_ENVS
    g = torch.Generator(device=DEV).manual_seed(11)
    ref_ppos = []
    for m in range(P):
        ref = NativePPO(refs[m], shards[m], lr=lrs[m], **{k: v[m] for k, v in EXT.items()})
        ref.gae(sbs[m])
        ref_ppos.append(ref)
    assert [r.extended() for r in ref_ppos] == [True, True, False]        # member 2 runs the PLAIN entry points
    for round_ in range(2):                                                # the second update continues the first
        perm = torch.stack([torch.stack([torch.randperm(samples, device=DEV, generator=g) for _ in range(2)]) for _ in range(P)])
        st = ppo.update(b, perm, 2, 2, stats=True)
        assert st.shape == (P, 4, 8) and bool(torch.isfinite(st).all())
        for m in range(P):
            r_st = ref_ppos[m].update(sbs[m], perm[m], 2, 2, stats=True)
            assert torch.equal(pop.params[m], refs[m].params), (round_, m, "params")
            assert torch.equal(ppo.adam_mv[m], ref_ppos[m].adam_mv), (round_, m, "moments")
            assert torch.equal(st[m, :, :r_st.shape[1]], r_st), (round_, m, "stats", st[m].tolist(), r_st.tolist())
            assert torch.equal(ppo.kl_coef[m:m + 1], ref_ppos[m].kl_coef), (round_, m, "coefficient")
        assert bool((st[2, :, 4:] == 0).all())                              # everything off: no KL, no norm, no coefficient
        assert bool((st[0, :, 4] > 0).all()) and bool((st[0, :, 5] == 0).all()) and bool((st[1, :, 5] > 0).all())
        assert bool((st[1, :, 4] == 0).all()) and bool((st[1, :, 6] == 0).all())
        print("member 1 gradient norms (bound 0.03): %s" % st[1, :, 5].tolist())
    # member 0's mean KL (noise of 0.3 on the logits: some 1e-2) is far above 2 x its target of 1e-4 in both updates
    assert bool((st[0, :, 4] > 1e-3).all()) and ppo.kl_coef.tolist() == [2.25, 0.0, 0.0]


@pytest.mark.parametrize("minibatches,chunks,last", [(3, 3, 132), (30, 29, 8)])
def test_population_ext_update_at_uneven_chunkings_is_bitwise_each_members_own(torch_cuda, setup, minibatches, chunks, last):
    """400 samples per member in 3 minibatches are chunks of 134, 134, 132; in 30 they are 29 chunks of 14, the last one of 8: the
    table rows, the stats rows and the adaptation count CHUNKS, in the population's loop as in the single policy's."""
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env, pop, b, shards, refs, sbs = setup
    samples, epochs = K * N_ENVS, 2
    sizes = [len(c) for c in torch.arange(samples).chunk(minibatches)]
    assert len(sizes) == chunks and sizes[-1] == last and sizes[0] > last
    lrs = [1e-3, 5e-4, 1e-4]
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, lr=lrs, **EXT)
        ppo.gae(b)
        g = torch.Generator(device=DEV).manual_seed(minibatches)
        perm = torch.stack([torch.stack([torch.randperm(samples, device=DEV, generator=g) for _ in range(epochs)]) for _ in range(P)])
        st = ppo.update(b, perm, epochs, minibatches, stats=True)
        assert st.shape == (P, epochs * chunks, 8) and bool(torch.isfinite(st).all()) and ppo.step == epochs * chunks
        for m in range(P):
            ref = NativePPO(refs[m], shards[m], lr=lrs[m], **{k: v[m] for k, v in EXT.items()})
            ref.gae(sbs[m])
            r_st = ref.update(sbs[m], perm[m], epochs, minibatches, stats=True)
            assert r_st.shape[0] == epochs * chunks and ref.step == ppo.step
            assert torch.equal(pop.params[m], refs[m].params), (m, "params")
            assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (m, "moments")
            assert torch.equal(st[m, :, :r_st.shape[1]], r_st), (m, "stats", st[m].tolist(), r_st.tolist())
            assert torch.equal(ppo.kl_coef[m:m + 1], ref.kl_coef), (m, "coefficient")
        assert bool((st[2, :, 4:] == 0).all()) and bool((st[0, :, 4] > 0).all()) and bool((st[1, :, 5] > 0).all())
        assert ppo.kl_coef.tolist() == [1.5, 0.0, 0.0]
    finally:
        pop.params.copy_(saved[0])
        for r, p0 in zip(refs, saved[1]):
            r.params.copy_(p0)


def test_exploit_carries_the_coefficient(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    env = _vec(4 * 16)
    pop = NativePopulation(_members(torch, env.states_history, 4))
    ppo = PopulationPPO(pop, env, kl_coef=[1.0, 2.0, 0.5, 0.25], kl_target=0.01)
    p0 = pop.params.clone()
    ppo.exploit([0, 3, 2, 3])                                               # 1 <- 3
    assert ppo.kl_coef.tolist() == [1.0, 0.25, 0.5, 0.25]
    assert torch.equal(pop.params[1], p0[3]) and torch.equal(pop.params[0], p0[0])
    env.close()


def test_pbt_trainer_with_the_references_loss_terms(torch_cuda):
    torch = torch_cuda
    spec = importlib.util.spec_from_file_location("pbt_native_ext_gpu", os.path.join(ROOT, "train", "pbt_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hist, det = mod.train(members=4, envs_per_member=64, updates=2, perturb_every=1, seed=0, log=lambda s: None, return_details=True,
                          kl_coeff=1.0, max_grad_norm=0.5)
    assert len(hist) == 2 and det["params"].shape[0] == 4 and bool(torch.isfinite(det["params"]).all())
    assert len(det["kl_coef"]) == 4 and all(c > 0 for c in det["kl_coef"])
