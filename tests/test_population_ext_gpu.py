"""GPU checks of the extended update for a population (ssg_pop_dist, ssg_pop_update_ext; PopulationPPO's vf_clip / max_grad_norm /
kl_coef / kl_target).  The reference of every check is the single-policy path: member m's update is NativePPO's with that member's
settings on a ``ShipVecEnv(n, n_maps=64, env_id_base=m*n)`` shard, and every comparison is torch.equal."""
import pytest

from gpu_support import DEV, load_script, torch_cuda  # noqa: F401
from population_harness import age, close_all, shard_rollouts, stacked_perms
from ppo_reference import actor_critic_policy

pytestmark = pytest.mark.gpu


def _vec(n, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64, env_id_base=base)


def _members(torch, D, P, seed=100):
    return [actor_critic_policy(torch, D, seed=seed + m)[1] for m in range(P)]


# P = 3: the reference's RLlib loss, PPO2's loss with its own clip range, and a member with everything off
P, N_ENVS, K = 3, 100, 4                        # 100 envs per member: a tail workgroup per member
EXT = {"vf_clip": [10.0, 0.05, 0.0], "max_grad_norm": [0.0, 0.03, 0.0], "kl_coef": [1.0, 0.0, 0.0], "kl_target": [1e-4, 0.0, 0.0]}


@pytest.fixture(scope="module")
def setup(torch_cuda):
    """One population rollout and the P shard rollouts (asserted equal); then, in both, the acting policy is made an older one:
    the same noise on the log-distribution and on the value prediction."""
    torch = torch_cuda
    sizes = [N_ENVS] * P
    env, pop, b, shards, refs, sbs = shard_rollouts(torch, _vec, lambda D: _members(torch, D, P), sizes, K, 7)
    age(torch, b, sbs, sizes, pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(3), False)
    yield env, pop, b, shards, refs, sbs
    close_all(env, shards)


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
        perm = stacked_perms(torch, g, P, 2, samples)
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
        perm = stacked_perms(torch, g, P, epochs, samples)
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
    mod = load_script("train/pbt_native.py")
    hist, det = mod.train(members=4, envs_per_member=64, updates=2, perturb_every=1, seed=0, log=lambda s: None, return_details=True,
                          kl_coeff=1.0, max_grad_norm=0.5)
    assert len(hist) == 2 and det["params"].shape[0] == 4 and bool(torch.isfinite(det["params"]).all())
    assert len(det["kl_coef"]) == 4 and all(c > 0 for c in det["kl_coef"])
