"""The cells of the update matrix no other test reached (profiles/update_call/README.md lists who reaches which): an update whose
caller passes no stats buffer, on every population path, and unequal slices x extended loss x per-minibatch advantage normalisation.

layout {equal slices on the common entry points, equal slices on schedules, unequal slices} x {plain, extended} x {batch, per-minibatch
normalisation}: the same update runs with and without stats, and every member's own NativePPO runs it on its shard without stats
(population_harness's comparison); parameters, Adam moments and KL coefficients are torch.equal all three ways, and the stats rows
that were asked for are the ones test_population_*_gpu.py and test_adv_norm_gpu.py pin — so the NULL-stats cell of one policy is
reached too.  The smallest shapes at which a wrong field of the call's record still shows: 192 envs, obs_dim 8 (history 1, 2 beams),
hidden 16, one layer, K = 3; P = 3 on equal slices and on slices (1, 63, 128): one env, a partial wave, two workgroups; epochs 2 x
minibatches 3, so the last chunk is shorter; schedules epochs (1, 2, 2) x minibatches (1, 3, 2), so member 0 idles after launch 0."""
import pytest

from gpu_support import DEV, env_config
from gpu_support import torch_cuda  # noqa: F401
from population_harness import age, cached, member_hparams, perms_per_member, shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy

pytestmark = pytest.mark.gpu

N_ENVS, D, H, K, P = 192, 8, 16, 3, 3
EXT = {"vf_clip": [10.0, 0.0, 0.2], "max_grad_norm": [0.0, 0.03, 0.5], "kl_coef": [1.0, 0.0, 0.5], "kl_target": [1e-4, 0.0, 10.0]}
LAYOUTS = {"equal-common": ((64, 64, 64), 2, 3), "equal-sched": ((64, 64, 64), [1, 2, 2], [1, 3, 2]), "sliced": ((1, 63, 128), 2, 3),
           "sliced-sched": ((1, 63, 128), [1, 2, 2], [1, 3, 2])}


def _setup(torch, sizes):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    sliced = len(set(sizes)) > 1

    def make_env(n, base):
        env = ShipVecEnv(n, n_maps=64, n_beams=2, env_config=env_config(1), env_id_base=base)
        assert env.states_history == D
        if sliced and n == N_ENVS:
            env.set_population_slices(list(sizes))
        return env

    def make():
        setup = shard_rollouts(torch, make_env, lambda d: [actor_critic_policy(torch, d, H, 1, seed=40 + m)[1] for m in range(P)], sizes, K, 5)
        env, pop, b, shards, refs, sbs = setup
        age(torch, b, sbs, list(sizes), pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(sum(sizes) + sizes[0]), True)
        return setup
    return cached(tuple(sizes), make)


@pytest.mark.parametrize("adv_norm", ["batch", "minibatch"])
@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_update_without_stats_is_the_update_with_them_and_each_members_own(torch_cuda, layout, ext, adv_norm):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    sizes, epochs, minibatches = LAYOUTS[layout]
    env, pop, b0, shards, refs, sbs0 = _setup(torch, sizes)
    terms = EXT if ext else {}
    hp = member_hparams(P)
    ep = epochs if isinstance(epochs, list) else [epochs] * P
    mbs = minibatches if isinstance(minibatches, list) else [minibatches] * P
    samples = [K * s for s in sizes]
    steps = [e * chunk_split(s, c)[1] for e, c, s in zip(ep, mbs, samples)]
    g = torch.Generator(device=DEV).manual_seed(17)
    perm = perms_per_member(torch, g, max(ep), samples) if len(set(sizes)) > 1 else stacked_perms(torch, g, P, max(ep), samples[0])
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        runs = []
        for stats in (True, False):
            pop.params.copy_(saved[0])
            b = dict(b0)
            ppo = PopulationPPO(pop, env, adv_norm=adv_norm, **hp, **terms)
            ppo.gae(b)
            st = ppo.update(b, perm, epochs, minibatches, stats=stats)
            assert ppo.extended() == ext and ppo.member_steps == steps
            assert (st is None) == (not stats)
            if stats:
                assert st.shape == (P, max(steps), 8 if ext else 4) and bool(torch.isfinite(st).all())
                for m in range(P):
                    assert bool((st[m, steps[m]:] == 0).all()), m             # (an idle member's rows stay zero)
            runs.append((pop.params.clone(), ppo.adam_mv.clone(), ppo.kl_coef.clone()))
        for with_stats, without in zip(*runs):
            assert torch.equal(with_stats, without)
        assert not torch.equal(runs[0][0], saved[0])
        for m in range(P):
            ref = NativePPO(refs[m], shards[m], lr=hp["lr"][m], betas=(hp["beta1"][m], 0.999), clip=hp["clip"][m], ent_coef=hp["ent_coef"][m],
                            adv_norm=adv_norm, **{k: v[m] for k, v in terms.items()})
            sb = dict(sbs0[m])
            ref.gae(sb, 0.99, hp["lam"][m])
            assert ref.update(sb, perm[m][:ep[m]].contiguous(), ep[m], mbs[m]) is None
            assert ref.step == steps[m]
            assert torch.equal(runs[1][0][m], refs[m].params), (m, "params")
            assert torch.equal(runs[1][1][m], ref.adam_mv), (m, "moments")
            assert torch.equal(runs[1][2][m:m + 1], ref.kl_coef), (m, "coefficient")
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)
