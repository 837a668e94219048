"""GPU checks of the population path (ssg_pop_*, ship_sim_gym_amd/population.py, train/pbt_native.py).  The reference of every check is
the single-policy path as it stands: member m's parameters are NativePolicy row m, its envs a ``ShipVecEnv(n, n_maps=64,
env_id_base=m*n)`` shard (train/ppo_torch.py's make_shards relies on such shards reproducing the unsplit batch), its update NativePPO's.
Every comparison is torch.equal: per member the population's launches run the single path's operations in the single path's order."""
import numpy as np
import pytest

from accounting_support import episode_stats_walk, layout
from gpu_support import DEV, env_config as _env_config, load_script, state_columns as _columns, torch_cuda  # noqa: F401
from population_harness import ROLLOUT_KEYS, close_all as _close, cols, member_hparams, shard_reference, shard_rollouts, stacked_perms
from ppo_reference import actor_critic_policy

pytestmark = pytest.mark.gpu


def _vec(n, base=0, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64, env_id_base=base, **kw)


def _members(torch, D, P, seed=100):
    """P NativePolicy objects with different seeded weights (built alike twice: once for the population, once as the references)."""
    return [actor_critic_policy(torch, D, seed=seed + m)[1] for m in range(P)]


def _population(torch, D, P, seed=100):
    from ship_sim_gym_amd.population import NativePopulation
    return NativePopulation(_members(torch, D, P, seed))


def _check_rollout(torch, P, n, K, philox, env_kw=None, seed=5, step0=3):
    """One population rollout against P shard rollouts; returns the number of env-steps compared."""
    env_kw = dict(env_kw or {})
    env = _vec(P * n, **env_kw)
    pop = _population(torch, env.states_history, P)
    refs = _members(torch, env.states_history, P)
    for m in range(P):
        assert torch.equal(pop.params[m], refs[m].params) and pop.member(m).params.data_ptr() == pop.params[m].data_ptr()
    g = torch.Generator(device=DEV).manual_seed(P * 1000 + n)
    U = None if philox else torch.rand((K, P * n), generator=g, device=DEV)
    env.reset_tensor()
    b = env.rollout_population(pop, K, seed=seed, step0=step0, uniforms=U)
    state = _columns(env)
    final_obs = env.obs.clone()
    for m in range(P):
        sh = _vec(n, base=m * n, **env_kw)
        sh.reset_tensor()
        r = sh.rollout_policy(pop.member(m), K, seed=seed, step0=step0, uniforms=None if philox else U[:, m * n:(m + 1) * n].contiguous())
        for k in ROLLOUT_KEYS:
            assert b[k].dtype == r[k].dtype and torch.equal(cols(b[k], m, [n] * P), r[k]), (P, n, m, k)
        assert torch.equal(b["last_val"][m * n:(m + 1) * n], r["last_val"]), (P, n, m, "last_val")
        assert torch.equal(final_obs[m * n:(m + 1) * n], sh.obs), (P, n, m, "final obs")
        for name, col in _columns(sh).items():
            assert torch.equal(state[name][..., m * n:(m + 1) * n], col), (P, n, m, name)
        sh.close()
    if P == 1:  # the same handle, the single-policy call
        env.reset_tensor()
        r = env.rollout_policy(pop.member(0), K, seed=seed, step0=step0, uniforms=U)
        for k in ROLLOUT_KEYS + ("last_val",):
            assert torch.equal(b[k], r[k]), k
    if P > 1:  # the members really act differently: the check is not one policy compared with itself P times
        assert not torch.equal(b["val"][0, :n], b["val"][0, n:2 * n])
    env.close()
    return K * P * n


@pytest.mark.parametrize("P,n", [(1, 1000), (3, 1000), (16, 4096), (5, 77)])
@pytest.mark.parametrize("philox", [False, True])
def test_rollout_is_bitwise_the_shards_rollouts(torch_cuda, P, n, philox):
    assert _check_rollout(torch_cuda, P, n, 8, philox) == 8 * P * n


def test_rollout_with_traffic_ships(torch_cuda):
    _check_rollout(torch_cuda, 2, 100, 8, False, env_kw={"n_ships": 4})


def test_rollout_with_three_frames_of_history(torch_cuda):
    _check_rollout(torch_cuda, 3, 77, 8, True, env_kw={"env_config": _env_config(3)})


def test_rollout_refuses_bad_populations(torch_cuda):
    torch = torch_cuda
    env = _vec(1000)
    pop = _population(torch, env.states_history, 3)
    with pytest.raises(ValueError, match="equal member slices"):
        env.rollout_population(pop, 4)
    with pytest.raises(ValueError, match="equal member slices"):
        env.population_act(pop)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# GAE and the update
# ------------------------------------------------------------------------------------------------------------------------------------
def _batches(torch, P, n, K, seed=7):
    """(env, pop, batch, shard envs, reference policies, shard batches): one population rollout and the P shard rollouts (asserted
    equal), then the same forced dones (terminations mid-rollout) and the same older-policy logp (ratios clipped on both sides) in both."""
    env, pop, b, shards, refs, sbs = shard_rollouts(torch, _vec, lambda D: _members(torch, D, P), [n] * P, K, seed)
    g = torch.Generator(device=DEV).manual_seed(P + n + K)
    forced = torch.rand(b["done"].shape, generator=g, device=DEV) < 0.05
    noise = (torch.rand(b["logp"].shape, generator=g, device=DEV) - 0.5) * 0.8
    for m, sb in enumerate(sbs):
        sb["done"] = (sb["done"] | forced[:, m * n:(m + 1) * n]).to(torch.uint8).contiguous()
        sb["logp"] = (sb["logp"] + noise[:, m * n:(m + 1) * n]).contiguous()
    b["done"] = (b["done"] | forced).to(torch.uint8).contiguous()
    b["logp"] = (b["logp"] + noise).contiguous()
    assert int(b["done"].sum()) > 0
    return env, pop, b, shards, refs, sbs


@pytest.mark.parametrize("P,n,K", [(3, 1000, 10), (5, 77, 8), (16, 4096, 8)])
def test_gae_is_bitwise_each_members_own(torch_cuda, P, n, K):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _batches(torch, P, n, K)
    gammas = [0.99 - 0.01 * (m % 3) for m in range(P)]
    lams = [0.9 + 0.1 * m / max(1, P - 1) for m in range(P)]           # 0.9 .. 1.0: every member its own lambda
    ppo = PopulationPPO(pop, env, gamma=gammas, lam=lams, adv_eps=[1e-8 * (1 + m) for m in range(P)])
    adv, ret = ppo.gae(b)
    stats = ppo.adv_stats().clone()
    for m in range(P):
        ref = NativePPO(refs[m], shards[m], adv_eps=1e-8 * (1 + m))
        r_adv, r_ret = ref.gae(sbs[m], gammas[m], lams[m])
        assert torch.equal(adv[:, m * n:(m + 1) * n], r_adv) and torch.equal(ret[:, m * n:(m + 1) * n], r_ret), m
        assert torch.equal(stats[m], ref.adv_stats()), (m, stats[m].tolist(), ref.adv_stats().tolist())
    assert len({float(s) for s in stats[:, 0]}) == P                       # per-member statistics, not one for the batch
    _close(env, shards)


def _check_update(torch, P, n, K, epochs, minibatch_counts):
    from ship_sim_gym_amd.ppo import chunk_split
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _batches(torch, P, n, K)
    hp = member_hparams(P)
    assert P < 2 or (hp["beta1"][1] <= 0.5 < hp["beta1"][0])               # both of lerp's branches run
    ppo = PopulationPPO(pop, env, **hp)
    ppo.gae(b)
    ref_ppos = [shard_reference(torch, m, hp, {}, refs, shards, sbs) for m in range(P)]
    samples = K * n
    g = torch.Generator(device=DEV).manual_seed(11)
    p0 = pop.params.clone()
    for i, mb in enumerate(minibatch_counts):
        chunk, n_chunks = chunk_split(samples, mb)
        perm = stacked_perms(torch, g, P, epochs, samples)
        step_before = ppo.step
        st = ppo.update(b, perm, epochs, mb, stats=True)
        assert st.shape == (P, epochs * n_chunks, 4) and bool(torch.isfinite(st).all())
        assert ppo.step == step_before + epochs * n_chunks
        for m in range(P):
            ref = ref_ppos[m]
            assert ref.step == step_before                                  # the same starting Adam step
            r_st = ref.update(sbs[m], perm[m], epochs, mb, stats=True)
            assert torch.equal(pop.params[m], refs[m].params), (i, mb, m, "params")
            assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (i, mb, m, "moments")
            assert torch.equal(st[m], r_st), (i, mb, m, "stats")
        if i == 0:  # again from the same start: bitwise the same
            first, first_mv = pop.params.clone(), ppo.adam_mv.clone()
            assert not torch.equal(first, p0)
            pop.params.copy_(p0)
            ppo.adam_mv.zero_()
            ppo.step = 0
            st2 = ppo.update(b, perm, epochs, mb, stats=True)
            assert torch.equal(pop.params, first) and torch.equal(ppo.adam_mv, first_mv) and torch.equal(st2, st)
    _close(env, shards)
    return samples


def test_update_is_bitwise_each_members_own(torch_cuda):
    """P = 3 x 1000 envs x K = 10: 10 000 samples per member into 4 chunks of 2 500 and into 6 chunks of 1 667 (the last 1 665) — chunk
    lengths that are no multiples of 64; the second update continues the first (step0 advanced)."""
    from ship_sim_gym_amd.ppo import chunk_split
    assert chunk_split(10000, 4) == (2500, 4) and chunk_split(10000, 6) == (1667, 6) and 2500 % 64 and 1667 % 64
    _check_update(torch_cuda, 3, 1000, 10, 2, [4, 6])


def test_update_with_fewer_chunks_than_asked(torch_cuda):
    """5 members x 77 envs (no multiple of 64, or of anything a workgroup likes) x K = 8: 616 samples per member.  Asked for 45
    minibatches, torch.chunk makes 44 chunks of 14; asked for 9, 9 chunks of 69 (the last 64)."""
    from ship_sim_gym_amd.ppo import chunk_split
    assert chunk_split(616, 45) == (14, 44) and chunk_split(616, 9) == (69, 9)
    _check_update(torch_cuda, 5, 77, 8, 1, [45, 9])


def test_update_of_sixteen_members(torch_cuda):
    _check_update(torch_cuda, 16, 4096, 8, 1, [4])


# ------------------------------------------------------------------------------------------------------------------------------------
# exploit, episode statistics, the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def test_exploit_copies_rows_and_the_destination_acts_as_its_source(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    P, n = 6, 100
    env = _vec(P * n)
    pop = _population(torch, env.states_history, P)
    ppo = PopulationPPO(pop, env)
    g = torch.Generator(device=DEV).manual_seed(2)
    ppo.adam_mv.copy_(torch.rand(ppo.adam_mv.shape, generator=g, device=DEV))
    env.reset_tensor()
    # identical observations and uniforms in every member's slice
    env.step_tensor(torch.ones(P * n, dtype=torch.int32, device=DEV))
    env.obs.copy_(env.obs[:n].repeat(P, 1))
    u = torch.rand(n, generator=g, device=DEV).repeat(P).contiguous()
    _, lp0, v0, _ = env.population_act(pop, uniforms=u)
    p0, mv0 = pop.params.clone(), ppo.adam_mv.clone()
    src = [0, 5, 2, 4, 4, 5]                                                # 1 <- 5, 3 <- 4; the others keep
    assert not torch.equal(lp0[n:2 * n], lp0[5 * n:]) and not torch.equal(v0[3 * n:4 * n], v0[4 * n:5 * n])
    ppo.exploit(src)
    for m, s in enumerate(src):
        assert torch.equal(pop.params[m], p0[s]) and torch.equal(ppo.adam_mv[m], mv0[s]), (m, s)
    _, lp1, v1, _ = env.population_act(pop, uniforms=u)
    for m, s in enumerate(src):
        assert torch.equal(lp1[m * n:(m + 1) * n], lp0[s * n:(s + 1) * n]) and torch.equal(v1[m * n:(m + 1) * n], v0[s * n:(s + 1) * n]), (m, s)
    assert torch.equal(pop.member(1).params, p0[5])                         # the member view IS the row
    from ship_sim_gym_amd._native import ShipSimError
    with pytest.raises(ShipSimError, match="chained"):
        ppo.exploit([0, 2, 3, 3, 4, 5])
    assert torch.equal(pop.params[1], p0[5]) and torch.equal(pop.params[2], p0[2])   # refused: nothing was launched
    env.close()


def test_episode_stats_match_a_forward_walk_and_the_handles_counters(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    P, n, K = 4, 250, 64
    env = _vec(P * n, env_config=_env_config(2, max_steps=40))               # K > max_steps: every env ends an episode per rollout
    pop = _population(torch, env.states_history, P)
    ppo = PopulationPPO(pop, env)
    env.reset_tensor()
    before = env.field_stats_tensor().cpu().numpy().copy()
    cum, length = np.zeros(P * n), np.zeros(P * n, dtype=np.int32)
    total = np.zeros((P, 3), dtype=np.int64)
    for r in range(3):
        b = env.rollout_population(pop, K, seed=9, step0=r * K)
        got = ppo.episode_stats(b).cpu().numpy()
        want, (cum, length) = episode_stats_walk(b["rew"].cpu().numpy(), b["done"].cpu().numpy(), cum, length, *layout([n] * P))
        assert np.array_equal(got, want), (r, got, want)
        assert (got[:, 2] >= n).all()                                       # every member finished episodes: nothing passes vacuously
        total += got
        assert np.array_equal(ppo.carry_length.cpu().numpy(), length) and np.array_equal(ppo.carry_return.cpu().numpy(), cum)
    assert int((length > 0).sum()) > 0                                      # episodes do span rollouts (the carry matters)
    after = env.field_stats_tensor().cpu().numpy()
    assert np.array_equal(total.sum(axis=0), (after - before)[:3]), (total.sum(axis=0), after - before)
    env.close()


def test_pbt_trainer_runs_exploits_and_is_reproducible(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/pbt_native.py")
    lines = []
    kw = dict(members=4, envs_per_member=512, updates=3, perturb_every=1, seed=0, return_details=True)
    hist, det = mod.train(log=lines.append, **kw)
    assert len(hist) == 3 and len(hist[0]) == 4
    assert len(det["exploits"]) >= 1 and any("exploit: member" in s for s in lines) and any("mutation: member" in s for s in lines)
    assert det["params"].shape[0] == 4 and bool(torch.isfinite(det["params"]).all())
    for ev in det["exploits"]:
        assert ev["member"] != ev["source"]
    _, again = mod.train(log=lambda s: None, **kw)
    assert torch.equal(det["params"], again["params"]) and det["hparams"] == again["hparams"]
    # the modules were loaded from the rows
    from ship_sim_gym_amd.policy import NativePolicy
    scale = torch.full((det["nets"][0].body[0].in_features,), 1000.0, dtype=torch.float64, device=DEV)
    for m, net in enumerate(det["nets"]):
        assert torch.equal(NativePolicy.from_actor_critic(net, scale).params, det["params"][m])
    # the learning-rate sweep: three members, no exploit
    hist, det = mod.train(members=3, envs_per_member=256, updates=2, lrs=[1e-3, 1e-4, 1e-5], pbt=False, log=lambda s: None, return_details=True)
    assert det["exploits"] == [] and det["hparams"]["lr"] == [1e-3, 1e-4, 1e-5] and bool(torch.isfinite(det["params"]).all())
