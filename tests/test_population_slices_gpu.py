"""GPU checks of per-member batch sizes: a population on unequal env slices (ssg_pop_set_slices; ShipVecEnv.set_population_slices,
PopulationPPO, NativeEvaluator, train/pbt_native.py --mutate-batch).  The reference of every check is the single-policy path: member
m is ``NativePolicy`` / ``NativePPO`` on a ``ShipVecEnv(n_m, n_maps=64, env_id_base=o_m)`` shard, and every comparison is torch.equal
(the idiom of tests/test_population_sched_gpu.py).

The base layout is P = 4 with (1, 63, 64, 257) envs and K = 5: a one-env member, slices below and exactly at the policy tile of 64,
one that crosses a 256-env GAE block, and member bases 1, 64 and 128 (an unaligned and two aligned ones)."""
import ctypes as C

import numpy as np
import pytest

from accounting_support import episode_stats_walk
from gpu_support import DEV, load_script, vec as split_vec
from gpu_support import torch_cuda  # noqa: F401
from population_harness import ROLLOUT_KEYS, age, cached, member_hparams as _hp, perms_per_member as _perms, shard_reference as _reference, \
    shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy, split_policy

pytestmark = pytest.mark.gpu

SPLIT_SHAPE = (22, 48, 2, 3, "tanh")  # D, H, layers, A, activation of the separate-value population
SIZES, K = (1, 63, 64, 257), 5


def _offsets(sizes):
    return [sum(sizes[:m]) for m in range(len(sizes))]


def _vec(n, base=0, split=False, **kw):
    if split:
        return split_vec(n, SPLIT_SHAPE[0], base=base)
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64, env_id_base=base, **kw)


def _members(torch, D, P, split, seed=100):
    if split:
        _, H, L, A, act = SPLIT_SHAPE
        return [split_policy(torch, D, H, L, act, A, seed=seed + m)[1] for m in range(P)]
    return [actor_critic_policy(torch, D, seed=seed + m)[1] for m in range(P)]


def _setup(torch, sizes, K, split=False):
    """(env with `sizes` bound, pop, batch, shard envs, reference policies, shard batches), computed once per shape and left unchanged.
    The rollout — every ROLLOUT_KEYS column slice and last_val — is asserted equal to the shards' here; then the same forced dones and
    the same older acting policy (noise on its log-distribution and value) go into both."""
    def make_env(n, base):
        env = _vec(n, base, split)
        if n == sum(sizes):                                                 # the population's handle
            env.set_population_slices(sizes)
            assert env.population_slices == list(sizes)
        return env

    def make():
        P, N = len(sizes), sum(sizes)
        setup = shard_rollouts(torch, make_env, lambda D: _members(torch, D, P, split), sizes, K, 7)
        env, pop, b, shards, refs, sbs = setup
        age(torch, b, sbs, sizes, pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(P * 1000 + N + K), True)
        return setup
    return cached((tuple(sizes), K, split), make)


# ------------------------------------------------------------------------------------------------------------------------------------
# rollout, acting, GAE
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["shared", "split"])
def test_rollout_and_acting_are_each_members_own_shard(torch_cuda, split):
    """The rollout comparison is _setup's; here the one-launch acts on the envs as the rollout left them: greedy, and sampled with the
    Philox counter on the GLOBAL env id."""
    torch = torch_cuda
    env, pop, b, shards, refs, sbs = _setup(torch, SIZES, K, split)
    greedy = env.population_act(pop, greedy=True)
    sampled = env.population_act(pop, seed=3, step=9)
    for m, (o, n) in enumerate(zip(_offsets(SIZES), SIZES)):
        for got, want in ((greedy, shards[m].policy_act(refs[m], greedy=True)), (sampled, shards[m].policy_act(refs[m], seed=3, step=9))):
            for i, (gt, wt) in enumerate(zip(got, want)):
                assert gt.dtype == wt.dtype and torch.equal(gt[o:o + n], wt), (m, i)
    assert len(set(sampled[0].tolist())) > 1


def test_gae_and_statistics_are_each_members_own(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _setup(torch, SIZES, K)
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    P, hp = len(SIZES), _hp(len(SIZES))
    ppo = PopulationPPO(pop, env, **hp)
    adv, ret = ppo.gae(b)
    stats = ppo.adv_stats().clone()
    assert stats.shape == (P, 3)
    for m, (o, n) in enumerate(zip(_offsets(SIZES), SIZES)):
        ref = _reference(torch, m, hp, {}, refs, shards, sbs)
        assert torch.equal(adv[:, o:o + n], sbs[m]["adv"]) and torch.equal(ret[:, o:o + n], sbs[m]["ret"]), m
        assert torch.equal(stats[m], ref.adv_stats()), (m, stats[m].tolist(), ref.adv_stats().tolist())   # divided by K * n_m
    with pytest.raises(ValueError):
        ppo.envs_per_member
    assert ppo.minibatches_for_size(64, member=3) == -(-K * 257 // 64) and ppo.minibatches_for_size(64, member=0) == 1


# ------------------------------------------------------------------------------------------------------------------------------------
# the update
# ------------------------------------------------------------------------------------------------------------------------------------
EXT4 = {"vf_clip": [10.0, 0.05, 0.0, 0.2], "max_grad_norm": [0.0, 0.03, 0.0, 0.5], "kl_coef": [1.0, 0.0, 0.0, 0.5],
        "kl_target": [1e-4, 0.0, 0.0, 10.0]}     # RLlib's loss; PPO2's; everything off; everything on with a target far above the KL
ROUNDS = [(2, 4),                                # common epochs and minibatches (member 0: its 5 samples in chunks of 2, 2, 1)
          ([1, 2, 3, 2], [1, 4, 5, 16])]         # per-member lists: every count is within the member's samples (5, 315, 320, 1285)


def _check_rounds(torch, setup, ext):
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import chunk_split
    env, pop, b, shards, refs, sbs = setup
    P = len(pop)
    samples = [K * n for n in SIZES]
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    hp = _hp(P)
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, **hp, **ext)
        ppo.gae(b)
        ref_ppos = [_reference(torch, m, hp, ext, refs, shards, sbs) for m in range(P)]
        cols = 8 if ppo.extended() else 4
        g = torch.Generator(device=DEV).manual_seed(11)
        for r, (epochs, minibatches) in enumerate(ROUNDS):
            ep = epochs if isinstance(epochs, list) else [epochs] * P
            mb = minibatches if isinstance(minibatches, list) else [minibatches] * P
            steps = [e * chunk_split(s, c)[1] for e, c, s in zip(ep, mb, samples)]
            perm = _perms(torch, g, max(ep), samples)
            before = list(ppo.member_steps)
            flat = torch.cat([q.reshape(-1) for q in perm])
            st = ppo.update(b, perm if r == 0 else flat, epochs, minibatches, stats=True)   # the list of P tensors, then the flat buffer
            assert st.shape == (P, max(steps), cols) and bool(torch.isfinite(st).all())
            assert ppo.member_steps == [s0 + s for s0, s in zip(before, steps)]
            for m in range(P):
                ref = ref_ppos[m]
                assert ref.step == before[m], (r, m)
                r_st = ref.update(sbs[m], perm[m][:ep[m]].contiguous(), ep[m], mb[m], stats=True)
                assert r_st.shape[0] == steps[m] and ref.step == ppo.member_steps[m], (r, m)
                assert torch.equal(pop.params[m], refs[m].params), (r, m, "params")
                assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (r, m, "moments")
                assert torch.equal(st[m, :steps[m], :r_st.shape[1]], r_st), (r, m, "stats")
                assert bool((st[m, steps[m]:] == 0).all()), (r, m, "rows past the member's steps")
                assert torch.equal(ppo.kl_coef[m:m + 1], ref.kl_coef), (r, m, "coefficient", ppo.kl_coef.tolist(), ref.kl_coef.tolist())
        assert not torch.equal(pop.params, saved[0])
        return ppo
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_update_on_unequal_slices_is_bitwise_each_members_own(torch_cuda, ext):
    torch = torch_cuda
    ppo = _check_rounds(torch, _setup(torch, SIZES, K), EXT4 if ext else {})
    assert ppo.extended() == ext and ppo.diverged()
    if ext:
        assert ppo.kl_coef.tolist() != EXT4["kl_coef"]                                  # the coefficients were adapted, per member


def test_update_on_unequal_slices_with_a_separate_value_network(torch_cuda):
    torch = torch_cuda
    setup = _setup(torch, SIZES, K, split=True)
    assert setup[1].separate_value
    _check_rounds(torch, setup, EXT4)


# ------------------------------------------------------------------------------------------------------------------------------------
# equal slices bound = nothing bound
# ------------------------------------------------------------------------------------------------------------------------------------
def test_equal_slices_bound_change_nothing(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    P, n, K4 = 3, 70, 4
    results = []
    for bound in (False, True):
        env = _vec(P * n)
        if bound:
            env.set_population_slices([n] * P)
        pop = NativePopulation(_members(torch, env.states_history, P, False))
        env.reset_tensor()
        b = dict(env.rollout_population(pop, K4, seed=7))
        ppo = PopulationPPO(pop, env, **_hp(P), **{k: v[:P] for k, v in EXT4.items()})
        assert ppo.envs_per_member == n and ppo.member_envs == [n] * P
        eps = ppo.episode_stats(b).clone()
        g = torch.Generator(device=DEV).manual_seed(3)
        b["done"] = (b["done"] | (torch.rand((K4, P * n), generator=g, device=DEV) < 0.05)).to(torch.uint8).contiguous()
        eps2 = ppo.episode_stats(b).clone()
        adv, ret = ppo.gae(b)
        stats = ppo.adv_stats().clone()
        la = ppo.dist(b).clone()
        perm = stacked_perms(torch, g, P, 3, K4 * n)
        st = ppo.update(b, [perm[m] for m in range(P)] if bound else perm, [1, 3, 2], [4, 1, 5], stats=True)
        act = env.population_act(pop, seed=1, step=2)
        ev = NativeEvaluator(env)
        ev.run(pop, 1, 6, greedy=True)
        red = ev.reduce(P).clone()
        results.append([b[k] for k in ROLLOUT_KEYS] + [b["last_val"], eps, eps2, adv, ret, stats, la, st, pop.params.clone(), ppo.adam_mv.clone(),
                                                       ppo.kl_coef.clone(), *act, ev.env_stats.clone(), red, env.obs.clone()])
        assert ppo.member_steps == [4, 3, 10]
        if bound:                                                                       # after unbinding the equal-slice calls work again
            env.set_population_slices(None)
            assert env.population_slices is None
            again = env.population_act(pop, greedy=True)
            ppo.update(b, perm[:, :1].contiguous(), 1, 2)
            assert bool(torch.isfinite(again[1]).all()) and ppo.member_steps == [6, 5, 12]
        env.close()
    assert len(results[0]) == len(results[1])
    for i, (a, c) in enumerate(zip(*results)):
        assert a.dtype == c.dtype and a.shape == c.shape and torch.equal(a, c), i


# ------------------------------------------------------------------------------------------------------------------------------------
# episode statistics and evaluation on the unequal layout
# ------------------------------------------------------------------------------------------------------------------------------------
def _short_episodes(max_steps):
    from ship_sim_gym_amd.config import EnvConfig

    class E(EnvConfig):
        MAX_STEPS = max_steps
    return E


def test_episode_stats_sum_each_members_own_columns(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    P, N, KK = len(SIZES), sum(SIZES), 48
    env = _vec(N, env_config=_short_episodes(40))                          # KK > max_steps: every env ends an episode per rollout
    env.set_population_slices(SIZES)
    pop = NativePopulation(_members(torch, env.states_history, P, False))
    ppo = PopulationPPO(pop, env)
    env.reset_tensor()
    cum, length = np.zeros(N), np.zeros(N, dtype=np.int32)
    for r in range(2):
        b = env.rollout_population(pop, KK, seed=9, step0=r * KK)
        got = ppo.episode_stats(b).cpu().numpy()
        want, (cum, length) = episode_stats_walk(b["rew"].cpu().numpy(), b["done"].cpu().numpy(), cum, length, _offsets(SIZES), SIZES)
        assert np.array_equal(got, want), (r, got, want)
        assert (got[:, 2] >= np.array(SIZES)).all()                         # every member finished episodes, the one-env member too
        assert np.array_equal(ppo.carry_length.cpu().numpy(), length) and np.array_equal(ppo.carry_return.cpu().numpy(), cum)
    env.close()


def test_evaluation_on_unequal_slices(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator, eval_walk
    from ship_sim_gym_amd.population import NativePopulation
    P, N, E, T = len(SIZES), sum(SIZES), 2, 50
    a, c = _vec(N, env_config=_short_episodes(20)), _vec(N, env_config=_short_episodes(20))
    a.set_population_slices(SIZES)
    c.set_population_slices(SIZES)
    pop = NativePopulation(_members(torch, a.states_history, P, False))
    ev = NativeEvaluator(a)
    a.reset_tensor()
    c.reset_tensor()
    ev.run(pop, E, T, greedy=False, seed=9, step0=3)                        # ssg_pop_evaluate on the slices
    r = c.rollout_population(pop, T, seed=9, step0=3)                       # ... against the recorded rollout, walked in numpy
    want, _ = eval_walk(r["rew"].cpu().numpy(), r["done"].cpu().numpy(), r["flags"].cpu().numpy(), E)
    rows = ev.env_stats.cpu().numpy()
    assert np.array_equal(rows, want) and int(want[:, 0].min()) >= 1
    per_member = np.stack([want[o:o + n].sum(0) for o, n in zip(_offsets(SIZES), SIZES)])
    assert np.array_equal(ev.reduce(P).cpu().numpy(), per_member)
    assert np.array_equal(ev.reduce(1).cpu().numpy(), want.sum(0, keepdims=True))      # one policy's reduce: the whole handle
    res = ev.evaluate(pop, E, greedy=False, seed=9, step0=3, max_steps=T, chunk=25)     # resets, runs the same T steps in two calls
    assert np.array_equal(res["per_member"].cpu().numpy(), per_member) and res["steps"] in (25, T)
    assert res["per_member"][0, 0].item() == E                              # the one-env member counted exactly its quota
    with pytest.raises(ValueError):
        ev.reduce(2)
    a.close()
    c.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_leave_the_buffers_untouched(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as NV
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    env, pop, b, shards, refs, sbs = _setup(torch, SIZES, K)
    L, h, N, P = NV.lib(), env._h, sum(SIZES), len(SIZES)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    # sizes that do not sum to N: refused, and the binding stays as it was
    for bad in ((1, 63, 64, 256), (1, 63, 64, 258), (0, 64, 64, 257)):
        with pytest.raises((ValueError, NV.ShipSimError)):
            env.set_population_slices(bad)
        assert env.population_slices == list(SIZES)
    # a population of another P while slices are bound (385 = 5 x 77 would split equally)
    pop5 = NativePopulation(_members(torch, env.states_history, 5, False))
    with pytest.raises(ValueError):
        env.population_act(pop5)
    rec5 = pop5.to_native()
    act = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    logp, val = torch.full((N,), -7.0, device=DEV), torch.full((N,), -7.0, device=DEV)
    assert L.ssg_pop_act(h, C.byref(rec5), vp(env.obs), None, 0, 0, vp(act), vp(logp), vp(val), None, stream) == -1
    assert b"slices for 4 members are bound" in L.ssg_last_error(h)
    assert L.ssg_pop_act_greedy(h, C.byref(rec5), vp(env.obs), vp(act), vp(logp), vp(val), None, stream) == -1
    la = torch.full((K, N, 4), -7.0, device=DEV)
    assert L.ssg_pop_dist(h, C.byref(rec5), K, vp(b["obs"]), vp(la), stream) == -1
    out3 = torch.full((5, 3), -7, dtype=torch.int64, device=DEV)
    cr, cl = torch.zeros(N, dtype=torch.float64, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    assert L.ssg_pop_episode_stats(h, 5, K, vp(b["rew"]), vp(b["done"]), vp(cr), vp(cl), vp(out3), stream) == -1
    es, ms = torch.zeros((N, 8), dtype=torch.int64, device=DEV), torch.full((5, 8), -7, dtype=torch.int64, device=DEV)
    assert L.ssg_eval_reduce(h, 5, vp(es), vp(ms), stream) == -1
    torch.cuda.synchronize()
    assert bool((act == -7).all()) and bool((logp == -7).all()) and bool((val == -7).all()) and bool((la == -7).all())
    assert bool((out3 == -7).all()) and bool((ms == -7).all()) and int(cl.sum()) == 0
    # ssg_pop_update / ssg_pop_update_ext while slices are bound: the update runs through ssg_pop_update_sched only
    ppo = PopulationPPO(pop, env)
    bb = dict(b)
    ppo.gae(bb)
    params, mv, ws = pop.params.clone(), ppo.adam_mv.clone(), ppo.workspace.clone()
    table = ppo._table(8)
    perm = torch.zeros((P, 1, K * 257), dtype=torch.int64, device=DEV)
    rec = pop.to_native()
    cols = [vp(bb["obs"]), vp(bb["act"]), vp(bb["logp"]), vp(bb["adv"]), vp(bb["ret"])]
    ppo._ws(K * 257, K * 257)
    ws = ppo.workspace.clone()
    assert L.ssg_pop_update(h, C.byref(rec), vp(table), 8, K, *cols, vp(perm), 1, 1, vp(ppo.adam_mv), None, vp(ppo.workspace),
                            ppo.workspace.numel(), stream) == -1
    assert b"ssg_pop_update_sched" in L.ssg_last_error(h)
    ext, ext_table = ppo._ext(bb, K, N)
    assert L.ssg_pop_update_ext(h, C.byref(rec), C.byref(ext), vp(table), 8, K, *cols, vp(perm), 1, 1, vp(ppo.adam_mv), None, vp(ppo.workspace),
                                ppo.workspace.numel(), stream) == -1
    torch.cuda.synchronize()
    assert torch.equal(pop.params, params) and torch.equal(ppo.adam_mv, mv) and torch.equal(ppo.workspace, ws)
    # K * n_m < 2 for the one-env member
    b1 = dict(env.rollout_population(pop, 1, seed=7))
    ws = ppo.workspace.clone()
    with pytest.raises(NV.ShipSimError, match="every member"):
        ppo.gae(b1)
    torch.cuda.synchronize()
    assert torch.equal(ppo.workspace, ws) and "adv" not in b1


# ------------------------------------------------------------------------------------------------------------------------------------
# train/pbt_native.py --mutate-batch
# ------------------------------------------------------------------------------------------------------------------------------------
def _seed_that_reslices(mod, P, n_envs, quantum):
    """The first seed whose first perturbation changes the slices WHOEVER ranks bottom and top — found on the CPU from the scheduler
    alone: the scheduler's draws do not depend on which members they are for."""
    from ship_sim_gym_amd.population import PBTScheduler, reference_mutations, slices_for_batch_sizes
    for seed in range(200):
        sched = PBTScheduler(P, seed=seed, perturbation_interval=1, mutations=reference_mutations(batch=True))
        batch = mod.initial_batch_sizes(sched, P)
        base = slices_for_batch_sizes(batch, n_envs, quantum)
        state = sched.rng.getstate()
        hp = {"lambda": [0.95] * P, "clip_param": [0.2] * P, "lr": [5e-4] * P, "train_batch_size": batch}
        changed = True
        for lo in range(P):
            for hi in range(P):
                if lo == hi:
                    continue
                sched.rng.setstate(state)
                scores = [1.0] * P
                scores[lo], scores[hi] = 0.0, 2.0
                src, new, events = sched.perturb(scores, hp)
                assert src[lo] == hi and len(events) == 1
                changed = changed and slices_for_batch_sizes(new["train_batch_size"], n_envs, quantum) != base
        if changed:
            return seed
    raise AssertionError("no seed re-slices")


def test_pbt_trainer_mutates_the_batch_and_reslices(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/pbt_native.py")
    P, n_envs, quantum = 4, 256, 16
    seed = _seed_that_reslices(mod, P, n_envs, quantum)
    lines = []
    hist, det = mod.train(members=P, envs=n_envs, quantum=quantum, horizon=4, updates=3, perturb_every=1, seed=seed, mutate_batch=True,
                          log=lines.append, return_details=True)
    assert len(hist) == 3 and len(hist[0]) == P
    assert len(det["exploits"]) >= 1
    sizes = [s for _, s in det["reslices"]]
    assert len(sizes) == 1 + 3 and det["reslices"][0][0] == 0                           # the initial layout, then one per perturbation
    assert all(len(s) == P and sum(s) == n_envs and min(s) >= quantum and all(x % quantum == 0 for x in s) for s in sizes)
    assert sizes[1] != sizes[0]                                                         # the first perturbation re-sliced the handle
    assert det["slices"] == sizes[-1]
    assert sum("re-slice: train_batch_size" in s for s in lines) == 3 and any(s.startswith("slices: train_batch_size") for s in lines)
    assert any("mutation: member" in s and "train_batch_size" in s for s in lines)
    assert det["params"].shape[0] == P and bool(torch.isfinite(det["params"]).all())
    assert all(isinstance(v, int) and v >= 1 for v in det["train_batch_size"])
