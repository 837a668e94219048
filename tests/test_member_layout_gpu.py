"""The launches whose member layout no other GPU test compares bit for bit with the member's own single-policy run on its shard: the
episode statistics, the evaluation reduce, the stand-alone observation-filter update, and the return filter both updating and frozen —
each on unequal and on equal slices.  (Acting, rollouts, time-out values, dist, GAE, permutations and the update have such tests
already; the matrix is in profiles/member_layout/README.md.)

Set-up and shapes are test_population_slices_gpu.py's: slices (1, 63, 64, 257) of 385 envs, K = 5 — the widest slice needs two 256-env
blocks where the equal split of 385 / 4 would get one, member 0 has a single env — and the same 385 envs and rollout data split equally
among 5 members of 77.  Output buffers hold NaN (a sentinel where they are integers) before the call, so a row no workgroup served
shows."""
import ctypes as C

import pytest

import test_population_slices_gpu as S
from gpu_support import DEV
from gpu_support import torch_cuda  # noqa: F401
from population_harness import close_cached, cols  # noqa: F401

pytestmark = pytest.mark.gpu

K = S.K
LAYOUTS = {"unequal": S.SIZES, "equal": (77,) * 5}


def rows(t, m, sizes):
    """Member m's env rows of an [N, ...] tensor."""
    o = sum(sizes[:m])
    return t[o:o + sizes[m]]


@pytest.fixture(scope="module")
def layouts(torch_cuda):
    """kind -> (the population's handle, the members' sizes, their shard handles, a population of that many members, its members alone,
    the rollout's rew and done with forced dones): test_population_slices_gpu's set-up, and for the equal split fresh handles of the
    same 385 envs, on which only these calls ever run."""
    torch = torch_cuda
    env, pop, b, shards, refs, sbs = S._setup(torch, S.SIZES, K)
    rew, done = b["rew"].contiguous(), b["done"].contiguous()
    sizes = LAYOUTS["equal"]
    eq, eq_shards = S._vec(sum(sizes)), [S._vec(n, sum(sizes[:m])) for m, n in enumerate(sizes)]
    from ship_sim_gym_amd.population import NativePopulation
    eq_refs = S._members(torch, eq.states_history, len(sizes), False)
    yield {"unequal": (env, S.SIZES, shards, pop, refs, rew, done), "equal": (eq, sizes, eq_shards, NativePopulation(eq_refs), eq_refs, rew, done)}
    for e in [eq] + eq_shards:
        e.close()


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_episode_stats_are_each_members_single_member_call(torch_cuda, layouts, kind):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    env, SIZES, shards, pop, refs, rew, done = layouts[kind]                 # (forced dones: episodes end mid-rollout)
    P = len(SIZES)
    ppo = PopulationPPO(pop, env)
    ones = [PopulationPPO(NativePopulation([refs[m]]), shards[m]) for m in range(P)]
    for r in range(2):                                                      # the second call continues the carries
        got = ppo.episode_stats({"rew": rew, "done": done}).clone()
        for m in range(P):
            one = ones[m].episode_stats({"rew": cols(rew, m, SIZES).contiguous(), "done": cols(done, m, SIZES).contiguous()})
            assert torch.equal(got[m:m + 1], one), (r, m)
            assert torch.equal(cols(ppo.carry_return, m, SIZES), ones[m].carry_return), (r, m)
            assert torch.equal(cols(ppo.carry_length, m, SIZES), ones[m].carry_length), (r, m)
    assert int(got[:, 2].sum()) > 0


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_eval_reduce_is_each_members_whole_handle_reduce(torch_cuda, layouts, kind):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    env, SIZES, shards = layouts[kind][:3]
    P = len(SIZES)
    ev = NativeEvaluator(env)
    g = torch.Generator(device=DEV).manual_seed(5)
    ev.env_stats.copy_(torch.randint(-1000, 1000, tuple(ev.env_stats.shape), generator=g, device=DEV))
    ev.member_stats.fill_(-7)
    got = ev.reduce(P).clone()
    assert bool((ev.member_stats[P:] == -7).all())
    for m in range(P):
        one = NativeEvaluator(shards[m])
        one.env_stats.copy_(rows(ev.env_stats, m, SIZES))
        one.member_stats.fill_(-7)
        assert torch.equal(got[m:m + 1], one.reduce(1)), m
    ev.member_stats.fill_(-7)                                               # one policy's reduce: the whole handle, whatever is bound
    assert torch.equal(ev.reduce(1)[0], ev.env_stats.sum(0))


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_obs_filter_update_is_each_members_single_filter(torch_cuda, layouts, kind):
    torch = torch_cuda
    from ship_sim_gym_amd.obs_filter import ObsFilter
    env, SIZES, shards = layouts[kind][:3]
    P = len(SIZES)
    flt = ObsFilter(env, n_members=P)
    ones = [ObsFilter(shards[m]) for m in range(P)]
    g = torch.Generator(device=DEV).manual_seed(6)
    for r in range(2):                                                      # the second batch merges into the first one's state
        obs = (torch.rand((sum(SIZES), env.states_history), generator=g, device=DEV, dtype=torch.float64) * 600.0).contiguous()
        flt.update(obs)
        for m in range(P):
            ones[m].update(rows(obs, m, SIZES).contiguous())
            assert torch.equal(flt.state[m], ones[m].state[0]), (r, m)
    assert flt.count.tolist() == [2.0 * n for n in SIZES]


def _apply(torch, flt, rew, done):
    """ReturnFilter.normalise's call on buffers that hold NaN before it."""
    from ship_sim_gym_amd import _native as N
    env, n = flt.env, flt.env.num_envs
    out = torch.full((K, n), float("nan"), dtype=torch.float64, device=DEV)
    den = torch.full((K, flt.n_members), float("nan"), dtype=torch.float64, device=DEV)
    rec = flt.to_native(K)
    N.check(N.lib().ssg_ret_filter_apply(env._h, C.byref(rec), K, C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), n,
                                         C.c_void_p(out.data_ptr()), C.c_void_p(den.data_ptr()), env._stream()), env._h, "ssg_ret_filter_apply")
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(den).any())
    return out, den


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_return_filter_updating_and_frozen_is_each_members_single_filter(torch_cuda, layouts, kind):
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    env, SIZES, shards, _, _, rew, done = layouts[kind]
    P = len(SIZES)
    gammas = [0.9 + 0.02 * m for m in range(P)]
    flt = ReturnFilter(env, n_members=P, gamma=gammas, clip=4.0)
    ones = [ReturnFilter(shards[m], gamma=gammas[m], clip=4.0) for m in range(P)]
    for updating in (True, True, False):                                    # two merging calls, then the frozen one on their state
        flt.train(updating)
        state0, carry0 = flt.state.clone(), flt.carry.clone()
        out, den = _apply(torch, flt, rew, done)
        assert torch.equal(flt.state, state0) != updating and (updating or torch.equal(flt.carry, carry0))
        for m in range(P):
            ones[m].train(updating)
            so, sd = _apply(torch, ones[m], cols(rew, m, SIZES).contiguous(), cols(done, m, SIZES).contiguous())
            assert torch.equal(cols(out, m, SIZES), so) and torch.equal(den[:, m], sd[:, 0]), (updating, m)
            assert torch.equal(flt.state[m], ones[m].state[0]) and torch.equal(cols(flt.carry, m, SIZES), ones[m].carry), (updating, m)
