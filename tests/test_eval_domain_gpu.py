"""The evaluation loop and its recorder at the shapes the other modules never visit (ssg_evaluate, ssg_set_eval_recorder; eval_account_kernel
inside the loop, eval_record_obs_kernel, eval_record_step_kernel).  Real runs, compared bit for bit with the step-by-step oracle of
tests/eval_record_support.py walked by eval_walk / record_walk.

Settings: max_steps 5 (every env ends an episode at least every 5 steps), T = 12 steps, history 2, 8 beams.  Without a recorder:
N in {1, 65, 257} (one env; a wave and one lane; a workgroup and one lane) x E in {1, 2}, one call of 12 steps against twelve calls
of one.  With a recorder, on 257 envs: one slot tracking env 256 (the second workgroup's only lane) and all 64 slots on a fixed
permutation of envs that holds 0, 63, 64, 255 and 256, at the capacities 1, 5 and 12, with one small frame per slot (frame_every above
the capacity).  At capacity 1 every slot overflows."""
import numpy as np
import pytest

from eval_record_support import _assert_frames, _assert_record, _oracle, _recorder, _run, _walk
from gpu_support import DEV, env_config as _env_config, same_columns as _same_columns, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _shared_policy

pytestmark = pytest.mark.gpu

MAX_STEPS, T, N_REC, SIZE = 5, 12, 257, (33, 17)
_rest = [int(e) for e in np.random.RandomState(64).permutation(N_REC) if e not in (0, 63, 64, 255, 256)][:59]
IDS64 = [int(e) for e in np.random.RandomState(65).permutation([0, 63, 64, 255, 256] + _rest)]
assert len(set(IDS64)) == 64 and {0, 63, 64, 255, 256} <= set(IDS64) and IDS64 != sorted(IDS64)


def _vec(n):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, env_config=_env_config(2, MAX_STEPS), n_maps=64, n_beams=8)


def _policy(torch, D, seed=5):
    return _shared_policy(torch, D, 64, 2, "tanh", 3, seed)[1]


def _uniforms(torch, n):
    return torch.rand((T, n), generator=torch.Generator().manual_seed(3 + n)).to(DEV)


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_one_call_of_twelve_steps_is_twelve_calls_of_one_and_the_oracle(torch_cuda, n, greedy):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import eval_walk
    env, twin = _vec(n), _vec(n)
    pol = _policy(torch, env.states_history)
    u = _uniforms(torch, n)
    s, _ = _oracle(torch, env, pol, T, [], greedy, u)
    assert (s["done"] != 0).sum(axis=0).min() >= 2                                 # every env ends two episodes inside the run
    for E in (1, 2):
        rows, (ret, ci) = eval_walk(s["rew"], s["done"], s["flags"], E)
        assert (rows[:, 0] == E).all() and (ci[:, 2] == E).all()
        one = _run(env, pol, None, [T], greedy, u, episodes=E)
        many = _run(twin, pol, None, [1] * T, greedy, u, episodes=E)
        for ev in (one, many):
            assert np.array_equal(ev.env_stats.cpu().numpy(), rows), (n, E)
            assert np.array_equal(ev.carry.cpu().numpy(), ci) and ev.carry_return.cpu().numpy().tobytes() == ret.tobytes(), (n, E)
            assert np.array_equal(ev.reduce(1).cpu().numpy(), rows.sum(axis=0, keepdims=True))
        assert _same_columns(torch, env, twin) and torch.equal(env.obs, twin.obs), (n, E)
        for k in ("act", "logp", "value", "reward", "done", "flags"):    # the last step's rows
            assert torch.equal(getattr(one, k), getattr(many, k)), k
        assert np.array_equal(one.reward.cpu().numpy(), s["rew"][T - 1]) and np.array_equal(one.act.cpu().numpy(), s["act"][T - 1])
    env.close(); twin.close()


@pytest.fixture(scope="module")
def world(torch_cuda):
    """257 envs, a policy, the uniforms and the sampled oracle with the 64 tracked envs' screens at every step."""
    torch = torch_cuda
    env = _vec(N_REC)
    pol = _policy(torch, env.states_history)
    u = _uniforms(torch, N_REC)
    s, screens = _oracle(torch, env, pol, T, IDS64, False, u, sizes=(SIZE,), debugs=(True,))
    yield {"env": env, "pol": pol, "u": u, "s": s, "screens": screens[(SIZE, True)]}
    env.close()


@pytest.mark.parametrize("capacity", [1, 5, 12])
@pytest.mark.parametrize("slots", ["env256", "all64"])
def test_record_at_the_slot_limits_equals_the_oracle(torch_cuda, world, slots, capacity):
    from ship_sim_gym_amd.evaluate import eval_walk
    env, s, E = world["env"], world["s"], 2
    ids = [256] if slots == "env256" else IDS64
    screens = world["screens"][:, [IDS64.index(e) for e in ids]]
    rec = _recorder(env, ids=ids, capacity=capacity, frames=SIZE, frame_every=capacity + 1)
    assert tuple(rec.frames.shape) == (len(ids), 1, SIZE[0], SIZE[1], 3)
    ev = _run(env, world["pol"], rec, [T], False, world["u"], episodes=E)
    want = _walk(s, ids, E, capacity)
    got = rec.numpy()
    print(slots, "capacity", capacity, "cursor", got["cursor"][:8], "overflow", got["overflow"][:8])
    _assert_record(got, want)
    _assert_frames(got, want, screens, capacity + 1)
    assert (want["counted"][ids] == E).all()                                # every tracked env ran into its quota inside the run
    if capacity == 1:    # a full slot of an env that still counts: every counted step but the first overflows
        assert (want["cursor"] == 1).all() and (want["overflow"] >= E - 1).all() and want["overflow"].max() > E
    if capacity == 12:   # two episodes of at most five steps fit
        assert not want["overflow"].any() and (want["cursor"] < 12).all() and (want["cursor"] >= E).all()
    assert np.array_equal(ev.env_stats.cpu().numpy(), eval_walk(s["rew"], s["done"], s["flags"], E)[0])
