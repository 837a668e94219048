"""The evaluation recorder on the device (ssg_set_eval_recorder, ssg_render_envs; ship_sim_gym_amd/evaluate.py EvalRecorder) against its
own step-by-step restatement: the public one-step calls in a Python loop from the same reset — clone env.obs, get_screen for the
tracked envs, policy_act, step_tensor with terminal observations on — walked by record_walk and eval_walk.  The oracle runs the same
kernels, so every comparison is bit for bit.

Shapes: 256 envs (two workgroups of the accounting kernel), 8 beams, history 2, max_steps 7 (every env ends an episode at least
every 7 steps), E = 3 episodes, T = 32 steps, five tracked envs [255, 0, 64, 65, 130] (unsorted; first and last env, two neighbours
of one wave, one env of the second workgroup), capacity 32."""
import ctypes as C

import numpy as np
import pytest

from eval_record_support import CAP, E, IDS, SENT, SENT_PIX, _assert_frames, _assert_record, _oracle, _recorder, _run, _walk
from gpu_support import DEV, env_config as _env_config, same_columns as _same_columns, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _shared_policy

pytestmark = pytest.mark.gpu

N_ENVS, MAX_STEPS, T = 256, 7, 32
SIZES = ((33, 17), (130, 3))            # the second crosses a 128-pixel block edge


def _vec(n=N_ENVS, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    kw.setdefault("n_maps", 64)
    kw.setdefault("n_beams", 8)
    return ShipVecEnv(n, env_config=_env_config(kw.pop("history", 2), kw.pop("max_steps", MAX_STEPS)), **kw)


def _policy(torch, D, seed=5):
    return _shared_policy(torch, D, 64, 2, "tanh", 3, seed)[1]


@pytest.fixture(scope="module")
def world(torch_cuda):
    """One env, one policy, the uniforms, and the two oracles (sampled with every frame variant, greedy without frames)."""
    torch = torch_cuda
    env = _vec()
    pol = _policy(torch, env.states_history)
    u = torch.rand((T, N_ENVS), generator=torch.Generator().manual_seed(3)).to(DEV)
    sampled, screens = _oracle(torch, env, pol, T, IDS, False, u, sizes=SIZES)
    greedy, _ = _oracle(torch, env, pol, T, IDS, True)
    w = {"env": env, "pol": pol, "u": u, "sampled": sampled, "greedy": greedy, "screens": screens}
    yield w
    env.close()


@pytest.mark.parametrize("mode", ["sampled", "greedy"])
def test_record_equals_the_step_by_step_oracle(torch_cuda, world, mode, native):
    from ship_sim_gym_amd.evaluate import eval_walk
    env, s = world["env"], world[mode]
    rec = _recorder(env)
    ev = _run(env, world["pol"], rec, [T], mode == "greedy", world["u"])
    want = _walk(s, IDS, E, CAP)
    got = rec.numpy()
    print(mode, "cursor", got["cursor"], "overflow", got["overflow"], "dones kept", [int(got["done"][r, :n].sum()) for r, n in enumerate(got["cursor"])])
    _assert_record(got, want)
    assert np.array_equal(rec.steps, want["cursor"]) and np.array_equal(rec.overflow, want["overflow"])
    # conditions on the inputs: every slot counted its E episodes before the run ended (at 7 steps an episode it is the clock that
    # ends them: episodes that end sooner are test_record_of_episodes_that_end_ahead_of_the_clock's)
    assert (want["counted"][IDS] == E).all() and (want["cursor"] < T).all() and not want["overflow"].any()
    assert int(s["done"].sum()) > 0
    rows, _ = eval_walk(s["rew"], s["done"], s["flags"], E)
    stats = ev.env_stats.cpu().numpy()
    assert np.array_equal(stats, rows)
    # the return check: llrint(100 * the sum of an episode's rewards in order), summed per env, is the env's stats column 1
    for r, eps in enumerate(rec.episodes()):
        assert len(eps) == E and all(ep["complete"] for ep in eps)
        total = 0
        for ep in eps:
            ret = 0.0
            for x in ep["reward"]:
                ret += float(x)
            total += int(np.rint(ret * 100.0))
        assert total == stats[IDS[r], native.EVAL_RETURN100] and stats[IDS[r], native.EVAL_EPISODES] == E
        assert sum(len(ep["act"]) for ep in eps) == stats[IDS[r], native.EVAL_LENGTH]
    ro = rec.as_rollouts()
    assert len(ro) == E * len(IDS) and np.array_equal(ro[0][0][0], s["obs"][0, IDS[0]]) and ro[0][-1][4] is True


def test_record_of_episodes_that_end_ahead_of_the_clock(torch_cuda, native):
    """max_steps 40, 100 steps of a uniform policy: collisions and leaving the bounds end episodes before the clock does.  The
    tracked envs are the first five whose FIRST episode ends that way (read from the oracle, which runs first), so the terminal
    observation of a true terminal state is among the kept rows."""
    torch = torch_cuda
    from ship_sim_gym_amd.policy import NativePolicy
    steps, E2 = 100, 2
    env = _vec(max_steps=40)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    pol = NativePolicy([(z(16, env.states_history), z(16))], (z(3, 16), torch.full((3,), 0.5, device=DEV)), (z(1, 16), z(1)), 600.0)
    u = torch.rand((steps, N_ENVS), generator=torch.Generator().manual_seed(7)).to(DEV)
    s, _ = _oracle(torch, env, pol, steps, [], False, u)
    early = []
    for e in range(N_ENVS):
        ends = np.flatnonzero(s["done"][:, e])
        if len(ends) and not (s["flags"][ends[0], e] & native.EV_MAX_STEPS):
            early.append(e)
    assert len(early) >= 5
    ids = early[:5][::-1]
    rec = _recorder(env, ids=ids, capacity=steps)
    _run(env, pol, rec, [steps], False, u, episodes=E2)
    want = _walk(s, ids, E2, steps)
    got = rec.numpy()
    print("early endings: envs", ids, "cursor", got["cursor"], "flags of the done rows", [list(got["flags"][r, :n][got["done"][r, :n] != 0]) for r, n in enumerate(got["cursor"])])
    _assert_record(got, want)
    for r in range(5):
        first = int(np.flatnonzero(got["done"][r, :got["cursor"][r]])[0])
        assert first < 39 and got["flags"][r, first] & (native.EV_COLLIDING | native.EV_OUT_OF_BOUNDS | native.EV_NO_GOALS_LEFT)
        assert not np.array_equal(got["next_obs"][r, first], got["obs"][r, first + 1])  # the terminal row, not the reset row after it
    env.close()


def test_capacity_ends_mid_episode(torch_cuda, world):
    env, s = world["env"], world["sampled"]
    rec = _recorder(env, capacity=10)
    _run(env, world["pol"], rec, [T], False, world["u"])
    want = _walk(s, IDS, E, 10)
    got = rec.numpy()
    print("capacity 10: overflow", got["overflow"], "done at row 9", got["done"][:, 9])
    assert (want["cursor"] == 10).all() and (want["overflow"] > 0).all()                # the input does overflow every slot
    _assert_record(got, want)                                                            # (nothing past row 9: there is no row 10)
    assert (got["cursor"] == 10).all() and np.array_equal(got["overflow"], want["overflow"])
    full = _walk(s, IDS, E, CAP)
    assert np.array_equal(got["overflow"], full["cursor"] - 10)                          # the counted steps not kept
    assert [eps[-1]["complete"] for eps in rec.episodes()] == [bool(d) for d in got["done"][:, 9]]


def test_two_calls_continue_at_the_cursors(torch_cuda, world):
    env, s = world["env"], world["sampled"]
    rec = _recorder(env, frames=SIZES[0], frame_every=3)
    _run(env, world["pol"], rec, [5, 27], False, world["u"])
    want = _walk(s, IDS, E, CAP)
    two = _walk(s, IDS, E, CAP, slice(5, T), state=_walk(s, IDS, E, CAP, slice(0, 5)))
    assert all(np.array_equal(want[k], two[k]) for k in want)
    got = rec.numpy()
    _assert_record(got, want)
    _assert_frames(got, want, world["screens"][(SIZES[0], True)], 3)


def test_evaluate_with_reset_twice_gives_identical_records(torch_cuda, world):
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    env, s = world["env"], world["greedy"]
    rec = _recorder(env)
    ev = NativeEvaluator(env)
    r1 = ev.evaluate(world["pol"], E, greedy=True, max_steps=T, chunk=8, recorder=rec)
    first = rec.numpy()
    pe1 = r1["per_env"].cpu().numpy().copy()
    r2 = ev.evaluate(world["pol"], E, greedy=True, max_steps=T, chunk=8, recorder=rec)  # reset=True: env, carries and cursors
    second = rec.numpy()
    assert all(np.array_equal(first[k], second[k]) for k in first if k != "frames")
    assert np.array_equal(pe1, r2["per_env"].cpu().numpy()) and r1["steps"] == r2["steps"]
    _assert_record(second, _walk(s, IDS, E, CAP, slice(0, r2["steps"])))                 # (chunks of 8: four calls at most)


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_frames_are_the_screens_of_the_moment(torch_cuda, world, size, S, debug):
    env, s = world["env"], world["sampled"]
    rec = _recorder(env, frames=size, frame_every=S, debug=debug)
    assert tuple(rec.frames.shape) == (len(IDS), (CAP + S - 1) // S, size[0], size[1], 3)
    _run(env, world["pol"], rec, [T], False, world["u"])
    want = _walk(s, IDS, E, CAP)
    got = rec.numpy()
    _assert_record(got, want)                                                            # the trajectory of a run without frames
    _assert_frames(got, want, world["screens"][(size, debug)], S)
    ep = rec.episodes()[0][0]
    assert ep["frames"].shape == ((len(ep["act"]) + S - 1) // S, size[1], size[0], 3)    # [T', H, W, 3]
    assert np.array_equal(ep["frames"][0], world["screens"][(size, debug)][0, 0].transpose(1, 0, 2))


@pytest.mark.parametrize("size", SIZES)
def test_get_screens_is_get_screen_per_env(torch_cuda, world, size):
    torch = torch_cuda
    env = world["env"]
    env.reset_tensor()
    acts = env.random_actions(5, 0, 6)
    for k in range(6):
        env.step_tensor(acts[k])
    one = torch.stack([env.get_screen(e, size[0], size[1]) for e in range(N_ENVS)])
    assert len({one[e].cpu().numpy().tobytes() for e in range(N_ENVS)}) > 1              # (the envs do differ)
    for ids in ([7], IDS, list(range(N_ENVS))):
        got = env.get_screens(ids, size[0], size[1])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (len(ids), size[0], size[1], 3)
        assert torch.equal(got, one[ids]), len(ids)
    plain = torch.stack([env.get_screen(e, size[0], size[1], debug=False) for e in IDS])
    assert torch.equal(env.get_screens(torch.tensor(IDS, dtype=torch.int32, device=DEV), size[0], size[1], debug=False), plain)
    # an id out of range leaves its frame unwritten and the others right (torch.empty gives no sentinel: call the library)
    from ship_sim_gym_amd import _native as N
    ids = torch.tensor([3, N_ENVS, 9, -1, 255], dtype=torch.int32, device=DEV)
    out = torch.full((5, size[0], size[1], 3), SENT_PIX, dtype=torch.uint8, device=DEV)
    N.check(N.lib().ssg_render_envs(env._h, C.c_void_p(ids.data_ptr()), 5, size[0], size[1], C.c_void_p(out.data_ptr()), 1, env._stream()), env._h)
    assert bool((out[1] == SENT_PIX).all()) and bool((out[3] == SENT_PIX).all())
    assert torch.equal(out[[0, 2, 4]], one[[3, 9, 255]])


def test_get_images_is_render_rgb_array_per_env(torch_cuda):
    env = _vec(64)
    env.reset_tensor()
    acts = env.random_actions(6, 0, 4)
    for k in range(4):
        env.step_tensor(acts[k])
    images = env.get_images()
    assert len(images) == 64
    for i, img in enumerate(images):
        want = env.render(mode="rgb_array", env=i)
        assert img.shape == want.shape == (600, 600, 3) and img.dtype == want.dtype and np.array_equal(img, want), i
    env.close()


def test_a_bound_recorder_is_invisible(torch_cuda, world):
    torch = torch_cuda
    pol, u = world["pol"], world["u"]
    a, b = _vec(), _vec()
    ta, tb = a.enable_terminal_obs(True), b.enable_terminal_obs(True)                   # the callers' own bindings
    rec = _recorder(a, frames=SIZES[0])
    eva, evb = _run(a, pol, rec, [T], False, u), _run(b, pol, None, [T], False, u)
    sa, sb = a.snapshot(), b.snapshot()
    assert torch.equal(sa["state"], sb["state"]) and torch.equal(sa["out"], sb["out"]) and torch.equal(a.obs, b.obs)
    assert torch.equal(eva.env_stats, evb.env_stats) and torch.equal(eva.reduce(1), evb.reduce(1))
    assert torch.equal(eva.carry, evb.carry) and torch.equal(eva.carry_return, evb.carry_return)
    for k in ("act", "logp", "value", "reward", "done", "flags"):
        assert torch.equal(getattr(eva, k), getattr(evb, k)), k
    # the caller's binding is back: the step after the evaluation stores its terminal observations in the caller's rows
    # (the clock ends every episode at a multiple of 7 steps: the 35th step is the next one that resets anybody)
    acts = a.random_actions(2, 0, 3)
    for k in range(2):
        a.step_tensor(acts[k]); b.step_tensor(acts[k])
    ta.fill_(SENT); tb.fill_(SENT)
    da = a.step_tensor(acts[2])[2].clone()
    b.step_tensor(acts[2])
    assert int(da.sum()) > 0 and torch.equal(ta, tb)
    assert bool((ta[da != 0] != SENT).all()) and bool((ta[da == 0] == SENT).all())
    a.close(); b.close()


def test_nothing_stays_bound_after_a_recorded_evaluation(torch_cuda, world, native):
    env = world["env"]
    rec = _recorder(env, frames=SIZES[0])
    ev = _run(env, world["pol"], rec, [T], True)
    before = rec.numpy()
    got = native.EvalRecorderRecord()
    native.check(native.lib().ssg_get_eval_recorder(env._h, C.byref(got)), env._h)
    assert got.struct_size == 0
    env.reset_tensor()
    ev.reset_carry()
    ev.run(world["pol"], E, T, greedy=True)                                              # recorder=None: the cursors are still below C
    after = rec.numpy()
    assert all(np.array_equal(before[k], after[k]) for k in before)


def test_population_slots_are_each_members_own_record(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation
    P, n = 2, 128
    env = _vec(P * n)
    pop = NativePopulation([_policy(torch, env.states_history, seed=40 + m) for m in range(P)])
    rec = _recorder(env, frames=SIZES[0], frame_every=3)
    ev = _run(env, pop, rec, [T], True)
    got = rec.numpy()
    assert (got["cursor"] > 0).all()
    for m in range(P):
        slots = [r for r, e in enumerate(IDS) if e // n == m]
        assert slots
        one = _vec(n, env_id_base=m * n)
        rec1 = _recorder(one, ids=[IDS[r] - m * n for r in slots], frames=SIZES[0], frame_every=3)
        ev1 = _run(one, pop.member(m), rec1, [T], True)
        g1 = rec1.numpy()
        for k in g1:
            assert np.array_equal(got[k][slots], g1[k]), (m, k)
        assert torch.equal(ev.env_stats[m * n:(m + 1) * n], ev1.env_stats) and torch.equal(env.obs[m * n:(m + 1) * n], one.obs)
        one.close()
    env.close()


def test_config4_record_equals_the_step_by_step_oracle(torch_cuda):
    torch = torch_cuda
    ids, steps, size = [63, 0], 16, SIZES[0]
    env = _vec(64, n_ships=4, n_maps=16)
    pol = _policy(torch, env.states_history, seed=2)
    s, screens = _oracle(torch, env, pol, steps, ids, True, sizes=(size,), debugs=(True,))
    rec = _recorder(env, ids=ids, capacity=steps, frames=size)
    _run(env, pol, rec, [steps], True)
    want = _walk(s, ids, E, steps)
    got = rec.numpy()
    _assert_record(got, want)
    _assert_frames(got, want, screens[(size, True)], 1)
    assert int(s["done"][:, ids].sum()) > 0                                              # a terminal observation was recorded
    assert (screens[(size, True)] == 0).all(axis=-1).any()                               # black pixels: the traffic hulls are in the frames
    env.close()


def test_refusals_leave_the_binding_and_the_outputs(torch_cuda, world, native):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import EvalRecorder, NativeEvaluator
    L = native.lib()
    env = world["env"]
    env.reset_tensor()
    rec = _recorder(env, frames=SIZES[0])
    rec.bind()
    good = rec.record()

    def bound():
        g = native.EvalRecorderRecord()
        native.check(L.ssg_get_eval_recorder(env._h, C.byref(g)), env._h)
        return (g.struct_size, g.n_tracked, g.capacity, [g.env_ids[i] for i in range(g.n_tracked)], g.dev_obs, g.dev_frames)

    kept = bound()
    assert kept == (C.sizeof(native.EvalRecorderRecord), len(IDS), CAP, IDS, rec.obs.data_ptr(), rec.frames.data_ptr())
    out_before, state_before, rec_before = env._out_blob.clone(), env.state.clone(), rec.numpy()
    cases = [("struct_size", 8), ("n_tracked", 0), ("n_tracked", native.EVAL_REC_MAX_ENVS + 1), ("capacity", 0), ("reserved", 1),
             ("frame_width", 0), ("frame_width", 8193), ("frame_height", 0), ("frame_height", 8193), ("frame_every", 0)]
    cases += [(name, None) for name in ("env_ids", "dev_obs", "dev_next_obs", "dev_act", "dev_logp", "dev_value", "dev_reward", "dev_done",
                                        "dev_flags", "dev_cursor", "dev_overflow", "dev_term_obs")]
    for field, bad in cases:
        r = rec.record()
        setattr(r, field, bad)
        assert L.ssg_set_eval_recorder(env._h, C.byref(r)) == -1, field
        assert bound() == kept, field
    for ids in ([0, 5, 0], [0, N_ENVS], [-1, 3]):                                        # a duplicate, two ids out of range
        r = rec.record()
        arr = (C.c_int32 * len(ids))(*ids)
        r.n_tracked, r.env_ids = len(ids), C.cast(arr, C.POINTER(C.c_int32))
        assert L.ssg_set_eval_recorder(env._h, C.byref(r)) == -1 and bound() == kept, ids
    r = rec.record()
    r.capacity, r.frame_width, r.frame_height = 11, 8192, 8192                           # 33 * 2^26 bytes of frames per slot
    assert L.ssg_set_eval_recorder(env._h, C.byref(r)) == -1 and b"2^31" in L.ssg_last_error(env._h) and bound() == kept
    assert L.ssg_set_eval_recorder(env._h, C.byref(good)) == 0 and bound() == kept      # (the record itself binds)
    torch.cuda.synchronize()
    now = rec.numpy()
    assert torch.equal(env._out_blob, out_before) and torch.equal(env.state, state_before)   # nothing was launched
    assert all(np.array_equal(rec_before[k], now[k]) for k in now)
    rec.unbind()
    assert bound()[0] == 0
    # the two refusals that depend on the handle: no in-kernel reset (BAD_ARG), history > 2 (UNSUPPORTED, ssg_set_timeout_boot's reason)
    for kw, text in ((dict(auto_reset=False), "SSG_FLAG_AUTO_RESET"), (dict(history=3), "history > 2")):
        other = _vec(64, **kw)
        rec2 = EvalRecorder(other, [0, 63], 4)
        with pytest.raises(native.ShipSimError, match=text):
            rec2.bind()
        if "history" in kw:
            assert L.ssg_set_eval_recorder(other._h, C.byref(rec2.record())) == -4
            pol = _policy(torch, other.states_history)
            other.reset_tensor()
            before = other.obs.clone()
            with pytest.raises(native.ShipSimError, match=text):
                NativeEvaluator(other).run(pol, E, 4, greedy=True, recorder=rec2)
            assert torch.equal(other.obs, before)                                        # refused before anything was enqueued
        else:
            assert L.ssg_set_eval_recorder(other._h, C.byref(rec2.record())) == -1
        g = native.EvalRecorderRecord()
        native.check(L.ssg_get_eval_recorder(other._h, C.byref(g)), other._h)
        assert g.struct_size == 0
        other.close()
