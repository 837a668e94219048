"""CPU-side checks of evaluation (ssg_policy_act_greedy, ssg_pop_act_greedy, ssg_evaluate, ssg_pop_evaluate, ssg_eval_reduce;
ship_sim_gym_amd/evaluate.py; train/evaluate_native.py): the symbols in the header and the binding, the ssg_eval record against ctypes,
every refusal before any device work, eval_walk on an oracle trajectory, and the script's and evaluate()'s argument handling.  No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_SYMBOLS = ("ssg_policy_act_greedy", "ssg_pop_act_greedy", "ssg_evaluate", "ssg_pop_evaluate", "ssg_eval_reduce", "ssg_eval_account")
PTR = C.sizeof(C.c_void_p)
Q = 0x30000  # a plausible device address (256-byte aligned; never dereferenced on the host)


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_eval_symbols_are_declared_exported_bound_and_abi_stays_9(native):
    text = _header()
    L = native.lib()
    for name in EVAL_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in native.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes, name                     # bound with its argument types
    assert native.ABI_VERSION == 9 and L.ssg_abi_version() == 9
    assert re.search(r"#define\s+SSG_ABI_VERSION\s+9\b", text)
    assert int(re.search(r"#define\s+SSG_EVAL_GREEDY\s+(0x[0-9a-fA-F]+)u", text).group(1), 0) == native.EVAL_GREEDY == 1
    assert int(re.search(r"#define\s+SSG_EVAL_STATS\s+(\d+)", text).group(1)) == native.EVAL_STATS == 8


def test_eval_record_matches_the_header(native):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct ssg_eval \{(.*?)\} ssg_eval;", text, flags=re.S).group(1)
    size_of = {"uint32_t": 4, "int32_t": 4, "uint64_t": 8, "int64_t": 8}
    names = []
    for line in body.split(";"):
        line = line.strip()
        if not line:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)$", line)
        assert m, line
        names.append((PTR if m.group(2) else size_of[m.group(1)], m.group(3)))
    assert [n for _, n in names] == [f for f, _ in native.Eval._fields_]
    assert [n for _, n in names][:6] == ["struct_size", "flags", "episodes_per_env", "n_steps", "seed", "step0"]
    off = 0
    for sz, name in names:
        off = (off + sz - 1) // sz * sz
        assert getattr(native.Eval, name).offset == off, name
        off += sz
    assert C.sizeof(native.Eval) == (off + 7) // 8 * 8 == 32 + 11 * PTR


def _handle(native, n_envs, bound, flags=None):
    L = native.lib()
    c = native.default_config()
    c.n_envs = n_envs
    if flags is not None:
        c.flags = flags
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if bound:  # (host only: the address is recorded, never touched before a launch — and every call below is refused before one)
        native.check(L.ssg_bind_state(h, C.c_void_p(0x100000)), h)
    return h


def _policy(native, D=32, H=64, L=2, A=3, params=0x10000, scale=0x20000):
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = D, H, L, A, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = params, scale
    return p


def _population(native, P=4, **kw):
    pol = _policy(native, **kw)
    p = native.Population()
    p.struct_size = C.sizeof(native.Population)
    p.n_members = P
    for k in ("obs_dim", "hidden", "n_hidden_layers", "n_actions", "activation", "dev_params", "dev_obs_scale"):
        setattr(p, k, getattr(pol, k))
    return p


POINTERS = ("dev_obs", "dev_act", "dev_logp", "dev_value", "dev_reward", "dev_done", "dev_flags", "dev_carry_return", "dev_carry",
            "dev_env_stats")


def _eval(native, **kw):
    e = native.Eval()
    e.struct_size = C.sizeof(native.Eval)
    e.flags, e.episodes_per_env, e.n_steps = native.EVAL_GREEDY, 2, 100
    for k in POINTERS:
        setattr(e, k, Q)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _all_calls(native, h):
    L = native.lib()
    q = C.c_void_p(Q)
    pol, pop, ev = C.byref(_policy(native)), C.byref(_population(native)), C.byref(_eval(native))
    return {"act_greedy": L.ssg_policy_act_greedy(h, pol, q, q, q, q, None, None),
            "pop_act_greedy": L.ssg_pop_act_greedy(h, pop, q, q, q, q, None, None),
            "evaluate": L.ssg_evaluate(h, pol, ev, None), "pop_evaluate": L.ssg_pop_evaluate(h, pop, ev, None),
            "reduce": L.ssg_eval_reduce(h, 4, q, q, None), "account": L.ssg_eval_account(h, 2, q, q, q, q, q, q, None)}


def test_eval_entry_points_refuse_without_a_handle_or_a_blob(native):
    L = native.lib()
    assert set(_all_calls(native, None).values()) == {-1}              # SSG_ERR_BAD_ARG without a handle
    h = _handle(native, 1000, bound=False)
    try:
        got = _all_calls(native, h)
        assert set(got.values()) == {-3}, got                          # SSG_ERR_NOT_BOUND without a bound blob ...
        q = C.c_void_p(Q)                                              # ... which is what the rollout counterparts return
        pol, pop = C.byref(_policy(native)), C.byref(_population(native))
        assert L.ssg_policy_act(h, pol, q, None, 0, 0, q, q, q, None, None) == got["act_greedy"]
        assert L.ssg_pop_act(h, pop, q, None, 0, 0, q, q, q, None, None) == got["pop_act_greedy"]
        assert L.ssg_rollout_policy(h, pol, 4, None, 0, 0, q, q, q, q, None, q, q, None, None, 1000, None) == got["evaluate"]
        assert L.ssg_pop_rollout(h, pop, 4, None, 0, 0, q, q, q, q, None, q, q, None, None, 1000, None) == got["pop_evaluate"]
    finally:
        L.ssg_destroy(h)


def test_eval_refusals_before_any_device_work(native):
    """With a (host-recorded) blob every bad record, missing pointer or unfit handle is SSG_ERR_BAD_ARG, judged on the host before the
    bank or the device is asked for anything — so this runs without one."""
    L = native.lib()
    h = _handle(native, 1000, bound=True)
    try:
        pol, pop = C.byref(_policy(native)), C.byref(_population(native))

        def both(ev):
            er = C.byref(ev) if ev is not None else None
            return L.ssg_evaluate(h, pol, er, None), L.ssg_pop_evaluate(h, pop, er, None)

        short = _eval(native)
        short.struct_size -= 8
        bad = {"NULL record": None, "struct_size": short, "E = 0": _eval(native, episodes_per_env=0), "E < 0": _eval(native, episodes_per_env=-3),
               "T = 0": _eval(native, n_steps=0), "T < 0": _eval(native, n_steps=-1),
               "uniforms with greedy": _eval(native, dev_uniform_TN=Q), "unknown flag": _eval(native, flags=2),
               "misaligned carry": _eval(native, dev_carry=Q + 8)}
        for k in POINTERS:
            bad["NULL " + k] = _eval(native, **{k: None})
        for what, ev in bad.items():
            assert both(ev) == (-1, -1), what
        assert b"dev_carry" in L.ssg_last_error(h) or b"dev_env_stats" in L.ssg_last_error(h)
        assert both(_eval(native, dev_uniform_TN=Q))[0] == -1 and b"SSG_EVAL_GREEDY" in L.ssg_last_error(h)
        # bad policy / population records
        good = C.byref(_eval(native))
        for rec in (_policy(native, H=40), _policy(native, D=31), _policy(native, params=0), _policy(native, A=5)):
            assert L.ssg_evaluate(h, C.byref(rec), good, None) == -1
            # (ssg_policy_act asks for the device before it reads the record, and so does its greedy form: both refuse alike)
            qq = C.c_void_p(Q)
            rc = L.ssg_policy_act_greedy(h, C.byref(rec), qq, qq, qq, qq, None, None)
            assert rc < 0 and rc == L.ssg_policy_act(h, C.byref(rec), qq, None, 0, 0, qq, qq, qq, None, None)
        assert L.ssg_evaluate(h, None, good, None) == -1 and L.ssg_pop_evaluate(h, None, good, None) == -1
        q = C.c_void_p(Q)
        for rec in (_population(native, P=0), _population(native, P=257), _population(native, P=3), _population(native, H=40)):
            assert L.ssg_pop_evaluate(h, C.byref(rec), good, None) == -1
            assert L.ssg_pop_act_greedy(h, C.byref(rec), q, q, q, q, None, None) == -1
        # the greedy population launch: NULL required pointers (dev_x alone is nullable)
        for i in range(4):
            args = [q, q, q, q]
            args[i] = None
            assert L.ssg_pop_act_greedy(h, pop, *args, None, None) == -1, i
        # the reduction: member counts and NULL buffers
        for P in (0, 257, 3):
            assert L.ssg_eval_reduce(h, P, q, q, None) == -1, P
        assert L.ssg_eval_reduce(h, 4, None, q, None) == -1 and L.ssg_eval_reduce(h, 4, q, None, None) == -1
        # the accounting launch alone: E < 1, NULL buffers, a misaligned carry
        assert L.ssg_eval_account(h, 0, q, q, q, q, q, q, None) == -1
        for i in range(6):
            args = [q] * 6
            args[i] = None
            assert L.ssg_eval_account(h, 2, *args, None) == -1, i
        assert L.ssg_eval_account(h, 2, q, q, q, q, C.c_void_p(Q + 4), q, None) == -1 and b"16-byte" in L.ssg_last_error(h)
        # (no VALID call is made here: with a device present it would be launched on these made-up addresses)
    finally:
        L.ssg_destroy(h)
    # a handle without SSG_FLAG_AUTO_RESET: a done env would never start its next episode
    h = _handle(native, 1000, bound=True, flags=0)
    try:
        pol, pop, ev = C.byref(_policy(native)), C.byref(_population(native)), C.byref(_eval(native))
        assert L.ssg_evaluate(h, pol, ev, None) == -1 and b"SSG_FLAG_AUTO_RESET" in L.ssg_last_error(h)
        assert L.ssg_pop_evaluate(h, pop, ev, None) == -1 and b"SSG_FLAG_AUTO_RESET" in L.ssg_last_error(h)
    finally:
        L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# eval_walk on an oracle trajectory
# ------------------------------------------------------------------------------------------------------------------------------------
N_ENVS, MAX_STEPS, T = 256, 40, 100


@pytest.fixture(scope="module")
def trajectory(oracle, native):
    """100 steps of 256 oracle envs over a 64-map bank with max_steps 40.  The oracle reports reward and done; the event bits are
    derived from them as the step kernel sets them: the reward is +1 exactly on a goal, -1 exactly out of bounds (no collision-reward
    fix), an episode that is done at its 40th step has timed out, and a done step that is neither is a collision."""
    from ship_sim_gym_amd import worldgen
    _, polys, goals = worldgen.build_bank(64, (600, 600))
    ob = oracle.Batch(N_ENVS, oracle.default_config(max_steps=MAX_STEPS), polys, goals)
    ob.reset()
    acts = oracle.fill_actions(5, 0, T, 0, N_ENVS)
    rew, done, flags = np.zeros((T, N_ENVS)), np.zeros((T, N_ENVS), np.uint8), np.zeros((T, N_ENVS), np.uint8)
    length = np.zeros(N_ENVS, dtype=np.int64)
    for t in range(T):
        _, rew[t], done[t] = ob.step(acts[t], auto_reset=True)
        length += 1
        d = done[t] != 0
        oob, tmo = d & (rew[t] == -1.0), d & (length == MAX_STEPS)
        f = np.where(rew[t] == 1.0, native.EV_GOAL_REACHED, 0) | np.where(oob, native.EV_OUT_OF_BOUNDS, 0)
        f |= np.where(tmo, native.EV_MAX_STEPS, 0) | np.where(d & ~oob & ~tmo, native.EV_COLLIDING, 0)
        flags[t] = f
        length[d] = 0
    return rew, done, flags


def test_eval_walk_counts_exactly_the_first_two_episodes_of_every_env(trajectory, native):
    from ship_sim_gym_amd.evaluate import eval_walk
    rew, done, flags = trajectory
    per_env_total = done.astype(np.int64).sum(0)
    assert per_env_total.min() >= 2                                   # the input's own condition: every env finishes at least 2 ...
    assert per_env_total.max() > 2                                    # ... and some more, so the quota is what stops the count
    rows, (ret, ci) = eval_walk(rew, done, flags, 2)
    assert rows.dtype == np.int64 and rows.shape == (N_ENVS, 8)
    assert (rows[:, 0] == 2).all() and int(rows[:, 0].sum()) == 512
    assert (ci[:, 2] == 2).all() and not ret.any() and not ci[:, :2].any()
    # each ending kind is among the counted episodes (keeps the GPU tests over this regime from passing vacuously)
    assert rows[:, native.EVAL_OUT_OF_BOUNDS].sum() > 0 and rows[:, native.EVAL_MAX_STEPS].sum() > 0
    assert rows[:, native.EVAL_COLLIDED].sum() > 0 and rows[:, native.EVAL_GOALS].sum() > 0
    assert (rows[:, 3:7].sum(1) >= 2).all()                           # every counted episode ended in some way
    # against a direct count per env: the first two done steps, the rewards and goal events up to the second
    for e in range(0, N_ENVS, 17):
        ends = np.flatnonzero(done[:, e])[:2]
        stop = ends[1] + 1
        assert rows[e, 2] == stop
        want = int(np.rint(100 * rew[:ends[0] + 1, e].sum())) + int(np.rint(100 * rew[ends[0] + 1:stop, e].sum()))
        assert rows[e, 1] == want
        assert rows[e, 7] == int((flags[:stop, e] & native.EV_GOAL_REACHED != 0).sum())
    # with no quota in reach every episode of the 100 steps is counted
    all_rows, _ = eval_walk(rew, done, flags, 1000)
    assert (all_rows[:, 0] == per_env_total).all()
    assert all_rows[:, 4].sum() == int(((rew == -1.0) & (done != 0)).sum())
    assert all_rows[:, 7].sum() + 0 <= int((rew == 1.0).sum())


def test_eval_walk_split_with_the_carry_gives_the_same_rows(trajectory):
    from ship_sim_gym_amd.evaluate import eval_walk
    rew, done, flags = trajectory
    for E in (2, 3):
        whole, (ret, ci) = eval_walk(rew, done, flags, E)
        a, carry = eval_walk(rew[:37], done[:37], flags[:37], E)
        kept = (carry[0].copy(), carry[1].copy())
        b, (ret2, ci2) = eval_walk(rew[37:], done[37:], flags[37:], E, carry=carry)
        assert np.array_equal(carry[0], kept[0]) and np.array_equal(carry[1], kept[1])   # the carry passed in is not modified
        assert np.array_equal(a + b, whole) and np.array_equal(ret, ret2) and np.array_equal(ci, ci2)
    with pytest.raises(ValueError):
        eval_walk(rew, done, flags, 0)
    with pytest.raises(ValueError):
        eval_walk(rew, done[:50], flags, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# the script and evaluate()'s arguments
# ------------------------------------------------------------------------------------------------------------------------------------
def test_evaluate_script_parses_its_arguments():
    mod = load_script("train/evaluate_native.py")
    with pytest.raises(SystemExit) as ex:
        mod.parse_args(["--help"])
    assert ex.value.code == 0
    a = mod.parse_args([])
    assert (a.checkpoint, a.sampled, a.separate_value, a.seed) == (None, False, False, 0) and a.envs >= 1 and a.episodes >= 1
    a = mod.parse_args(["--envs", "256", "--episodes", "1", "--sampled", "--separate-value", "--seed", "3", "--device", "cuda:0",
                        "--checkpoint", "w.pt"])
    assert (a.envs, a.episodes, a.sampled, a.separate_value, a.seed, a.device, a.checkpoint) == (256, 1, True, True, 3, "cuda:0", "w.pt")
    for bad in (["--envs", "0"], ["--episodes", "0"]):
        with pytest.raises(SystemExit):
            mod.parse_args(bad)
    assert "rollout.py" in mod.__doc__
    for script in ("ppo_torch.py", "pbt_native.py"):                   # the trainers' periodic evaluation is off by default
        src = open(os.path.join(ROOT, "train", script)).read()
        assert "--eval-every" in src and "--eval-episodes" in src


def test_evaluate_argument_errors_raise_value_error():
    """evaluate() judges its arguments before it touches the env: checked on an evaluator over a stand-in env, no device."""
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    ev = NativeEvaluator.__new__(NativeEvaluator)
    ev.env = types.SimpleNamespace(cfg=types.SimpleNamespace(max_steps=40), num_envs=8)
    pol = object()
    for kw in (dict(episodes=0), dict(episodes=-1), dict(episodes=2, chunk=0), dict(episodes=2, max_steps=0),
               dict(episodes=2, greedy=True, uniforms=np.zeros((80, 8), dtype=np.float32))):
        with pytest.raises(ValueError):
            ev.evaluate(pol, **kw)
    with pytest.raises(ValueError):
        ev.run(pol, 2, 10, greedy=True, uniforms=np.zeros((10, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        ev.run(pol, 0, 10)
    with pytest.raises(ValueError):
        ev.run(pol, 2, 0)
