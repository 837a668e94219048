"""ShipVecEnv's host side (ship_sim_gym_amd/vec_env.py) over the three map modes: the two vector-env protocols against each other,
reset_at outside a done, step_wait's host auto-reset, and what the tensor API refuses.  Small envs (64 at the most), short episodes
(MAX_STEPS = 25), seeded numpy actions; "bit for bit" compares bytes."""
import random

import numpy as np
import pytest

from gpu_support import DEV, env_config, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

MODES = {"bank": (64, dict(map_mode="bank", n_maps=4)), "fresh_device": (64, dict(map_mode="fresh_device", ring=4)),
         "fresh": (8, dict(map_mode="fresh"))}
STEPS = 200


def _env(mode, hist=2, **kw):
    """A handle of MODES[mode].  "fresh" draws its worlds from the global random streams, from the constructor on: both are seeded
    here, so two handles made one after the other see the same worlds as long as they draw in the same order."""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    random.seed(11)
    np.random.seed(11)
    n, mode_kw = MODES[mode]
    return ShipVecEnv(n, env_config=env_config(hist, 25), **mode_kw, **kw)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _end(env, native):
    return env.field(native.F_MAP_ID).cpu().numpy(), env.stats()


@pytest.mark.parametrize("hist", [2, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_protocols_agree(torch_cuda, native, mode, hist):
    """The stable-baselines protocol (`step`: a done env is reset inside the step) and the RLlib protocol (rllib=True: `vector_step`,
    then `reset_at` of every done env) on the same seeded actions: rewards and dones bit for bit, observations bit for bit off the
    done rows, reset_at's row = SB's row, and the same map ids and episode counters at the end.  Every env finishes at least seven
    episodes (an episode lasts 25 steps at the most), so a ring of 4 wraps.  The two handles run one after the other: "fresh" draws
    its worlds from the global streams."""
    if (mode, hist) == ("fresh_device", 3):  # the library refuses the handle: the ring's kernels serve history <= 2
        for kw in ({}, {"rllib": True}):
            with pytest.raises(native.ShipSimError, match="map_ring needs history <= 2"):
                _env(mode, hist, **kw)
        return
    n = MODES[mode][0]
    acts = np.random.RandomState(5).randint(0, 3, size=(STEPS, n))
    sb = _env(mode, hist)
    first, steps = sb.reset(), []
    for a in acts:
        o, r, d, _ = sb.step(a)
        steps.append((o.copy(), r, d))
    ids_sb, stats_sb = _end(sb, native)
    sb.close()
    episodes = np.sum([d for _, _, d in steps], axis=0)
    assert episodes.min() >= 7, episodes

    rl = _env(mode, hist, rllib=True)
    assert rl.rllib and rl._rllib_fused == (hist <= 2 and mode != "fresh") and rl.auto_reset == rl._rllib_fused
    assert _same(np.stack(rl.vector_reset()), first)
    for k, a in enumerate(acts):
        o_sb, r_sb, d_sb = steps[k]
        o, r, d, _ = rl.vector_step(list(a))
        assert _same(r, r_sb) and _same(d, d_sb), k
        assert _same(np.asarray(o)[~d_sb], o_sb[~d_sb]), k
        for i in np.nonzero(d_sb)[0]:
            assert _same(rl.reset_at(int(i)), o_sb[i]), (k, i)
    ids_rl, stats_rl = _end(rl, native)
    rl.close()
    assert _same(ids_rl, ids_sb)
    assert stats_rl == stats_sb and stats_sb["episodes"] == int(episodes.sum())


@pytest.mark.parametrize("mode", list(MODES))
def test_reset_at_with_nothing_pending_is_a_one_hot_reset(torch_cuda, native, mode):
    """reset_at(i) on an env that was not reported done: the whole observation block and the map ids equal those of a twin that
    gets reset_tensor with a one-hot mask — with the next map's id in "bank", no ids in "fresh_device" (the env moves on in its
    ring), and a newly drawn world in env i's own record in "fresh"."""
    torch = torch_cuda
    n = MODES[mode][0]
    i = n - 3
    acts = torch.from_numpy(np.random.RandomState(3).randint(0, 3, size=(5, n)).astype(np.int32)).to(DEV)

    def started():
        env = _env(mode)
        env.reset()
        for a in acts:
            env.step_tensor(a)
        return env

    env = started()
    before = env.obs.cpu().numpy()
    row = env.reset_at(i)
    got = env.obs.cpu().numpy()
    ids, _ = _end(env, native)
    env.close()
    assert _same(row, got[i]) and not _same(row, before[i])
    assert np.all(row[:env.n_states] == -1) and row[env.n_states] == env.bounds[0] / 2

    twin = started()
    mask = torch.zeros(n, dtype=torch.uint8, device=DEV)
    mask[i] = 1
    if mode == "bank":
        next_ids = twin.field(native.F_MAP_ID).clone()
        next_ids[i] = (next_ids[i] + 1) % twin.n_maps
        twin.reset_tensor(mask=mask, map_ids=next_ids.to(torch.int32).contiguous())
    elif mode == "fresh_device":
        twin.reset_tensor(mask=mask)
    else:
        twin._fresh_world(i)
        twin.bank.copy_(torch.from_numpy(twin.bank_host))
        twin.reset_tensor(mask=mask)
    torch.cuda.synchronize()
    want = twin.obs.cpu().numpy()
    want_ids, _ = _end(twin, native)
    twin.close()
    assert _same(got, want) and _same(ids, want_ids)


def test_step_wait_resets_done_envs_from_the_host_in_fresh_mode(torch_cuda, native):
    """map_mode="fresh": step_wait itself resets the done envs (a new world each, drawn on the host).  Their rows of the returned array
    are reset observations — every frame but the last is -1, the last starts at the spawn, bounds[0] / 2 — and the device's `obs`
    is the returned array."""
    env = _env("fresh")
    env.reset()
    F = env.n_states
    rs = np.random.RandomState(9)
    finished = np.zeros(env.num_envs, dtype=np.int64)
    for _ in range(STEPS):
        o, _, d, _ = env.step(rs.randint(0, 3, size=env.num_envs))
        assert _same(env.obs.cpu().numpy(), o)
        assert np.all(o[d][:, :F] == -1) and np.all(o[d][:, F] == env.bounds[0] / 2)
        assert not np.any(np.all(o[~d][:, :F] == -1, axis=1))  # (an env that went on shows its previous frame)
        finished += d
        if finished.min() >= 2:
            break
    assert finished.min() >= 2, finished
    env.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
K = 3
# argument -> (dtype, shape as a function of (n, D), rows the call needs at least — None: shape[0])
ARGS = {
    "step_tensor.actions": ("int32", lambda n, D: (n,), None),
    "rollout_tensor.actions": ("int32", lambda n, D: (K, n), None),
    "rollout_tensor.out[0]": ("float64", lambda n, D: (K, n, D), None),
    "rollout_tensor.out[1]": ("float64", lambda n, D: (K, n), None),
    "rollout_tensor.out[2]": ("uint8", lambda n, D: (K, n), None),
    "rollout_tensor.out[3]": ("uint8", lambda n, D: (K, n), None),
    "reset_tensor.mask": ("uint8", lambda n, D: (n,), None),
    "reset_tensor.map_ids": ("int32", lambda n, D: (n,), None),
    "wake_dynamics.mask": ("uint8", lambda n, D: (n,), None),
    "policy_act.uniforms": ("float32", lambda n, D: (n,), None),
    "policy_act.x_out": ("float32", lambda n, D: (n, D), None),
    "rollout_policy.uniforms": ("float32", lambda n, D: (K, n), None),
    "rollout_policy.out[obs]": ("float32", lambda n, D: (K, n, D), None),
    "rollout_policy.out[act]": ("int32", lambda n, D: (K, n), None),
    "rollout_policy.out[logp]": ("float32", lambda n, D: (K, n), None),
    "rollout_policy.out[val]": ("float32", lambda n, D: (K, n), None),
    "rollout_policy.out[rew]": ("float64", lambda n, D: (K, n), None),
    "rollout_policy.out[done]": ("uint8", lambda n, D: (K, n), None),
    "rollout_policy.out[flags]": ("uint8", lambda n, D: (K, n), None),
    "rollout_policy.out[last_val]": ("float32", lambda n, D: (n,), None),
    "timeout_values.flags": ("uint8", lambda n, D: (K, n), 1),  # (K is read off the flags: any K >= 1 is a valid call)
    "timeout_values.term_obs": ("float64", lambda n, D: (K, n, D), None),
    "timeout_values.out": ("float32", lambda n, D: (K, n), None),
    "set_bank.bank": ("float64", lambda n, D: (4, 145), None),
}
WRONG_DTYPE = {"int32": "int64", "float32": "float64", "float64": "float32", "uint8": "int32"}
# The defects: "dtype" another dtype; "count" a 1-D tensor of one element more; "trailing" the last dimension one longer (2-D and
# 3-D arguments); "strided" the right shape, every other element of a tensor twice as wide; "cpu" the right tensor in host memory;
# "rows" one row fewer than the call needs.  Not applicable and left out: "count" where a longer first dimension is allowed and the
# argument is 1-D (more uniforms than envs are accepted); "rows" where it is "count" (1-D arguments of exactly n elements) or where
# the first dimension is free (rollout_tensor's actions, the bank); "cpu" for set_bank, which uploads a host bank.
FLAT, ROWS1, MATRIX, MATRIX_ANY_K = (("dtype", "count", "strided", "cpu"), ("dtype", "strided", "cpu", "rows"),
                                     ("dtype", "count", "trailing", "strided", "cpu", "rows"), ("dtype", "count", "trailing", "strided", "cpu"))
# argument, the exception the call raises for each defect, the defects
REFUSALS = [
    ("step_tensor.actions", "ValueError", FLAT),
    ("rollout_tensor.actions", "ValueError", MATRIX_ANY_K),
    ("rollout_tensor.out[0]", "AssertionError", MATRIX),
    ("rollout_tensor.out[1]", "AssertionError", MATRIX),
    ("rollout_tensor.out[2]", "AssertionError", MATRIX),
    ("rollout_tensor.out[3]", "AssertionError", MATRIX),
    ("reset_tensor.mask", "ValueError", FLAT),
    ("reset_tensor.map_ids", "ValueError", FLAT),
    ("wake_dynamics.mask", "ValueError", FLAT),
    ("policy_act.uniforms", "ValueError", ROWS1),
    ("policy_act.x_out", "ValueError", MATRIX),
    ("rollout_policy.uniforms", "ValueError", MATRIX),
    ("rollout_policy.out[obs]", "ValueError", MATRIX),
    ("rollout_policy.out[act]", "ValueError", MATRIX),
    ("rollout_policy.out[logp]", "ValueError", MATRIX),
    ("rollout_policy.out[val]", "ValueError", MATRIX),
    ("rollout_policy.out[rew]", "ValueError", MATRIX),
    ("rollout_policy.out[done]", "ValueError", MATRIX),
    ("rollout_policy.out[flags]", "ValueError", MATRIX),
    ("rollout_policy.out[last_val]", "ValueError", ROWS1),
    ("timeout_values.flags", "ValueError", MATRIX),
    ("timeout_values.term_obs", "ValueError", MATRIX),
    ("timeout_values.out", "ValueError", MATRIX),
    ("set_bank.bank", "AssertionError", ("dtype", "count", "trailing", "strided")),
]


def _argument(torch, env, name, defect=None):
    """The argument `name` of a valid call, or that argument with one defect."""
    dtype, shape, need_rows = ARGS[name]
    shape = tuple(shape(env.num_envs, env.states_history))
    device = "cpu" if defect == "cpu" else env.device
    if defect == "dtype":
        dtype = WRONG_DTYPE[dtype]
    elif defect == "count":
        shape = (int(np.prod(shape)) + 1,)
    elif defect == "trailing":
        shape = shape[:-1] + (shape[-1] + 1,)
    elif defect == "rows":
        shape = ((need_rows or shape[0]) - 1,) + shape[1:]
    elif defect == "strided":
        t = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=getattr(torch, dtype), device=device)[..., ::2]
        assert tuple(t.shape) == shape and not t.is_contiguous()
        return t
    return torch.zeros(shape, dtype=getattr(torch, dtype), device=device)


def _call(torch, env, pol, name, t):
    """The call that takes `t` as its argument `name`; every other argument is valid."""
    ok = lambda other: _argument(torch, env, other)  # noqa: E731
    method, arg = name.split(".")
    key = arg[arg.index("[") + 1: -1] if "[" in arg else None
    if name == "step_tensor.actions":
        return env.step_tensor(t)
    if name == "rollout_tensor.actions":
        return env.rollout_tensor(t)
    if method == "rollout_tensor":
        out = [ok("rollout_tensor.out[%d]" % j) for j in range(4)]
        out[int(key)] = t
        return env.rollout_tensor(ok("rollout_tensor.actions"), trajectory=True, out=tuple(out))
    if name == "reset_tensor.mask":
        return env.reset_tensor(mask=t)
    if name == "reset_tensor.map_ids":
        return env.reset_tensor(mask=ok("reset_tensor.mask"), map_ids=t)
    if name == "wake_dynamics.mask":
        return env.wake_dynamics(t)
    if method == "policy_act":
        return env.policy_act(pol, **{arg: t})
    if name == "rollout_policy.uniforms":
        return env.rollout_policy(pol, K, uniforms=t)
    if method == "rollout_policy":
        out = {k[k.index("[") + 1: -1]: ok(k) for k in ARGS if k.startswith("rollout_policy.out[")}
        out[key] = t
        return env.rollout_policy(pol, K, out=out)
    if method == "timeout_values":
        a = {k: (t if k == arg else ok("timeout_values." + k)) for k in ("flags", "term_obs", "out")}
        return env.timeout_values(pol, a["flags"], a["term_obs"], out=a["out"])
    assert name == "set_bank.bank"
    return env.set_bank(t)


def test_refusals_leave_the_env_as_it_was(torch_cuda, native):
    """Every tensor argument of the tensor API with every defect that applies to it: the call raises the exception of REFUSALS and
    launches nothing — after the whole table the env steps bit for bit like a twin that was never misused.  (A tensor on a second
    GPU is not tried: the test machine has one.)"""
    torch = torch_cuda
    from ship_sim_gym_amd.policy import NativePolicy
    env, twin = _env("bank"), _env("bank")
    env.reset_tensor()
    twin.reset_tensor()
    D, H = env.states_history, 16
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    pol = NativePolicy([(z(H, D), z(H))], (z(3, H), z(3)), (z(1, H), z(1)), 600.0)
    assert sorted(ARGS) == sorted(name for name, _, _ in REFUSALS)
    wrong = []
    for name, exc, defects in REFUSALS:
        for defect in defects:
            try:
                _call(torch, env, pol, name, _argument(torch, env, name, defect))
                wrong.append("%s, %s: accepted" % (name, defect))
            except Exception as ex:
                if type(ex).__name__ != exc:
                    wrong.append("%s, %s: %s instead of %s (%s)" % (name, defect, type(ex).__name__, exc, ex))
    assert not wrong, "\n".join(wrong)
    acts = torch.from_numpy(np.random.RandomState(4).randint(0, 3, size=(40, env.num_envs)).astype(np.int32)).to(DEV)
    for a in acts:
        got, want = env.step_tensor(a), twin.step_tensor(a)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    torch.cuda.synchronize()
    assert torch.equal(env.state, twin.state) and torch.equal(env.bank, twin.bank) and env.stats() == twin.stats()
    env.close()
    twin.close()
