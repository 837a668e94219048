"""The evaluation recorder without a GPU: the header, the binding and the ABI version agree on the new record, constants and entry
points; the host-side refusals of ssg_set_eval_recorder / ssg_render_envs; and record_walk, split_episodes and rollouts_of
(ship_sim_gym_amd/evaluate.py) on hand-made arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "shipsim.h")).read()


def _handle(native, n_envs=8, flags=None, history=2):
    c = native.default_config()
    c.n_envs, c.history = n_envs, history
    c.flags = native.FLAG_AUTO_RESET if flags is None else flags
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _record(native, ids, capacity=4, frames=False, keep=[]):
    """A record whose pointers are never dereferenced (no call here gets as far as a launch)."""
    r = native.EvalRecorderRecord()
    r.struct_size, r.n_tracked, r.capacity = C.sizeof(native.EvalRecorderRecord), len(ids), capacity
    arr = (C.c_int32 * max(1, len(ids)))(*ids)
    keep.append(arr)
    r.env_ids = C.cast(arr, C.POINTER(C.c_int32))
    for name in ("dev_obs", "dev_next_obs", "dev_act", "dev_logp", "dev_value", "dev_reward", "dev_done", "dev_flags", "dev_cursor",
                 "dev_overflow", "dev_term_obs"):
        setattr(r, name, 0x1000)
    if frames:
        r.dev_frames, r.frame_width, r.frame_height, r.frame_every, r.frame_flags = 0x1000, 16, 8, 1, 1
    return r


def test_header_binding_and_abi_agree(native):
    assert native.ABI_VERSION == 9 and native.lib().ssg_abi_version() == 9              # additive: the version stays
    consts = dict(re.findall(r"#define\s+(SSG_[A-Z_]+)\s+(\d+)", HEADER))
    assert int(consts["SSG_ABI_VERSION"]) == 9
    assert int(consts["SSG_EVAL_REC_MAX_ENVS"]) == native.EVAL_REC_MAX_ENVS
    assert int(consts["SSG_RENDER_MAX_ENVS"]) == native.RENDER_MAX_ENVS >= 4096
    body = re.search(r"typedef struct ssg_eval_recorder \{(.*?)\} ssg_eval_recorder;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.search(r"(\w+)\s*$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert fields == [f[0] for f in native.EvalRecorderRecord._fields_]
    sizes = {"uint32_t": 4, "int32_t": 4}
    want = 0
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        n = 8 if "*" in decl else sizes[decl.split()[0]]
        want = (want + n - 1) // n * n + n
    assert C.sizeof(native.EvalRecorderRecord) == want == 136
    L = native.lib()
    for name in ("ssg_render_envs", "ssg_set_eval_recorder", "ssg_get_eval_recorder"):
        assert name in native.EXPORTS and hasattr(L, name) and re.search(r"\bint %s\(" % name, HEADER)
    assert C.sizeof(native.Eval) == 4 * 4 + 2 * 8 + 11 * 8                                                # ssg_eval keeps its size


def test_bind_get_unbind_and_every_refusal_keeps_the_previous_binding(native):
    L = native.lib()
    h = _handle(native)
    got = native.EvalRecorderRecord()
    assert L.ssg_get_eval_recorder(h, C.byref(got)) == 0 and got.struct_size == 0       # nothing bound
    assert L.ssg_set_eval_recorder(None, None) == -1 and L.ssg_get_eval_recorder(h, None) == -1
    first = _record(native, [7, 0, 3], capacity=5)
    assert L.ssg_set_eval_recorder(h, C.byref(first)) == 0

    def bound():
        g = native.EvalRecorderRecord()
        assert L.ssg_get_eval_recorder(h, C.byref(g)) == 0
        return (g.struct_size, g.n_tracked, g.capacity, [g.env_ids[i] for i in range(g.n_tracked)], g.dev_frames)

    assert bound() == (136, 3, 5, [7, 0, 3], None)                                      # the library's own copy, in the caller's order
    cases = []
    r = _record(native, [1]); r.struct_size = 135; cases.append((r, b"struct_size"))
    r = _record(native, [1]); r.reserved = 1; cases.append((r, b"reserved"))
    r = _record(native, []); cases.append((r, b"n_tracked"))
    r = _record(native, list(range(8)) * 9); cases.append((r, b"n_tracked"))             # 72 > 64 (and repeats, never reached)
    r = _record(native, [1], capacity=0); cases.append((r, b"capacity"))
    for name in ("env_ids", "dev_obs", "dev_next_obs", "dev_act", "dev_logp", "dev_value", "dev_reward", "dev_done", "dev_flags",
                 "dev_cursor", "dev_overflow", "dev_term_obs"):
        r = _record(native, [1])
        setattr(r, name, None)
        cases.append((r, b"NULL"))
    cases.append((_record(native, [1, 2, 1]), b"repeats"))
    cases.append((_record(native, [1, 8]), b"outside"))
    cases.append((_record(native, [-1]), b"outside"))
    for field, bad in (("frame_width", 0), ("frame_width", 8193), ("frame_height", 0), ("frame_height", 8193), ("frame_every", 0),
                       ("frame_every", -1)):
        r = _record(native, [1], frames=True)
        setattr(r, field, bad)
        cases.append((r, b"frame_"))
    r = _record(native, [1], capacity=11, frames=True)                                   # 11 frames of 8192 x 8192 x 3 = 33 * 2^26 bytes ...
    r.frame_width = r.frame_height = 8192
    cases.append((r, b"2^31"))
    for rec, text in cases:
        assert L.ssg_set_eval_recorder(h, C.byref(rec)) == -1, text
        assert text in L.ssg_last_error(h), (text, L.ssg_last_error(h))
        assert bound() == (136, 3, 5, [7, 0, 3], None)
    r.frame_every = 2                                                                    # ... 6 frames: 18 * 2^26 bytes, in range
    assert L.ssg_set_eval_recorder(h, C.byref(r)) == 0 and bound()[1:4] == (1, 11, [1])
    assert L.ssg_set_eval_recorder(h, None) == 0 and bound()[0] == 0
    L.ssg_destroy(h)
    for flags, history, code, text in ((0, 2, -1, b"SSG_FLAG_AUTO_RESET"), (native.FLAG_AUTO_RESET, 3, -4, b"history > 2")):
        h2 = _handle(native, flags=flags, history=history)
        assert L.ssg_set_eval_recorder(h2, C.byref(_record(native, [1]))) == code and text in L.ssg_last_error(h2)
        assert L.ssg_get_eval_recorder(h2, C.byref(got)) == 0 and got.struct_size == 0
        assert L.ssg_set_eval_recorder(h2, None) == 0                                    # unbinding always passes
        L.ssg_destroy(h2)


def test_render_envs_refuses_bad_arguments_before_any_device_work(native):
    """ssg_render's checks in its order, plus the count and the 2^31-byte bound; arguments in range reach SSG_ERR_NOT_BOUND."""
    L = native.lib()
    h = _handle(native)
    buf = C.c_void_p(0x1000)
    assert L.ssg_render_envs(None, buf, 1, 4, 4, buf, 1, None) == -1
    assert L.ssg_render_envs(h, None, 1, 4, 4, buf, 1, None) == -1 and b"ssg_render_envs" in L.ssg_last_error(h)
    assert L.ssg_render_envs(h, buf, 1, 4, 4, None, 1, None) == -1
    for v in (0, -1, 8193):
        assert L.ssg_render_envs(h, buf, 1, v, 4, buf, 1, None) == -1, v
        assert L.ssg_render_envs(h, buf, 1, 4, v, buf, 0, None) == -1, v
    for count in (0, -1, native.RENDER_MAX_ENVS + 1):
        assert L.ssg_render_envs(h, buf, count, 4, 4, buf, 1, None) == -1 and b"count" in L.ssg_last_error(h), count
    assert L.ssg_render_envs(h, buf, 11, 8192, 8192, buf, 1, None) == -1 and b"2^31" in L.ssg_last_error(h)   # 11 * 3 * 2^26 > 2^31
    for count, w, hh in ((1, 4, 4), (native.RENDER_MAX_ENVS, 4, 4), (10, 8192, 8192), (2048, 1024, 341)):
        assert L.ssg_render_envs(h, buf, count, w, hh, buf, 0, None) == -3, (count, w, hh)
        assert b"ssg_bind_state" in L.ssg_last_error(h)
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# record_walk on hand-made arrays
# ------------------------------------------------------------------------------------------------------------------------------------
T, N_ENVS, D = 12, 4, 3
# env 0: episodes end at steps 2, 5, 8, 11; env 1: at 3 and 10; env 2: never; env 3: at every step
ENDS = {0: (2, 5, 8, 11), 1: (3, 10), 2: (), 3: tuple(range(T))}


def _steps():
    k, e = np.meshgrid(np.arange(T), np.arange(N_ENVS), indexing="ij")
    done = np.zeros((T, N_ENVS), dtype=np.uint8)
    for env, ends in ENDS.items():
        done[list(ends), env] = 1
    tag = 100.0 * k + 10.0 * e                                                           # every (step, env) is its own value
    obs = tag[..., None] + np.arange(D)
    after, term = obs + 0.25, obs + 0.5
    from ship_sim_gym_amd.evaluate import next_observations
    s = {"obs": obs, "act": (k + e) % 3, "logp": -(tag + 1).astype(np.float32), "value": (tag + 2).astype(np.float32), "rew": tag + 3,
         "done": done, "flags": (done * 8 + 2 * ((k + e) % 2)).astype(np.uint8), "next_obs": next_observations(after, term, done)}
    return s, after, term


def _walk(s, ids, E, cap, sl=slice(None), state=None):
    from ship_sim_gym_amd.evaluate import record_walk
    return record_walk(*(s[k][sl] for k in ("obs", "act", "logp", "value", "rew", "done", "flags", "next_obs")), ids, E, cap, state=state)


def test_next_obs_is_the_terminal_row_exactly_on_done_steps():
    s, after, term = _steps()
    d = s["done"] != 0
    assert d.any() and (~d).any()
    assert np.array_equal(s["next_obs"][d], term[d]) and np.array_equal(s["next_obs"][~d], after[~d])
    rec = _walk(s, [1], 2, T)
    assert rec["cursor"][0] == 11 and list(np.flatnonzero(rec["done"][0, :11])) == [3, 10]
    for t in range(11):
        assert np.array_equal(rec["next_obs"][0, t], (term if t in (3, 10) else after)[t, 1])


def test_an_env_that_finishes_its_episodes_mid_run_stops_recording():
    s, _, _ = _steps()
    rec = _walk(s, [0, 2], 2, T)                                                         # env 0 counts its 2nd episode at step 5
    assert list(rec["cursor"]) == [6, 12] and list(rec["overflow"]) == [0, 0]
    assert np.array_equal(rec["obs"][0, :6], s["obs"][:6, 0]) and np.array_equal(rec["reward"][0, :6], s["rew"][:6, 0])
    assert np.array_equal(rec["act"][0, :6], s["act"][:6, 0]) and np.array_equal(rec["flags"][0, :6], s["flags"][:6, 0])
    assert np.array_equal(rec["logp"][0, :6], s["logp"][:6, 0]) and np.array_equal(rec["value"][0, :6], s["value"][:6, 0])
    assert list(rec["iteration"][0]) == [0, 1, 2, 3, 4, 5] + [-1] * 6
    for k in ("obs", "next_obs", "act", "logp", "value", "reward", "done", "flags"):
        assert not rec[k][0, 6:].any(), k                                                # nothing past the cursor
    assert np.array_equal(rec["obs"][1], s["obs"][:, 2]) and not rec["done"][1].any()    # env 2 never ends: all 12 steps
    assert list(rec["counted"]) == [2, 2, 0, 2]


def test_capacity_reached_mid_episode_counts_the_steps_not_kept():
    s, _, _ = _steps()
    rec = _walk(s, [0, 1, 2], 3, 7)                                                      # env 0 counts 9 steps; envs 1 and 2 never reach 3 episodes: all 12
    assert list(rec["cursor"]) == [7, 7, 7] and list(rec["overflow"]) == [2, 5, 5]
    assert np.array_equal(rec["obs"][0], s["obs"][:7, 0]) and rec["done"][0, 6] == 0    # cut inside env 0's third episode
    assert list(rec["counted"][:3]) == [3, 2, 0]                                         # the accounting goes on past the capacity


def test_one_episode_per_env_and_unsorted_ids():
    s, _, _ = _steps()
    rec = _walk(s, [3, 0, 1], 1, T)
    assert list(rec["cursor"]) == [1, 3, 4] and list(rec["overflow"]) == [0, 0, 0]       # each env's first episode, then silence
    assert all(rec["done"][r, n - 1] == 1 and not rec["done"][r, :n - 1].any() for r, n in enumerate(rec["cursor"]))
    a, b = _walk(s, [0, 1, 3], 1, T), rec
    for k in ("obs", "next_obs", "act", "logp", "value", "reward", "done", "flags", "cursor", "overflow", "iteration"):
        assert np.array_equal(a[k][[2, 0, 1]], b[k]), k                                  # a slot depends on its env alone
    with pytest.raises(ValueError):
        _walk(s, [0, 0], 1, T)
    with pytest.raises(ValueError):
        _walk(s, [N_ENVS], 1, T)


@pytest.mark.parametrize("T1", [1, 4, 6, 11])
def test_two_calls_equal_one(T1):
    s, _, _ = _steps()
    one = _walk(s, [1, 0, 3], 3, 8)
    first = _walk(s, [1, 0, 3], 3, 8, slice(0, T1))
    kept = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in first.items()}
    two = _walk(s, [1, 0, 3], 3, 8, slice(T1, T), state=first)
    assert set(one) == set(two)
    for k in one:
        assert np.array_equal(one[k], two[k]), k
        assert np.array_equal(first[k], kept[k]), k                                      # the state was continued, not modified


def test_episodes_and_rollouts_split_where_done_is_set():
    from ship_sim_gym_amd.evaluate import RECORD_ROWS, rollouts_of, split_episodes
    s, _, term = _steps()
    rec = _walk(s, [0, 2, 3], 3, 8)                                                      # env 0: 3 + 3 + 2 of 3 steps (capacity); env 2: no end
    S = 3
    rec["frames"] = np.arange(3 * 3 * 2 * 5 * 3, dtype=np.uint8).reshape(3, 3, 2, 5, 3)  # [R, ceil(8 / 3), W = 2, H = 5, 3]
    eps = split_episodes(rec, frame_every=S)
    assert [len(e) for e in eps] == [3, 1, 3]
    assert [len(ep["act"]) for ep in eps[0]] == [3, 3, 2] and [ep["complete"] for ep in eps[0]] == [True, True, False]
    assert len(eps[1][0]["act"]) == 8 and eps[1][0]["complete"] is False                 # cut by the capacity
    assert [len(ep["act"]) for ep in eps[2]] == [1, 1, 1] and all(ep["complete"] for ep in eps[2])
    for r, slot in enumerate(eps):
        for k in RECORD_ROWS:
            assert np.array_equal(np.concatenate([ep[k] for ep in slot]), rec[k][r, :rec["cursor"][r]]), (r, k)
    # frames: the steps t with t % 3 == 0 belong to the episode that holds step t, as [T', H, W, 3]
    assert [ep["frames"].shape for ep in eps[0]] == [(1, 5, 2, 3), (1, 5, 2, 3), (1, 5, 2, 3)]
    assert np.array_equal(eps[0][1]["frames"][0], rec["frames"][0, 1].transpose(1, 0, 2))   # step 3 opens env 0's second episode
    assert eps[1][0]["frames"].shape == (3, 5, 2, 3) and eps[2][1]["frames"].shape == (0, 5, 2, 3)
    rollouts = rollouts_of(eps)
    assert len(rollouts) == 7 and [len(ep) for ep in rollouts] == [3, 3, 2, 8, 1, 1, 1]
    state, action, next_state, reward, done = rollouts[0][2]
    assert np.array_equal(state, s["obs"][2, 0]) and action == int(s["act"][2, 0]) and isinstance(action, int)
    assert np.array_equal(next_state, term[2, 0]) and reward == float(s["rew"][2, 0]) and done is True
    assert rollouts[0][0][4] is False and rollouts[3][-1][4] is False
    rec["frames"] = None
    assert "frames" not in split_episodes(rec)[0][0]
