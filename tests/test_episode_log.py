"""The episode log on the host: episode_log_reference against hand-written cases, EpisodeLog's reading side and state on a CPU stand-in
for the env (the ring filled by the reference), MonitorWriter's file, and the ctypes signatures of the new header functions."""
import ctypes as C
import copy
import os
import re
import warnings

import numpy as np
import pytest
import torch

from ship_sim_gym_amd import _native as N
from ship_sim_gym_amd import episode_log as EL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOAL, COLL, OOB, TIME, NOGOAL = N.EV_GOAL_REACHED, N.EV_COLLIDING, N.EV_OUT_OF_BOUNDS, N.EV_MAX_STEPS, N.EV_NO_GOALS_LEFT


def _empty(n, cap):
    return np.zeros(n), np.zeros((n, 2), dtype=np.int32), np.zeros(2, dtype=np.int64), np.zeros(cap, dtype=EL.RECORD_DTYPE)


def _rec(ret, step, env, length, goals, end):
    return np.array([(ret, step, env, length, goals, end)], dtype=EL.RECORD_DTYPE)[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# episode_log_reference, case by case
# ------------------------------------------------------------------------------------------------------------------------------------
def test_an_episode_spanning_three_calls_is_recorded_once_at_its_end():
    cret, c, head, ring = _empty(1, 4)
    step0 = 0
    blocks = [(np.array([[1.0], [-0.01]]), np.array([[0], [0]]), np.array([[GOAL], [0]])),
              (np.array([[-0.01], [1.0], [-0.01]]), np.array([[0], [0], [0]]), np.array([[0], [GOAL], [0]])),
              (np.array([[-0.01], [-1.0], [-0.01]]), np.array([[0], [1], [0]]), np.array([[0], [COLL], [0]]))]
    for rew, done, fl in blocks:
        ring, head, cret, c = EL.episode_log_reference(rew, done, fl, cret, c, head, ring, step0=step0, env_base=7)
        step0 += rew.shape[0]
    assert head.tolist() == [1, 1]
    want = ((((((1.0 + -0.01) + -0.01) + 1.0) + -0.01) + -0.01) + -1.0)
    assert ring[0] == _rec(want, 6, 7, 7, 2, COLL)
    assert cret.tolist() == [-0.01] and c.tolist() == [[1, 0]]  # the next episode is one step old
    assert all(ring[i] == _rec(0, 0, 0, 0, 0, 0) for i in (1, 2, 3))


def test_dones_at_the_first_and_the_last_row_and_two_dones_of_one_env():
    cret, c, head, ring = _empty(2, 8)
    cret[:] = [0.5, 0.0]
    c[:] = [[3, 1], [0, 0]]
    rew = np.array([[1.0, -0.01], [-0.01, -0.01], [-1.0, 1.0]])
    done = np.array([[1, 0], [0, 0], [1, 1]])
    fl = np.array([[GOAL | NOGOAL, 0], [0, 0], [COLL, GOAL | TIME]], dtype=np.uint8)
    ring, head, cret, c = EL.episode_log_reference(rew, done, fl, cret, c, head, ring, step0=10, members=[0, 1])
    assert head.tolist() == [3, 3]
    # (t, env) order: (0, 0), (2, 0), (2, 1); env 0 ends twice, its second episode starts from nothing
    assert ring[0] == _rec(0.5 + 1.0, 10, 0, 4, 2, GOAL | NOGOAL)
    assert ring[1] == _rec(-0.01 + -1.0, 12, 0, 2, 0, COLL)
    assert ring[2] == _rec((-0.01 + -0.01) + 1.0, 12, 1, 3, 1, GOAL | TIME | (1 << 8))
    assert cret.tolist() == [0.0, 0.0] and c.tolist() == [[0, 0], [0, 0]]


def test_the_ring_wraps_and_a_call_with_more_episodes_than_slots_skips_its_first_ranks():
    n, cap = 5, 3
    cret, c, head, ring = _empty(n, cap)
    rew = np.arange(10, dtype=np.float64).reshape(2, n)
    ones = np.ones((2, n), dtype=np.uint8)
    # a first call that ends two episodes, then one that ends ten: ranks 0..6 of it are never written
    ring, head, cret, c = EL.episode_log_reference(rew[:1], np.array([[1, 0, 0, 1, 0]]), None, cret, c, head, ring)
    assert head.tolist() == [2, 2] and [int(r["env"]) for r in ring] == [0, 3, 0] and ring[2] == _rec(0, 0, 0, 0, 0, 0)
    marked = ring.copy()
    ring, head, cret, c = EL.episode_log_reference(rew, ones, None, cret, c, head, ring, step0=1)
    assert head.tolist() == [12, 10]
    # episodes 9, 10, 11 (ranks 7, 8, 9 = (t 1, env 2), (1, 3), (1, 4)) sit in slots 0, 1, 2
    assert [int(r["env"]) for r in ring] == [2, 3, 4] and [int(r["step"]) for r in ring] == [2, 2, 2]
    assert [float(r["ret"]) for r in ring] == [7.0, 8.0, 9.0] and all(int(r["end"]) == 0 and int(r["goals"]) == 0 for r in ring)
    # the same as writing every rank in order, the later ones over the earlier
    big = np.zeros(64, dtype=EL.RECORD_DTYPE)
    big[:2] = marked[:2]
    cr, cc = np.zeros(n), np.zeros((n, 2), dtype=np.int32)
    cr[[1, 2, 4]] = rew[0, [1, 2, 4]]
    cc[[1, 2, 4], 0] = 1
    big, hb, _, _ = EL.episode_log_reference(rew, ones, None, cr, cc, np.array([2, 2]), big, step0=1)
    assert hb[0] == 12 and all(ring[i % cap] == big[i] for i in (9, 10, 11))


def test_two_calls_leave_what_one_call_leaves():
    rng = np.random.RandomState(3)
    n, K = 37, 9
    rew = rng.choice([1.0, -1.0, -0.01], size=(K, n))
    done = (rng.rand(K, n) < 0.3).astype(np.uint8)
    fl = rng.randint(0, 32, size=(K, n)).astype(np.uint8)
    for cap in (1, 5, 1000):
        one = EL.episode_log_reference(rew, done, fl, *_empty(n, cap))
        cret, c, head, ring = _empty(n, cap)
        ring, head, cret, c = EL.episode_log_reference(rew[:4], done[:4], fl[:4], cret, c, head, ring)
        two = EL.episode_log_reference(rew[4:], done[4:], fl[4:], cret, c, head, ring, step0=4)
        assert np.array_equal(one[0], two[0]) and one[1][0] == two[1][0]
        assert np.array_equal(one[2], two[2]) and np.array_equal(one[3], two[3])
    # the order is np.nonzero's
    ring = one[0]
    tt, ee = np.nonzero(done)
    assert ring["step"][:len(tt)].tolist() == tt.tolist() and ring["env"][:len(tt)].tolist() == ee.tolist()


# ------------------------------------------------------------------------------------------------------------------------------------
# EpisodeLog's reading side and its state, on a CPU stand-in for the env
# ------------------------------------------------------------------------------------------------------------------------------------
class _Env(object):
    def __init__(self, n):
        self.num_envs, self.device = n, torch.device("cpu")


def _log(n=6, cap=8, members=1):
    return EL.EpisodeLog(_Env(n), capacity=cap, n_members=members)


def _feed(log, rew, done, flags, members=None):
    """What append would leave, through the reference."""
    h, ring = log.head.numpy().copy(), log.ring.numpy().view(EL.RECORD_DTYPE).copy()
    ring, h, cret, c = EL.episode_log_reference(rew, done, flags, log.carry_return.numpy(), log.carry.numpy(), h, ring, step0=log.steps,
                                                members=members)
    log.ring.copy_(torch.from_numpy(ring.view(np.uint8)))
    log.head.copy_(torch.from_numpy(h))
    log.carry_return.copy_(torch.from_numpy(cret))
    log.carry.copy_(torch.from_numpy(c))
    log.steps += np.asarray(rew).shape[0]
    log._host_copy = None


def _block(seed, K, n, p=0.4):
    rng = np.random.RandomState(seed)
    ends = np.array([COLL, OOB, TIME, NOGOAL, COLL | OOB, GOAL | NOGOAL], dtype=np.uint8)
    done = (rng.rand(K, n) < p).astype(np.uint8)
    fl = np.where(done != 0, ends[rng.randint(0, len(ends), size=(K, n))], np.where(rng.rand(K, n) < 0.2, GOAL, 0)).astype(np.uint8)
    return rng.choice([1.0, -1.0, -0.01], size=(K, n)), done, fl


def test_records_come_back_in_append_order_with_an_exact_drop_count():
    log = _log(n=6, cap=8)
    assert log.records()[0].shape == (0,) and log.mean_last(100) is None and log.total() == 0
    rew, done, fl = _block(0, 7, 6, p=0.6)
    big = EL.episode_log_reference(rew, done, fl, *_empty(6, 1000))[0]
    total = int(np.count_nonzero(done))
    assert total > 8 + 3
    _feed(log, rew[:3], done[:3], fl[:3])
    first = int(np.count_nonzero(done[:3]))
    rec, dropped = log.records()
    assert dropped == 0 and np.array_equal(rec, big[max(0, first - 8):first])
    _feed(log, rew[3:], done[3:], fl[3:])
    assert log.total() == total and log.steps == 7
    rec, dropped = log.records()
    assert dropped == 0 and np.array_equal(rec, big[total - 8:total])
    rec, dropped = log.records(since=2)
    assert dropped == total - 8 - 2 and np.array_equal(rec, big[total - 8:total])
    rec, dropped = log.records(since=total - 3)
    assert dropped == 0 and np.array_equal(rec, big[total - 3:total])
    assert log.records(since=total)[0].shape == (0,)
    with pytest.raises(ValueError, match="since"):
        log.records(since=total + 1)


def test_mean_last_end_counts_and_timesteps():
    members = EL.member_of_envs(6, 3)
    assert members.tolist() == [0, 0, 1, 1, 2, 2] and EL.member_of_envs(6, slices=[1, 3, 2]).tolist() == [0, 1, 1, 1, 2, 2]
    log = _log(n=6, cap=64, members=3)
    rew, done, fl = _block(1, 9, 6)
    _feed(log, rew, done, fl, members)
    rec, _ = log.records()
    assert rec.shape[0] == int(np.count_nonzero(done)) > 12
    assert log.mean_last(5) == float(np.mean(rec["ret"][-5:])) and log.mean_last(10 ** 6) == float(np.mean(rec["ret"]))
    assert log.mean_last(0) is None
    for m in range(3):
        mine = rec[np.isin(rec["env"], np.nonzero(members == m)[0])]
        assert np.array_equal(EL.record_member(mine), np.full(mine.shape[0], m))
        assert log.mean_last(4, member=m) == float(np.mean(mine["ret"][-4:]))
    assert log.mean_last(4, member=3 + 200) is None
    assert log.timesteps(rec).tolist() == [(int(s) + 1) * 6 for s in rec["step"]]
    f = fl[done != 0]
    counts = log.end_counts(rec)
    assert counts == {"episodes": len(f), "collided": int(np.count_nonzero(f & COLL)), "out_of_bounds": int(np.count_nonzero(f & OOB)),
                      "max_steps": int(np.count_nonzero(f & TIME)), "no_goals_left": int(np.count_nonzero(f & NOGOAL))}
    assert counts["collided"] + counts["out_of_bounds"] + counts["max_steps"] + counts["no_goals_left"] > counts["episodes"]  # (not exclusive)
    from ship_sim_gym_amd import evaluate
    assert set(counts) - {"episodes"} <= set(evaluate.COLUMNS)


def _state_equal(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else (type(a[k]) is type(b[k]) and a[k] == b[k]) for k in a)


def test_state_round_trip_and_refusals_that_leave_the_object_unchanged():
    from ship_sim_gym_amd import checkpoint
    log = _log(n=6, cap=8)
    rew, done, fl = _block(2, 5, 6)
    _feed(log, rew, done, fl)
    log.rows_written, log.flushed = 3, 4
    sd = log.state_dict()
    checkpoint.check_plain(sd)
    assert set(sd) == {"capacity", "n_members", "num_envs", "ring", "head", "carry_return", "carry", "steps", "rows_written", "flushed"}
    twin = _log(n=6, cap=8)
    twin.load_state_dict(copy.deepcopy(sd))
    assert _state_equal(twin.state_dict(), sd) and np.array_equal(twin.records()[0], log.records()[0])
    fresh = _log(n=6, cap=8)
    _feed(fresh, *_block(5, 2, 6))
    before = fresh.state_dict()
    bad = [(k, {kk: v for kk, v in sd.items() if kk != k}) for k in sorted(sd)]
    bad += [("capacity", dict(sd, capacity=9)), ("n_members", dict(sd, n_members=2)), ("num_envs", dict(sd, num_envs=7)),
            ("ring", dict(sd, ring=sd["ring"][:-32])), ("ring", dict(sd, ring=sd["ring"].to(torch.int8))), ("head", dict(sd, head=[1, 2])),
            ("carry_return", dict(sd, carry_return=sd["carry_return"].float())), ("carry", dict(sd, carry=sd["carry"][:, :1])),
            ("steps", dict(sd, steps=1.5)), ("rows_written", dict(sd, rows_written="3")), ("flushed", dict(sd, flushed=True)),
            ("flushed", dict(sd, flushed=2)), ("flushed", dict(sd, flushed=10 ** 6)), ("steps", dict(sd, steps=-1))]
    for key, state in bad:
        with pytest.raises(ValueError, match=key):
            fresh.load_state_dict(state)
        assert _state_equal(fresh.state_dict(), before), key
    with pytest.raises(ValueError, match="a dict"):
        fresh.load_state_dict([1])
    for kw in (dict(capacity=0), dict(n_members=0), dict(n_members=N.POP_MAX_MEMBERS + 1)):
        with pytest.raises(ValueError):
            EL.EpisodeLog(_Env(4), **kw)


# ------------------------------------------------------------------------------------------------------------------------------------
# MonitorWriter
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows(path):
    with open(path) as f:
        return f.read().splitlines()


def test_monitor_file_header_rows_and_one_warning_for_dropped_records(tmp_path):
    path = str(tmp_path / "run.monitor.csv")
    members = EL.member_of_envs(6, 2)
    log = _log(n=6, cap=8, members=2)
    w = EL.MonitorWriter(path, log, env_id="ShipSim-v0")
    lines = _rows(path)
    assert len(lines) == 2 and lines[0].startswith("#") and lines[1] == "r,l,t,timesteps,env,member,goals,end"
    import json
    hdr = json.loads(lines[0][1:])
    assert set(hdr) == {"t_start", "env_id"} and hdr["env_id"] == "ShipSim-v0" and abs(hdr["t_start"] - w.t_start) == 0
    assert w.flush() == 0 and len(_rows(path)) == 2
    rew, done, fl = _block(4, 6, 6, p=0.5)
    big = EL.episode_log_reference(rew, done, fl, *_empty(6, 1000), members=members)[0]
    a = int(np.count_nonzero(done[:2]))
    assert 0 < a <= 8
    _feed(log, rew[:2], done[:2], fl[:2], members)
    assert w.flush() == a and (log.rows_written, log.flushed) == (a, a)
    assert w.flush() == 0
    hdr2, cols = EL.read_monitor(path)
    assert hdr2 == hdr and list(cols) == list(EL.MONITOR_COLUMNS)
    assert cols["r"].tolist() == big["ret"][:a].tolist() and cols["l"].tolist() == big["length"][:a].tolist()
    assert cols["timesteps"].tolist() == ((big["step"][:a] + 1) * 6).tolist() and cols["env"].tolist() == big["env"][:a].tolist()
    assert cols["member"].tolist() == members[big["env"][:a]].tolist() and cols["goals"].tolist() == big["goals"][:a].tolist()
    assert cols["end"].tolist() == (big["end"][:a] & 0xff).tolist() and np.all(cols["t"] >= 0) and len(set(cols["t"])) == 1
    # more episodes than slots between two flushes: the rows that survived, one warning with the count, none the second time
    total = int(np.count_nonzero(done))
    assert total - a > 8
    _feed(log, rew[2:], done[2:], fl[2:], members)
    with pytest.warns(RuntimeWarning, match=r"\b%d episodes" % (total - a - 8)):
        assert w.flush() == 8
    assert (log.rows_written, log.flushed) == (a + 8, total)
    assert EL.read_monitor(path)[1]["r"].tolist() == big["ret"][:a].tolist() + big["ret"][total - 8:total].tolist()
    _feed(log, *_block(9, 4, 6, p=0.9), members)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert w.flush() == 8
    # what pandas / load_results do with the file: skip the '#' line, take the header row
    body = _rows(path)[1:]
    assert all(len(line.split(",")) == 8 for line in body) and re.match(r"^-?\d", body[1])


def test_loading_a_state_cuts_the_file_back_to_its_rows(tmp_path):
    path = str(tmp_path / "m.csv")
    log = _log(n=6, cap=64)
    w = EL.MonitorWriter(path, log)
    blocks = [_block(s, 3, 6, p=0.5) for s in (11, 12, 13)]
    _feed(log, *blocks[0])
    w.flush()
    saved, kept = log.state_dict(), _rows(path)
    for b in blocks[1:]:
        _feed(log, *b)
        w.flush()
    whole = _rows(path)
    assert len(whole) > len(kept) > 2
    # a new process: the file is left as it is, the state cuts it back, and the same blocks give the same file but for t
    log2 = _log(n=6, cap=64)
    w2 = EL.MonitorWriter(path, log2, resume=True)
    assert _rows(path) == whole and w2.t_start == w.t_start
    log2.load_state_dict(saved)
    assert _rows(path) == kept
    for b in blocks[1:]:
        _feed(log2, *b)
        w2.flush()
    strip = lambda lines: [",".join(c for i, c in enumerate(line.split(",")) if i != 2) for line in lines[2:]]  # noqa: E731
    assert strip(_rows(path)) == strip(whole) and _rows(path)[:2] == whole[:2]
    # a file that holds fewer rows than the state: refused by name, log and file as they were
    log3 = _log(n=6, cap=64)
    w3 = EL.MonitorWriter(path, log3, resume=True)
    more = dict(saved, rows_written=len(whole), flushed=len(whole), head=torch.tensor([len(whole), 0]))
    before, lines = log3.state_dict(), _rows(path)
    with pytest.raises(ValueError, match="rows_written"):
        log3.load_state_dict(more)
    assert _state_equal(log3.state_dict(), before) and _rows(path) == lines and w3.t_start == w.t_start
    with pytest.raises(ValueError, match="not a monitor file"):
        EL.MonitorWriter(str(tmp_path / "absent.csv"), _log(), resume=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# the binding and the trainers' host side
# ------------------------------------------------------------------------------------------------------------------------------------
def test_ctypes_signatures_exist_for_every_new_header_function(native):
    text = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ssg_episode_log_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["ssg_episode_log_append", "ssg_episode_log_workspace_nbytes"]
    L = native.lib()
    for name in declared:
        assert name in native.EXPORTS and getattr(L, name).argtypes, name
    assert len(L.ssg_episode_log_append.argtypes) == 9 and len(L.ssg_episode_log_workspace_nbytes.argtypes) == 3
    assert C.sizeof(native.EpisodeRecord) == 32 == EL.RECORD_DTYPE.itemsize
    assert [(n, EL.RECORD_DTYPE.fields[n][1]) for n in EL.RECORD_DTYPE.names] == [(f[0], getattr(native.EpisodeRecord, f[0]).offset)
                                                                                 for f in native.EpisodeRecord._fields_]
    assert int(re.search(r"#define\s+SSG_EPISODE_LOG_MAX_CELLS\s+\(1 << (\d+)\)", text).group(1)) == 22 and native.EPISODE_LOG_MAX_CELLS == 1 << 22
    # the workspace call judges its arguments on the host
    nb = C.c_size_t()
    assert L.ssg_episode_log_workspace_nbytes(513, 5, C.byref(nb)) == 0 and nb.value == 16 + 4 * 5 * 3
    for args in ((0, 1), (1, 0), (256 * 4096 + 1, 1024), (1, (1 << 22) + 1)):
        assert L.ssg_episode_log_workspace_nbytes(args[0], args[1], C.byref(nb)) == -1, args
    assert L.ssg_episode_log_workspace_nbytes(256 * 4096, 1024, C.byref(nb)) == 0
    assert L.ssg_episode_log_workspace_nbytes(8, 1, None) == -1
    # ... and so does the append: a NULL handle or record before anything else
    assert L.ssg_episode_log_append(None, None, 1, 0, None, None, None, 0, None) == -1


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


def test_the_trainers_refuse_the_flags_on_the_host(monkeypatch, capsys):
    from gpu_support import load_script
    single, pbt = load_script("train/ppo_torch.py"), load_script("train/pbt_native.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    native_flags = ["--mode", "native", "--update", "native"]
    a = single.parse_args(native_flags + ["--episode-log", "m.csv", "--episode-log-capacity", "100", "--best-window", "100"])
    assert (a.episode_log, a.episode_log_capacity, a.best_window) == ("m.csv", 100, 100)
    a = single.parse_args([])
    assert (a.episode_log, a.episode_log_capacity, a.best_window) == (None, 65536, 0)
    rows = {r[0]: r for r in single.EPISODE_LOG_REQUIREMENTS}
    assert set(rows) == {"episode_log", "best_window"} and all(len(r) == len(single.REQUIREMENTS[0]) for r in rows.values())
    assert rows["episode_log"][3] == ("mode", "update") and rows["episode_log"][4] is True and rows["best_window"][3] == ("episode_log",)
    for argv, words in ((["--episode-log", "m.csv"], ("--episode-log", "--mode native")),
                        (["--mode", "native", "--episode-log", "m.csv"], ("--episode-log", "--update native")),
                        (native_flags + ["--best-window", "5"], ("--best-window", "--episode-log")),
                        (native_flags + ["--episode-log", "m.csv", "--gpus", "2"], ("--episode-log", "more than one rank")),
                        (native_flags + ["--episode-log-capacity", "5"], ("--episode-log-capacity", "--episode-log")),
                        (native_flags + ["--episode-log", "m.csv", "--episode-log-capacity", "0"], ("--episode-log-capacity",)),
                        (native_flags + ["--episode-log", "m.csv", "--best-window", "-1"], ("--best-window",))):
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv)
        err = capsys.readouterr().err
        assert ex.value.code not in (0, None) and all(w in err for w in words), (argv, err)
    for kw, words in ((dict(episode_log="m.csv"), ("episode_log", "mode='native'")),
                      (dict(episode_log="m.csv", mode="native"), ("episode_log", "update='native'")),
                      (dict(best_window=5, mode="native", update="native"), ("best_window", "episode_log")),
                      (dict(episode_log="m.csv", mode="native", update="native", episode_log_capacity=0), ("episode_log_capacity",))):
        with pytest.raises(ValueError) as ex:
            single.train(envs=8, updates=1, log=None, **kw)
        assert all(w in str(ex.value) for w in words), (kw, str(ex.value))
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match="episode_log") as ex:
        single.train(envs=8, updates=1, log=None, episode_log="m.csv", mode="native", update="native")
    assert "more than one rank" in str(ex.value)
    # the configuration and the section table
    cfg = single.run_config(episode_log="m.csv", best_window=100)
    assert (cfg["episode_log"], cfg["episode_log_capacity"], cfg["best_window"]) == ("m.csv", 65536, 100)
    assert single.run_config()["episode_log"] == "None" and pbt.run_config()["episode_log"] == "None"
    loop = single.loop
    assert loop.resume_sections(("a",), False, False) == ("a",) and loop.resume_sections(("a",), False, False, None) == ("a",)
    assert loop.resume_sections(("a",), True, True, "m.csv") == ("a", "obs_filter", "ret_filter", "episode_log")
    assert loop.resume_sections(("a",), False, False, "m.csv") == ("a", "episode_log")
    from ship_sim_gym_amd import checkpoint
    assert "episode_log" in checkpoint.SECTIONS
    # the population script's flags
    a = pbt.parse_args(["--episode-log", "p.csv"])
    assert (a.episode_log, a.episode_log_capacity) == ("p.csv", 65536) and pbt.parse_args([]).episode_log is None
    with pytest.raises(SystemExit):
        pbt.parse_args(["--episode-log-capacity", "7"])
    capsys.readouterr()
    import ship_sim_gym_amd
    assert ship_sim_gym_amd.EpisodeLog is EL.EpisodeLog and ship_sim_gym_amd.MonitorWriter is EL.MonitorWriter
