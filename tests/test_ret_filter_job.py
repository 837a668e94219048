"""CPU checks of the job-wide return filter (include/shipsim.h "Job-wide return filter"; ship_sim_gym_amd/ret_filter.py,
``ReturnFilter(job=True)``): the two entry points as header, binding and library see them and every refusal they add, on an unbound
handle (the library judges the arguments before the handle); the numpy restatements ``batch_rows_reference`` and ``job_reference``
against ``ret_filter_reference`` at one rank, their dependence on the rank order at three, rows of count 0, an empty base and a base count
of 2^40; the trainer's flag; and DataParallelPPO's decision about a plain filter in a job.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import load_script
from ret_filter_support import _ramp_inputs, _same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARDS = (257, 1, 2305)
NEW = {"ssg_ret_filter_batches": 8, "ssg_ret_filter_apply_rows": 10}
REW, DONE, OUT, DEN, ROWS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
NOT_BOUND = -3  # what a call that passed every host-side check answers on a handle without a state blob


# ------------------------------------------------------------------------------------------------------------------------------------
# header, binding, library; the refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(native):
    text = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = native.lib()
    for name, n_args in NEW.items():
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert decl and len(decl.group(1).split(",")) == n_args, name
        assert name in native.EXPORTS and hasattr(L, name) and len(getattr(L, name).argtypes) == n_args, name
    assert "Job-wide return filter (ABI 9 addition)" in text and native.ABI_VERSION == 9
    # the record, the plain call and the workspace formula are what they were
    assert C.sizeof(native.RetFilterRecord) == 72 and len(L.ssg_ret_filter_apply.argtypes) == 9
    need = C.c_size_t()
    assert L.ssg_ret_filter_workspace_nbytes(1000, 5, 1, C.byref(need)) == 0 and need.value == 8 * 5 * (2 * 4 + 1)


def _handle(native, n_envs=1000):
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _record(native, n_envs=1000, K=4, P=1, **kw):
    r = native.RetFilterRecord()
    r.struct_size = C.sizeof(native.RetFilterRecord)
    r.flags, r.n_members, r.reserved, r.clip, r.eps = native.RET_FILTER_UPDATE, P, 0, 10.0, 1e-8
    r.dev_gamma, r.dev_state, r.dev_carry, r.dev_workspace = 0x10000, 0x20000, 0x30000, 0x40000
    need = C.c_size_t()
    native.check(native.lib().ssg_ret_filter_workspace_nbytes(n_envs, K, max(1, min(P, 256)), C.byref(need)))
    r.workspace_nbytes = need.value
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def _batches(native, h, rec, K=4, rew=REW, done=DONE, stride=1000, rows=ROWS):
    return native.lib().ssg_ret_filter_batches(h, C.byref(rec) if rec is not None else None, K, C.c_void_p(rew), C.c_void_p(done), stride,
                                               C.c_void_p(rows), None)


def _apply_rows(native, h, rec, K=4, rows=ROWS, n_rows=2, rew=REW, stride=1000, out=OUT, den=DEN):
    return native.lib().ssg_ret_filter_apply_rows(h, C.byref(rec) if rec is not None else None, K, C.c_void_p(rows), n_rows, C.c_void_p(rew),
                                                  stride, C.c_void_p(out), C.c_void_p(den), None)


def test_refusals_come_before_the_handle(native):
    L = native.lib()
    h = _handle(native)
    good = _record(native)
    calls = {"ssg_ret_filter_batches": _batches, "ssg_ret_filter_apply_rows": _apply_rows}
    for name, call in calls.items():
        # nothing to refuse: as far as the handle's state blob; so with a padded stride, clip = eps = 0, K at the cap
        assert call(native, h, good) == NOT_BOUND, name
        assert call(native, h, _record(native, clip=0.0, eps=0.0), stride=1005) == NOT_BOUND
        kmax = native.RET_FILTER_MAX_STEPS
        assert call(native, h, _record(native, K=kmax), K=kmax) == NOT_BOUND
        # everything ssg_ret_filter_apply refuses of the record, K and the stride
        assert call(native, None, good) == -1 and call(native, h, None) == -1
        bad = [dict(struct_size=8), dict(struct_size=good.struct_size + 8), dict(n_members=0), dict(n_members=257), dict(dev_state=None),
               dict(dev_workspace=None), dict(dev_gamma=None), dict(dev_carry=None), dict(workspace_nbytes=good.workspace_nbytes - 1),
               dict(flags=2), dict(flags=3), dict(clip=-1.0), dict(eps=-1e-9), dict(clip=float("nan")), dict(eps=float("nan"))]
        for kw in bad:
            assert call(native, h, _record(native, **kw)) == -1, (name, kw)
            assert name.encode() in L.ssg_last_error(h)
        for kw in (dict(K=0), dict(K=-1), dict(K=kmax + 1), dict(stride=999), dict(rew=None)):
            assert call(native, h, _record(native, K=min(max(kw.get("K", 4), 1), kmax)), **kw) == -1, (name, kw)
        # what the job calls add: one member, an updating record, the rows
        for P in (2, 4):                                                   # (the plain call serves these: 1000 envs split)
            assert call(native, h, _record(native, P=P)) == -1 and b"one member" in L.ssg_last_error(h), (name, P)
        assert call(native, h, _record(native, flags=0)) == -1 and b"frozen" in L.ssg_last_error(h), name
        for rows, word in ((None, b"NULL rows"), (ROWS + 4, b"8-byte aligned"), (ROWS + 1, b"8-byte aligned")):
            assert call(native, h, good, rows=rows) == -1 and word in L.ssg_last_error(h), (name, rows)
        assert call(native, h, good, rows=ROWS + 8) == NOT_BOUND           # (8-byte aligned is enough)
    # ... each its own buffers
    assert _batches(native, h, good, done=None) == -1
    assert _apply_rows(native, h, good, out=None) == -1
    assert _apply_rows(native, h, good, out=REW) == -1 and b"must not be the reward buffer" in L.ssg_last_error(h)
    assert _apply_rows(native, h, good, den=None) == NOT_BOUND             # (the denoms are optional)
    for n_rows in (0, -1, native.DP_MAX_SHARDS + 1):
        assert _apply_rows(native, h, good, n_rows=n_rows) == -1 and b"n_rows" in L.ssg_last_error(h), n_rows
    for n_rows in (1, native.DP_MAX_SHARDS):
        assert _apply_rows(native, h, good, n_rows=n_rows) == NOT_BOUND, n_rows
    # rows that overlap the state's 32 bytes: K = 4 rows of 32 bytes per rank
    st, row_bytes = good.dev_state, 4 * 32
    for rows, n_rows, ok in ((st, 1, False), (st + 24, 1, False), (st + 32, 1, True), (st - row_bytes, 1, True), (st - row_bytes + 8, 1, False),
                             (st - 2 * row_bytes, 2, True), (st - 2 * row_bytes + 8, 2, False), (st - 2 * row_bytes + 8, 1, True)):
        assert _apply_rows(native, h, good, rows=rows, n_rows=n_rows) == (NOT_BOUND if ok else -1), (rows - st, n_rows)
        if not ok:
            assert b"overlap" in L.ssg_last_error(h)
    for rows, ok in ((st, False), (st + 24, False), (st + 32, True), (st - row_bytes, True), (st - row_bytes + 8, False)):
        assert _batches(native, h, good, rows=rows) == (NOT_BOUND if ok else -1), rows - st
    # a bound slices layout for another member count refuses one member, as the plain call does
    sizes = (C.c_int32 * 3)(300, 300, 400)
    assert L.ssg_pop_set_slices(h, 3, sizes, C.c_void_p(0x50000)) == 0
    assert _batches(native, h, good) == -1 and b"slices" in L.ssg_last_error(h)
    assert _apply_rows(native, h, good) == -1 and b"slices" in L.ssg_last_error(h)
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# the numpy restatements
# ------------------------------------------------------------------------------------------------------------------------------------
def _out(rew, denoms, clip):
    out = rew / denoms[:, None]
    return np.clip(out, -clip, clip) if clip > 0.0 else out


@pytest.mark.parametrize("n", (1, 257, 2305))
@pytest.mark.parametrize("gamma", (0.0, 0.99, 1.0))
def test_one_rank_is_the_plain_reference_bit_for_bit(n, gamma):
    from ship_sim_gym_amd.ret_filter import batch_rows_reference, job_reference, ret_filter_reference
    K, clip, eps = 5, 3.0, 1e-8
    rew, done = _ramp_inputs(K, n, 100 + n)
    rng = np.random.RandomState(n)
    carry0 = rng.uniform(-1.0, 1.0, n)
    for state0 in (np.zeros(4), np.array([0.25, 40.0, np.sqrt(40.0 / 999.0) + eps, 1000.0])):
        want_state, want_carry, want_out, want_den = ret_filter_reference(state0, carry0, rew, done, gamma, clip, eps)
        rows, carry = batch_rows_reference(carry0, rew, done, gamma)
        assert rows.shape == (K, 4) and (rows[:, 3] == n).all() and not rows[:, 2].any()
        state, denoms = job_reference(state0, rows[None], eps)
        assert _same_bits(state, want_state), (state, want_state)
        assert _same_bits(carry, want_carry) and _same_bits(denoms, want_den)
        assert _same_bits(_out(rew, denoms, clip), want_out)
    # two calls over K1 and K2 leave what one call leaves
    r1, c1 = batch_rows_reference(carry0, rew[:2], done[:2], gamma)
    r2, c2 = batch_rows_reference(c1, rew[2:], done[2:], gamma)
    assert _same_bits(np.concatenate([r1, r2]), rows) and _same_bits(c2, carry)
    s1, d1 = job_reference(state0, r1[None], eps)
    s2, d2 = job_reference(s1, r2[None], eps)
    assert _same_bits(s2, state) and _same_bits(np.concatenate([d1, d2]), denoms)


def _shard_rows(K, gamma, seed):
    from ship_sim_gym_amd.ret_filter import batch_rows_reference
    rows = []
    for r, n in enumerate(SHARDS):
        rew, done = _ramp_inputs(K, n, seed + r)
        rows.append(batch_rows_reference(np.zeros(n), rew * (r + 1.0), done, gamma)[0])
    return np.stack(rows)


def test_three_unequal_ranks_in_the_stated_order():
    from ship_sim_gym_amd.ret_filter import job_reference
    K, eps = 4, 1e-8
    rows = _shard_rows(K, 0.99, 7)
    state0 = np.array([0.25, 40.0, np.sqrt(40.0 / 999.0) + eps, 1000.0])
    state, denoms = job_reference(state0, rows, eps)
    again, denoms2 = job_reference(state0, rows.copy(), eps)
    assert _same_bits(state, again) and _same_bits(denoms, denoms2)       # one result for one order
    assert state[3] == 1000.0 + K * sum(SHARDS)
    # the header's chain, by hand in scalar floats: step_k from rows[0][k] on, in rank order, then into the state
    def merge(a, b):
        if b[0] == 0.0:
            return a
        if a[0] == 0.0:
            return b
        n2 = a[0] + b[0]
        w = b[0] / n2
        d = b[1] - a[1]
        return n2, a[1] + d * w, (a[2] + b[2]) + (d * d) * (a[0] * w)
    s = (float(state0[3]), float(state0[0]), float(state0[1]))
    for k in range(K):
        a = (float(rows[0, k, 3]), float(rows[0, k, 0]), float(rows[0, k, 1]))
        for r in (1, 2):
            a = merge(a, (float(rows[r, k, 3]), float(rows[r, k, 0]), float(rows[r, k, 1])))
        s = merge(s, a)
        assert denoms[k] == np.sqrt(np.float64(s[2]) / (s[0] - 1.0)) + eps
    assert (state[3], state[0], state[1]) == s
    # another order is another result: the order is part of the definition
    others = [job_reference(state0, rows[list(p)], eps)[0] for p in ((1, 0, 2), (0, 2, 1), (2, 1, 0))]
    assert all(o[3] == state[3] for o in others)
    assert any(not _same_bits(o[:2], state[:2]) for o in others)
    assert all(np.allclose(o[:2], state[:2], rtol=1e-12) for o in others)  # (the same statistics, to rounding)
    # the merged statistics are those of the concatenated samples
    with_stats = job_reference(np.zeros(4), rows[:, :1], eps)[0]
    assert with_stats[3] == sum(SHARDS)
    mean = sum(rows[r, 0, 0] * n for r, n in enumerate(SHARDS)) / sum(SHARDS)
    assert abs(with_stats[0] - mean) <= 1e-12 * max(1.0, abs(mean))


def test_rows_of_count_zero_are_skipped():
    from ship_sim_gym_amd.ret_filter import job_reference
    K, eps = 3, 1e-8
    rows = _shard_rows(K, 0.99, 11)
    state0 = np.array([-0.5, 9.0, np.sqrt(9.0 / 99.0) + eps, 100.0])
    want = job_reference(state0, rows, eps)
    junk = np.zeros((1, K, 4))
    junk[0, :, 0], junk[0, :, 1] = 1e300, np.nan                          # (a count of 0: mean and M2 are not read)
    for at in range(4):                                                   # first, between, last
        got = job_reference(state0, np.concatenate([rows[:at], junk, rows[at:]]), eps)
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), at
    # a step whose rows are all empty leaves the state and repeats its denom; empty rows alone leave the state as it is
    holes = rows.copy()
    holes[:, 1] = junk[0, 1]
    got = job_reference(state0, holes, eps)
    assert got[1][1] == got[1][0] and got[0][3] == 100.0 + 2 * sum(SHARDS)
    assert _same_bits(got[0], job_reference(state0, rows[:, [0, 2]], eps)[0])
    state, denoms = job_reference(state0, junk, eps)
    assert _same_bits(state[[0, 1, 3]], state0[[0, 1, 3]]) and (denoms == np.sqrt(9.0 / 99.0) + eps).all()


def test_empty_base_and_a_base_count_of_2_to_40():
    from ship_sim_gym_amd.ret_filter import job_reference
    K, eps = 3, 1e-8
    rows = _shard_rows(K, 1.0, 13)
    # an empty base: the state after step 0 is step 0 itself, exactly
    state, denoms = job_reference(np.zeros(4), rows[:, :1], eps)
    step0 = job_reference(np.zeros(4), rows[:1, :1], eps)[0]               # rank 0 alone ...
    assert state[3] == sum(SHARDS) and step0[3] == SHARDS[0] and _same_bits(step0[:2], rows[0, 0, :2])
    n = float(sum(SHARDS))
    assert denoms[0] == np.sqrt(state[1] / (n - 1.0)) + eps
    # ... and one sample in all: no variance, the denom is 1
    one = np.array([[[0.7, 0.0, 0.0, 1.0]]])
    state, denoms = job_reference(np.zeros(4), one, eps)
    assert _same_bits(state, np.array([0.7, 0.0, 1.0, 1.0])) and denoms[0] == 1.0
    # a base of 2^40 returns: the counts stay exact, the mean moves by delta * n / (2^40 + n)
    big = 2.0 ** 40
    state0 = np.array([0.125, big * 4.0, np.sqrt(big * 4.0 / (big - 1.0)) + eps, big])
    state, denoms = job_reference(state0, rows, eps)
    assert state[3] == big + K * sum(SHARDS) and int(state[3]) == 2 ** 40 + K * sum(SHARDS)
    assert np.isfinite(state).all() and abs(state[0] - 0.125) < 1e-3 and state[1] >= big * 4.0
    # (a step adds at most n (3 * 2600)^2 < 1.6e11 to an M2 of 4.4e12, the ramp's samples being below 3 * 2600: the variance stays in 4 .. 4.5)
    assert np.all((denoms > 1.999) & (denoms < np.sqrt(4.5)))
    # eps = 0 on constant returns: a denom of 0 divides by 1, the state keeps the 0
    const = np.array([[[1.5, 0.0, 0.0, 4.0]], [[1.5, 0.0, 0.0, 2.0]]])
    state, denoms = job_reference(np.zeros(4), const, 0.0)
    assert _same_bits(state, np.array([1.5, 0.0, 0.0, 6.0])) and denoms[0] == 1.0
    for bad in (np.zeros((2, 4)), np.zeros((0, 2, 4)), np.zeros((1, 0, 4)), np.zeros((1, 2, 3))):
        with pytest.raises(ValueError, match="job_reference"):
            job_reference(np.zeros(4), bad)


# ------------------------------------------------------------------------------------------------------------------------------------
# the Python class, the trainer's flag, the job's decision
# ------------------------------------------------------------------------------------------------------------------------------------
class _Env(object):
    num_envs, device = 8, "cpu"


def test_job_filter_construction_and_state_dict():
    import torch
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    plain, job = ReturnFilter(_Env()), ReturnFilter(_Env(), job=True, clip=5.0)
    assert plain.job is False and job.job is True
    for P in (2, 4):
        with pytest.raises(ValueError, match="one member"):
            ReturnFilter(_Env(), n_members=P, job=True)
    assert sorted(job.state_dict()) == sorted(plain.state_dict()) == ["carry", "clip", "eps", "gamma", "n_members", "state"]
    job.state.copy_(torch.tensor([[0.5, 2.0, 1.0, 3.0]], dtype=torch.float64))
    job.carry.copy_(torch.arange(8, dtype=torch.float64))
    for other in (ReturnFilter(_Env(), job=True), ReturnFilter(_Env())):   # (a plain filter reads a job's dict, and the reverse)
        other.load_state_dict(job.state_dict())
        assert torch.equal(other.state, job.state) and torch.equal(other.carry, job.carry) and other.clip == 5.0
    batch = {"rew": torch.zeros((2, 8), dtype=torch.float64), "done": torch.zeros((2, 8), dtype=torch.uint8)}
    for call in (lambda: plain.shard_rows(batch), lambda: plain.apply_rows(batch, torch.zeros((1, 2, 4), dtype=torch.float64))):
        with pytest.raises(ValueError, match="job=True"):
            call()
    for rows in (torch.zeros((2, 4), dtype=torch.float64), torch.zeros((0, 2, 4), dtype=torch.float64), torch.zeros((65, 2, 4), dtype=torch.float64),
                 torch.zeros((1, 2, 4)), torch.zeros((1, 3, 4), dtype=torch.float64), torch.zeros((1, 2, 3), dtype=torch.float64)):
        with pytest.raises(ValueError, match="apply_rows"):
            job.apply_rows(batch, rows)
    with pytest.raises(ValueError, match="frozen"):
        job.train(False).shard_rows(batch)


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


def test_trainer_flag_and_its_refusals(capsys, monkeypatch):
    single = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    native_flags = ["--mode", "native", "--update", "native"]
    assert single.parse_args([]).job_norm_reward is False
    for extra in ([], ["--gpus", "2"], ["--gpus", "8"], ["--reward-clip", "5"]):  # one rank or more; --reward-clip applies
        assert single.parse_args(native_flags + ["--job-norm-reward"] + extra).job_norm_reward is True
    # its row is in a table of its own; REQUIREMENTS keeps exactly its rows
    assert [r[0] for r in single.REQUIREMENTS] == ["save_obs_filter", "obs_filter", "norm_reward", "timeout_bootstrap", "eval_every", "perm",
                                                   "resume", "save_every", "adv_norm", "ranks", "update"]
    (row,) = single.JOB_NORM_REWARD_REQUIREMENTS
    assert row[:2] == ("job_norm_reward", "--job-norm-reward") and row[3] == ("mode", "update") and row[4] is False
    for argv, words in ((["--job-norm-reward"], ("--job-norm-reward", "--mode native")),
                        (["--mode", "native", "--job-norm-reward"], ("--job-norm-reward", "--update native")),
                        (native_flags + ["--job-norm-reward", "--norm-reward"], ("--job-norm-reward", "together with --norm-reward")),
                        (native_flags + ["--norm-reward", "--gpus", "2"], ("--norm-reward", "more than one rank")),
                        (native_flags + ["--job-norm-reward", "--norm-reward", "--gpus", "2"], ("--job-norm-reward", "together with --norm-reward")),
                        (native_flags + ["--reward-clip", "5"], ("--reward-clip", "--norm-reward")),
                        (native_flags + ["--job-norm-reward", "--resume", "f.ckpt", "--gpus", "2"], ("--resume", "more than one rank"))):
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv)
        err = capsys.readouterr().err
        assert ex.value.code not in (0, None) and all(w in err for w in words), (argv, err)
    for kw, words in ((dict(job_norm_reward=True), ("job_norm_reward", "mode='native'")),
                      (dict(job_norm_reward=True, mode="native"), ("job_norm_reward", "update='native'")),
                      (dict(job_norm_reward=True, norm_reward=True, mode="native", update="native"), ("job_norm_reward", "together with norm_reward"))):
        with pytest.raises(ValueError) as ex:
            single.train(envs=8, updates=1, log=None, **kw)
        assert all(w in str(ex.value) for w in words), (kw, str(ex.value))
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match="norm_reward") as ex:
        single.train(envs=8, updates=1, log=None, mode="native", update="native", norm_reward=True)
    assert "more than one rank" in str(ex.value)
    # the flag is part of a run's configuration, and a resumed run of it needs the filter's section
    assert single.run_config(job_norm_reward=True)["job_norm_reward"] is True and single.run_config()["job_norm_reward"] is False
    assert "job_norm_reward" not in single.CONFIG_EXEMPT
    assert "--job-norm-reward" in single.make_arg_parser().format_help()
    from train import loop
    assert loop.resume_sections(("a",), False, True) == ("a", "ret_filter")


def test_a_plain_filter_is_refused_in_a_job_of_two_ranks():
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    plain, job = ReturnFilter(_Env()), ReturnFilter(_Env(), job=True)
    for world in (2, 8):
        with pytest.raises(ValueError, match="job=True"):
            dp.check_return_filter(plain, world)
        dp.check_return_filter(job, world)
        dp.check_return_filter(None, world)
    dp.check_return_filter(plain, 1)                                       # (one rank: its statistics are the job's)
    dp.check_return_filter(job, 1)
