"""GPU checks of the job-wide episode log (ssg_job_episode_log_shard / ssg_job_episode_log_merge_blocks; EpisodeLog(job=True)).  The inputs are
tests/test_episode_log_gpu.py's synthetic [K, N] buffers and an env serves as the handle only, but for the trainer runs at the end.  The
references are ``shard_block_reference`` and ``merge_blocks_reference`` (tests/test_episode_log_job.py shows on the host that the two
compose to ``episode_log_reference`` over all envs); every comparison is of bytes.

Shapes: shards of 1, 63, 64, 65 and 257 envs (one env; below / at / above a wave; a tile and one env) x K in (1, 5, 9) (one row; below
and above the walk's eight-row staging) x the five done patterns; jobs of W in (1, 2, 3, 8) with unequal shards; the capacities 1,
count - 1, count, count + 1 and a prime below count."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from episode_log_job_support import FILL, JOBS, PATTERNS, Job, Single, capacities, inputs, shard_ranges
from gpu_support import DEV, load_script, torch_cuda, vec  # noqa: F401
from ret_filter_support import handles  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(torch, arrays, pad=0):
    """Device copies as [:, :n] views of buffers with a row pitch of n + pad (the padding holds NaN / 0xFF: a done byte there would count)."""
    out = []
    for a in arrays:
        K, n = a.shape
        t = torch.full((K, n + pad), float("nan") if a.dtype == np.float64 else 0xFF, dtype=torch.float64 if a.dtype == np.float64 else torch.uint8,
                       device=DEV)
        t[:, :n] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        out.append(t[:, :n])
    return out


def _batch(torch, a, pad=0):
    return dict(zip(("rew", "done", "flags"), _dev(torch, a, pad)))


def _job_log(env, cap, rows, W, total):
    """A job log whose ring holds a known pattern (a slot no rank owns keeps it)."""
    from ship_sim_gym_amd.episode_log import EpisodeLog
    log = EpisodeLog(env, capacity=cap, job=True, rows=rows, world=W, total_envs=total)
    log.ring.fill_(FILL)
    return log


def _same_block(got, want, rows, S, what):
    """Header, lb (with its tail past K and its padding) and the slots the call's episodes own."""
    from ship_sim_gym_amd.episode_log import block_layout, block_owned_slots, block_views
    lb_n, rec_off, nbytes = block_layout(rows, S)
    assert got.shape == want.shape == (nbytes,)
    assert got[:32].tobytes() == want[:32].tobytes(), ("header", what, block_views(got, rows, S)[0], block_views(want, rows, S)[0])
    assert got[32:rec_off].tobytes() == want[32:rec_off].tobytes(), ("lb", what)
    owned = block_owned_slots(int(block_views(want, rows, S)[0]["count"][0]), S)
    assert block_views(got, rows, S)[2][owned].tobytes() == block_views(want, rows, S)[2][owned].tobytes(), ("slots", what)


SHARDS = [(n, K) for n in (1, 63, 64, 65, 257) for K in (1, 5, 9)]


@pytest.mark.parametrize("n,K", SHARDS, ids=["n%d-K%d" % s for s in SHARDS])
def test_the_shard_call_is_the_reference_byte_for_byte(torch_cuda, handles, n, K):
    torch = torch_cuda
    from ship_sim_gym_amd.episode_log import shard_block_reference
    env = handles(n)
    for pi, pattern in enumerate(PATTERNS):
        a, b = inputs(K, n, pattern, 1000 * n + 10 * K + pi), inputs(K, n, pattern, 1000 * n + 10 * K + pi + 5)
        da, db = _batch(torch, a), _batch(torch, b)
        counts = [int(np.count_nonzero(x[1])) for x in (a, b)]
        rows = K + pi % 3
        for cap in sorted({max(1, c) for c in (1, min(counts) - 1, max(counts) + 1, rows * n)}):  # S below, at and above a call's count
            log = _job_log(env, cap, rows, 2, 2 * n)  # (two equal shards: S = min(cap, rows * n))
            S = log.stage
            assert S == min(cap, rows * n)
            log.to_native(K)
            log.workspace.fill_(0xFF)  # (neither the workspace's nor the block's contents enter the result)
            cret, c = np.zeros(n), np.zeros((n, 2), dtype=np.int32)
            for call, (x, dx) in enumerate(((a, da), (b, db))):
                out = torch.full((log.block_nbytes,), 0xEE, dtype=torch.uint8, device=DEV)
                got = log.shard_block(dx, out=out).cpu().numpy()
                want, cret, c = shard_block_reference(*x, cret, c, rows, S, step0=log.steps, env_base=0)
                _same_block(got, want, rows, S, (pattern, cap, call))
                assert log.carry_return.cpu().numpy().tobytes() == cret.tobytes() and log.carry.cpu().numpy().tobytes() == c.tobytes(), (pattern, cap, call)
                log._pending, log.steps = None, log.steps + K  # (no merge here: the next block's steps follow)
            assert not log.head.any() and bool((log.ring == FILL).all())  # the shard call leaves the job's ring alone


@pytest.mark.parametrize("n,K,pad", [(257, 5, 7), (65, 9, 1)])
def test_the_shard_call_with_a_padded_row_pitch_and_an_env_id_base(torch_cuda, n, K, pad):
    torch = torch_cuda
    from ship_sim_gym_amd.episode_log import block_views, shard_block_reference
    env = vec(n, 7, base=1000)
    a = inputs(K, n, "p0.3", n + K)
    d = _batch(torch, a, pad)
    assert d["rew"].stride(0) == n + pad
    log = _job_log(env, 4096, K, 3, 3 * n - 1)
    got = log.shard_block(d, out=torch.full((log.block_nbytes,), 0xEE, dtype=torch.uint8, device=DEV)).cpu().numpy()
    want, cret, c = shard_block_reference(*a, np.zeros(n), np.zeros((n, 2), dtype=np.int32), K, log.stage, step0=0, env_base=1000)
    _same_block(got, want, K, log.stage, "padded")
    tt, ee = np.nonzero(a[1])
    slots = block_views(got, K, log.stage)[2][:len(tt)]
    assert slots["step"].tolist() == tt.tolist() and slots["env"].tolist() == (ee + 1000).tolist()
    assert log.carry_return.cpu().numpy().tobytes() == cret.tobytes()
    env.close()


MERGES = [(W, n, K) for W, n in JOBS for K in (5,)] + [(3, 191, 1), (8, 517, 9), (2, 3, 9)]


@pytest.mark.parametrize("W,n,K", MERGES, ids=["W%d-n%d-K%d" % m for m in MERGES])
def test_the_merge_call_is_the_reference_byte_for_byte(torch_cuda, handles, W, n, K):
    """Host-made blocks (shard_block_reference per shard), stacked and merged on the device against merge_blocks_reference; two calls,
    so that the second finds the head where the first left it and wraps the ring."""
    torch = torch_cuda
    env = handles(1)
    for pi, pattern in enumerate(PATTERNS):
        a, b = inputs(K, n, pattern, 100000 * W + 100 * n + 10 * K + pi), inputs(K, n, pattern, 100000 * W + 100 * n + 10 * K + pi + 5)
        count = int(np.count_nonzero(a[1]) + np.count_nonzero(b[1]))
        rows = K + pi % 3
        for cap in capacities(count):
            job, one = Job(n, W, cap, rows), Single(n, cap)
            log = _job_log(env, cap, rows, W, n)
            assert log.stage == job.stage
            for call, x in enumerate((a, b)):
                step0 = job.steps
                job.append(*x)
                one.append(*x)
                log.merge_blocks(torch.from_numpy(job.blocks).to(DEV), K=K, step0=step0)
                assert log.ring.cpu().numpy().tobytes() == job.ring.tobytes() == one.ring.tobytes(), ("ring", pattern, cap, call)
                assert log.head.cpu().numpy().tolist() == job.head.tolist() == one.head.tolist(), ("head", pattern, cap, call)
                assert log.steps == job.steps


def test_one_rank_job_append_is_append_bit_for_bit(torch_cuda, handles):
    torch = torch_cuda
    from ship_sim_gym_amd.episode_log import EpisodeLog
    n, K = 257, 9
    env = handles(n)
    for pattern in PATTERNS:
        a, b = inputs(K, n, pattern, 31), inputs(K - 4, n, pattern, 32)
        for cap in (1, 97, 100000):
            job, own = EpisodeLog(env, capacity=cap, job=True, rows=K), EpisodeLog(env, capacity=cap)
            assert (job.world, job.total_envs, job.stage) == (1, n, min(cap, K * n))
            for log in (job, own):
                log.ring.fill_(FILL)
            for x in (a, b):
                job.job_append(_batch(torch, x))
                own.append(_batch(torch, x))
                for name in ("ring", "head", "carry_return", "carry"):
                    assert torch.equal(getattr(job, name), getattr(own, name)), (name, pattern, cap)
            assert job.steps == own.steps == 2 * K - 4
    job = EpisodeLog(env, capacity=64, job=True, rows=K)
    with pytest.raises(ValueError, match="job_append"):
        job.append(_batch(torch, a))
    with pytest.raises(ValueError, match="job=True"):
        EpisodeLog(env, capacity=64).job_append(_batch(torch, a))
    with pytest.raises(ValueError, match="SSG_EPISODE_LOG_MAX_CELLS"):
        EpisodeLog(env, capacity=64, job=True, rows=(1 << 22) // 2 + 1)


def _replay(torch, logs, ranges, x, pad=0):
    """One call of a replayed job: every shard's block, torch.stack as the gather, every shard's merge."""
    blocks = [log.shard_block(_batch(torch, [v[:, lo:hi] for v in x], pad)) for log, (lo, hi) in zip(logs, ranges)]
    stacked = torch.stack(blocks)
    for log in logs:
        log.merge_blocks(stacked)
    return stacked


def test_three_shards_replayed_in_one_process(torch_cuda):
    """Shards of 64, 64 and 63 envs over their own handles against ONE EpisodeLog.append_rows over a 191-env handle; and K1 then K2
    against K1 + K2 (a batch of more rows than `rows` goes in pieces)."""
    torch = torch_cuda
    from ship_sim_gym_amd.episode_log import EpisodeLog
    n, W, K1, K2, base = 191, 3, 5, 9, 500
    ranges = shard_ranges(n, W)
    assert [hi - lo for lo, hi in ranges] == [64, 64, 63]
    envs, whole = [vec(hi - lo, 7, base=base + lo) for lo, hi in ranges], vec(n, 7, base=base)
    for pattern in ("p0.3", "p1", "last_row"):
        a = inputs(K1 + K2, n, pattern, 77)
        count = int(np.count_nonzero(a[1]))
        for cap in (max(1, count // 3), count + 5):
            logs = [_job_log(env, cap, K2, W, n) for env in envs]
            one, two = EpisodeLog(whole, capacity=cap), EpisodeLog(whole, capacity=cap)
            one.ring.fill_(FILL)
            two.ring.fill_(FILL)
            _replay(torch, logs, ranges, [v[:K1] for v in a], pad=3)
            one.append_rows(*_dev(torch, [v[:K1] for v in a]))
            for log in logs:
                assert torch.equal(log.ring, one.ring) and torch.equal(log.head, one.head), (pattern, cap, "K1")
            _replay(torch, logs, ranges, [v[K1:] for v in a])
            one.append_rows(*_dev(torch, [v[K1:] for v in a]))
            two.append_rows(*_dev(torch, a))  # K1 + K2 in one call
            for log in logs:
                assert torch.equal(log.ring, one.ring) and torch.equal(log.head, one.head), (pattern, cap, "K2")
                assert torch.equal(log.ring, two.ring) and int(log.head[0]) == int(two.head[0]) == count
            assert torch.equal(torch.cat([log.carry_return for log in logs]), one.carry_return)
            assert torch.equal(torch.cat([log.carry for log in logs]), one.carry)
            rec, dropped = logs[1].records()
            want, _ = one.records()
            assert rec.tobytes() == want.tobytes() and logs[0].timesteps(rec).tolist() == ((rec["step"] + 1) * n).tolist()
    # job_append on a one-rank log cuts a batch of more than `rows` rows into pieces
    a = inputs(K1 + K2, n, "p0.3", 78)
    job, one = EpisodeLog(whole, capacity=4096, job=True, rows=4), EpisodeLog(whole, capacity=4096)
    job.job_append(_batch(torch, a))
    one.append(_batch(torch, a))
    assert torch.equal(job.ring, one.ring) and int(job.head[0]) == int(one.head[0]) and torch.equal(job.carry, one.carry) and job.steps == K1 + K2
    for env in envs + [whole]:
        env.close()


def _native_record(N, torch, ring_t, head_t, cap):
    rec = N.EpisodeLogRecord()
    rec.struct_size = C.sizeof(N.EpisodeLogRecord)
    rec.n_members, rec.capacity = 1, cap
    rec.dev_records, rec.dev_head = ring_t.data_ptr(), head_t.data_ptr()
    return rec


def test_malformed_blocks_are_skipped_inside_the_ring(torch_cuda, handles):
    """Host-made blocks with a record step outside the call, an lb that overruns the count, and counts the block cannot hold: the merge
    is merge_blocks_reference (which skips them), and a guard region on either side of the ring keeps its bytes."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.episode_log import block_views, merge_blocks_reference
    env = handles(1)
    n, W, K, rows, cap, G = 127, 2, 5, 6, 61, 64
    good = Job(n, W, cap, rows).append(*inputs(K, n, "p0.3", 3))
    S = good.stage

    def step_outside(b):
        slots = block_views(b[1], rows, S)[2]
        slots["step"][0], slots["step"][1], slots["step"][2] = K, -1, 2 ** 40

    def lb_overrun(b):  # block 0 claims 1 000 episodes more in every row: block 1's ranks move up by 1 000, all of them alike
        block_views(b[0], rows, S)[1][1:K + 1] += 1000

    def lb_negative(b):
        block_views(b[0], rows, S)[1][:] = -7
        block_views(b[1], rows, S)[1][:] = -7

    def count_beyond(b):
        block_views(b[0], rows, S)[0]["count"] = 2 ** 50 + 3
        block_views(b[1], rows, S)[0]["count"] = -4

    for name, spoil in (("good", lambda b: None), ("step", step_outside), ("lb", lb_overrun), ("lb<0", lb_negative), ("count", count_beyond)):
        blocks = good.blocks.copy()
        spoil(blocks)
        buf = torch.full(((cap + 2 * G) * 32,), 0xCD, dtype=torch.uint8, device=DEV)
        head = torch.tensor([cap - 3, 0], dtype=torch.int64, device=DEV)  # (the call wraps the ring)
        rec = _native_record(N, torch, buf[G * 32:], head, cap)
        dev_blocks = torch.from_numpy(blocks).to(DEV)
        rc = N.lib().ssg_job_episode_log_merge_blocks(env._h, C.byref(rec), K, 0, rows, S, C.c_void_p(dev_blocks.data_ptr()), W, env._stream())
        assert rc == 0, (name, N.lib().ssg_last_error(env._h))
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        ring, want_head = merge_blocks_reference(blocks, np.full(cap * 32, 0xCD, dtype=np.uint8).view(good.ring.dtype), [cap - 3, 0], K, 0, rows, S)
        assert (got[:G * 32] == 0xCD).all() and (got[(G + cap) * 32:] == 0xCD).all(), ("guard", name)
        written = np.flatnonzero((ring.view(np.uint8).reshape(cap, 32) != 0xCD).any(axis=1))
        # no two surviving records of any of these blocks meet in a slot (shown below for the overrun): the ring is the reference's, every byte
        assert got[G * 32:(G + cap) * 32].tobytes() == ring.tobytes(), ("ring", name)
        assert head.cpu().numpy().tolist() == want_head.tolist(), ("head", name)
        if name == "good":
            assert len(written) == min(cap, int(want_head[1])) and int(want_head[1]) == int(np.count_nonzero(inputs(K, n, "p0.3", 3)[1]))
        if name == "lb":
            # a block's own lb cancels in its records' R, so block 0's keep R = their true rank, below total - capacity now: skipped; block
            # 1's are true rank + 1 000, distinct, and those of the last `cap` true ranks survive, each in a slot of its own
            env_of_rank = (np.nonzero(inputs(K, n, "p0.3", 3)[1])[1])  # np.nonzero's order is the rank order
            survivors = int(np.count_nonzero(env_of_rank[-cap:] >= 64))  # shard 1 owns envs 64 .. 126
            assert int(want_head[1]) == len(env_of_rank) + 1000 and 0 < survivors < cap and len(written) == survivors
            assert set(ring[written]["env"].tolist()) <= set(range(64, 127))
        if name == "lb<0":
            assert int(want_head[1]) == 0 and len(written) == 0


def test_every_refusal_is_bad_arg_and_leaves_head_and_ring(torch_cuda, handles):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    n, K, rows, S = 257, 3, 4, 50
    env = handles(n)
    a = inputs(K, n, "p1", 5)
    d = _batch(torch, a)
    log = _job_log(env, 64, rows, 2, 2 * n)
    log.stage = S
    good = log.to_native(rows)
    L, h = N.lib(), env._h
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    nb = C.c_size_t()
    assert L.ssg_job_episode_log_block_nbytes(rows, S, C.byref(nb)) == 0 and nb.value == 32 + 32 + 32 * S
    assert L.ssg_job_episode_log_block_nbytes(3, 1, C.byref(nb)) == 0 and nb.value == 32 + 16 + 32
    for args in ((0, 1), (1, 0), (-1, 5), (N.EPISODE_LOG_MAX_CELLS + 1, 1), (2 ** 31 - 1, 1)):
        assert L.ssg_job_episode_log_block_nbytes(args[0], args[1], C.byref(nb)) == -1, args
    assert L.ssg_job_episode_log_block_nbytes(1, 1, None) == -1
    L.ssg_job_episode_log_block_nbytes(rows, S, C.byref(nb))
    block = torch.full((2 * nb.value + 16,), 0xEE, dtype=torch.uint8, device=DEV)

    def changed(**kw):
        rec = N.EpisodeLogRecord.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(rec, k, v)
        return rec

    def shard(rec=good, K=K, rew=vp(d["rew"]), done=vp(d["done"]), stride=n, handle=h, rows=rows, stage=S, blk=block.data_ptr(), nbytes=nb.value):
        return L.ssg_job_episode_log_shard(handle, C.byref(rec) if rec is not None else None, K, 0, rew, done, vp(d["flags"]), stride, rows, stage,
                                       C.c_void_p(blk) if blk is not None else None, nbytes, env._stream())

    def merge(rec=good, K=K, handle=h, rows=rows, stage=S, blk=block.data_ptr(), n_blocks=2):
        return L.ssg_job_episode_log_merge_blocks(handle, C.byref(rec) if rec is not None else None, K, 0, rows, stage,
                                              C.c_void_p(blk) if blk is not None else None, n_blocks, env._stream())

    ring_ptr = good.dev_records
    both = {"a NULL handle": dict(handle=None), "a NULL record": dict(rec=None), "struct_size": dict(rec=changed(struct_size=8)),
            "capacity 0": dict(rec=changed(capacity=0)), "n_members 2": dict(rec=changed(n_members=2)), "n_members 0": dict(rec=changed(n_members=0)),
            "K 0": dict(K=0), "K < 0": dict(K=-1), "K > rows": dict(K=rows + 1), "rows 0": dict(rows=0),
            "rows above the bound": dict(rows=N.EPISODE_LOG_MAX_CELLS + 1), "rows at INT_MAX": dict(rows=2 ** 31 - 1), "stage 0": dict(stage=0),
            "stage < 0": dict(stage=-3), "a NULL block": dict(blk=None), "a block that is not 16-byte aligned": dict(blk=block.data_ptr() + 8),
            "NULL dev_records": dict(rec=changed(dev_records=None)), "NULL dev_head": dict(rec=changed(dev_head=None)),
            "records not 16-byte aligned": dict(rec=changed(dev_records=ring_ptr + 8)),
            "a block inside the ring": dict(blk=ring_ptr, rec=changed(capacity=1 << 20)),
            "a block that ends inside the ring": dict(rec=changed(dev_records=block.data_ptr() + nb.value - 32))}
    only_shard = {"n_members that does not divide": dict(rec=changed(n_members=2)), "stride < n_envs": dict(stride=n - 1), "NULL reward": dict(rew=None),
                  "NULL done": dict(done=None), "workspace too small": dict(rec=changed(workspace_nbytes=15)),
                  "carry not 8-byte aligned": dict(rec=changed(dev_carry=good.dev_carry + 4)), "NULL dev_carry": dict(rec=changed(dev_carry=None)),
                  "NULL dev_carry_return": dict(rec=changed(dev_carry_return=None)), "NULL dev_workspace": dict(rec=changed(dev_workspace=None)),
                  "a block smaller than block_nbytes": dict(nbytes=nb.value - 1), "K * tiles above the bound": dict(K=N.EPISODE_LOG_MAX_CELLS // 2 + 1,
                                                                                                                  rows=N.EPISODE_LOG_MAX_CELLS)}
    only_merge = {"n_blocks 0": dict(n_blocks=0), "n_blocks 65": dict(n_blocks=N.DP_MAX_SHARDS + 1), "n_blocks < 0": dict(n_blocks=-1)}
    for what, kw in list(both.items()) + list(only_shard.items()):
        assert shard(**kw) == -1, what
        if kw.get("handle", h) is not None:
            assert b"ssg_job_episode_log_shard" in L.ssg_last_error(h), what
    for what, kw in list(both.items()) + list(only_merge.items()):
        assert merge(**kw) == -1, what
        if kw.get("handle", h) is not None:
            assert b"ssg_job_episode_log_merge_blocks" in L.ssg_last_error(h), what
    torch.cuda.synchronize()
    assert not log.head.any() and bool((log.ring == FILL).all()) and not log.carry.any() and not log.carry_return.any() and bool((block == 0xEE).all())
    assert shard() == 0  # (the calls the refusals were cut from are good ones)
    block[nb.value:2 * nb.value] = block[:nb.value]
    assert merge() == 0
    torch.cuda.synchronize()
    assert log.head.tolist() == [2 * K * n, 2 * K * n] and bool((block[2 * nb.value:] == 0xEE).all())
    cfg = N.default_config()  # an unbound handle is NOT_BOUND, after the arguments
    cfg.n_envs = n
    h2 = C.c_void_p()
    N.check(L.ssg_create(C.byref(cfg), C.byref(h2)))
    assert shard(handle=h2) == -3 and shard(handle=h2, K=0) == -1 and merge(handle=h2) == -3 and merge(handle=h2, n_blocks=0) == -1
    L.ssg_destroy(h2)


def test_a_checkpoint_in_the_middle_of_a_replayed_run_continues_bit_for_bit(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.episode_log import EpisodeLog
    n, W, K, cap = 129, 2, 5, 83
    ranges = shard_ranges(n, W)
    envs = [vec(hi - lo, 7, base=lo) for lo, hi in ranges]
    calls = [inputs(K, n, p, 40 + i) for i, p in enumerate(("p0.3", "p1", "p0.3"))]
    logs, again = [[_job_log(env, cap, K, W, n) for env in envs] for _ in range(2)]
    _replay(torch, logs, ranges, calls[0])
    states = [log.state_dict() for log in logs]
    assert states[0]["job_world"] == 2 and states[0]["job_total_envs"] == n and states[1]["job_env_base"] == 65
    assert torch.equal(states[0]["ring"], states[1]["ring"]) and not torch.equal(states[0]["carry"][:64], states[1]["carry"])
    for x in calls[1:]:
        _replay(torch, logs, ranges, x)
    for log, sd in zip(again, states):
        log.load_state_dict(sd)
    for x in calls[1:]:
        _replay(torch, again, ranges, x)
    for a, b in zip(logs, again):
        for name in ("ring", "head", "carry_return", "carry"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert a.steps == b.steps == 3 * K
    # a mismatch raises and changes nothing
    before = again[0].state_dict()
    for spoil in (dict(job_world=3), dict(job_total_envs=n + 1), dict(job_rows=K + 1), dict(capacity=cap + 1), dict(job_env_base=7)):
        with pytest.raises(ValueError, match=list(spoil)[0]):
            again[0].load_state_dict(dict(states[0], **spoil))
    with pytest.raises(ValueError, match="job_world"):
        again[0].load_state_dict({k: v for k, v in states[0].items() if k != "job_world"})
    with pytest.raises(ValueError, match="job log"):
        EpisodeLog(envs[0], capacity=cap).load_state_dict(states[0])
    with pytest.raises(ValueError, match="num_envs"):
        again[0].load_state_dict(states[1])  # the other shard's carries
    after = again[0].state_dict()
    assert all(torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k] for k in before)
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# two ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_hold_the_same_ring_and_replay(torch_cuda, handles, tmp_path):
    torch = torch_cuda
    import episode_log_job_worker as Wk
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "episode_log_job_worker.py"), str(r), "2", str(port), str(tmp_path)])
             for r in range(2)]
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=300))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert rcs == [0, 0], rcs
    rk = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=True) for r in range(2)]
    want_backend = "nccl" if torch.cuda.device_count() >= 2 else "gloo"
    n, steps = Wk.JOB_ENVS, sum(c[0] for c in Wk.CALLS)
    assert all((k["backend"], k["world"], k["total_envs"], k["steps"]) == (want_backend, 2, n, steps) for k in rk)
    assert torch.equal(rk[0]["ring"], rk[1]["ring"]) and torch.equal(rk[0]["head"], rk[1]["head"])
    assert not torch.equal(rk[0]["blocks"], rk[1]["blocks"])  # (the shards saw different envs)
    # the single log over all envs, in numpy; and the replay in this process: the ranks' saved blocks stacked and merged
    one = Single(n, Wk.CAPACITY)
    log = _job_log(handles(1), Wk.CAPACITY, Wk.ROWS, 2, n)
    assert log.stage == rk[0]["stage"]
    for i, (K, pattern, seed) in enumerate(Wk.CALLS):
        one.append(*inputs(K, n, pattern, seed))
        log.merge_blocks(torch.stack([rk[0]["blocks"][i], rk[1]["blocks"][i]]).to(DEV), K=K, step0=log.steps)
    assert rk[0]["ring"].numpy().tobytes() == one.ring.tobytes() and rk[0]["head"].numpy().tolist() == one.head.tolist()
    assert int(one.head[0]) > Wk.CAPACITY  # (the ring wrapped)
    assert torch.equal(log.ring.cpu(), rk[0]["ring"]) and torch.equal(log.head.cpu(), rk[0]["head"])
    assert torch.cat([rk[0]["carry_return"], rk[1]["carry_return"]]).numpy().tobytes() == one.cret.tobytes()
    assert torch.cat([rk[0]["carry"], rk[1]["carry"]]).numpy().tobytes() == one.c.tobytes()


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
# hidden 16, 4 beams and a step limit of 11, as tests/test_episode_log_cli_gpu.py: every env ends an episode in every update
TRAIN = dict(envs=256, horizon=8, mode="native", update="native", seed=4, hidden=16, env_kw={"n_beams": 4})


@pytest.fixture
def short_episodes():
    from ship_sim_gym_amd.config import EnvConfig
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(EnvConfig, "MAX_STEPS", 11)
        yield


def _columns_but_t(EL, path):
    cols = EL.read_monitor(path)[1]
    return {k: v for k, v in cols.items() if k != "t"}


def test_trainer_on_one_rank_writes_the_episode_logs_file_and_resumes(tmp_path, torch_cuda, short_episodes):
    """One rank: --job-episode-log's file is --episode-log's in every column but t; a saved-and-resumed run leaves the uninterrupted
    run's file."""
    from ship_sim_gym_amd import episode_log as EL
    single = load_script("train/ppo_torch.py")
    job, own, cut, ckpt, lines = tmp_path / "job.csv", tmp_path / "own.csv", tmp_path / "cut.csv", tmp_path / "run.ckpt", []
    single.train(updates=3, log=lines.append, job_episode_log=str(job), job_best_window=20, episode_log_capacity=4096, **TRAIN)
    single.train(updates=3, log=lambda *a: None, episode_log=str(own), best_window=20, episode_log_capacity=4096, **TRAIN)
    a, b = _columns_but_t(EL, job), _columns_but_t(EL, own)
    assert len(a["r"]) >= 2 * 256 and set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert sum("episode log:" in ln and "rows written" in ln for ln in lines) == 3
    kw = dict(TRAIN, log=lambda *a: None, job_episode_log=str(cut), episode_log_capacity=4096)
    single.train(updates=2, save=str(ckpt), **kw)
    single.train(updates=3, **kw)  # (the run goes on past its checkpoint, from a fresh start: the file is written anew)
    single.train(updates=3, resume=str(ckpt), **kw)
    c = _columns_but_t(EL, cut)
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    with pytest.raises(ValueError, match="not supported together"):
        single.train(updates=1, log=None, job_episode_log=str(job), episode_log=str(own), **TRAIN)


def test_trainer_on_two_ranks_writes_the_jobs_file(tmp_path, torch_cuda):
    from ship_sim_gym_amd import episode_log as EL
    path = os.path.join(str(tmp_path), "job.csv")
    env = dict(os.environ, SSG_TRAIN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--gpus", "2", "--envs", "256", "--horizon", "64",
                        "--updates", "3", "--mode", "native", "--update", "native", "--perm", "native", "--job-episode-log", path,
                        "--job-best-window", "50", "--episode-log-capacity", "4096"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    cols = EL.read_monitor(path)[1]
    assert len(cols["r"]) > 0
    key = list(zip(cols["timesteps"].tolist(), cols["env"].tolist()))
    assert key == sorted(key) and len(set(key)) == len(key)                          # (timesteps, env) ascending: the single log's order
    assert cols["env"].min() < 128 <= cols["env"].max() and cols["env"].max() < 256  # both shards' envs
    assert (cols["timesteps"] % 256 == 0).all() and cols["timesteps"].max() <= 3 * 64 * 256  # the job's envs count, not a shard's
    assert "episode log:" in r.stdout and "mean return of the last 50 at most" in r.stdout
