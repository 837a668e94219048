"""Host checks of the job-wide episode log's protocol (ship_sim_gym_amd/episode_log.py: shard_block_reference, merge_blocks_reference):
the composed references — a [K, N] batch cut into W contiguous shards by shard_range, one block per shard, the blocks merged — leave,
byte for byte, the ring, the head and the concatenated carries that episode_log_reference leaves on the whole batch.

Cases: W in (1, 2, 3, 8) with unequal shards, some of 1, 63, 64, 65 and 257 envs (episode_log_job_support.JOBS); K in (1, 5, 9);
tests/test_episode_log_gpu.py's done patterns; the capacities 1, count - 1, count, count + 1 and a prime below count, where count is what
the two calls of a case end together.  test_the_cases_cover_the_protocol asserts, on the numpy side, that these inputs contain what the
protocol has to get right."""
import numpy as np
import pytest

from episode_log_job_support import JOBS, PATTERNS, Job, Single, capacities, inputs, shard_ranges, shard_sizes

KS = (1, 5, 9)
CASES = [(W, n, K) for W, n in JOBS for K in KS]


def _seed(W, n, K, pi):
    return 100000 * W + 100 * n + 10 * K + pi


def _rows(K, pi):
    return K + (pi % 3)  # (rows at and above K: lb's tail past K and its padding are part of the block)


def _two_calls(W, n, K, pi):
    return inputs(K, n, PATTERNS[pi], _seed(W, n, K, pi)), inputs(K, n, PATTERNS[pi], _seed(W, n, K, pi) + 5)


def test_the_jobs_have_the_shard_sizes_the_kernels_branch_on():
    sizes = set()
    for W, n in JOBS:
        s = shard_sizes(n, W)
        assert sum(s) == n and len(s) == W and (W == 1 or len(set(s)) > 1), (W, n, s)  # unequal shards
        sizes.update(s)
    assert {1, 63, 64, 65, 257} <= sizes and {W for W, _ in JOBS} == {1, 2, 3, 8}


@pytest.mark.parametrize("W,n,K", CASES, ids=["W%d-n%d-K%d" % c for c in CASES])
def test_the_composed_references_are_the_single_log_byte_for_byte(W, n, K):
    for pi, pattern in enumerate(PATTERNS):
        a, b = _two_calls(W, n, K, pi)
        count = int(np.count_nonzero(a[1]) + np.count_nonzero(b[1]))
        for cap in capacities(count):
            job, one = Job(n, W, cap, _rows(K, pi), env_base=7), Single(n, cap, env_base=7)
            job.append(*a).same_as(one.append(*a), (pattern, cap, "first call"))
            job.append(*b).same_as(one.append(*b), (pattern, cap, "second call"))  # the carries in flight, the head where it was left
            assert int(job.head[0]) == count and int(job.head[1]) == int(np.count_nonzero(b[1]))


def test_the_cases_cover_the_protocol():
    """The inputs above contain: a row with episodes on at least two shards; a shard with none; a shard with count_r > S; total >
    capacity; a head that wraps the ring."""
    from ship_sim_gym_amd.episode_log import job_stage
    seen = dict.fromkeys(("row_on_two_shards", "empty_shard", "shard_beyond_stage", "total_beyond_capacity", "head_wraps"), 0)
    for W, n, K in CASES:
        for pi in range(len(PATTERNS)):
            a, b = _two_calls(W, n, K, pi)
            count = int(np.count_nonzero(a[1]) + np.count_nonzero(b[1]))
            for cap in capacities(count):
                S, head = job_stage(cap, _rows(K, pi), n, W), 0
                for _, done, _ in (a, b):
                    per = np.stack([np.count_nonzero(done[:, lo:hi], axis=1) for lo, hi in shard_ranges(n, W)])  # [W, K]
                    total = int(per.sum())
                    seen["row_on_two_shards"] += int(np.any(np.count_nonzero(per, axis=0) >= 2))
                    seen["empty_shard"] += int(total > 0 and np.any(per.sum(axis=1) == 0))
                    seen["shard_beyond_stage"] += int(np.any(per.sum(axis=1) > S))
                    seen["total_beyond_capacity"] += int(total > cap)
                    seen["head_wraps"] += int(total > 0 and head % cap + min(total, cap) > cap)
                    head += total
    assert all(v > 0 for v in seen.values()), seen


SPLITS = [(3, 191, 5, 9), (8, 517, 1, 5), (2, 127, 9, 1), (1, 65, 5, 5)]


@pytest.mark.parametrize("W,n,K1,K2", SPLITS, ids=["W%d-n%d-%d+%d" % s for s in SPLITS])
def test_two_calls_leave_what_one_call_leaves(W, n, K1, K2):
    """K1 rows and then K2 rows through the shards against ONE single-log call over the K1 + K2 rows: ring, head[0] and carries (head[1]
    is the last call's own count)."""
    for pi, pattern in enumerate(PATTERNS):
        a = inputs(K1 + K2, n, pattern, _seed(W, n, K1 + K2, pi) + 1)
        count = int(np.count_nonzero(a[1]))
        for cap in capacities(count):
            job, one = Job(n, W, cap, max(K1, K2)), Single(n, cap)
            job.append(*(x[:K1] for x in a)).append(*(x[K1:] for x in a))
            job.same_as(one.append(*a), (pattern, cap), head1=False)
            assert int(job.head[1]) == int(np.count_nonzero(a[1][K1:]))


def test_a_block_is_what_the_header_says():
    """The layout: a 32-byte header (count, step0, K, S), lb[t] = the episodes of rows before t with zeros past K and in the padding to
    16 bytes, local rank q in slot q % S, the last S ranks only; and block_nbytes = 32 + 16 ceil((rows + 1) / 4) + 32 S."""
    from ship_sim_gym_amd.episode_log import (RECORD_DTYPE, block_layout, block_owned_slots, block_views, episode_log_reference,
                                              shard_block_reference)
    rew, done, flags = inputs(5, 65, "p0.3", 11)
    count = int(np.count_nonzero(done))
    for rows, S in ((5, count + 3), (6, count), (9, 7)):
        lb_n, rec_off, nbytes = block_layout(rows, S)
        assert lb_n % 4 == 0 and lb_n >= rows + 1 and rec_off == 32 + 4 * lb_n and nbytes == rec_off + 32 * S and nbytes % 16 == 0
        block, cret, c = shard_block_reference(rew, done, flags, np.zeros(65), np.zeros((65, 2), dtype=np.int32), rows, S, step0=40, env_base=100)
        hdr, lb, slots = block_views(block, rows, S)
        assert (int(hdr["count"][0]), int(hdr["step0"][0]), int(hdr["K"][0]), int(hdr["stage"][0]), int(hdr["reserved"][0])) == (count, 40, 5, S, 0)
        assert lb[:6].tolist() == [0] + np.cumsum(np.count_nonzero(done, axis=1)).tolist() and not lb[6:].any()
        full = episode_log_reference(rew, done, flags, np.zeros(65), np.zeros((65, 2), dtype=np.int32), np.zeros(2, dtype=np.int64),
                                     np.zeros(count, dtype=RECORD_DTYPE), step0=40, env_base=100)
        owned = block_owned_slots(count, S)
        assert len(owned) == min(count, S)
        for q in range(max(0, count - S), count):
            assert slots[q % S] == full[0][q]
        assert cret.tobytes() == full[2].tobytes() and c.tobytes() == full[3].tobytes()


def test_the_merge_skips_what_is_malformed():
    """A record whose step lies outside the call, and an lb that overruns the count, are skipped; nothing else changes."""
    from ship_sim_gym_amd.episode_log import block_views, merge_blocks_reference
    n, W, K, cap = 127, 2, 5, 4096
    a = inputs(K, n, "p0.3", 3)
    job = Job(n, W, cap, K).append(*a)
    good_ring, good_head = job.ring.copy(), job.head.copy()
    blocks = job.blocks.copy()
    lb0 = block_views(blocks[0], K, job.stage)[1]
    hdr, lb, slots = block_views(blocks[1], K, job.stage)
    assert int(hdr["count"][0]) >= 2 and int(hdr["count"][0]) <= job.stage  # (slot q holds local rank q)
    ranks = [q + int(lb0[int(slots["step"][q]) + 1]) for q in (0, 1)]      # R of block 1's local ranks 0 and 1, by the formula
    slots["step"][0] = K + 3      # past the call
    slots["step"][1] = -1         # before it
    ring, head = merge_blocks_reference(blocks, np.zeros(cap, dtype=good_ring.dtype), np.zeros(2, dtype=np.int64), K, 0, K, job.stage)
    want = np.zeros(cap, dtype=good_ring.dtype)
    want[:int(good_head[0])] = good_ring[:int(good_head[0])]
    want[ranks] = np.zeros(1, dtype=good_ring.dtype)[0]  # the two stay what the ring held
    assert ring.tobytes() == want.tobytes() and head.tolist() == good_head.tolist()
    # an lb that claims more episodes than the shard has: every rank it pushes outside [0, total) is dropped, the head takes lb's total
    blocks = job.blocks.copy()
    hdr, lb, slots = block_views(blocks[0], K, job.stage)
    lb[1:K + 1] += 1000
    ring, head = merge_blocks_reference(blocks, np.zeros(cap, dtype=good_ring.dtype), np.zeros(2, dtype=np.int64), K, 0, K, job.stage)
    assert int(head[0]) == int(good_head[0]) + 1000 and int(head[1]) == int(head[0])
