"""CPU-side checks of per-member batch sizes (unequal env slices): ssg_pop_pack_slices, ssg_pop_set_slices / ssg_pop_get_slices,
ssg_pop_pack_schedule_samples, population.slices_for_batch_sizes, the train_batch_size mutation and train/pbt_native.py's flags.  The
schedule table is checked against a Python restatement built on ppo.chunk_split, member by member with the member's OWN sample count."""
import ctypes as C
import os
import random
import struct
from fractions import Fraction

import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------------------
# ssg_pop_pack_slices, ssg_pop_set_slices, ssg_pop_get_slices
# ------------------------------------------------------------------------------------------------------------------------------------
def _pack_slices(native, sizes, short=0):
    P = len(sizes)
    arr = (C.c_int32 * max(P, 1))(*sizes)
    n = native.POP_SLICE_ROW * P
    buf = (C.c_int32 * max(n, 1))(*([-7] * max(n, 1)))
    return native.lib().ssg_pop_pack_slices(P, arr, buf, n - short), list(buf)[:n]


@pytest.mark.parametrize("sizes", [(1, 63, 64, 257), (5,), (256, 257, 1, 512, 513), (70, 70, 70), tuple([1] * 256)])
def test_slices_table_rows_are_prefix_offsets_sizes_and_gae_blocks(native, sizes):
    assert native.POP_SLICE_ROW == 4
    rc, table = _pack_slices(native, sizes)
    assert rc == 0
    o = 0
    for m, n_m in enumerate(sizes):
        assert table[4 * m: 4 * m + 4] == [o, n_m, (n_m + 255) // 256, 0], m
        o += n_m


def test_pack_slices_refusals(native):
    L = native.lib()
    assert _pack_slices(native, (3, 0, 4))[0] == -1                         # an entry < 1
    assert _pack_slices(native, (3, -2, 4))[0] == -1
    assert _pack_slices(native, (2 ** 30, 2 ** 30))[0] == -1                # the sum passes 2^31 - 1
    assert _pack_slices(native, (2 ** 30, 2 ** 30 - 1))[0] == 0             # ... and exactly 2^31 - 1 does not
    assert _pack_slices(native, (4, 4), short=1)[0] == -1                   # a short buffer
    assert _pack_slices(native, [1] * 257)[0] == -1                         # P out of range
    arr, buf = (C.c_int32 * 2)(4, 4), (C.c_int32 * 8)()
    assert L.ssg_pop_pack_slices(0, arr, buf, 8) == -1
    assert L.ssg_pop_pack_slices(2, None, buf, 8) == -1 and L.ssg_pop_pack_slices(2, arr, None, 8) == -1
    assert b"ssg_pop_pack_slices" in L.ssg_last_error(None)


def test_set_slices_binds_to_the_handle_and_refuses_what_does_not_fit(native):
    L = native.lib()
    c = native.default_config()
    c.n_envs = 385
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    P, out = C.c_int(-1), (C.c_int32 * 8)()
    native.check(L.ssg_pop_get_slices(h, C.byref(P), None), h)
    assert P.value == 0                                                      # nothing bound on a fresh handle
    table = C.c_void_p(0x1000)                                               # (the handle only keeps the pointer)
    sizes = (C.c_int32 * 4)(1, 63, 64, 257)
    native.check(L.ssg_pop_set_slices(h, 4, sizes, table), h)
    native.check(L.ssg_pop_get_slices(h, C.byref(P), out), h)
    assert P.value == 4 and list(out)[:4] == [1, 63, 64, 257]
    sizes[0] = 99                                                            # the handle holds a COPY of the host array
    native.check(L.ssg_pop_get_slices(h, C.byref(P), out), h)
    assert list(out)[:4] == [1, 63, 64, 257]
    for bad in ((1, 63, 64, 256), (1, 63, 64, 258), (0, 64, 64, 257), (-1, 65, 64, 257)):
        assert L.ssg_pop_set_slices(h, 4, (C.c_int32 * 4)(*bad), table) == -1, bad
        assert b"ssg_pop_set_slices" in L.ssg_last_error(h)
        native.check(L.ssg_pop_get_slices(h, C.byref(P), out), h)
        assert P.value == 4 and list(out)[:4] == [1, 63, 64, 257]            # a refused call leaves the binding as it was
    assert L.ssg_pop_set_slices(h, 257, (C.c_int32 * 257)(*([1] * 257)), table) == -1
    assert L.ssg_pop_set_slices(h, -1, (C.c_int32 * 4)(1, 63, 64, 257), table) == -1
    # before a state blob is bound every population entry point still answers NOT_BOUND first, as without slices
    assert L.ssg_pop_episode_stats(h, 4, 1, None, None, None, None, None, None) == -3
    for unbind in ((0, sizes, table), (4, None, table), (4, sizes, None)):
        native.check(L.ssg_pop_set_slices(h, 4, (C.c_int32 * 4)(1, 63, 64, 257), table), h)
        native.check(L.ssg_pop_set_slices(h, *unbind), h)
        native.check(L.ssg_pop_get_slices(h, C.byref(P), None), h)
        assert P.value == 0, unbind
    assert L.ssg_pop_get_slices(None, C.byref(P), None) == -1 and L.ssg_pop_get_slices(h, None, None) == -1
    assert L.ssg_pop_set_slices(None, 4, sizes, table) == -1
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# ssg_pop_pack_schedule_samples
# ------------------------------------------------------------------------------------------------------------------------------------
def _restate(samples, epochs, minibatches):
    """(header rows, {(j, m): record}, steps): per member the chunking of ITS samples, as ppo.chunk_split has it; a header row is
    (steps, chunks, C, epochs, prefix of the samples before it); a record (offset, M, G, first, active, 1/(float)M as f32 bits)."""
    from ship_sim_gym_amd.ppo import chunk_split
    hdr, recs, steps, prefix = [], {}, [], 0
    for m, (n, ep, mb) in enumerate(zip(samples, epochs, minibatches)):
        chunk, chunks = chunk_split(n, mb)
        hdr.append((ep * chunks, chunks, chunk, ep, prefix))
        prefix += n
        steps.append(ep * chunks)
        for j in range(ep * chunks):
            e, c = divmod(j, chunks)
            b0 = c * chunk
            M = min(chunk, n - b0)
            inv = struct.unpack("<i", struct.pack("<f", 1.0 / struct.unpack("<f", struct.pack("<f", float(M)))[0]))[0]
            recs[(j, m)] = (e * n + b0, M, min(-(-M // 64), 512), int(c == 0), 1, inv)
    return hdr, recs, steps


def _pack_samples(native, samples, epochs, minibatches, short=0):
    L = native.lib()
    P = len(epochs)
    sm, ep, mb = (C.c_int64 * P)(*samples), (C.c_int32 * P)(*epochs), (C.c_int32 * P)(*minibatches)
    steps, launches = (C.c_int32 * P)(), C.c_int32(-1)
    rc = L.ssg_pop_pack_schedule_samples(P, sm, ep, mb, None, 0, steps, C.byref(launches))
    if rc:
        return rc, [], [], -1
    ints = native.pop_sched_ints(P, launches.value)
    buf = (C.c_int32 * ints)(*([-7] * ints))
    rc = L.ssg_pop_pack_schedule_samples(P, sm, ep, mb, buf, ints - short, steps, C.byref(launches))
    return rc, list(buf), list(steps), launches.value


def _i64(lo, hi):
    return struct.unpack("<q", struct.pack("<ii", lo, hi))[0]


SAMPLE_CASES = [
    ((5, 315, 320, 1285), [2, 2, 2, 2], [4, 4, 4, 4]),         # the GPU test's layout (1, 63, 64, 257) x K = 5, common schedule
    ((5, 315, 320, 1285), [1, 2, 3, 1], [1, 4, 5, 16]),        # ... and its per-member one: chunks of 5, 79, 64, 81
    ((64, 65, 32768, 33600), [1, 3, 1, 2], [1, 2, 4, 1]),      # one tile exactly, one sample past it, the full grid, the capped grid
    ((2000, 160000), [30, 1], [16, 10]),                        # the reference's 80-fold spread (pbt.py:42)
    ((7,), [3], [100]),                                         # more minibatches than samples: chunks of one sample
]


@pytest.mark.parametrize("samples,epochs,minibatches", SAMPLE_CASES)
def test_schedule_of_per_member_samples_is_each_members_own_chunking(native, samples, epochs, minibatches):
    from ship_sim_gym_amd.ppo import chunk_split
    P, R = len(samples), native.POP_SCHED_ROW
    rc, table, steps, launches = _pack_samples(native, samples, epochs, minibatches)
    assert rc == 0
    hdr, recs, want_steps = _restate(samples, epochs, minibatches)
    assert steps == want_steps and launches == max(want_steps)
    assert len(table) == P * R * (1 + launches)
    for m in range(P):
        row = table[m * R: (m + 1) * R]
        # C_m, chunks_m from the member's own count; the int64 at [4..5] is the start of its permutation block, in samples
        assert (row[0], row[1], row[2], row[3], _i64(row[4], row[5])) == hdr[m] and row[6:] == [0, 0], (m, row)
        assert (row[2], row[1]) == chunk_split(samples[m], minibatches[m])
        assert _i64(row[4], row[5]) == sum(samples[:m])
    for j in range(launches):
        for m in range(P):
            row = table[((1 + j) * P + m) * R: ((1 + j) * P + m + 1) * R]
            got = (_i64(row[0], row[1]), row[native.SCHED_M], row[native.SCHED_G], row[native.SCHED_FIRST], row[native.SCHED_ACTIVE],
                   row[native.SCHED_INVM])
            if j < steps[m]:
                assert got == recs[(j, m)] and row[7] == 0, (j, m, got)
                assert got[2] == min(-(-got[1] // 64), 512)                             # G = min(ceil(M / 64), 512)
                assert 0 <= got[0] and got[0] + got[1] <= epochs[m] * samples[m]        # inside the member's OWN block
            else:
                assert row == [0] * R, (j, m, row)
    # with perm_epochs rows per member the blocks tile the flat buffer in member order, unpadded
    perm_epochs = max(epochs)
    ends = [perm_epochs * (hdr[m][4] + samples[m]) for m in range(P)]
    assert [perm_epochs * hdr[m][4] for m in range(P)] == [0] + ends[:-1] and ends[-1] == perm_epochs * sum(samples)


@pytest.mark.parametrize("n,epochs,minibatches", [(616, [1, 3, 2], [45, 9, 1]), (800, [2, 1, 3, 2], [4, 1, 5, 3]), (33600, [1, 2, 30], [1, 7, 2048])])
def test_equal_counts_reproduce_pack_schedule_int_for_int(native, n, epochs, minibatches):
    L = native.lib()
    P, R = len(epochs), native.POP_SCHED_ROW
    rc, table, steps, launches = _pack_samples(native, [n] * P, epochs, minibatches)
    assert rc == 0
    ep, mb = (C.c_int32 * P)(*epochs), (C.c_int32 * P)(*minibatches)
    steps0, launches0 = (C.c_int32 * P)(), C.c_int32()
    buf = (C.c_int32 * len(table))()
    native.check(L.ssg_pop_pack_schedule(P, n, ep, mb, buf, len(table), steps0, C.byref(launches0)), None)
    assert steps == list(steps0) and launches == launches0.value
    assert table[P * R:] == list(buf)[P * R:]                                # every record of every launch
    for m in range(P):                                                       # the header rows but for the permutation offsets
        assert table[m * R: m * R + 4] == list(buf)[m * R: m * R + 4] and _i64(table[m * R + 4], table[m * R + 5]) == m * n


def test_pack_schedule_samples_refusals(native):
    L = native.lib()
    assert _pack_samples(native, (5, 0), [1, 1], [1, 1])[0] == -1            # a member without samples
    assert _pack_samples(native, (5, 5), [1, 0], [1, 1])[0] == -1            # epochs < 1
    assert _pack_samples(native, (5, 5), [1, 1], [0, 1])[0] == -1            # minibatches < 1
    assert _pack_samples(native, (5, 5), [1, 1], [1, 1], short=1)[0] == -1   # a short buffer
    assert _pack_samples(native, [5] * 257, [1] * 257, [1] * 257)[0] == -1   # P out of range
    sm, ep, n = (C.c_int64 * 2)(5, 5), (C.c_int32 * 2)(1, 1), C.c_int32()
    assert L.ssg_pop_pack_schedule_samples(2, None, ep, ep, None, 0, None, C.byref(n)) == -1
    assert L.ssg_pop_pack_schedule_samples(2, sm, None, ep, None, 0, None, C.byref(n)) == -1
    assert L.ssg_pop_pack_schedule_samples(2, sm, ep, ep, None, 0, None, None) == -1
    assert b"ssg_pop_pack_schedule_samples" in L.ssg_last_error(None)


# ------------------------------------------------------------------------------------------------------------------------------------
# slices_for_batch_sizes
# ------------------------------------------------------------------------------------------------------------------------------------
def _apportion_cases():
    rng = random.Random(11)
    cases = [([1, 2, 4, 8] * 4, 16 * 4096, 64), ([10000, 20000, 40000, 10000], 256, 16), ([1, 1, 1], 192, 64), ([2000, 160000], 81 * 64, 64),
             ([1.5, 2.5, 0.25], 4096, 1), ([7] * 5, 5 * 64, 64)]
    for _ in range(40):
        P = rng.randint(1, 24)
        q = rng.choice([1, 16, 64])
        cases.append(([rng.randint(2000, 160000) for _ in range(P)], q * rng.randint(P, 40 * P), q))
    return cases


@pytest.mark.parametrize("batch,n_envs,quantum", _apportion_cases())
def test_slices_for_batch_sizes_is_a_largest_remainder_apportionment(batch, n_envs, quantum):
    from ship_sim_gym_amd.population import slices_for_batch_sizes
    sizes = slices_for_batch_sizes(batch, n_envs, quantum)
    P = len(batch)
    assert len(sizes) == P and all(isinstance(s, int) for s in sizes) and sum(sizes) == n_envs
    assert all(s % quantum == 0 and s >= quantum for s in sizes)              # whole quanta, and one each at the least
    assert sizes == slices_for_batch_sizes(list(batch), n_envs, quantum)     # deterministic
    # what largest remainder guarantees, exactly: of the quanta left after everyone's first, no member is a whole quantum or more
    # away from its exact proportional share (Fractions: no rounding in the bound)
    rest, total = n_envs // quantum - P, sum(Fraction(b) for b in batch)
    for m in range(P):
        share = rest * Fraction(batch[m]) / total
        assert abs(Fraction(sizes[m], quantum) - 1 - share) < 1, (m, sizes[m], float(share))
    # ties go to the lower index; equal batch sizes differ by one quantum at the most, the larger ones first
    for a in range(P):
        for b in range(a + 1, P):
            if batch[a] == batch[b]:
                assert sizes[a] - sizes[b] in (0, quantum), (a, b)
            if batch[a] > batch[b]:
                assert sizes[a] >= sizes[b]
    # shares, not absolute counts
    assert sizes == slices_for_batch_sizes([3 * b for b in batch], n_envs, quantum)


def test_slices_for_batch_sizes_refusals():
    from ship_sim_gym_amd.population import slices_for_batch_sizes
    for batch, n_envs, quantum in (([1, 2], 100, 64), ([1, 2, 3], 128, 64), ([], 128, 64), ([1, 0], 128, 64), ([1, -2], 128, 64),
                                   ([1, float("nan")], 128, 64), ([1, float("inf")], 128, 64), ([1, 2], 128, 0), ([1, 2], 0, 64)):
        with pytest.raises(ValueError):
            slices_for_batch_sizes(batch, n_envs, quantum)
    assert slices_for_batch_sizes([1, 2], 128, 64) == [64, 64]               # exactly one quantum each: nothing left to deal
    assert slices_for_batch_sizes([1, 1, 1, 1], 320, 64) == [128, 64, 64, 64]  # a tie: the lower index


def test_reference_mutations_carry_train_batch_size_on_request():
    from ship_sim_gym_amd.population import PBTScheduler, reference_mutations
    assert "train_batch_size" not in reference_mutations() and "train_batch_size" not in reference_mutations(schedule=True)
    mut = reference_mutations(schedule=True, batch=True)
    assert list(mut) == ["lambda", "clip_param", "lr", "num_sgd_iter", "sgd_minibatch_size", "train_batch_size"]   # pbt.py:36-42
    assert list(reference_mutations(batch=True)) == ["lambda", "clip_param", "lr", "train_batch_size"]
    rng = random.Random(3)
    draws = [mut["train_batch_size"](rng) for _ in range(2000)]
    assert all(isinstance(d, int) and 2000 <= d <= 160000 for d in draws) and min(draws) < 4000 and max(draws) > 150000
    # the value travels with an exploit and is explored as an int
    s = PBTScheduler(4, seed=1, mutations=reference_mutations(batch=True))
    hp = {"lambda": [0.95] * 4, "clip_param": [0.2] * 4, "lr": [5e-4] * 4, "train_batch_size": [10000, 20000, 40000, 10000]}
    src, new, events = s.perturb([0.0, 1.0, 2.0, 3.0], hp)
    assert src == [3, 1, 2, 3] and new["train_batch_size"][1:] == hp["train_batch_size"][1:]
    (key, kind, old, val), = [e for e in events[0]["mutations"] if e[0] == "train_batch_size"]
    assert old == 10000 and isinstance(val, int) and (val in (12000, 8000) if kind == "perturb" else 2000 <= val <= 160000)


# ------------------------------------------------------------------------------------------------------------------------------------
# train/pbt_native.py
# ------------------------------------------------------------------------------------------------------------------------------------
def test_pbt_trainer_parses_the_batch_flags():
    mod = load_script("train/pbt_native.py")
    a = mod.parse_args([])
    assert (a.mutate_batch, a.batch_shares, a.envs, a.quantum) == (False, None, None, None)
    a = mod.parse_args(["--members", "4", "--envs", "256", "--mutate-batch", "--mutate-schedule"])
    assert (a.members, a.envs, a.envs_per_member, a.mutate_batch, a.mutate_schedule) == (4, 256, 64, True, True)
    a = mod.parse_args(["--batch-shares", "1,2,4", "--no-pbt", "--quantum", "32"])
    assert a.members == 3 and a.batch_shares == [1.0, 2.0, 4.0] and a.pbt is False and a.quantum == 32
    for bad in (["--batch-shares", "1,x"], ["--batch-shares", "1,0"], ["--batch-shares", "1,2", "--mutate-batch"],
                ["--lrs", "1e-3,1e-4", "--batch-shares", "1,2,4"], ["--members", "4", "--envs", "3", "--mutate-batch"],
                ["--members", "4", "--envs", "258"], ["--quantum", "0"]):
        with pytest.raises((SystemExit, ValueError)):
            mod.parse_args(bad)
    assert mod.INITIAL_BATCH == [10000, 20000, 40000]                        # train/rllib/pbt.py:69-70
    assert "share" in mod.make_arg_parser().format_help()                    # a batch size is a share of the envs, and says so
    # the default quantum: the policy tile where the handle is large enough, smaller on a small one
    assert mod.default_quantum(16 * 4096, 16) == 64 and mod.default_quantum(256, 4) == 16 and mod.default_quantum(7, 3) == 1


def test_clamp_schedule_uses_the_members_own_samples():
    mod = load_script("train/pbt_native.py")
    from ship_sim_gym_amd.population import slices_for_batch_sizes
    slices = slices_for_batch_sizes([10000, 20000, 40000, 10000], 256, 16)   # 48, 64, 112, 32 envs
    assert slices == [48, 64, 112, 32]
    samples = [4 * s for s in slices]                                        # horizon 4: 192, 256, 448, 128 samples
    used = [mod.clamp_schedule(20, 2048, s, 30) for s in samples]
    assert used == [(20, 192), (20, 256), (20, 448), (20, 128)]              # each clamped to ITS samples, not to the widest member's
    assert [mod.clamp_schedule(40, 100, s, 30) for s in samples] == [(30, 128)] * 4
    assert mod.clamp_schedule(0, 1, 64, 30) == (1, 64)                       # fewer samples than the floor of 128
