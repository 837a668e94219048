"""CPU-side checks of per-member update schedules (ssg_pop_pack_schedule, ssg_pop_pack_hparams_steps, the scheduler's schedule
mutations, train/pbt_native.py's flags).  The schedule table is checked against a Python restatement built on ppo.chunk_split — the
chunking NativePPO.update documents — so a record here is exactly the minibatch the single-policy loop would run at that step."""
import ctypes as C
import os
import struct
import sys

import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restate(n, epochs, minibatches):
    """(header rows, {(j, m): record}, steps, launches): the table as the issue words it.  A record is (offset, M, G, first, active,
    1/(float)M as f32 bits)."""
    from ship_sim_gym_amd.ppo import chunk_split
    hdr, recs, steps = [], {}, []
    for m, (ep, mb) in enumerate(zip(epochs, minibatches)):
        chunk, chunks = chunk_split(n, mb)
        hdr.append((ep * chunks, chunks, chunk, ep))
        steps.append(ep * chunks)
        for j in range(ep * chunks):
            e, c = divmod(j, chunks)
            b0 = c * chunk
            M = min(chunk, n - b0)
            inv = struct.unpack("<i", struct.pack("<f", 1.0 / struct.unpack("<f", struct.pack("<f", float(M)))[0]))[0]
            recs[(j, m)] = (e * n + b0, M, min(-(-M // 64), 512), int(c == 0), 1, inv)
    return hdr, recs, steps, max(steps)


def _pack(native, n, epochs, minibatches, short=0):
    L = native.lib()
    P = len(epochs)
    ep, mb = (C.c_int32 * P)(*epochs), (C.c_int32 * P)(*minibatches)
    steps, launches = (C.c_int32 * P)(), C.c_int32(-1)
    native.check(L.ssg_pop_pack_schedule(P, n, ep, mb, None, 0, steps, C.byref(launches)), None, "size query")
    ints = native.pop_sched_ints(P, launches.value)
    buf = (C.c_int32 * ints)(*([-7] * ints))
    rc = L.ssg_pop_pack_schedule(P, n, ep, mb, buf, ints - short, steps, C.byref(launches))
    return rc, list(buf), list(steps), launches.value


CASES = [
    (616, [1, 3, 2], [45, 9, 1]),                       # 44 x 14, 9 x 69 (last 64), 1 x 616: the GPU test's schedule
    (616, [2, 1, 1, 1], [616, 617, 5000, 1]),           # chunks of ONE sample; more minibatches than samples allow
    (800, [2, 1, 3, 2], [4, 1, 5, 3]),                  # 800 / 3: chunks of 267, 267, 266
    (10000, [1, 4, 2, 3, 1], [4, 6, 1, 157, 10000]),    # 6 x 1667 (last 1665); 157 x 64 (last 16): M = one tile exactly
    (33600, [1, 2, 30], [1, 7, 2048]),                  # 525 tiles on the capped grid of 512 next to 75-tile chunks; chunks of 17
]


@pytest.mark.parametrize("n,epochs,minibatches", CASES)
def test_schedule_table_is_the_chunking_restated(native, n, epochs, minibatches):
    P = len(epochs)
    rc, table, steps, launches = _pack(native, n, epochs, minibatches)
    assert rc == 0
    hdr, recs, want_steps, want_launches = _restate(n, epochs, minibatches)
    assert steps == want_steps and launches == want_launches == max(steps)
    R = native.POP_SCHED_ROW
    assert len(table) == P * R * (1 + launches)
    for m in range(P):
        assert tuple(table[m * R: m * R + 4]) == hdr[m] and table[m * R + 4: (m + 1) * R] == [0] * 4, m
    seen_idle = False
    for j in range(launches):
        for m in range(P):
            row = table[((1 + j) * P + m) * R: ((1 + j) * P + m + 1) * R]
            off = struct.unpack("<q", struct.pack("<ii", row[0], row[1]))[0]
            got = (off, row[native.SCHED_M], row[native.SCHED_G], row[native.SCHED_FIRST], row[native.SCHED_ACTIVE], row[native.SCHED_INVM])
            if j < steps[m]:
                assert got == recs[(j, m)] and row[7] == 0, (j, m, got, recs[(j, m)])
                assert 0 <= off and off + got[1] <= epochs[m] * n               # the minibatch lies inside the member's own rows
            else:
                assert row == [0] * R, (j, m, row)                              # idle: G = 0, inactive
                seen_idle = True
    assert seen_idle == (len(set(steps)) > 1)
    # every sample of every epoch of every member is in exactly one minibatch
    for m in range(P):
        covered = sorted((recs[(j, m)][0], recs[(j, m)][0] + recs[(j, m)][1]) for j in range(steps[m]))
        assert covered[0][0] == 0 and covered[-1][1] == epochs[m] * n and all(a[1] == b[0] for a, b in zip(covered, covered[1:]))


def test_schedule_cases_cover_the_grid_and_the_chunking_edges():
    from ship_sim_gym_amd.ppo import chunk_split
    assert chunk_split(616, 45) == (14, 44) and chunk_split(616, 9) == (69, 9) and chunk_split(616, 5000) == (1, 616)
    assert chunk_split(33600, 1) == (33600, 1) and -(-33600 // 64) == 525 > 512 and chunk_split(33600, 7) == (4800, 7) and 4800 // 64 == 75
    assert chunk_split(10000, 157) == (64, 157) and chunk_split(800, 3) == (267, 3)


def test_schedule_size_query_and_refusals(native):
    L = native.lib()
    rc, table, steps, launches = _pack(native, 616, [1, 3, 2], [45, 9, 1], short=1)
    assert rc == -1 and b"SSG_POP_SCHED_INTS" in L.ssg_last_error(None)
    assert table == [-7] * len(table)                                           # refused: nothing written
    assert (steps, launches) == ([44, 27, 2], 44)                               # (the size query had answered)
    ep, mb, n_l = (C.c_int32 * 2)(1, 2), (C.c_int32 * 2)(3, 4), C.c_int32()
    buf = (C.c_int32 * 1024)()
    assert L.ssg_pop_pack_schedule(2, 100, ep, mb, buf, 1024, None, C.byref(n_l)) == 0 and n_l.value == 8   # steps_out is optional
    assert L.ssg_pop_pack_schedule(2, 100, None, mb, buf, 1024, None, C.byref(n_l)) == -1
    assert L.ssg_pop_pack_schedule(2, 100, ep, None, buf, 1024, None, C.byref(n_l)) == -1
    assert L.ssg_pop_pack_schedule(2, 100, ep, mb, buf, 1024, None, None) == -1
    assert L.ssg_pop_pack_schedule(0, 100, ep, mb, buf, 1024, None, C.byref(n_l)) == -1
    assert L.ssg_pop_pack_schedule(257, 100, ep, mb, buf, 1024, None, C.byref(n_l)) == -1
    assert L.ssg_pop_pack_schedule(2, 0, ep, mb, buf, 1024, None, C.byref(n_l)) == -1
    for bad_ep, bad_mb in (((0, 2), (3, 4)), ((1, 2), (3, 0)), ((1, -1), (3, 4))):
        assert L.ssg_pop_pack_schedule(2, 100, (C.c_int32 * 2)(*bad_ep), (C.c_int32 * 2)(*bad_mb), buf, 1024, None, C.byref(n_l)) == -1
        assert b"< 1" in L.ssg_last_error(None)


def _hparams(native, P):
    hp = (native.PpoHparams * P)()
    for m in range(P):
        hp[m].struct_size = C.sizeof(native.PpoHparams)
        hp[m].gamma, hp[m].lam, hp[m].clip, hp[m].vf_coef, hp[m].ent_coef = 0.99, 0.9 + 0.02 * m, 0.1 + 0.05 * m, 0.5, 0.01
        hp[m].lr, hp[m].beta1, hp[m].beta2, hp[m].eps, hp[m].adv_eps = 1e-3 / (1 + m), 0.3 if m == 1 else 0.9, 0.999, 1e-8, 1e-8
    return hp


def test_hparams_steps_rows_are_each_members_own_start(native):
    L = native.lib()
    P, n_steps = 4, 6
    hp = _hparams(native, P)
    step0 = [0, 44, 27, 1000003]
    n = native.pop_table_floats(P, n_steps)
    buf = (C.c_float * n)()
    native.check(L.ssg_pop_pack_hparams_steps(P, hp, (C.c_int64 * P)(*step0), n_steps, buf, n), None, "ssg_pop_pack_hparams_steps")
    got = bytes(buf)
    row = 8 * 4                                                                  # bytes per member row
    rows_differ = set()
    for m in range(P):
        ref = (C.c_float * n)()
        native.check(L.ssg_pop_pack_hparams(P, hp, step0[m], n_steps, ref, n), None, "ssg_pop_pack_hparams")
        ref = bytes(ref)
        for j in range(1 + n_steps):                                             # row 0: the loss constants; then the Adam rows
            a = (j * P + m) * row
            assert got[a: a + row] == ref[a: a + row], (m, j)
            other = (C.c_float * n)()
            native.check(L.ssg_pop_pack_hparams(P, hp, step0[(m + 1) % P], n_steps, other, n), None, "ssg_pop_pack_hparams")
            if j and bytes(other)[a: a + row] != got[a: a + row]:
                rows_differ.add(m)
    assert rows_differ == set(range(P))                                          # the starting step matters to every member's rows
    # equal starts: the whole table is ssg_pop_pack_hparams'
    same = (C.c_float * n)()
    native.check(L.ssg_pop_pack_hparams_steps(P, hp, (C.c_int64 * P)(*[17] * P), n_steps, same, n), None, "ssg_pop_pack_hparams_steps")
    ref = (C.c_float * n)()
    native.check(L.ssg_pop_pack_hparams(P, hp, 17, n_steps, ref, n), None, "ssg_pop_pack_hparams")
    assert bytes(same) == bytes(ref)
    assert L.ssg_pop_pack_hparams_steps(P, hp, None, n_steps, buf, n) == -1
    assert L.ssg_pop_pack_hparams_steps(P, hp, (C.c_int64 * P)(0, -1, 0, 0), n_steps, buf, n) == -1
    assert L.ssg_pop_pack_hparams_steps(P, hp, (C.c_int64 * P)(*step0), n_steps, buf, n - 1) == -1
    assert L.ssg_pop_pack_hparams_steps(P, hp, (C.c_int64 * P)(*step0), -1, buf, n) == -1


def test_update_sched_refuses_before_it_needs_a_device(native):
    """No handle, then no bound state: the order of refusals its neighbours keep."""
    L = native.lib()
    assert L.ssg_pop_update_sched(None, None, None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, 0,
                                  None) == -1
    c = native.default_config()
    c.n_envs = 64
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    assert L.ssg_pop_update_sched(h, None, None, None, 0, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, 0,
                                  None) == -3
    assert b"ssg_bind_state" in L.ssg_last_error(h)
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# the scheduler
# ------------------------------------------------------------------------------------------------------------------------------------
def test_default_mutations_are_unchanged_and_schedule_appends_two():
    from ship_sim_gym_amd.population import reference_mutations
    assert list(reference_mutations()) == ["lambda", "clip_param", "lr"]
    assert list(reference_mutations(schedule=False)) == ["lambda", "clip_param", "lr"]
    mut = reference_mutations(schedule=True)
    assert list(mut) == ["lambda", "clip_param", "lr", "num_sgd_iter", "sgd_minibatch_size"]
    import random
    rng = random.Random(0)
    it = [mut["num_sgd_iter"](rng) for _ in range(2000)]
    sz = [mut["sgd_minibatch_size"](rng) for _ in range(2000)]
    assert all(isinstance(v, int) for v in it + sz)
    assert min(it) == 1 and max(it) == 30 and 128 <= min(sz) and max(sz) <= 16384 and max(sz) > 8192    # train/rllib/pbt.py:40-41


def _start(P):
    return {"lambda": [0.95] * P, "clip_param": [0.2] * P, "lr": [5e-4] * P, "num_sgd_iter": [10, 20, 30, 7] * (P // 4),
            "sgd_minibatch_size": [128, 512, 2048, 333] * (P // 4)}


def _scores(P, rounds, seed=1234):
    import random
    rng = random.Random(seed)
    return [[rng.uniform(-5.0, 5.0) for _ in range(P)] for _ in range(rounds)]


def test_scheduler_keeps_ints_ints_with_truncation():
    from ship_sim_gym_amd.population import PBTScheduler, reference_mutations
    P = 16
    sched = PBTScheduler(P, seed=3, mutations=reference_mutations(schedule=True))
    hp = _start(P)
    kinds, truncated = set(), 0
    for scores in _scores(P, 150):
        src, new, events = sched.perturb(scores, hp)
        for e in events:
            assert [k for k, _, _, _ in e["mutations"]] == ["lambda", "clip_param", "lr", "num_sgd_iter", "sgd_minibatch_size"]
            for key, kind, old, val in e["mutations"]:
                assert old == hp[key][e["source"]] and new[key][e["member"]] == val
                if key in ("num_sgd_iter", "sgd_minibatch_size"):
                    kinds.add((key, kind))
                    assert type(old) is int and type(val) is int, (key, kind, old, val)
                    if kind == "perturb":
                        assert val in (int(old * 1.2), int(old * 0.8)), (key, old, val)
                        truncated += val not in (old * 1.2, old * 0.8)
                    elif key == "num_sgd_iter":
                        assert 1 <= val <= 30
                    else:
                        assert 128 <= val <= 16384
                elif key != "lr" and kind == "perturb":
                    assert val in (old * 1.2, old * 0.8) and isinstance(val, float)    # floats are perturbed as before
        hp = new
    assert kinds == {(k, kind) for k in ("num_sgd_iter", "sgd_minibatch_size") for kind in ("resample", "perturb")}
    assert truncated > 50                                                       # the truncation rule was exercised, not only exact products
    assert all(type(v) is int for k in ("num_sgd_iter", "sgd_minibatch_size") for v in hp[k])
    # int(old * 0.8) of 1 is 0: the scheduler does not clamp (the trainer does, before use)
    assert int(1 * 0.8) == 0


def test_schedule_mutations_are_seed_deterministic():
    from ship_sim_gym_amd.population import PBTScheduler, reference_mutations
    P = 8
    a, b, c = (PBTScheduler(P, seed=s, mutations=reference_mutations(schedule=True)) for s in (5, 5, 6))
    ha, hb, hc = _start(P), _start(P), _start(P)
    differs = False
    for scores in _scores(P, 40):
        ra, rb, rc = a.perturb(scores, ha), b.perturb(scores, hb), c.perturb(scores, hc)
        assert ra == rb
        differs = differs or ra[1] != rc[1]
        ha, hb, hc = ra[1], rb[1], rc[1]
    assert differs


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer's arguments
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_parses_schedule_flags_lists_and_clamps(monkeypatch):
    monkeypatch.setitem(sys.modules, "ray", None)
    mod = load_script("train/pbt_native.py")
    a = mod.parse_args([])
    assert (a.epochs, a.minibatches, a.mutate_schedule, a.max_epochs, a.members) == (2, 4, False, 30, 16)    # the defaults stay ints
    a = mod.parse_args(["--epochs", "3", "--minibatches", "8"])
    assert (a.epochs, a.minibatches) == (3, 8)
    a = mod.parse_args(["--mutate-schedule", "--max-epochs", "12", "--members", "8"])
    assert a.mutate_schedule is True and a.max_epochs == 12 and a.members == 8
    a = mod.parse_args(["--epochs", "1,2,4", "--minibatches", "4,4,8", "--no-pbt"])
    assert a.epochs == [1, 2, 4] and a.minibatches == [4, 4, 8] and a.members == 3 and a.pbt is False
    a = mod.parse_args(["--epochs", "1,2,4", "--minibatches", "16"])            # one list, one common value
    assert a.epochs == [1, 2, 4] and a.minibatches == 16 and a.members == 3
    a = mod.parse_args(["--lrs", "1e-3,1e-4", "--epochs", "5,6"])
    assert a.members == 2 and a.epochs == [5, 6]
    for bad in (["--epochs", "1,2", "--minibatches", "1,2,3"], ["--lrs", "1e-3,1e-4", "--epochs", "1,2,3"], ["--epochs", "0"],
                ["--minibatches", "4,0"], ["--epochs", "many"], ["--max-epochs", "0"]):
        with pytest.raises((SystemExit, ValueError)):
            mod.parse_args(bad)
    assert mod.INITIAL_SCHEDULE == {"num_sgd_iter": [10, 20, 30], "sgd_minibatch_size": [128, 512, 2048]}   # train/rllib/pbt.py:65-68
    # clamps: num_sgd_iter to [1, max_epochs], the minibatch size to [min(128, n), n]
    assert mod.clamp_schedule(0, 100, 512, 30) == (1, 128)
    assert mod.clamp_schedule(36, 16384, 512, 30) == (30, 512)
    assert mod.clamp_schedule(7, 300, 512, 30) == (7, 300)
    assert mod.clamp_schedule(7, 300, 64, 5) == (5, 64)                         # fewer than 128 samples: the only size is all of them
    assert mod.clamp_schedule(3, 1, 64, 5) == (3, 64)
    assert all(type(v) is int for v in mod.clamp_schedule(2.0, 200.0, 512, 30))
    text = mod.make_arg_parser().format_help()
    assert "--mutate-schedule" in text and "--max-epochs" in text
    assert "ray clamps nothing" in mod.__doc__
