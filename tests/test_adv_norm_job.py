"""Job-wide per-minibatch advantage normalisation, host side (ssg_ppo_minibatch_adv_sums, ssg_ppo_set_minibatch_adv_rows, the table
binding; ship_sim_gym_amd/dp.py's DataParallelPPO(job_adv_norm="minibatch")): the numpy restatements against the single-handle
reference and against exact sums, every refusal of the new entry points that needs no device (a handle with a made-up bound blob and
made-up device addresses, as in test_dp.py: nothing is ever touched), the last-binding-wins rule, and the trainer's command line.
No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

Q = 0x30000  # a plausible device address (256-byte aligned; never dereferenced on the host)
BIG = 1 << 40


# ------------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------------
def _perm(rng, epochs, n, n_samples, bad=0):
    """int64 [epochs, n]: permutations of [0, n) (n == n_samples) with `bad` entries per row replaced by indices outside the range."""
    perm = np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int64)
    for e in range(epochs):
        at = rng.choice(n, size=min(bad, n), replace=False)
        perm[e, at] = rng.choice([-1, -7, n_samples, n_samples + 5], size=at.size)
    return perm


@pytest.mark.parametrize("n,chunk", [(7, 3), (1025, 1025), (2049, 1024), (3000, 750)])
def test_one_shard_is_the_single_handle_reference(n, chunk):
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.ppo import minibatch_adv_reference
    rng = np.random.RandomState(n)
    adv = (rng.randn(n) * np.exp(rng.randn(n))).astype(np.float32)
    perm = _perm(rng, 2, n, n, bad=3)
    rows, parts = dp.minibatch_sums_reference(adv, perm, chunk, n, partials=True)
    C_ = -(-n // chunk)
    assert rows.shape == (2 * C_, 4) and rows.dtype == np.float64 and len(parts) == 2 * C_ and not rows[:, 3].any()
    table = dp.minibatch_rows_reference(rows[None], 1e-8)
    assert table.shape == (2 * C_, 4) and table.dtype == np.float32
    for e in range(2):
        for j in range(C_):
            idx = perm[e, j * chunk: min(n, (j + 1) * chunk)]
            valid = (idx >= 0) & (idx < n)
            row, part = minibatch_adv_reference(adv[np.where(valid, idx, 0)], valid, 1e-8, partials=True)
            assert np.array_equal(table[e * C_ + j].view(np.uint32), row.view(np.uint32)), (e, j)
            assert np.array_equal(parts[e * C_ + j].view(np.uint64), part.view(np.uint64)), (e, j)
            assert part.shape == (min(64, -(-idx.size // 1024)), 3) and rows[e * C_ + j, 2] == valid.sum()


@pytest.mark.parametrize("shards", [(700, 431), (1500, 2, 300)])
def test_job_sums_against_exact_sums(shards):
    """The job's S and Q of one minibatch (the shards' rows added in rank order) against math.fsum over the union: every term passes
    through fewer than M additions, M the union's size, so |S - exact| <= M * 2^-53 * sum|a|; likewise for a^2 (the squares of f32
    values are exact in f64)."""
    from ship_sim_gym_amd import dp
    rng = np.random.RandomState(len(shards))
    S = Qs = cnt = 0.0
    union = []
    for r, m in enumerate(shards):
        adv = (rng.randn(m) * 3 + 0.5).astype(np.float32)
        row = dp.minibatch_sums_reference(adv, rng.permutation(m)[None].astype(np.int64), m, m)[0]
        S, Qs, cnt = (row[0], row[1], row[2]) if r == 0 else (S + row[0], Qs + row[1], cnt + row[2])
        union.extend(float(v) for v in adv)
    M = len(union)
    assert cnt == M == sum(shards)
    u = 2.0 ** -53
    assert abs(S - math.fsum(union)) <= M * u * math.fsum(abs(v) for v in union)
    assert abs(Qs - math.fsum(v * v for v in union)) <= M * u * math.fsum(v * v for v in union)


def test_rows_merge_in_rank_order():
    from ship_sim_gym_amd import dp
    rows = np.zeros((3, 1, 4))
    rows[:, 0, 0] = (1e16, 1.0, -1e16)
    rows[:, 0, 1] = (1e32, 1.0, 1e32)
    rows[:, 0, 2] = (5.0, 5.0, 5.0)
    a = dp.minibatch_rows_reference(rows, 1e-8)
    b = dp.minibatch_rows_reference(rows[[0, 2, 1]], 1e-8)
    assert float(a[0, 0]) == 0.0 and float(b[0, 0]) == np.float32(1.0 / 15.0)  # (1e16 + 1 is 1e16: the 1 is lost unless it comes last)
    assert not np.array_equal(a, b)
    with pytest.raises(ValueError, match="rows must be"):
        dp.minibatch_rows_reference(rows[0], 1e-8)


def test_no_sample_and_one_sample():
    from ship_sim_gym_amd import dp
    adv = np.array([3.5, -2.0], dtype=np.float32)
    perm = np.array([[-1, 5], [1, -3]], dtype=np.int64)  # epoch 0: every index invalid; epoch 1: one sample
    rows = dp.minibatch_sums_reference(adv, perm, 2, 2)
    assert rows.tolist() == [[0.0, 0.0, 0.0, 0.0], [-2.0, 4.0, 1.0, 0.0]]
    table = dp.minibatch_rows_reference(rows[None], 0.25)
    assert table[0].tolist() == [0.0, 1.0, 1.0, 0.0]
    assert table[1].tolist() == [-2.0, 0.25, 4.0, 0.0]  # (a zero variance: std+ is adv_eps alone)
    both = dp.minibatch_rows_reference(np.stack([rows, rows[::-1]]), 0.25)  # (an empty shard adds nothing to the other's row)
    assert np.array_equal(both[0], table[1]) and np.array_equal(both[1], table[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def _handle(native, bound=True):
    L = native.lib()
    c = native.default_config()
    c.n_envs, c.history, c.n_beams = 64, 1, 2
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if bound:
        native.check(L.ssg_bind_state(h, C.c_void_p(Q)), h)
    return h


def _sums(native, h, n_samples=256, adv=Q, perm=Q, epochs=2, n=256, chunk=64, out=Q, scratch=Q, nbytes=BIG):
    p = lambda v: C.c_void_p(v) if v else None  # noqa: E731
    return native.lib().ssg_ppo_minibatch_adv_sums(h, n_samples, p(adv), p(perm), epochs, n, chunk, p(out), p(scratch), nbytes, None)


def _rows(native, h, W=2, nb=8, rows=Q, eps=1e-8, table=Q):
    p = lambda v: C.c_void_p(v) if v else None  # noqa: E731
    return native.lib().ssg_ppo_set_minibatch_adv_rows(h, W, nb, p(rows), eps, p(table), None)


SUMS_REFUSALS = [
    ("NULL advantages", dict(adv=0), b"NULL dev_adv, dev_perm, dev_out or dev_scratch"),
    ("NULL permutations", dict(perm=0), b"NULL dev_adv, dev_perm, dev_out or dev_scratch"),
    ("NULL rows", dict(out=0), b"NULL dev_adv, dev_perm, dev_out or dev_scratch"),
    ("a NULL scratch", dict(scratch=0), b"NULL dev_adv, dev_perm, dev_out or dev_scratch"),
    ("no samples", dict(n_samples=0), b"n_samples, epochs, n or chunk < 1"),
    ("no epochs", dict(epochs=0), b"n_samples, epochs, n or chunk < 1"),
    ("an empty row", dict(n=0, chunk=1), b"n_samples, epochs, n or chunk < 1"),
    ("an empty chunk", dict(chunk=0), b"n_samples, epochs, n or chunk < 1"),
    ("a chunk longer than the row", dict(chunk=257), b"chunk > n"),
    ("too many minibatches", dict(epochs=2, n=65536, chunk=2), b"more than SSG_ADV_TABLE_MAX_ROWS minibatches"),
    ("too many minibatches by one", dict(epochs=1, n=65536, chunk=1), b"more than SSG_ADV_TABLE_MAX_ROWS minibatches"),
    ("a misaligned scratch", dict(scratch=Q + 8), b"dev_scratch must be 256-byte aligned"),
    ("a scratch too small", dict(nbytes=8 * 64 * 24 - 1), b"8 minibatches need 12288"),
]


@pytest.mark.parametrize("what,kw,text", SUMS_REFUSALS, ids=[c[0] for c in SUMS_REFUSALS])
def test_sums_refuses(native, what, kw, text):
    L = native.lib()
    h = _handle(native)
    assert _sums(native, h, **kw) == -1, what  # SSG_ERR_BAD_ARG
    assert text in L.ssg_last_error(h) and b"ssg_ppo_minibatch_adv_sums" in L.ssg_last_error(h), (what, L.ssg_last_error(h))
    L.ssg_destroy(h)


ROWS_REFUSALS = [
    ("NULL rows", dict(rows=0), b"NULL dev_rows or dev_table"),
    ("a NULL table", dict(table=0), b"NULL dev_rows or dev_table"),
    ("no shards", dict(W=0), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"),
    ("too many shards", dict(W=65), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"),
    ("no minibatches", dict(nb=0), b"n_batches must be in 1..SSG_ADV_TABLE_MAX_ROWS"),
    ("too many minibatches", dict(nb=65536), b"n_batches must be in 1..SSG_ADV_TABLE_MAX_ROWS"),
    ("an infinite adv_eps", dict(eps=float("inf")), b"adv_eps is not finite"),
    ("a NaN adv_eps", dict(eps=float("nan")), b"adv_eps is not finite"),
]


@pytest.mark.parametrize("what,kw,text", ROWS_REFUSALS, ids=[c[0] for c in ROWS_REFUSALS])
def test_rows_refuses(native, what, kw, text):
    L = native.lib()
    h = _handle(native)
    assert _rows(native, h, **kw) == -1, what
    assert text in L.ssg_last_error(h) and b"ssg_ppo_set_minibatch_adv_rows" in L.ssg_last_error(h), (what, L.ssg_last_error(h))
    L.ssg_destroy(h)


def test_launching_calls_refuse_by_handle_and_size_their_scratch(native):
    L = native.lib()
    assert _sums(native, None) == -1 and _rows(native, None) == -1
    h = _handle(native, bound=False)
    assert _sums(native, h) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)  # SSG_ERR_NOT_BOUND
    assert _rows(native, h) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)
    L.ssg_destroy(h)
    nb = C.c_size_t()
    for n_batches, want in ((1, 1536), (3, 4608), (5, 7680), (65535, 65535 * 1536)):  # f64 [n][64][3], rounded up to 256 bytes
        assert L.ssg_ppo_minibatch_adv_nbytes(n_batches, C.byref(nb)) == 0 and nb.value == want and want % 256 == 0
    for args in ((0, C.byref(nb)), (65536, C.byref(nb)), (1, None)):
        assert L.ssg_ppo_minibatch_adv_nbytes(*args) == -1
        assert b"ssg_ppo_minibatch_adv_nbytes: NULL nbytes or n_batches outside 1..SSG_ADV_TABLE_MAX_ROWS" in L.ssg_last_error(None)
    assert native.ADV_TABLE_MAX_ROWS == 65535


def _table(native, h):
    table, rows, row = C.c_void_p(), C.c_int(), C.c_int()
    assert native.lib().ssg_ppo_get_adv_table(h, C.byref(table), C.byref(rows), C.byref(row)) == 0
    return table.value, rows.value, row.value


def _mode(native, h):
    mode, members = C.c_int(), C.c_int()
    assert native.lib().ssg_ppo_get_adv_norm(h, C.byref(mode), C.byref(members)) == 0
    return mode.value, members.value


def test_table_binding_refuses_and_keeps_what_was_bound(native):
    L = native.lib()
    q = C.c_void_p(Q)
    assert L.ssg_ppo_set_adv_table(None, q, 8) == -1 and b"ssg_ppo_set_adv_table: NULL handle" in L.ssg_last_error(None)
    assert L.ssg_ppo_select_adv_row(None, 0) == -1 and b"ssg_ppo_select_adv_row: NULL handle" in L.ssg_last_error(None)
    h = _handle(native, bound=False)  # (host only: no state blob is needed)
    assert _table(native, h) == (None, 0, 0)
    assert L.ssg_ppo_select_adv_row(h, 0) == -1 and b"no advantage table is bound" in L.ssg_last_error(h)
    assert L.ssg_ppo_set_adv_table(h, C.c_void_p(Q + 8), 8) == -1 and b"dev_table must be 16-byte aligned" in L.ssg_last_error(h)
    for n_rows in (0, -1):
        assert L.ssg_ppo_set_adv_table(h, q, n_rows) == -1 and b"n_rows < 1" in L.ssg_last_error(h)
    assert _table(native, h) == (None, 0, 0)
    assert L.ssg_ppo_set_adv_table(h, q, 8) == 0 and _table(native, h) == (Q, 8, 0)
    assert L.ssg_ppo_select_adv_row(h, 7) == 0 and _table(native, h) == (Q, 8, 7)
    for row in (-1, 8):
        assert L.ssg_ppo_select_adv_row(h, row) == -1 and b"outside [0, 8)" in L.ssg_last_error(h)
    assert _table(native, h) == (Q, 8, 7)
    assert L.ssg_ppo_set_adv_table(h, C.c_void_p(Q + 4), 3) == -1 and _table(native, h) == (Q, 8, 7)  # (refused: the binding stays)
    assert L.ssg_ppo_set_adv_table(h, C.c_void_p(Q + 16), 3) == 0 and _table(native, h) == (Q + 16, 3, 0)  # (a new table: row 0)
    assert L.ssg_ppo_set_adv_table(h, None, 99) == 0 and _table(native, h) == (None, 0, 0)
    for args in ((None, C.byref(C.c_void_p()), C.byref(C.c_int()), C.byref(C.c_int())), (h, None, C.byref(C.c_int()), C.byref(C.c_int()))):
        assert L.ssg_ppo_get_adv_table(*args) == -1
    L.ssg_destroy(h)


def test_the_last_binding_wins(native):
    """A handle has one source of per-minibatch statistics: a table puts the mode back to SSG_ADV_NORM_BATCH, a successful
    ssg_ppo_set_adv_norm (either mode) drops the table, a refused call of either leaves both as they were."""
    L = native.lib()
    h = _handle(native)
    q = C.c_void_p(Q)
    need = C.c_size_t()
    native.check(L.ssg_ppo_adv_norm_nbytes(1, C.byref(need)))
    mb = lambda: L.ssg_ppo_set_adv_norm(h, native.ADV_NORM_MINIBATCH, 1, q, need.value)  # noqa: E731
    assert mb() == 0 and _mode(native, h) == (native.ADV_NORM_MINIBATCH, 1)
    assert L.ssg_ppo_set_adv_table(h, q, 0) == -1 and _mode(native, h) == (native.ADV_NORM_MINIBATCH, 1)  # (refused: the mode stays)
    assert L.ssg_ppo_set_adv_table(h, q, 6) == 0
    assert _mode(native, h) == (native.ADV_NORM_BATCH, 0) and _table(native, h) == (Q, 6, 0)
    assert L.ssg_ppo_set_adv_norm(h, 9, 0, None, 0) == -1 and _table(native, h) == (Q, 6, 0)  # (refused: the table stays)
    assert L.ssg_ppo_set_adv_norm(h, native.ADV_NORM_MINIBATCH, 1, q, 1) == -1 and _table(native, h) == (Q, 6, 0)
    assert mb() == 0 and _mode(native, h) == (native.ADV_NORM_MINIBATCH, 1) and _table(native, h) == (None, 0, 0)
    assert L.ssg_ppo_set_adv_table(h, q, 6) == 0 and L.ssg_ppo_select_adv_row(h, 5) == 0
    assert L.ssg_ppo_set_adv_norm(h, native.ADV_NORM_BATCH, 0, None, 0) == 0
    assert _mode(native, h) == (native.ADV_NORM_BATCH, 0) and _table(native, h) == (None, 0, 0)
    assert L.ssg_ppo_set_adv_table(h, None, 0) == 0 and _mode(native, h) == (native.ADV_NORM_BATCH, 0)  # (unbinding nothing: fine)
    assert mb() == 0 and L.ssg_ppo_set_adv_table(h, None, 0) == 0
    assert _mode(native, h) == (native.ADV_NORM_MINIBATCH, 1)  # (an unbind of no table leaves the mode alone)
    L.ssg_destroy(h)


TABLE_TEXT = b"an advantage table is bound to the handle (ssg_ppo_set_adv_table)"


def test_update_loops_refuse_a_bound_table(native):
    """A table row is one minibatch's: the entry points that run many minibatches, or many members', are refused while a table is
    bound — after everything else the host judges about the call, ahead of the device.  ssg_ppo_update consults the device first
    (test_update_refusals.py): without one it answers for the device; test_adv_norm_job_gpu.py sees its text."""
    import test_update_refusals as U
    L = native.lib()
    for entry in ("ssg_ppo_update_ext", "ssg_pop_update", "ssg_pop_update_ext", "ssg_pop_update_sched"):
        h = U.handle(native, "bound")
        native.check(L.ssg_ppo_set_adv_table(h, C.c_void_p(Q), 6), h)
        assert U.call(native, entry, h) == -1, entry
        assert TABLE_TEXT in L.ssg_last_error(h) and entry.encode() in L.ssg_last_error(h), (entry, L.ssg_last_error(h))
        # ... and an earlier refusal of the same call keeps its place and its text
        assert U.call(native, entry, h, mv=0) == -1 and TABLE_TEXT not in L.ssg_last_error(h), entry
        assert U.call(native, entry, h, nbytes=16) == -1 and b"workspace of 16 bytes" in L.ssg_last_error(h), entry
        L.ssg_destroy(h)
    h = U.handle(native, "bound")
    native.check(L.ssg_ppo_set_adv_table(h, C.c_void_p(Q), 6), h)
    rc = U.call(native, "ssg_ppo_update", h)
    assert rc != 0 and (rc != -1 or TABLE_TEXT in L.ssg_last_error(h)), (rc, L.ssg_last_error(h))
    L.ssg_destroy(h)
    # the two that read a row are not refused for the table: on a handle of another device than the current one (so that nothing is
    # ever launched, with or without a device) they pass the table and answer for the device
    h = U.handle(native, "device1")
    native.check(L.ssg_ppo_set_adv_table(h, C.c_void_p(Q), 6), h)
    for entry in ("ssg_ppo_grad", "ssg_ppo_grad_ext"):
        assert U.call(native, entry, h) != 0 and TABLE_TEXT not in L.ssg_last_error(h), (entry, L.ssg_last_error(h))
    assert U.call(native, "ssg_ppo_update_ext", h) == -1 and TABLE_TEXT in L.ssg_last_error(h)
    L.ssg_destroy(h)


def test_apply_shards_runs_with_a_table_bound(native):
    """ssg_ppo_apply_shards reads no advantage: with a table bound it is refused for what is wrong with the call (step = 0), not for
    the table; SSG_ADV_NORM_MINIBATCH keeps its refusal and its text."""
    import test_dp as D
    L = native.lib()
    h = D._handle(native)
    native.check(L.ssg_ppo_set_adv_table(h, C.c_void_p(Q), 6), h)
    assert D._apply(native, h, step=0) == -1 and b"step must be >= 1" in L.ssg_last_error(h)
    assert D._apply(native, h, ws=0) == -1 and b"NULL workspace" in L.ssg_last_error(h)  # (the last thing the host judges about it)
    L.ssg_destroy(h)
    h = D._handle(native, advnorm=True)
    assert D._apply(native, h) == -1
    assert b"SSG_ADV_NORM_MINIBATCH is bound to the handle (ssg_ppo_set_adv_norm): per-minibatch statistics across shards are out of scope" in L.ssg_last_error(h)
    L.ssg_destroy(h)


# ------------------------------------------------------------------------------------------------------------------------------------
# the command line and the trainer class
# ------------------------------------------------------------------------------------------------------------------------------------
BASE = ["--mode", "native", "--update", "native"]


def test_trainer_flag_parses_at_any_rank_count(monkeypatch):
    from gpu_support import load_script
    mod = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = mod.parse_args(BASE + ["--gpus", "2", "--job-adv-norm", "minibatch"])
    assert (a.gpus, a.job_adv_norm, a.adv_norm) == (2, "minibatch", "batch")
    assert mod.parse_args(BASE + ["--job-adv-norm", "minibatch"]).gpus == 1
    assert mod.parse_args(BASE).job_adv_norm == "batch"
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("WORLD_SIZE", "3")
    assert mod.parse_args(BASE + ["--job-adv-norm", "minibatch"]).job_adv_norm == "minibatch"
    # its row stands in a table of its own; the rows of the flags refused with more than one rank are what they were
    assert [r[0] for r in mod.JOB_ADV_NORM_REQUIREMENTS] == ["job_adv_norm"] and "job_adv_norm" not in [r[0] for r in mod.REQUIREMENTS]
    (row,) = [r for r in mod.REQUIREMENTS if r[0] == "adv_norm"]
    assert row[4] is True and row[5] == "a rank's minibatch statistics are not the job's"


EXCLUSIONS = [("together with --adv-norm minibatch", BASE + ["--adv-norm", "minibatch", "--job-adv-norm", "minibatch"], "--adv-norm minibatch"),
              ("with the torch update", ["--mode", "native", "--update", "torch", "--job-adv-norm", "minibatch"], "--update native"),
              ("with the default mode and update", ["--job-adv-norm", "minibatch"], "--mode native")]


@pytest.mark.parametrize("what,argv,names", EXCLUSIONS, ids=[c[0] for c in EXCLUSIONS])
def test_trainer_flag_exclusions(what, argv, names, capsys, monkeypatch):
    from gpu_support import load_script
    mod = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for extra in ([], ["--gpus", "2"]):
        with pytest.raises(SystemExit) as ex:
            mod.main(argv + extra)
        assert ex.value.code not in (0, None)
        err = capsys.readouterr().err
        assert "--job-adv-norm minibatch" in err and names in err, err
    # train() refuses the same with its own names, before any device work
    kw = dict(mode="native", update="native", job_adv_norm="minibatch")
    with pytest.raises(ValueError, match="job_adv_norm.*adv_norm='minibatch'"):
        mod.train(adv_norm="minibatch", **kw)
    with pytest.raises(ValueError, match="job_adv_norm.*update='native'"):
        mod.train(**dict(kw, update="torch"))
    with pytest.raises(ValueError, match="job_adv_norm must be"):
        mod.train(**dict(kw, job_adv_norm="bogus"))


def test_data_parallel_ppo_checks_the_mode_first():
    from ship_sim_gym_amd.dp import DataParallelPPO
    with pytest.raises(ValueError, match="job_adv_norm must be 'batch' or 'minibatch'"):
        DataParallelPPO(None, None, job_adv_norm="bogus")
    with pytest.raises(ValueError, match="adv_norm must be 'batch'"):  # (the single-handle mode stays refused, whatever the job's)
        DataParallelPPO(None, None, adv_norm="minibatch", job_adv_norm="minibatch")
