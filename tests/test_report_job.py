"""The update report of a data-parallel job on the host: the sum row and the rows' merge restated in numpy against the one-policy
restatement (bit for bit) and against exact totals (math.fsum), and the trainer's four flags.  No GPU needed
(tests/test_report_job_gpu.py compares the device with the restatements bit for bit)."""
import os
import re

import numpy as np
import pytest

from gpu_support import ROOT, load_script
from report_job_support import SHARDS, bits, fsum_record, group, make_batch


def test_header_declares_and_binding_binds_the_job_report(native):
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    for name in ("ssg_ppo_report_sums", "ssg_ppo_report_rows"):
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in native.EXPORTS
        assert getattr(native.lib(), name).argtypes is not None, name
    assert int(re.search(r"#define SSG_REPORT_ROW_COLS (\d+)", src).group(1)) == native.REPORT_ROW_COLS == 12
    assert native.lib().ssg_abi_version() == 9


@pytest.mark.parametrize("post", (False, True))
@pytest.mark.parametrize("K,n", ((1, 1), (5, 255), (2, 256), (3, 257)))
def test_one_row_gives_the_one_policy_record_bit_for_bit(K, n, post, native):
    from ship_sim_gym_amd.report import report_reference, rows_reference, sums_reference
    rng = np.random.default_rng(K * 1000 + n)
    for const_ret in (False, True):
        b = make_batch(K, n, seed=K * n + post, offset=2.0, post=post, const_ret=const_ret)
        for clip in (0.2, 1.0, 2.5):
            row = sums_reference(b["val"], b["ret"], b["adv"], clip=clip, **group(b))
            assert row.shape == (12,) and row.dtype == np.float64
            assert row[9] == K * n and row[10] == float(post) and row[11] == 0.0
            if not post:
                assert not row[6:9].any()
            for stats, used in ((None, None), (rng.standard_normal((6, 4)).astype(np.float32), None),
                                (rng.standard_normal((5, 8)).astype(np.float32), 3), (rng.standard_normal((5, 8)).astype(np.float32), 0)):
                want = report_reference(b["val"], b["ret"], b["adv"], clip=clip, stats=stats, rows=used, **group(b))
                got = rows_reference(row[None], stats, used)
                assert bits(got) == bits(want), (const_ret, clip, used)
                assert np.isnan(got[5]) == (const_ret or K * n == 1)
                both = rows_reference(row[None], stats, used, per_shard=True)
                assert both.shape == (2, 24) and bits(both[0]) == bits(want) and bits(both[1]) == bits(want)


def _shard_rows(b, clip):
    from ship_sim_gym_amd.report import sums_reference
    rows, e0 = [], 0
    for n in SHARDS:
        c = slice(e0, e0 + n)
        rows.append(sums_reference(b["val"][:, c], b["ret"][:, c], b["adv"][:, c], clip=clip, **group(b, c)))
        e0 += n
    return np.stack(rows)


@pytest.mark.parametrize("offset", (-3.0, 0.0, 3.0))
def test_shards_merged_against_exact_totals(offset, native):
    """f64 sums of 4 800 terms of this size are within a few 1e-11 of the exact ones on the means and variances, and ve / vr of
    about 0.2 keeps the explained variance there: 1e-9 is far outside.  The clip fraction is a count: exactly equal."""
    from ship_sim_gym_amd.report import rows_reference
    assert sum(SHARDS) == 600
    b = make_batch(8, 600, seed=int(offset) + 7, offset=offset)
    rows = _shard_rows(b, 0.05)  # (d ~ 0.05 noise: about a third of the samples lie outside log1p(+-0.05))
    rec = rows_reference(rows)
    want = fsum_record(b, 0.05)
    assert rec[0] == 4800.0 == want[0] and rec[8] == 1.0
    for c in (1, 2, 3, 4, 5, 6, 7, 9, 10):
        assert abs(rec[c] - want[c]) <= 1e-9, (c, rec[c], want[c])
    assert rec[11] == want[11] and 0.0 < rec[11] < 1.0
    assert not rec[12:].any()


def test_row_order_mixed_flags_and_per_shard(native):
    from ship_sim_gym_amd.report import rows_reference
    b = make_batch(8, 600, seed=3, offset=1.0)
    rows = _shard_rows(b, 0.2)
    stats = np.random.default_rng(5).standard_normal((4, 8)).astype(np.float32)
    rec = rows_reference(rows, stats)
    # the reference follows the row order: left to right from row 0's value
    tot = rows[0, :10].copy()
    for r in rows[1:]:
        tot = tot + r[:10]
    assert rec[0] == tot[9] and bits(rec[1]) == bits(tot[0] / tot[9]) and bits(rec[9]) == bits(-(tot[6] / tot[9]))
    orders = {bits(rows_reference(rows[list(p)])[1:8]) for p in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1))}
    assert len(orders) > 1  # (f64 addition does not commute over four rows of this size)
    # per-shard: record 1 + r is the record of row r alone, with the same stats columns
    both = rows_reference(rows, stats, per_shard=True)
    assert both.shape == (5, 24) and bits(both[0]) == bits(rec)
    for r in range(4):
        assert bits(both[1 + r]) == bits(rows_reference(rows[r: r + 1], stats))
        assert both[1 + r, 0] == 8 * SHARDS[r] and bits(both[1 + r, 12:21]) == bits(rec[12:21])
    # mixed post flags: NaN in [8..11] of the job's record, nothing else disturbed; all off: zeros
    mixed = rows.copy()
    mixed[2, 10] = 0.0
    out = rows_reference(mixed, stats, per_shard=True)
    assert np.isnan(out[0, 8:12]).all() and bits(out[0, :8]) == bits(rec[:8]) and bits(out[0, 12:]) == bits(rec[12:])
    assert out[3, 8] == 0.0 and not out[3, 9:12].any() and out[1, 8] == 1.0
    off = rows.copy()
    off[:, 10] = 0.0
    assert not rows_reference(off)[8:12].any()


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


JOB_FLAGS = (("--job-report", []), ("--job-report-kl", []), ("--job-progress", ["p.csv"]), ("--job-report-shards", []))


def test_trainer_flags_and_their_refusals(capsys, monkeypatch):
    single = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    native_flags = ["--mode", "native", "--update", "native"]
    a = single.parse_args([])
    assert (a.job_report, a.job_report_kl, a.job_progress, a.job_report_shards) == (False, False, None, False)
    for flag, value in JOB_FLAGS:
        name = flag[2:].replace("-", "_")
        for extra in ([], ["--gpus", "2"]):  # one rank or more
            assert getattr(single.parse_args(native_flags + [flag] + value + extra), name) == (value[0] if value else True)
        for argv, words in (([flag] + value, (flag, "--mode native")),
                            (["--mode", "native", flag] + value, (flag, "--update native"))):
            with pytest.raises(SystemExit) as ex:
                single.parse_args(argv)
            err = capsys.readouterr().err
            assert ex.value.code not in (0, None) and all(w in err for w in words), (argv, err)
        for other, ovalue in (("--report", []), ("--report-kl", []), ("--progress", ["q.csv"])):
            for extra in ([], ["--gpus", "2"]):
                with pytest.raises(SystemExit) as ex:
                    single.parse_args(native_flags + [flag] + value + [other] + ovalue + extra)
                err = capsys.readouterr().err
                assert ex.value.code not in (0, None) and flag in err and "together with %s" % other in err, (flag, other, err)
        kw = {name: value[0] if value else True}
        for more, words in ((dict(), (name, "mode='native'")), (dict(mode="native"), (name, "update='native'"))):
            with pytest.raises(ValueError) as ex:
                single.train(envs=8, updates=1, log=None, **dict(kw, **more))
            assert all(w in str(ex.value) for w in words), (kw, str(ex.value))
        for other in (dict(report=True), dict(report_kl=True), dict(progress="q.csv")):
            with pytest.raises(ValueError) as ex:
                single.train(envs=8, updates=1, log=None, mode="native", update="native", **dict(kw, **other))
            assert name in str(ex.value) and "together with %s" % list(other)[0] in str(ex.value), str(ex.value)
        # what a resumed run may change: not part of the configuration
        assert name in single.CONFIG_EXEMPT and single.run_config(**kw) == single.run_config()
        assert flag in single.make_arg_parser().format_help()
    # the rank's own report stays refused in a job, exactly as it was
    for flag, value in (("--report", []), ("--report-kl", []), ("--progress", ["q.csv"])):
        with pytest.raises(SystemExit):
            single.parse_args(native_flags + [flag] + value + ["--gpus", "2"])
        err = capsys.readouterr().err
        assert flag in err and "more than one rank" in err and "their own shard" in err
    assert [r[0] for r in single.JOB_REPORT_REQUIREMENTS] == ["job_progress", "job_report_shards", "job_report_kl", "job_report"]
    assert all(r[3] == ("mode", "update") and r[4] is False for r in single.JOB_REPORT_REQUIREMENTS)
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match="more than one rank"):
        single.train(envs=8, updates=1, log=None, mode="native", update="native", report=True)
