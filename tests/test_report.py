"""The update report on the host: the header and the binding, the clip thresholds, the numpy restatement against a plain two-pass
computation, the CSV writer, and the trainers' refusals.  No GPU needed (tests/test_report_gpu.py compares the device with the
restatement bit for bit)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import ROOT, load_script

ENTRY_POINTS = ("ssg_report_clip_bounds", "ssg_ppo_report_workspace_nbytes", "ssg_ppo_report", "ssg_pop_report")


def _no_env(*a, **k):
    pytest.fail("an env was built before the refusal")


def test_header_declares_and_binding_binds_the_report(native):
    src = open(os.path.join(ROOT, "include", "shipsim.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, src, flags=re.M), name
        assert name in native.EXPORTS
        assert getattr(native.lib(), name).argtypes is not None, name
    consts = {"SSG_REPORT_COLS": native.REPORT_COLS, "SSG_REPORT_EXPLAINED_VARIANCE": native.REPORT_EXPLAINED_VARIANCE,
              "SSG_REPORT_POST": native.REPORT_POST, "SSG_REPORT_STATS": native.REPORT_STATS, "SSG_REPORT_ROWS": native.REPORT_ROWS}
    for name, value in consts.items():
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == value, name
    assert native.REPORT_COLS == 24
    assert int(re.search(r"#define SSG_ABI_VERSION (\d+)", src).group(1)) == 9 and native.lib().ssg_abi_version() == 9 == native.ABI_VERSION
    from ship_sim_gym_amd import report as R
    assert len(R.REPORT_FIELDS) == 24 and len(set(R.REPORT_FIELDS)) == 24
    assert R.REPORT_FIELDS[5] == "explained_variance"
    assert R.REPORT_FIELDS[12:19] == ("policy_loss", "value_loss", "entropy", "clip_fraction_minibatch", "kl", "grad_norm", "kl_coef")


@pytest.mark.parametrize("clip", (0.01, 0.2, 0.5, 1.0, 2.0))
def test_clip_bounds_are_log1p_rounded_from_double(clip, native):
    from ship_sim_gym_amd.report import clip_bounds
    lo, hi = clip_bounds(clip)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert hi.tobytes() == np.float32(np.log1p(clip)).tobytes()
    if clip >= 1.0:
        assert lo == -np.inf
    else:
        assert lo.tobytes() == np.float32(np.log1p(-clip)).tobytes()


def test_clip_bounds_and_workspace_refusals(native):
    L = native.lib()
    out = (C.c_float * 2)(7.0, 7.0)
    for clip in (0.0, -0.5, float("nan")):
        assert L.ssg_report_clip_bounds(clip, out) != 0
    assert L.ssg_report_clip_bounds(0.2, None) != 0
    assert tuple(out) == (7.0, 7.0)
    need = C.c_size_t(0)
    for n_envs, members in ((0, 1), (8, 0), (8, native.POP_MAX_MEMBERS + 1)):
        assert L.ssg_ppo_report_workspace_nbytes(n_envs, members, C.byref(need)) != 0
    assert L.ssg_ppo_report_workspace_nbytes(8, 1, None) != 0
    assert L.ssg_ppo_report_workspace_nbytes(65537, 3, C.byref(need)) == 0
    assert need.value >= 3 * 257 * 9 * 8 and need.value % 256 == 0


def _inputs(K, n, mean, std, seed):
    rng = np.random.default_rng(seed)
    ret = (mean + std * rng.standard_normal((K, n))).astype(np.float32)
    val = (ret + 0.5 * std * rng.standard_normal((K, n))).astype(np.float32)
    adv = rng.standard_normal((K, n)).astype(np.float32)
    return val, ret, adv


@pytest.mark.parametrize("K,n,mean,std", ((1, 1000, 0.0, 1.0), (7, 1000, 3.0, 1.0), (16, 4099, -4.0, 1.0), (5, 257, 40.0, 10.0), (3, 70001, 2.0, 0.5)))
def test_reference_agrees_with_a_two_pass_computation(K, n, mean, std, native):
    """|mean| <= 4 std: the raw-sum formula amplifies 2^-53 by about 1 + mean^2 / var <= 17 and by the summation depth, far below 1e-10."""
    from ship_sim_gym_amd.report import report_reference
    val, ret, adv = _inputs(K, n, mean, std, 11)
    rec = report_reference(val, ret, adv)
    r, e = ret.astype(np.float64), ret.astype(np.float64) - val.astype(np.float64)
    assert rec[0] == K * n
    np.testing.assert_allclose(rec[1], r.mean(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(rec[2], np.var(r), rtol=1e-10)
    np.testing.assert_allclose(rec[3], e.mean(), rtol=0, atol=1e-10)
    np.testing.assert_allclose(rec[4], np.var(e), rtol=1e-10)
    assert abs(rec[5] - (1.0 - np.var(e) / np.var(r))) <= 1e-10
    np.testing.assert_allclose(rec[6], val.astype(np.float64).mean(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(rec[7], adv.astype(np.float64).mean(), rtol=0, atol=1e-10)
    assert not rec[8:].any()


def test_reference_post_group_and_stats_rows(native):
    from ship_sim_gym_amd.report import clip_bounds, report_reference
    K, n, clip = 4, 600, 0.3
    rng = np.random.default_rng(5)
    val, ret, adv = _inputs(K, n, 1.0, 1.0, 6)
    act = rng.integers(0, 4, size=(K, n)).astype(np.int32)
    logp = (-1.0 + 0.1 * rng.standard_normal((K, n))).astype(np.float32)
    lpa = (logp[..., None] + 0.3 * rng.standard_normal((K, n, 4))).astype(np.float32)
    stats = rng.standard_normal((7, 8)).astype(np.float32)
    stats[5:] = np.nan  # (rows past the count are not read)
    rec = report_reference(val, ret, adv, act, logp, lpa, clip, stats, rows=5)
    d = np.take_along_axis(lpa, act[..., None].astype(np.int64), -1)[..., 0] - logp
    assert d.dtype == np.float32
    lo, hi = clip_bounds(clip)
    assert rec[8] == 1.0
    np.testing.assert_allclose(rec[9], -d.astype(np.float64).mean(), rtol=1e-10)
    np.testing.assert_allclose(rec[10], 0.5 * (d.astype(np.float64) ** 2).mean(), rtol=1e-10)
    assert rec[11] == ((d > hi) | (d < lo)).sum() / (K * n)
    np.testing.assert_allclose(rec[12:20], stats[:5].astype(np.float64).mean(0), rtol=1e-12)
    assert rec[20] == 5 and not rec[21:].any()
    four = report_reference(val, ret, adv, stats=stats[:3, :4])
    np.testing.assert_allclose(four[12:16], stats[:3, :4].astype(np.float64).mean(0), rtol=1e-12)
    assert not four[16:20].any() and four[20] == 3
    none = report_reference(val, ret, adv, stats=stats, rows=0)
    assert not none[12:].any()
    with pytest.raises(ValueError):
        report_reference(val, ret, adv, act=act)


def test_constant_returns_have_no_explained_variance(native):
    from ship_sim_gym_amd.report import report_reference
    val, _, adv = _inputs(3, 300, 0.0, 1.0, 2)
    rec = report_reference(val, np.full((3, 300), 2.5, dtype=np.float32), adv)
    assert rec[2] == 0.0 and np.isnan(rec[5]) and rec[1] == 2.5
    assert np.isfinite(np.delete(rec, 5)).all()


def _record(seed):
    from ship_sim_gym_amd.report import REPORT_FIELDS
    rng = np.random.default_rng(seed)
    rec = {k: float(x) for k, x in zip(REPORT_FIELDS, rng.standard_normal(24))}
    rec["explained_variance"] = float("nan") if seed % 2 else rec["explained_variance"]
    return rec


def test_progress_writer_rows_and_resume_cut(tmp_path, native):
    from ship_sim_gym_amd.report import PROGRESS_COLUMNS, REPORT_FIELDS, ProgressWriter, read_progress
    path = tmp_path / "progress.csv"
    assert PROGRESS_COLUMNS[:3] == ("update", "timesteps", "member") and PROGRESS_COLUMNS[-3:] == ("lr", "clip", "t")
    assert [c for c in PROGRESS_COLUMNS[3:-3]] == [f for f in REPORT_FIELDS if not f.startswith("unused")]
    w = ProgressWriter(path)
    recs = [_record(u) for u in range(5)]
    for u, rec in enumerate(recs):
        w.write(u, (u + 1) * 64, rec, 3e-4, 0.2)
    pop = {k: np.array([recs[0][k], recs[1][k], recs[2][k]]) for k in REPORT_FIELDS}
    assert w.write(5, 6 * 64, pop, [1e-3, 2e-3, 3e-3], [0.1, 0.2, 0.3]) == 3
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(PROGRESS_COLUMNS) and len(lines) == 1 + 5 + 3
    cols = read_progress(path)
    assert cols["update"].tolist() == [0, 1, 2, 3, 4, 5, 5, 5] and cols["member"].tolist() == [0] * 5 + [0, 1, 2]
    assert cols["timesteps"].tolist() == [64, 128, 192, 256, 320, 384, 384, 384]
    for k in PROGRESS_COLUMNS[3:-3]:  # %r: the floats read back bit for bit, NaN as NaN
        want = np.array([r[k] for r in recs] + [recs[m][k] for m in range(3)])
        assert np.array_equal(cols[k], want, equal_nan=True), k
    assert cols["lr"].tolist() == [3e-4] * 5 + [1e-3, 2e-3, 3e-3] and cols["clip"].tolist() == [0.2] * 5 + [0.1, 0.2, 0.3]
    # a run saved after update 2 and killed after update 5 resumes: the rows of updates 3.. are cut, then written again
    before = open(path).read().splitlines()
    w2 = ProgressWriter(path, resume=True)
    assert open(path).read().splitlines() == before  # (resume leaves the file until the checkpoint's update is known)
    assert w2.cut_back(2) == 5
    assert open(path).read().splitlines() == before[:4] and not os.path.exists(str(path) + ".tmp")
    for u in range(3, 5):
        w2.write(u, (u + 1) * 64, recs[u], 3e-4, 0.2)
    w2.write(5, 6 * 64, pop, [1e-3, 2e-3, 3e-3], [0.1, 0.2, 0.3])
    strip = lambda ls: [ln.rsplit(",", 1)[0] for ln in ls]  # noqa: E731  (every column but t)
    assert strip(open(path).read().splitlines()) == strip(before)
    assert ProgressWriter(path, resume=True).cut_back(99) == 0
    other = tmp_path / "other.csv"
    other.write_text("r,l,t\n1,2,3\n")
    with pytest.raises(ValueError, match="progress file"):
        ProgressWriter(other, resume=True)
    ProgressWriter(tmp_path / "new.csv", resume=True)  # (none there yet: started)
    assert open(tmp_path / "new.csv").read() == ",".join(PROGRESS_COLUMNS) + "\n"


@pytest.mark.parametrize("flag,kw", (("--report", {"report": True}), ("--report-kl", {"report_kl": True}), ("--progress", {"progress": "p.csv"})))
def test_single_policy_trainer_refuses_the_flags_without_the_device_update_or_with_ranks(flag, kw, capsys, monkeypatch):
    single = load_script("train/ppo_torch.py")
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(single, "ShipVecEnv", _no_env)
    argv = [flag] + (["p.csv"] if flag == "--progress" else [])
    for extra in ([], ["--mode", "native"], ["--mode", "native", "--update", "torch"]):
        with pytest.raises(SystemExit) as ex:
            single.parse_args(argv + extra)
        assert ex.value.code not in (0, None)
        err = capsys.readouterr().err
        assert flag in err and "--update native" in err, err
    a = single.parse_args(argv + ["--mode", "native", "--update", "native"])
    assert a.report or a.report_kl or a.progress
    with pytest.raises(SystemExit):
        single.parse_args(argv + ["--mode", "native", "--update", "native", "--gpus", "2"])
    assert "more than one rank" in capsys.readouterr().err
    for bad in (dict(mode="native", update="torch"), dict(mode="graph", update="torch")):
        with pytest.raises(ValueError, match=list(kw)[0]):
            single.train(envs=8, updates=1, log=None, **dict(kw, **bad))
    monkeypatch.setattr(single, "job_ranks", lambda: (1, 2))
    with pytest.raises(ValueError, match="more than one rank"):
        single.train(envs=8, updates=1, log=None, mode="native", update="native", **kw)


def test_the_flags_may_change_between_a_run_and_its_resumption():
    single, pbt = load_script("train/ppo_torch.py"), load_script("train/pbt_native.py")
    for mod in (single, pbt):
        assert {"report", "report_kl", "progress"} <= set(mod.CONFIG_EXEMPT)
        base = mod.run_config()
        assert mod.run_config(report=True, report_kl=True, progress="p.csv") == base  # (a file written before the flags compares equal)
        assert not {"report", "report_kl", "progress"} & set(base)
        a = mod.parse_args([] if mod is pbt else ["--mode", "native", "--update", "native"])
        assert (a.report, a.report_kl, a.progress) == (False, False, None)
