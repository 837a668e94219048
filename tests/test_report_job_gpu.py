"""The update report of a data-parallel job on the device (ssg_ppo_report_sums / ssg_ppo_report_rows; NativePPO.report_row, report_rows,
job_report) against the numpy restatements report.sums_reference / rows_reference bit for bit, against ssg_ppo_report on one row, as a
job replayed in one process, on two rank processes, and through the trainer script."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, load_script
from gpu_support import torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, synthetic_batch
from report_job_support import fsum_record, group, make_batch

pytestmark = pytest.mark.gpu

BAD = -1  # SSG_ERR_BAD_ARG
SENTINEL = -12345.5
# the unroll-4 remainder and a partly filled block; 257 blocks: thread 0 of the sums launch adds two partials
ROW_SHAPES = ((1, 1), (5, 255), (5, 256), (5, 257), (2, 65537))


@pytest.fixture(scope="module")
def env(torch_cuda):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    e = ShipVecEnv(64, n_maps=4)
    yield e
    e.close()


def same_bits(got, want):
    """Two f64 arrays: NaN in the same places, every other entry bit for bit."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(torch):
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def on_device(torch, b, post, stats=None):
    from ship_sim_gym_amd.report import scratch_nbytes
    t = {k: dev(torch, b[k]) for k in ("val", "ret", "adv")}
    t.update({k: dev(torch, b[k]) if post else None for k in ("act", "logp", "logp_all_new")})
    t["stats"] = dev(torch, stats)
    t["scratch"] = torch.full((scratch_nbytes(b["val"].shape[1], 1),), 0xFF, dtype=torch.uint8, device=DEV)  # (NaN bytes)
    return t


def report_sums(torch, env, b, post, clip=0.2, rc_only=False, **over):
    """ssg_ppo_report_sums through ctypes on numpy inputs; `over` replaces arguments by name.  Returns the row, or (rc, the row buffer)."""
    from ship_sim_gym_amd import _native as N
    K, n = b["val"].shape
    t = on_device(torch, b, post)
    before = {k: v.clone() for k, v in t.items() if v is not None and k != "scratch"}
    t["row"] = torch.full((N.REPORT_ROW_COLS,), SENTINEL, dtype=torch.float64, device=DEV)
    a = dict(K=K, N=n, clip=clip, scratch_nbytes=t["scratch"].numel(), **{k: ptr(v) for k, v in t.items()})
    a.update(over)
    rc = N.lib().ssg_ppo_report_sums(env._h, a["K"], a["N"], a["val"], a["ret"], a["adv"], a["act"], a["logp"], a["logp_all_new"], a["clip"],
                                     a["scratch"], a["scratch_nbytes"], a["row"], stream(torch))
    assert all(torch.equal(t[k], v) for k, v in before.items())  # the call reads its inputs only
    if rc_only:
        return rc, t["row"].cpu().numpy()
    N.check(rc, env._h, "ssg_ppo_report_sums")
    return t["row"].cpu().numpy()


def report_rows(torch, env, rows_np, stats=None, per_shard=False, rc_only=False, **over):
    """ssg_ppo_report_rows through ctypes on numpy inputs; `over` replaces arguments by name (the refusals)."""
    from ship_sim_gym_amd import _native as N
    rows = np.asarray(rows_np, dtype=np.float64).reshape(-1, N.REPORT_ROW_COLS)
    t = dict(rows=dev(torch, rows), stats=dev(torch, stats))
    before = {k: v.clone() for k, v in t.items() if v is not None}
    t["out"] = torch.full((1 + rows.shape[0], N.REPORT_COLS), SENTINEL, dtype=torch.float64, device=DEV)
    a = dict(h=env._h, n_rows=rows.shape[0], n_stat_rows=0 if stats is None else stats.shape[0], n_cols=0 if stats is None else stats.shape[1],
             per_shard=int(per_shard), **{k: ptr(v) for k, v in t.items()})
    a.update(over)
    rc = N.lib().ssg_ppo_report_rows(a["h"], a["n_rows"], a["rows"], a["stats"], a["n_stat_rows"], a["n_cols"], a["per_shard"], a["out"], stream(torch))
    assert all(torch.equal(t[k], v) for k, v in before.items())
    out = t["out"].cpu().numpy()
    if rc_only:
        return rc, out
    N.check(rc, env._h, "ssg_ppo_report_rows")
    used = 1 + rows.shape[0] if per_shard else 1
    assert (out[used:] == SENTINEL).all()  # nothing past the records asked for
    return out[:used] if per_shard else out[0]


def ppo_report(torch, env, b, post, clip=0.2, stats=None):
    """ssg_ppo_report's record on the same inputs."""
    from ship_sim_gym_amd import _native as N
    K, n = b["val"].shape
    t = on_device(torch, b, post, stats)
    out = torch.full((N.REPORT_COLS,), SENTINEL, dtype=torch.float64, device=DEV)
    N.check(N.lib().ssg_ppo_report(env._h, K, n, ptr(t["val"]), ptr(t["ret"]), ptr(t["adv"]), ptr(t["act"]), ptr(t["logp"]),
                                   ptr(t["logp_all_new"]), clip, ptr(t["stats"]), 0 if stats is None else stats.shape[0],
                                   0 if stats is None else stats.shape[1], ptr(t["scratch"]), t["scratch"].numel(), ptr(out), stream(torch)),
            env._h, "ssg_ppo_report")
    return out.cpu().numpy()


def make_stats(shape, seed):
    return None if shape is None else np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------------
# the sum row
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", (False, True), ids=("plain", "post"))
@pytest.mark.parametrize("K,n", ROW_SHAPES, ids=["%dx%d" % s for s in ROW_SHAPES])
def test_row_against_reference_bit_for_bit(K, n, post, env, torch_cuda):
    from ship_sim_gym_amd.report import sums_reference
    b = make_batch(K, n, seed=K * 100003 + n, offset=1.5, post=post)
    got = report_sums(torch_cuda, env, b, post, clip=0.05)
    want = sums_reference(b["val"], b["ret"], b["adv"], clip=0.05, **group(b))
    assert same_bits(got, want), (got, want)
    assert got[9] == K * n and got[10] == float(post) and got[11] == 0.0
    if post and K * n > 100:
        assert 0.0 < got[8] < K * n  # (samples on both sides of the thresholds)
    if not post:
        assert not got[6:9].any()


# ------------------------------------------------------------------------------------------------------------------------------------
# one row is ssg_ppo_report
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", (False, True), ids=("plain", "post"))
@pytest.mark.parametrize("K,n", ((1, 1), (5, 257), (2, 65537)), ids=("1x1", "5x257", "2x65537"))
def test_one_row_against_ssg_ppo_report(K, n, post, env, torch_cuda):
    torch = torch_cuda
    for const_ret in (False, True):
        b = make_batch(K, n, seed=K * 7 + n, offset=-2.0, post=post, const_ret=const_ret)
        row = report_sums(torch, env, b, post)
        for i, shape in enumerate((None, (7, 4), (7, 8), (1, 8))):
            stats = make_stats(shape, i)
            want = ppo_report(torch, env, b, post, stats=stats)
            assert same_bits(report_rows(torch, env, row, stats), want), (const_ret, shape)
            both = report_rows(torch, env, row, stats, per_shard=True)
            assert same_bits(both[0], want) and same_bits(both[1], want)
            assert np.isnan(want[5]) == (const_ret or K * n == 1)


def _trained(torch, n, K=4, seed=5, **kw):
    """(env, policy, NativePPO, batch, stats rows) after gae and one update of 2 epochs x 3 minibatches."""
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    env = ShipVecEnv(n, n_maps=4)
    _, pol = actor_critic_policy(torch, env.states_history, seed=seed)
    ppo = NativePPO(pol, env, **kw)
    batch = synthetic_batch(torch, pol, K, n, 31)
    ppo.gae(batch)
    g = torch.Generator(device=DEV).manual_seed(1)
    perm = torch.stack([torch.randperm(K * n, device=DEV, generator=g) for _ in range(2)])
    return env, pol, ppo, batch, ppo.update(batch, perm, 2, 3, stats=True)


def test_job_report_on_one_rank_is_report_key_for_key(torch_cuda):
    torch = torch_cuda
    env, pol, ppo, batch, st = _trained(torch, 300, kl_coef=0.5, kl_target=0.01, clip=0.15)
    try:
        before = {k: v.clone() for k, v in batch.items()}
        state = [t.clone() for t in (pol.params, ppo.adam_mv, ppo.kl_coef, st)]
        for post in (False, True):
            for stats in (None, st):
                want = ppo.report(batch, stats=stats, post=post)
                got = ppo.job_report(batch, stats=stats, post=post)
                assert got.pop("shards") == 1 and set(got) == set(want)
                for k in want:
                    assert same_bits(got[k], want[k]) and type(got[k]) is type(want[k]), (k, got[k], want[k])
        rec = ppo.job_report(batch, stats=st, post=True, per_shard=True)
        (shard,) = rec["shard_records"]
        assert all(same_bits(shard[k], rec[k]) for k in shard) and rec["post"] == 1.0 and rec["approxkl_ppo2"] > 0.0
        # enqueued only, on the device; the acting policy's distribution stays; nothing of the trainer moves
        row = ppo.report_row(batch, post=True)
        assert row.is_cuda and row.dtype == torch.float64 and tuple(row.shape) == (12,)
        out = ppo.report_rows(row[None], st)
        assert out.is_cuda and tuple(out.shape) == (24,) and tuple(ppo.report_rows(torch.stack([row, row]), st, per_shard=True).shape) == (3, 24)
        assert torch.equal(out, ppo.report_device(batch, stats=st, post=True))
        assert set(batch) == set(before) and all(torch.equal(batch[k], before[k]) for k in before)
        assert all(torch.equal(a, b) for a, b in zip(state, (pol.params, ppo.adam_mv, ppo.kl_coef, st)))
        with pytest.raises(ValueError, match="report_rows"):
            ppo.report_rows(torch.zeros((2, 11), dtype=torch.float64, device=DEV))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# a job replayed in one process
# ------------------------------------------------------------------------------------------------------------------------------------
def test_three_shards_replayed_in_one_process(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.report import rows_reference
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    K, sizes = 8, (64, 300, 1)
    envs = [ShipVecEnv(n, n_maps=4) for n in sizes]
    try:
        _, pol = actor_critic_policy(torch, envs[0].states_history, seed=5)
        ppos = [NativePPO(pol, e, clip=0.15) for e in envs]
        batches = [synthetic_batch(torch, pol, K, n, 40 + r) for r, n in enumerate(sizes)]
        for p, b in zip(ppos, batches):
            p.gae(b)
        stats = dev(torch, make_stats((6, 8), 3))
        rows = torch.stack([p.report_row(b, post=True) for p, b in zip(ppos, batches)])
        got = ppos[0].report_rows(rows, stats, per_shard=True).cpu().numpy()
        want = rows_reference(rows.cpu().numpy(), stats.cpu().numpy(), per_shard=True)
        assert same_bits(got, want)
        for r, (p, b) in enumerate(zip(ppos, batches)):
            own = p.report_device(b, stats=stats, post=True).cpu().numpy()
            assert same_bits(got[1 + r, :12], own[:12]) and same_bits(got[1 + r], own), r
        # against exact totals over the concatenated batch: the CPU test's bound; the clip fraction is a count
        whole = {k: np.concatenate([b[k].cpu().numpy().reshape(K, n) for b, n in zip(batches, sizes)], axis=1) for k in ("val", "ret", "adv", "act", "logp")}
        whole["logp_all_new"] = np.concatenate([p.dist({"obs": b["obs"]}).cpu().numpy().reshape(K, n, 4) for p, b, n in zip(ppos, batches, sizes)], axis=1)
        exact = fsum_record(whole, 0.15)
        assert got[0, 0] == K * sum(sizes) == exact[0] and got[0, 8] == 1.0
        for c in (1, 2, 3, 4, 5, 6, 7, 9, 10):
            print("column %d: device %r, exact %r, difference %.3e" % (c, got[0, c], exact[c], abs(got[0, c] - exact[c])))
            assert abs(got[0, c] - exact[c]) <= 1e-9, c
        assert got[0, 11] == exact[11] and 0.0 < exact[11] < 1.0
        # W = 64 rows
        many = torch.stack([rows[i % 3] for i in range(64)])
        got64 = ppos[0].report_rows(many, stats, per_shard=True).cpu().numpy()
        assert got64.shape == (65, 24) and same_bits(got64, rows_reference(many.cpu().numpy(), stats.cpu().numpy(), per_shard=True))
        assert got64[0, 0] == sum(K * sizes[i % 3] for i in range(64))
        # rows whose post flags disagree: NaN in the job's [8..11], the shards' own views stand
        mixed = rows.clone()
        mixed[1, 10] = 0.0
        out = ppos[0].report_rows(mixed, None, per_shard=True).cpu().numpy()
        assert same_bits(out, rows_reference(mixed.cpu().numpy(), None, per_shard=True)) and np.isnan(out[0, 8:12]).all() and out[2, 8] == 0.0
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(env, torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.report import scratch_nbytes
    b = make_batch(2, 300, seed=13)
    small = torch.zeros(scratch_nbytes(300, 1) + 256, dtype=torch.uint8, device=DEV)
    for what, over in (("NULL value", dict(val=None)), ("NULL ret", dict(ret=None)), ("NULL adv", dict(adv=None)), ("NULL row", dict(row=None)),
                       ("NULL scratch", dict(scratch=None)), ("K < 1", dict(K=0)), ("N < 1", dict(N=0)), ("act alone missing", dict(act=None)),
                       ("logp alone missing", dict(logp=None)), ("logp_all_new alone missing", dict(logp_all_new=None)),
                       ("only act", dict(logp=None, logp_all_new=None)), ("clip 0 with the post group", dict(clip=0.0)),
                       ("scratch too small", dict(scratch_nbytes=2 * 9 * 8 - 1)),
                       ("scratch misaligned", dict(scratch=C.c_void_p(small.data_ptr() + 8)))):
        rc, row = report_sums(torch, env, b, True, rc_only=True, **over)
        assert rc == BAD and (row == SENTINEL).all(), what
    rc, row = report_sums(torch, env, b, True, rc_only=True, scratch_nbytes=2 * 9 * 8)  # (exactly what 300 envs need)
    assert rc == 0 and row[9] == 600.0
    rows = np.stack([row, row])
    stats = make_stats((3, 4), 2)
    for what, over in (("NULL handle", dict(h=None)), ("NULL rows", dict(rows=None)), ("NULL out", dict(out=None)), ("no rows", dict(n_rows=0)),
                       ("negative rows", dict(n_rows=-1)), ("65 rows", dict(n_rows=65)), ("n_cols 5", dict(n_cols=5)), ("n_cols 0", dict(n_cols=0)),
                       ("no stats rows", dict(n_stat_rows=0))):
        rc, out = report_rows(torch, env, rows, stats, per_shard=True, rc_only=True, **over)
        assert rc == BAD and (out == SENTINEL).all(), what
    rc, out = report_rows(torch, env, rows, None, rc_only=True, n_cols=5, n_stat_rows=0)  # (not read without stats)
    assert rc == 0 and out[0, 0] == 1200.0 and (out[1:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# two ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_hold_the_same_record_and_replay(env, torch_cuda, tmp_path):
    torch = torch_cuda
    import report_job_worker as W
    from ship_sim_gym_amd.report import REPORT_FIELDS, rows_reference
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "report_job_worker.py"), str(r), "2", str(port), str(tmp_path)])
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
    assert all((k["backend"], k["world"], k["shard_envs"]) == (want_backend, 2, [200, 200]) for k in rk)

    def flat(rec):
        return np.array([[d[k] for k in REPORT_FIELDS] for d in [rec] + rec["shard_records"]])

    a, b = flat(rk[0]["record"]), flat(rk[1]["record"])
    assert same_bits(a, b) and torch.equal(rk[0]["stats"], rk[1]["stats"])
    for k in ("lr", "clip", "step", "updates", "kl_coef_now", "shards"):
        assert rk[0]["record"][k] == rk[1]["record"][k], k
    assert rk[0]["record"]["shards"] == 2 and a[0, 0] == 2 * W.K * 200 and a[0, 8] == 1.0 and a[0, 20] == W.EPOCHS * W.MINIBATCHES
    assert not torch.equal(rk[0]["row"], rk[1]["row"])  # (the shards saw different envs)
    # the replay in this process: the ranks' saved rows stacked, the job's stats rows
    rows, stats = np.stack([k["row"].numpy() for k in rk]), rk[0]["stats"].numpy()
    assert same_bits(report_rows(torch, env, rows, stats, per_shard=True), a)
    assert same_bits(rows_reference(rows, stats, per_shard=True), a)
    for r in range(2):  # shard r's view is rank r's own report
        own = np.array([rk[r]["own"][k] for k in REPORT_FIELDS])
        assert same_bits(a[1 + r], own) and a[1 + r, 0] == W.K * 200


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_on_one_rank_writes_the_reports_file(tmp_path, torch_cuda):
    from ship_sim_gym_amd.report import read_progress
    single = load_script("train/ppo_torch.py")
    kw = dict(envs=256, updates=2, horizon=8, mode="native", update="native", seed=4)
    job, own, lines = tmp_path / "job.csv", tmp_path / "own.csv", []
    single.train(log=lines.append, job_report_kl=True, job_progress=str(job), job_report_shards=True, **kw)
    single.train(log=lambda *a: None, report_kl=True, progress=str(own), **kw)
    a, b = read_progress(job), read_progress(own)
    assert a["update"].tolist() == [0, 1] and a["timesteps"].tolist() == [2048, 4096] and (a["n"] == 2048).all() and (a["post"] == 1).all()
    for k in b:
        if k != "t":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert sum("job report (1 ranks, 2048 samples): explained variance" in ln for ln in lines) == 2
    assert sum("job report, shard 0: 2048 samples" in ln for ln in lines) == 2


def test_a_resumed_run_cuts_the_jobs_file_back(tmp_path, torch_cuda):
    """One rank: --resume cuts --job-progress's file back to the checkpoint's update, as it cuts --progress's."""
    from ship_sim_gym_amd.report import read_progress
    single = load_script("train/ppo_torch.py")
    kw = dict(envs=256, horizon=8, mode="native", update="native", seed=4, log=lambda *a: None, job_report_kl=True)
    whole, cut, ckpt = tmp_path / "whole.csv", tmp_path / "cut.csv", tmp_path / "run.ckpt"
    single.train(updates=3, job_progress=str(whole), **kw)
    single.train(updates=2, job_progress=str(cut), save=str(ckpt), **kw)  # (the file holds updates 0 and 1; the checkpoint is update 1's)
    single.train(updates=3, job_progress=str(cut), **kw)  # the run goes on past its checkpoint: rows 0 .. 2 from a fresh start
    single.train(updates=3, job_progress=str(cut), resume=str(ckpt), **kw)
    a, b = read_progress(whole), read_progress(cut)
    assert a["update"].tolist() == [0, 1, 2] == b["update"].tolist()
    for k in a:
        if k != "t":
            assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_trainer_on_two_ranks_reports_the_job(tmp_path, torch_cuda):
    from ship_sim_gym_amd.report import read_progress
    path = os.path.join(str(tmp_path), "job.csv")
    env = dict(os.environ, SSG_TRAIN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--gpus", "2", "--envs", "256", "--horizon", "8",
                        "--updates", "2", "--mode", "native", "--update", "native", "--perm", "native", "--job-report-kl", "--job-progress", path,
                        "--job-report-shards"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    cols = read_progress(path)
    assert cols["update"].tolist() == [0, 1] and cols["member"].tolist() == [0, 0] and cols["timesteps"].tolist() == [2048, 4096]
    assert (cols["n"] == 2 * 8 * 128).all() and (cols["post"] == 1).all() and (cols["stats_rows"] == 8).all()
    assert np.isfinite(cols["policy_loss"]).all() and (cols["approxkl_ppo2"] > 0).all()
    # the ranks share one pipe, and a write is atomic, not a line: rank 1's checksum may land between a line of rank 0's and its newline,
    # so the checksums are found and taken out by pattern, then rank 0's lines are counted
    checksum = r"parameter checksum after \d+ Adam steps: [0-9a-f]{64}"
    sums = re.findall(checksum, r.stdout)
    assert len(sums) == 2 and sums[0] == sums[1], sums
    out = re.sub(checksum, "", r.stdout).splitlines()
    assert sum("job report (2 ranks, 2048 samples): explained variance" in ln for ln in out) == 2
    assert sum("job report, shard %d: 1024 samples" % s in ln for ln in out for s in (0, 1)) == 4
