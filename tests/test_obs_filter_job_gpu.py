"""The job-wide observation filter on the device (ship_sim_gym_amd/csrc/shipsim_filter.hip: the dual finalise kernel and the rows-merge
kernel; include/shipsim.h "Job-wide observation filter"; ``ObsFilter(job=True)``).

Shapes: N in {1, 257, 2305} rows — one row, a tile and a one-row tail, ten tiles in runs of 2,2,2,2,2,0,0,0 — at D = 7 and D = 176
(one pass and six passes of the finalise loop); one member, and three members on the unequal slices (257, 1, 2305) as
tests/test_obs_filter_domain_gpu.py lays them out.

* dual finalise: a filter with a base loaded and its buffer bound against the plain update from the same base (state, all four rows, bit
  for bit) and against the plain update from empty (buffer, all four rows, bit for bit), on a workspace of NaN bytes;
* rollouts: 3 steps of rollout_policy / rollout_population with the buffer bound and unbound, same seeds: every output and the state bit
  for bit, the buffer bit for bit an empty filter's state over the same observation rows;
* rows merge against ``merge_rows_reference``: count, mean, M2 bit for bit, denom within 2 ulp of the square root formed from the
  device's own M2; rows of count 0, counts past 2^31, an empty base;
* two shards replayed in one process, torch.stack as the gather: identical states, both the reference's;
* train/ppo_torch.py --gpus 2 --job-obs-filter over gloo on one device: the ranks' checksums agree, the file evaluates."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, env_config, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy

pytestmark = pytest.mark.gpu

HIST_BEAMS = {7: (1, 1), 176: (8, 16)}
SIZES = (1, 257, 2305)
SLICES = (257, 1, 2305)
K = 3


def _vec(n, D, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    history, beams = HIST_BEAMS[D]
    env = ShipVecEnv(n, n_maps=16, n_beams=beams, env_config=env_config(history), env_id_base=base)
    assert env.states_history == D
    return env


def _filter(env, **kw):
    from ship_sim_gym_amd.obs_filter import ObsFilter
    return ObsFilter(env, **kw)


def _stats(rng, P, D, counts):
    """State blocks [P, 4, D] of hand-written statistics: arbitrary means, M2 = U(1, 100) * count in the even columns and U(1, 100) in
    the odd ones (test_obs_filter_domain_gpu.py's _count_state), the last column constant; a count of 0 is the empty block."""
    st = np.zeros((P, 4, D))
    for m, count in enumerate(counts):
        if count == 0:
            continue
        st[m, 0] = rng.uniform(-5.0, 5.0, D)
        st[m, 1] = rng.uniform(1.0, 100.0, D) * np.where(np.arange(D) % 2 == 0, float(count), 1.0) if count >= 2 else 0.0
        st[m, 0, D - 1], st[m, 1, D - 1] = -1.0, 0.0
        st[m, 2] = np.sqrt(st[m, 1] / (count - 1.0)) + 1e-8 if count >= 2 else 1.0
        st[m, 3, 0] = float(count)
        assert int(st[m, 3, 0]) == count
    return st


def _batch(rng, n, D, t):
    """tests/test_obs_filter_domain_gpu.py's batch: columns of different scales, a ramp, an ill-conditioned exact column, a constant."""
    x = (rng.random_sample((n, D)) - 0.3) * (10.0 ** (t - 1) * 10.0 ** (np.arange(D) % 4 - 1))
    x[:, D - 3] = 0.37 * np.arange(n) + 1000.0 * t + rng.random_sample(n)
    x[:, D - 2] = rng.randint(-1024, 1025, n) * 2.0 ** -10 + 2.0 ** 20
    x[:, D - 1] = -1.0
    return x


def _layouts():
    return [("one", (n,)) for n in SIZES] + [("three", SLICES)]


def _env_for(sizes, D):
    env = _vec(sum(sizes), D)
    if len(sizes) > 1:
        env.set_population_slices(sizes)
    return env


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the dual finalise kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
@pytest.mark.parametrize("sizes", [s for _, s in _layouts()], ids=["%s-%d" % (w, sum(s)) for w, s in _layouts()])
def test_dual_finalise_is_the_plain_update_twice(torch_cuda, D, sizes):
    torch = torch_cuda
    P, n = len(sizes), sum(sizes)
    env = _env_for(sizes, D)
    rng = np.random.RandomState(1000 * D + n)
    base = torch.from_numpy(_stats(rng, P, D, [1000 + 37 * m for m in range(P)])).to(DEV)
    A, C_, B = _filter(env, n_members=P, job=True), _filter(env, n_members=P), _filter(env, n_members=P)
    A.load_state_dict(dict(A.state_dict(), state=base, base=base, buffer=torch.zeros_like(base)))
    C_.state.copy_(base)
    for t in range(2):                                                 # (the second batch meets a non-empty buffer)
        x = torch.from_numpy(_batch(rng, n, D, t)).to(DEV)
        A.workspace.fill_(0xFF)
        A.update(x)
        C_.update(x)
        B.update(x)
        for k, (got, want) in {"state": (A.state, C_.state), "buffer": (A.buffer, B.state)}.items():
            assert torch.isfinite(got).all() and torch.equal(got, want), (t, k, torch.nonzero(got != want)[:4].tolist())
        assert torch.equal(A.base, base)                               # (the base is the synchronisation's to change)
    assert A.buffer[:, 3, 0].tolist() == [2.0 * s for s in sizes]
    assert A.state[:, 3, 0].tolist() == [1000.0 + 37 * m + 2.0 * s for m, s in enumerate(sizes)]
    assert (A.buffer[:, 0, D - 1] == -1.0).all() and not A.buffer[:, 1, D - 1].any() and not A.buffer[:, 3, 1:].any()
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the rollout loops
# ------------------------------------------------------------------------------------------------------------------------------------
def _policy(torch, D, P):
    from ship_sim_gym_amd.population import NativePopulation
    if P == 1:
        return actor_critic_policy(torch, D, H=16, seed=D)[1]
    return NativePopulation([actor_critic_policy(torch, D, H=16, seed=D + m)[1] for m in range(P)])


def _same_outputs(torch, ra, rb, what):
    assert set(ra) == set(rb)
    for k in ra:
        if torch.is_tensor(ra[k]):
            assert ra[k].dtype == rb[k].dtype and torch.equal(ra[k], rb[k]), (what, k)


@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
@pytest.mark.parametrize("sizes", [s for _, s in _layouts()], ids=["%s-%d" % (w, sum(s)) for w, s in _layouts()])
@pytest.mark.parametrize("with_base", [False, True], ids=["empty-base", "base"])
def test_rollouts_with_the_buffer_bound(torch_cuda, D, sizes, with_base):
    """The fused loops through the dual finalise against the same loops through the plain one.  With an empty base the unbuffered
    filter itself is the empty filter over the same rollout; with a base, a third env walks the rollout step by step and feeds the rows
    it sees to an empty filter as well."""
    torch = torch_cuda
    P, n = len(sizes), sum(sizes)
    pol = _policy(torch, D, P)
    rng = np.random.RandomState(D + n)
    base = torch.from_numpy(_stats(rng, P, D, [(500 + m) * with_base for m in range(P)])).to(DEV)
    envs = [_env_for(sizes, D) for _ in range(3 if with_base else 2)]
    a, c = envs[:2]
    fa, fc = _filter(a, n_members=P, job=True), _filter(c, n_members=P)
    fa.load_state_dict(dict(fa.state_dict(), state=base, base=base, buffer=torch.zeros_like(base)))
    fc.state.copy_(base)
    a.set_obs_filter(fa)
    c.set_obs_filter(fc)
    roll = (lambda e: e.rollout_policy(pol, K, seed=9, step0=2)) if P == 1 else (lambda e: e.rollout_population(pol, K, seed=9, step0=2))
    for e in envs:
        e.reset_tensor()
    fa.workspace.fill_(0xFF)
    ra, rc = roll(a), roll(c)
    _same_outputs(torch, ra, rc, "buffer bound against unbound")
    assert torch.equal(fa.state, fc.state) and torch.equal(a.obs, c.obs) and torch.isfinite(fa.state).all() and torch.isfinite(fa.buffer).all()
    assert torch.equal(fa.base, base) and fa.buffer[:, 3, 0].tolist() == [float(K * s) for s in sizes]
    if not with_base:
        assert torch.equal(fa.buffer, fc.state)
    else:
        e = envs[2]
        fe, empty = _filter(e, n_members=P), _filter(e, n_members=P)
        fe.state.copy_(base)
        e.set_obs_filter(fe)
        act = (lambda k: e.policy_act(pol, seed=9, step=2 + k)) if P == 1 else (lambda k: e.population_act(pol, seed=9, step=2 + k))
        for k in range(K):
            empty.update(e.obs)
            fe.update()
            e.step_tensor(act(k)[0])
        assert torch.equal(fe.state, fa.state) and torch.equal(e.obs, a.obs)     # (the walk is the rollout)
        assert torch.equal(fa.buffer, empty.state)
    # unbinding the buffer: train() and load_state_dict() bind it again, set_obs_filter(plain) drops it
    from ship_sim_gym_amd import _native as N
    import ctypes as C
    out = C.c_void_p()
    for rebind in (lambda: fa.train(True), lambda: fa.load_state_dict(fa.state_dict()), lambda: a.set_obs_filter(fa)):
        rebind()
        N.check(N.lib().ssg_get_obs_filter_buffer(a._h, C.byref(out)), a._h)
        assert out.value == fa.buffer.data_ptr()
    a.set_obs_filter(fa.frozen())
    N.check(N.lib().ssg_get_obs_filter_buffer(a._h, C.byref(out)), a._h)
    assert out.value is None
    for e in envs:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the rows merge
# ------------------------------------------------------------------------------------------------------------------------------------
COUNTS = {1: [(300,), (0,), (2 ** 31 + 12345,)],
          2: [(0, 5), (2 ** 40, 4097), (1, 1)],
          8: [(0, 5, 2 ** 31 + 12345, 1, 0, 2 ** 40, 300, 7), (0, 0, 0, 0, 0, 0, 0, 0), (0, 0, 0, 2, 0, 0, 0, 0)]}


def _check_merged(got, base, rows, eps):
    """One member's merged rows (numpy [4, D]) against merge_rows_reference: tests/test_obs_filter_gpu.py's _check_state rule."""
    from ship_sim_gym_amd.obs_filter import merge_rows_reference
    want = merge_rows_reference(base, rows, eps=eps)
    assert np.isfinite(got).all()
    assert got[3, 0] == want[3, 0] and not got[3, 1:].any()
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])
    cnt = got[3, 0]
    den = np.sqrt(got[1] / (cnt - 1.0)) + eps if cnt >= 2 else np.ones_like(got[1])
    assert np.all(np.abs(got[2] - den) <= 2 * np.spacing(den)), np.abs(got[2] - den).max()
    return want


@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
@pytest.mark.parametrize("P", [1, 3])
def test_merge_rows_against_the_reference(torch_cuda, D, P):
    torch = torch_cuda
    env = _vec(257, D)
    flt = _filter(env, n_members=P, job=True)
    rng = np.random.RandomState(10 * D + P)
    for W, cases in sorted(COUNTS.items()):
        for case, counts in enumerate(cases):
            for base_count in (0, 2 ** 33 + 1, 3):
                base = _stats(rng, P, D, [base_count] * P)
                # member m sees the case's counts rotated by m, so that the members' rows differ and a misplaced block shows
                rows = np.stack([_stats(rng, P, D, [counts[(r + m) % W] for m in range(P)]) for r in range(W)])
                flt.state.fill_(float("nan"))                          # (every entry of the four rows is written)
                flt.base.copy_(torch.from_numpy(base))
                flt.buffer.fill_(1.0)
                flt.merge_rows(torch.from_numpy(rows).to(DEV))
                got = flt.state.cpu().numpy()
                for m in range(P):
                    want = _check_merged(got[m], base[m], rows[:, m], flt.eps)
                    assert want[3, 0] == base_count + sum(counts), (W, case, base_count, m)
                    if base_count + sum(counts):
                        assert got[m, 0, D - 1] == -1.0 and got[m, 1, D - 1] == 0.0      # the constant column
                    else:
                        assert not got[m, :2].any() and (got[m, 2] == 1.0).all()         # all empty: count 0, denom 1.0
                assert torch.equal(flt.base, flt.state) and not flt.buffer.any()
    # refused on a live handle, nothing launched: rows that alias the state; a plain filter
    from ship_sim_gym_amd._native import ShipSimError
    keep = flt.state.clone()
    with pytest.raises(ShipSimError, match="overlaps"):
        flt.merge_rows(flt.state[None])
    torch.cuda.synchronize()
    assert torch.equal(flt.state, keep)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. a two-rank job replayed in one process
# ------------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_replayed_in_one_process(torch_cuda):
    """Shards of 257 and 300 envs of one job (global env ids 0..556), a job filter each, the same policy: two rounds of {3-step rollout
    on each shard, torch.stack of the buffers as the gather, merge_rows on each}.  The shards' states differ during a rollout and are
    identical after every merge, both the reference's; an evaluation env's frozen view sees them."""
    torch = torch_cuda
    D, shard_envs = 7, (257, 300)
    pol = _policy(torch, D, 1)
    shards = [_vec(n, D, base=o) for n, o in zip(shard_envs, (0, 257))]
    flts = [_filter(e, job=True) for e in shards]
    ev = _vec(64, D)
    view = flts[0].frozen(ev)
    ev.set_obs_filter(view)
    for e, f in zip(shards, flts):
        e.set_obs_filter(f)
        e.reset_tensor()
    base = np.zeros((4, D))
    for rnd in range(2):
        for e in shards:
            e.rollout_policy(pol, K, seed=3, step0=K * rnd)
        assert not torch.equal(flts[0].state, flts[1].state)          # rank-local progress
        assert [f.buffer[0, 3, 0].item() for f in flts] == [float(K * n) for n in shard_envs]
        rows = torch.stack([f.buffer for f in flts])                  # [W, 1, 4, D]: the gather
        for f in flts:
            f.merge_rows(rows.clone())
        assert torch.equal(flts[0].state, flts[1].state)
        got = flts[0].state[0].cpu().numpy()
        _check_merged(got, base, rows[:, 0].cpu().numpy(), flts[0].eps)
        base = got
        assert got[3, 0] == (rnd + 1) * K * sum(shard_envs)
        for f in flts:
            assert torch.equal(f.base, f.state) and not f.buffer.any()
        assert view.state.data_ptr() == flts[0].state.data_ptr() and view.count.item() == got[3, 0]
    # sync() without a process group merges the filter's own buffer: one rank
    shards[0].rollout_policy(pol, K, seed=3, step0=2 * K)
    rows = flts[0].buffer.clone()[None]
    before = flts[0].base[0].cpu().numpy()
    flts[0].sync()
    _check_merged(flts[0].state[0].cpu().numpy(), before, rows[:, 0].cpu().numpy(), flts[0].eps)
    for e in shards + [ev]:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. two ranks: sync() through a process group, then the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_sync_to_the_same_bits(torch_cuda, tmp_path):
    """tests/obs_filter_job_worker.py as two ranks over gloo on one device: after every sync() the ranks' states are identical and are
    the reference's merge of the two buffers, in rank order, into the state before."""
    torch = torch_cuda
    import socket
    import obs_filter_job_worker as W
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "obs_filter_job_worker.py"), str(r), "2", str(port), str(tmp_path)])
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
    assert [(d["backend"], d["world"], d["envs"], d["env_id_base"]) for d in rk] == [("gloo", 2, 279, 0), ("gloo", 2, 278, 279)]
    base = np.zeros((4, rk[0]["states"][0].shape[-1]))
    for rnd in range(W.ROUNDS):
        assert torch.equal(rk[0]["states"][rnd], rk[1]["states"][rnd]), rnd
        assert [d["buffers"][rnd][0, 3, 0].item() for d in rk] == [float(W.K * d["envs"]) for d in rk]
        assert not torch.equal(rk[0]["buffers"][rnd], rk[1]["buffers"][rnd])
        got = rk[0]["states"][rnd][0].numpy()
        _check_merged(got, base, np.stack([d["buffers"][rnd][0].numpy() for d in rk]), rk[0]["eps"])
        assert got[3, 0] == (rnd + 1) * W.K * W.JOB_ENVS
        base = got
def test_trainer_on_one_rank_with_the_job_filter(torch_cuda):
    """The flag is valid with one rank: sync() merges the rank's own buffer after every rollout."""
    torch = torch_cuda
    from gpu_support import load_script
    single = load_script("train/ppo_torch.py")
    lines = []
    _, details = single.train(envs=256, updates=2, horizon=8, mode="native", update="native", job_obs_filter=True, return_details=True,
                              log=lambda *a, **k: lines.append(" ".join(str(x) for x in a)))
    sd = details["obs_filter"]
    assert sd["state"][0, 3, 0] == 2 * 8 * 256 and torch.isfinite(sd["state"]).all()
    assert torch.equal(sd["base"], sd["state"]) and not sd["buffer"].any()
    assert [ln for ln in lines if "(obs filter:" in ln and "rows merged)" in ln] and all(torch.isfinite(p).all() for p in details["params"])


def test_trainer_on_two_ranks_with_the_job_filter(torch_cuda, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    path = os.path.join(str(tmp_path), "job.ckpt")
    env = dict(os.environ, SSG_TRAIN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--mode", "native", "--update", "native", "--gpus", "2",
                        "--job-obs-filter", "--envs", "256", "--horizon", "8", "--updates", "2", "--save", path],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for head in ("parameter checksum", "observation filter checksum after %d rows merged" % (2 * 8 * 256)):
        sums = [ln for ln in r.stdout.splitlines() if ln.startswith(head)]
        assert len(sums) == 2 and sums[0] == sums[1], (head, sums)
    ckpt = checkpoint.load(path, require=("policy", "trainer", "obs_filter"))
    sd = ckpt["obs_filter"]
    assert sd["state"].shape == (1, 4, sd["obs_dim"]) and sd["state"][0, 3, 0] == 2 * 8 * 256 and torch.isfinite(sd["state"]).all()
    assert torch.equal(sd["base"], sd["state"]) and not sd["buffer"].any()
    assert len([ln for ln in r.stdout.splitlines() if "(obs filter: %d rows merged)" % (8 * 256) in ln]) == 1
    # the file evaluates, and with the job's statistics: without the section the same policy sees other inputs
    from gpu_support import load_script
    ev = load_script("train/evaluate_native.py")
    quiet = lambda *a, **k: None  # noqa: E731
    res = ev.evaluate(envs=256, episodes=1, checkpoint=path, seed=4, log=quiet)
    assert res["complete"] and np.isfinite(res["per_member"]).all()
    bare = os.path.join(str(tmp_path), "bare.ckpt")
    checkpoint.save(bare, {k: ckpt[k] for k in ("policy", "config")})
    res0 = ev.evaluate(envs=256, episodes=1, checkpoint=bare, seed=4, log=quiet)
    assert not np.array_equal(res["per_member"], res0["per_member"])
