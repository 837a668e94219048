"""The job-wide return filter on the device (ship_sim_gym_amd/csrc/shipsim_retfilter.hip: ret_batch_kernel and ret_job_chain_kernel;
include/shipsim.h "Job-wide return filter"; ``ReturnFilter(job=True)``).  The inputs are tests/ret_filter_support.py's synthetic [K, N]
tensors with the last step a ramp over the env index (the tiles' and the shards' means then lie far apart, so the association of
every merge shows in M2's last bits); an env serves as the handle only.

Shapes: N in {1, 257, 2305} (one row; a tile and a one-row tail; ten tiles in runs of 2,2,2,2,2,0,0,0) x K in {1, 3, 5, 33} (below one
staged pass of the walk, one pass plus one, across the 32-steps-per-workgroup grid of ret_batch_kernel); at N = 1 also K = 257 (across
ret_job_chain_kernel's 256-thread stride), K = 513 (across the 512 steps its LDS serves at a time) and K = 1025 (chunked calls on both
sides of ONE gather).

* one rank against today's call, from the same state and carry, on a workspace of NaN bytes: state (all four entries), carry, out and
  denoms bit for bit; against the numpy restatements: rows, count, mean, M2 and carry bit for bit, denoms within 2 ulp, out bit for bit
  the division by the device's own denoms (tests/ret_filter_support.py's ``_check``, as tests/test_ret_filter_gpu.py compares);
* value edges: gamma in {0, 0.99, 1}, a step with every env done and one with none, constant rewards at eps = 0;
* two calls over K1 and then K2 leave what one call over K1 + K2 leaves;
* W in {2, 3, 8} ranks replayed in one process, torch.stack as the gather, the unequal shards (257, 1, 2305) among them: every rank ends
  with the same state, ``job_reference``'s; each rank's out is its rewards over the common denoms; a rank's rows are a lone filter's;
* ``DataParallelPPO.gae`` with a job filter against ``NativePPO.gae`` with a plain one, with and without "boot";
* train/ppo_torch.py: one rank is --norm-reward bit for bit and resumes; --gpus 2 over gloo on one device: the checksums agree."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, load_script, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy
from ret_filter_support import D, _check, _dev, _filter, _ramp_inputs, _same_bits, _ulp_close, handles  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(n, K) for n in (1, 257, 2305) for K in (1, 3, 5, 33)] + [(1, 257), (1, 513), (1, 1025)]
SHARDS = (257, 1, 2305)
STATE0 = np.array([0.25, 40.0, np.sqrt(40.0 / 999.0) + 1e-8, 1000.0])


def _load(torch, flt, state0, carry0):
    flt.state.copy_(torch.from_numpy(np.asarray(state0, dtype=np.float64)).reshape(1, 4))
    flt.carry.copy_(torch.from_numpy(np.asarray(carry0, dtype=np.float64)))
    return flt


def _split_apply(torch, flt, r, d, K, fill=0xFF):
    """shard_rows plus apply_rows with the rank's own rows, on a workspace of `fill` bytes: (batch, rows)."""
    flt.to_native(min(K, 1024))
    flt.workspace.fill_(fill)
    batch = {"rew": r, "done": d}
    rows = flt.shard_rows(batch)
    assert rows.shape == (K, 4) and rows.dtype == torch.float64
    flt.apply_rows(batch, rows[None])
    return batch, rows


@pytest.mark.parametrize("n,K", SHAPES, ids=["n%d-K%d" % s for s in SHAPES])
def test_one_rank_is_the_plain_call_and_the_references(torch_cuda, handles, n, K):
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import batch_rows_reference, job_reference
    env = handles(n)
    gamma = (0.0, 0.99, 1.0)[(n + K) % 3]
    rew, done = _ramp_inputs(K, n, seed=1000 * n + K)
    carry0 = np.random.RandomState(K).uniform(-1.0, 1.0, n)
    r, d = _dev(torch, rew, done, pad=3 if K == 5 else 0)
    for state0 in (np.zeros(4), STATE0):
        plain = _load(torch, _filter(env, gamma=gamma, clip=10.0, eps=1e-8), state0, carry0)
        job = _load(torch, _filter(env, gamma=gamma, clip=10.0, eps=1e-8, job=True), state0, carry0)
        out, den = plain.normalise(r, d)
        batch, rows = _split_apply(torch, job, r, d, K)
        # today's call, bit for bit
        for name, got, want in (("state", job.state, plain.state), ("carry", job.carry, plain.carry), ("out", batch["rew_norm"], out),
                                ("denom", batch["rew_denom"], den)):
            assert got.shape == want.shape and _same_bits(got.cpu().numpy(), want.cpu().numpy()), (name, state0[3])
        assert batch["rew_norm"].stride(0) == r.stride(0) and torch.isfinite(batch["rew_norm"]).all()
        # the restatements
        want_rows, want_carry = batch_rows_reference(carry0, rew, done, gamma)
        assert _same_bits(rows.cpu().numpy(), want_rows)
        assert _same_bits(job.carry.cpu().numpy(), want_carry)
        want_state, want_den = job_reference(state0, want_rows[None], job.eps)
        st = job.state[0].cpu().numpy()
        assert st[3] == want_state[3] == state0[3] + K * n and _same_bits(st[:2], want_state[:2])
        assert _ulp_close(batch["rew_denom"][:, 0].cpu().numpy(), want_den)
        _check(job, state0, carry0, rew, done, batch["rew_norm"], batch["rew_denom"], gamma=gamma)
        assert torch.equal(r.cpu(), torch.from_numpy(rew))               # the raw rewards stay


@pytest.mark.parametrize("gamma", (0.0, 0.99, 1.0))
def test_value_edges(torch_cuda, handles, gamma):
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import batch_rows_reference, job_reference
    n, K = 257, 5
    env = handles(n)
    rew, done = _ramp_inputs(K, n, seed=31)
    done[1], done[3] = 1, 0                                            # every env done at one step, none at another
    carry0 = np.random.RandomState(5).uniform(-1.0, 1.0, n)
    r, d = _dev(torch, rew, done)
    plain = _load(torch, _filter(env, gamma=gamma, clip=0.0, eps=1e-8), STATE0, carry0)
    job = _load(torch, _filter(env, gamma=gamma, clip=0.0, eps=1e-8, job=True), STATE0, carry0)
    out, den = plain.normalise(r, d)
    batch, rows = _split_apply(torch, job, r, d, K)
    assert torch.equal(job.state, plain.state) and torch.equal(job.carry, plain.carry)
    assert torch.equal(batch["rew_norm"], out) and torch.equal(batch["rew_denom"], den)
    want_rows, want_carry = batch_rows_reference(carry0, rew, done, gamma)
    assert _same_bits(rows.cpu().numpy(), want_rows) and _same_bits(job.carry.cpu().numpy(), want_carry)
    # (after the all-done step every carry is 0: row 2 is the batch of rew[2] alone, whatever gamma)
    assert _same_bits(rows[2].cpu().numpy(), batch_rows_reference(np.zeros(n), rew[2:3], done[2:3], gamma)[0][0])
    _check(job, STATE0, carry0, rew, done, batch["rew_norm"], batch["rew_denom"], gamma=gamma)
    # constant rewards from an empty state with eps = 0: M2 is exactly 0 at gamma = 0, the denom 0 and the division by 1
    if gamma == 0.0:
        const = np.full((K, n), -0.01)
        rc, dc = _dev(torch, const, done)
        plain0, job0 = _filter(env, gamma=0.0, clip=0.0, eps=0.0), _filter(env, gamma=0.0, clip=0.0, eps=0.0, job=True)
        out0, den0 = plain0.normalise(rc, dc)
        b0, rows0 = _split_apply(torch, job0, rc, dc, K)
        assert torch.equal(job0.state, plain0.state) and job0.state[0].tolist() == [-0.01, 0.0, 0.0, float(K * n)]
        assert rows0.cpu().tolist() == [[-0.01, 0.0, 0.0, float(n)]] * K
        assert (b0["rew_denom"] == 1.0).all() and torch.equal(b0["rew_denom"], den0)
        assert torch.equal(b0["rew_norm"], rc) and torch.equal(b0["rew_norm"], out0)
        state, denoms = job_reference(np.zeros(4), rows0.cpu().numpy()[None], 0.0)
        assert _same_bits(state, job0.state[0].cpu().numpy()) and (denoms == 1.0).all()


@pytest.mark.parametrize("n,K1,K2", [(257, 3, 4), (1, 40, 300)])
def test_two_calls_continue_as_one(torch_cuda, handles, n, K1, K2):
    torch = torch_cuda
    env = handles(n)
    rew, done = _ramp_inputs(K1 + K2, n, seed=77 + n)
    r, d = _dev(torch, rew, done)
    one = _load(torch, _filter(env, gamma=0.95, clip=1.0, job=True), STATE0, np.zeros(n))
    two = _load(torch, _filter(env, gamma=0.95, clip=1.0, job=True), STATE0, np.zeros(n))
    b, rows = _split_apply(torch, one, r, d, K1 + K2)
    b1, rows1 = _split_apply(torch, two, r[:K1], d[:K1], K1)
    b2, rows2 = _split_apply(torch, two, r[K1:], d[K1:], K2)
    assert torch.equal(torch.cat([rows1, rows2]), rows)
    assert torch.equal(two.state, one.state) and torch.equal(two.carry, one.carry)
    assert torch.equal(torch.cat([b1["rew_norm"], b2["rew_norm"]]), b["rew_norm"])
    assert torch.equal(torch.cat([b1["rew_denom"], b2["rew_denom"]]), b["rew_denom"])


# ------------------------------------------------------------------------------------------------------------------------------------
# replayed jobs: W ranks in one process, torch.stack as the gather
# ------------------------------------------------------------------------------------------------------------------------------------
JOBS = {2: (257, 2305), 3: SHARDS, 8: (1, 257, 1, 257, 2305, 1, 257, 1)}


@pytest.mark.parametrize("W", sorted(JOBS))
def test_replayed_ranks_agree_on_the_reference(torch_cuda, handles, W):
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import batch_rows_reference, job_reference
    sizes, K, gamma, clip, eps = JOBS[W], 5, 0.99, 10.0, 1e-8
    flts = [_filter(handles(n), gamma=gamma, clip=clip, eps=eps, job=True) for n in sizes]
    state, carries = np.zeros(4), [np.zeros(n) for n in sizes]
    for rnd in range(2):                                               # (the second rollout meets a state and carries in flight)
        data = [_ramp_inputs(K, n, seed=100 * W + 10 * rnd + r) for r, n in enumerate(sizes)]
        data = [(rew * (r + 1.0), done) for r, (rew, done) in enumerate(data)]  # (the shards' returns differ in scale)
        batches = [dict(zip(("rew", "done"), _dev(torch, rew, done))) for rew, done in data]
        rows = [f.shard_rows(b) for f, b in zip(flts, batches)]
        for r, (rew, done) in enumerate(data):                         # a rank's rows are a lone filter's rows on that shard
            want_rows, carries[r] = batch_rows_reference(carries[r], rew, done, gamma)
            assert _same_bits(rows[r].cpu().numpy(), want_rows), (rnd, r)
            assert _same_bits(flts[r].carry.cpu().numpy(), carries[r]), (rnd, r)
        if rnd == 0:
            lone = _filter(handles(sizes[-1]), gamma=gamma, clip=clip, eps=eps, job=True)
            assert torch.equal(lone.shard_rows(batches[-1]), rows[-1]) and not lone.state.any()
        gathered = torch.stack(rows)                                   # [W, K, 4]: the gather
        for f, b in zip(flts, batches):
            f.apply_rows(b, gathered.clone())
        want_state, want_den = job_reference(state, gathered.cpu().numpy(), eps)
        den = batches[0]["rew_denom"]
        for r, (f, b) in enumerate(zip(flts, batches)):
            assert torch.equal(f.state, flts[0].state) and torch.equal(b["rew_denom"], den), (rnd, r)
            want = np.clip(data[r][0] / den[:, 0].cpu().numpy()[:, None], -clip, clip)
            assert _same_bits(b["rew_norm"].cpu().numpy(), want), (rnd, r)
        st = flts[0].state[0].cpu().numpy()
        assert st[3] == want_state[3] == (rnd + 1) * K * sum(sizes)
        assert _same_bits(st[:2], want_state[:2]), (rnd, st, want_state)
        assert _ulp_close(den[:, 0].cpu().numpy(), want_den)
        own = np.sqrt(st[1] / (st[3] - 1.0)) + eps
        assert _ulp_close(st[2], own) and st[2] == den[-1, 0].item()
        state = st
    if W == 3:                                                         # the stated order is the computed one: another order, other bits
        swapped = job_reference(np.zeros(4), gathered.cpu().numpy()[[2, 1, 0]], eps)[0]
        first = job_reference(np.zeros(4), gathered.cpu().numpy(), eps)[0]
        assert swapped[3] == first[3] and not _same_bits(swapped[:2], first[:2])
        probe = _filter(handles(sizes[0]), gamma=gamma, clip=clip, eps=eps, job=True)
        probe.apply_rows(batches[0], gathered[[2, 1, 0]].contiguous())
        assert _same_bits(probe.state[0, :2].cpu().numpy(), swapped[:2])
        # a rank with nothing to add (rows of count 0) changes nothing
        probe2 = _filter(handles(sizes[0]), gamma=gamma, clip=clip, eps=eps, job=True)
        probe2.apply_rows(batches[0], torch.cat([gathered[:1], torch.zeros_like(gathered[:1]), gathered[1:]]))
        assert _same_bits(probe2.state[0, :2].cpu().numpy(), first[:2]) and probe2.state[0, 3].item() == first[3]


def test_a_long_rollout_of_two_ranks_is_served_in_chunks_around_one_gather(torch_cuda, handles):
    """K = 1025 at N = 1 on both ranks: two library calls on each side, the second call's rows a copy out of the gathered [2, 1025, 4]."""
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import batch_rows_reference, job_reference
    K, gamma, eps = 1025, 0.99, 1e-8
    flts = [_filter(handles(1), gamma=gamma, clip=0.0, eps=eps, job=True) for _ in range(2)]
    data = [_ramp_inputs(K, 1, seed=900 + r) for r in range(2)]
    batches = [dict(zip(("rew", "done"), _dev(torch, rew, done))) for rew, done in data]
    rows = [f.shard_rows(b) for f, b in zip(flts, batches)]
    for r, (rew, done) in enumerate(data):
        want_rows, want_carry = batch_rows_reference(np.zeros(1), rew, done, gamma)
        assert _same_bits(rows[r].cpu().numpy(), want_rows) and _same_bits(flts[r].carry.cpu().numpy(), want_carry)
    gathered = torch.stack(rows)
    assert gathered.shape == (2, K, 4)
    for f, b in zip(flts, batches):
        f.apply_rows(b, gathered)
    want_state, want_den = job_reference(np.zeros(4), gathered.cpu().numpy(), eps)
    st = flts[0].state[0].cpu().numpy()
    assert torch.equal(flts[0].state, flts[1].state) and st[3] == want_state[3] == 2 * K and _same_bits(st[:2], want_state[:2])
    den = batches[0]["rew_denom"][:, 0].cpu().numpy()
    assert torch.equal(batches[0]["rew_denom"], batches[1]["rew_denom"]) and _ulp_close(den, want_den)
    for r, b in enumerate(batches):
        assert _same_bits(b["rew_norm"].cpu().numpy(), data[r][0] / den[:, None])


# ------------------------------------------------------------------------------------------------------------------------------------
# GAE
# ------------------------------------------------------------------------------------------------------------------------------------
def _gae_batch(torch, K, n, seed, boot):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    rew, done = _ramp_inputs(K, n, seed)
    b = dict(rew=torch.from_numpy(rew).to(DEV), done=torch.from_numpy(done).to(DEV), val=torch.randn((K, n), generator=g, device=DEV),
             last_val=torch.randn((n,), generator=g, device=DEV))
    if boot:
        bt = torch.randn((K, n), generator=g, device=DEV)
        b["boot"] = torch.where(b["done"] != 0, bt, torch.zeros_like(bt)).contiguous()
    return b


@pytest.mark.parametrize("boot", (False, True), ids=("plain", "boot"))
def test_data_parallel_gae_with_a_job_filter_is_native_gae_with_a_plain_one(torch_cuda, handles, boot):
    torch = torch_cuda
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO
    n, K = 769, 5
    env = handles(n)
    pol = actor_critic_policy(torch, D, seed=3)[1]
    a, b = _gae_batch(torch, K, n, 21, boot), _gae_batch(torch, K, n, 21, boot)
    plain, job = _filter(env, gamma=0.97), _filter(env, gamma=0.97, job=True)
    adv, ret = NativePPO(pol, env).gae(a, 0.97, 0.9, return_filter=plain)
    dp = DataParallelPPO(pol, env)
    assert (dp.rank, dp.world) == (0, 1)
    adv2, ret2 = dp.gae(b, 0.97, 0.9, return_filter=job)
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2)
    assert torch.equal(a["rew_norm"], b["rew_norm"]) and torch.equal(a["rew_denom"], b["rew_denom"]) and torch.equal(job.state, plain.state)
    assert torch.equal(job.carry, plain.carry) and job.count.item() == K * n
    if boot:
        fresh = _gae_batch(torch, K, n, 21, True)
        assert torch.equal(b["boot"], fresh["boot"]) and torch.equal(b["rew"], fresh["rew"])  # boot goes to GAE as it is
        adv3, _ = dp.gae({k: v for k, v in fresh.items() if k != "boot"}, 0.97, 0.9)
        assert not torch.equal(adv3, adv2)
    # one rank: a plain filter's statistics are the job's
    dp.gae(_gae_batch(torch, K, n, 22, boot), 0.97, 0.9, return_filter=plain)


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainer
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_on_one_rank_is_norm_reward_and_resumes(torch_cuda, tmp_path):
    torch = torch_cuda
    single = load_script("train/ppo_torch.py")
    quiet = lambda *a, **k: None  # noqa: E731
    kw = dict(envs=256, horizon=8, mode="native", update="native", reward_clip=5.0, return_details=True, log=quiet)
    _, plain = single.train(updates=3, norm_reward=True, **kw)
    half = os.path.join(str(tmp_path), "half.ckpt")
    single.train(updates=2, job_norm_reward=True, save=half, **kw)
    _, job = single.train(updates=3, job_norm_reward=True, resume=half, **kw)
    assert all(torch.equal(p, q) for p, q in zip(plain["params"], job["params"]))
    a, b = plain["ret_filter"], job["ret_filter"]
    assert sorted(a) == sorted(b) and torch.equal(a["state"], b["state"]) and torch.equal(a["carry"], b["carry"]) and b["clip"] == 5.0
    assert b["state"][0, 3] == 3 * 8 * 256 and torch.isfinite(b["state"]).all()


def test_trainer_on_two_ranks_with_the_job_filter(torch_cuda, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    path = os.path.join(str(tmp_path), "job.ckpt")
    env = dict(os.environ, SSG_TRAIN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--mode", "native", "--update", "native", "--gpus", "2",
                        "--job-norm-reward", "--envs", "256", "--horizon", "8", "--updates", "2", "--save", path],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    for head in ("parameter checksum", "return filter checksum after %d returns merged" % (2 * 8 * 256)):
        sums = [ln for ln in r.stdout.splitlines() if ln.startswith(head)]
        assert len(sums) == 2 and sums[0] == sums[1], (head, sums)
    ckpt = checkpoint.load(path, require=("policy", "trainer", "ret_filter"))
    sd = ckpt["ret_filter"]
    assert sd["state"].shape == (1, 4) and sd["state"][0, 3] == 2 * 8 * 256 and torch.isfinite(sd["state"]).all()
    assert sd["carry"].shape == (128,) and sd["n_members"] == 1           # (rank 0's returns in flight)
    assert len([ln for ln in r.stdout.splitlines() if "(return filter: %d returns merged" % (8 * 256) in ln]) == 1
