"""GPU checks of the job-wide per-minibatch advantage normalisation (ssg_ppo_minibatch_adv_sums, ssg_ppo_set_minibatch_adv_rows, the
table binding; DataParallelPPO(job_adv_norm="minibatch")): the sums and their partials against the numpy restatement bit for bit at
every length at which the kernels take another path; the rows merge against its restatement; one rank against
NativePPO(adv_norm="minibatch") bit for bit; a job of unequal shards replayed in one process; two rank processes against each other
and against the replay; the trainer script on one rank.

Shapes: a 64-env handle for the synthetic advantages (the handle's size plays no part in them); hidden 32, 2 layers, K = 8 and 3
minibatches for the updates: 256 envs make chunks of 683 / 683 / 682."""
import ctypes as C
import hashlib
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import adv_norm_job_support as S
from dp_support import assert_bits, f32 as _np
from gpu_support import ROOT, load_script, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, split_policy

pytestmark = pytest.mark.gpu


def _vec(n, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=16, env_id_base=base)


@pytest.fixture(scope="module")
def trainer(torch_cuda):
    """A 64-env handle, a policy and a DataParallelPPO in the job mode for the synthetic tests."""
    from ship_sim_gym_amd.dp import DataParallelPPO
    env = _vec(64)
    _, pol = actor_critic_policy(torch_cuda, env.states_history, S.HIDDEN, 2, "tanh", 3, seed=4)
    yield env, pol, DataParallelPPO(pol, env, perm_seed=1, job_adv_norm="minibatch")
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the sums against the reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _device_sums(torch, env, adv, perm, chunk, n_samples):
    """ssg_ppo_minibatch_adv_sums with an explicit chunk length: (rows f64 [epochs * C, 4], partials f64 [epochs * C, 64, 3])."""
    from ship_sim_gym_amd import _native as N
    epochs, n = perm.shape
    nb = epochs * -(-n // chunk)
    need = C.c_size_t()
    N.check(N.lib().ssg_ppo_minibatch_adv_nbytes(nb, C.byref(need)))
    assert need.value == nb * 64 * 24
    scratch = torch.full((need.value,), 0xFF, dtype=torch.uint8, device="cuda:0")  # (NaN bytes: what is read was written first)
    out = torch.full((nb, 4), float("nan"), dtype=torch.float64, device="cuda:0")
    a, p = torch.from_numpy(adv).cuda(), torch.from_numpy(perm).cuda()
    assert a.numel() == n_samples
    N.check(N.lib().ssg_ppo_minibatch_adv_sums(env._h, n_samples, C.c_void_p(a.data_ptr()), C.c_void_p(p.data_ptr()), epochs, n, chunk,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel(), None),
            env._h, "ssg_ppo_minibatch_adv_sums")
    torch.cuda.synchronize()
    return out.cpu().numpy(), scratch.view(torch.float64).view(nb, 64, 3).cpu().numpy()


def _values(rng, kind, n):
    if kind == "spread":
        return (rng.randn(n) * np.exp(2 * rng.randn(n))).astype(np.float32)
    if kind == "equal":
        return np.full(n, np.float32(0.3), dtype=np.float32)
    if kind == "zeros":
        return np.where(rng.rand(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    if kind == "huge":
        return (rng.randn(n) * 1e18).astype(np.float32)
    a = rng.randn(n).astype(np.float32)  # "nonfinite": one NaN and one inf (the same entry when n == 1)
    a[rng.randint(n)] = np.inf
    a[rng.randint(n)] = np.nan
    return a


SUMS_CASES = [(1, 1), (7, 3), (256, 256), (257, 257), (1025, 1025), (2049, 1024), (65600, 65600)]


@pytest.mark.parametrize("epochs", [1, 3])
@pytest.mark.parametrize("n,chunk", SUMS_CASES, ids=["%dx%d" % c for c in SUMS_CASES])
def test_sums_against_the_reference_bitwise(torch_cuda, trainer, n, chunk, epochs):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    env, _, _ = trainer
    C_ = -(-n // chunk)
    for seed, kind in enumerate(("spread", "equal", "zeros", "huge", "nonfinite")):
        rng = np.random.RandomState(1000 * n + 10 * epochs + seed)
        adv = _values(rng, kind, n)
        perm = np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int64)
        if n > 1:  # indices below 0 and at or above n_samples, sprinkled in
            for e in range(epochs):
                at = rng.choice(n, size=max(1, n // 50), replace=False)
                perm[e, at] = rng.choice([-1, -(1 << 40), n, n + 1, 1 << 40], size=at.size)
        if epochs == 3:  # one minibatch with every index invalid
            j = C_ - 1
            perm[1, j * chunk: min(n, (j + 1) * chunk)] = -1
        want, want_parts = dp.minibatch_sums_reference(adv, perm, chunk, n, partials=True)
        got, got_parts = _device_sums(torch, env, adv, perm, chunk, n)
        nan_ok = kind == "nonfinite"
        assert_bits(got, want, (kind, "rows"), nan_ok=nan_ok)
        if epochs == 3:
            assert got[C_ + C_ - 1].tolist() == [0.0, 0.0, 0.0, 0.0]
        for y, part in enumerate(want_parts):
            M = min(chunk, n - (y % C_) * chunk)
            assert part.shape[0] == min(64, -(-M // 1024))
            assert_bits(got_parts[y, :part.shape[0]], part, (kind, "partials of minibatch", y), nan_ok=nan_ok)


def test_sums_through_the_trainer(torch_cuda, trainer):
    """shard_minibatch_sums cuts the minibatches update() cuts: chunk_split's chunk over the batch's samples."""
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    env, pol, tr = trainer
    rng = np.random.RandomState(5)
    adv = rng.randn(8, 250).astype(np.float32)  # 2000 samples, 3 minibatches: 667 / 667 / 666
    perm = np.stack([rng.permutation(2000) for _ in range(2)]).astype(np.int64)
    rows, parts = tr.shard_minibatch_sums({"adv": torch.from_numpy(adv).cuda()}, torch.from_numpy(perm).cuda(), 3, partials=True)
    want, want_parts = dp.minibatch_sums_reference(adv, perm, 667, 2000, partials=True)
    assert tuple(rows.shape) == (6, 4) and tuple(parts.shape) == (6, 64, 3)
    assert_bits(rows.cpu().numpy(), want, "rows")
    assert_bits(parts[:, 0].cpu().numpy(), np.stack([p[0] for p in want_parts]), "partials")
    assert rows[:, 2].tolist() == [667.0, 667.0, 666.0] * 2
    with pytest.raises(ValueError, match="perm must be"):
        tr.shard_minibatch_sums({"adv": torch.from_numpy(adv).cuda()}, torch.from_numpy(perm[:, :-1].copy()).cuda(), 3)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the rows merge
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 64])
def test_rows_merge_against_the_reference_bitwise(torch_cuda, trainer, W):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    env, pol, tr = trainer
    rng = np.random.RandomState(W)
    nb = 300  # (two workgroups, the second ragged)
    cnt = rng.randint(0, 700, (W, nb)).astype(np.float64)
    mean = rng.randn(W, nb) * np.exp(rng.randn(W, nb))
    rows = np.zeros((W, nb, 4))
    rows[:, :, 0], rows[:, :, 2] = mean * cnt, cnt
    rows[:, :, 1] = cnt * (mean ** 2 + np.exp(rng.randn(W, nb)))
    rows[:, 1] = 0.0                       # a minibatch no shard has a sample of
    rows[:, 2] = 0.0
    rows[W - 1, 2, :3] = (-1.5, 2.25, 1.0)  # ... and one with ONE sample in the whole job
    rows[:, 3, 0] = -0.0                    # a signed zero sum
    if W >= 3:  # the order shows: (1e16 + 1) - 1e16 is 0, (1e16 - 1e16) + 1 is 1
        rows[:, 0] = 0.0
        rows[0, 0, :3], rows[1, 0, :3], rows[W - 1, 0, :3] = (1e16, 1e32, 5.0), (1.0, 1.0, 5.0), (-1e16, 1e32, 5.0)
    want = dp.minibatch_rows_reference(rows, tr.hp.adv_eps)
    table = tr.set_minibatch_rows(torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    assert_bits(_np(table), want, "table")
    assert _np(table)[1].tolist() == [0.0, 1.0, 1.0, 0.0] and _np(table)[2, 0] == -1.5 and _np(table)[2, 1] == np.float32(tr.hp.adv_eps)
    if W >= 3:
        assert _np(table)[0, 0] == 0.0
        swapped = rows.copy()
        swapped[[1, W - 1]] = swapped[[W - 1, 1]]
        assert _np(tr.set_minibatch_rows(torch.from_numpy(swapped).cuda()))[0, 0] == np.float32(1.0 / 15.0)
    assert env.adv_table() == (tr.minibatch_table().data_ptr(), nb, 0) and env.adv_norm() == (0, 0)
    with pytest.raises(ValueError, match="rows must be"):
        tr.set_minibatch_rows(torch.from_numpy(rows[0]).cuda())


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. one rank is NativePPO(adv_norm="minibatch")
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_envs", [256, 192])
@pytest.mark.parametrize("case", ["plain", "ext", "split_ext"])
def test_one_rank_is_the_single_handle_mode_bitwise(torch_cuda, case, n_envs):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    kw = {} if case == "plain" else S.TERMS
    make = split_policy if case == "split_ext" else actor_critic_policy
    envs, pols = [_vec(n_envs), _vec(n_envs)], []
    for env in envs:
        pols.append(make(torch, env.states_history, S.HIDDEN, 2, "tanh", 3, seed=3)[1])
        env.reset_tensor()
    single = NativePPO(pols[0], envs[0], perm_seed=11, adv_norm="minibatch", **kw)
    job = DataParallelPPO(pols[1], envs[1], perm_seed=11, job_adv_norm="minibatch", **kw)
    p0 = pols[0].params.clone()
    bs = [dict(env.rollout_policy(pol, S.K, seed=5, step0=0)) for env, pol in zip(envs, pols)]
    single.gae(bs[0])
    job.gae(bs[1])
    assert all(torch.equal(bs[0][k], bs[1][k]) for k in ("obs", "act", "logp", "adv", "ret"))
    n = S.K * n_envs
    perm = single.draw_perm(n, S.EPOCHS)
    assert torch.equal(perm, job.draw_perm(n, S.EPOCHS))
    chunk, n_chunks = chunk_split(n, S.MINIBATCHES)
    assert n_chunks == 3 and (n - 2 * chunk < chunk) == (n_envs == 256)
    s0 = single.update(bs[0], perm, S.EPOCHS, S.MINIBATCHES, stats=True)
    s1 = job.update(bs[1], perm, S.EPOCHS, S.MINIBATCHES, stats=True)
    assert s0.shape == s1.shape == (S.EPOCHS * 3, 4 if case == "plain" else 8) and torch.equal(s0, s1), (s0, s1)
    assert torch.equal(pols[0].params, pols[1].params) and torch.equal(single.adam_mv, job.adam_mv)
    assert torch.equal(single.kl_coef, job.kl_coef) and (single.step, single.updates) == (job.step, job.updates) == (6, 1)
    assert not torch.equal(pols[0].params, p0)
    # every table row is the row the single-handle mode's two launches write for that minibatch
    table = job.minibatch_table()
    assert tuple(table.shape) == (S.EPOCHS * 3, 4) and envs[1].adv_table() == (table.data_ptr(), 6, 5)
    for e in range(S.EPOCHS):
        for j in range(3):
            single.grad(bs[0], perm[e, j * chunk: (j + 1) * chunk])
            assert torch.equal(single.minibatch_adv_stats()[0], table[e * 3 + j]), (e, j)
    assert not torch.equal(table[0], table[1])
    # a table row is one minibatch's: the update loop in C refuses it, and the table stays bound
    with pytest.raises(N.ShipSimError, match=r"ssg_ppo_update(_ext)?: an advantage table is bound to the handle \(ssg_ppo_set_adv_table\)"):
        NativePPO.update(job, bs[1], perm, S.EPOCHS, S.MINIBATCHES)
    assert envs[1].adv_table()[:2] == (table.data_ptr(), 6) and (job.step, job.updates) == (6, 1)
    # another trainer on the env rebinds its own source: the table is dropped, and the job's trainer binds it again
    other = NativePPO(pols[1], envs[1], **kw)
    other.grad(bs[1], perm[0, :chunk])
    assert envs[1].adv_table() == (None, 0, 0)
    job.select_minibatch(1, 2)
    job.local_row(bs[1], perm[1, 2 * chunk:])
    assert envs[1].adv_table() == (table.data_ptr(), 6, 5)
    sd = job.state_dict()
    assert sd["job_adv_norm"] == "minibatch"
    job.load_state_dict(sd)
    with pytest.raises(ValueError, match="job_adv_norm"):
        job.load_state_dict({k: v for k, v in sd.items() if k != "job_adv_norm"})  # (a state without the key is a "batch" one)
    for env in envs:
        env.close()


def test_batch_mode_states_load_without_the_key(torch_cuda, trainer):
    from ship_sim_gym_amd.dp import DataParallelPPO
    env, pol, tr = trainer
    plain = DataParallelPPO(pol, env)
    sd = plain.state_dict()
    assert sd["job_adv_norm"] == "batch"
    plain.load_state_dict({k: v for k, v in sd.items() if k != "job_adv_norm"})  # (a checkpoint from before the mode)
    with pytest.raises(ValueError, match="job_adv_norm"):
        plain.load_state_dict(dict(sd, job_adv_norm="minibatch"))
    for who in ("shard_minibatch_sums", "set_minibatch_rows", "select_minibatch", "minibatch_table"):
        with pytest.raises(ValueError, match="job_adv_norm is 'batch'"):
            getattr(plain, who)(*([None] * {"shard_minibatch_sums": 3, "set_minibatch_rows": 1, "select_minibatch": 2, "minibatch_table": 0}[who]))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. a job replayed in one process
# ------------------------------------------------------------------------------------------------------------------------------------
def _shard_trainers(torch, shard_envs):
    from ship_sim_gym_amd.dp import DataParallelPPO
    envs, trainers, base = [], [], 0
    for r, n in enumerate(shard_envs):
        env = _vec(n, base)
        _, pol = actor_critic_policy(torch, env.states_history, S.HIDDEN, 2, "tanh", 3, seed=S.POLICY_SEED)
        trainers.append(DataParallelPPO(pol, env, perm_seed=S.PERM_SEED, member=r, job_adv_norm="minibatch", **S.TERMS))
        env.reset_tensor()
        envs.append(env)
        base += n
    return envs, trainers


@pytest.mark.parametrize("shard_envs", [(128, 64), (64, 64, 64)], ids=["128+64", "64+64+64"])
def test_a_job_replayed_in_one_process(torch_cuda, shard_envs):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    envs, trainers = _shard_trainers(torch, shard_envs)
    p0 = trainers[0].policy.params.clone()
    for rnd in range(2):
        bs = [dict(env.rollout_policy(tr.policy, S.K, seed=S.ROLLOUT_SEED, step0=rnd * S.K)) for env, tr in zip(envs, trainers)]
        stacked, stats = S.replay_update(torch, trainers, bs, shard_envs)
        assert tuple(stacked.shape) == (len(shard_envs), S.EPOCHS * 3, 4) and tuple(stats.shape) == (S.EPOCHS * 3, 8)
        want = dp.minibatch_rows_reference(stacked.cpu().numpy(), trainers[0].hp.adv_eps)
        for r, tr in enumerate(trainers):
            assert_bits(_np(tr.minibatch_table()), want, ("table of shard", r, "round", rnd))
            assert torch.equal(tr.policy.params, trainers[0].policy.params) and torch.equal(tr.adam_mv, trainers[0].adam_mv), (r, rnd)
            assert torch.equal(tr.kl_coef, trainers[0].kl_coef) and tr.step == 6 * (rnd + 1)
        # the counts are the job's minibatches': chunk j of every shard together
        counts = stacked[:, :, 2].sum(0).cpu().tolist()
        assert counts == [float(sum(dp.chunk_counts(S.K, shard_envs, S.MINIBATCHES, j))) for j in range(3)] * S.EPOCHS
        # ... and the job's row is not a shard's own
        own = dp.minibatch_rows_reference(stacked[:1].cpu().numpy(), trainers[0].hp.adv_eps)
        assert not np.array_equal(own, want)
    assert not torch.equal(trainers[0].policy.params, p0)
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. two ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_print_the_replays_checksum(torch_cuda, tmp_path):
    torch = torch_cuda
    import adv_norm_job_worker as W
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "adv_norm_job_worker.py"), str(r), "2", str(port), str(tmp_path)],
                              stdout=subprocess.PIPE, text=True) for r in range(2)]
    outs = []
    try:
        for p in procs:
            outs.append((p.communicate(timeout=300)[0], p.returncode))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [rc for _, rc in outs] == [0, 0], outs
    sums = [[ln for ln in out.splitlines() if ln.startswith("checksum ")] for out, _ in outs]
    assert all(len(s) == 1 for s in sums) and sums[0] == sums[1], sums
    rk = [torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r), weights_only=True) for r in range(2)]
    shard_envs = rk[0]["shard_envs"]
    assert shard_envs == rk[1]["shard_envs"] == [96, 96] and rk[0]["step"] == W.ROUNDS * S.EPOCHS * 3
    assert all(torch.equal(a, b) for a, b in zip(rk[0]["stats"], rk[1]["stats"]))
    assert not torch.equal(rk[0]["batches"][0]["obs"], rk[1]["batches"][0]["obs"])  # (the shards saw different envs)
    envs, trainers = _shard_trainers(torch, (64, 64))  # (the handles' sizes play no part in the halves: the batches are the ranks')
    for rnd in range(W.ROUNDS):
        bs = [{k: v.to("cuda:0") for k, v in rk[r]["batches"][rnd].items()} for r in range(2)]
        _, stats = S.replay_update(torch, trainers, bs, shard_envs)
        assert torch.equal(stats.cpu(), rk[0]["stats"][rnd]), rnd
    tr = trainers[1]
    assert "checksum %s" % S.checksum(tr.policy.params, tr.adam_mv, tr.minibatch_table()) == sums[0][0]
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. the trainer script on one rank
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_on_one_rank_leaves_the_single_handle_modes_parameters(torch_cuda, capsys, monkeypatch):
    torch = torch_cuda
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    mod = load_script("train/ppo_torch.py")
    line = ["--mode", "native", "--update", "native", "--envs", "256", "--horizon", "8", "--updates", "2"]
    capsys.readouterr()
    assert mod.main(line + ["--job-adv-norm", "minibatch"]) == 0
    sums = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("parameter checksum")]
    assert len(sums) == 1 and sums[0].startswith("parameter checksum after 16 Adam steps: "), sums
    a = mod.parse_args(line + ["--adv-norm", "minibatch"])
    _, details = mod.train(device="cuda:0", return_details=True, log=lambda *_: None, **{k: v for k, v in vars(a).items() if k != "gpus"})
    packed = torch.cat([p.reshape(-1) for p in details["params"]]).cpu().numpy()
    assert sums[0].endswith(": " + hashlib.sha256(packed.tobytes()).hexdigest())
    b = mod.parse_args(line)  # (and the rule matters: the batch mode's parameters are others)
    _, plain = mod.train(device="cuda:0", return_details=True, log=lambda *_: None, **{k: v for k, v in vars(b).items() if k != "gpus"})
    assert not np.array_equal(torch.cat([p.reshape(-1) for p in plain["params"]]).cpu().numpy(), packed)
