"""GPU checks of data-parallel native PPO (ship_sim_gym_amd/dp.py; ssg_ppo_adv_moments, ssg_ppo_set_adv_moments, ssg_ppo_apply_shards):
one rank is NativePPO bit for bit; the apply and the job-wide advantage statistics against their numpy restatements bit for bit; two
shards against the one batch they are the halves of (the f64 autograd gradient of the concatenated minibatch under the job-wide
normalisation); two rank processes against each other and against a sequential replay in this process; the trainer script on two
ranks.

Shapes: hidden 32, 2 layers, the env's own observation width (D = 32): P + 8 = 2252 is no multiple of 256.  K = 7 and 200 envs per
shard: a tail workgroup in GAE, chunks of 467 / 467 / 466 at 3 minibatches."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from dp_support import KLACC, f32 as _f32, layout as _layout
from gpu_support import ROOT, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, check_per_tensor, ref_grad, split_policy, synthetic_batch

pytestmark = pytest.mark.gpu

H, K, N_SHARD, EPOCHS, MINIBATCHES = 32, 7, 200, 2, 3
EXT = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)


def _vec(n=N_SHARD, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=16, env_id_base=base)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. one rank is NativePPO
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "ext", "split_ext"])
def test_one_rank_is_native_ppo_bitwise(torch_cuda, case):
    torch = torch_cuda
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO
    kw = {} if case == "plain" else EXT
    make = split_policy if case == "split_ext" else actor_critic_policy
    envs, pols, tr = [_vec(), _vec()], [], []
    for env, cls in zip(envs, (NativePPO, DataParallelPPO)):
        _, pol = make(torch, env.states_history, H, 2, "tanh", 3, seed=3)
        pols.append(pol)
        tr.append(cls(pol, env, perm_seed=11, **kw))
        env.reset_tensor()
    assert torch.equal(pols[0].params, pols[1].params) and (tr[1].rank, tr[1].world, tr[1].shard_envs) == (0, 1, [N_SHARD])
    p0 = pols[0].params.clone()
    for r in range(2):
        out = []
        for env, pol, t in zip(envs, pols, tr):
            b = dict(env.rollout_policy(pol, K, seed=5, step0=r * K))
            t.gae(b)
            head = t.adv_stats().clone()
            out.append((b, head, t.update(b, None, EPOCHS, MINIBATCHES, stats=True)))
        (b0, h0, s0), (b1, h1, s1) = out
        assert all(torch.equal(b0[k], b1[k]) for k in ("obs", "act", "logp", "adv", "ret")), r
        assert torch.equal(h0, h1), (r, h0, h1)
        assert s0.shape == s1.shape == (EPOCHS * 3, 4 if case == "plain" else 8) and torch.equal(s0, s1), (r, s0, s1)
        assert torch.equal(pols[0].params, pols[1].params) and torch.equal(tr[0].adam_mv, tr[1].adam_mv), r
        assert torch.equal(tr[0].kl_coef, tr[1].kl_coef) and (tr[0].step, tr[0].updates) == (tr[1].step, tr[1].updates) == (6 * (r + 1), r + 1)
    assert not torch.equal(pols[0].params, p0)
    if case != "plain":
        assert float(s0[:, 5].min()) > 0.0 and float(s0[0, 6]) > 0.0  # the norm and the coefficient were in use
    sd = tr[1].state_dict()
    assert (sd["world"], sd["rank"]) == (1, 0)
    tr[1].load_state_dict(sd)
    with pytest.raises(ValueError, match="world"):
        tr[1].load_state_dict(dict(sd, world=2))
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the apply against numpy
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trainer(torch_cuda):
    """One env, policy and DataParallelPPO (the extended loss) for the synthetic-row tests, which restore what they change."""
    from ship_sim_gym_amd.dp import DataParallelPPO
    env = _vec()
    _, pol = actor_critic_policy(torch_cuda, env.states_history, H, 2, "tanh", 3, seed=4)
    yield env, pol, DataParallelPPO(pol, env, perm_seed=1, **EXT)
    env.close()


def _rows(torch, W, P, seed, kl):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    rows = torch.randn((W, P + 8), generator=g, device="cuda:0") * 0.05  # (a combined norm of about 1.3: a clip at 0.5 bites)
    rows[:, P:] = 0.0
    rows[:, P: P + 4] = torch.rand((W, 4), generator=g, device="cuda:0")
    rows[:, P + 4] = torch.tensor(kl, device="cuda:0")
    return rows.contiguous()


APPLY_CASES = [
    # W, counts, max_grad_norm, first, last, klacc before, kl_target, the factor the adaptation must take
    ("clip coefficient 1", 3, (467, 466, 131), 1e6, True, False, 7.0, 0.01, 1.0),
    ("the clip bites", 3, (467, 466, 131), 0.5, True, False, 7.0, 0.01, 1.0),
    ("five rows, a later chunk", 5, (467, 466, 131, 1, 300), 0.5, False, False, 0.0625, 0.01, 1.0),
    ("last chunk, above 2 x target", 5, (467, 466, 131, 1, 300), 0.5, False, True, 0.0625, 0.01, 1.5),
    ("last chunk, below target / 2", 3, (467, 466, 131), 0.5, False, True, 0.0625, 0.2, 0.5),
    ("last chunk, between", 3, (467, 466, 131), 0.5, False, True, 0.0625, 0.03, 1.0),
    ("last chunk, no target", 3, (467, 466, 131), 0.5, True, True, 0.0625, 0.0, 1.0),
    ("no clip", 3, (467, 466, 131), 0.0, True, False, 0.0, 0.01, 1.0),
]


@pytest.mark.parametrize("what,W,counts,mgn,first,last,klacc0,target,factor", APPLY_CASES, ids=[c[0] for c in APPLY_CASES])
def test_apply_against_numpy_bitwise(torch_cuda, trainer, what, W, counts, mgn, first, last, klacc0, target, factor):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    env, pol, tr = trainer
    P = tr.n_params
    assert (P + 8) % 256 != 0
    rows = _rows(torch, W, P, 10 + W, [0.02, 0.05, 0.03, 0.04, 0.06][:W])
    g = torch.Generator(device="cuda:0").manual_seed(2)
    saved = pol.params.clone(), tr.adam_mv.clone(), tr.kl_coef.clone(), tr.step, tr.max_grad_norm, tr.kl_target, tr._since_first
    try:
        tr.adam_mv.copy_(torch.randn(2 * P, generator=g, device="cuda:0").abs() * 1e-3)
        tr.step, tr.max_grad_norm, tr.kl_target = 4, float(mgn), float(target)
        tr._since_first = 1  # (a later chunk is the second apply of its epoch)
        tr._ws(1, 1)
        tr.workspace[KLACC: KLACC + 4].view(torch.float32).fill_(klacc0)
        ref = dp.apply_reference(_f32(rows), counts, _f32(pol.params), _f32(tr.adam_mv), 5, tr.hp, max_grad_norm=mgn, ext=True,
                                 kl_coef=float(tr.kl_coef), klacc=klacc0, first_chunk=first, last_chunk=last,
                                 n_chunks=1 if first else 2, kl_target=target)
        st = tr.apply_rows(rows, counts, first, last, stats=True)
        torch.cuda.synchronize()
        assert tr.step == 5 and st.shape == (8,)
        if mgn > 0:  # the combined gradient and the workgroups' partials are in the workspace
            gv, part = _layout(P)
            got = _f32(tr.workspace[gv: gv + 4 * P].view(torch.float32))
            assert np.array_equal(got, ref["g"]), (what, np.abs(got - ref["g"]).max())
            nb = -(-(P + 8) // 256)
            total = 0.0
            for v in _f32(tr.workspace[part: part + 8 * nb].view(torch.float64)):
                total += float(v)
            assert np.float32(np.sqrt(total)) == ref["norm"] == _f32(st)[5]
            assert (ref["coef"] == 1.0) == (mgn > 1.0)
        assert np.array_equal(_f32(st), ref["stats"]), (what, _f32(st), ref["stats"])
        assert np.array_equal(_f32(tr.adam_mv), ref["adam_mv"]), (what, np.abs(_f32(tr.adam_mv) - ref["adam_mv"]).max())
        assert np.array_equal(_f32(pol.params), ref["params"]), (what, np.abs(_f32(pol.params) - ref["params"]).max())
        assert _f32(tr.workspace[KLACC: KLACC + 4].view(torch.float32))[0] == ref["klacc"]
        assert np.float32(float(tr.kl_coef)) == ref["kl_coef"] == np.float32(saved[2].item() * factor), (what, float(tr.kl_coef), ref["kl_coef"])
    finally:
        pol.params.copy_(saved[0]); tr.adam_mv.copy_(saved[1]); tr.kl_coef.copy_(saved[2])
        tr.step, tr.max_grad_norm, tr.kl_target, tr._since_first = saved[3:]


def test_running_kl_sum_survives_workspace_growth(torch_cuda, trainer):
    """A replay may meet a larger shard in the middle of an epoch: the grown workspace keeps the statistics and the running KL sum."""
    torch = torch_cuda
    env, pol, tr = trainer
    tr._ws(1, 1)
    tr.workspace[:16].view(torch.float32).copy_(torch.tensor([0.25, 1.5, 2.0 / 3.0, 0.0]))
    tr.workspace[KLACC: KLACC + 4].view(torch.float32).fill_(0.375)
    before = tr.workspace.numel()
    tr._ws(before, before)  # (more samples and a longer minibatch than the workspace serves)
    assert tr.workspace.numel() > before
    assert tr.workspace[:16].view(torch.float32).tolist()[:2] == [0.25, 1.5]
    assert float(tr.workspace[KLACC: KLACC + 4].view(torch.float32)[0]) == 0.375


def test_shards_that_make_different_chunk_counts_are_refused(torch_cuda, trainer):
    torch = torch_cuda
    env, pol, tr = trainer
    b = synthetic_batch(torch, pol, 1, N_SHARD, seed=2)
    tr.gae(b)
    saved, before = tr.shard_envs, (tr.step, tr.updates, pol.params.clone())
    try:
        assert tr.check_chunks(K, MINIBATCHES) == (3, [467])
        tr.shard_envs = [N_SHARD, 3]  # (K = 1, 3 minibatches: 200 samples make 3 chunks of 67, 3 samples 3 chunks of 1 — the same number)
        assert tr.check_chunks(1, 3) == (3, [67, 1])
        tr.shard_envs = [N_SHARD, 4]  # (4 samples make 2 chunks of 2)
        with pytest.raises(ValueError, match="the same number"):
            tr.update(b, torch.arange(N_SHARD, device="cuda:0")[None], 1, 3)
        tr.shard_envs = [N_SHARD + 1]
        with pytest.raises(ValueError, match="this rank's shard"):
            tr.update(b, torch.arange(N_SHARD, device="cuda:0")[None], 1, 3)
    finally:
        tr.shard_envs = saved
    assert (tr.step, tr.updates) == before[:2] and torch.equal(pol.params, before[2])  # (refused before anything ran)


def test_apply_plain_loss_against_numpy_bitwise(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.dp import DataParallelPPO
    env = _vec()
    _, pol = actor_critic_policy(torch, env.states_history, H, 2, "tanh", 3, seed=4)
    tr = DataParallelPPO(pol, env)
    P, counts = tr.n_params, (467, 466, 131)
    rows = _rows(torch, 3, P, 21, [0.0, 0.0, 0.0])
    ref = dp.apply_reference(_f32(rows), counts, _f32(pol.params), _f32(tr.adam_mv), 1, tr.hp)
    st = tr.apply_rows(rows, counts, True, True, stats=True)
    assert st.shape == (4,) and np.array_equal(_f32(st), ref["stats"][:4])
    assert np.array_equal(_f32(pol.params), ref["params"]) and np.array_equal(_f32(tr.adam_mv), ref["adam_mv"])
    assert np.array_equal(_f32(tr.adam_mv)[:P], np.float32(0.1) * ref["g"])  # (Adam's first step from zero moments: m = w1 * g)
    with pytest.raises(ValueError, match="rows must be"):
        tr.apply_rows(rows[:2], counts, True, True)
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the job-wide advantage statistics
# ------------------------------------------------------------------------------------------------------------------------------------
def test_set_moments_against_numpy_bitwise(torch_cuda, trainer):
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    env, pol, tr = trainer
    rows = torch.tensor([[12.5, 900.25, 1400.0, 0.0], [-3.75, 1100.5, 1400.0, 0.0], [0.125, 80.0, 131.0, 0.0]], dtype=torch.float64,
                        device="cuda:0")
    tr.set_moments(rows)
    got = _f32(tr.workspace[:16].view(torch.float32))
    assert np.array_equal(got, dp.moments_reference(_f32(rows), tr.hp.adv_eps)), got
    tr.set_moments(torch.tensor([[1.0, 1.0, 1.0, 0.0]], dtype=torch.float64, device="cuda:0"))  # fewer than 2 samples: refused
    got = _f32(tr.workspace[:16].view(torch.float32))
    assert np.isnan(got[:3]).all() and got[3] == 0
    with pytest.raises(ValueError, match="rows must be"):
        tr.set_moments(rows[:, :3])


@pytest.mark.parametrize("n", [N_SHARD, 600])
def test_one_row_round_trip_is_gaes_own_head(torch_cuda, trainer, n):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env, pol, tr = trainer
    b = synthetic_batch(torch, pol, K, n, seed=n)
    NativePPO.gae(tr, b)
    head = tr.workspace[:16].clone()
    m = tr.shard_moments(b)
    adv = b["adv"].double()
    assert float(m[2]) == K * n and float(m[3]) == 0.0
    assert abs(float(m[0]) - float(adv.sum())) <= 1e-12 * float(adv.abs().sum()) and abs(float(m[1]) - float((adv * adv).sum())) <= 1e-12 * float(m[1])
    tr.workspace[:16].zero_()
    tr.set_moments(m[None])
    assert torch.equal(tr.workspace[:16], head), (tr.workspace[:16].view(torch.float32), head.view(torch.float32))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. two shards against the one batch they are the halves of
# ------------------------------------------------------------------------------------------------------------------------------------
def test_two_shards_against_the_whole_batch(torch_cuda):
    """The gradient bound is the project's (ppo_reference.check_per_tensor): the combine adds at most W + 1 roundings per entry,
    under its 1e-6 * max term."""
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec()
    _, pol = actor_critic_policy(torch, env.states_history, H, 2, "tanh", 3, seed=6)
    terms = dict(vf_clip=0.2, kl_coef=1.0)
    tr = DataParallelPPO(pol, env, betas=(0.0, 0.999), **terms)  # (beta1 = 0: Adam's m is the combined gradient, exactly)
    whole = synthetic_batch(torch, pol, K, 2 * N_SHARD, seed=9)
    shards = [{k: (v[:, s].contiguous() if v.dim() > 1 else v[s].contiguous()) for k, v in whole.items()}
              for s in (slice(0, N_SHARD), slice(N_SHARD, 2 * N_SHARD))]
    moments = []
    for b in shards:
        NativePPO.gae(tr, b)
        moments.append(tr.shard_moments(b))
    own = tr.adv_stats().clone()  # (the second shard's own statistics: what a shard-local normalisation would use)
    tr.set_moments(torch.stack(moments))
    st = tr.adv_stats().clone()
    adv = torch.cat([b["adv"] for b in shards], dim=1)
    assert adv.numel() == 2800
    a64 = adv.double().reshape(-1)
    mean, stdp = np.float32(float(a64.mean())), np.float32(float(a64.std())) + np.float32(1e-8)
    got = _f32(st)
    assert abs(got[0] - mean) <= np.spacing(mean) and abs(got[1] - stdp) <= np.spacing(stdp), (got, mean, stdp)
    assert abs(got[2] - np.float32(1.0) / stdp) <= 2 * np.spacing(got[2])
    assert np.array_equal(_f32(tr.workspace[:16].view(torch.float32)), dp.moments_reference(_f32(torch.stack(moments)), 1e-8))
    assert not torch.equal(own, st)
    # one minibatch: 467 samples of shard 0 and 131 of shard 1, against the concatenated batch's autograd under the job's statistics
    whole["ret"] = torch.cat([b["ret"] for b in shards], dim=1).contiguous()
    g = torch.Generator(device="cuda:0").manual_seed(1)
    idx = [torch.randperm(K * N_SHARD, device="cuda:0", generator=g)[:m] for m in (467, 131)]
    rows = torch.stack([tr.local_row(b, i) for b, i in zip(shards, idx)])
    cat_idx = torch.cat([(i // N_SHARD) * (2 * N_SHARD) + s * N_SHARD + i % N_SHARD for s, i in enumerate(idx)])
    advn = (adv.reshape(-1) - st[0]) / st[1]
    kw = dict(vf_clip=0.2, kl_coef=1.0)
    g64 = ref_grad(torch, pol, whole, cat_idx, advn, torch.float64, **kw)[0]
    g32 = ref_grad(torch, pol, whole, cat_idx, advn, torch.float32, **kw)[0]
    P = tr.n_params
    ref = dp.apply_reference(_f32(rows), (467, 131), _f32(pol.params), _f32(tr.adam_mv), 1, tr.hp, ext=True, kl_coef=1.0)
    tr.apply_rows(rows, (467, 131), True, False)
    mine = tr.adam_mv[:P].clone()
    assert np.array_equal(_f32(mine), ref["g"])
    check_per_tensor(torch, pol, mine, g64, g32, "two shards", verbose=True)
    # what it catches: equal weights (a wrong weight) miss the bound's own scale by far
    wrong = 0.5 * rows[0, :P] + 0.5 * rows[1, :P]
    assert float((wrong.double() - g64).abs().max()) > 100 * float((mine.double() - g64).abs().max())
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. two ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_hold_the_same_bits_and_replay(torch_cuda, tmp_path):
    torch = torch_cuda
    import dp_worker as W
    from ship_sim_gym_amd.dp import DataParallelPPO, chunk_counts
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    port = _free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dp_worker.py"), str(r), "2", str(port), str(tmp_path)])
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
    for r in range(2):
        assert (rk[r]["backend"], rk[r]["world"], rk[r]["shard_envs"], rk[r]["env_id_base"]) == (want_backend, 2, [200, 200], 200 * r), rk[r]["backend"]
    # both ranks hold identical bits
    for k in ("params", "adam_mv", "kl_coef", "adv_stats"):
        assert torch.equal(rk[0][k], rk[1][k]), k
    assert all(torch.equal(a, b) for a, b in zip(rk[0]["stats"], rk[1]["stats"]))
    assert (rk[0]["step"], rk[0]["updates"]) == (rk[1]["step"], rk[1]["updates"]) == (W.ROUNDS * W.EPOCHS * 3, W.ROUNDS)
    assert not torch.equal(rk[0]["batches"][0]["obs"], rk[1]["batches"][0]["obs"])  # (the shards saw different envs)
    # the sequential replay: one policy from the same seed, the ranks' batches, torch.stack as the gather
    env = _vec()
    _, pol = actor_critic_policy(torch, env.states_history, W.HIDDEN, 2, "tanh", 3, seed=W.POLICY_SEED)
    tr = DataParallelPPO(pol, env, perm_seed=W.PERM_SEED, **W.TERMS)
    envs = rk[0]["shard_envs"]
    for rnd in range(W.ROUNDS):
        bs = [{k: v.to("cuda:0") for k, v in rk[r]["batches"][rnd].items()} for r in range(2)]
        moments = []
        for b in bs:
            NativePPO.gae(tr, b)
            moments.append(tr.shard_moments(b))
        tr.set_moments(torch.stack(moments))
        perms = []
        for r, b in enumerate(bs):
            tr.dist(b)  # (from the parameters on entry, as update() takes it)
            tr.member = r
            perms.append(tr.draw_perm(b, W.EPOCHS))
        chunk, n_chunks = chunk_split(W.K * envs[0], W.MINIBATCHES)
        rows_st = []
        for e in range(W.EPOCHS):
            for j in range(n_chunks):
                rows = torch.stack([tr.local_row(b, perms[r][e, j * chunk: (j + 1) * chunk]) for r, b in enumerate(bs)])
                rows_st.append(tr.apply_rows(rows, chunk_counts(W.K, envs, W.MINIBATCHES, j), j == 0,
                                             e == W.EPOCHS - 1 and j == n_chunks - 1, stats=True))
        tr.updates += 1
        assert torch.equal(torch.stack(rows_st).cpu(), rk[0]["stats"][rnd]), rnd
    assert torch.equal(pol.params.cpu(), rk[0]["params"]) and torch.equal(tr.adam_mv.cpu(), rk[0]["adam_mv"])
    assert torch.equal(tr.kl_coef.cpu(), rk[0]["kl_coef"]) and torch.equal(tr.adv_stats().cpu(), rk[0]["adv_stats"])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. the trainer script on two ranks
# ------------------------------------------------------------------------------------------------------------------------------------
def test_trainer_on_two_ranks(torch_cuda, tmp_path):
    from ship_sim_gym_amd import checkpoint
    path = os.path.join(str(tmp_path), "dp.ckpt")
    env = dict(os.environ, SSG_TRAIN_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--gpus", "2", "--envs", "256", "--horizon", "8",
                        "--updates", "2", "--mode", "native", "--update", "native", "--perm", "native", "--save", path],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    ckpt = checkpoint.load(path, require=("policy", "trainer"))
    assert (ckpt["trainer"]["world"], ckpt["trainer"]["rank"], ckpt["trainer"]["updates"]) == (2, 0, 2) and "env" not in ckpt
    sums = [ln for ln in r.stdout.splitlines() if ln.startswith("parameter checksum")]
    assert len(sums) == 2 and sums[0] == sums[1], sums
    # a refused flag ends the launcher itself, before any rank is started (every flag: tests/test_dp.py, in process)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "train", "ppo_torch.py"), "--gpus", "2", "--mode", "native", "--update", "native",
                          "--obs-filter"], capture_output=True, text=True, timeout=120, env=env)
    assert bad.returncode != 0 and "--obs-filter" in bad.stderr and "parameter checksum" not in bad.stdout
    # rank 0 alone logs, and what it logs is the job's: one line per update
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("update") and "mean return so far" in ln]) == 2
