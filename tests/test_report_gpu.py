"""The update report on the device (ssg_ppo_report / ssg_pop_report) against its numpy restatement, report.report_reference: bit for bit
on all 24 columns, NaN positions equal.  The batches are synthetic; the entry points take a batch width of their own (N), so one small
handle serves every single-policy shape."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, load_script
from gpu_support import torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, synthetic_batch

pytestmark = pytest.mark.gpu

BAD = -1  # SSG_ERR_BAD_ARG
SHAPES = ((1, 1), (5, 1), (3, 63), (4, 256), (3, 257), (2, 600), (2, 65537))  # (the last: 257 block partials, a finishing thread adds two)
STATS_SHAPES = (None, (1, 4), (7, 4), (1, 8), (7, 8))
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def env(torch_cuda):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    e = ShipVecEnv(1024, n_maps=4)
    yield e
    e.close()


def same_bits(got, want):
    """Two f64 arrays: NaN in the same places, every other entry bit for bit."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def make_batch(K, n, seed, mean=0.5, std=1.0):
    """numpy inputs of one policy: val / ret / adv f32 [K, n] and the post-update group (act, logp, logp_all_new)."""
    rng = np.random.default_rng(seed)
    ret = (mean + std * rng.standard_normal((K, n))).astype(np.float32)
    val = (ret + 0.5 * std * rng.standard_normal((K, n))).astype(np.float32)
    adv = rng.standard_normal((K, n)).astype(np.float32)
    act = rng.integers(0, 4, size=(K, n)).astype(np.int32)
    logp = (-1.0 + 0.2 * rng.standard_normal((K, n))).astype(np.float32)
    lpa = (logp[..., None] + 0.15 * rng.standard_normal((K, n, 4))).astype(np.float32)  # (d on both sides of clip 0.2's thresholds)
    return dict(val=val, ret=ret, adv=adv, act=act, logp=logp, lpa=lpa)


def make_stats(shape, seed):
    return None if shape is None else np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def dev(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def scratch_for(torch, n_envs, members=1):
    from ship_sim_gym_amd.report import scratch_nbytes
    return torch.full((scratch_nbytes(n_envs, members),), 0xFF, dtype=torch.uint8, device=DEV)  # (NaN bytes: every partial read was written)


def stream(torch):
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def ppo_report(torch, env, b, post, clip=0.2, stats=None, rc_only=False, **over):
    """ssg_ppo_report through ctypes on numpy inputs; `over` replaces arguments by name (the refusals).  Returns the record (numpy), or
    with rc_only (the return code, the out buffer)."""
    from ship_sim_gym_amd import _native as N
    K, n = b["val"].shape
    t = {k: dev(torch, b[k]) for k in ("val", "ret", "adv")}
    t.update({k: dev(torch, b[k]) if post else None for k in ("act", "logp", "lpa")})
    t["stats"] = dev(torch, stats)
    t["scratch"] = scratch_for(torch, n)
    t["out"] = torch.full((N.REPORT_COLS,), SENTINEL, dtype=torch.float64, device=DEV)
    a = dict(K=K, N=n, clip=clip, n_rows=0 if stats is None else stats.shape[0], n_cols=0 if stats is None else stats.shape[1],
             scratch_nbytes=t["scratch"].numel(), **{k: ptr(v) for k, v in t.items()})
    a.update(over)
    rc = N.lib().ssg_ppo_report(env._h, a["K"], a["N"], a["val"], a["ret"], a["adv"], a["act"], a["logp"], a["lpa"], a["clip"], a["stats"],
                                a["n_rows"], a["n_cols"], a["scratch"], a["scratch_nbytes"], a["out"], stream(torch))
    if rc_only:
        return rc, t["out"].cpu().numpy()
    N.check(rc, env._h, "ssg_ppo_report")
    return t["out"].cpu().numpy()


def reference(b, post, clip=0.2, stats=None, rows=None):
    from ship_sim_gym_amd.report import report_reference
    grp = dict(act=b["act"], logp=b["logp"], logp_all_new=b["lpa"]) if post else {}
    return report_reference(b["val"], b["ret"], b["adv"], clip=clip, stats=stats, rows=rows, **grp)


# ------------------------------------------------------------------------------------------------------------------------------------
# one policy
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("post", (False, True), ids=("plain", "post"))
@pytest.mark.parametrize("K,n", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_shapes_bit_for_bit(K, n, post, env, torch_cuda):
    b = make_batch(K, n, seed=K * 100003 + n)
    for i, shape in enumerate(STATS_SHAPES):
        stats = make_stats(shape, i)
        got, want = ppo_report(torch_cuda, env, b, post, stats=stats), reference(b, post, stats=stats)
        assert same_bits(got, want), (shape, got, want)
        assert got[0] == K * n and got[8] == float(post) and got[20] == (0 if shape is None else shape[0])
    if post and K * n > 100:
        assert 0.0 < got[11] < 1.0  # (samples on both sides of the thresholds)


@pytest.mark.parametrize("clip", (0.2, 0.01, 1.0))
def test_clip_decision_at_its_thresholds(clip, env, torch_cuda):
    """d exactly hi, exactly lo and one f32 ulp to either side of each: both inequalities are strict, the clipped samples are counted."""
    from ship_sim_gym_amd.report import clip_bounds
    lo, hi = clip_bounds(clip)
    K, n = 2, 64
    b = make_batch(K, n, seed=3)
    b["logp"][:] = 0.0  # d = logp_all_new[act] - 0: exactly the planted values
    b["lpa"][:] = 0.0
    inf = np.float32(np.inf)
    planted = [(hi, False), (np.nextafter(hi, inf), True), (np.nextafter(hi, -inf), False)]
    if np.isfinite(lo):
        planted += [(lo, False), (np.nextafter(lo, -inf), True), (np.nextafter(lo, inf), False)]
    else:
        planted += [(np.float32(-100.0), False), (np.finfo(np.float32).min, False)]  # (clip >= 1: nothing is below lo)
    clipped = 0
    for j, (d, is_clipped) in enumerate(planted):
        for t in range(K):
            e = 7 * j + t
            b["lpa"][t, e, b["act"][t, e]] = d
            clipped += int(is_clipped)
    got = ppo_report(torch_cuda, env, b, True, clip=clip)
    assert got[11] == clipped / float(K * n) and clipped == (4 if np.isfinite(lo) else 2)
    assert same_bits(got, reference(b, True, clip=clip))


def test_value_edges(env, torch_cuda):
    K, n = 3, 300
    b = make_batch(K, n, seed=8)
    b["val"] = b["ret"].copy()  # a perfect value network
    got = ppo_report(torch_cuda, env, b, False)
    assert got[3] == 0.0 and got[4] == 0.0 and got[5] == 1.0 and same_bits(got, reference(b, False))
    b = make_batch(K, n, seed=9)
    b["val"][:] = 0.25  # a constant value network explains nothing
    got = ppo_report(torch_cuda, env, b, False)
    assert same_bits(got, reference(b, False)) and abs(got[5]) < 1e-12 and got[6] == 0.25
    b = make_batch(K, n, seed=10)
    b["ret"][:] = -1.5  # constant returns: no variance to explain
    got = ppo_report(torch_cuda, env, b, False)
    assert got[2] == 0.0 and np.isnan(got[5]) and same_bits(got, reference(b, False))
    b = make_batch(K, n, seed=11, mean=1e3, std=1.0)
    got = ppo_report(torch_cuda, env, b, True)
    assert same_bits(got, reference(b, True))
    r = b["ret"].astype(np.float64)
    np.testing.assert_allclose(got[2], np.var(r), rtol=1e-8)  # (1 + mean^2 / var = 1e6 times 2^-53, and the summation depth)


def test_two_calls_and_two_streams_give_the_same_record(env, torch_cuda):
    torch = torch_cuda
    b = make_batch(3, 700, seed=12)
    stats = make_stats((7, 8), 1)
    first = ppo_report(torch, env, b, True, stats=stats)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        second = ppo_report(torch, env, b, True, stats=stats)
    assert same_bits(first, second)


def test_refusals_launch_nothing(env, torch_cuda):
    torch = torch_cuda
    b = make_batch(2, 300, seed=13)
    stats = make_stats((3, 4), 2)
    small = scratch_for(torch, 300)
    cases = [("NULL value", dict(val=None)), ("NULL ret", dict(ret=None)), ("NULL adv", dict(adv=None)), ("NULL out", dict(out=None)),
             ("NULL scratch", dict(scratch=None)), ("K < 1", dict(K=0)), ("N < 1", dict(N=0)), ("n_cols 5", dict(n_cols=5)),
             ("n_cols 0", dict(n_cols=0)), ("n_rows 0", dict(n_rows=0)), ("act alone missing", dict(act=None)),
             ("logp alone missing", dict(logp=None)), ("logp_all_new alone missing", dict(lpa=None)),
             ("only act", dict(logp=None, lpa=None)), ("only logp_all_new", dict(act=None, logp=None)),
             ("clip 0 with the post group", dict(clip=0.0)),
             ("scratch too small", dict(scratch_nbytes=2 * 9 * 8 - 1)),
             ("scratch misaligned", dict(scratch=C.c_void_p(small.data_ptr() + 8)))]
    for what, over in cases:
        if over.get("out", 1) is None:
            rc, _ = ppo_report(torch, env, b, True, stats=stats, rc_only=True, **over)
            assert rc == BAD, what
            continue
        rc, out = ppo_report(torch, env, b, True, stats=stats, rc_only=True, **over)
        assert rc == BAD and (out == SENTINEL).all(), what
    rc, out = ppo_report(torch, env, b, True, stats=stats, rc_only=True, scratch_nbytes=2 * 9 * 8)  # (exactly what 300 envs need)
    assert rc == 0 and same_bits(out, reference(b, True, stats=stats))


# ------------------------------------------------------------------------------------------------------------------------------------
# populations
# ------------------------------------------------------------------------------------------------------------------------------------
def pop_report(torch, env, P, b, post, clips=None, stats=None, rows=None, rc_only=False, **over):
    """ssg_pop_report through ctypes on [K, n_envs] numpy inputs."""
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.report import clip_bounds
    K, n = b["val"].shape
    t = {k: dev(torch, b[k]) for k in ("val", "ret", "adv")}
    t.update({k: dev(torch, b[k]) if post else None for k in ("act", "logp", "lpa")})
    t["bounds"] = dev(torch, np.array([clip_bounds(c) for c in clips], dtype=np.float32)) if post else None
    t["stats"], t["rows"] = dev(torch, stats), dev(torch, None if rows is None else np.asarray(rows, dtype=np.int32))
    t["scratch"] = scratch_for(torch, n, min(max(P, 1), 4))  # (a refused member count still gets a real scratch)
    t["out"] = torch.full((max(P, 1), N.REPORT_COLS), SENTINEL, dtype=torch.float64, device=DEV)
    a = dict(P=P, K=K, rows_max=0 if stats is None else stats.shape[1], n_cols=0 if stats is None else stats.shape[2],
             scratch_nbytes=t["scratch"].numel(), **{k: ptr(v) for k, v in t.items()})
    a.update(over)
    rc = N.lib().ssg_pop_report(env._h, a["P"], a["K"], a["val"], a["ret"], a["adv"], a["act"], a["logp"], a["lpa"], a["bounds"], a["stats"],
                                a["rows_max"], a["n_cols"], a["rows"], a["scratch"], a["scratch_nbytes"], a["out"], stream(torch))
    if rc_only:
        return rc, t["out"].cpu().numpy()
    N.check(rc, env._h, "ssg_pop_report")
    return t["out"].cpu().numpy()


def member_batch(b, o, n):
    return {k: np.ascontiguousarray(v[:, o:o + n]) for k, v in b.items()}


def test_population_equal_slices_bound_and_unbound(env, torch_cuda):
    torch = torch_cuda
    P, K, clips = 4, 3, (0.1, 0.2, 0.3, 1.5)
    b = make_batch(K, 1024, seed=21)
    stats = make_stats((P, 7, 8), 3)
    unbound = pop_report(torch, env, P, b, True, clips, stats)
    env.set_population_slices([256] * P)
    try:
        bound = pop_report(torch, env, P, b, True, clips, stats)
    finally:
        env.set_population_slices(None)
    assert same_bits(unbound, bound)
    for m in range(P):
        mb = member_batch(b, 256 * m, 256)
        assert same_bits(unbound[m], ppo_report(torch, env, mb, True, clip=clips[m], stats=stats[m])), m
        assert same_bits(unbound[m], reference(mb, True, clip=clips[m], stats=stats[m])), m


@pytest.mark.parametrize("post", (False, True), ids=("plain", "post"))
def test_population_unequal_slices_own_clips_and_row_counts(post, env, torch_cuda):
    torch = torch_cuda
    sizes, K, clips, rows = (300, 3, 131, 590), 3, (0.1, 0.2, 0.3, 1.0), (5, 1, 7, 3)
    b = make_batch(K, 1024, seed=22)
    stats = make_stats((4, 7, 4), 4)
    for m, r in enumerate(rows):
        stats[m, r:] = np.nan  # rows past a member's count are never read
    env.set_population_slices(list(sizes))
    try:
        got = pop_report(torch, env, 4, b, post, clips, stats, rows)
        all_rows = pop_report(torch, env, 4, b, post, clips, np.nan_to_num(stats), None)  # dev_rows NULL: rows_max for everyone
    finally:
        env.set_population_slices(None)
    o = 0
    for m, n in enumerate(sizes):
        mb = member_batch(b, o, n)
        assert same_bits(got[m], ppo_report(torch, env, mb, post, clip=clips[m], stats=stats[m, :rows[m]])), m
        assert same_bits(got[m], reference(mb, post, clip=clips[m], stats=stats[m], rows=rows[m])), m
        assert same_bits(all_rows[m], reference(mb, post, clip=clips[m], stats=np.nan_to_num(stats[m]))), m
        assert got[m][0] == K * n and got[m][20] == rows[m] and all_rows[m][20] == 7
        o += n


def test_population_refusals_launch_nothing(env, torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    b = make_batch(2, 1024, seed=23)
    clips = (0.2,) * 4
    for what, P, over in (("no members", 0, {}), ("too many members", N.POP_MAX_MEMBERS + 1, {}), ("1024 % 3 != 0, unbound", 3, {}),
                          ("NULL bounds with the post group", 4, dict(bounds=None)), ("NULL out", 4, dict(out=None)),
                          ("K < 1", 4, dict(K=0)), ("scratch too small", 4, dict(scratch_nbytes=4 * 9 * 8 - 1))):
        rc, out = pop_report(torch, env, P, b, True, clips[:max(P, 1)] if P <= 4 else clips, rc_only=True, **over)
        assert rc == BAD and (over.get("out", 1) is None or (out == SENTINEL).all()), what
    env.set_population_slices([512, 512])
    try:
        rc, out = pop_report(torch, env, 4, b, True, clips, rc_only=True)
    finally:
        env.set_population_slices(None)
    assert rc == BAD and (out == SENTINEL).all()  # slices bound for another member count


# ------------------------------------------------------------------------------------------------------------------------------------
# the trainers' objects
# ------------------------------------------------------------------------------------------------------------------------------------
def test_native_ppo_report_is_pure_and_matches_the_reference(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.report import REPORT_FIELDS
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    K, n = 4, 300
    env = ShipVecEnv(n, n_maps=4)
    try:
        _, pol = actor_critic_policy(torch, env.states_history, seed=5)
        ppo = NativePPO(pol, env, kl_coef=0.5, kl_target=0.01, clip=0.15)
        batch = synthetic_batch(torch, pol, K, n, 31)
        ppo.gae(batch)
        g = torch.Generator(device=DEV).manual_seed(1)
        perm = torch.stack([torch.randperm(K * n, device=DEV, generator=g) for _ in range(2)])
        st = ppo.update(batch, perm, 2, 3, stats=True)
        assert tuple(st.shape) == (6, 8)
        before = {k: v.clone() for k, v in batch.items()}
        state = [t.clone() for t in (pol.params, ppo.adam_mv, ppo.workspace, ppo.kl_coef, st)]
        rec = ppo.report(batch, stats=st, post=True)
        again = ppo.report(batch, stats=st, post=True)
        assert set(batch) == set(before) and all(torch.equal(batch[k], before[k]) for k in before)  # logp_all: the acting policy's, still
        assert all(torch.equal(a, b) for a, b in zip(state, (pol.params, ppo.adam_mv, ppo.workspace, ppo.kl_coef, st)))
        row = np.array([rec[k] for k in REPORT_FIELDS])
        assert same_bits(row, np.array([again[k] for k in REPORT_FIELDS]))
        new = ppo.dist({"obs": batch["obs"]})
        assert not torch.equal(new, batch["logp_all"])
        want = reference(dict(val=batch["val"].cpu().numpy(), ret=batch["ret"].cpu().numpy(), adv=batch["adv"].cpu().numpy(),
                              act=batch["act"].cpu().numpy(), logp=batch["logp"].cpu().numpy(), lpa=new.cpu().numpy()), True, clip=0.15,
                         stats=st.cpu().numpy())
        assert same_bits(row, want)
        assert rec["post"] == 1.0 and rec["stats_rows"] == 6 and rec["approxkl_ppo2"] > 0.0
        assert (rec["lr"], rec["clip"], rec["step"], rec["updates"]) == (3e-4, 0.15, 6, 1)
        assert rec["kl_coef_now"] == float(ppo.kl_coef.item()) and all(isinstance(rec[k], float) for k in REPORT_FIELDS)
        d = ppo.report_device(batch)
        assert d.dtype == torch.float64 and tuple(d.shape) == (24,) and d.is_cuda
        plain = d.cpu().numpy()
        assert same_bits(plain[:8], want[:8]) and not plain[8:].any()
    finally:
        env.close()


@pytest.mark.parametrize("sizes", ((64, 64, 64), (100, 3, 89)), ids=("equal", "unequal"))
def test_population_ppo_report_on_member_schedules(sizes, torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.report import REPORT_FIELDS
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    K, P, N_ = 4, len(sizes), sum(sizes)
    env = ShipVecEnv(N_, n_maps=4)
    try:
        if len(set(sizes)) > 1:
            env.set_population_slices(list(sizes))
        pop = NativePopulation([actor_critic_policy(torch, env.states_history, seed=40 + m)[1] for m in range(P)])
        clips = [0.1, 0.2, 0.3]
        ppo = PopulationPPO(pop, env, clip=clips, perm_seed=9)
        env.reset_tensor()
        batch = dict(env.rollout_population(pop, K, seed=3))
        ppo.gae(batch)
        st = ppo.update(batch, None, [1, 3, 2], [2, 1, 2], stats=True)  # member m takes 2, 3 and 4 steps of its own
        assert tuple(st.shape) == (P, 4, 4)
        keys = set(batch)
        rec = ppo.report(batch, stats=st, post=True)
        assert set(batch) == keys
        new = ppo.dist({"rew": batch["rew"], "obs": batch["obs"]}).cpu().numpy()
        host = {k: batch[k].cpu().numpy() for k in ("val", "ret", "adv", "act", "logp")}
        o = 0
        for m, n in enumerate(sizes):
            mb = {k: np.ascontiguousarray(v[:, o:o + n]) for k, v in host.items()}
            mb["lpa"] = np.ascontiguousarray(new[:, o:o + n])
            want = reference(mb, True, clip=clips[m], stats=st[m].cpu().numpy(), rows=(2, 3, 4)[m])
            assert same_bits(np.array([rec[k][m] for k in REPORT_FIELDS]), want), m
            o += n
        assert rec["stats_rows"].tolist() == [2, 3, 4] and rec["clip"].tolist() == clips and rec["step"].tolist() == [2, 3, 4]
        assert tuple(ppo.report_device(batch).shape) == (P, 24)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------------------------------------------
def test_single_policy_trainer_reports_and_changes_nothing(tmp_path, torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.report import read_progress
    single = load_script("train/ppo_torch.py")
    kw = dict(envs=256, updates=3, horizon=8, mode="native", update="native", return_details=True, seed=4)
    lines = []
    plain_hist, plain = single.train(log=lambda *a: None, **kw)
    path = tmp_path / "progress.csv"
    hist, det = single.train(log=lines.append, report=True, report_kl=True, progress=str(path), **kw)
    assert hist == plain_hist
    assert all(torch.equal(a, b) for a, b in zip(det["params"], plain["params"])) and torch.equal(det["env_state"], plain["env_state"])
    cols = read_progress(path)
    assert cols["update"].tolist() == [0, 1, 2] and cols["member"].tolist() == [0, 0, 0] and cols["timesteps"].tolist() == [2048, 4096, 6144]
    assert (cols["n"] == 2048).all() and (cols["stats_rows"] == 8).all() and (cols["post"] == 1).all()
    ev = cols["explained_variance"]
    assert (np.isnan(ev) | (np.isfinite(ev) & (ev <= 1.0))).all()
    for k in ("policy_loss", "value_loss", "entropy", "clip_fraction_minibatch", "approx_kl", "approxkl_ppo2", "clip_fraction", "lr", "clip"):
        assert np.isfinite(cols[k]).all(), k
    assert (cols["entropy"] > 0).all() and (cols["approxkl_ppo2"] > 0).all() and (cols["lr"] == 3e-4).all() and (cols["clip"] == 0.2).all()
    assert sum("report: explained variance" in ln for ln in lines) == 3


def test_population_trainer_writes_a_row_per_member(tmp_path, torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.report import read_progress
    pbt = load_script("train/pbt_native.py")
    kw = dict(members=2, envs_per_member=64, updates=2, horizon=8, perturb_every=1, seed=2, return_details=True)
    _, plain = pbt.train(log=lambda *a: None, **kw)
    lines = []
    path = tmp_path / "progress.csv"
    _, det = pbt.train(log=lines.append, progress=str(path), **kw)
    assert torch.equal(det["params"], plain["params"]) and torch.equal(det["env_state"], plain["env_state"])
    cols = read_progress(path)
    assert cols["update"].tolist() == [1, 1, 2, 2] and cols["member"].tolist() == [0, 1, 0, 1] and cols["timesteps"].tolist() == [1024, 1024, 2048, 2048]
    assert (cols["n"] == 512).all() and (cols["post"] == 0).all() and np.isfinite(cols["policy_loss"]).all()
    assert sum("  report\n" in ln for ln in lines) == 2


def test_a_resumed_run_leaves_the_uninterrupted_runs_progress_file(tmp_path, torch_cuda):
    from ship_sim_gym_amd.report import read_progress
    single = load_script("train/ppo_torch.py")
    kw = dict(envs=256, horizon=8, mode="native", update="native", seed=4, log=lambda *a: None, report_kl=True)
    whole, cut, ckpt = tmp_path / "whole.csv", tmp_path / "cut.csv", tmp_path / "run.ckpt"
    single.train(updates=4, progress=str(whole), **kw)
    single.train(updates=2, progress=str(cut), save=str(ckpt), **kw)
    single.train(updates=3, progress=str(cut), **kw)  # the run goes on past its checkpoint and is killed: a row of update 2 is there
    assert read_progress(cut)["update"].tolist() == [0, 1, 2]
    single.train(updates=4, progress=str(cut), resume=str(ckpt), **kw)
    a, b = read_progress(whole), read_progress(cut)
    assert a["update"].tolist() == [0, 1, 2, 3] == b["update"].tolist()
    for k in a:
        if k != "t":
            assert np.array_equal(a[k], b[k], equal_nan=True), k
