"""Data parallel, host side: the numpy restatements of ssg_ppo_apply_shards / ssg_ppo_set_adv_moments are self-consistent, every
refusal of the three entry points that needs no device comes back as SSG_ERR_BAD_ARG (a handle with a made-up bound blob and made-up
device addresses, as in test_update_refusals.py: nothing is ever touched), and the gather works without a process group.  No GPU."""
import ctypes as C

import numpy as np
import pytest

Q = 0x30000  # a plausible device address (256-byte aligned; never dereferenced on the host)
BIG = 1 << 40
HP = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8)


# ------------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------------
def test_one_shard_is_the_identity_on_the_gradient():
    from ship_sim_gym_amd import dp
    rng = np.random.RandomState(3)
    P = 301
    row = rng.randn(1, P + 8).astype(np.float32)
    params, mv = rng.randn(P).astype(np.float32), np.abs(rng.randn(2 * P)).astype(np.float32)
    out = dp.apply_reference(row, [467], params, mv, 3, HP)
    assert dp.shard_weights([467]).tolist() == [1.0]
    assert np.array_equal(out["g"], row[0, :P]) and np.array_equal(out["stats"][:4], row[0, P:P + 4])
    assert out["norm"] == 0 and out["coef"] == 1 and list(out["stats"][4:]) == [0, 0, 0, 0]  # (the plain loss has no KL column)
    ext = dp.apply_reference(row, [467], params, mv, 3, HP, ext=True)
    assert np.array_equal(ext["stats"][:5], row[0, P:P + 5]) and list(ext["stats"][5:]) == [0, 0, 0] and np.array_equal(ext["params"], out["params"])
    p2, mv2 = dp.adam_reference(row[0, :P], params, mv, 3, HP)
    assert np.array_equal(out["params"], p2) and np.array_equal(out["adam_mv"], mv2)
    assert not np.array_equal(p2, params)
    # the clip: its norm is the f64 root of the sum of squares to f32 rounding, and a coefficient of 1 changes nothing
    big = dp.apply_reference(row, [467], params, mv, 3, HP, max_grad_norm=1e9, ext=True)
    assert big["coef"] == 1 and np.array_equal(big["params"], p2)
    assert abs(float(big["norm"]) - np.sqrt(np.sum(row[0, :P].astype(np.float64) ** 2))) <= 1e-6 * float(big["norm"])
    bite = dp.apply_reference(row, [467], params, mv, 3, HP, max_grad_norm=0.5, ext=True)
    assert bite["coef"] < 1 and bite["stats"][5] == bite["norm"] and not np.array_equal(bite["params"], p2)


def test_weights_and_combination():
    from ship_sim_gym_amd import dp
    w = dp.shard_weights([467, 466, 131])
    assert w.dtype == np.float32 and [float(v) for v in w] == [float(np.float32(c / 1064.0)) for c in (467, 466, 131)]
    rng = np.random.RandomState(4)
    rows = rng.randn(3, 40 + 8).astype(np.float32)
    out = dp.apply_reference(rows, [467, 466, 131], np.zeros(40, np.float32), np.zeros(80, np.float32), 1, HP)
    exact = (w.astype(np.float64)[:, None] * rows.astype(np.float64)).sum(0)
    assert np.max(np.abs(out["g"] - exact[:40])) <= 4 * 2.0 ** -24 * np.max(np.abs(rows))  # W + 1 roundings per entry
    # equal rows combine to (nearly) themselves: the weights sum to 1 within rounding
    same = dp.apply_reference(np.repeat(rows[:1], 3, 0), [10, 10, 10], np.zeros(40, np.float32), np.zeros(80, np.float32), 1, HP)
    assert np.max(np.abs(same["g"] - rows[0, :40])) <= 4 * 2.0 ** -24 * np.max(np.abs(rows[0]))


def test_kl_sum_and_adaptation():
    from ship_sim_gym_amd import dp
    P = 16
    rows = np.zeros((2, P + 8), dtype=np.float32)
    rows[:, P + 4] = (0.03, 0.05)  # the shards' mean KL
    z, zz = np.zeros(P, np.float32), np.zeros(2 * P, np.float32)
    a = dp.apply_reference(rows, [8, 8], z, zz, 1, HP, ext=True, kl_coef=1.0, first_chunk=True)
    kl = np.float32(np.float32(0.5) * np.float32(0.03)) + np.float32(np.float32(0.5) * np.float32(0.05))
    assert a["klacc"] == kl and a["stats"][6] == 1.0 and a["kl_coef"] == 1.0
    b = dp.apply_reference(rows, [8, 8], z, zz, 2, HP, ext=True, kl_coef=1.0, klacc=a["klacc"], first_chunk=False, last_chunk=True,
                           n_chunks=2, kl_target=0.01)
    assert b["klacc"] == np.float32(kl + kl) and b["kl_coef"] == np.float32(1.5)  # mean 0.04 > 2 x 0.01
    c = dp.apply_reference(rows, [8, 8], z, zz, 2, HP, ext=True, kl_coef=1.0, klacc=a["klacc"], first_chunk=False, last_chunk=True,
                           n_chunks=2, kl_target=0.1)
    assert c["kl_coef"] == np.float32(0.5)                                         # mean 0.04 < 0.5 x 0.1
    d = dp.apply_reference(rows, [8, 8], z, zz, 2, HP, ext=True, kl_coef=1.0, klacc=a["klacc"], first_chunk=False, last_chunk=True,
                           n_chunks=2, kl_target=0.04)
    assert d["kl_coef"] == np.float32(1.0)
    e = dp.apply_reference(rows, [8, 8], z, zz, 2, HP, ext=True, kl_coef=1.0, klacc=5.0, first_chunk=True, last_chunk=False, kl_target=0.01)
    assert e["klacc"] == kl and e["kl_coef"] == 1.0                                # first_chunk restarts the sum; no adaptation


def test_moments_of_one_row_are_the_gae_statistics():
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.ppo import _tree256, gae_boot_reference
    rng = np.random.RandomState(5)
    K, n = 7, 200
    rew, done = rng.randn(K, n), (rng.rand(K, n) < 0.1).astype(np.uint8)
    val, last = rng.randn(K, n).astype(np.float32), rng.randn(n).astype(np.float32)
    adv, _, stats = gae_boot_reference(rew, done, val, last, np.zeros((K, n), np.float32))
    a = adv.astype(np.float64)
    # S and Q as the device forms them for one 256-env block: per env the sums in the walk's order (t = K-1 .. 0), then the halving tree
    cols = np.zeros((256, 2))
    for t in range(K - 1, -1, -1):
        cols[:n, 0] += a[t]
        cols[:n, 1] += a[t] * a[t]
    S, Q2 = _tree256(cols)
    row = dp.moments_reference([[S, Q2, K * n, 0.0]], 1e-8)
    assert row.dtype == np.float32 and np.array_equal(row, stats)
    # two halves give the whole
    h = n // 2
    parts = [[a[:, :h].sum(), (a[:, :h] ** 2).sum(), K * h, 0.0], [a[:, h:].sum(), (a[:, h:] ** 2).sum(), K * (n - h), 0.0]]
    both = dp.moments_reference(parts, 1e-8)
    assert np.all(np.abs(both[:3] - stats[:3]) <= np.spacing(np.abs(stats[:3])))
    assert abs(float(both[0]) - a.mean()) <= np.spacing(np.float32(a.mean())) and abs(float(both[1]) - a.std(ddof=1)) <= 2e-7 * a.std(ddof=1)
    assert np.isnan(dp.moments_reference([[1.0, 1.0, 1.0, 0.0]], 1e-8)[:3]).all()


@pytest.mark.parametrize("W,P", [(3, 5), (64, 3)])
def test_references_against_exact_rational_arithmetic(W, P):
    """apply_reference's combine and moments_reference against fractions.Fraction, so that the GPU modules' bitwise agreement with
    them is agreement with the arithmetic and not with a shared mistake.

    The combine, u = 2^-24: entry p is W products and W - 1 sums, 2W - 1 roundings, and every weight carries its own rounding (the f64
    quotient rounded to f32).  A term w_r row_r[p] passes through at most W + 1 of them (its weight, its product, the W - 1 sums), so
    |g - exact| <= ((1 + u')^(W + 1) - 1) sum_r |w_r row_r[p]|, u' = u (1 + 2^-29) for the weight's double rounding — below the bound
    asserted here, (2W - 1) u sum_r |w_r row_r[p]| for the entry's roundings plus u sum_r |w_r row_r[p]| for the weights', for every
    W >= 2.  (No product here is subnormal.)

    The mean: with row sums that are exact in f64 it is the exact S / n rounded to f64 once, then to f32 once."""
    from fractions import Fraction as Fr
    from ship_sim_gym_amd import dp
    rng = np.random.RandomState(100 * W + P)
    counts = [int(c) for c in rng.randint(1, 2000, W)]
    rows = (rng.randn(W, P + 8) * np.exp(rng.randn(W, 1))).astype(np.float32)
    out = dp.apply_reference(rows, counts, np.zeros(P, np.float32), np.zeros(2 * P, np.float32), 1, HP, ext=True, kl_coef=1.0)
    got = np.concatenate([out["g"], out["stats"][:5]])
    total, u, worst = sum(counts), Fr(1, 2 ** 24), Fr(0)
    assert W >= 2 and (1 + u * (1 + Fr(1, 2 ** 29))) ** (W + 1) - 1 <= 2 * W * u
    for p in range(P + 5):
        terms = [Fr(c, total) * Fr(float(rows[r, p])) for r, c in enumerate(counts)]
        err, bound = abs(Fr(float(got[p])) - sum(terms)), 2 * W * u * sum(abs(t) for t in terms)
        assert err <= bound, (p, float(err), float(bound))
        worst = max(worst, err / bound)
    print("combine W=%d: worst |g - exact| / bound %.3f" % (W, float(worst)))
    assert worst > 0  # (the f32 combine is not exact: the bound is not met by accident)
    w = dp.shard_weights(counts)
    assert all(abs(Fr(float(w[r])) - Fr(c, total)) <= u * Fr(c, total) for r, c in enumerate(counts))
    # the moments: S_r multiples of 2^-10 below 2^20, Q_r likewise, integer n_r — every f64 sum of W of them is exact
    m = np.zeros((W, 4))
    m[:, 2] = rng.randint(1, 5000, W)
    m[:, 0] = np.round(rng.randn(W) * m[:, 2] * 1024) / 1024
    m[:, 1] = np.round((m[:, 0] ** 2 / m[:, 2] + m[:, 2] * (0.5 + rng.rand(W))) * 1024) / 1024
    S, Q2, n = (sum(Fr(float(v)) for v in m[:, c]) for c in range(3))
    assert all(float(x) == float(np.sum(m[:, c])) and Fr(float(x)) == x for c, x in enumerate((S, Q2, n)))
    row = dp.moments_reference(m, 1e-8)
    mean = S / n
    assert row[0] == np.float32(float(mean))  # (int / int true division is correctly rounded: one f64 rounding, then one f32)
    assert abs(Fr(float(row[0])) - mean) <= (u + Fr(1, 2 ** 53)) * (1 + u) * abs(mean)
    var = (Q2 - S * mean) / (n - 1)
    assert var > 0 and abs(float(row[1]) - float(var) ** 0.5) <= 4 * float(u) * float(var) ** 0.5 and row[2] == np.float32(1.0) / row[1]


def test_support_restatements_agree_with_the_references():
    """tests/dp_support.py's sums (what the GPU module compares the workspace's partials with) against the references that form the
    same sums inside: apply_reference's norm, gae_boot_reference's statistics past one trip of the strided loop."""
    import dp_support as S
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.ppo import _tree256, gae_boot_reference
    rng = np.random.RandomState(9)
    P = 600
    rows = rng.randn(2, P + 8).astype(np.float32)
    out = dp.apply_reference(rows, [3, 5], np.zeros(P, np.float32), np.zeros(2 * P, np.float32), 1, HP, max_grad_norm=0.5, ext=True)
    part = S.square_partials(out["g"], P + 8)
    assert part.shape == (3,) and S.norm_of_partials(part) == out["norm"]
    tail = float(np.sum(out["g"][512:].astype(np.float64) ** 2))  # (the third workgroup: 88 entries, then zeros)
    assert abs(part[2] - tail) <= 88 * 2.0 ** -53 * tail
    x = rng.randn(4, 256)
    assert np.array_equal(S.trees256(x), [_tree256(r.copy().reshape(256, 1))[0] for r in x])
    K, n = 1, 65537
    rew, done = rng.randn(K, n), (rng.rand(K, n) < 0.1).astype(np.uint8)
    val, last = rng.randn(K, n).astype(np.float32), rng.randn(n).astype(np.float32)
    adv, _, stats = gae_boot_reference(rew, done, val, last, np.zeros((K, n), np.float32))
    a = np.zeros(257 * 256)
    a[:n] = adv[0].astype(np.float64)
    gae_part = np.stack([S.trees256(a), S.trees256(a * a)], axis=1)  # K = 1: a workgroup's partial is the tree over its 256 envs
    s, q, trips = S.readd_partials(gae_part)
    assert trips == 2 and np.array_equal(dp.moments_reference([[s, q, float(n), 0.0]], 1e-8), stats)
    assert S.bits(np.array([-0.0, 0.0], np.float32)).tolist() == [0x80000000, 0]
    with pytest.raises(AssertionError):
        S.assert_bits(np.array([-0.0], np.float32), np.array([0.0], np.float32), "signed zero")
    S.assert_bits(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32), "NaN payloads", nan_ok=True)


def test_chunk_counts():
    from ship_sim_gym_amd import dp
    assert dp.shard_chunks(7, [200, 200], 3) == [(467, 3), (467, 3)]
    assert [dp.chunk_counts(7, [200, 200], 3, j) for j in range(3)] == [[467, 467], [467, 467], [466, 466]]
    assert dp.shard_chunks(1, [4, 3], 3) == [(2, 2), (1, 3)]  # different numbers of chunks: what DataParallelPPO refuses


def test_all_gather_rows_without_a_process_group():
    import torch
    from ship_sim_gym_amd import sharding
    t = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    out = sharding.all_gather_rows(t)
    assert tuple(out.shape) == (1, 2, 3) and torch.equal(out[0], t)


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def _handle(native, bound=True, advnorm=False):
    L = native.lib()
    c = native.default_config()
    c.n_envs, c.history, c.n_beams = 64, 1, 2
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if bound:
        native.check(L.ssg_bind_state(h, C.c_void_p(Q)), h)
    if advnorm:
        nb = C.c_size_t()
        native.check(L.ssg_ppo_adv_norm_nbytes(1, C.byref(nb)))
        native.check(L.ssg_ppo_set_adv_norm(h, native.ADV_NORM_MINIBATCH, 1, C.c_void_p(Q), nb.value), h)
    return h


def _apply(native, h, pol=None, hp=None, ext=None, sh=None, counts=(467, 466, 131), mv=Q, step=1, ws=Q, nbytes=BIG, null_pol=False,
           null_hp=False, null_sh=False):
    """ssg_ppo_apply_shards with good arguments, overridden field by field."""
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = 8, 16, 1, 3, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = Q, Q
    for k, v in (pol or {}).items():
        setattr(p, k, v)
    r = native.PpoHparams()
    r.struct_size = C.sizeof(native.PpoHparams)
    r.gamma, r.lam, r.clip, r.vf_coef, r.ent_coef = 0.99, 0.95, 0.2, 0.5, 0.01
    r.lr, r.beta1, r.beta2, r.eps, r.adv_eps = 3e-4, 0.9, 0.999, 1e-8, 1e-8
    for k, v in (hp or {}).items():
        setattr(r, k, v)
    e = None
    if ext is not None:
        e = native.PpoExt()
        e.struct_size = C.sizeof(native.PpoExt)
        for k, v in ext.items():
            setattr(e, k, v)
    cnt = (C.c_int64 * max(len(counts), 1))(*counts)
    s = native.PpoShards()
    s.struct_size = C.sizeof(native.PpoShards)
    s.n_shards, s.dev_rows, s.counts, s.first_chunk, s.last_chunk, s.n_chunks = len(counts), Q, cnt, 1, 0, 1
    for k, v in (sh or {}).items():
        setattr(s, k, v)
    return native.lib().ssg_ppo_apply_shards(h, None if null_pol else C.byref(p), None if null_hp else C.byref(r),
                                             None if e is None else C.byref(e), None if null_sh else C.byref(s),
                                             C.c_void_p(mv) if mv else None, step, None, C.c_void_p(ws) if ws else None, nbytes, None)


APPLY_REFUSALS = [
    ("a NULL policy", dict(null_pol=True), b"NULL policy"),
    ("a policy of another size", dict(pol={"struct_size": 4}), b"ssg_policy.struct_size"),
    ("NULL hparams", dict(null_hp=True), b"NULL hparams"),
    ("an ext record of another size", dict(ext={"struct_size": 4}), b"ssg_ppo_ext.struct_size"),
    ("a max_grad_norm that is not finite", dict(ext={"max_grad_norm": float("nan")}), b"not finite"),
    ("a NULL shards record", dict(null_sh=True), b"NULL ssg_ppo_shards"),
    ("a shards record of another size", dict(sh={"struct_size": 8}), b"ssg_ppo_shards.struct_size"),
    ("no shards", dict(sh={"n_shards": 0}), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"),
    ("too many shards", dict(sh={"n_shards": 65}), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"),
    ("a reserved field in use", dict(sh={"reserved": 1}), b"reserved must be 0"),
    ("NULL rows", dict(sh={"dev_rows": None}), b"NULL dev_rows, counts or dev_adam_mv"),
    ("NULL counts", dict(sh={"counts": None}), b"NULL dev_rows, counts or dev_adam_mv"),
    ("NULL moments", dict(mv=0), b"NULL dev_rows, counts or dev_adam_mv"),
    ("an empty shard", dict(counts=(467, 0, 131)), b"count is < 1"),
    ("a negative count", dict(counts=(-1,)), b"count is < 1"),
    ("step 0", dict(step=0), b"step must be >= 1"),
    ("an adaptation without its divisor", dict(ext={"kl_target": 0.01, "dev_kl_coef": Q}, sh={"last_chunk": 1, "n_chunks": 0}), b"n_chunks must be >= 1"),
    ("a NULL workspace", dict(ws=0), b"NULL workspace"),
    ("a misaligned workspace", dict(ws=Q + 8), b"256-byte aligned"),
    ("a workspace too small for the plain loss", dict(nbytes=255), b"this call needs 256"),
    ("a workspace too small for the extended loss", dict(ext={}, nbytes=512), b"this call needs"),
]


@pytest.mark.parametrize("what,kw,text", APPLY_REFUSALS, ids=[c[0] for c in APPLY_REFUSALS])
def test_apply_shards_refuses(native, what, kw, text):
    L = native.lib()
    h = _handle(native)
    assert _apply(native, h, **kw) == -1, what  # SSG_ERR_BAD_ARG
    assert text in L.ssg_last_error(h), (what, L.ssg_last_error(h))
    L.ssg_destroy(h)


def test_apply_shards_refuses_by_handle(native):
    L = native.lib()
    assert _apply(native, None) == -1                                  # no handle
    h = _handle(native, bound=False)
    assert _apply(native, h) == -3 and b"ssg_bind_state" in L.ssg_last_error(h)  # SSG_ERR_NOT_BOUND
    L.ssg_destroy(h)
    h = _handle(native, advnorm=True)
    assert _apply(native, h) == -1 and b"SSG_ADV_NORM_MINIBATCH" in L.ssg_last_error(h)
    L.ssg_destroy(h)


def test_moments_entry_points_refuse(native):
    L = native.lib()
    q = C.c_void_p(Q)
    assert L.ssg_ppo_adv_moments(None, 7, 200, q, BIG, q, None) == -1
    assert L.ssg_ppo_set_adv_moments(None, 1, q, 1e-8, q, BIG, None) == -1
    h = _handle(native, bound=False)
    assert L.ssg_ppo_adv_moments(h, 7, 200, q, BIG, q, None) == -3
    assert L.ssg_ppo_set_adv_moments(h, 1, q, 1e-8, q, BIG, None) == -3
    L.ssg_destroy(h)
    h = _handle(native)
    for args, text in (((7, 200, q, BIG, None, None), b"NULL dev_out4"), ((0, 200, q, BIG, q, None), b"K and N must be >= 1"),
                       ((7, 0, q, BIG, q, None), b"K and N must be >= 1"), ((7, 200, None, BIG, q, None), b"NULL workspace"),
                       ((7, 600, q, 256 + 2 * 16, q, None), b"this call needs 304")):
        assert L.ssg_ppo_adv_moments(h, *args) == -1 and text in L.ssg_last_error(h), (args, L.ssg_last_error(h))
    for args, text in (((1, None, 1e-8, q, BIG, None), b"NULL dev_rows"), ((0, q, 1e-8, q, BIG, None), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"),
                       ((65, q, 1e-8, q, BIG, None), b"n_shards must be in 1..SSG_DP_MAX_SHARDS"), ((1, q, float("inf"), q, BIG, None), b"not finite"),
                       ((1, q, 1e-8, None, BIG, None), b"NULL workspace"), ((1, q, 1e-8, q, 16, None), b"this call needs 256")):
        assert L.ssg_ppo_set_adv_moments(h, *args) == -1 and text in L.ssg_last_error(h), (args, L.ssg_last_error(h))
    L.ssg_destroy(h)


REFUSED_FLAGS = [("--resume", ["--resume", "x.ckpt"]), ("--save-every", ["--save", "x.ckpt", "--save-every", "1"]), ("--obs-filter", ["--obs-filter"]),
                 ("--norm-reward", ["--norm-reward"]), ("--adv-norm minibatch", ["--adv-norm", "minibatch"])]


@pytest.mark.parametrize("flag,extra", REFUSED_FLAGS, ids=[f for f, _ in REFUSED_FLAGS])
def test_trainer_refuses_flags_with_more_than_one_rank(flag, extra, capsys, monkeypatch):
    """The script's exit on its own command line (host only: refused before any process is started or any device touched), with
    --gpus 2 and as a rank of a launcher's job."""
    from gpu_support import load_script
    mod = load_script("train/ppo_torch.py")
    base = ["--mode", "native", "--update", "native"]
    for argv, world in ((base + ["--gpus", "2"] + extra, None), (base + extra, "2")):
        monkeypatch.delenv("RANK", raising=False)
        monkeypatch.delenv("WORLD_SIZE", raising=False)
        if world:
            monkeypatch.setenv("RANK", "1")
            monkeypatch.setenv("WORLD_SIZE", world)
        with pytest.raises(SystemExit) as ex:
            mod.main(argv)
        assert ex.value.code not in (0, None)
        assert flag in capsys.readouterr().err
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert mod.parse_args(base + extra).gpus == 1  # (one rank: the flag is fine)
    with pytest.raises(SystemExit):
        mod.parse_args(["--gpus", "2"])  # (the default --mode / --update are not the device's)
    capsys.readouterr()


def test_data_parallel_ppo_refuses_minibatch_statistics():
    from ship_sim_gym_amd.dp import DataParallelPPO
    with pytest.raises(ValueError, match="adv_norm"):
        DataParallelPPO(None, None, adv_norm="minibatch")
