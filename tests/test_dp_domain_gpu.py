"""GPU checks of data-parallel native PPO over its domain (ship_sim_gym_amd/dp.py; ssg_ppo_adv_moments, ssg_ppo_set_adv_moments,
ssg_ppo_apply_shards; dp_adv_moments_kernel, dp_set_adv_moments_kernel and dp_apply_kernel at the end of csrc/shipsim_ppo.hip), where
tests/test_dp_gpu.py holds them at one policy shape, three and five rows, one counts vector and well-scaled values.

Every comparison with a numpy restatement (dp.apply_reference, dp.moments_reference, dp.adam_reference, dp_support's sums) is on bit
patterns, so -0.0 and NaN payloads count; a case with NaN compares the NaN-ness of the same entries and the bits of every other one.
Every apply and every set_moments call runs twice from cloned state, first on a workspace whose bytes from 512 on are 0xFF, then on
a zeroed one, and must give the same bits: a partial or gradient entry the call read without writing it would differ.

Policy shapes.  P = tower(s) + A*H + A + H + 1 with H a multiple of 16 and A in 2..4, so P mod 16 is A + 1: 3, 4 or 5.  The eight stats
columns P .. P + 7 therefore never straddle a workgroup of 256 entries (P mod 256 is at most 245), which _shape() asserts for every
shape in use; the edges that do exist are a single workgroup (one partial), a tail workgroup that holds a few gradient entries and
the stats columns, a workgroup with 253 of 256 lanes in use, and the 309 workgroups of the largest policy the library accepts.

The Python loop runs in one process on three unequal shards (torch.stack as the gather) against ONE torch PPO on the whole batch,
within the project's bound (ppo_reference.check_per_tensor), and at the adaptation's decision boundaries."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from dp_support import HEAD, KLACC, assert_bits, bits, f32 as _f32, gae_inputs, layout, norm_of_partials, order_partials, readd_partials, \
    square_partials
from gpu_support import DEV, env_config, torch_cuda, vec  # noqa: F401
from ppo_reference import KL_BOUNDARY_FACTORS, actor_critic_policy, check_per_tensor, kl_boundary_targets, kl_factor, kl_mean, ref_update, \
    split_policy, synthetic_batch

pytestmark = pytest.mark.gpu

F32 = np.float32
HIST_BEAMS = {7: (1, 1), 9: (1, 3), 12: (1, 6), 22: (1, 16), 176: (8, 16)}  # obs_dim D = history * (6 + n_beams)
EXT = dict(vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)
NAN_WORD = 0xFFFFFFFF
CANARY = 0xC3
COUNTS3 = (467, 306, 7)
# (D, H, layers, A, separate value tower): P, workgroups of dp_apply_kernel
SHAPES = {
    "P179": ((7, 16, 1, 2, False), 179, 1),
    "P259": ((12, 16, 1, 2, False), 259, 2),
    "P245": ((9, 16, 1, 4, False), 245, 1),
    "P501": ((12, 16, 1, 4, True), 501, 2),
    "P78981": ((176, 128, 2, 4, True), 78981, 309),
}
_T0 = []


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    """The module's wall time, printed for profiles/dp/README.md."""
    _T0.append(time.time())
    yield
    print("\ntests/test_dp_domain_gpu.py: %.1f s wall" % (time.time() - _T0[0]))


@pytest.fixture(scope="module")
def envs(torch_cuda):
    """One 64-env handle per obs_dim (check_policy ties obs_dim to the handle; the PPO calls take their own K, N)."""
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    made = {}

    def get(D):
        if D not in made:
            history, n_beams = HIST_BEAMS[D]
            made[D] = ShipVecEnv(64, n_maps=4, n_beams=n_beams, env_config=env_config(history))
            assert made[D].states_history == D
        return made[D]
    yield get
    for e in made.values():
        e.close()


_MADE = {}


def _shape(torch, envs, name):
    """(policy, the extended-loss trainer, the plain-loss trainer) of SHAPES[name], made once; the two trainers share the policy."""
    from ship_sim_gym_amd.dp import DataParallelPPO
    if name not in _MADE:
        (D, H, L, A, split), P, nwg = SHAPES[name]
        make = split_policy if split else actor_critic_policy
        _, pol = make(torch, D, H, L, "tanh", A, seed=P)
        ext, plain = DataParallelPPO(pol, envs(D), perm_seed=1, **EXT), DataParallelPPO(pol, envs(D))
        assert ext.n_params == P and ext.extended() and not plain.extended()
        assert H % 16 == 0 and P % 16 == A + 1 and P // 256 == (P + 7) // 256  # the stats columns share one workgroup
        assert -(-(P + 8) // 256) == nwg
        g = torch.Generator(device=DEV).manual_seed(P)
        for tr in (ext, plain):
            tr.adam_mv.copy_(torch.randn(2 * P, generator=g, device=DEV).abs() * 1e-3)
            tr.step = 4
        _MADE[name] = (pol, ext, plain)
    return _MADE[name]


@pytest.fixture(scope="module", autouse=True)
def _forget_shapes():
    yield
    _MADE.clear()


# ------------------------------------------------------------------------------------------------------------------------------------
# the apply: run twice, collect, compare
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows(torch, W, P, seed, norm=2.0, counts=None):
    """f32 [W, P + 8]: normal gradient entries scaled so that the combined gradient's norm is about `norm`; stats columns 0..3 uniform,
    column 4 (the shards' mean KL) in 0.01..0.06, columns 5..7 nonzero (the kernel must not pass them on)."""
    from ship_sim_gym_amd import dp
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = dp.shard_weights(counts if counts is not None else [1] * W).astype(np.float64)
    rows = torch.randn((W, P + 8), generator=g, device=DEV) * (norm / math.sqrt(P * float((w * w).sum())))
    rows[:, P: P + 4] = torch.rand((W, 4), generator=g, device=DEV)
    rows[:, P + 4] = 0.01 + 0.05 * torch.rand((W,), generator=g, device=DEV)
    rows[:, P + 5:] = 7.0 + torch.rand((W, 3), generator=g, device=DEV)
    return rows.contiguous()


def _snap(tr, pol):
    return dict(params=pol.params.clone(), mv=tr.adam_mv.clone(), klc=tr.kl_coef.clone(), step=tr.step, mgn=tr.max_grad_norm,
                target=tr.kl_target, since=tr._since_first)


def _restore(tr, pol, s):
    pol.params.copy_(s["params"]); tr.adam_mv.copy_(s["mv"]); tr.kl_coef.copy_(s["klc"])
    tr.step, tr.max_grad_norm, tr.kl_target, tr._since_first = s["step"], s["mgn"], s["target"], s["since"]


def _set_word(torch, ws, offset, word):
    ws[offset: offset + 4].copy_(torch.from_numpy(np.array([word], dtype=np.uint32).view(np.uint8).copy()).to(ws.device))


def _word(ws, offset):
    return int(ws[offset: offset + 4].cpu().numpy().view(np.uint32)[0])


def _word_of(x):
    return int(np.array([x], dtype=F32).view(np.uint32)[0])


def _float_of(word):
    return np.array([word], dtype=np.uint32).view(F32)[0]


def _apply_twice(torch, tr, pol, rows, counts, first=True, last=False, word=NAN_WORD, stats=True, nan_ok=False):
    """apply_rows twice from the state on entry — on a workspace whose bytes from HEAD on are 0xFF, then zeros; bytes 0..HEAD-1 zero but
    for the running KL sum's word — and the two runs' outputs must hold the same bits.  Returns the outputs as numpy (the state is
    left as the second run left it): params, mv, kl_coef, stats (None without), word, and under the clip gvec f32 [P], part f64 [nb]."""
    P = tr.n_params
    clip = tr.extended() and tr.max_grad_norm > 0.0
    tr._ws(1, 1)
    s0, outs = _snap(tr, pol), []
    for fill in (0xFF, 0x00):
        _restore(tr, pol, s0)
        tr.workspace[:HEAD].zero_()
        tr.workspace[HEAD:].fill_(fill)
        _set_word(torch, tr.workspace, KLACC, word)
        st = tr.apply_rows(rows, counts, first, last, stats=stats)
        torch.cuda.synchronize()
        assert tr.step == s0["step"] + 1
        out = dict(params=_f32(pol.params), mv=_f32(tr.adam_mv), kl_coef=_f32(tr.kl_coef), stats=None if st is None else _f32(st),
                   word=_word(tr.workspace, KLACC))
        if clip:
            gv, part = layout(P)
            nb = -(-(P + 8) // 256)
            out["gvec"] = _f32(tr.workspace[gv: gv + 4 * P].view(torch.float32))
            out["part"] = _f32(tr.workspace[part: part + 8 * nb].view(torch.float64))
        outs.append(out)
    a, b = outs
    for k in a:
        if k == "word" or a[k] is None:
            assert a[k] == b[k], (k, a[k], b[k])
        else:
            assert_bits(a[k], b[k], "0xFF workspace against zeroed: " + k, nan_ok=nan_ok)
    return a


def _reference(tr, rows, counts, s0, first=True, last=False, word=NAN_WORD, n_chunks=1):
    """dp.apply_reference from the snapshot s0 (the state _apply_twice started from) under tr's settings."""
    from ship_sim_gym_amd import dp
    ext = tr.extended()
    with np.errstate(all="ignore"):
        return dp.apply_reference(_f32(rows), counts, _f32(s0["params"]), _f32(s0["mv"]), s0["step"] + 1, tr.hp, max_grad_norm=tr.max_grad_norm,
                                  ext=ext, kl_coef=float(s0["klc"]) if ext and tr._kl_on else None, klacc=_float_of(word),
                                  first_chunk=first, last_chunk=last, n_chunks=n_chunks, kl_target=tr.kl_target)


def _check(out, ref, tr, what, nan_ok=False):
    """Everything one apply leaves, against the reference: under the clip the combined gradient, every workgroup partial and the norm;
    the stats row, the parameters, the moments, the running KL sum's word and the coefficient."""
    P = tr.n_params
    ext = tr.extended()
    if ext and tr.max_grad_norm > 0.0:
        assert_bits(out["gvec"], ref["g"], (what, "combined gradient"), nan_ok)
        assert out["part"].shape == (-(-(P + 8) // 256),)
        assert_bits(out["part"], square_partials(ref["g"], P + 8), (what, "partials"), nan_ok)
        norm = norm_of_partials(out["part"])
        assert _word_of(norm) == _word_of(ref["norm"]), (what, norm, ref["norm"])
        if out["stats"] is not None:
            assert _word_of(out["stats"][5]) == _word_of(norm), (what, out["stats"][5], norm)
    if out["stats"] is not None:
        assert_bits(out["stats"], ref["stats"][:8 if ext else 4], (what, "stats"), nan_ok)
    assert_bits(out["params"], ref["params"], (what, "params"), nan_ok)
    assert_bits(out["mv"], ref["adam_mv"], (what, "moments"), nan_ok)
    if ext:
        if nan_ok and np.isnan(ref["klacc"]):
            assert np.isnan(_float_of(out["word"])), what
        else:
            assert out["word"] == _word_of(ref["klacc"]), (what, _float_of(out["word"]), ref["klacc"])
        if tr._kl_on:
            assert_bits(out["kl_coef"], np.array([ref["kl_coef"]], dtype=F32), (what, "kl_coef"))


def _run(torch, tr, pol, rows, counts, what, mgn=None, first=True, last=False, word=NAN_WORD, stats=True, nan_ok=False, step=None,
         n_chunks=1, target=None):
    """One case: settings, the two runs, the reference, the comparison; the trainer and policy are left as they were."""
    saved = _snap(tr, pol)
    try:
        if mgn is not None:
            tr.max_grad_norm = float(mgn)
        if target is not None:
            tr.kl_target = float(target)
        if step is not None:
            tr.step = step - 1
        tr._since_first = n_chunks - 1  # (apply_rows counts this apply in: a first chunk makes it 1)
        s0 = _snap(tr, pol)
        out = _apply_twice(torch, tr, pol, rows, counts, first, last, word, stats, nan_ok)
        ref = _reference(tr, rows, counts, s0, first, last, word, 1 if first else n_chunks)
        _check(out, ref, tr, what, nan_ok)
        if not tr.extended():
            assert out["word"] == word, (what, "the plain loss touched the running KL sum")
        return out, ref
    finally:
        _restore(tr, pol, saved)


def _different_counts(W):
    """W counts whose f32 weights all differ, in no monotonic order."""
    from ship_sim_gym_amd import dp
    counts = [3 * ((37 * r) % 64) + 1 for r in range(W)]
    w = dp.shard_weights(counts)
    assert len(set(w.tolist())) == W
    return counts


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the apply over policy shapes
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_apply_over_policy_shapes(torch_cuda, envs, name):
    torch = torch_cuda
    pol, ext, plain = _shape(torch, envs, name)
    P = ext.n_params
    rows = _rows(torch, 3, P, P + 3, counts=COUNTS3)
    out, ref = _run(torch, ext, pol, rows, COUNTS3, (name, "the clip bites"), mgn=0.5)
    assert ref["norm"] > 1.0 and ref["coef"] < 0.5
    out1, ref1 = _run(torch, ext, pol, rows, COUNTS3, (name, "clip coefficient 1"), mgn=1e6)
    assert ref1["coef"] == 1.0 and ref1["norm"] == ref["norm"]
    out0, ref0 = _run(torch, ext, pol, rows, COUNTS3, (name, "clip off"), mgn=0.0)
    assert out0["stats"][5] == 0.0
    assert_bits(out0["params"], out1["params"], (name, "a coefficient of 1 is no clip"))
    assert not np.array_equal(out["params"], out0["params"])
    _run(torch, plain, pol, rows, COUNTS3, (name, "plain loss"))
    if name in ("P179", "P78981"):
        counts = _different_counts(64)
        _run(torch, ext, pol, _rows(torch, 64, P, P + 64, counts=counts), counts, (name, "64 rows"), mgn=0.5)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. rows and weights (P = 259: two workgroups, the second holds 3 gradient entries and the stats columns)
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(torch_cuda, envs):
    return _shape(torch_cuda, envs, "P259")


@pytest.mark.parametrize("W", [1, 2, 63, 64])
def test_apply_row_counts(torch_cuda, small, W):
    pol, ext, plain = small
    counts = _different_counts(W)
    rows = _rows(torch_cuda, W, ext.n_params, 500 + W, counts=counts)
    _run(torch_cuda, ext, pol, rows, counts, ("rows", W), mgn=0.5)
    _run(torch_cuda, plain, pol, rows, counts, ("rows, plain", W))


def test_apply_refuses_65_rows_and_changes_nothing(torch_cuda, small):
    torch = torch_cuda
    from ship_sim_gym_amd._native import ShipSimError
    pol, ext, plain = small
    counts = [5] * 65
    rows = _rows(torch, 65, ext.n_params, 565, counts=counts)
    saved = _snap(ext, pol)
    ext._ws(1, 1)
    ext.workspace.fill_(CANARY)
    try:
        with pytest.raises(ShipSimError, match="n_shards must be in 1..SSG_DP_MAX_SHARDS"):
            ext.apply_rows(rows, counts, True, False, stats=True)
        torch.cuda.synchronize()
        assert ext.step == saved["step"] and torch.equal(pol.params, saved["params"]) and torch.equal(ext.adam_mv, saved["mv"])
        assert torch.equal(ext.kl_coef, saved["klc"]) and bool((ext.workspace == CANARY).all())
    finally:
        _restore(ext, pol, saved)


COUNT_CASES = [
    ("four equal counts: weights of exactly 0.25", (300, 300, 300, 300)),
    ("2^31 and 1", (1 << 31, 1)),
    ("a sum above 2^24", ((1 << 24) + 1, (1 << 25) - 1, 7)),
    ("2^40 twice", (1 << 40, 1 << 40)),
    ("one row, one sample", (1,)),
]


@pytest.mark.parametrize("what,counts", COUNT_CASES, ids=[c[0] for c in COUNT_CASES])
def test_apply_counts(torch_cuda, small, what, counts):
    from ship_sim_gym_amd import dp
    pol, ext, plain = small
    w = dp.shard_weights(counts)
    assert np.isfinite(w).all() and (w > 0).all()
    if len(set(counts)) == 1:
        assert (w == F32(1.0 / len(counts))).all()
    if counts == (1 << 31, 1):
        assert w[0] == 1.0 and 0 < w[1] < 1e-9
    rows = _rows(torch_cuda, len(counts), ext.n_params, 600 + len(what), counts=counts)
    _run(torch_cuda, ext, pol, rows, counts, what, mgn=0.5)
    _run(torch_cuda, ext, pol, rows, counts, (what, "clip off"), mgn=0.0)


def _columns(P):
    """Gradient columns at both workgroups' ends, and the stats columns the kernel combines."""
    return [0, 1, 255, 256, P - 1] + [P + c for c in range(5)]


def _entry_rows(torch, P, what):
    """(rows, counts) of a value-edge case: random rows with chosen entries in _columns(P)."""
    tiny, top = F32(2.0 ** -140), np.finfo(F32).max
    if what == "signed zeros":
        counts = (5, 5, 5)
        rows = _f32(_rows(torch, 3, P, 700, counts=counts))
        for i, c in enumerate(_columns(P)):
            rows[:, c] = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0)][i % 4]
    elif what == "2^-140 under weights of 1/3":
        counts = (5, 5, 5)
        rows = _f32(_rows(torch, 3, P, 701, counts=counts))
        for i, c in enumerate(_columns(P)):
            rows[:, c] = [(0.0, tiny, 0.0), (tiny, tiny, tiny), (-tiny, 0.0, tiny), (tiny, -0.0, -tiny)][i % 4]
    elif what == "the largest f32 in two rows under weights of 0.5":
        counts = (9, 9)
        rows = _f32(_rows(torch, 2, P, 702, counts=counts))
        for i, c in enumerate(_columns(P)):
            rows[:, c] = [(top, top), (-top, -top), (top, -top)][i % 3]
    else:
        counts = (5, 5, 5)
        rows = _f32(_rows(torch, 3, P, 703, counts=counts))
        bad = {"+inf": np.inf, "NaN": np.nan}[what]
        for i, c in enumerate(_columns(P)):
            rows[i % 3, c] = bad
    return torch.from_numpy(rows).to(DEV).contiguous(), counts


@pytest.mark.parametrize("what", ["signed zeros", "2^-140 under weights of 1/3", "the largest f32 in two rows under weights of 0.5"])
def test_apply_row_entries(torch_cuda, small, what):
    from ship_sim_gym_amd import dp
    pol, ext, plain = small
    P = ext.n_params
    rows, counts = _entry_rows(torch_cuda, P, what)
    for mgn in (0.5, 0.0):
        out, ref = _run(torch_cuda, ext, pol, rows, counts, (what, mgn), mgn=mgn)
    g, tail = ref["g"], ref["stats"]
    if what == "signed zeros":  # -0.0 survives where every row holds it, and only there
        assert [bool(np.signbit(g[c])) for c in (0, 1, 255, 256, P - 1)] == [False, True, False, False, False] and (g[[0, 1, 255, 256, P - 1]] == 0).all()
        assert [bool(np.signbit(v)) for v in tail[:5]] == [True, False, False, False, True]
    elif what.startswith("2^-140"):  # the products are subnormal and none is flushed
        w = dp.shard_weights(counts)[0]
        prod = w * F32(2.0 ** -140)
        assert 0 < prod < np.finfo(F32).tiny and g[0] == prod and g[1] == (prod + prod) + prod and g[255] == 0 and g[256] == 0
        assert tail[0] == (prod + prod) + prod and tail[3] == prod
    else:
        top = np.finfo(F32).max
        assert g[0] == top and g[1] == -top and g[255] == 0.0 and np.isfinite(ref["params"]).all()


@pytest.mark.parametrize("what", ["+inf", "NaN"])
def test_apply_non_finite_entries_with_the_clip_off(torch_cuda, small, what):
    """One +inf or NaN per chosen column, clip off: the entry's own parameter and moments are not finite (Adam on inf gives NaN), every
    other parameter and moment keeps the reference's bits.  (Under the clip the norm would spread them: not the subject here.)"""
    pol, ext, plain = small
    P = ext.n_params
    rows, counts = _entry_rows(torch_cuda, P, what)
    out, ref = _run(torch_cuda, ext, pol, rows, counts, what, mgn=0.0, nan_ok=True)
    cols = [0, 1, 255, 256, P - 1]
    assert np.isnan(out["params"][cols]).all() and np.isfinite(np.delete(out["params"], cols)).all()
    assert not np.isfinite(out["mv"][cols]).any() and np.isfinite(np.delete(out["mv"][:P], cols)).all()
    assert not np.isfinite(out["stats"][:5]).any() and (out["stats"][[5, 7]] == 0).all() and out["stats"][6] == 1.0
    _run(torch_cuda, plain, pol, rows, counts, (what, "plain"), nan_ok=True)


def test_apply_all_zero_gradient_under_the_clip(torch_cuda, small):
    """Norm 0, coefficient min(1, 0.5 / 1e-6) = 1, Adam on g = 0: m and v decay, the parameters move by the old moments alone."""
    pol, ext, plain = small
    P = ext.n_params
    rows = _rows(torch_cuda, 3, P, 710, counts=COUNTS3)
    rows[:, :P] = 0.0
    out, ref = _run(torch_cuda, ext, pol, rows, COUNTS3, "zero gradient", mgn=0.5)
    assert ref["norm"] == 0.0 and ref["coef"] == 1.0 and out["stats"][5] == 0.0 and not out["part"].any() and not out["gvec"].any()
    assert (out["mv"][:P] != 0).all() and not np.array_equal(out["params"], _f32(pol.params))


@pytest.mark.parametrize("step", [1, 100000, (1 << 31) + 5])
def test_apply_adam_step(torch_cuda, small, step):
    """The bias corrections of step 1, of a late step, and of a step that a 32-bit integer would turn negative (a negative exponent makes
    1 - beta^step negative: the step size changes sign and sqrt(bc2) is NaN)."""
    from ship_sim_gym_amd import dp
    pol, ext, plain = small
    P = ext.n_params
    rows = _rows(torch_cuda, 3, P, 720, counts=COUNTS3)
    for tr, mgn in ((ext, 0.5), (ext, 0.0), (plain, None)):
        out, ref = _run(torch_cuda, tr, pol, rows, COUNTS3, ("step", step, mgn), mgn=mgn, step=step)
        g = ref["g"] * ref["coef"] if mgn else ref["g"]
        p2, mv2 = dp.adam_reference(g, _f32(pol.params), _f32(tr.adam_mv), step, tr.hp)
        assert_bits(out["params"], p2, ("adam_reference", step))
        assert_bits(out["mv"], mv2, ("adam_reference", step))
        assert np.isfinite(out["params"]).all()


def test_apply_kl_word(torch_cuda, small):
    torch = torch_cuda
    pol, ext, plain = small
    P = ext.n_params
    rows = _rows(torch, 3, P, 730, counts=COUNTS3)
    # first_chunk sets the word: what it held (a NaN pattern) is not added to
    out, ref = _run(torch, ext, pol, rows, COUNTS3, "first chunk", mgn=0.5, first=True, word=NAN_WORD)
    kl = ref["stats"][4]
    assert out["word"] == _word_of(kl) and 0.01 < kl < 0.06
    # a later chunk adds in f32 (1/3 + kl rounds)
    third = F32(1.0) / F32(3.0)
    out, ref = _run(torch, ext, pol, rows, COUNTS3, "later chunk", mgn=0.5, first=False, word=_word_of(third), n_chunks=2)
    assert out["word"] == _word_of(F32(third + kl)) and out["word"] not in (_word_of(kl), _word_of(third))
    # ... and the adaptation divides that sum (0.34 .. 0.40) by the applies since the first chunk
    for n_chunks, target, factor in ((2, 0.05, 1.5), (40, 0.05, 0.5), (2, 0.5, 0.5), (2, 0.15, 1.0)):
        out, ref = _run(torch, ext, pol, rows, COUNTS3, ("adaptation", n_chunks, target), mgn=0.5, first=False, last=True,
                        word=_word_of(third), n_chunks=n_chunks, target=target)
        assert out["kl_coef"][0] == F32(factor) == ref["kl_coef"], (n_chunks, target, out["kl_coef"])
    # kl_coef <= 0 writes 0 into column 6
    saved = ext.kl_coef.clone()
    try:
        for coef in (0.0, -0.5):
            ext.kl_coef.fill_(coef)
            out, ref = _run(torch, ext, pol, rows, COUNTS3, ("kl_coef", coef), mgn=0.5)
            assert _word_of(out["stats"][6]) == 0 and out["word"] == _word_of(kl)
    finally:
        ext.kl_coef.copy_(saved)


def _apply_direct(torch, tr, pol, rows, counts, stats_out, first=True):
    """ssg_ppo_apply_shards as DataParallelPPO.apply_rows calls it for the plain loss, with the caller's own stats buffer."""
    from ship_sim_gym_amd import _native as N
    W = len(counts)
    cnt = (C.c_int64 * W)(*[int(c) for c in counts])
    sh = N.PpoShards()
    sh.struct_size = C.sizeof(N.PpoShards)
    sh.n_shards, sh.dev_rows, sh.counts, sh.first_chunk, sh.last_chunk, sh.n_chunks = W, rows.data_ptr(), cnt, int(first), 0, 1
    ws, nb = tr._ws_ptr()
    native, h = pol.to_native(), tr.env._h
    tr._bind_adv_norm()
    with torch.cuda.device(pol.device):
        N.check(N.lib().ssg_ppo_apply_shards(h, C.byref(native), C.byref(tr.hp), None, C.byref(sh), C.c_void_p(tr.adam_mv.data_ptr()), tr.step + 1,
                                             C.c_void_p(stats_out.data_ptr()), ws, nb, tr._stream()), h, "ssg_ppo_apply_shards")
    torch.cuda.synchronize()


def test_apply_plain_loss_leaves_the_workspace_and_zeroes_columns_4_to_7(torch_cuda, small):
    """The plain loss has no KL column: whatever the rows hold in columns 4..7, the stats row's are zero, and no byte of the workspace
    (the running KL sum's word included) changes."""
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    pol, ext, plain = small
    P = plain.n_params
    rows = _rows(torch, 3, P, 740, counts=COUNTS3)
    assert float(rows[:, P + 4:].abs().min()) > 0.0
    saved = _snap(plain, pol)
    plain._ws(1, 1)
    try:
        ref = dp.apply_reference(_f32(rows), COUNTS3, _f32(pol.params), _f32(plain.adam_mv), plain.step + 1, plain.hp)
        for fill in (0xFF, 0x00):
            _restore(plain, pol, saved)
            plain.workspace.fill_(CANARY)
            st = torch.full((32,), fill, dtype=torch.uint8, device=DEV).view(torch.float32)
            _apply_direct(torch, plain, pol, rows, COUNTS3, st)
            got = _f32(st)
            assert_bits(got, ref["stats"], ("plain stats", fill))
            assert not bits(got)[4:].any() and (got[:4] != 0).all()
            assert bool((plain.workspace == CANARY).all()), fill
            assert_bits(_f32(pol.params), ref["params"], "plain params")
            assert_bits(_f32(plain.adam_mv), ref["adam_mv"], "plain moments")
    finally:
        _restore(plain, pol, saved)


def test_apply_without_a_stats_buffer(torch_cuda, small):
    """NULL dev_stats with the clip on: parameters, moments, partials and the KL word are the bits of the run with one."""
    pol, ext, plain = small
    rows = _rows(torch_cuda, 3, ext.n_params, 750, counts=COUNTS3)
    with_st, _ = _run(torch_cuda, ext, pol, rows, COUNTS3, "with stats", mgn=0.5)
    without, _ = _run(torch_cuda, ext, pol, rows, COUNTS3, "without stats", mgn=0.5, stats=False)
    assert without["stats"] is None and without["word"] == with_st["word"]
    for k in ("params", "mv", "gvec", "part", "kl_coef"):
        assert_bits(without[k], with_st[k], ("no stats buffer", k))


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. ssg_ppo_adv_moments: loop trips, order, the count
# ------------------------------------------------------------------------------------------------------------------------------------
def _gae_batch(torch, K, n, seed, boot=False):
    """What NativePPO.gae reads, drawn directly (no policy forward): dp_support.gae_inputs on the device."""
    return {k: torch.from_numpy(v).to(DEV).contiguous() for k, v in gae_inputs(K, n, seed, boot).items()}


# (N = 1 runs at K = 2: ssg_ppo_gae refuses a batch of fewer than 2 samples, which test_adv_moments_count_is_a_double_product shows)
MOMENT_CASES = [(2, 1, 1, 1), (1, 255, 1, 1), (1, 256, 1, 1), (1, 257, 2, 1), (1, 65280, 255, 1), (1, 65536, 256, 1), (1, 65537, 257, 2),
                (1, 131073, 513, 3), (7, 600, 3, 1)]  # K, N, partials, trips of the strided loop


@pytest.mark.parametrize("K,n,nblocks,trips", MOMENT_CASES, ids=["K%d-N%d" % c[:2] for c in MOMENT_CASES])
def test_adv_moments_trips_order_and_round_trip(torch_cuda, small, K, n, nblocks, trips):
    """(a) S and Q are GAE's partials re-added in the kernel's order (lane t: partials t, t + 256, ...; then the halving tree), bit for
    bit — and so are the sums of a probe written over GAE's partials, which another order misses by 1 (GAE's own seldom show it).  (b) Against the exact sums (math.fsum over the f32 advantages; a square of an f32 is exact in f64).  The bound: an advantage
    passes through at most m = K + 16 + ceil(nblocks / 256) additions — K in its env's walk, 8 levels of its workgroup's tree, the
    strided loop's trips, 8 levels of the last tree — each of which rounds its partial sum, itself at most sum|adv| (first order), by
    at most 2^-53 relative: |S - exact| <= m 2^-53 sum|adv|, and likewise |Q - exact| <= m 2^-53 sum adv^2.  (c) One row through
    ssg_ppo_set_adv_moments gives back the 16 bytes GAE left."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    pol, tr, _ = small
    b = _gae_batch(torch, K, n, seed=K * n, boot=(K == 7))
    NativePPO.gae(tr, b)
    head = tr.workspace[:16].clone()
    part = _f32(tr.workspace[256: 256 + 16 * nblocks].view(torch.float64)).reshape(nblocks, 2).copy()
    m = _f32(tr.shard_moments(b))
    assert -(-n // 256) == nblocks
    S, Q, t = readd_partials(part)
    assert t == trips
    assert_bits(m, np.array([S, Q, float(K) * float(n), 0.0]), ("moments", K, n))
    adv = _f32(b["adv"]).astype(np.float64).reshape(-1)
    bound = (K + 16 + trips) * 2.0 ** -53
    e_s, e_q = abs(m[0] - math.fsum(adv)), abs(m[1] - math.fsum(adv * adv))
    b_s, b_q = bound * math.fsum(np.abs(adv)), bound * math.fsum(adv * adv)
    print("adv moments K=%d N=%d: |S - exact| / bound %.3f  |Q - exact| / bound %.3f" % (K, n, e_s / b_s, e_q / b_q))
    assert e_s <= b_s and e_q <= b_q, (e_s, b_s, e_q, b_q)
    for fill in (0xFF, 0x00):
        tr.workspace[:16].fill_(fill)
        tr.set_moments(torch.from_numpy(m[None].copy()).to(DEV))
        assert torch.equal(tr.workspace[:16], head), (fill, tr.workspace[:16].view(torch.float32), head.view(torch.float32))
    # (a) again on partials that tell orders apart (dp_support.order_partials), in the place of GAE's
    probe = order_partials(nblocks, seed=nblocks)
    tr.workspace[256: 256 + 16 * nblocks].view(torch.float64).copy_(torch.from_numpy(probe.reshape(-1).copy()).to(DEV))
    S, Q, _ = readd_partials(probe)
    assert_bits(_f32(tr.shard_moments(b)), np.array([S, Q, float(K) * float(n), 0.0]), ("moments of the order probe", K, n))
    if trips > 1:  # (a condition on the probe: the sums under a stride of 128 and under one lane's walk are 1 away)
        for other in (readd_partials(probe, lanes=128), readd_partials(probe, lanes=1)):
            assert abs(other[0] - S) > 0.5 and abs(other[1] - Q) > 0.5, (other, S, Q)


def test_adv_moments_count_is_a_double_product(torch_cuda, small):
    """K = 2^31 - 1, N = 2: the count is 4 294 967 294.0 exactly (an int product would wrap).  The call reads N = 2's one partial."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.ppo import NativePPO
    pol, tr, _ = small
    with pytest.raises(N.ShipSimError, match="K\\*N >= 2"):  # (one sample has no unbiased std: GAE itself refuses K = N = 1)
        NativePPO.gae(tr, _gae_batch(torch, 1, 1, seed=1))
    b = _gae_batch(torch, 1, 2, seed=2)
    NativePPO.gae(tr, b)
    want = _f32(tr.shard_moments(b))
    out = torch.full((4,), -1.0, dtype=torch.float64, device=DEV)
    ws, nb = tr._ws_ptr()
    h = tr.env._h
    with torch.cuda.device(pol.device):
        N.check(N.lib().ssg_ppo_adv_moments(h, (1 << 31) - 1, 2, ws, nb, C.c_void_p(out.data_ptr()), tr._stream()), h, "ssg_ppo_adv_moments")
    got = _f32(out)
    assert got[2] == 4294967294.0 and want[2] == 2.0
    assert_bits(got[[0, 1, 3]], want[[0, 1, 3]], "the sums do not depend on K")


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. ssg_ppo_set_adv_moments: value edges
# ------------------------------------------------------------------------------------------------------------------------------------
def _set_twice(torch, tr, rows, adv_eps=1e-8, nan_ok=False):
    """set_moments twice — the statistics row and the bytes from HEAD on 0xFF, then zero; bytes 16 .. HEAD-1 a canary — against
    dp.moments_reference on bits; the kernel writes floats 0..3 and nothing else.  Returns the row."""
    from ship_sim_gym_amd import dp
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    with np.errstate(all="ignore"):
        want = dp.moments_reference(rows, adv_eps)
    dev = torch.from_numpy(rows.copy()).to(DEV)
    saved = tr.hp.adv_eps
    tr._ws(1, 1)
    try:
        tr.hp.adv_eps = float(adv_eps)
        for fill in (0xFF, 0x00):
            tr.workspace.fill_(fill)
            tr.workspace[16:HEAD].fill_(CANARY)
            tr.set_moments(dev)
            torch.cuda.synchronize()
            got = _f32(tr.workspace[:16].view(torch.float32))
            assert_bits(got, want, ("set_moments", fill, rows[:3].tolist(), adv_eps), nan_ok)
            assert bool((tr.workspace[16:HEAD] == CANARY).all()) and bool((tr.workspace[HEAD:] == fill).all()), fill
    finally:
        tr.hp.adv_eps = saved
    return want


def _is_refused(row):
    return bool(np.isnan(row[:3]).all()) and bits(row)[3] == 0


def test_set_moments_row_counts_and_order(torch_cuda, small):
    pol, tr, _ = small
    rng = np.random.RandomState(64)
    for W in (1, 64):
        rows = np.zeros((W, 4))
        rows[:, 2] = rng.randint(1, 2000, W)
        rows[:, 0] = rng.randn(W) * rows[:, 2]
        rows[:, 1] = rows[:, 2] * (1.0 + rng.rand(W)) + rows[:, 0] ** 2 / rows[:, 2]
        row = _set_twice(torch_cuda, tr, rows)
        assert np.isfinite(row).all() and row[1] > 0
    # a sum in any order but the rows' gives another S: 2^60 absorbs the 1 that is added to it
    big, one = [2.0 ** 60, 0.0, 1.0, 0.0], [1.0, 1.0, 1.0, 0.0]
    neg = [-2.0 ** 60, 0.0, 1.0, 0.0]
    means = [_set_twice(torch_cuda, tr, order)[0] for order in ([one, big, neg], [big, one, neg], [big, neg, one])]
    assert means == [0.0, 0.0, F32(1.0 / 3.0)]


def test_set_moments_sample_counts(torch_cuda, small):
    pol, tr, _ = small
    torch = torch_cuda
    assert np.isfinite(_set_twice(torch, tr, [[3.0, 5.0, 2.0, 0.0]])).all()                                # n exactly 2
    assert np.isfinite(_set_twice(torch, tr, [[1.0, 2.0, 1.5, 0.0], [2.0, 3.0, 0.5, 0.0]])).all()            # 1.5 + 0.5
    for n in (1.0, 0.0, np.nan, 1.9999999999999998):
        assert _is_refused(_set_twice(torch, tr, [[1.0, 1.0, n, 0.0]], nan_ok=True)), n
    row = _set_twice(torch, tr, [[1e9, 3e9, 2.0 ** 31 + 1.0, 0.0]])                                           # a count past int32
    assert np.isfinite(row).all() and abs(row[0] - 1e9 / (2.0 ** 31 + 1.0)) < 1e-7
    row = _set_twice(torch, tr, [[1e15, 3e15, 2.0 ** 53, 0.0], [1e15, 3e15, 2.0, 0.0]])                       # 2^53 + 2, past f64's integers
    assert np.isfinite(row).all() and row[0] == F32(2e15 / (2.0 ** 53 + 2.0))


def _sequential_moments(value, count):
    S = Q = 0.0
    v = float(F32(value))
    for _ in range(count):
        S, Q = S + v, Q + v * v
    return S, Q


def test_set_moments_variance_edges(torch_cuda, small):
    pol, tr, _ = small
    torch = torch_cuda
    # constant advantages whose raw variance is negative: the clamp runs
    S, Q = _sequential_moments(0.1, 1400)
    raw = (Q - S * (S / 1400.0)) / 1399.0
    assert raw < 0.0 and abs(raw + 1.168e-16) < 1e-18, raw
    row = _set_twice(torch, tr, [[S, Q, 1400.0, 0.0]])
    assert row[1] == F32(1e-8) and row[0] == F32(0.1)
    # ... and its neighbour that is not clamped
    S, Q = _sequential_moments(-2.3, 1400)
    raw = (Q - S * (S / 1400.0)) / 1399.0
    assert raw > 0.0 and abs(raw - 1.50e-13) < 1e-15, raw
    row = _set_twice(torch, tr, [[S, Q, 1400.0, 0.0]])
    assert abs(row[1] - 3.9e-7) < 1e-8
    # adv_eps = 0 with variance 0: std 0, its inverse +inf
    row = _set_twice(torch, tr, [[2.0, 2.0, 2.0, 0.0]], adv_eps=0.0)
    assert bits(row).tolist() == [_word_of(1.0), 0, _word_of(np.inf), 0]
    row = _set_twice(torch, tr, [[12.5, 900.25, 1400.0, 0.0], [-3.75, 1100.5, 1400.0, 0.0]], adv_eps=0.5)
    assert 1.3 < row[1] < 1.4
    # Q = +inf: std inf, inverse 0;  S = NaN: every statistic NaN (the clamp is a comparison, which NaN fails)
    row = _set_twice(torch, tr, [[1.0, np.inf, 10.0, 0.0]])
    assert row[0] == F32(0.1) and row[1] == np.inf and bits(row)[2] == 0
    row = _set_twice(torch, tr, [[np.nan, 5.0, 10.0, 0.0], [1.0, 1.0, 10.0, 0.0]], nan_ok=True)
    assert np.isnan(row[:3]).all() and bits(row)[3] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the Python loop on unequal shards, against one PPO on the whole batch
# ------------------------------------------------------------------------------------------------------------------------------------
JOB_ENVS, JOB_K, JOB_MINIBATCHES, JOB_EPOCHS = (200, 131, 3), 7, 3, 2
JOB_TERMS = dict(vf_clip=0.2, max_grad_norm=0.05, kl_coef=1.0)
JOB_COUNTS = [[467, 306, 7], [467, 306, 7], [466, 305, 7]]


@pytest.fixture(scope="module")
def job(torch_cuda):
    """The three-shard job, set up once: policy (hidden 32, 2 layers, D = 22), one DataParallelPPO whose shard_envs are the job's, the
    whole synthetic batch and its column slices, the shards' moments, the job's statistics, the shards' permutations and per
    minibatch (e, j) the whole batch's indices of the shards' chunks j of epoch e."""
    torch = torch_cuda
    from ship_sim_gym_amd import dp
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env = vec(64, 22)
    _, pol = actor_critic_policy(torch, 22, 32, 2, "tanh", 3, seed=17)
    tr = DataParallelPPO(pol, env, perm_seed=23, **JOB_TERMS)
    tr.shard_envs = list(JOB_ENVS)
    n_all, offs = sum(JOB_ENVS), np.cumsum((0,) + JOB_ENVS)
    whole = synthetic_batch(torch, pol, JOB_K, n_all, seed=29)
    shards = [{k: (v[:, o: o + n].contiguous() if v.dim() > 1 else v[o: o + n].contiguous()) for k, v in whole.items()}
              for o, n in zip(offs, JOB_ENVS)]
    moments = []
    for b in shards:
        NativePPO.gae(tr, b)
        moments.append(tr.shard_moments(b))
    moments = torch.stack(moments)
    tr.set_moments(moments)
    torch.cuda.synchronize()
    stats = tr.workspace[:16].clone()
    assert_bits(_f32(stats.view(torch.float32)), dp.moments_reference(_f32(moments), 1e-8), "the job's statistics")
    whole["adv"] = torch.cat([b["adv"] for b in shards], dim=1).contiguous()
    whole["ret"] = torch.cat([b["ret"] for b in shards], dim=1).contiguous()
    st = stats.view(torch.float32)
    advn = (whole["adv"].reshape(-1) - st[0]) / st[1]
    n_chunks, lens = tr.check_chunks(JOB_K, JOB_MINIBATCHES)
    assert (n_chunks, lens) == (3, [467, 306, 7])
    assert [dp.chunk_counts(JOB_K, JOB_ENVS, JOB_MINIBATCHES, j) for j in range(3)] == JOB_COUNTS
    perms = []
    for r, b in enumerate(shards):
        tr.member = r
        perms.append(tr.draw_perm(b, JOB_EPOCHS))
    local, cat = [], []
    for e in range(JOB_EPOCHS):
        for j in range(n_chunks):
            idx = [perms[r][e, j * lens[r]: min(JOB_K * n, (j + 1) * lens[r])] for r, n in enumerate(JOB_ENVS)]
            assert [i.numel() for i in idx] == JOB_COUNTS[j]
            local.append(idx)
            cat.append(torch.cat([(i // n) * n_all + int(o) + i % n for i, o, n in zip(idx, offs, JOB_ENVS)]))
    assert sorted(torch.cat(cat[:3]).tolist()) == list(range(JOB_K * n_all))  # an epoch's minibatches are the whole batch, once
    yield dict(env=env, pol=pol, tr=tr, whole=whole, shards=shards, moments=moments, stats=stats, advn=advn, local=local, cat=cat,
               p0=pol.params.detach().clone())
    env.close()


def _job_update(torch, job, target):
    """One update of the job from its initial state with kl_target = target, as DataParallelPPO.update walks it: per minibatch the
    shards' local rows, torch.stack as the gather, the apply with chunk_counts.  Returns the stats rows [6, 8]."""
    from ship_sim_gym_amd import dp
    tr, pol = job["tr"], job["pol"]
    pol.params.copy_(job["p0"])
    tr.adam_mv.zero_()
    tr.kl_coef.fill_(JOB_TERMS["kl_coef"])
    tr.step, tr.updates, tr.kl_target, tr._since_first = 0, 0, float(target), 0
    tr._ws(JOB_K * max(JOB_ENVS), 467)
    tr.workspace[:16].copy_(job["stats"])
    out = []
    for e in range(JOB_EPOCHS):
        for j in range(3):
            rows = []
            for r, b in enumerate(job["shards"]):
                tr.member = r
                rows.append(tr.local_row(b, job["local"][3 * e + j][r]))
            out.append(tr.apply_rows(torch.stack(rows), dp.chunk_counts(JOB_K, JOB_ENVS, JOB_MINIBATCHES, j), j == 0,
                                     e == JOB_EPOCHS - 1 and j == 2, stats=True))
    tr.updates += 1
    torch.cuda.synchronize()
    return torch.stack(out)


def test_unequal_shards_against_one_ppo_on_the_whole_batch(torch_cuda, job):
    """Three shards of 200, 131 and 3 envs trained this way are ONE PPO on the concatenated minibatches under the job's statistics:
    parameters and both Adam moments after 2 epochs x 3 minibatches, with value clipping, the gradient-norm clip and the KL term,
    against torch (autograd, clip_grad_norm_, one torch.optim.Adam) in f64, within the project's bound per tensor."""
    torch = torch_cuda
    tr, pol = job["tr"], job["pol"]
    pol.params.copy_(job["p0"])
    kw = dict(max_grad_norm=JOB_TERMS["max_grad_norm"], index_lists=job["cat"], vf_clip=JOB_TERMS["vf_clip"], kl_coef=JOB_TERMS["kl_coef"])
    r64, s64, kl64 = ref_update(torch, pol, job["whole"], job["advn"], None, None, torch.float64, **kw)
    r32, s32, _ = ref_update(torch, pol, job["whole"], job["advn"], None, None, torch.float32, **kw)
    st = _job_update(torch, job, 0.0)
    assert st.shape == (6, 8) and tr.step == int(s64["step"]) == 6 and float(tr.kl_coef) == 1.0
    assert float(st[:, 5].min()) > JOB_TERMS["max_grad_norm"] and bool((st[:, 6] == 1.0).all())  # the clip bit in every minibatch
    P = tr.n_params
    check_per_tensor(torch, pol, pol.params, r64, r32, "unequal shards, params", verbose=True)
    check_per_tensor(torch, pol, tr.adam_mv[:P], s64["exp_avg"], s32["exp_avg"], "unequal shards, exp_avg", verbose=True)
    check_per_tensor(torch, pol, tr.adam_mv[P:], s64["exp_avg_sq"], s32["exp_avg_sq"], "unequal shards, exp_avg_sq", verbose=True)
    assert len(kl64) == 6 and bool((st[:, 4] > 0).all())
    # run to run
    again = _job_update(torch, job, 0.0)
    assert torch.equal(again, st)


def test_unequal_shards_adaptation_at_its_boundaries(torch_cuda, job):
    """The adaptation's divisor is the LAST epoch's three chunks.  From a probe's stats rows the four targets at the decision's
    boundaries; one update per target changes nothing but the coefficient, by x 1.5, 1, 1, 0.5.  A divisor of 6 (the applies of the
    whole update) would halve the mean and take the other side at the first and third target, which the test asserts first."""
    torch = torch_cuda
    tr, pol = job["tr"], job["pol"]
    probe = _job_update(torch, job, 0.0)
    p1, mv1 = pol.params.clone(), tr.adam_mv.clone()
    kls = _f32(probe[:, 4])
    last = kls[3:]
    assert (kls > 0).all() and np.isfinite(kls).all()
    pairs = kl_boundary_targets(last)
    assert tuple(f for _, f in pairs) == KL_BOUNDARY_FACTORS
    for name, wrong in (("a divisor of 6", kl_mean(last, divisor=6)), ("both epochs over 3", kl_mean(kls, divisor=3)),
                        ("the last chunk alone", kl_mean(last[-1:], divisor=3))):
        assert [kl_factor(wrong, t) for t, _ in pairs] != list(KL_BOUNDARY_FACTORS), name
    wrong = kl_mean(last, divisor=6)
    assert [kl_factor(wrong, t) for t, _ in pairs] == [1.0, 1.0, 0.5, 0.5]
    for target, factor in pairs:
        st = _job_update(torch, job, target)
        assert torch.equal(st, probe) and torch.equal(pol.params, p1) and torch.equal(tr.adam_mv, mv1), target
        assert _f32(tr.kl_coef)[0] == F32(F32(JOB_TERMS["kl_coef"]) * F32(factor)), (target, factor, float(tr.kl_coef))
