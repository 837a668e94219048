"""CPU checks of the return filter (include/shipsim.h "Return filter"; ship_sim_gym_amd/ret_filter.py): the record and the entry points
as header, binding and library see them, the workspace size against its documented formula, what ssg_ret_filter_apply refuses (it
judges its arguments on the host before it asks for a state blob or a device), the numpy restatement against a plain hand loop and, at the shapes of
tests/test_ret_filter_domain_gpu.py, against exact rational arithmetic, and the trainers' flags.  Nothing here launches a kernel."""
import ctypes as C
import fractions
import os
import re

import numpy as np
import pytest

from gpu_support import load_script
from ret_filter_support import _geometry, _ill_inputs, _inputs, _ramp_inputs, _samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_header_binding_and_library_agree(native):
    text = _header()
    consts = dict(re.findall(r"#define\s+(SSG_[A-Z_]+)\s+(0x[0-9a-fA-F]+u?|\d+)", text))
    assert int(consts["SSG_ABI_VERSION"]) == 9 == native.ABI_VERSION == native.lib().ssg_abi_version()
    assert int(consts["SSG_RET_FILTER_UPDATE"].rstrip("u"), 0) == native.RET_FILTER_UPDATE == 1
    assert int(consts["SSG_RET_FILTER_MAX_STEPS"]) == native.RET_FILTER_MAX_STEPS >= 1024
    body = re.search(r"typedef struct ssg_ret_filter \{(.*?)\} ssg_ret_filter;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(.*?)\s+(\**\w+(?:\s*,\s*\**\w+)*)$", decl)
        ctype, names = m.group(1).strip(), [n.strip() for n in m.group(2).split(",")]
        fields += [(n.lstrip("*"), ctype + ("*" if n.startswith("*") else "")) for n in names]
    want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double, "double*": C.c_void_p, "const double*": C.c_void_p,
            "void*": C.c_void_p, "size_t": C.c_size_t}
    assert [(n, want[t]) for n, t in fields] == list(native.RetFilterRecord._fields_)
    assert [n for n, _ in fields] == ["struct_size", "flags", "n_members", "reserved", "clip", "eps", "dev_gamma", "dev_state", "dev_carry",
                                      "dev_workspace", "workspace_nbytes"]
    assert C.sizeof(native.RetFilterRecord) == 72
    L = native.lib()
    for name in ("ssg_ret_filter_workspace_nbytes", "ssg_ret_filter_apply"):
        assert name in native.EXPORTS and hasattr(L, name) and re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_workspace_formula_and_refusals(native):
    L = native.lib()

    def ws(n, k, p):
        out = C.c_size_t(0)
        rc = L.ssg_ret_filter_workspace_nbytes(n, k, p, C.byref(out))
        return rc, out.value

    # f64 [P][K][ceil(n / 256)][2] partials, then f64 [K][P] denoms
    for n, k, p in ((1, 1, 1), (256, 1, 1), (257, 1, 1), (257, 5, 3), (65536, 32, 1), (7049, 64, 3), (768, 1024, 256)):
        assert ws(n, k, p) == (0, 8 * p * k * (2 * ((n + 255) // 256) + 1)), (n, k, p)
    for bad in ((0, 1, 1), (256, 0, 1), (256, 1, 0), (-1, 1, 1), (256, native.RET_FILTER_MAX_STEPS + 1, 1), (256, 1, 257)):
        assert ws(*bad)[0] == -1, bad
    assert L.ssg_ret_filter_workspace_nbytes(256, 1, 1, None) == -1


def _handle(native, n_envs=1000):
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _record(native, n_envs=1000, K=4, P=1, **kw):
    r = native.RetFilterRecord()
    r.struct_size = C.sizeof(native.RetFilterRecord)
    r.flags, r.n_members, r.clip, r.eps = native.RET_FILTER_UPDATE, P, 10.0, 1e-8
    r.dev_gamma, r.dev_state, r.dev_carry, r.dev_workspace = 0x10000, 0x20000, 0x30000, 0x40000  # (never dereferenced by the host)
    need = C.c_size_t()
    native.check(native.lib().ssg_ret_filter_workspace_nbytes(n_envs, K, max(1, min(P, 256)), C.byref(need)))
    r.workspace_nbytes = need.value
    for k, v in kw.items():
        setattr(r, k, v)
    return r


REW, DONE, OUT, DEN = 0x100000, 0x200000, 0x300000, 0x400000
NOT_BOUND = -3  # what a call that passed every host-side check answers on a handle without a state blob


def _apply(native, h, rec, K=4, rew=REW, done=DONE, stride=1000, out=OUT, den=DEN):
    return native.lib().ssg_ret_filter_apply(h, C.byref(rec) if rec is not None else None, K, C.c_void_p(rew), C.c_void_p(done), stride,
                                             C.c_void_p(out), C.c_void_p(den), None)


def test_apply_refusals_come_before_the_device(native):
    L = native.lib()
    h = _handle(native)
    good = _record(native)
    # a call with nothing to refuse gets as far as the handle's state blob; so does one without the optional denom buffer, a frozen
    # one, a padded stride, clip = eps = 0 and K at the cap
    assert _apply(native, h, good) == NOT_BOUND
    assert _apply(native, h, good, den=None) == NOT_BOUND
    assert _apply(native, h, _record(native, flags=0, clip=0.0, eps=0.0), stride=1005) == NOT_BOUND
    kmax = native.RET_FILTER_MAX_STEPS
    assert _apply(native, h, _record(native, K=kmax), K=kmax) == NOT_BOUND
    # the record: what ssg_set_obs_filter refuses for its record
    bad = [dict(struct_size=8), dict(struct_size=good.struct_size + 8), dict(n_members=0), dict(n_members=257), dict(dev_state=None),
           dict(dev_workspace=None), dict(dev_gamma=None), dict(dev_carry=None), dict(workspace_nbytes=good.workspace_nbytes - 1),
           dict(flags=2), dict(flags=3), dict(clip=-1.0), dict(eps=-1e-9), dict(clip=float("nan")), dict(eps=float("nan"))]
    for kw in bad:
        assert _apply(native, h, _record(native, **kw)) == -1, kw
        assert L.ssg_last_error(h), kw
    # the call's own arguments
    assert _apply(native, h, None) == -1
    assert L.ssg_ret_filter_apply(None, C.byref(good), 4, C.c_void_p(REW), C.c_void_p(DONE), 1000, C.c_void_p(OUT), None, None) == -1
    for kw in (dict(K=0), dict(K=-1), dict(K=kmax + 1), dict(stride=999), dict(stride=0), dict(rew=None), dict(done=None), dict(out=None),
               dict(out=REW)):
        rec = _record(native, K=min(max(kw.get("K", 4), 1), kmax))
        assert _apply(native, h, rec, **kw) == -1, kw
    assert b"must not be the reward buffer" in L.ssg_last_error(h)
    assert _apply(native, h, _record(native, K=4), K=5) == -1 and b"workspace_nbytes" in L.ssg_last_error(h)   # sized for K = 4
    # member counts the handle's envs do not split into
    for P in (3, 7, 256):
        assert _apply(native, h, _record(native, P=P)) == -1, P
    assert b"do not split" in L.ssg_last_error(h)
    for P in (2, 4, 8, 250):
        assert _apply(native, h, _record(native, P=P)) == NOT_BOUND, P
    # ... or that differ from a bound slices layout
    sizes = (C.c_int32 * 3)(300, 300, 400)
    assert L.ssg_pop_set_slices(h, 3, sizes, C.c_void_p(0x50000)) == 0
    assert _apply(native, h, _record(native, P=2)) == -1 and b"slices" in L.ssg_last_error(h)
    assert _apply(native, h, _record(native, P=1)) == -1
    assert _apply(native, h, _record(native, P=3)) == NOT_BOUND
    L.ssg_destroy(h)


def _hand(state, carry, rew, done, gamma, clip, eps):
    """The header's walk and merge in scalar Python floats, for batches of at most one 256-row tile (one tile, one run)."""
    cnt, mean, m2 = state[3], state[0], state[1]
    c = list(carry)
    n = len(c)
    outs, dens = [], []

    def tree(v):
        v = list(v) + [0.0] * (256 - len(v))
        h = 128
        while h:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]

    for k in range(len(rew)):
        for e in range(n):
            p = c[e] * gamma
            c[e] = p + rew[k][e]
        mu = tree(c) / float(n)
        q = tree([(x - mu) * (x - mu) for x in c])
        if cnt == 0.0:
            cnt, mean, m2 = float(n), mu, q
        else:
            n2 = cnt + n
            w = n / n2
            d = mu - mean
            mean, m2, cnt = mean + d * w, (m2 + q) + (d * d) * (cnt * w), n2
        den = (m2 / (cnt - 1.0)) ** 0.5 + eps if cnt >= 2.0 else 1.0
        dens.append(den)
        div = 1.0 if den == 0.0 else den
        outs.append([min(max(r / div, -clip), clip) if clip > 0.0 else r / div for r in rew[k]])
        for e in range(n):
            if done[k][e]:
                c[e] = 0.0
    return (mean, m2, dens[-1], cnt), c, outs, dens


def test_reference_against_a_hand_loop():
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    rew = [[-0.01, 1.0, -0.01], [-0.01, -0.01, 0.3371], [-1.0, -0.01, -0.01], [-0.01, 1.0, -0.01]]     # N = 3, K = 4
    done = [[0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]]                                                 # dones in the middle
    gamma = 0.97
    for clip, eps in ((10.0, 1e-8), (0.0, 0.0), (0.5, 1e-3)):
        st, carry, out, den = ret_filter_reference(np.zeros(4), np.zeros(3), rew, done, gamma, clip, eps)
        hst, hcarry, hout, hden = _hand((0.0, 0.0, 0.0, 0.0), [0.0] * 3, rew, done, gamma, clip, eps)
        assert tuple(st) == hst and list(carry) == hcarry and out.tolist() == hout and den.tolist() == hden, (clip, eps)
        assert st[3] == 12.0 and carry[1] == 0.0 and carry[0] == -0.01 and carry[2] != 0.0
        # a second call continues the first: two calls over 2 + 2 rows leave what one call over the 4 rows does
        a = ret_filter_reference(np.zeros(4), np.zeros(3), rew[:2], done[:2], gamma, clip, eps)
        b = ret_filter_reference(a[0], a[1], rew[2:], done[2:], gamma, clip, eps)
        assert np.array_equal(b[0], st) and np.array_equal(b[1], carry) and np.array_equal(np.concatenate([a[2], b[2]]), out)
        assert np.array_equal(np.concatenate([a[3], b[3]]), den)
    assert np.abs(out).max() == 0.5 and (np.abs(out) < 0.5).any()      # (the last clip bites: 1 / denom is far above 0.5)
    # one row, one env: a single sample has denom 1
    st, carry, out, den = ret_filter_reference(np.zeros(4), [0.25], [[2.0]], [[0]], 0.5, 0.0, 1e-8)
    assert st.tolist() == [2.125, 0.0, 1.0, 1.0] and carry.tolist() == [2.125] and out.tolist() == [[2.0]] and den.tolist() == [1.0]


def _exact_mean_m2(samples):
    """(mean, M2, N) of all samples as fractions.Fraction.  Every f64 is an integer over a power of two, so the two sums are formed as
    Python integers over the largest such power and divided once: M2 = sum x^2 - (sum x)^2 / N, exactly."""
    ratios = [float(v).as_integer_ratio() for v in np.asarray(samples, dtype=np.float64).ravel()]
    big = max(q for _, q in ratios)
    ints = [p * (big // q) for p, q in ratios]
    n = len(ints)
    s1, s2 = sum(ints), sum(i * i for i in ints)
    return fractions.Fraction(s1, big * n), fractions.Fraction(s2, big * big) - fractions.Fraction(s1 * s1, big * big * n), n


#             name              K     n      inputs        gamma  dones
EXACT_CASES = [("K33-n257", 33, 257, _inputs, 0.99, True),
               ("K65-n2049-ramp", 65, 2049, _ramp_inputs, 0.99, True),
               ("K1024-n3", 1024, 3, _inputs, 0.99, True),
               ("K3-n16385-ramp", 3, 16385, _ramp_inputs, 0.99, True),
               ("K5-n4097-ill", 5, 4097, _ill_inputs, 0.0, True),
               ("K40-n300-ill", 40, 300, _ill_inputs, 0.0, True),
               ("K1024-n3-gamma1-no-dones", 1024, 3, _inputs, 1.0, False)]


@pytest.mark.parametrize("name,K,n,make,gamma,dones", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_reference_against_exact_arithmetic(name, K, n, make, gamma, dones):
    """The restatement's (mean, M2) over a whole call from the empty state against the exact mean and M2 of the same K n samples.  The
    samples come from the documented recurrence, which is elementwise, so every implementation forms the same f64 values; their mean
    and M2 are then computed in fractions.Fraction.  This is the one check of the reduction order and of the merge that shares nothing
    with the device's order: tests/test_ret_filter_domain_gpu.py compares the kernels with the restatement bit for bit, so a mistake the
    two shared in the order or in the merge would show here and nowhere else.

    Bound.  With u = 2^-53, M2 is a sum of non-negative terms (squared deviations, and delta^2 weights at every merge), built in
    levels: 8 levels of a tile's halving tree, at most L merges along a run, 3 levels of the tree over the runs, K merges into the
    state: depth = 8 + L + 3 + K on the longest path.  Each level rounds a few times (the sum, the product delta * delta, the weight
    n (n_b / n'), their product: at most 8 roundings counting those of delta itself), and a sum of non-negative terms carries relative
    errors forward without amplifying them, so the roundings of the M2 path alone give a relative error of at most 8 u depth.  What
    does amplify is the error of the means: a mean near |mean| is known to about u depth |mean| absolute, it enters delta, and an error
    e in the deltas moves M2 by up to about 2 e sqrt(N M2): relative to M2 that is u depth |mean| sqrt(N / M2) <= u depth kappa with
    kappa = sqrt(1 + N mean^2 / M2), the condition number of the variance.  Hence
        |M2 - exact| <= 8 u depth kappa exact      and      |mean - exact| <= 8 u depth kappa sqrt(M2 / N),
    the second because a mean's error is a sum of rounding errors of quantities of size |mean| <= kappa sqrt(M2 / N).  kappa is taken
    from the exact values.

    Measured with these inputs (errors in units of u, and the bound 8 depth kappa in the same unit): see profiles/ret_filter/README.md."""
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    rew, done = make(K, n, seed=1000 * n + K)
    if not dones:
        done = np.zeros_like(done)
    s, carry = _samples(np.zeros(n), rew, done, gamma)
    st, ref_carry, _, _ = ret_filter_reference(np.zeros(4), np.zeros(n), rew, done, gamma)
    assert np.array_equal(ref_carry, carry) and st[3] == K * n
    mean, m2, N = _exact_mean_m2(s)
    assert N == K * n and m2 > 0
    u = 2.0 ** -53
    depth = 8 + _geometry(n)[1] + 3 + K
    kappa = float(1 + N * mean * mean / m2) ** 0.5
    err_m2 = float(abs(fractions.Fraction(float(st[1])) - m2) / m2)
    err_mean = float(abs(fractions.Fraction(float(st[0])) - mean))
    scale = float(m2 / N) ** 0.5
    print("%s: kappa %.4g  depth %d  M2 error %.4g u (bound %.4g u)  mean error %.4g u sqrt(M2/N) (same bound)"
          % (name, kappa, depth, err_m2 / u, 8 * depth * kappa, err_mean / scale / u))
    assert err_m2 <= 8 * u * depth * kappa, (err_m2 / u, 8 * depth * kappa)
    assert err_mean <= 8 * u * depth * kappa * scale, (err_mean / scale / u, 8 * depth * kappa)
    if "ill" in name:
        assert kappa > 1e6 and (s == rew).all()                            # (gamma = 0: the samples are the rewards)


def test_frozen_reference():
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    rng = np.random.RandomState(4)
    rew = rng.uniform(-1.0, 1.0, (4, 3))
    done = rng.random_sample((4, 3)) < 0.3
    # the empty state: the rewards come back unchanged, state and carry stay
    st, carry, out, den = ret_filter_reference(np.zeros(4), np.zeros(3), rew, done, 0.99, 0.0, 1e-8, update=False)
    assert np.array_equal(out, rew) and not st.any() and not carry.any() and den.tolist() == [1.0] * 4
    # a state with statistics: every row is divided by the state's own denom
    state, c0 = np.array([0.1, 7.0, 0.25, 29.0]), np.array([0.5, -0.5, 2.0])
    st, carry, out, den = ret_filter_reference(state, c0, rew, done, 0.99, 3.0, 1e-8, update=False)
    assert np.array_equal(st, state) and np.array_equal(carry, c0) and den.tolist() == [0.25] * 4
    assert np.array_equal(out, np.clip(rew / 0.25, -3.0, 3.0)) and np.abs(out).max() == 3.0
    with pytest.raises(ValueError):
        ret_filter_reference(np.zeros(4), np.zeros(2), rew, done, 0.99)


class _Env(object):
    """What ReturnFilter reads of an env, on the CPU."""
    num_envs = 300

    def __init__(self):
        import torch
        self.device = torch.device("cpu")


def test_filter_object_on_the_host(native):
    import torch
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    f = ReturnFilter(_Env(), n_members=3, gamma=[0.9, 0.99, 1.0], clip=5.0, eps=1e-6)
    assert f.state.shape == (3, 4) and f.carry.shape == (300,) and f.state.dtype == f.carry.dtype == f.gamma_dev.dtype == torch.float64
    assert not f.state.any() and not f.carry.any() and f.gamma_dev.tolist() == [0.9, 0.99, 1.0] and f.workspace.numel() == 0
    rec = f.to_native(8)
    assert (rec.struct_size, rec.flags, rec.n_members, rec.reserved, rec.clip, rec.eps) == (72, 1, 3, 0, 5.0, 1e-6)
    assert rec.workspace_nbytes == f.workspace.numel() == 8 * 3 * 8 * (2 * 2 + 1)
    assert f.to_native(4).workspace_nbytes == rec.workspace_nbytes                 # kept while it serves
    assert f.to_native(16).workspace_nbytes == 2 * rec.workspace_nbytes            # regrown when K grows
    assert f.train(False).to_native().flags == 0 and f.train(True).to_native().flags == 1
    keep = f.gamma_dev
    assert f.set_gamma([0.9, 0.99, 1.0]).gamma_dev is keep and f.set_gamma(0.5).gamma_dev.tolist() == [0.5] * 3
    f.state[1] = torch.tensor([0.5, 8.0, 2.0, 3.0], dtype=torch.float64)
    f.carry[7] = 1.5
    assert f.count.tolist() == [0.0, 3.0, 0.0] and f.var.tolist() == [1.0, 4.0, 1.0] and f.denom[1].item() == 2.0
    sd = f.state_dict()
    assert sd["state"].data_ptr() != f.state.data_ptr() and (sd["n_members"], sd["clip"], sd["eps"], sd["gamma"]) == (3, 5.0, 1e-6, [0.5] * 3)
    g = ReturnFilter(_Env(), n_members=3).load_state_dict(sd)
    assert torch.equal(g.state, f.state) and torch.equal(g.carry, f.carry) and (g.clip, g.eps, g.gamma) == (5.0, 1e-6, [0.5] * 3)
    assert f.reset_carry().carry.any().item() is False and f.state.any()
    with pytest.raises(ValueError):
        ReturnFilter(_Env(), n_members=1).load_state_dict(sd)
    for bad in (dict(n_members=0), dict(n_members=257), dict(clip=-1.0), dict(eps=float("nan")), dict(gamma=1.5), dict(gamma=-0.1),
                dict(gamma=float("nan")), dict(n_members=2, gamma=[0.9]), dict(n_members=2, gamma=[0.9, 2.0])):
        with pytest.raises(ValueError):
            ReturnFilter(_Env(), **bad)


def test_trainer_flags(capsys):
    ppo = load_script("train/ppo_torch.py")
    a = ppo.parse_args(["--mode", "native", "--update", "native"])
    assert a.norm_reward is False and a.reward_clip == 10.0                     # off by default
    a = ppo.parse_args(["--mode", "native", "--update", "native", "--norm-reward", "--reward-clip", "5"])
    assert a.norm_reward is True and a.reward_clip == 5.0
    assert ppo.parse_args(["--mode", "native", "--update", "native", "--norm-reward", "--reward-clip", "0"]).reward_clip == 0.0
    for argv in (["--mode", "eager", "--norm-reward"], ["--mode", "graph", "--norm-reward"], ["--mode", "native", "--norm-reward"]):
        with pytest.raises(SystemExit):
            ppo.parse_args(argv)
        assert "--norm-reward needs --mode native --update native" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ppo.parse_args(["--mode", "native", "--update", "native", "--reward-clip", "5"])
    with pytest.raises(SystemExit):
        ppo.parse_args(["--mode", "native", "--update", "native", "--norm-reward", "--reward-clip", "-1"])
    for kw in (dict(mode="eager"), dict(mode="native", update="torch")):
        with pytest.raises(ValueError):
            ppo.train(envs=8, updates=1, norm_reward=True, **kw)               # (refused before any env is made)
    pbt = load_script("train/pbt_native.py")
    assert pbt.parse_args([]).norm_reward is False and pbt.parse_args([]).reward_clip == 10.0
    a = pbt.parse_args(["--norm-reward", "--reward-clip", "2.5"])
    assert a.norm_reward is True and a.reward_clip == 2.5
    with pytest.raises(SystemExit):
        pbt.parse_args(["--reward-clip", "2.5"])
