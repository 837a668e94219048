"""CPU checks of the observation filter (include/shipsim.h "Observation filter"; ship_sim_gym_amd/obs_filter.py): the record and the
entry points as header, binding and library see them, the workspace size, what ssg_set_obs_filter refuses (it judges on the host), the
numpy restatement of the device's reduction against a two-pass long-double computation, the state_dict round trip and the trainers'
flags.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_header_binding_and_library_agree(native):
    text = _header()
    consts = dict(re.findall(r"#define\s+(SSG_[A-Z_]+)\s+(0x[0-9a-fA-F]+u?|\d+)", text))
    assert int(consts["SSG_ABI_VERSION"]) == 9 == native.ABI_VERSION == native.lib().ssg_abi_version()
    assert int(consts["SSG_FILTER_ROWS"]) == native.FILTER_ROWS == 4
    assert int(consts["SSG_FILTER_UPDATE"].rstrip("u"), 0) == native.FILTER_UPDATE == 1
    body = re.search(r"typedef struct ssg_obs_filter \{(.*?)\} ssg_obs_filter;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(.*?)\s+(\**\w+(?:\s*,\s*\**\w+)*)$", decl)
        ctype, names = m.group(1).strip(), [n.strip() for n in m.group(2).split(",")]
        fields += [(n.lstrip("*"), ctype + ("*" if n.startswith("*") else "")) for n in names]
    want = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "double": C.c_double, "double*": C.c_void_p, "void*": C.c_void_p,
            "size_t": C.c_size_t}
    assert [(n, want[t]) for n, t in fields] == list(native.ObsFilterRecord._fields_)
    assert C.sizeof(native.ObsFilterRecord) == 56
    L = native.lib()
    for name in ("ssg_obs_filter_workspace_nbytes", "ssg_obs_filter_update", "ssg_set_obs_filter", "ssg_get_obs_filter"):
        assert name in native.EXPORTS and hasattr(L, name) and re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_workspace_grows_and_refuses(native):
    L = native.lib()

    def ws(n, d, p):
        out = C.c_size_t(0)
        rc = L.ssg_obs_filter_workspace_nbytes(n, d, p, C.byref(out))
        return rc, out.value

    rc, base = ws(256, 28, 1)
    assert rc == 0 and base == 2 * 28 * 8          # one tile: a mean and an M2 per column
    assert ws(257, 28, 1) == (0, 2 * base)         # a second tile
    assert ws(256, 48, 1)[1] > base and ws(256, 28, 3) == (0, 3 * base) and ws(65536, 28, 1) == (0, 256 * base)
    for bad in ((0, 28, 1), (256, 0, 1), (256, 28, 0), (-1, 28, 1), (256, 177, 1), (256, 28, 257)):
        assert ws(*bad)[0] == -1, bad
    assert L.ssg_obs_filter_workspace_nbytes(256, 28, 1, None) == -1


def _handle(native, n_envs=1000, beams=8, history=2):
    c = native.default_config()
    c.n_envs, c.n_beams, c.history = n_envs, beams, history
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _record(native, n_envs=1000, D=28, P=1, **kw):
    r = native.ObsFilterRecord()
    r.struct_size = C.sizeof(native.ObsFilterRecord)
    r.flags, r.n_members, r.obs_dim, r.clip, r.eps = native.FILTER_UPDATE, P, D, 10.0, 1e-8
    r.dev_state, r.dev_workspace = 0x10000, 0x20000  # (never dereferenced by the host-side checks)
    need = C.c_size_t()
    native.check(native.lib().ssg_obs_filter_workspace_nbytes(n_envs, D, max(1, min(P, 256)), C.byref(need)))
    r.workspace_nbytes = need.value
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_set_obs_filter_refusals_leave_the_binding(native):
    L = native.lib()
    h = _handle(native)
    got = native.ObsFilterRecord()
    assert L.ssg_get_obs_filter(h, C.byref(got)) == 0 and got.struct_size == 0      # nothing bound
    good = _record(native, clip=5.0)
    assert L.ssg_set_obs_filter(h, C.byref(good)) == 0
    bad = [dict(struct_size=8), dict(obs_dim=27), dict(n_members=0), dict(n_members=257), dict(dev_state=None), dict(dev_workspace=None),
           dict(workspace_nbytes=good.workspace_nbytes - 1), dict(flags=2), dict(flags=3), dict(clip=-1.0), dict(eps=-1e-9),
           dict(clip=float("nan")), dict(eps=float("nan"))]
    for kw in bad:
        r = _record(native, **kw)
        assert L.ssg_set_obs_filter(h, C.byref(r)) == -1, kw
        assert L.ssg_last_error(h), kw
        assert L.ssg_get_obs_filter(h, C.byref(got)) == 0
        assert (got.struct_size, got.clip, got.dev_state, got.flags) == (good.struct_size, 5.0, 0x10000, native.FILTER_UPDATE), kw
    # a member count that differs from a bound slices layout
    sizes = (C.c_int32 * 3)(300, 300, 400)
    assert L.ssg_pop_set_slices(h, 3, sizes, C.c_void_p(0x30000)) == 0
    assert L.ssg_set_obs_filter(h, C.byref(_record(native, P=2))) == -1 and b"slices" in L.ssg_last_error(h)
    assert L.ssg_set_obs_filter(h, C.byref(_record(native, P=1))) == -1
    assert L.ssg_set_obs_filter(h, C.byref(_record(native, P=3, clip=0.0, eps=0.0, flags=0))) == 0
    assert L.ssg_get_obs_filter(h, C.byref(got)) == 0 and (got.n_members, got.clip, got.flags) == (3, 0.0, 0)
    assert L.ssg_set_obs_filter(h, None) == 0                                       # NULL unbinds
    assert L.ssg_get_obs_filter(h, C.byref(got)) == 0 and got.struct_size == 0 and got.dev_state is None
    assert L.ssg_set_obs_filter(None, C.byref(good)) == -1 and L.ssg_get_obs_filter(h, None) == -1
    # the update asks for a bound state blob first (then it judges its record, then it looks for a device)
    assert L.ssg_obs_filter_update(h, C.byref(good), C.c_void_p(0x40000), None) == -3   # no state blob bound
    L.ssg_destroy(h)


def _columns(rng, n):
    """Columns like the env's own: positions, rudder, heading, lidar, the two constants, and the history half's -1 / value mixture."""
    mix = np.where(rng.random_sample(n) < 0.5, -1.0, rng.uniform(0.0, 1000.0, n))
    return np.stack([rng.uniform(0.0, 1000.0, n), rng.uniform(-35.0, 35.0, n), rng.uniform(-3.2, 3.2, n), rng.uniform(0.0, 150.0, n),
                     np.full(n, -1.0), np.full(n, 150.0), mix], axis=1)


CONST = (4, 5)


@pytest.mark.parametrize("n", [1, 2, 63, 255, 256, 257, 769, 4096, 2049, 16385, 35000])
def test_merge_reference_against_long_double(n):
    """After T successive merges of n rows each: |mean - ref| <= 16 T u max|column|, |M2 - ref| <= 64 T u ref (u = 2^-53; ref: the
    two-pass mean and sum of squared deviations over all rows so far in np.longdouble), constant columns exact."""
    from ship_sim_gym_amd.obs_filter import merge_reference
    rng = np.random.RandomState(1000 + n)
    st = np.zeros((4, 7))
    seen = np.zeros((0, 7))
    for T in range(1, 5):
        rows = _columns(rng, n)
        if n >= 63 and T == 1:  # (the columns that are kept: std / |mean| >= 1e-2, so conditioning does not set the error)
            assert all(rows[:, c].std() / abs(rows[:, c].mean()) >= 1e-2 for c in range(7) if c not in CONST)
        st = merge_reference(st, rows)
        seen = np.concatenate([seen, rows])
        ld = seen.astype(np.longdouble)
        mu = ld.sum(axis=0) / np.longdouble(len(ld))
        m2 = ((ld - mu) ** 2).sum(axis=0)
        assert st[3, 0] == T * n and not st[3, 1:].any()
        for c in range(7):
            assert abs(np.longdouble(st[0, c]) - mu[c]) <= 16 * T * U * np.abs(seen[:, c]).max(), (T, c)
            assert abs(np.longdouble(st[1, c]) - m2[c]) <= 64 * T * U * m2[c], (T, c, st[1, c], m2[c])
        for c in CONST:
            assert st[0, c] == seen[0, c] and st[1, c] == 0.0, (T, c)
        if T * n >= 2:
            np.testing.assert_array_equal(st[2], np.sqrt(st[1] / (T * n - 1.0)) + 1e-8)
        else:
            np.testing.assert_array_equal(st[2], np.ones(7))


EXACT_OFFSETS = (0.0, 2.0 ** 20, 2.0 ** 30)
EXACT_C = 0.27  # 8 x the worst measured ratio: test_merge_reference_on_an_ill_conditioned_exact_column's docstring


def _exact_column(rng, n, offset):
    """k 2^-10 + offset with k uniform in -1024..1024: every value, and every sum of such values in Python integers, is exact."""
    k = rng.randint(-1024, 1025, n)
    return k, k * 2.0 ** -10 + offset


@pytest.mark.parametrize("n", [2049, 16385])
def test_merge_reference_on_an_ill_conditioned_exact_column(n):
    """What the reduction order delivers when the mean dwarfs the spread.  One column per offset in {0, 2^20, 2^30} of values
    k 2^-10 + offset (k uniform integers in -1024..1024), three successive merges of n rows each; the exact mean and M2 of all rows so
    far come from Python integers: mean = offset + 2^-10 sum(k) / N, M2 = 2^-20 (sum(k^2) - sum(k)^2 / N).

    * mean, every offset: |mean - exact| <= 16 T u max|x|, the bound of test_merge_reference_against_long_double.
    * M2, offset 0 (well conditioned): that test's 64 T u exact.
    * M2, offset > 0: |M2 - exact| <= c kappa u exact with kappa = offset / std (std: the exact sample standard deviation of the rows so
      far, about 0.577 here, so kappa is about 1.8e6 and 1.9e9) and u = 2^-53.  The two-pass tile sums are as accurate as the well
      conditioned case; what grows with kappa is the Chan merge's delta * delta term, delta being a difference of two means that each
      carry an error of some u * offset.  So the error is a multiple of kappa u, and the multiple is measured, not derived: over the
      cases of this test (both n, both offsets, T = 1..3) the worst |M2 - exact| / (kappa u exact) of merge_reference is
      0.0337 (n = 2049, T = 3, offset 2^20; per case, printed below: 0.0001 .. 0.0337 at 2^20 and 0.0022 .. 0.0168 at 2^30), and
      c = EXACT_C = 0.27 is eight times that, rounded up to two digits: the ratio varies several-fold between draws of one size.

    tests/test_obs_filter_domain_gpu.py feeds columns of this kind to the device and requires merge_reference's bits, which carries
    these bounds over to the kernels without a tolerance on the device side."""
    from fractions import Fraction
    from ship_sim_gym_amd.obs_filter import merge_reference
    D = len(EXACT_OFFSETS)
    rng = np.random.RandomState(7000 + n)
    st = np.zeros((4, D))
    ks = [np.zeros(0, dtype=np.int64) for _ in EXACT_OFFSETS]
    for T in range(1, 4):
        rows = np.empty((n, D))
        for c, off in enumerate(EXACT_OFFSETS):
            k, rows[:, c] = _exact_column(rng, n, off)
            ks[c] = np.concatenate([ks[c], k.astype(np.int64)])
        st = merge_reference(st, rows)
        N = T * n
        assert st[3, 0] == N
        for c, off in enumerate(EXACT_OFFSETS):
            s1, s2 = int(ks[c].sum()), int((ks[c] * ks[c]).sum())
            mean = Fraction(int(off)) + Fraction(s1, N * 1024)
            m2 = Fraction(s2 * N - s1 * s1, N * 1024 * 1024)
            std = float(m2 / (N - 1)) ** 0.5
            e_mean, e_m2 = abs(Fraction(st[0, c]) - mean), abs(Fraction(st[1, c]) - m2)
            rel = float(e_m2 / m2)
            print("n %d T %d offset %g: |mean err| %.3e = %.2f u |mean|   |M2 err| / M2 %.3e = %.2f u%s"
                  % (n, T, off, float(e_mean), float(e_mean) / (U * max(abs(float(mean)), 1e-300)), rel, rel / U,
                     " = %.4f kappa u" % (rel / (off / std * U)) if off else ""))
            assert e_mean <= Fraction(16 * T * U * np.abs(ks[c] * 2.0 ** -10 + off).max()), (T, off, float(e_mean))
            if off == 0.0:
                assert e_m2 <= Fraction(64 * T * U) * m2, (T, off, rel)
            else:
                assert e_m2 <= Fraction(EXACT_C * (off / std) * U) * m2, (T, off, rel, rel / (off / std * U))


def test_merge_reference_order_is_the_documented_one():
    """The restatement against a second, scalar statement of the header's order on a shape with a tail tile and uneven runs."""
    from ship_sim_gym_amd.obs_filter import merge_reference
    rng = np.random.RandomState(5)
    n, D = 9 * 256 + 77, 2                       # 10 tiles: L = 2, runs of 2, 2, 2, 2, 2, 0, 0, 0 tiles
    x = rng.uniform(-50.0, 900.0, (n, D))

    def tree(v):
        v = list(v) + [0.0] * (256 - len(v))
        h = 128
        while h:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]

    def merge(a, b):
        if b[0] == 0:
            return a
        if a[0] == 0:
            return b
        n2 = a[0] + b[0]
        w = b[0] / n2
        d = b[1] - a[1]
        return (n2, a[1] + d * w, (a[2] + b[2]) + (d * d) * (a[0] * w))

    got = merge_reference(np.zeros((4, D)), x, eps=0.5)
    for c in range(D):
        tiles = []
        for t in range(10):
            v = [float(q) for q in x[t * 256:(t + 1) * 256, c]]
            mu = tree(v) / float(len(v))
            tiles.append((float(len(v)), mu, tree([(q - mu) * (q - mu) for q in v])))
        runs = []
        for g in range(8):
            a = (0.0, 0.0, 0.0)
            for t in range(2 * g, min(2 * g + 2, 10)):
                a = merge(a, tiles[t])
            runs.append(a)
        for h in (4, 2, 1):
            for g in range(h):
                runs[g] = merge(runs[g], runs[g + h])
        assert (got[3, 0], got[0, c], got[1, c]) == runs[0], c
        assert got[2, c] == np.sqrt(runs[0][2] / (n - 1.0)) + 0.5


class _Env(object):
    """What ObsFilter reads of an env, on the CPU."""
    num_envs, states_history = 300, 7

    def __init__(self):
        import torch
        self.device = torch.device("cpu")


def test_state_dict_round_trip_and_normalise():
    import torch
    from ship_sim_gym_amd.obs_filter import ObsFilter, merge_reference
    rng = np.random.RandomState(3)
    f = ObsFilter(_Env(), n_members=2, clip=5.0, eps=1e-6)
    assert f.state.shape == (2, 4, 7) and f.state.dtype == torch.float64 and not f.state.any()
    obs = torch.from_numpy(_columns(rng, 300))
    # the empty state: mean 0, denom 1
    assert torch.equal(f.normalise(obs), obs.clamp(-5.0, 5.0).float())
    for m in range(2):
        f.state[m].copy_(torch.from_numpy(merge_reference(np.zeros((4, 7)), obs[150 * m:150 * (m + 1)].numpy(), eps=1e-6)))
    assert f.count.tolist() == [150.0, 150.0] and torch.equal(f.var, f.M2 / 149.0)
    x = f.normalise(obs)
    for m in range(2):
        rows = obs[150 * m:150 * (m + 1)]
        assert torch.equal(x[150 * m:150 * (m + 1)], ((rows - f.mean[m]) / f.denom[m]).clamp(-5.0, 5.0).float())
        assert torch.equal(f.normalise(rows, member=m), x[150 * m:150 * (m + 1)])
    assert not x[:, 4].any() and not x[:, 5].any()                     # constant columns: (c - c) / eps
    sd = f.state_dict()
    assert sd["state"].data_ptr() != f.state.data_ptr() and (sd["n_members"], sd["obs_dim"], sd["clip"], sd["eps"]) == (2, 7, 5.0, 1e-6)
    g = ObsFilter(_Env(), n_members=2).load_state_dict(sd)
    assert torch.equal(g.state, f.state) and (g.clip, g.eps) == (5.0, 1e-6)
    with pytest.raises(ValueError):
        ObsFilter(_Env(), n_members=1).load_state_dict(sd)
    fr = f.frozen()
    assert fr.state.data_ptr() == f.state.data_ptr() and fr.to_native().flags == 0 and f.to_native().flags == 1
    sd2 = dict(sd, clip=3.0, eps=1e-4)
    f.load_state_dict(sd2)                                              # a frozen view follows its filter's clip and eps
    assert (fr.clip, fr.eps) == (3.0, 1e-4) == (f.clip, f.eps) and (fr.to_native().clip, fr.to_native().eps) == (3.0, 1e-4)
    f.load_state_dict(sd)
    assert f.train(False).to_native().flags == 0 and f.train(True).to_native().flags == 1
    for bad in (dict(n_members=0), dict(clip=-1.0), dict(eps=float("nan"))):
        with pytest.raises(ValueError):
            ObsFilter(_Env(), **bad)


def test_trainer_flags(capsys):
    ppo = load_script("train/ppo_torch.py")
    a = ppo.parse_args(["--mode", "native"])
    assert a.obs_filter is False and a.save_obs_filter is None          # off by default
    a = ppo.parse_args(["--mode", "native", "--update", "native", "--obs-filter", "--save-obs-filter", "f.pt"])
    assert a.obs_filter is True and a.save_obs_filter == "f.pt"
    for mode in ("eager", "graph", "pingpong"):
        with pytest.raises(SystemExit):
            ppo.parse_args(["--mode", mode, "--obs-filter"])
        assert "--obs-filter needs --mode native" in capsys.readouterr().err
        with pytest.raises(ValueError):
            ppo.train(envs=8, updates=1, mode=mode, obs_filter=True)     # (refused before any env is made)
    with pytest.raises(SystemExit):
        ppo.parse_args(["--mode", "native", "--save-obs-filter", "f.pt"])
    pbt = load_script("train/pbt_native.py")
    assert pbt.parse_args([]).obs_filter is False and pbt.parse_args(["--obs-filter"]).obs_filter is True
    ev = load_script("train/evaluate_native.py")
    assert ev.parse_args([]).obs_filter is None and ev.parse_args(["--obs-filter", "f.pt"]).obs_filter == "f.pt"
