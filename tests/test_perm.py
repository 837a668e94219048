"""CPU checks of the minibatch permutations (ssg_host_perm / ssg_ppo_perm / ssg_pop_perm; csrc/shipsim_perm.h; ppo.perm_reference;
--perm of the trainers): the ABI surface, every refusal, the C function against the numpy restatement bit for bit, that every row is an
exact permutation, that the keys separate the rows, and three kinds of uniformity test with fixed seeds.  Nothing touches a device.

Uniformity thresholds are the 1 - 1e-6 quantile of chi-square by Wilson-Hilferty; the same statistics computed from
numpy.random.default_rng(seed).permutation must pass too, which validates the tests themselves.  The shipped function's values are
recorded in profiles/perm/README.md."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ssg_host_perm", "ssg_ppo_perm", "ssg_pop_perm")
LARGE = (4095, 4096, 4097, 65535, 65536, 65537, 100003)
BAD = -1  # SSG_ERR_BAD_ARG


def _ppo():
    from ship_sim_gym_amd import ppo
    return ppo


@pytest.fixture(scope="module")
def host(native):
    """ssg_host_perm as a function returning the whole row (numpy int64)."""
    return _ppo().host_perm


def test_symbols_are_exported_declared_and_cite_the_reference(native):
    text, L = open(os.path.join(ROOT, "include", "shipsim.h")).read(), native.lib()
    decls = [(m.start(), m.group(1)) for m in re.finditer(r'^\s*(?:int|const char\s*\*)\s+(ssg_\w+)\s*\(', text, flags=re.M)]
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name), name
        i = [d[1] for d in decls].index(name)
        comment = text[decls[i - 1][0]: decls[i][0]]                         # what tests/test_abi.py reads for this declaration
        assert "train/stable_baselines/ppo.py:90" in comment, name
    assert L.ssg_abi_version() == native.ABI_VERSION == 9                    # additive: the version stays
    hdr = open(os.path.join(ROOT, "ship_sim_gym_amd", "csrc", "shipsim_perm.h")).read()
    consts = dict(re.findall(r"(kPerm[A-Za-z]+) = (\d+)", hdr))
    assert (int(consts["kPermRounds"]), int(consts["kPermMinBits"]), int(consts["kPermWalkCap"])) == (
        native.PERM_ROUNDS, native.PERM_MIN_BITS, native.PERM_WALK_CAP)


def _handle(native, n_envs=256):
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


PTR = 0x100000  # (the host never dereferences a device pointer)


def test_every_refusal_is_bad_arg(native):
    L = native.lib()
    out = (C.c_int64 * 8)()
    good = dict(seed=1, update=0, member=0, epoch=0, n=8, first=0, count=8)
    assert L.ssg_host_perm(*good.values(), out) == 0 and sorted(out) == list(range(8))
    for key, val in (("update", -1), ("member", -1), ("epoch", -1), ("n", 0), ("n", -5), ("n", (1 << 32) + 1), ("first", -1), ("first", 8),
                     ("count", 0), ("count", 9), ("count", -1)):
        args = dict(good)
        args[key] = val
        assert L.ssg_host_perm(*args.values(), out) == BAD, (key, val)
    assert L.ssg_host_perm(1, 0, 0, 0, 8, 4, 5, out) == BAD                  # a window past the row's end
    assert L.ssg_host_perm(*good.values(), None) == BAD and b"out" in L.ssg_last_error(None)
    assert L.ssg_host_perm(1, 0, 0, 0, 1 << 32, (1 << 32) - 8, 8, out) == 0   # the largest n is served
    assert L.ssg_ppo_perm(None, 1, 0, 0, 1, 8, C.c_void_p(PTR), None) == BAD
    assert L.ssg_pop_perm(None, 1, 0, 1, 1, 8, 1, C.c_void_p(PTR), None) == BAD
    h = _handle(native)
    try:
        ppo_good = dict(seed=1, update=0, member=0, epochs=2, n=1024)
        for key, val, word in (("update", -1, b"update"), ("member", -1, b"member"), ("epochs", 0, b"epochs"), ("epochs", -2, b"epochs"),
                               ("n", 0, b"n_samples"), ("n", (1 << 32) + 1, b"n_samples")):
            args = dict(ppo_good)
            args[key] = val
            assert L.ssg_ppo_perm(h, *args.values(), C.c_void_p(PTR), None) == BAD and word in L.ssg_last_error(h), (key, val)
        assert L.ssg_ppo_perm(h, *ppo_good.values(), None, None) == BAD and b"dev_perm" in L.ssg_last_error(h)
        pop_good = dict(seed=1, update=0, members=4, K=4, n=64, perm_epochs=2)
        for key, val, word in (("update", -1, b"update"), ("members", 0, b"members"), ("members", 257, b"members"), ("K", 0, b"K"),
                               ("n", 0, b"n < 1"), ("perm_epochs", 0, b"perm_epochs"), ("n", (1 << 30) + 1, b"2^32")):
            args = dict(pop_good)
            args[key] = val
            assert L.ssg_pop_perm(h, *args.values(), C.c_void_p(PTR), None) == BAD and word in L.ssg_last_error(h), (key, val)
        assert L.ssg_pop_perm(h, *pop_good.values(), None, None) == BAD and b"dev_perm" in L.ssg_last_error(h)
        # members against bound slices (host only: the device table is never read here)
        sizes = (C.c_int32 * 3)(64, 128, 64)
        assert L.ssg_pop_set_slices(h, 3, sizes, C.cast(C.c_void_p(PTR), C.POINTER(C.c_int32))) == 0
        args = dict(pop_good)
        assert L.ssg_pop_perm(h, *args.values(), C.c_void_p(PTR), None) == BAD and b"slices for 3 members" in L.ssg_last_error(h)
        # good arguments get past the argument checks: what refuses then is the missing state blob, not BAD_ARG
        args["members"] = 3
        assert L.ssg_pop_perm(h, *args.values(), C.c_void_p(PTR), None) == -3
        assert L.ssg_ppo_perm(h, *ppo_good.values(), C.c_void_p(PTR), None) == -3
    finally:
        L.ssg_destroy(h)


def test_c_equals_numpy_bit_for_bit(host):
    ref = _ppo().perm_reference
    for n in list(range(1, 301)) + list(LARGE):
        key = (0x1234ABCD + n, n % 7, n % 5, n % 3)
        a, b = host(*key, n), ref(*key, n)
        assert a.dtype == b.dtype == np.int64 and a.shape == b.shape == (n,) and np.array_equal(a, b), n
    for n, first, count in ((300, 17, 100), (4097, 4000, 97), (100003, 99999, 4), (65536, 0, 1), (1, 0, 1)):
        whole = host(5, 2, 1, 0, n)
        assert np.array_equal(host(5, 2, 1, 0, n, first, count), whole[first: first + count]), (n, first)
        assert np.array_equal(ref(5, 2, 1, 0, n, first, count), whole[first: first + count]), (n, first)
    # the far end of the range: b = 32, no walk at n = 2^32; a window of a row nobody materialises
    for n in (1 << 32, (1 << 32) - 1, (1 << 31) + 1):
        a, b = host(9, 1, 0, 0, n, n - 1000, 1000), ref(9, 1, 0, 0, n, n - 1000, 1000)
        assert np.array_equal(a, b) and a.min() >= 0 and a.max() < n and np.unique(a).size == 1000, n


def test_every_row_is_an_exact_permutation(host):
    for n in list(range(1, 4097)) + list(LARGE):
        row = host(77, 3, n % 4, n % 2, n)
        assert np.array_equal(np.sort(row), np.arange(n)), n                 # (so no -1 either: the walk's cap was not reached)


def test_walks_stay_under_their_bound_and_the_cap():
    """A walk takes at most 2^b - n + 1 applications (csrc/shipsim_perm.h), which at the floor width is the cap itself."""
    ref, bits = _ppo().perm_reference, _ppo().perm_bits
    assert [bits(n) for n in (1, 2, 256, 257, 512, 513, 1 << 31, (1 << 31) + 1, 1 << 32)] == [8, 8, 8, 9, 9, 10, 31, 32, 32]
    longest = {}
    for n in (1, 2, 3, 5, 100, 129, 255, 256, 257, 4097, 65537):
        for seed in range(20):
            row, taken = ref(seed, 0, 0, 0, n, walks=True)
            assert row.min() >= 0 and 1 <= taken.min() and taken.max() <= min(256, (1 << bits(n)) - n + 1), (n, seed)
            longest[n] = max(longest.get(n, 0), int(taken.max()))
    print("longest walks (applications) by n: %s" % longest)
    assert longest[256] == 1                                                 # the domain is the row: nothing to walk past


def test_rows_whose_keys_differ_in_one_part_differ(host):
    n = 4096
    base = dict(seed=11, update=4, member=2, epoch=1)
    row0 = host(*base.values(), n)
    for key in base:
        for delta in (1, 2, 256):
            other = dict(base)
            other[key] += delta
            row = host(*other.values(), n)
            fixed = int((row == row0).sum())
            print("%s + %d: %d fixed points" % (key, delta, fixed))
            assert not np.array_equal(row, row0), (key, delta)
            assert fixed <= 12, (key, delta, fixed)                          # expected 1; 12 is beyond 1e-9 for a Poisson(1)
    # n is part of the key as well: a row over n + 1 is no extension of the row over n
    assert not np.array_equal(host(*base.values(), n + 1)[:n], row0)


# ---------------------------------------------------------------------------------------------------------------------------------
# uniformity
# ---------------------------------------------------------------------------------------------------------------------------------
def chi2_threshold(dof):
    """The 1 - 1e-6 quantile of chi-square with dof degrees of freedom (Wilson-Hilferty; 4.7534 = the normal's 1 - 1e-6 quantile)."""
    return dof * (1.0 - 2.0 / (9.0 * dof) + 4.7534 * math.sqrt(2.0 / (9.0 * dof))) ** 3


def _numpy_rows(n, seeds):
    return np.stack([np.random.default_rng(s).permutation(n) for s in seeds])


def _library_rows(host, n, seeds):
    return np.stack([host(s, 0, 0, 0, n) for s in seeds])


SOURCES = ("library", "numpy")


def _rows(source, host, n, seeds):
    return _library_rows(host, n, seeds) if source == "library" else _numpy_rows(n, seeds)


def test_thresholds_are_the_issue_s():
    got = [chi2_threshold(d) for d in (1, 5, 23, 16, 121, 99 * 99)]
    want = [27.5, 37.5, 71.2, 59.2, 210, 10481]
    for g, w in zip(got, want):
        assert abs(g - w) <= 0.006 * w, (g, w)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n,n_seeds", ((2, 4000), (3, 6000), (4, 24000)))
def test_every_permutation_occurs(host, source, n, n_seeds):
    """(a) seeds 0 .. n_seeds - 1: all n! permutations occur, and the chi-square over them (dof n! - 1) is under the threshold."""
    rows = _rows(source, host, n, range(n_seeds))
    codes = (rows * (n ** np.arange(n))).sum(axis=1)
    perms = {sum(v * n ** i for i, v in enumerate(p)): j for j, p in enumerate(itertools.permutations(range(n)))}
    counts = np.zeros(len(perms))
    for c, k in zip(*np.unique(codes, return_counts=True)):
        counts[perms[int(c)]] = k                                            # (KeyError: a row that is no permutation)
    exp = n_seeds / len(perms)
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print("(a) %s n = %d: chi-square %.2f, threshold %.1f" % (source, n, chi2, chi2_threshold(len(perms) - 1)))
    assert counts.min() > 0
    assert chi2 < chi2_threshold(len(perms) - 1)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("n", (5, 12, 100))
def test_position_by_value_counts_are_uniform(host, source, n):
    """(b) seeds 0 .. 20 n - 1: the chi-square of the n x n position x value counts against 20 each, dof (n - 1)^2."""
    n_seeds = 20 * n
    rows = _rows(source, host, n, range(n_seeds))
    counts = np.zeros((n, n))
    np.add.at(counts, (np.tile(np.arange(n), n_seeds), rows.reshape(-1)), 1)
    exp = n_seeds / n
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    print("(b) %s n = %d: chi-square %.1f, threshold %.1f" % (source, n, chi2, chi2_threshold((n - 1) ** 2)))
    assert chi2 < chi2_threshold((n - 1) ** 2)


@pytest.mark.parametrize("source", SOURCES)
def test_chunk_co_membership_is_uniform(host, source):
    """(c) n = 12 in 3 chunks of 4 (a perm row's chunk(3)), seeds 0 .. 19 999: every pair of samples shares a chunk with frequency 3/11;
    the largest |z| over the 66 pairs stays below 5.7 (two-sided 1e-6 after Bonferroni)."""
    n, n_seeds, p = 12, 20000, 3.0 / 11.0
    rows = _rows(source, host, n, range(n_seeds))
    chunk_of = np.empty((n_seeds, n), dtype=np.int64)                        # chunk_of[s, v]: the chunk sample v landed in
    np.put_along_axis(chunk_of, rows, np.tile(np.arange(n) // 4, (n_seeds, 1)), axis=1)
    worst = 0.0
    for i, j in itertools.combinations(range(n), 2):
        together = float((chunk_of[:, i] == chunk_of[:, j]).sum())
        worst = max(worst, abs(together - n_seeds * p) / math.sqrt(n_seeds * p * (1.0 - p)))
    print("(c) %s: largest |z| %.2f" % (source, worst))
    assert worst < 5.7


# ---------------------------------------------------------------------------------------------------------------------------------
# Python surface (no device)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_update_without_perm_or_seed_raises():
    """The refusal comes before anything of the batch or the device is touched."""
    from ship_sim_gym_amd.population import PopulationPPO
    ppo = _ppo()
    for cls in (ppo.NativePPO, PopulationPPO):
        obj = cls.__new__(cls)                                               # (no device here: the object's key alone)
        obj.perm_seed, obj.updates = None, 0
        with pytest.raises(ValueError, match="perm_seed"):
            obj.update({}, None, 2, 4)
        with pytest.raises(ValueError, match="perm_seed"):
            obj.draw_perm(1024, 2)
    with pytest.raises(ValueError):
        ppo.perm_reference(0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        ppo.perm_reference(0, 0, 0, 0, (1 << 32) + 1)


def test_trainers_parse_perm():
    ppo = load_script("train/ppo_torch.py")
    assert ppo.parse_args([]).perm == "torch"
    assert ppo.parse_args(["--mode", "native", "--update", "native", "--perm", "native"]).perm == "native"
    assert ppo.parse_args(["--mode", "native", "--update", "native"]).perm == "torch"
    with pytest.raises(SystemExit):
        ppo.parse_args(["--perm", "native"])                                 # needs --update native
    pbt = load_script("train/pbt_native.py")
    assert pbt.parse_args([]).perm == "torch" and pbt.parse_args(["--perm", "native"]).perm == "native"
    for mod in (ppo, pbt):
        with pytest.raises(SystemExit):
            mod.parse_args(["--perm", "numpy"])
    with pytest.raises(ValueError):
        ppo.train(perm="numpy")                                              # refused before any device is touched
    with pytest.raises(ValueError):
        ppo.train(perm="native", update="torch")
    with pytest.raises(ValueError):
        pbt.train(perm="numpy")
