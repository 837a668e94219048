"""sincos_body (csrc/shipsim_internal.h), built for the host from the committed header, against exact values.

The routine is IEEE f64 arithmetic with fma and rint and nothing else, so a host build with contraction off computes the
device's bits (tests/test_sincos_gpu.py reads the device's own and compares).  The fixture tests/golden/ref_sincos.npz holds
exact sin / cos (mpmath, 200 bits, as double-doubles) of arguments built around the routine's edges: tests/sincos_args.py.

Asserted: the fixture is the generator's output and its families are what they claim; for every |a| <= 2^18 the error of both
results is at most max(1 ulp of the exact value, 2^-100 |a|); (0) -> (0, 1) exactly; sin(-a) = -sin(a) and cos(-a) = cos(a)
bit for bit at every non-zero argument.  At -0.0 the routine returns (+0.0, 1): fma(+0, HI, -0.0) is +0.0, the reduced
argument loses the sign.  Equal in value, and an angle column is +0.0 at reset and never becomes -0.0 (0.0 + w dt is +0.0
for w dt = -0.0), so the test pins that behaviour instead of asking the body's chain for another instruction.  Last, a digest
pins the routine's bits over the fixture: what the bound cannot see (HOST_BITS_SHA256 below).  The measured figures, and which
assertion caught which deliberate change on a scratch copy of the header: profiles/sincos/README.md.
"""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import sincos_args as A

# SHA-256 of the routine's sin bits, then its cos bits, over the fixture's arguments with |a| <= 2^18, in fixture order.  The bound
# alone cannot see every change: the third reduction term moves a result by less than the bound wherever it moves one at all (it
# changes the bits of 228 of the fixture's arguments, every one a double next to k pi/2), a coefficient changed in its last bit
# likewise (214).  fma and rint are exactly rounded on every host, so the digest is the same wherever this compiles; a deliberate
# change of the arithmetic re-pins it, with the bound still asserted beside it.
HOST_BITS_SHA256 = "7a4225ccb8a363531a2e7fbc108a9af54d79de2eb9d26757d2f0356f7ebd3270"


@pytest.fixture(scope="module")
def fix():
    return A.load()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = A.build_host(tmp_path_factory.mktemp("sincos_host"))
    if exe is None:
        pytest.skip("no hipcc: the header is HIP source")
    return exe


def test_fixture_is_the_generators(fix):
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_sincos", os.path.join(os.path.dirname(A.GOLDEN), "make_golden_sincos.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = gen.compute()
    assert sorted(want) == sorted(fix)
    for name in want:
        assert want[name].dtype == fix[name].dtype, name
        assert np.array_equal(want[name].view(np.uint8), fix[name].view(np.uint8)), name  # bit for bit, -0.0 included


def test_fixture_families(fix):
    a, fam, k = fix["a"], fix["family"], fix["k"]
    sh, ch = np.abs(fix["sin_hi"]), np.abs(fix["cos_hi"])
    assert fixture_size() <= largest_other_fixture()  # no larger than what tests/golden already held (ref_controlflow.npz)
    b, f2, k2 = A.build()
    assert np.array_equal(A.bits(a), A.bits(b)) and np.array_equal(fam, f2) and np.array_equal(k, k2)
    assert {n: int((fam == i).sum()) for i, n in enumerate(A.FAMILIES)} == A.COUNTS
    assert 4000 <= len(a) <= 6000 and len(set(A.bits(a).tolist())) == len(a)
    # both signs of every argument (mirror_index raises where one is missing)
    j = A.mirror_index(a)
    assert np.array_equal(A.bits(a[j]), A.bits(-a)) and np.array_equal(fam[j], fam)
    for x in A.NAMED:
        assert fam[A.bits(a) == A.bits(np.float64(-x))][0] == 0
    gap = np.spacing(np.abs(a))
    # half_pi: the five doubles around k pi/2, so |a - k pi/2| <= 2.5 gaps, and that is the tiny one of |sin|, |cos| (sin for
    # an even k); for |k| <= 200 (gap <= 2^-44) below 2^-40 as the issue asks; beyond, a gap is up to 2^-35 and 2^-40 cannot hold
    h = fam == 1
    ks = np.unique(np.abs(k[h]))
    assert set(range(A.K_DENSE + 1)) <= set(ks.tolist()) and ks.max() == A.K_MAX and len(ks) == A.K_DENSE + 2 + A.K_SEEDED
    tiny = np.where(k % 2 == 0, sh, ch)
    assert np.all(tiny[h] <= 2.5 * gap[h]) and np.all(np.where(k % 2 == 0, ch, sh)[h] > 0.999999)
    dense = h & (np.abs(k) <= A.K_DENSE)
    assert dense.sum() >= 5 * (2 * A.K_DENSE + 1) - 10 and np.all(tiny[dense] < 2.0 ** -40)
    assert np.all(np.abs(a[h]) <= A.LIMIT) and np.abs(a[h]).max() > A.LIMIT - 1.0
    # quarter_pi: |sin| and |cos| within 2.5 sqrt(2) gaps of each other (+ their own rounding); rint takes both sides
    q = fam == 2
    assert np.all(np.abs(sh - ch)[q] <= 4.0 * gap[q] + 2.0 ** -52)
    side = np.rint(np.abs(a[q]) * 6.36619772367581382433e-01) - np.abs(k[q])  # (2k + 1) pi/4 = (k + 1/2) pi/2: 0 rounded down, 1 up
    assert set(np.unique(side).tolist()) == {0.0, 1.0} and min((side == 0).sum(), (side == 1).sum()) >= 200
    assert np.abs(a[q]).max() > A.LIMIT - 2.0 and np.abs(a[q]).max() < A.LIMIT
    # wide, body, tiny, fallback
    assert np.all(np.abs(a[fam == 3]) <= A.LIMIT) and np.abs(a[fam == 3]).max() > A.LIMIT * 0.99
    assert np.all(np.abs(a[fam == 4]) <= 10.0)
    t = np.abs(a[fam == 5])
    assert t.max() < 2.0 ** -19 and (t < 2.2250738585072014e-308).sum() >= 2 and (t > 1e-100).any() and t.min() > 0.0
    assert (a == 0.0).sum() == 2 and np.signbit(a[a == 0.0]).sum() == 1
    fb = a[fam == 6]
    for x in (A.LIMIT, np.nextafter(A.LIMIT, 0.0), np.nextafter(A.LIMIT, np.inf)) + A.FALLBACK_LARGE:
        assert (fb == x).any() and (fb == -x).any()
    assert (np.abs(a) > A.LIMIT).sum() == 2 * (1 + len(A.FALLBACK_LARGE)) and np.all(fam[np.abs(a) > A.LIMIT] == 6)
    # the double-double: lo is below half an ulp of hi
    for n in ("sin", "cos"):
        assert np.all(np.abs(fix[n + "_lo"]) <= 0.5 * np.spacing(np.abs(fix[n + "_hi"])))


def fixture_size():
    return os.path.getsize(A.GOLDEN)


def largest_other_fixture():
    d = os.path.dirname(A.GOLDEN)
    return max(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)
               if os.path.isfile(os.path.join(d, f)) and os.path.join(d, f) != A.GOLDEN)


def test_host_build_meets_the_contract(fix, host):
    a = fix["a"]
    sn, cs = A.run_host(host, a)
    own = np.abs(a) <= A.LIMIT
    for line in A.report(a, fix, sn, cs, own):
        print(line, flush=True)
    for name, got in (("sin", sn), ("cos", cs)):
        hi, lo = fix[name + "_hi"], fix[name + "_lo"]
        err, bound = np.abs(A.error(got, hi, lo)), A.bound(a, hi, lo)
        bad = own & ~(err <= bound)
        assert not bad.any(), (name, int(bad.sum()), [(float(a[i]), float(got[i]), float(hi[i]), float(err[i]), float(bound[i]))
                                                       for i in np.nonzero(bad)[0][:8]])
        # the library's path beyond 2^18: not ours, unreachable by a body's angle; only that the switch hands over cleanly
        assert np.all(err[~own] <= 2.0 ** -50), name
    # (0) -> (0, 1) exactly, -0.0 too (see the module docstring)
    z = a == 0.0
    assert np.array_equal(A.bits(sn[z]), A.bits(np.zeros(2))) and np.array_equal(A.bits(cs[z]), A.bits(np.ones(2)))
    # sin odd, cos even, bit for bit
    j = A.mirror_index(a)
    nz = own & ~z
    assert np.array_equal(A.bits(sn[j])[nz], A.bits(-sn)[nz])
    assert np.array_equal(A.bits(cs[j])[nz], A.bits(cs)[nz])
    # beyond 2^18 the library's own symmetry holds as well
    assert np.array_equal(A.bits(sn[j])[~own], A.bits(-sn)[~own]) and np.array_equal(A.bits(cs[j])[~own], A.bits(cs)[~own])


def test_host_bits_are_pinned(fix, host):
    a = fix["a"]
    sn, cs = A.run_host(host, a)
    own = np.abs(a) <= A.LIMIT
    got = hashlib.sha256(A.bits(sn)[own].astype("<i8").tobytes() + A.bits(cs)[own].astype("<i8").tobytes()).hexdigest()
    assert got == HOST_BITS_SHA256, "sincos_body's arithmetic changed: some result of the fixture has other bits"
