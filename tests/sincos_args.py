"""The arguments sincos_body (csrc/shipsim_internal.h) is tested on, and the arithmetic of its contract.

The arguments are built around the routine's edges, not drawn at random: random doubles never land next to k pi/2, which is
exactly where a Cody-Waite reduction shows its error.  Families (build() returns them in this order; an argument that two
families produce keeps the first one's label):

  named      the two arguments at which the "within 1 ulp" of the routine's earlier comment was found false
  half_pi    the double nearest k pi/2 and its two neighbours on each side: every k in [0, 200], K_SEEDED seeded k up to K_MAX,
             and K_MAX itself (the last k whose nearest double is <= 2^18)
  quarter_pi the same five doubles around (2k + 1) pi/4, where rint switches k and the sin / cos kernels swap
  wide       uniform in [0, 2^18]
  body       uniform in [0, 10]: where body angles live
  tiny       0.0 and log-uniform magnitudes from the smallest subnormal up to 2^-20
  fallback   2^18 and nextafter on either side of it, and larger arguments: above 2^18 the routine calls the library
then every argument's negative (-0.0 included): the fixture holds both signs of everything.

tests/golden/make_golden_sincos.py stores for every argument the exact sin and cos (mpmath, 200 bits) as a double-double:
hi the correctly rounded value, lo = round(exact - hi).  error(got, hi, lo) = (got - hi) - lo is then the error of a result in
plain f64: got - hi is exact whenever got is within a factor of two of hi (Sterbenz), the subtraction of lo rounds at 2^-53 of
the ERROR — so errors far below an ulp of a 1e-14 result are measured, not rounded away.

The contract (bound()): for |a| <= 2^18, |error| <= max(1 ulp of the exact value, 2^-100 |a|).
"""
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sincos.npz")
# 50 decimals of pi: 166 bits, three times what the nearest double of k pi/2 needs (the generator checks them against mpmath)
PI = Fraction(314159265358979323846264338327950288419716939937510, 10 ** 50)
LIMIT = 262144.0            # 2^18: sincos_body's own path up to here, the library's beyond
K_MAX = 166886              # the last k with k pi/2 <= 2^18
K_DENSE = 200
K_SEEDED, Q_DENSE, Q_SEEDED, N_WIDE, N_BODY, N_TINY = 100, 60, 38, 400, 400, 100
SEED = 20261020
FAMILIES = ("named", "half_pi", "quarter_pi", "wide", "body", "tiny", "fallback")
NAMED = (182.212373908208, 45.553093477052)  # k = 116 (640 ulp) and k = 29 (241 ulp) by the earlier comment's measure
FALLBACK_LARGE = (262145.5, 1.0e6, 1.0e9, 2.0 ** 40 + 0.5, 1.0e15, 1.0e22, 1.0e300)
# arguments per family in the fixture, both signs (0.0 and -0.0 are half_pi's, k = 0).  Asserted on the committed file by tests/test_sincos.py.
COUNTS = {"named": 4, "half_pi": 3012, "quarter_pi": 1000, "wide": 800, "body": 800, "tiny": 200, "fallback": 20}


def nearest(q):
    """the double nearest the rational q (int / int division rounds correctly)"""
    return q.numerator / q.denominator


def five(x):
    """x and its two neighbours on each side, ascending"""
    lo1 = np.nextafter(x, -np.inf)
    hi1 = np.nextafter(x, np.inf)
    return [float(np.nextafter(lo1, -np.inf)), float(lo1), float(x), float(hi1), float(np.nextafter(hi1, np.inf))]


def half_pi_ks():
    rng = np.random.RandomState(SEED)
    seeded = rng.randint(K_DENSE + 1, K_MAX, size=4 * K_SEEDED)
    ks = list(range(K_DENSE + 1))
    for k in seeded:  # (the first K_SEEDED distinct ones)
        if int(k) not in ks and len(ks) < K_DENSE + 1 + K_SEEDED:
            ks.append(int(k))
    return ks + [K_MAX]


def quarter_pi_ks():
    rng = np.random.RandomState(SEED + 1)
    seeded = rng.randint(Q_DENSE + 1, K_MAX - 1, size=4 * Q_SEEDED)
    ks = list(range(Q_DENSE + 1))
    for k in seeded:
        if int(k) not in ks and len(ks) < Q_DENSE + 1 + Q_SEEDED:
            ks.append(int(k))
    return ks + [K_MAX - 1]  # (2k + 1) pi/4 = (k + 1/2) pi/2: the last one below 2^18


def build():
    """(a f64 [n], family uint8 [n], k int32 [n]): the arguments, their family's index in FAMILIES, and for half_pi / quarter_pi
    the multiple they sit at (k pi/2, (2k + 1) pi/4; negative for the mirrored half), 0 elsewhere"""
    rows = []  # (a, family, k), non-negative half
    for a in NAMED:
        rows.append((a, 0, 0))
    for k in half_pi_ks():
        for a in five(nearest(PI * k / 2)):
            if abs(a) <= LIMIT:
                rows.append((a, 1, k))
    for k in quarter_pi_ks():
        for a in five(nearest(PI * (2 * k + 1) / 4)):
            rows.append((a, 2, k))
    rng = np.random.RandomState(SEED + 2)
    rows += [(float(a), 3, 0) for a in rng.uniform(0.0, LIMIT, N_WIDE)]
    rows += [(float(a), 4, 0) for a in rng.uniform(0.0, 10.0, N_BODY)]
    rows.append((0.0, 5, 0))
    rows += [(float(np.ldexp(m, int(e))), 5, 0) for m, e in zip(rng.uniform(0.5, 1.0, N_TINY), rng.randint(-1073, -19, N_TINY))]
    rows += [(float(a), 6, 0) for a in (np.nextafter(LIMIT, 0.0), LIMIT, np.nextafter(LIMIT, np.inf)) + FALLBACK_LARGE]
    seen, a, fam, kk = set(), [], [], []
    for sign in (1.0, -1.0):
        for x, f, k in rows:
            v = np.float64(sign * x)  # (k = 0 of half_pi: the subnormal neighbours below 0.0 are the mirrored ones above it)
            bits = int(v.view(np.int64))
            if bits in seen:
                continue
            seen.add(bits)
            a.append(v); fam.append(f); kk.append(int(sign) * k)
    return np.array(a, dtype=np.float64), np.array(fam, dtype=np.uint8), np.array(kk, dtype=np.int32)


def load():
    """the committed fixture as a dict of arrays: a, family, k, sin_hi, sin_lo, cos_hi, cos_lo"""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def ulp_exact(hi, lo):
    """one ulp of the exact value hi + lo: 2^(e - 52) for 2^e <= |exact| < 2^(e + 1), the subnormal spacing at the least"""
    m, e = np.frexp(np.abs(hi))
    e = np.where(hi == 0.0, -2000, e)
    e = e - ((m == 0.5) & (lo != 0.0) & (np.signbit(lo) != np.signbit(hi)))  # hi a power of two and the exact value just below it
    return np.ldexp(1.0, np.maximum(e - 53, -1074))


def error(got, hi, lo):
    return (got - hi) - lo


def bound(a, hi, lo):
    """the contract's bound for |a| <= 2^18: max(1 ulp of the exact value, 2^-100 |a|)"""
    return np.maximum(ulp_exact(hi, lo), np.ldexp(np.abs(a), -100))


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ship_sim_gym_amd", "csrc")


def build_host(out_dir, csrc=CSRC):
    """Compiles tests/sincos_host.cpp — sincos_body of the header in `csrc`, for the host, contraction off like the library —
    into out_dir; returns the program's path, or None where there is no hipcc (the header is HIP source)."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isfile(hipcc) and os.access(hipcc, os.X_OK)):
        return None
    exe = os.path.join(str(out_dir), "sincos_host")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "sincos_host.cpp"), "-o", exe])
    return exe


def run_host(exe, a):
    """(sin, cos) f64 [n] each of the host program on the arguments a"""
    import subprocess
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = subprocess.run([exe], input=a.tobytes(), stdout=subprocess.PIPE, check=True).stdout
    sc = np.frombuffer(out, dtype=np.float64).reshape(-1, 2)
    assert len(sc) == len(a)
    return sc[:, 0].copy(), sc[:, 1].copy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def mirror_index(a):
    """j with a[j[i]] = -a[i] bit for bit (the fixture holds both signs of every argument)"""
    where = {int(b): i for i, b in enumerate(bits(a))}
    return np.array([where[int(b)] for b in bits(-a)])


def report(a, f, sn, cs, own):
    """the figures profiles/sincos/README.md records, over the arguments `own` (|a| <= 2^18): per function the worst error in ulps
    of the exact value where that is at least 2^-35, the worst error in ulps anywhere, the worst absolute error where the error
    exceeds an ulp, the share of correctly rounded results"""
    rows = []
    for name, got in (("sin", sn), ("cos", cs)):
        hi, lo = f[name + "_hi"], f[name + "_lo"]
        e, u = np.abs(error(got, hi, lo))[own], ulp_exact(hi, lo)[own]
        big = np.abs(hi[own]) >= 2.0 ** -35
        rows.append("%s: worst %.3f ulp where |%s| >= 2^-35, %.1f ulp anywhere; worst |error| beyond 1 ulp %.3e; %.2f %% correctly rounded"
                    % (name, (e / u)[big].max(), name, (e / u).max(), e[e > u].max(initial=0.0), 100.0 * np.mean(got[own] == hi[own])))
    return rows
