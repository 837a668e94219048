"""The law of a generated world, stated once, and the tools that hold a generator to it.  Plain numpy, no GPU.

THE LAW (the reference's: game_map.py:34-63 for the banks, game.py:300-330 for the goal path).  With
``s_w = width_frac * width / 2`` the strip of side s is ``[x_min, x_max]`` = ``[0, s_w]`` (left) or ``[width - s_w, width]``
(right), and the reference's ``x_middle = x_min + (x_max - x_min)`` IS ``x_max``.  Vertex ``i = 1..10`` of a side is a draw
``x ~ gauss(x_max, 50)``, ``y ~ -100 + gauss(y_delta * i, 20)`` repeated until x falls inside the strip, hence

* ``t = (x_max - x) / 50`` lies in ``[0, s_w / 50]`` with CDF ``(2 Phi(t) - 1) / (2 Phi(s_w / 50) - 1)`` (a half-normal cut at
  the strip's inner edge: the draws above x_max are all rejected),
* ``(y - y_start - y_delta * i) / 20 ~ N(0, 1)``, independent of x (y is redrawn with x, and x alone decides), ``y_delta =
  (1.2 * height + 100) / 10``,
* vertices 11 and 12 are the side's two map corners ``(edge, height)``, ``(edge, 0)``, exactly,
* goal ``i = 1..n``: ``y - gy_delta * i`` is uniform on the 41 integers -20..20 (``gy_delta = height / (n + 1)``), ``fallback -
  (width / 2) * i`` is uniform on the 101 integers -50..50, and ``u`` (np.random.uniform's sample) is uniform on [0, 1),

all mutually independent.  The reference accepts try number 1000 whatever it is; `cap_free_bank_width` works out where that
can be ignored, and `cap_share` what the DEVICE's generator (a folded draw: every try passes with probability 2q, not q) does
below it.

THE TESTS all run at ALPHA = 1e-6 per assertion, with critical values derived here (math.erfc, the exact chi-square series):
one-sample Kolmogorov-Smirnov with the Dvoretzky-Kiefer-Wolfowitz-Massart bound ``P(D_n > d) <= 2 exp(-2 n d^2)`` (valid for
every n, so the level is at most alpha, not approximately alpha), Pearson's chi-square against a discrete uniform, and the
correlation of probability-integral-transformed pairs, ``sqrt(n) r -> N(0, 1)`` under independence.

THE CENSUS walks one world's goal path under the oracle and reports which of the segment query's branches its rays took.
"""
import collections
import math

import numpy as np

ALPHA = 1e-6
N_SEG, Y_START, X_SIGMA, Y_SIGMA = 10, -100.0, 50.0, 20.0
Y_JITTER, X_JITTER, MAX_TRIES = 20, 50, 1000
RAY_RADIUS, TOLERANCE = 10.0, 60.0     # game.py:322-325


# ---------------------------------------------------------------------------------------------------------------------
# normal CDF, critical values
# ---------------------------------------------------------------------------------------------------------------------
def phi(z):
    """Standard normal CDF, elementwise, in double precision (0.5 erfc(-z / sqrt 2))."""
    z = np.asarray(z, dtype=np.float64)
    try:
        import torch
        return (0.5 * torch.erfc(torch.from_numpy(np.ascontiguousarray(-z / math.sqrt(2.0))))).numpy().reshape(z.shape)
    except ImportError:  # pragma: no cover - (slow path)
        return 0.5 * np.frompyfunc(math.erfc, 1, 1)(-z / math.sqrt(2.0)).astype(np.float64)


def _bisect(f, lo, hi, n=200):
    """root of the DEcreasing f on [lo, hi]"""
    for _ in range(n):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def z_two_sided(alpha=ALPHA):
    """z with P(|Z| > z) = alpha for a standard normal Z."""
    return _bisect(lambda z: math.erfc(z / math.sqrt(2.0)) - alpha, 0.0, 40.0)


def ks_critical(n, alpha=ALPHA):
    return math.sqrt(-math.log(alpha / 2.0) / (2.0 * n))


def chi2_sf(x, dof):
    """P(chi^2_dof > x), exact: the finite series of the regularised upper incomplete gamma function at half-integers."""
    if x <= 0.0:
        return 1.0
    h = 0.5 * x
    if dof % 2 == 0:
        term, total = 1.0, 1.0                      # sum_{j < dof/2} h^j / j!
        for j in range(1, dof // 2):
            term *= h / j
            total += term
        return math.exp(-h) * total
    term = math.sqrt(h) / math.gamma(1.5)           # sum_{j = 1 .. (dof-1)/2} h^(j - 1/2) / Gamma(j + 1/2)
    total = term if dof >= 3 else 0.0
    for j in range(2, (dof - 1) // 2 + 1):
        term *= h / (j - 0.5)
        total += term
    return math.erfc(math.sqrt(h)) + math.exp(-h) * total


def chi2_critical(dof, alpha=ALPHA):
    return _bisect(lambda x: chi2_sf(x, dof) - alpha, 0.0, 100.0 * dof + 1000.0)


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
Check = collections.namedtuple("Check", "name stat crit ok")


def _check(name, stat, crit, ok=None):
    stat = float(stat)
    return Check(name, stat, float(crit), bool(stat < crit if ok is None else ok))


def ks_statistic(pit):
    """Kolmogorov's D_n of a sample ALREADY mapped through the hypothesised CDF (so: against the uniform law on [0, 1])."""
    f = np.sort(np.asarray(pit, dtype=np.float64).ravel())
    n = len(f)
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max(np.max(i / n - f), np.max(f - (i - 1.0) / n)))


def ks_check(name, pit, alpha=ALPHA):
    pit = np.asarray(pit).ravel()
    return _check(name, ks_statistic(pit), ks_critical(len(pit), alpha))


def chi2_uniform_check(name, values, lo, hi, alpha=ALPHA):
    """Pearson's chi-square of integer `values` against the uniform law on lo..hi; also fails when a value is out of range or
    one of the hi - lo + 1 values never occurs."""
    v = np.asarray(values).ravel()
    k = hi - lo + 1
    inside = (v >= lo) & (v <= hi)
    counts = np.bincount((v[inside] - lo).astype(np.int64), minlength=k)
    e = len(v) / k
    stat = float(np.sum((counts - e) ** 2) / e)
    crit = chi2_critical(k - 1, alpha)
    return _check(name, stat, crit, ok=bool(inside.all() and counts.min() > 0 and stat < crit))


def corr_check(name, a, b, alpha=ALPHA):
    """|Pearson r| of two samples of uniforms (probability-integral transforms) against z_alpha / sqrt(n)."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    r = float(np.dot(a, b) / math.sqrt(np.dot(a, a) * np.dot(b, b)))
    return _check(name, abs(r), z_two_sided(alpha) / math.sqrt(len(a)))


def proportion_bounds(p, n, alpha=ALPHA):
    """[lo, hi] holding a Binomial(n, p) / n with probability >= 1 - alpha (Hoeffding: P(|X/n - p| >= d) <= 2 exp(-2 n d^2);
    a bound for every n, no normal approximation in the tail)."""
    d = math.sqrt(-math.log(alpha / 2.0) / (2.0 * n))
    return p - d, p + d


# ---------------------------------------------------------------------------------------------------------------------
# the law
# ---------------------------------------------------------------------------------------------------------------------
def strip_width(width, width_frac):
    return width_frac * width / 2


def y_delta(height):
    return (height * 1.2 - Y_START) / N_SEG


def t_cdf(t, s_w):
    """CDF of t = (x_max - x) / 50 on [0, s_w / 50]."""
    return (2.0 * phi(t) - 1.0) / (2.0 * float(phi(s_w / X_SIGMA)) - 1.0)


def standardise_banks(polys, width, height, width_frac):
    """polys [M, 2, 12, 2] -> (t, zy), each [M, 2, 10]: the strip-relative x in sigmas and the standardised y deviate."""
    polys = np.asarray(polys, dtype=np.float64)
    s_w = strip_width(width, width_frac)
    x_max = np.array([s_w, width], dtype=np.float64)[None, :, None]
    i = np.arange(1, N_SEG + 1, dtype=np.float64)[None, None, :]
    t = (x_max - polys[:, :, :N_SEG, 0]) / X_SIGMA
    zy = (polys[:, :, :N_SEG, 1] - Y_START - y_delta(height) * i) / Y_SIGMA
    return t, zy


def corners(width, height):
    return np.array([[[0.0, height], [0.0, 0.0]], [[width, height], [width, 0.0]]])


def bank_law_checks(polys, width, height, width_frac, tag=""):
    """Every statistical check of the bank vertices' law on polys [M, 2, 12, 2].  Returns a list of Check."""
    s_w = strip_width(width, width_frac)
    t, zy = standardise_banks(polys, width, height, width_frac)
    M = len(t)
    out = []
    bad = int(np.sum(~np.isfinite(t)) + np.sum(~np.isfinite(zy)) + np.sum(t < 0.0) + np.sum(t > s_w / X_SIGMA))
    out.append(_check(tag + "x inside the strip, all finite (violations)", bad, 1))
    out.append(_check(tag + "corner vertices exact (violations)",
                      int(np.sum(np.asarray(polys)[:, :, N_SEG:, :] != corners(width, height)[None])), 1))
    ut = np.clip(t_cdf(t, s_w), 0.0, 1.0)
    vy = phi(zy)
    for s, side in enumerate(("left", "right")):
        out.append(ks_check(tag + "KS x %s pooled" % side, ut[:, s]))
        out.append(ks_check(tag + "KS y %s pooled" % side, vy[:, s]))
        for i in range(N_SEG):
            out.append(ks_check(tag + "KS x %s vertex %d" % (side, i + 1), ut[:, s, i]))
            out.append(ks_check(tag + "KS y %s vertex %d" % (side, i + 1), vy[:, s, i]))
    fy = np.abs(2.0 * vy - 1.0)  # |y deviate|'s transform: a y taken from the x deviate is uncorrelated with |z| but not this
    out.append(corr_check(tag + "corr x,y within a vertex", ut, vy))
    out.append(corr_check(tag + "corr x,|y| within a vertex", ut, fy))
    us, vs, fs = ut.reshape(M, 2 * N_SEG), vy.reshape(M, 2 * N_SEG), fy.reshape(M, 2 * N_SEG)  # the stream's order
    for na, a in (("x", us), ("y", vs), ("|y|", fs)):
        for nb, b in (("x", us), ("y", vs), ("|y|", fs)):
            out.append(corr_check(tag + "corr %s(v),%s(v+1) across vertices" % (na, nb), a[:, :-1], b[:, 1:]))
    if M > 1:
        for na, a in (("x", us), ("y", vs)):
            for nb, b in (("x", us), ("y", vs)):
                out.append(corr_check(tag + "corr %s(m),%s(m+1) across maps" % (na, nb), a[:-1], b[1:]))
        out.append(corr_check(tag + "corr last vertex of m, first of m+1", vs[:-1, -1], us[1:, 0]))
    return out


def goal_law_checks(gy, u, fb, width, height, n_goals, tag=""):
    """gy, u, fb: [M, n_goals] goal rows, uniform draws, fallback columns (any may be None)."""
    out = []
    i = np.arange(1, n_goals + 1, dtype=np.float64)[None, :]
    pits = {}
    if gy is not None:
        j = np.asarray(gy, dtype=np.float64) - (height / (n_goals + 1)) * i
        jr = np.rint(j)
        out.append(_check(tag + "goal y jitter integral (violations)", int(np.sum(~(np.abs(j - jr) < 1e-9))), 1))
        out.append(chi2_uniform_check(tag + "chi2 goal y jitter", jr.astype(np.int64), -Y_JITTER, Y_JITTER))
        pits["y"] = (jr + Y_JITTER + 0.5) / (2 * Y_JITTER + 1)
    if fb is not None:
        j = np.asarray(fb, dtype=np.float64) - (width / 2) * i
        jr = np.rint(j)
        out.append(_check(tag + "fallback jitter integral (violations)", int(np.sum(~(np.abs(j - jr) < 1e-9))), 1))
        out.append(chi2_uniform_check(tag + "chi2 fallback jitter", jr.astype(np.int64), -X_JITTER, X_JITTER))
        pits["fb"] = (jr + X_JITTER + 0.5) / (2 * X_JITTER + 1)
    if u is not None:
        u = np.asarray(u, dtype=np.float64)
        out.append(_check(tag + "u in [0, 1) (violations)", int(np.sum(~((u >= 0.0) & (u < 1.0)))), 1))
        out.append(ks_check(tag + "KS u", u))
        pits["u"] = u
    names = sorted(pits)
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            out.append(corr_check(tag + "corr %s,%s within a goal" % (names[a], names[b]), pits[names[a]], pits[names[b]]))
    for nm in names:
        if n_goals > 1:
            out.append(corr_check(tag + "corr %s(g),%s(g+1) across goals" % (nm, nm), pits[nm][:, :-1], pits[nm][:, 1:]))
        if len(pits[nm]) > 1:
            out.append(corr_check(tag + "corr %s(m),%s(m+1) across maps" % (nm, nm), pits[nm][:-1], pits[nm][1:]))
    return out


def failures(checks):
    return [c for c in checks if not c.ok]


def describe(checks, kinds=("KS x", "KS y", "KS u", "chi2", "corr")):
    """One line per kind of check: the largest statistic / critical value ratio among the checks of that kind."""
    lines = []
    for k in kinds:
        cs = [c for c in checks if k in c.name]
        if cs:
            w = max(cs, key=lambda c: c.stat / c.crit)
            lines.append("%-5s worst of %3d: %-48s %.6g against %.6g" % (k, len(cs), w.name, w.stat, w.crit))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------------
# the try cap
# ---------------------------------------------------------------------------------------------------------------------
def pass_probability(s_w):
    """q = Phi(s_w / 50) - 1/2: the chance that ONE two-sided try of the reference lands inside a strip s_w wide."""
    return 0.5 * math.erf(s_w / (X_SIGMA * math.sqrt(2.0)))


def cap_free_bank_width(p=1e-12):
    """The ``width_frac * width`` above which a vertex reaches try 1000 with probability below p under the REFERENCE's law,
    (1 - q)^999 < p — the device's folded draw passes with 2q per try and is far below p there.  Above it the two laws are
    the same law; below it they part (the reference's capped vertex is whatever try 1000 drew, the device's is folded)."""
    q = 1.0 - math.exp(math.log(p) / (MAX_TRIES - 1))
    s_w = _bisect(lambda s: q - pass_probability(s), 0.0, 1000.0)
    return 2.0 * s_w


def cap_share(s_w):
    """Share of the DEVICE generator's vertices left outside a strip s_w wide: tries 1..999 are redrawn while outside (each
    passes with 2q), try 1000 is kept whatever it is, so (1 - 2q)^999 vertices reach the cap and (1 - 2q) of those lie outside.
    Returns ((1 - 2q)^999, (1 - 2q)^1000)."""
    q2 = 2.0 * pass_probability(s_w)
    return (1.0 - q2) ** (MAX_TRIES - 1), (1.0 - q2) ** MAX_TRIES


# ---------------------------------------------------------------------------------------------------------------------
# samplers: the reference's algorithm (Mersenne-Twister) and a numpy model of the device's draw with its mutants
# ---------------------------------------------------------------------------------------------------------------------
def reference_polys(n_maps, bounds, width_frac, seed):
    """n_maps worlds' banks by the package's port of gen_river_poly (pinned to the reference by tests/golden/ref_maps.npz),
    one python Mersenne-Twister stream for all of them.  [n_maps, 2, 12, 2]."""
    import random
    from ship_sim_gym_amd import game_map
    rng = random.Random(seed)
    return np.asarray([game_map.gen_river_poly(bounds, width_frac=width_frac, rng=rng) for _ in range(n_maps)], dtype=np.float64)


MUTANTS = ("no_fold", "x_sigma_52", "y_sigma_21", "y_from_cosine", "randint_no_plus_one", "centre_mid_strip")


def device_model_polys(n_maps, width, height, width_frac, seed, mutant=None):
    """The device generator's draw, restated in numpy: per candidate ONE Box-Muller transform, x = centre - |50 r cos|, y from
    r sin, redrawn while x is outside the strip.  `mutant` plants one of MUTANTS.  [n_maps, 2, 12, 2]."""
    assert mutant is None or mutant in MUTANTS
    g = np.random.Generator(np.random.PCG64(seed))
    s_w = strip_width(width, width_frac)
    polys = np.zeros((n_maps, 2, 12, 2))
    xs = X_SIGMA * (1.04 if mutant == "x_sigma_52" else 1.0)
    ys = Y_SIGMA * (1.05 if mutant == "y_sigma_21" else 1.0)
    for s in range(2):
        x_min, x_max = (width - s_w, width) if s else (0.0, s_w)
        centre = 0.5 * (x_min + x_max) if mutant == "centre_mid_strip" else x_min + (x_max - x_min)
        i = np.broadcast_to(np.arange(1, N_SEG + 1, dtype=np.float64), (n_maps, N_SEG)).ravel()
        x, y = np.zeros(n_maps * N_SEG), np.zeros(n_maps * N_SEG)
        todo = np.arange(n_maps * N_SEG)
        for tries in range(1, MAX_TRIES + 1):
            u1, u2 = 1.0 - g.random(len(todo)), g.random(len(todo))
            rad = np.sqrt(-2.0 * np.log(u1))
            cs, sn = np.cos(2.0 * np.pi * u2), np.sin(2.0 * np.pi * u2)
            if mutant == "no_fold":
                cx = np.clip(centre + xs * (rad * cs), x_min, x_max)
            else:
                cx = centre - np.abs(xs * (rad * cs))
            cy = Y_START + (y_delta(height) * i[todo] + ys * (rad * (cs if mutant == "y_from_cosine" else sn)))
            x[todo], y[todo] = cx, cy
            todo = todo[((cx < x_min) | (cx > x_max)) & (tries < MAX_TRIES)]
            if len(todo) == 0:
                break
        polys[:, s, :N_SEG, 0], polys[:, s, :N_SEG, 1] = x.reshape(n_maps, N_SEG), y.reshape(n_maps, N_SEG)
        polys[:, s, N_SEG:] = corners(width, height)[s]
    return polys


def device_model_goals(n_maps, n_goals, width, height, seed, mutant=None):
    """The device's goal draws: randint as lo + ((u32 * span) >> 32), u with 53 random bits.  -> (gy, u, fb), [n_maps, n_goals]."""
    g = np.random.Generator(np.random.PCG64(seed))
    plus = 0 if mutant == "randint_no_plus_one" else 1

    def randint(lo, hi):
        r = g.integers(0, 1 << 32, size=(n_maps, n_goals), dtype=np.uint64)
        return lo + ((r * np.uint64(hi - lo + plus)) >> np.uint64(32)).astype(np.int64)

    i = np.arange(1, n_goals + 1, dtype=np.float64)[None, :]
    gy = (height / (n_goals + 1)) * i + randint(-Y_JITTER, Y_JITTER)
    a = g.integers(0, 1 << 27, size=(n_maps, n_goals), dtype=np.uint64)
    b = g.integers(0, 1 << 26, size=(n_maps, n_goals), dtype=np.uint64)
    u = (a * np.uint64(1 << 26) + b).astype(np.float64) * (1.0 / 9007199254740992.0)
    fb = (width / 2) * i + randint(-X_JITTER, X_JITTER)
    return gy, u, fb


# ---------------------------------------------------------------------------------------------------------------------
# the census, and the record the oracle derives from a world's raw draws
# ---------------------------------------------------------------------------------------------------------------------
# The configurations of the geometry sweep: (width, height, n_goals, width_frac, n_maps).  Every width_frac of
# {0.05, 0.3, 0.5, 0.7, 0.8, 0.97, 1.0} at the default bounds, every n_goals 1..6, a wide and a tall world, every n_maps of
# {1, 63, 65, 4097} (partial last workgroups of the 64-lane generator), 22 517 worlds in all.  What each is FOR:
# * width_frac >= 0.97: the left bank ends within 10 of the mid-line, where every ray starts: hits at alpha 0 (the point
#   query), and right-going rays answered by the LEFT bank.  (The right bank crowds the map's right edge — its centre is
#   x_max too — and never comes near the mid-line of a 600-wide map.)
# * the flat world (40 x 10, six goals): its goal rows, height / 7 * i +- 20, leave the map, so rays pass over or under a bank
#   — beyond the reach of the corner vertices that otherwise put a hull under every ray's end.  It is the only kind of world
#   where a left-going ray can miss the left bank and be answered by the right one, and where a ray can miss both banks
#   (gen_goal_path's fallback arm).  Both banks are within 10 of its mid-line.
SWEEP = (
    (600, 600, 5, 0.05, 65), (600, 600, 5, 0.3, 63), (600, 600, 5, 0.5, 4097), (600, 600, 5, 0.7, 1000), (600, 600, 5, 0.8, 1),
    (600, 600, 5, 0.97, 4097), (600, 600, 5, 1.0, 4097),
    (600, 600, 1, 1.0, 500), (600, 600, 2, 0.97, 500), (600, 600, 3, 0.7, 500), (600, 600, 4, 0.3, 500), (600, 600, 6, 1.0, 1000),
    (1200, 300, 5, 0.7, 1000), (300, 1200, 5, 1.0, 1000), (40, 10, 6, 1.0, 4097),
)
CAP_WIDTH_FRAC = 4e-5   # the try-cap run: at width 600 a strip 0.012 wide, 83 % of the vertices reach try 1000


def corners_within_reach(height, n_goals):
    """True where every goal row lies in [-10, height + 10]: gy_delta * i +- 20 with gy_delta = height / (n_goals + 1) >= 10.
    The ray's far end (edge, y) is then within 10 of that side's corner edge (edge, 0)-(edge, height), and a fat ray that
    reaches a convex hull from outside hits it: no ray of such a world misses, and the left bank answers every left-going one."""
    return height / (n_goals + 1) >= 10.0


RAY_CLASSES =("alpha0", "edge", "vertex", "left_by_right", "right_by_left", "box_miss")


class Census:
    """Counts over worlds: rays by how they were answered, (ray, bank) queries by how they missed, hulls by vertex count."""

    def __init__(self):
        self.rays = collections.Counter()
        self.hulls = collections.Counter()
        self.worlds = 0

    def add(self, other):
        self.rays.update(other.rays)
        self.hulls.update(other.hulls)
        self.worlds += other.worlds
        return self

    def shortfalls(self, need=50, hull_kinds=4):
        short = ["%s: %d < %d" % (k, self.rays[k], need) for k in RAY_CLASSES if self.rays[k] < need]
        if len(self.hulls) < hull_kinds:
            short.append("hull vertex counts seen: %s" % sorted(self.hulls))
        return short

    def __str__(self):
        return "%d worlds; rays: %s; hull vertex counts: %s" % (
            self.worlds, ", ".join("%s %d" % (k, self.rays[k]) for k in RAY_CLASSES + ("box_pass_miss", "ray_miss")),
            ", ".join("%d: %d" % kv for kv in sorted(self.hulls.items())))


def census_world(O, world, polys, goal_ys, width, census):
    """Walk one world's goal path under the oracle alone.  `world`: an oracle.World of the world's width / height (its banks are
    replaced here); polys [2, 12, 2]; goal_ys: the goal rows.  Every ray — left-going, then right-going, per goal — asks the
    left bank first and the right one on a miss (ora_goal_x_range's order, and game.py:322-323 [0] with one hit per ray).
    Counted per RAY: the answering hit's kind — `alpha0` (the start lies within 10 of the hull: reported normal from the point
    query), `edge` (the reported normal IS one of the hull's edge normals) or `vertex` (a vertex circle's) — and
    `left_by_right` / `right_by_left` when the left-going ray was answered by the right bank / the right-going one by the left
    bank; `ray_miss` when neither bank answered.  Counted per QUERY that missed: `box_miss` (the ray's box widened by 10 does not
    meet the hull's box: the kernel's early-out), `box_pass_miss` otherwise.  Returns per goal (hit, lo, hi), World.goal_x_range's
    answer, checked here against the two answering hits' points."""
    polys = np.asarray(polys, dtype=np.float64)
    banks = [O.make_poly(polys[0]), O.make_poly(polys[1])]
    for s in range(2):
        n = len(O.convex_hull(polys[s]))
        assert n == banks[s].count
        census.hulls[n] += 1
    world.set_banks_only(polys[0], polys[1])
    census.worlds += 1
    r2, xm, out = RAY_RADIUS, width / 2, []
    for y in goal_ys:
        y = float(y)
        pts = []
        for ray, bx in enumerate((0.0, float(width))):
            answered = None
            for k in range(2):
                p = banks[k]
                hit, point, normal, alpha = O.segment_query(p, (xm, y), (bx, y), r2)
                if hit:
                    answered = (k, point, normal, alpha)
                    break
                boxed = max(xm, bx) + r2 < p.bb_l or min(xm, bx) - r2 > p.bb_r or y + r2 < p.bb_b or y - r2 > p.bb_t
                census.rays["box_miss" if boxed else "box_pass_miss"] += 1
            if answered is None:
                census.rays["ray_miss"] += 1
                pts.append(None)
                continue
            k, point, normal, alpha = answered
            p = banks[k]
            if alpha == 0.0:
                kind = "alpha0"
            elif any(normal == (p.wn[j].x, p.wn[j].y) for j in range(p.count)):
                kind = "edge"
            else:
                kind = "vertex"
            census.rays[kind] += 1
            if k != ray:
                census.rays["left_by_right" if ray == 0 else "right_by_left"] += 1
            pts.append(point[0])
        ok, lo, hi = world.goal_x_range(y)
        assert ok == (pts[0] is not None and pts[1] is not None)
        if ok:
            assert lo == pts[0] + TOLERANCE and hi == pts[1] - TOLERANCE
        out.append((ok, lo, hi))
    return out


def oracle_record(O, N, world, polys, goal_raw, width, spawn, census):
    """The map-bank record (N.MAP_STRIDE doubles) the ORACLE derives from one world's raw draws: polys [2, 12, 2] and goal_raw
    [n_goals, 3] = (y, u, fallback x) per goal.  cpConvexHull order, cpPolyShapeSetVerts planes, cpPolyShapeCacheData boxes,
    gen_goal_path's x = lo + (hi - lo) u (np.random.uniform's arithmetic) or the fallback, ShipEnv's nearest goal to the spawn
    point (first minimum).  Unused slots and the pad double stay zero."""
    rec = np.zeros(N.MAP_STRIDE)
    for s in range(2):
        p = O.make_poly(polys[s])
        hull = O.convex_hull(polys[s])
        n = p.count
        rec[N.MAP_OFF_COUNTS + s] = n
        rec[N.MAP_OFF_AABB + 4 * s: N.MAP_OFF_AABB + 4 * s + 4] = (p.bb_l, p.bb_b, p.bb_r, p.bb_t)
        for j in range(n):
            assert (p.lv[j].x, p.lv[j].y) == (hull[j, 0], hull[j, 1])
            o = N.MAP_OFF_PLANES + (s * N.MAX_HULL + j) * N.PLANE_DOUBLES
            nx, ny = p.ln[j].x, p.ln[j].y  # (the body sits at the origin unrotated: the LOCAL normals, whose zeros keep their sign)
            rec[o: o + 5] = (hull[j, 0], hull[j, 1], nx, ny, hull[j, 0] * nx + hull[j, 1] * ny)
    goal_raw = np.asarray(goal_raw, dtype=np.float64).reshape(-1, 3)
    ranges = census_world(O, world, polys, goal_raw[:, 0], width, census)
    best = None
    for i, ((ok, lo, hi), (y, u, fb)) in enumerate(zip(ranges, goal_raw)):
        x = lo + (hi - lo) * u if ok else fb
        rec[N.MAP_OFF_GOALS + 2 * i: N.MAP_OFF_GOALS + 2 * i + 2] = (x, y)
        dx, dy = x - spawn[0], y - spawn[1]
        d = math.sqrt(dx * dx + dy * dy)
        if best is None or d < best:
            best = d
            rec[N.MAP_OFF_SPAWN_GOAL: N.MAP_OFF_SPAWN_GOAL + 2] = (x, y)
    return rec
