"""Lidar scenes at the decision boundaries of cpPolyShapeSegmentQuery, and an exact classifier of their beams.

A scene is one env: a bank record (two hull polygons of 12 points) and a player pose (x, y, angle) for each of two steps.
Hull features (vertices, edges, planes, AABB extents) are placed relative to one chosen beam of the pose, at signed offsets
from the decision boundary, for the families of the lidar issue: vertex, parallel, end_on_edge, origin_on_plane, inside,
first_shape, planes (plane counts), cull (AABB x extent), sticky.

classify() recomputes every predicate of ora_poly_segment_query (oracle/ssg_oracle.c) in exact rational arithmetic from the
oracle's own f64 inputs (lidar origin, beam end, hull planes).  A beam is CLEAR when every predicate that decides it holds by a
margin of at least 1e-12 x the coordinate scale (6e-10), and BAND otherwise; a band beam comes with every reading it may legitimately
show: a hit reading of each hull plane (or the far end for an origin inside a hull) that might decide it, and the previous
(sticky) reading when every hull may miss.
"""
import math
from fractions import Fraction as Fr

import numpy as np

W = H = 600.0
SCALE = 600.0                 # coordinate scale of the scenes
DELTA = 1e-12 * SCALE         # clear / band margin of a predicate: >= 1e3 x its f64 rounding (~1e-13 here) and the HIP path's beam-end
                              # difference (~1e-13, the angle-sum identity), below the kernel's kSignEps = 1e-9 so that origins
                              # 1e-9 .. 2e-9 from a plane are decided, not band
ETA = 1e-12 * SCALE           # bound on the f64 rounding of a plane offset (d = a.n - v0.n), for the readings of band planes
FAR_GOALS = [[-4000.0 - 40.0 * g, -4000.0] for g in range(5)]  # no beam and no ship comes near them
OFFSETS = (1e-6, -1e-6, 1e-9, -1e-9, 1e-12, -1e-12, 0.0)
FAMILIES = ("vertex", "parallel", "end_on_edge", "origin_on_plane", "inside", "first_shape", "planes", "cull", "sticky")


# ---------------------------------------------------------------------------------------------------------------- geometry
def _ngon(cx, cy, rx, ry, k, phase):
    return [(cx + rx * math.cos(phase + 2 * math.pi * i / k), cy + ry * math.sin(phase + 2 * math.pi * i / k)) for i in range(k)]


def pad12(pts):
    """A convex polygon of k <= 12 vertices as the 12 points a bank record holds: the rest are interior points (hulled away)."""
    pts = [tuple(map(float, p)) for p in pts]
    cx = sum(p[0] for p in pts) / len(pts)
    cy = sum(p[1] for p in pts) / len(pts)
    out = list(pts)
    i = 0
    while len(out) < 12:
        p = pts[i % len(pts)]
        f = 0.15 + 0.1 * (i // len(pts))
        out.append((cx + f * (p[0] - cx) + 0.37 * (i + 1), cy + f * (p[1] - cy) - 0.29 * (i + 1)))
        i += 1
    return np.array(out, dtype=np.float64)


def layouts():
    """(name, left 12 points, right 12 points): hull 0 is listed first.  Plane counts 3, 4, 5, 8, 9, 12 on both hulls; banks
    as the game lays them out, swapped (hull 0 the right bank), a hull in mid-river, overlapping hulls, bank corners on (0, 0)
    and (W, 0)."""
    out = []
    pairs = ((3, 12), (4, 9), (5, 8), (8, 5), (9, 4), (12, 3))
    for i, (k0, k1) in enumerate(pairs):
        left = _ngon(110, 300, 75, 190, k0, 0.3 + 0.1 * i)
        right = _ngon(490, 300, 75, 190, k1, 1.1 + 0.1 * i)
        out.append(("banks%d_%d" % (k0, k1), pad12(left), pad12(right)))
        out.append(("swapped%d_%d" % (k0, k1), pad12(_ngon(480, 310, 70, 180, k0, 0.7 + 0.1 * i)),
                    pad12(_ngon(120, 290, 70, 180, k1, 0.2 + 0.1 * i))))
    for k in (3, 8, 12):
        out.append(("mid1_%d" % k, pad12(_ngon(100, 300, 70, 200, 9, 0.4)), pad12(_ngon(300, 300, 45, 60, k, 0.5))))
        out.append(("mid0_%d" % k, pad12(_ngon(300, 300, 45, 60, k, 0.9)), pad12(_ngon(500, 300, 70, 200, 8, 0.1))))
    out.append(("overlap5_8", pad12(_ngon(280, 300, 80, 90, 5, 0.2)), pad12(_ngon(330, 310, 80, 90, 8, 0.6))))
    out.append(("overlap12_4", pad12(_ngon(300, 280, 70, 70, 12, 0.0)), pad12(_ngon(300, 330, 90, 50, 4, 0.3))))
    # bank corners exactly on (0, 0) and (W, 0), as the game's banks have them
    out.append(("corners", pad12([(0.0, 0.0), (150.0, 0.0), (190.0, 250.0), (120.0, 600.0), (0.0, 600.0)]),
                pad12([(W, 0.0), (W, 600.0), (470.0, 600.0), (400.0, 300.0), (450.0, 0.0)])))
    out.append(("corners_hi", pad12([(0.0, 0.0), (90.0, 0.0), (160.0, 300.0), (0.0, 420.0)]),
                pad12([(W, 0.0), (W, 500.0), (430.0, 200.0), (510.0, 0.0)])))
    return out


class Hull:
    """The oracle's cpPolyShape of 12 record points: count, world vertices v0 and normals n of the splitting planes."""

    def __init__(self, O, pts12):
        p = O.make_poly(pts12)
        self.count = p.count
        self.v = [(p.wv[j].x, p.wv[j].y) for j in range(p.count)]
        self.n = [(p.wn[j].x, p.wn[j].y) for j in range(p.count)]
        self.bb = (min(x for x, _ in self.v), min(y for _, y in self.v), max(x for x, _ in self.v), max(y for _, y in self.v))
        self.fv = [(Fr(x), Fr(y)) for x, y in self.v]
        self.fn = [(Fr(x), Fr(y)) for x, y in self.n]

    def centroid(self):
        return sum(x for x, _ in self.v) / self.count, sum(y for _, y in self.v) / self.count

    def edge(self, j):
        """plane j's edge: v[j-1] -> v[j], its unit outward normal"""
        return self.v[j - 1], self.v[j], self.n[j]


# ------------------------------------------------------------------------------------------------------------------- beams
class Lidar:
    """LiDAR.query's beams (models.py:39-76) in the oracle's own f64 operations (oracle/ssg_oracle.c lidar_query)."""

    def __init__(self, O, n_beams, spread=90.0, dist=100.0):
        self.nb, self.spread, self.dist = n_beams, spread, dist
        self.d2r = math.pi / 180.0
        self.delta = (spread / n_beams) * self.d2r
        self.w = O.World(O.default_config(n_beams=n_beams))
        self.w.set_banks_only(pad12(_ngon(-900, -900, 5, 5, 4, 0)), pad12(_ngon(-800, -900, 5, 5, 4, 0)))

    def origin(self, x, y, a):
        self.w.place_player(x, y, a)
        return self.w.lidar_origin()

    def rotation(self, a, i):
        return (a + (90 - self.spread / 2) * self.d2r) + (self.delta * i)

    def beams(self, x, y, a):
        cx, cy = self.origin(x, y, a)
        out = []
        for i in range(self.nb):
            r = self.rotation(a, i)
            out.append(((cx, cy), (cx + self.dist * math.cos(r), cy + self.dist * math.sin(r))))
        return out

    def pose_for(self, c, theta, i, exact=False):
        """A pose whose beam i starts at (about, or with exact=True exactly) the point c and points along theta."""
        a = theta - (90 - self.spread / 2) * self.d2r - self.delta * i
        hx, hy = self.origin(0.0, 0.0, a)
        x, y = c[0] - hx, c[1] - hy
        for _ in range(4):
            ox, oy = self.origin(x, y, a)
            if (ox, oy) == tuple(c):
                break
            x, y = x - (ox - c[0]), y - (oy - c[1])
        if exact:  # best effort: a few ulps around, for an origin exactly on the point (not every point is reachable)
            for dx in range(-3, 4):
                for dy in range(-3, 4):
                    xx = float(np.nextafter(x, np.sign(dx) * np.inf)) if dx else x
                    yy = float(np.nextafter(y, np.sign(dy) * np.inf)) if dy else y
                    for _ in range(abs(dx) - 1):
                        xx = float(np.nextafter(xx, np.sign(dx) * np.inf))
                    for _ in range(abs(dy) - 1):
                        yy = float(np.nextafter(yy, np.sign(dy) * np.inf))
                    if self.origin(xx, yy, a) == tuple(c):
                        return xx, yy, float(a)
        return float(x), float(y), float(a)


# ------------------------------------------------------------------------------------------------------------------ scenes
class Scene:
    __slots__ = ("family", "rec", "pose1", "pose2", "beam", "tag")

    def __init__(self, family, rec, pose1, beam, tag, pose2=None):
        self.family, self.rec, self.pose1, self.beam, self.tag = family, rec, pose1, beam, tag
        self.pose2 = pose1 if pose2 is None else pose2


def _unit(t):
    return math.cos(t), math.sin(t)


def _ang(u):
    return math.atan2(u[1], u[0])


def build_scenes(O, n_beams, seed=0):
    """Every family over the layouts; returns (layouts, hulls [R][2], scenes) with the scenes in a fixed random order (families
    interleaved inside every wave of 64 envs)."""
    rng = np.random.RandomState(seed)
    lay = layouts()
    hulls = [(Hull(O, l), Hull(O, r)) for _, l, r in lay]
    lid = Lidar(O, n_beams)
    L = lid.dist
    sc = []
    k = 0  # round-robin over the beams that carry the scene

    def beam_i():
        nonlocal k
        k += 1
        return (k * 7 + 3) % n_beams

    def add(fam, rec, c, theta, tag, exact=False, pose2=None):
        i = beam_i()
        sc.append(Scene(fam, rec, lid.pose_for(c, theta, i, exact), i, tag, pose2))
        return sc[-1]

    for r, (name, _, _) in enumerate(lay):
        for s in (0, 1):
            h = hulls[r][s]
            n = h.count
            # 1. a beam through a hull vertex: left of it, right of it, exactly through it
            for j in (r % n, (r + n // 2) % n):
                v = h.v[j]
                n0, n1 = h.n[j], h.n[(j + 1) % n]
                bis = (n0[0] + n1[0], n0[1] + n1[1])
                u = _unit(_ang((-bis[0], -bis[1])) + rng.uniform(-0.35, 0.35))
                p = (-u[1], u[0])
                dist = rng.uniform(35, 70)
                for off in OFFSETS:
                    c = (v[0] - dist * u[0] + off * p[0], v[1] - dist * u[1] + off * p[1])
                    add("vertex", r, c, _ang(u), "%s h%d v%d off=%g" % (name, s, j, off))
            # 2. a beam parallel to an edge, outside and inside its line, at 0 and +-1e-15 rad
            j = (r + 1 + s) % n
            a0, a1, nn = h.edge(j)
            ed = (a1[0] - a0[0], a1[1] - a0[1])
            th = _ang(ed) + (math.pi if (r + s) % 2 else 0.0)
            start = a0 if (r + s) % 2 == 0 else a1
            u = _unit(th)
            for hh in (1e-6, 1e-9, 0.0, -1e-9, -1e-6, 2e-2):
                for dth in ((0.0, 1e-15, -1e-15) if hh in (0.0, 1e-9) else (((r + s) % 3 - 1) * 1e-15,)):
                    c = (start[0] - 10 * u[0] + hh * nn[0], start[1] - 10 * u[1] + hh * nn[1])
                    add("parallel", r, c, th + dth, "%s h%d e%d h=%g dth=%g" % (name, s, j, hh, dth))
            # 3. a beam whose end is on an edge, just short of it, just past it (t = 1)
            j = (r + 2 + s) % n
            a0, a1, nn = h.edge(j)
            tau = rng.uniform(0.3, 0.7)
            P = (a0[0] + tau * (a1[0] - a0[0]), a0[1] + tau * (a1[1] - a0[1]))
            u = _unit(_ang((-nn[0], -nn[1])) + rng.uniform(-0.6, 0.6))
            for off in OFFSETS:
                c = (P[0] + off * u[0] - L * u[0], P[1] + off * u[1] - L * u[1])
                add("end_on_edge", r, c, _ang(u), "%s h%d e%d off=%g" % (name, s, j, off))
            # 4. an origin at a distance from a plane: on the edge, on its extension beyond the extent; into / away from the hull
            j = (r + 3 + s) % n
            a0, a1, nn = h.edge(j)
            for tau in ((0.5, -0.3) if (r + s) % 2 else (0.5, 1.25)):
                P = (a0[0] + tau * (a1[0] - a0[0]), a0[1] + tau * (a1[1] - a0[1]))
                for hh in sorted(set((0.0, 1e-10, -1e-10, 1e-9, -1e-9, 2e-9, -2e-9, 1e-6, -1e-6)[(r + s) % 2::2] + (0.0, 1e-9, -1e-9))):
                    for into in (True, False):
                        if not into and tau != 0.5:
                            continue
                        th = _ang((-nn[0], -nn[1]) if into else nn) + rng.uniform(-0.5, 0.5)
                        c = (P[0] + hh * nn[0], P[1] + hh * nn[1])
                        add("origin_on_plane", r, c, th, "%s h%d e%d tau=%g d=%g %s" % (name, s, j, tau, hh, "in" if into else "out"))
            # 7. plane counts: beams from outside at the hull's middle, one per edge (the chunk boundaries of the plane loops)
            cx, cy = h.centroid()
            for j in range(0, n, max(1, n // 6)):
                a0, a1, nn = h.edge(j)
                P = ((a0[0] + a1[0]) / 2, (a0[1] + a1[1]) / 2)
                u = _unit(_ang((-nn[0], -nn[1])) + rng.uniform(-0.4, 0.4))
                dist = rng.uniform(20, 90)
                add("planes", r, (P[0] - dist * u[0], P[1] - dist * u[1]), _ang(u), "%s h%d n=%d e%d" % (name, s, n, j))
                # and one that ends within the vertex's rounding at the end of the edge
                add("planes", r, (a1[0] - L * u[0], a1[1] - L * u[1]), _ang(u), "%s h%d n=%d v%d end" % (name, s, n, j))
            # 8. a beam end within 1e-6 of the hull's x extent (the cull's widened box)
            if s == 0:
                xe = h.bb[2]
                jv = max(range(n), key=lambda q: h.v[q][0])
                sgn = 1.0
            else:
                xe = h.bb[0]
                jv = min(range(n), key=lambda q: h.v[q][0])
                sgn = -1.0
            v = h.v[jv]
            for g in ((0.0, 0.5) if (r + s) % 2 else (0.0, -0.5)):
                for off in (1e-6, -1e-6, 1e-9, -1e-9, 0.0):
                    b = (xe + sgn * off, v[1] + g)
                    th = (math.pi if s == 0 else 0.0) + rng.uniform(-0.7, 0.7)
                    u = _unit(th)
                    add("cull", r, (b[0] - L * u[0], b[1] - L * u[1]), th, "%s h%d x-extent g=%g off=%g" % (name, s, g, off))
            # 5. origin inside the hull
            for q in range(3):
                th = rng.uniform(-math.pi, math.pi)
                add("inside", r, (cx + rng.uniform(-5, 5), cy + rng.uniform(-5, 5)), th, "%s h%d inside" % (name, s))
            # 9. sticky: a clear hit, then a pose whose beam misses everything (and back), on both hulls
            j = (r + 4 + s) % n
            a0, a1, nn = h.edge(j)
            P = ((a0[0] + a1[0]) / 2, (a0[1] + a1[1]) / 2)
            u = _unit(_ang((-nn[0], -nn[1])))
            hit_c = (P[0] - 50 * u[0], P[1] - 50 * u[1])
            far = (P[0] + 150 * nn[0], P[1] + 150 * nn[1])  # outward, away from the hull: the beam points further out
            i = beam_i()
            hit_pose = lid.pose_for(hit_c, _ang(u), i)
            miss_pose = lid.pose_for(far, _ang(nn), i)
            short_pose = lid.pose_for((P[0] - L * u[0], P[1] - L * u[1]), _ang(u), i)  # ends on the edge: band
            sc.append(Scene("sticky", r, hit_pose, i, "%s h%d hit->miss" % (name, s), miss_pose))
            sc.append(Scene("sticky", r, miss_pose, i, "%s h%d miss->hit" % (name, s), hit_pose))
            sc.append(Scene("sticky", r, hit_pose, i, "%s h%d hit->edge" % (name, s), short_pose))
        # 6. first listed shape: one beam through both hulls (hull 1 nearer where the layout allows), one hull hit at distance 0
        h0, h1 = hulls[r]
        c0, c1 = h0.centroid(), h1.centroid()
        dx, dy = c0[0] - c1[0], c0[1] - c1[1]
        dd = math.hypot(dx, dy)
        if dd < 150:
            u = (dx / dd, dy / dd)
            for q in range(4):
                back = rng.uniform(0, 40)
                c = (c1[0] - back * u[0], c1[1] - back * u[1])
                add("first_shape", r, c, _ang(u) + rng.uniform(-0.2, 0.2), "%s both hulls" % name)
            for q in range(3):
                c = (c0[0] - back * u[0] - rng.uniform(0, 30), c0[1] - back * u[1])
                add("first_shape", r, c, _ang(u) + rng.uniform(-0.2, 0.2), "%s both hulls (1)" % name)
        for s in (0, 1):
            h = hulls[r][s]
            for jv in range(0, h.count, 2):
                v = h.v[jv]
                for th in (0.3, 1.9, -2.2):
                    add("first_shape", r, v, th, "%s h%d origin on vertex %d" % (name, s, jv), exact=True)
        if name.startswith("corners"):
            for c in ((0.0, 0.0), (W, 0.0)):
                for th in (-0.4, 0.0, 0.5, 1.5707963267948966, 2.5, math.pi, -2.0):
                    add("inside", r, c, th, "%s origin on corner %r" % (name, c), exact=True)
    order = rng.permutation(len(sc))
    return lay, hulls, [sc[i] for i in order]


# -------------------------------------------------------------------------------------------------------------- classifier
CLEAR, BAND = "clear", "band"


def _sgn(x, m=DELTA):
    return 1 if x >= m else (-1 if x <= -m else 0)


def _sqrt_once(q):
    """sqrt of a non-negative Fraction, rounded once to f64 (the floor of a 2^-160-scaled integer root is far below an ulp)"""
    if q == 0:
        return 0.0
    s = math.isqrt((q.numerator << 320) // q.denominator)
    return float(Fr(s, 1 << 160))


def _sg(f, exact):
    """_sgn of a predicate value: its f64 evaluation f (error < 1e-12 here) decides far from the thresholds +-DELTA, the exact
    rational value exact() near them"""
    if f >= 2 * DELTA:
        return 1
    if f <= -2 * DELTA:
        return -1
    if abs(f) <= 0.5 * DELTA:
        return 0
    return _sgn(float(exact()))


def _pair(a, b, h, lenf):
    """One (beam, hull) pair: (clear, hits [(lo, hi)], can_miss)."""
    bl, bb, br, bt = h.bb
    if (max(a[0], b[0]) < bl - 2 * DELTA or min(a[0], b[0]) > br + 2 * DELTA or max(a[1], b[1]) < bb - 2 * DELTA
            or min(a[1], b[1]) > bt + 2 * DELTA):
        return True, [], True  # the segment's box is clearly disjoint from the hull's: a clear miss
    ax, ay, bx, by = Fr(a[0]), Fr(a[1]), Fr(b[0]), Fr(b[1])
    n = h.count
    # cpPolyShapePointQuery's sign test: n.(a - v0) > 0 for some plane = outside
    ex_d = [(lambda j=j: h.fn[j][0] * (ax - h.fv[j][0]) + h.fn[j][1] * (ay - h.fv[j][1])) for j in range(n)]
    sd = [_sg(h.n[j][0] * (a[0] - h.v[j][0]) + h.n[j][1] * (a[1] - h.v[j][1]), ex_d[j]) for j in range(n)]
    if max(sd) == 1:
        pq = -1
    elif min(sd) == max(sd) == -1:
        return True, [(lenf - 1e-12, lenf + 1e-12)], False  # inside: a hit at alpha 0 whose reported point is the far end
    else:
        pq = 0
    acc, band = [], []
    for j in range(n):
        if sd[j] == -1:
            continue
        nx, ny = h.fn[j]
        vx, vy = h.fv[j]
        px, py = h.fv[j - 1]
        d = ex_d[j]()
        den = nx * (ax - bx) + ny * (ay - by)
        e = den - d
        dtmin = nx * py - ny * px
        dtmax = nx * vy - ny * vx
        # the edge-extent predicates as the vertices' distances from the beam's line (dt - dt_min scaled by sin of the angle
        # between beam and edge): f64 errors of t and the lerp scale with 1/sin as the margin does
        k = abs(float(den)) / lenf

        def dt_at(t):
            return nx * (ay + t * (by - ay)) - ny * (ax + t * (bx - ax))

        def dts(t):
            dt = dt_at(t)
            return min(_sgn(float(dt - dtmin) * k), _sgn(float(dtmax - dt) * k))

        se = _sgn(float(e))
        if sd[j] == 1 and se == -1:
            continue
        if sd[j] == 1:
            st = dts(d / den)
            if st == -1:
                continue
            (acc if (se == 1 and st == 1) else band).append((j, d, den))
            continue
        # the origin is within DELTA of the plane: rejected only if the edge test fails, on the same side, at every t the f64
        # path can reach
        if float(den) >= DELTA:
            t1 = (max(d, 0) + Fr(ETA)) / den
            if dts(Fr(0)) == -1 and dts(t1) == -1 and (dt_at(Fr(0)) < dtmin) == (dt_at(t1) < dtmin):
                continue
        elif float(den) <= -DELTA and dts(Fr(0)) == -1:
            continue
        band.append((j, d, den))
    hits = []
    l2 = (bx - ax) ** 2 + (by - ay) ** 2
    for (j, d, den) in acc:
        t = d / den
        r = _sqrt_once(t * t * l2)
        w = 1e-12 + 2e-12 * (lenf + r) / float(den)  # the f64 evaluation's rounding: ~1e-13 on d and den, amplified by 1/den
        hits.append((r - w, r + w))
    for (j, d, den) in band:
        if float(den) >= 2 * ETA:
            lo = min(max((d - Fr(ETA)) / den, Fr(0)), Fr(1))
            hi = min(max((d + Fr(ETA)) / den, Fr(0)), Fr(1))
            hits.append((float(lo) * lenf, float(hi) * lenf))
        else:
            hits.append((0.0, lenf))
    if pq == 0:
        hits.append((lenf - 1e-12, lenf + 1e-12))
    clear = pq != 0 and not band and len(acc) <= 1
    return clear, hits, not acc


def classify_beam(a, b, hull_pair):
    """(clear, candidates): candidates are reading intervals (lo, hi), plus None for 'the previous reading' (every hull may
    miss: lidar_vals[i] is sticky)."""
    lenf = _sqrt_once((Fr(b[0]) - Fr(a[0])) ** 2 + (Fr(b[1]) - Fr(a[1])) ** 2)
    clear, cands = True, []
    for h in hull_pair:
        c, hits, can_miss = _pair(a, b, h, lenf)
        clear &= c
        cands += hits
        if not can_miss:
            return clear, cands
    return clear, cands + [None]


def classify_pose(lid, hull_pair, pose):
    return [classify_beam(a, b, hull_pair) for a, b in lid.beams(*pose)]


def accepts(cands, r, prev, tol=1e-9):
    """is reading r one of the candidates (within tol; the previous reading bit for bit)"""
    if r != r or (r == 0.0 and math.copysign(1.0, r) < 0):
        return False
    for c in cands:
        if c is None:
            if r == prev or (r == 0.0 and prev == 0.0):
                return True
        elif c[0] - tol <= r <= c[1] + tol:
            return True
    return False


def expected(cands, prev):
    """the one reading of a clear beam"""
    assert len(cands) == 1
    return prev if cands[0] is None else cands[0][0]


# ------------------------------------------------------------------------------------------------------------- the oracle side
ACTION = 1  # rudder only: no thrust, so a pose written at rest stays put through the step's cpSpaceStep


def bank_arrays(lay):
    polys = np.stack([np.stack([l, r]) for _, l, r in lay])
    goals = np.repeat(np.asarray(FAR_GOALS, dtype=np.float64)[None], len(lay), axis=0)
    return polys, goals


def oracle_config(O, n_beams, history):
    return O.default_config(n_beams=n_beams, history=history)


def run_oracle(O, lay, scenes, n_beams, history):
    """Both steps of every scene on an oracle Batch (no auto-reset).  Returns a dict: obs0 (reset), obs1, obs2 [n, D],
    rew [2, n], done [2, n], flags [2, n, 2] (colliding, goal_reached)."""
    polys, goals = bank_arrays(lay)
    n = len(scenes)
    ob = O.Batch(n, oracle_config(O, n_beams, history), polys, goals, map_ids=np.array([s.rec for s in scenes], dtype=np.int32))
    out = {"obs0": ob.reset()}
    act = np.full(n, ACTION, dtype=np.int32)
    rew, done, flags = [], [], []
    for k, attr in ((1, "pose1"), (2, "pose2")):
        for e, s in enumerate(scenes):
            ob.place_player(e, *getattr(s, attr))
        o, r, d = ob.step(act, auto_reset=False)
        pk = ob.peek_all()
        out["obs%d" % k] = o
        rew.append(r); done.append(d); flags.append(pk[:, 9:11].copy())
    out["rew"], out["done"], out["flags"] = np.stack(rew), np.stack(done), np.stack(flags)
    return out


def lidar_cols(obs, n_beams, history):
    F = 6 + n_beams
    return obs[:, (history - 1) * F + 6:(history - 1) * F + 6 + n_beams]


def classify_scenes(O, lay, hulls, scenes, n_beams):
    """[(step-1 classes, step-2 classes)] per scene; each a list over beams of (clear, candidates)."""
    lid = Lidar(O, n_beams)
    out = []
    for s in scenes:
        c1 = classify_pose(lid, hulls[s.rec], s.pose1)
        c2 = c1 if s.pose2 is s.pose1 else classify_pose(lid, hulls[s.rec], s.pose2)
        out.append((c1, c2))
    return out
