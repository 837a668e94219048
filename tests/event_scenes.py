"""Scenes at the decision boundaries of the step kernel's events (collide_ship, collide_goal, determine_reward, is_done), their
oracle run, and an exact classifier of their predicates.

A scene is one env: a bank record (two hulls and the record's goal centres), a goal mask, a start step count, a player pose
(x, y, angle) and an optional velocity (vx, vy, w).  The player is written once, before the first of K = 4 steps; action 1 (the
rudder only) keeps a ship at rest where it is, so the same pose is judged at every step of a launch.  Features are placed at the
signed offsets lidar_scenes.OFFSETS from the boundary.  Everything is deterministic from one seed.

Families (FAMILIES):
  sat_bank_axis      a ship vertex on a bank edge: bank plane j of hull s decides (every plane of hulls of 3 .. 12 planes)
  sat_ship_axis      a bank vertex q on ship edge i: one of the five ship planes decides
  sat_vertex_vertex  ship vertex on bank vertex: no single feature decides
  sat_contain        ship inside a hull, a small hull inside the ship's box but disjoint, overlapping hulls
  reject             x extents (or y extents) of ship and hull exactly equal, the other extents far apart or touching
  serve              one decisive scene in 1, 2, 63, 64 lanes of a wave (and in the last, partly filled wave), the rest far away
  goal_dist          a goal centre at distance r + offset from the ship's hull, by Voronoi region; the bounding-box reject
  goal_queue         0 .. 25 and all (lane, goal) pairs of a wave near; one reached pair in every queue position
  bounds             x, y at 0, the largest negative number, -0.0, width, the number after width (and height)
  limit              the step count next to max_steps
  precedence         every combination of colliding, goal reached, out of bounds, step limit, no goals left
  approach           a moving ship crosses a bank edge, a goal's rim or a bound in step 0, 1, 2 or 3 of the launch
  exact              angle 0, dyadic coordinates, axis-aligned edges, offsets 0 and +-1 ulp: touching collides

classify_run() judges every (scene, step) from the oracle's f64 inputs of that step, with formulations of its own, in exact rational
arithmetic wherever the answer is within 1e-7 of a boundary (further away the same formulas in f64, whose error is below 1e-11 at
these coordinates, decide; a hull whose box is more than 1 away from the ship's is a miss): two closed convex polygons intersect iff two edges intersect or a vertex of one lies in the other (not SAT over the
stored normals); the squared distance of a point to a closed convex polygon (not the point-query code).  A predicate is CLEAR
when its deciding quantity (separation / penetration; distance - r; distance to the bound) is at least lidar_scenes.DELTA from
zero or when every operation that leads to it is exact (family exact, a bound or the step limit of a ship at rest); BAND
otherwise.
"""
import collections
import math
from fractions import Fraction as Fr

import numpy as np

import lidar_scenes as LS
from dyn_scenes import PARK_SHIPS
from lidar_scenes import DELTA, OFFSETS, _ngon, layouts, pad12

W = H = 600.0
GOAL_R = 5.0
K = 4
ACTION = 1                     # rudder only: no thrust
MAX_STEPS = 1000               # EnvConfig.MAX_STEPS
DAMP = 0.4                     # pow(space.damping, dt), dt = 1
SHIP_PTS = ((0.0, 0.0), (0.0, 30.0), (10.0, 45.0), (20.0, 30.0), (20.0, 0.0))  # models.py:6 SHIP_TEMPLATE x (2, 3)
FAMILIES = ("sat_bank_axis", "sat_ship_axis", "sat_vertex_vertex", "sat_contain", "reject", "serve", "goal_dist", "goal_queue",
            "bounds", "limit", "precedence", "approach", "exact")
BANDED = tuple(f for f in FAMILIES if f not in ("exact", "serve", "limit", "bounds"))  # families that must show both classes
FAR_GOALS = [[-4000.0 - 40.0 * g, -4000.0] for g in range(6)]
# the goal records' centres.  cluster: at the pose P0 = (290, 290, 0) all six are inside the ship's box + r; 0, 1 (coincident) and
# 5 are reached there, 2, 3 and 4 are not; 2 and 4 are mirror images about x = 300
CLUSTER = ((300.0, 310.0), (300.0, 310.0), (291.0, 334.0), (286.0, 286.0), (309.0, 334.0), (304.0, 300.0))
P0 = (290.0, 290.0, 0.0)
# prec: a goal next to each of the four (colliding, out of bounds) poses, one spare
PREC = ((73.0, 310.0), (10.0, 560.0), (10.0, 510.0), (300.0, 300.0), (300.0, 450.0), (450.0, 300.0))
PREC_POSES = {(0, 0): ((295.0, 290.0), 3), (1, 0): ((50.0, 300.0), 0), (0, 1): ((-1.0, 540.0), 1), (1, 1): ((-1.0, 470.0), 2)}
FAR_POSE = (300.0, 60.0, 0.0)  # in the river of every record, far from every goal of the goal records


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _pad_inside(pts):
    """12 record points of a SMALL convex polygon: the rest are shrunk copies (pad12's fixed shifts would leave such a hull)"""
    pts = [tuple(map(float, p)) for p in pts]
    cx, cy = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    out, i = list(pts), 0
    while len(out) < 12:
        p = pts[i % len(pts)]
        f = 0.2 + 0.05 * (i // len(pts))
        out.append((cx + f * (p[0] - cx), cy + f * (p[1] - cy)))
        i += 1
    return np.array(out, dtype=np.float64)


def records(n_goals):
    """[(name, left 12 points, right 12 points, goals [n_goals][2])]: the lidar suite's layouts with goals nobody comes near,
    then rect / rect_h (axis-aligned hulls with edges of power-of-two length: unit normals without rounding), tiny (hulls smaller
    than the ship), cluster and prec (goal records).  A done env is reset onto the next record, whose river is free at the spawn."""
    far = FAR_GOALS[:n_goals]
    out = [(name, l, r, far) for name, l, r in layouts()]
    out.append(("rect", pad12(_rect(0, 0, 64, 512)), pad12(_rect(536, 0, 600, 512)), far))
    out.append(("rect_h", pad12(_rect(128, 128, 256, 160)), pad12(_rect(384, 128, 512, 160)), far))
    out.append(("tiny", _pad_inside(_ngon(200, 300, 2.0, 2.0, 3, 0.4)), np.array(_ngon(400, 300, 2.5, 2.5, 12, 0.2)), far))
    bl, br = out[0][1], out[0][2]
    out.append(("cluster", bl, br, [list(c) for c in CLUSTER[:n_goals]]))
    out.append(("prec", pad12(_rect(0, 100, 60, 500)), pad12(_rect(540, 100, 600, 500)), [list(c) for c in PREC[:n_goals]]))
    return out


def bank_arrays(recs):
    return np.stack([np.stack([l, r]) for _, l, r, _ in recs]), np.array([g for _, _, _, g in recs], dtype=np.float64)


class Ship:
    """The player's hull as the oracle holds it: local vertices lv and normals ln (plane i = edge lv[i-1] -> lv[i]), and its
    world vertices at a pose in the oracle's own operations (cpPolyShapeCacheData on rot = (cos a, sin a))."""

    def __init__(self, O):
        self.O = O
        self.pts = np.array(SHIP_PTS)
        p = O.make_poly(self.pts)
        assert p.count == 5
        self.lv = [(p.lv[i].x, p.lv[i].y) for i in range(5)]
        self.ln = [(p.ln[i].x, p.ln[i].y) for i in range(5)]

    def world(self, x, y, a):
        p = self.O.make_poly(self.pts, (x, y), a)
        return [(p.wv[i].x, p.wv[i].y) for i in range(5)], (p.bb_l, p.bb_b, p.bb_r, p.bb_t)

    def pose_at(self, local, world, a):
        """the pose (x, y, a) that carries the local point onto the world point (to the rounding of one rotation)"""
        c, s = math.cos(a), math.sin(a)
        return world[0] - (local[0] * c - local[1] * s), world[1] - (local[0] * s + local[1] * c), float(a)

    def edge_pt(self, i, tau):
        a, b = self.lv[i - 1], self.lv[i]
        return a[0] + tau * (b[0] - a[0]), a[1] + tau * (b[1] - a[1])

    def cone(self, i):
        """unit bisector of vertex i's normal cone (planes i and i + 1 meet there)"""
        n0, n1 = self.ln[i], self.ln[(i + 1) % 5]
        d = (n0[0] + n1[0], n0[1] + n1[1])
        ll = math.hypot(*d)
        return d[0] / ll, d[1] / ll


def _rot(v, a):
    c, s = math.cos(a), math.sin(a)
    return v[0] * c - v[1] * s, v[0] * s + v[1] * c


def _ang(u):
    return math.atan2(u[1], u[0])


def _ulps(x, k):
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


# ------------------------------------------------------------------------------------------------------------------ scenes
class Scene:
    __slots__ = ("family", "tag", "rec", "pose", "vel", "mask", "steps0", "target", "meta")

    def __init__(self, family, tag, rec, pose, target, vel=(0.0, 0.0, 0.0), mask=None, steps0=0, **meta):
        self.family, self.tag, self.rec, self.pose, self.vel = family, tag, rec, tuple(map(float, pose)), tuple(map(float, vel))
        self.mask, self.steps0, self.target, self.meta = mask, steps0, target, meta

    def copy(self, family, tag, **kw):
        s = Scene(family, tag, self.rec, self.pose, self.target, self.vel, self.mask, self.steps0, **self.meta)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    @property
    def at_rest(self):
        return self.vel == (0.0, 0.0, 0.0)


class Builder:
    def __init__(self, O, n_goals, seed):
        self.O, self.ng = O, n_goals
        self.full = (1 << n_goals) - 1
        self.rng = np.random.RandomState(seed)
        self.recs = records(n_goals)
        self.R = {name: i for i, (name, _, _, _) in enumerate(self.recs)}
        self.hulls = [(LS.Hull(O, l), LS.Hull(O, r)) for _, l, r, _ in self.recs]
        self.ship = Ship(O)
        self.n_lay = len(layouts())
        self.k = 0

    def off(self):
        self.k += 1
        return OFFSETS[self.k % len(OFFSETS)]

    # ---- placements: each returns a pose
    def vertex_on_bank_edge(self, h, j, i, off, tau=None, jit=None):
        """ship vertex i at distance off outside plane j of hull h, above the edge's interior; the vertex's cone faces the edge"""
        a0, a1, n = h.edge(j)
        tau = self.rng.uniform(0.3, 0.7) if tau is None else tau
        jit = self.rng.uniform(-0.2, 0.2) if jit is None else jit
        a = _ang((-n[0], -n[1])) - _ang(self.ship.cone(i)) + jit
        P = (a0[0] + tau * (a1[0] - a0[0]) + off * n[0], a0[1] + tau * (a1[1] - a0[1]) + off * n[1])
        return self.ship.pose_at(self.ship.lv[i], P, a)

    def bank_vertex_on_ship_edge(self, h, q, i, off, a=None, tau=None):
        """hull vertex q at distance off outside ship plane i, above the edge's interior; without a: the hull vertex's cone faces
        the ship edge"""
        n0, n1 = h.n[q], h.n[(q + 1) % h.count]
        if a is None:
            a = _ang((-(n0[0] + n1[0]), -(n0[1] + n1[1]))) - _ang(self.ship.ln[i]) + self.rng.uniform(-0.1, 0.1)
        N = _rot(self.ship.ln[i], a)
        pl = self.ship.edge_pt(i, self.rng.uniform(0.3, 0.7) if tau is None else tau)
        return self.ship.pose_at(pl, (h.v[q][0] - off * N[0], h.v[q][1] - off * N[1]), a)

    def vertex_on_vertex(self, h, q, i, off):
        """ship vertex i at offset off from hull vertex q along the hull vertex's bisector, the two cones facing each other; a
        negative offset is scaled so that the penetration depth (the least overlap over the four planes that meet there) is -off"""
        n0, n1 = h.n[q], h.n[(q + 1) % h.count]
        u = (n0[0] + n1[0], n0[1] + n1[1])
        ll = math.hypot(*u)
        u = (u[0] / ll, u[1] / ll)
        a = _ang((-u[0], -u[1])) - _ang(self.ship.cone(i)) + self.rng.uniform(-0.05, 0.05)
        if off < 0:
            axes = [n0, n1] + [tuple(-c for c in _rot(self.ship.ln[m], a)) for m in (i, (i + 1) % 5)]
            off = off / min(u[0] * ax[0] + u[1] * ax[1] for ax in axes)
        return self.ship.pose_at(self.ship.lv[i], (h.v[q][0] + off * u[0], h.v[q][1] + off * u[1]), a)

    def goal_pose(self, c, kind, i, off, a):
        """the pose at angle a that puts the goal centre c at signed distance r + off from the hull (kind edge / vertex /
        extension), at signed distance off from edge i (inside), or on vertex i (on_vertex)"""
        sh = self.ship
        if kind == "edge":
            pl, n = sh.edge_pt(i, self.rng.uniform(0.25, 0.75)), sh.ln[i]
            loc = (pl[0] + (GOAL_R + off) * n[0], pl[1] + (GOAL_R + off) * n[1])
        elif kind == "vertex":
            d = _rot(sh.cone(i), self.rng.uniform(-0.3, 0.3))
            loc = (sh.lv[i][0] + (GOAL_R + off) * d[0], sh.lv[i][1] + (GOAL_R + off) * d[1])
        elif kind == "extension":
            e = (sh.lv[i][0] - sh.lv[i - 1][0], sh.lv[i][1] - sh.lv[i - 1][1])
            ll = math.hypot(*e)
            loc = (sh.lv[i][0] + (GOAL_R + off) * e[0] / ll, sh.lv[i][1] + (GOAL_R + off) * e[1] / ll)
        elif kind == "inside":
            pl, n = sh.edge_pt(i, self.rng.uniform(0.25, 0.75)), sh.ln[i]
            loc = (pl[0] + off * n[0], pl[1] + off * n[1])
        else:
            loc = sh.lv[i]
        return sh.pose_at(loc, c, a)

    # ---- families
    def sat(self):
        out, ship = [], self.ship
        for r in range(self.n_lay):
            name = self.recs[r][0]
            for s in (0, 1):
                h = self.hulls[r][s]
                n = h.count
                if name.startswith(("banks", "swapped")):
                    for j in range(n):
                        i, off = (j + r + s) % 5, self.off()
                        out.append(Scene("sat_bank_axis", "%s h%d plane %d/%d vertex %d off=%g" % (name, s, j, n, i, off), r,
                                         self.vertex_on_bank_edge(h, j, i, off), ("hull", s), s=s, plane=j, vert=i, off=off))
                if not name.startswith(("overlap", "corners")):
                    for m, q in enumerate(sorted({0, n // 2, n - 1})):
                        for rep in range(2):
                            i, off = (q + r + s + rep + m) % 5, self.off()
                            out.append(Scene("sat_ship_axis", "%s h%d vertex %d/%d edge %d off=%g" % (name, s, q, n, i, off), r,
                                             self.bank_vertex_on_ship_edge(h, q, i, off), ("hull", s), s=s, q=q, edge=i, off=off))
                    for q in sorted({1 % n, (n + 1) // 2}):
                        i, off = (q + r + 2 * s) % 5, self.off()
                        out.append(Scene("sat_vertex_vertex", "%s h%d vertex %d/%d ship vertex %d off=%g" % (name, s, q, n, i, off), r,
                                         self.vertex_on_vertex(h, q, i, off), ("hull", s), s=s, q=q, vert=i, off=off))
                # the ship wholly inside the hull (where it fits)
                cx, cy = h.centroid()
                a = self.rng.uniform(-math.pi, math.pi)
                pose = ship.pose_at((10.0, 20.0), (cx, cy), a)
                wv, _ = ship.world(*pose)
                if all(h.n[j][0] * (x - h.v[j][0]) + h.n[j][1] * (y - h.v[j][1]) < -1.0 for x, y in wv for j in range(n)):
                    out.append(Scene("sat_contain", "%s h%d ship inside" % (name, s), r, pose, ("hull", s), s=s, kind="inside"))
            if name.startswith("overlap"):
                c0, c1 = self.hulls[r][0].centroid(), self.hulls[r][1].centroid()
                for t in (0.3, 0.5, 0.7):
                    P = (c0[0] + t * (c1[0] - c0[0]), c0[1] + t * (c1[1] - c0[1]))
                    out.append(Scene("sat_contain", "%s both hulls t=%g" % (name, t), r, ship.pose_at((10.0, 20.0), P, self.rng.uniform(-3, 3)),
                                     ("hull", 0), s=0, kind="both"))
        # a hull smaller than the ship inside the ship's box, next to a bow edge (angle 0): disjoint by the offset
        r = self.R["tiny"]
        for s in (0, 1):
            h = self.hulls[r][s]
            for i in (3, 4):
                N = ship.ln[i]
                q = min(range(h.count), key=lambda m: N[0] * h.v[m][0] + N[1] * h.v[m][1])
                tau = 0.6387 if i == 3 else 0.3613  # where the circle inscribed in the box's empty corner touches the bow edge
                for off in OFFSETS:
                    out.append(Scene("sat_contain", "tiny h%d in the box at bow edge %d off=%g" % (s, i, off), r,
                                     self.bank_vertex_on_ship_edge(h, q, i, off, a=0.0, tau=tau), ("hull", s), s=s, q=q, edge=i, off=off, kind="in_box"))
        return out

    def reject(self):
        out, ship = [], self.ship
        for r in range(self.n_lay):
            name = self.recs[r][0]
            for s in (0, 1):
                h = self.hulls[r][s]
                bl, bb, br, bt = h.bb
                far_y = bb - 70.0
                # x extents equal (and +-1 ulp), y extents far apart: the x-only reject passes, the SAT separates
                for side, x0 in (("ar", br), ("al", al_pose(bl))):
                    u = (0, 1, -1)[(r + s + (side == "al")) % 3]
                    out.append(Scene("reject", "%s h%d x extent %s %+d ulp, y far" % (name, s, side, u), r, (_ulps(x0, u), far_y, 0.0),
                                     ("hull", s), s=s, kind="x_eq_y_far"))
                # the reverse: y extents equal, x extents far apart
                far_x = next(x for x in (br + 30.0, bl - 60.0, br + 70.0, bl - 90.0) if _off_the_parks(x, bt))
                out.append(Scene("reject", "%s h%d y extent top, x far" % (name, s), r, (far_x, _ulps(bt, (r % 3) - 1), 0.0), ("hull", s), s=s,
                                 kind="y_eq_x_far"))
                # x extents within an offset AND touching: the ship's vertical edge on the hull's extreme vertex
                jr = max(range(h.count), key=lambda m: h.v[m][0])
                jl = min(range(h.count), key=lambda m: h.v[m][0])
                for side, q, i in (("right", jr, 0), ("left", jl, 2)):
                    off = self.off()
                    pl = ship.edge_pt(i, self.rng.uniform(0.3, 0.7))
                    N = ship.ln[i]
                    pose = ship.pose_at(pl, (h.v[q][0] - off * N[0], h.v[q][1]), 0.0)
                    out.append(Scene("reject", "%s h%d ship edge %d on the %s-most vertex off=%g" % (name, s, i, side, off), r, pose,
                                     ("hull", s), s=s, q=q, edge=i, off=off, kind="x_touch"))
        return out

    def goal_dist(self):
        out, r = [], self.R["cluster"]
        gi = 0

        def add(kind, i, off, a, tag, extra=0):
            nonlocal gi
            gi += 1
            g = (0, 2, 3, 4, 5, 1)[gi % 6] % self.ng if self.ng > 1 else 0
            out.append(Scene("goal_dist", "%s g%d %s" % (kind, g, tag), r, self.goal_pose(CLUSTER[g], kind, i, off, a), ("goal", g),
                             mask=(1 << g) | extra, g=g, kind=kind, feat=i, off=off))

        for i in range(5):
            for off in OFFSETS:
                add("edge", i, off, self.rng.uniform(-math.pi, math.pi), "edge %d off=%g" % (i, off))
                add("vertex", i, off, self.rng.uniform(-math.pi, math.pi), "vertex %d off=%g" % (i, off))
                add("extension", i, off, self.rng.uniform(-math.pi, math.pi), "edge %d extended off=%g" % (i, off))
        for m, off in enumerate(OFFSETS + (-2.0, -6.0)):
            add("inside", m % 5, off, self.rng.uniform(-math.pi, math.pi), "at %g from edge %d" % (off, m % 5))
            add("inside", (m + 2) % 5, off, 0.0, "at %g from edge %d, angle 0" % (off, (m + 2) % 5))
        for i in range(5):
            add("on_vertex", i, 0.0, 0.0 if i % 2 else self.rng.uniform(-math.pi, math.pi), "vertex %d" % i)
        # the bounding-box reject at equality on its four sides (angle 0, whole numbers): beside an edge the distance is exactly r,
        # beside a corner of the box the pair is near and not reached
        for g in sorted({0, self.ng - 1}):
            gx, gy = CLUSTER[g]
            sides = (("gx-r=sbr", gx - GOAL_R - 20.0, gy - 12.0, 0), ("sbl=gx+r", gx + GOAL_R, gy - 12.0, 0),
                     ("gy-r=sbt", gx - 10.0, gy - GOAL_R - 45.0, 1), ("sbb=gy+r", gx - 8.0, gy + GOAL_R, 1),
                     ("gx-r=sbr corner", gx - GOAL_R - 20.0, gy + 4.0, 0), ("sbl=gx+r corner", gx + GOAL_R, gy - 49.0, 0),
                     ("gy-r=sbt corner", gx + 4.0, gy - GOAL_R - 45.0, 1), ("sbb=gy+r corner", gx - 24.0, gy + GOAL_R, 1))
            for tag, x, y, ax in sides:
                for u in (0, 1, -1):
                    pose = (_ulps(x, u), y, 0.0) if ax == 0 else (x, _ulps(y, u), 0.0)
                    out.append(Scene("goal_dist", "box g%d %s %+d ulp" % (g, tag, u), r, pose, ("goal", g), mask=1 << g, g=g, kind="box"))
        return out

    def near_miss(self, g):
        """a pose at which goal g is inside the ship's box + r and sqrt(32) > r from the hull"""
        return CLUSTER[g][0] + 4.0, CLUSTER[g][1] + 4.0, 0.0

    def goal_queue(self):
        """(interleaved scenes, whole waves)"""
        r, ng, full = self.R["cluster"], self.ng, self.full
        sub = lambda *gs: sum(1 << g for g in set(gs) if g < ng)
        mixed = []
        add = lambda tag, pose, mask, g=0: mixed.append(Scene("goal_queue", tag, r, pose, ("goal", g), mask=mask, g=g, kind="case"))
        add("several goals reached in one step", P0, full)
        add("coincident goals reached", P0, sub(0, 1))
        add("the last listed goal reached", P0, sub(0))
        add("the last two listed goals reached", P0, sub(0, 1))
        add("reached goals masked off beforehand", P0, full & ~sub(0, 1, 5))
        add("no goal listed", P0, 0)
        add("no goal listed, far", FAR_POSE, 0)
        if ng > 3:
            add("the nearest goal reached, another stays listed", (287.0, 287.0, 0.0), sub(0, 3), 3)
            add("the nearest goal reached, all stay listed", (287.0, 287.0, 0.0), full, 3)
        if ng > 4:
            add("two listed goals at the same distance", (300.0, 300.0, 0.0), sub(2, 4), 2)
            add("two listed goals at the same distance, reversed", (300.0, 330.0, 0.0), sub(4, 2), 4)
        waves = []
        lanes = [(7 * i + 3) % 64 for i in range(64)]
        far = lambda tag: Scene("goal_queue", tag + " (far lane)", r, FAR_POSE, None, mask=full, kind="far")

        def filler(tag, g, two=False):
            return Scene("goal_queue", tag, r, self.near_miss(g), None, mask=sub(0, 1) if two else 1 << g, g=g, kind="filler")

        def wave_of(count, tag, pairs=True):
            w = [far(tag) for _ in range(64)]
            left, m = count, 0
            for li, lane in enumerate(lanes):
                if left == 0:
                    break
                two = pairs and ng > 1 and li % 3 == 0 and left >= 2
                g = 0 if two else m % ng
                m += 0 if two else 1
                w[lane] = filler(tag, g, two)
                left -= 2 if two else 1
            assert left == 0
            return w

        for count in (0, 1, 11, 12, 13, 24, 25):
            waves.append(("count %d" % count, wave_of(count, "queue of %d" % count)))
        waves.append(("all", [Scene("goal_queue", "every goal of every lane near", r, P0, None, mask=full, kind="all") for _ in range(64)]))
        reached = (-1e-6, -1e-9, -1e-12, 0.0)
        for pos in range(25):
            w = wave_of(25, "queue of 25, reached at %d" % pos, pairs=False)
            order = queue_order(list(enumerate(w)), ng, self.ship)
            lane, g = order[pos]
            off = reached[pos % 4]
            kind, i = ("edge", "vertex", "extension")[pos % 3], pos % 5
            w[lane] = Scene("goal_queue", "reached pair at queue position %d (pass %d slot %d) off=%g" % (pos, pos // 12, pos % 12, off), r,
                            self.goal_pose(CLUSTER[g], kind, i, off, self.rng.uniform(0.2, 1.3) + (pos % 4) * math.pi / 2), ("goal", g),
                            mask=w[lane].mask, g=g, kind="single", pos=pos, off=off)
            waves.append(("single %d" % pos, w))
        return mixed, waves

    def bounds(self):
        out = []
        tiny = 5e-324
        for name, x, hy in (("mid1_8", 300.0, 550.0), ("mid0_12", 290.0, 520.0)):
            r = self.R[name]
            for v, tag in ((0.0, "0"), (-tiny, "largest negative"), (-0.0, "-0.0"), (tiny, "smallest positive"), (W, "width"),
                           (_ulps(W, 1), "after width"), (_ulps(W, -1), "before width")):
                out.append(Scene("bounds", "%s x = %s" % (name, tag), r, (v, hy, 0.0), ("bound",)))
                out.append(Scene("bounds", "%s y = %s (height)" % (name, tag), r, (x, v, 0.0), ("bound",)))
        return out

    def limit(self):
        out = []
        for m, name in enumerate(("banks3_12", "mid0_3", "rect")):
            for d in (5, 4, 3, 2, 1, 0):
                out.append(Scene("limit", "%s step count max_steps - %d" % (name, d), self.R[name], (300.0 + m, 60.0 + 7 * d, 0.1 * m), ("limit",),
                                 steps0=MAX_STEPS - d))
        return out

    def precedence(self):
        out, r, ng = [], self.R["prec"], self.ng
        spare = 4 if ng > 4 else None
        for (c, o), ((x, y), g) in sorted(PREC_POSES.items()):
            g = g if g < ng else None
            for lim in (0, 1):
                states = [("none listed", 0)]
                if g is not None:
                    states.append(("reached, none left", 1 << g))
                    if spare is not None:
                        states += [("reached, one left", (1 << g) | (1 << spare)), ("not reached", 1 << spare)]
                elif spare is not None:
                    states.append(("not reached", 1 << spare))
                for tag, mask in states:
                    out.append(Scene("precedence", "colliding=%d out=%d limit=%d goal %s" % (c, o, lim, tag), r, (x, y, 0.0),
                                     ("hull", 0) if c else ("bound",) if o else ("limit",), mask=mask, steps0=(MAX_STEPS - 1) * lim, kind="combo",
                                     want=(c, o, lim, tag)))
        # the same table with the collision, and the goal, at the offsets: ship edge 0 on the left bank's edge x = 60 (goal 0 inside
        # the ship), goal 3 at r + off from ship edge 0
        for off in OFFSETS:
            for lim in (0, 1):
                for left in (0, 1):
                    if left and spare is None:
                        continue
                    m0 = (1 << 0) | ((1 << spare) if left else 0)
                    out.append(Scene("precedence", "collision at off=%g limit=%d goal reached, %d left" % (off, lim, left), r, (60.0 + off, 300.0, 0.0),
                                     ("hull", 0), mask=m0, steps0=(MAX_STEPS - 1) * lim, kind="band_c", off=off))
                    if ng > 3:
                        m3 = (1 << 3) | ((1 << spare) if left else 0)
                        out.append(Scene("precedence", "goal at off=%g limit=%d, %d more listed" % (off, lim, left), r,
                                         (PREC[3][0] + GOAL_R + off, 290.0, 0.0), ("goal", 3), mask=m3, steps0=(MAX_STEPS - 1) * lim, kind="band_g",
                                         g=3, off=off))
                    else:
                        out.append(Scene("precedence", "goal 0 at off=%g limit=%d" % (off, lim), r,
                                         (PREC[0][0] + GOAL_R + off, 300.0, 0.0), ("goal", 0), mask=1, steps0=(MAX_STEPS - 1) * lim, kind="band_g",
                                         g=0, off=off))
        return out

    def approach(self):
        """the crossing pose `at` is reached after step + 1 position updates: p0 = at - v (1 + 0.4 + ...), corrected once for rounding"""
        out, ship = [], self.ship

        def start(at, v, step):
            p = [at[0] - v[0] * sum(DAMP ** m for m in range(step + 1)), at[1] - v[1] * sum(DAMP ** m for m in range(step + 1))]
            for _ in range(3):
                q, vv = list(p), list(v)
                for _ in range(step + 1):
                    q = [q[0] + vv[0] * 1.0, q[1] + vv[1] * 1.0]
                    vv = [vv[0] * DAMP + 0.0 * 0.2 * 1.0, vv[1] * DAMP + 0.0 * 0.2 * 1.0]
                p = [p[0] - (q[0] - at[0]), p[1] - (q[1] - at[1])]
            return p

        m = 0
        for step in range(K):
            for off in OFFSETS:
                m += 1
                # a bank edge
                r = (2 * m) % 12
                s = m % 2
                h = self.hulls[r][s]
                j, i = m % h.count, m % 5
                pose = self.vertex_on_bank_edge(h, j, i, off)
                n = h.n[j]
                sp = 2.0 + (m % 3)
                v = (-n[0] * sp, -n[1] * sp)
                p0 = start(pose, v, step)
                out.append(Scene("approach", "%s h%d plane %d crossed in step %d off=%g" % (self.recs[r][0], s, j, step, off), r,
                                 (p0[0], p0[1], pose[2]), ("hull", s), vel=(v[0], v[1], 0.0), s=s, step=step, off=off, kind="bank"))
                # a goal's rim
                g = m % self.ng
                a = self.rng.uniform(-math.pi, math.pi)
                e = m % 5
                pose = self.goal_pose(CLUSTER[g], "edge", e, off, a)
                N = _rot(ship.ln[e], a)
                v = (N[0] * sp, N[1] * sp)
                p0 = start(pose, v, step)
                out.append(Scene("approach", "goal %d rim crossed in step %d off=%g" % (g, step, off), self.R["cluster"], (p0[0], p0[1], a),
                                 ("goal", g), vel=(v[0], v[1], 0.0), mask=1 << g, g=g, step=step, off=off, kind="goal"))
                # a bound
                side = m % 4
                at = ((off, 550.0), (W - off, 550.0), (300.0, off), (300.0, H - off))[side]
                v = ((-sp, 0.0), (sp, 0.0), (0.0, -sp), (0.0, sp))[side]
                p0 = start(at, v, step)
                out.append(Scene("approach", "bound %d crossed in step %d off=%g" % (side, step, off), self.R["mid0_8" if side == 1 else "mid1_8"],
                                 (p0[0], p0[1], 0.0), ("bound",), vel=(v[0], v[1], 0.0), step=step, off=off, kind="bound"))
        for q in range(4):  # a spinning, drifting ship in a hull's reach: the pose of every step is the oracle's
            out.append(Scene("approach", "spinning %d" % q, q, (190.0 + 5 * q, 300.0, 0.3 * q), ("hull", 0), vel=(-2.0, 1.0, 0.2 - 0.1 * q),
                             s=0, kind="spin"))
        return out

    def exact(self):
        out = []
        r1, r2 = self.R["rect"], self.R["rect_h"]
        cases = (("left bank's edge x=64 / ship edge 0", r1, 0, 64.0, 200.0, 0), ("right bank's edge x=536 / ship edge 2", r1, 1, 516.0, 200.0, 0),
                 ("hull 0 top y=160 / ship edge 1", r2, 0, 180.0, 160.0, 1), ("hull 0 bottom y=128 / ship vertex 3", r2, 0, 180.0, 83.0, 1),
                 ("hull 0 right x=256 / ship edge 0", r2, 0, 256.0, 130.0, 0), ("hull 1 left x=384 / ship edge 2", r2, 1, 364.0, 130.0, 0),
                 ("hull 1 top y=160 / ship edge 1", r2, 1, 400.0, 160.0, 1), ("hull 1 bottom y=128 / ship vertex 3", r2, 1, 470.0, 83.0, 1),
                 ("corner (256,160) / ship vertex 0, x", r2, 0, 256.0, 160.0, 0), ("corner (256,160) / ship vertex 0, y", r2, 0, 256.0, 160.0, 1),
                 ("corner (384,160) / ship vertex 1, x", r2, 1, 364.0, 160.0, 0), ("corner (384,160) / ship vertex 1, y", r2, 1, 364.0, 160.0, 1))
        for tag, r, s, x, y, ax in cases:
            for u in (0, 1, -1):
                pose = (_ulps(x, u), y, 0.0) if ax == 0 else (x, _ulps(y, u), 0.0)
                out.append(Scene("exact", "%s %+d ulp" % (tag, u), r, pose, ("hull", s), s=s, ulp=u))
        return out

    def serve(self):
        """(whole waves, the lanes of the last, partly filled wave)"""
        r = self.R["banks12_3"]
        h = self.hulls[r][0]
        poses = [self.bank_vertex_on_ship_edge(h, 11, 3, +1e-6), self.bank_vertex_on_ship_edge(h, 11, 3, -1e-6)]

        def wave(tag, on, width=64):
            w = []
            for lane in range(width):
                if lane in on:
                    v = (lane + len(on)) % 2
                    w.append(Scene("serve", "%s lane %d %s" % (tag, lane, ("separated", "colliding")[v]), r, poses[v], ("hull", 0), s=0, q=11,
                                   edge=3, off=(1e-6, -1e-6)[v], lane=lane, served=True))
                else:
                    w.append(Scene("serve", "%s lane %d far" % (tag, lane), r, (300.0 - lane % 7, 200.0 + lane, 0.02 * lane), ("hull", 0), s=0,
                                   lane=lane, served=False))
            return w

        every = set(range(64))
        waves = [("lane %s" % sorted(on)[:3], wave("%d served" % len(on), on))
                 for on in ({0}, {31}, {32}, {63}, {31, 32}, every - {17}, every)]
        return waves, wave("last wave", {0, 31, 32, 36}, 37)


def _off_the_parks(x, y):
    """is a ship at (x, y, 0) well away from config 4's parked traffic ships (their contact is another suite's)"""
    boxes = [(PARK_SHIPS[k][0], PARK_SHIPS[k][1], PARK_SHIPS[k][0] + w, PARK_SHIPS[k][1] + h) for k, (w, h) in enumerate(((10, 15), (15, 30), (10, 45)))]
    return all(x + 20.0 < l - 8 or x > r + 8 or y + 45.0 < b - 8 or y > t + 8 for l, b, r, t in boxes)


def al_pose(al):
    """an x whose ship (20 wide at angle 0) has its right extent exactly on al, where such an x exists"""
    x = al - 20.0
    for k in (0, 1, -1, 2, -2):
        if _ulps(x, k) + 20.0 == al:
            return _ulps(x, k)
    return x


def box_near(bb, c):
    """cpBBIntersects of the goal's box and the ship's (closed intervals), as collide_goal's reject restates it"""
    return c[0] - GOAL_R <= bb[2] and bb[0] <= c[0] + GOAL_R and c[1] - GOAL_R <= bb[3] and bb[1] <= c[1] + GOAL_R


def queue_order(lane_scenes, n_goals, ship):
    """The (lane, goal) pairs of one wave in the order collide_goal queues them: goal by goal, lanes ascending, a pair being in when
    the goal is listed and its box meets the ship's.  lane_scenes: [(lane, scene)] of one record with CLUSTER goals."""
    out = []
    for g in range(n_goals):
        for lane, s in lane_scenes:
            if not (s.mask >> g) & 1:
                continue
            x, y, a = s.pose
            bb = (x, y, x + 20.0, y + 45.0) if a == 0.0 else ship.world(x, y, a)[1]
            if box_near(bb, CLUSTER[g]):
                out.append((lane, g))
    return out


def build_scenes(O, n_goals, seed=20261017):
    """(records, hulls [R][2], scenes): the interleaved families in a fixed random order filling whole waves (padded with far
    ships), then the waves that goal_queue and serve own, then serve's last, partly filled wave."""
    b = Builder(O, n_goals, seed)
    gq_mixed, gq_waves = b.goal_queue()
    sv_waves, sv_last = b.serve()
    mixed = b.sat() + b.reject() + b.goal_dist() + gq_mixed + b.bounds() + b.limit() + b.precedence() + b.approach() + b.exact()
    order = b.rng.permutation(len(mixed))
    mixed = [mixed[i] for i in order]
    m = 0
    while len(mixed) % 64:
        m += 1
        mixed.append(Scene("limit", "pad %d" % m, (3 * m) % b.n_lay, (300.0, 60.0 + m, 0.0), None))
    scenes = list(mixed)
    for _, w in gq_waves + sv_waves:
        assert len(w) == 64
        scenes += w
    scenes += sv_last
    info = {"mixed": len(mixed), "gq_waves": [(t, len(mixed) + 64 * i) for i, (t, _) in enumerate(gq_waves)],
            "serve_waves": [(t, len(mixed) + 64 * (len(gq_waves) + i)) for i, (t, _) in enumerate(sv_waves)],
            "serve_last": len(scenes) - len(sv_last)}
    for s in scenes:
        if s.mask is None:
            s.mask = b.full
    # config 4 holds the goals as bodies of the env: there every goal_dist scene is moved as a whole, ship and listed goals, by a whole
    # number of its own, so that the goal centres the kernel tests come from the body columns and differ from env to env
    for i, s in enumerate(x for x in scenes if x.family == "goal_dist"):
        s.meta["shift"] = (8.0 * (i % 5 - 2), 8.0 * (i % 3 - 1))
    return b.recs, Hulls(b.hulls), scenes, info


class Hulls(list):
    """[R][2] hulls of the records, with the classifier's memo of the scenes judged on them"""

    def __init__(self, items):
        super().__init__(items)
        self.memo = {}


def dyn_pose(s):
    """config 4: the scene's pose, moved by its shift"""
    dx, dy = s.meta.get("shift", (0.0, 0.0))
    return (s.pose[0] + dx, s.pose[1] + dy, s.pose[2])


def dyn_goal_bodies(s, n_goals):
    """config 4: [(g, x, y)] goal bodies the scene writes (the listed goals of a shifted scene)"""
    if "shift" not in s.meta:
        return []
    dx, dy = s.meta["shift"]
    return [(g, CLUSTER[g][0] + dx, CLUSTER[g][1] + dy) for g in range(n_goals) if (s.mask >> g) & 1]


# ------------------------------------------------------------------------------------------------------------- the oracle side
def oracle_config(O, n_beams, history, n_goals, dyn=False):
    return O.default_config(n_beams=n_beams, history=history, n_goals=n_goals, n_traffic=3 if dyn else 0, max_steps=MAX_STEPS)


def run_oracle(O, recs, scenes, n_beams, history, n_goals, auto_reset, dyn=False, steps=K):
    """Every scene written into an oracle Batch after the reset, then `steps` steps of action 1.  Per step, BEFORE the auto-reset
    of the done envs: peek [n, 19] (pose, step count, colliding, goal_reached, record, cumulative reward, listed goals), goal
    centres [n, n_goals, 2], listed [n] (the goals listed before the step); after it: obs, rew, done.  dyn (config 4): three parked
    traffic ships; a goal the scene does not list leaves the list and the space; shifted scenes write their listed goals' bodies."""
    polys, goals = bank_arrays(recs)
    n = len(scenes)
    ob = O.Batch(n, oracle_config(O, n_beams, history, n_goals, dyn), polys, goals, map_ids=np.array([s.rec for s in scenes], dtype=np.int32))
    out = {"obs0": ob.reset(), "obs": [], "rew": [], "done": [], "peek": [], "goals": [], "listed": [], "after": []}
    for e, s in enumerate(scenes):
        ob.poke_state(e, *((dyn_pose(s) if dyn else s.pose) + s.vel))
        ob.poke_episode(e, s.mask, s.steps0)
        if dyn:
            for k in range(3):
                ob.poke_traffic(e, k, *PARK_SHIPS[k])
            for g, x, y in dyn_goal_bodies(s, n_goals):
                ob.poke_goal(e, g, x, y)
    listed = np.array([s.mask for s in scenes], dtype=np.int64)
    act = np.full(n, ACTION, dtype=np.int32)
    for k in range(steps):
        o, r, d = ob.step(act, auto_reset=False, n_threads=8)
        pk = ob.peek_all()
        if dyn:
            gl = np.stack([ob.peek_dyn(e)["goals"][:n_goals, :2] for e in range(n)])
        else:
            gl = goals[pk[:, 11].astype(np.int64)]
        out["peek"].append(pk); out["goals"].append(gl); out["listed"].append(listed.copy())
        if auto_reset:
            o = ob.auto_reset_done()
        out["obs"].append(o); out["rew"].append(r); out["done"].append(d.copy())
        after = ob.peek_all() if auto_reset else pk
        out["after"].append(after)
        listed = after[:, 13].astype(np.int64)
    for key in ("obs", "rew", "done", "peek", "goals", "listed", "after"):
        out[key] = np.stack(out[key])
    return out


# -------------------------------------------------------------------------------------------------------------- the classifier
CLEAR, BAND = "clear", "band"
_FAST = 1e-7  # an f64 evaluation (error < 1e-11 at these coordinates) decides a quantity at least this far from zero


def _orient(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def _in_poly(p, poly):
    """p in the closed convex polygon (counter-clockwise)"""
    return all(_orient(poly[k - 1], poly[k], p) >= 0 for k in range(len(poly)))


def _on_seg(a, b, p):
    return min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def _segs_meet(a, b, c, d):
    o1, o2, o3, o4 = _orient(a, b, c), _orient(a, b, d), _orient(c, d, a), _orient(c, d, b)
    if ((o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0)) and ((o3 > 0 and o4 < 0) or (o3 < 0 and o4 > 0)):
        return True
    return (o1 == 0 and _on_seg(a, b, c)) or (o2 == 0 and _on_seg(a, b, d)) or (o3 == 0 and _on_seg(c, d, a)) or (o4 == 0 and _on_seg(c, d, b))


def _d2_seg(p, a, b):
    """squared distance of p to the closed segment a b"""
    ex, ey = b[0] - a[0], b[1] - a[1]
    t = ((p[0] - a[0]) * ex + (p[1] - a[1]) * ey) / (ex * ex + ey * ey)
    t = 0 if t < 0 else (1 if t > 1 else t)
    dx, dy = p[0] - (a[0] + t * ex), p[1] - (a[1] + t * ey)
    return dx * dx + dy * dy


def _d2_boundary(p, poly):
    return min(_d2_seg(p, poly[k - 1], poly[k]) for k in range(len(poly)))


def _polys(A, B):
    """(intersect, q2, scale): disjoint: q2 = squared separation, scale 1; intersecting: the penetration is the least, over the
    edges of both, of -min_v m.(v - a) / |m| (m the edge's outward normal, not normalised); returned as that edge's numerator
    squared and |m|^2, so that depth^2 = q2 / scale"""
    meet = any(_in_poly(p, B) for p in A) or any(_in_poly(p, A) for p in B) or \
        any(_segs_meet(A[i - 1], A[i], B[j - 1], B[j]) for i in range(len(A)) for j in range(len(B)))
    if not meet:
        d2 = min(min(_d2_boundary(p, B) for p in A), min(_d2_boundary(p, A) for p in B))
        return False, d2, 1
    best = None
    for P, Q in ((A, B), (B, A)):
        for k in range(len(P)):
            a, b = P[k - 1], P[k]
            m = (b[1] - a[1], -(b[0] - a[0]))
            num = -min(m[0] * (v[0] - a[0]) + m[1] * (v[1] - a[1]) for v in Q)
            mm = m[0] * m[0] + m[1] * m[1]
            num = max(num, 0)
            if best is None or num * num * best[1] < best[0] * mm:
                best = (num * num, mm)
    return True, best[0], best[1]


def _hull_pred(sv, fsv, h, exact):
    """(colliding, clear, signed separation: negative = penetration) of the ship (f64 vertices sv, rational fsv) and hull h"""
    if not exact:
        if sv_box_far(sv, h.bb):
            return False, True, 1.0
        meet, q2, sc = _polys(sv, h.v)
        q = math.sqrt(q2 / sc)
        if q >= _FAST:
            return meet, True, -q if meet else q
    meet, q2, sc = _polys(fsv, h.fv)
    clear = exact or q2 >= Fr(DELTA) ** 2 * sc
    q = math.sqrt(float(q2 / sc))
    return meet, clear, -q if meet else q


def sv_box_far(sv, bb):
    return (max(x for x, _ in sv) < bb[0] - 1.0 or min(x for x, _ in sv) > bb[2] + 1.0 or max(y for _, y in sv) < bb[1] - 1.0
            or min(y for _, y in sv) > bb[3] + 1.0)


def _goal_pred(sv, fsv, c):
    """(reached, clear, signed distance - r)"""
    inside = _in_poly(c, sv)
    d = math.sqrt(_d2_boundary(c, sv))
    q = (-d if inside else d) - GOAL_R
    if abs(q) >= _FAST:
        return q <= 0, True, q
    fc = (Fr(c[0]), Fr(c[1]))
    inside = _in_poly(fc, fsv)
    d2 = _d2_boundary(fc, fsv)
    r2 = Fr(GOAL_R) ** 2
    reached = inside or d2 <= r2
    clear = inside or d2 >= (Fr(GOAL_R) + Fr(DELTA)) ** 2 or d2 <= (Fr(GOAL_R) - Fr(DELTA)) ** 2
    return reached, clear, (-1 if inside else 1) * math.sqrt(float(d2)) - GOAL_R


class Verdict:
    """one (scene, step): hull [(colliding, clear, q)] x 2, goal {g: (reached, clear, q)} of the goals listed before the step, the
    bound (out, clear), and what follows: colliding / reached (value, clear), the listed goals after the step (mask, clear)"""
    __slots__ = ("hull", "goal", "out", "colliding", "reached", "listed")


def classify_step(memo, ship, rec, hulls, pose, goals, listed, exact, at_rest):
    key = (rec, pose, tuple(map(tuple, goals)) if listed else (), listed, exact, at_rest)
    v = memo.get(key)
    if v is not None:
        return v
    sv, _ = ship.world(*pose)
    fsv = [(Fr(x), Fr(y)) for x, y in sv]
    v = Verdict()
    v.hull = [_hull_pred(sv, fsv, h, exact) for h in hulls]
    v.goal = {g: _goal_pred(sv, fsv, (float(goals[g][0]), float(goals[g][1]))) for g in range(len(goals)) if (listed >> g) & 1}
    x, y = pose[0], pose[1]
    v.out = (x < 0 or x > W or y < 0 or y > H, at_rest or min(abs(x), abs(x - W), abs(y), abs(y - H)) >= DELTA)
    hit = [c for c, cl, _ in v.hull if cl and c]
    v.colliding = (any(c for c, _, _ in v.hull), bool(hit) or all(cl for _, cl, _ in v.hull))
    gcl = all(cl for _, cl, _ in v.goal.values())
    v.reached = (any(r for r, _, _ in v.goal.values()), gcl or any(r and cl for r, cl, _ in v.goal.values()))
    v.listed = (listed & ~sum(1 << g for g, (r, _, _) in v.goal.items() if r), gcl)
    memo[key] = v
    return v


def classify_run(O, hulls, scenes, ref):
    """[step][env] Verdict of an oracle run: every (scene, step) from the oracle's inputs of that step (pose, record, goal centres,
    listed goals).  A scene's family and rest state hold up to its first done (after a reset the env is a ship at rest at the
    spawn point).  Scenes judged before on the same Hulls object come from its memo."""
    ship = Ship(O)
    memo = getattr(hulls, "memo", {})
    steps, n = ref["peek"].shape[:2]
    out = []
    fresh = np.zeros(n, dtype=bool)
    for k in range(steps):
        pk = ref["peek"][k]
        row = []
        for e, s in enumerate(scenes):
            pose = (pk[e, 0], pk[e, 1], pk[e, 4])
            row.append(classify_step(memo, ship, int(pk[e, 11]), hulls[int(pk[e, 11])], pose, ref["goals"][k][e], int(ref["listed"][k][e]),
                                     s.family == "exact" and not fresh[e], s.at_rest or fresh[e]))
        out.append(row)
        fresh |= (ref["after"][k][:, 14] != pk[:, 14])
    return out


def target_pred(s, v, steps_after=None):
    """the (value, clear) of the predicate a scene was built for, from its step's Verdict (the step limit: from the oracle's step
    count after the step, whole numbers)"""
    if s.target is None:
        return None
    if s.target[0] == "hull":
        c, cl, _ = v.hull[s.target[1]]
        return c, cl
    if s.target[0] == "goal":
        if s.target[1] not in v.goal:
            return None
        r, cl, _ = v.goal[s.target[1]]
        return r, cl
    if s.target[0] == "bound":
        return v.out
    return (None if steps_after is None else (steps_after >= MAX_STEPS, True))


# --------------------------------------------------------------------------------------------------------- the precedence table
EV_COLLIDING, EV_GOAL_REACHED, EV_OUT_OF_BOUNDS, EV_MAX_STEPS, EV_NO_GOALS_LEFT = 0x1, 0x2, 0x4, 0x8, 0x10


def table(colliding, reached, out, limit, none_left, fix):
    """(reward, done, event flags) of determine_reward (ship_env.py:62-77: the collision branch is overwritten by the chain after
    it, unless fix_collision_reward) and is_done (ship_env.py:115-134)"""
    rew = 1.0 if reached else (-1.0 if out else -0.01)
    if fix and colliding and not reached:
        rew = -1.0
    done = bool(colliding or none_left or out or limit)
    ev = (EV_COLLIDING if colliding else 0) | (EV_GOAL_REACHED if reached else 0) | (EV_OUT_OF_BOUNDS if out else 0) | \
        (EV_MAX_STEPS if limit else 0) | (EV_NO_GOALS_LEFT if none_left else 0)
    return rew, done, ev


def expected(ref, fix, auto_reset):
    """From the oracle's own predicates of every step (peek before the auto-reset): reward [K, n], done, flags, and the cumulative
    reward after the launch, by the precedence table."""
    pk = ref["peek"]
    steps, n = pk.shape[:2]
    rew, done, ev = np.zeros((steps, n)), np.zeros((steps, n), dtype=np.uint8), np.zeros((steps, n), dtype=np.uint8)
    cum = np.zeros(n)
    for k in range(steps):
        for e in range(n):
            p = pk[k, e]
            out = p[0] < 0 or p[0] > W or p[1] < 0 or p[1] > H
            r, d, f = table(p[9] != 0, p[10] != 0, out, p[7] >= MAX_STEPS, p[8] == 0, fix)
            rew[k, e], done[k, e], ev[k, e] = r, d, f
            cum[e] = 0.0 if (d and auto_reset) else cum[e] + r
    return rew, done, ev, cum


# ------------------------------------------------------------------------------------------------------------ the conditions
def check_conditions(count):
    """the issue's conditions on the (family, clear) counts of the target predicates of one run"""
    for f in BANDED:
        c, b = count[(f, True)], count[(f, False)]
        assert c >= 10 and b >= 10, (f, c, b)
        assert c >= b, (f, c, b)  # at least half of them clear
    for f in ("exact", "bounds", "limit"):
        assert count[(f, True)] > 0 and count[(f, False)] == 0, (f, count[(f, True)], count[(f, False)])


def count_targets(scenes, cls, ref):
    """(family, clear) -> target predicates of an oracle run and its classification: a scene at rest is judged once (the same pose at every step), a moving one per step"""
    count = collections.Counter()
    for k in range(len(cls)):
        for e, s in enumerate(scenes):
            if k and s.family != "approach":
                continue
            tp = target_pred(s, cls[k][e], ref["peek"][k][e, 7])
            if tp is not None:
                count[(s.family, tp[1])] += 1
    return count
