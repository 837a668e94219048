"""What the body-chain suites share (tests/test_sincos_gpu.py, tests/test_body_integrator_gpu.py): one open river, handles whose
ssg_config fields a test overrides, and the numpy restatement of the body role's per-step arithmetic.

The river is event_scenes' "rect" record alone: banks x <= 64 and x >= 536, goals nobody comes near.  A ship whose body sits at
CLEAR = (300, 300) stays 190 clear of both banks, of the bounds and of config 4's parked traffic at every rotation (the hull
reaches 46.1 from the body's origin), so no event of the step kernel interferes with the columns read back.

restate_step() is handle_discrete_action (game.py:140-153, models.py:129-146), cpBodyUpdatePosition and cpBodyUpdateVelocity as
oracle/ssg_oracle.c states them (apply_action, ora_body_apply_force_at_local_point, ora_body_update_position / _velocity), one IEEE
operation per line on numpy f64 arrays — numpy never contracts a product into a sum — with Chipmunk's additions of zero (v_bias,
gravity, the force accumulator) kept, so that the kernel's leaving them out is itself under test.
"""
import numpy as np

import event_scenes as ES
import sincos_args as A
from lidar_scenes import pad12

CLEAR = (300.0, 300.0)
LAYOUTS = (("64", False), ("128", False), ("256", False), ("64", True), ("128", True), ("256", True))
BEAMS = (1, 8, 10, 16)  # one beam count from each compiled beam group (1-4, 5-8, 9-12, 13-16)
NG = 5
SPEEDS = (1, 10, 30, 40)
K = 40
VALUES = (1e-300, 1e-150, 3.3e-30, 1.7e-8, 0.1, 0.7853981633974483, 1.0, 7.3, 123.456, 1e3, 0.0, 5e-324, 2.3e-310)
N_COAST = 64 * 5 + 44   # two 256-env workgroups, six waves, the last one 44 lanes
N_STEP = 64 * 9 + 44
PRELUDE = ((1, 1, 1, 1), (1, 1, 1, 2), (1, 2, 1, 2), (2, 2, 2, 1), (2, 2, 2, 2), (0, 0, 0, 0))
PRELUDE_RUDDER = (-10, -5, 0, 5, 10, 0)
STEP_ACTIONS = (0, 0, 0, 1, 2)


def river():
    """(polys [1, 2, 12, 2], goals [1, NG, 2]) of the one record"""
    left, right = pad12(ES._rect(0, 0, 64, 512)), pad12(ES._rect(536, 0, 600, 512))
    return np.stack([np.stack([left, right])]), np.array([ES.FAR_GOALS[:NG]], dtype=np.float64)


def make_vec(monkeypatch, n, n_beams=10, blk=None, in_global=False, n_ships=1, speed=10, **fields):
    """A ShipVecEnv of n envs on the river, auto_reset off, whose ssg_config carries `fields` (force_y, ship_m_inv, thrust_px0, ...):
    the production constructor, handed another default record — no production code knows about the test."""
    from ship_sim_gym_amd import _native as N, config as cfgmod, worldgen
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    stock = N.default_config

    def patched():
        c = stock()
        for name, value in fields.items():
            assert hasattr(c, name), name
            setattr(c, name, value)
        return c

    class GC(cfgmod.GameConfig):
        SPEED = speed

    polys, goals = river()
    assert cfgmod.N_GOALS == NG
    bank = np.stack([worldgen.build_record(p[0], p[1], g, (ES.W / 2, 25.0)) for p, g in zip(polys, goals)])
    with monkeypatch.context() as m:
        m.setattr(N, "default_config", patched)
        if blk is not None:
            m.setenv("SSG_BLOCK", blk)
        vec = ShipVecEnv(n, game_config=GC, n_beams=n_beams, bank=bank, bank_in_global=in_global, auto_reset=False, n_ships=n_ships)
    for name, value in fields.items():
        assert getattr(vec.cfg, name) == value
    assert vec.cfg.dt == speed * cfgmod.BASE_DT
    vec.bank_polys, vec.bank_goals = polys, goals  # (what helpers.run_pair / an oracle Batch are given)
    return vec


POSE_FIELDS = ("F_X", "F_Y", "F_ANGLE", "F_VX", "F_VY", "F_W")


def write_pose(torch, N, vec, cols):
    """cols: f64 [6, n] (x, y, angle, vx, vy, w) into the state columns; config 4: the traffic parked, then wake_dynamics()"""
    t = torch.from_numpy(np.ascontiguousarray(cols, dtype=np.float64)).to(vec.device)
    for i, name in enumerate(POSE_FIELDS):
        vec.field(getattr(N, name))[:] = t[i]
    if vec.n_ships > 1:
        T = vec.field(N.F_TRAFFIC)
        for k in range(3):
            T[9 * k: 9 * k + 9] = 0.0
            T[9 * k + 0] = ES.PARK_SHIPS[k][0]
            T[9 * k + 1] = ES.PARK_SHIPS[k][1]
        vec.wake_dynamics()


def read_state(N, vec):
    """{x, y, a, vx, vy, w f64 [n]; rudder int32 [n]; bit7 bool [n]} of the state columns"""
    out = {k: vec.field(getattr(N, f)).cpu().numpy().copy() for k, f in zip(("x", "y", "a", "vx", "vy", "w"), POSE_FIELDS)}
    out["rudder"] = vec.field(N.F_RUDDER).cpu().numpy().copy()
    out["bit7"] = (vec.field(N.F_GOAL_MASK).cpu().numpy() & 0x80) != 0
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return bits(a) == bits(b)


def constants(vec):
    c = vec.cfg
    return {"dt": c.dt, "damp": c.damping_pow_dt, "m_inv": c.ship_m_inv, "i_inv": c.ship_i_inv, "force_y": c.force_y,
            "px0": c.thrust_px0, "py0": c.thrust_py0, "rudder_step": int(c.rudder_step), "rudder_max": int(c.rudder_max)}


def restate_step(st, act, k, s, c):
    """One step of the body's chain.  st: read_state()'s dict (not modified); act int [n]; k: constants(); (s, c): the rotation of
    the PRE-step angle, (sin, cos) f64 [n] — read only by the lanes that thrust.  Returns the post-step dict."""
    x, y, a, vx, vy, w = (st[n] for n in ("x", "y", "a", "vx", "vy", "w"))
    rudder, bit7 = st["rudder"].copy(), st["bit7"].copy()
    dt, damp, zero = k["dt"], k["damp"], np.zeros_like(x)
    thrust = act == 0
    # Ship.move_forward: cpBodyApplyForceAtLocalPoint((0, F) * 1, point_of_thrust); the point is (px0, py0) until the first
    # rotate(), then (0 - rudder, py0) (models.py:109,146)
    px = np.where(bit7, 0.0 - rudder.astype(np.float64), k["px0"])
    py = np.full_like(x, k["py0"])
    ms = -s
    f_x, f_y = 0.0 * 1, k["force_y"] * 1
    t1 = c * f_x
    t2 = ms * f_y
    fwx = t1 + t2          # cpTransformVect(transform, force)
    t3 = s * f_x
    t4 = c * f_y
    fwy = t3 + t4
    u1 = c * px
    u2 = ms * py
    u3 = u1 + u2
    pwx = u3 + x           # cpTransformPoint(transform, point)
    u4 = s * px
    u5 = c * py
    u6 = u4 + u5
    pwy = u6 + y
    o1 = c * 0.0
    o2 = ms * 0.0
    o3 = o1 + o2
    ox = o3 + x            # cpTransformPoint(transform, cog), cog = (0, 0)
    o4 = s * 0.0
    o5 = c * 0.0
    o6 = o4 + o5
    oy = o6 + y
    rx = pwx - ox
    ry = pwy - oy
    m1 = rx * fwy
    m2 = ry * fwx
    cross = m1 - m2
    fx = np.where(thrust, zero + fwx, zero)    # body->f = cpvadd(body->f, force)
    fy = np.where(thrust, zero + fwy, zero)
    tq = np.where(thrust, zero + cross, zero)  # body->t += cpvcross(r, force)
    # Ship.rotate(-5 / +5) + clamp_rudder
    turn = (act == 1) | (act == 2)
    moved = rudder + np.where(act == 1, -k["rudder_step"], k["rudder_step"])
    moved = np.maximum(-k["rudder_max"], np.minimum(k["rudder_max"], moved))
    rudder = np.where(turn, moved, rudder).astype(np.int32)
    bit7 = bit7 | turn
    # cpBodyUpdatePosition
    vbx = vx + 0.0
    dx = vbx * dt
    nx = x + dx
    vby = vy + 0.0
    dy = vby * dt
    ny = y + dy
    wb = w + 0.0
    da = wb * dt
    na = a + da
    # cpBodyUpdateVelocity, gravity 0
    ax = fx * k["m_inv"]
    gx = 0.0 + ax
    ix = gx * dt
    kx = vx * damp
    nvx = kx + ix
    ay = fy * k["m_inv"]
    gy = 0.0 + ay
    iy = gy * dt
    ky = vy * damp
    nvy = ky + iy
    kw = w * damp
    aw = tq * k["i_inv"]
    iw = aw * dt
    nw = kw + iw
    return {"x": nx, "y": ny, "a": na, "vx": nvx, "vy": nvy, "w": nw, "rudder": rudder, "bit7": bit7}


# ------------------------------------------------------------------------------------------------------ the integrator suites' lanes
def coast_lanes():
    """(cols f64 [6, n], act int32 [K, n], untouched bool [n])"""
    n = N_COAST
    rng = np.random.RandomState(20261021)
    v = np.array([s * x for x in VALUES for s in (1.0, -1.0)])
    i = np.arange(n)
    cols = np.stack([CLEAR[0] + rng.uniform(-50, 50, n), CLEAR[1] + rng.uniform(-50, 50, n), rng.uniform(-3, 3, n),
                     v[i % len(v)], v[(7 * i + 3) % len(v)], v[(11 * i + 5) % len(v)]])
    pat = i % 8
    act = np.empty((K, n), dtype=np.int32)
    act[:, pat == 0] = 1
    act[:, pat == 1] = 2
    act[:, pat == 2] = np.array([1] * 4 + [2] * 8 + [1] * 8 + [2] * 20)[:, None]
    act[:, pat == 3] = np.array([1, 2] * 20)[:, None]
    act[:, pat == 4] = np.array([2, 2, 1, 1, 1, 1, 2, 2] * 5)[:, None]
    act[:, pat >= 5] = rng.randint(1, 3, size=(K, int((pat >= 5).sum())))
    untouched = pat == 7
    act[:, untouched] = 0
    cols[2:, untouched] = 0.0  # angle 0, at rest: the rotation is (0, 1) exactly and stays so
    return cols, act, untouched


def step_lanes(fix):
    """(cols [6, n], prelude int32 [4, n], act int32 [n], combo [n], fixture index of the lane's angle [n])"""
    n = N_STEP
    a, fam = fix["a"], fix["family"]
    ok = (np.abs(a) <= A.LIMIT) & (np.abs(fix["sin_hi"]) > 2.0 ** -30) & (np.abs(fix["cos_hi"]) > 2.0 ** -30) & (a > 0)
    pick = np.concatenate([np.nonzero(ok & (fam == f))[0][:m] for f, m in ((4, 8), (3, 4), (2, 4))])
    pick = np.concatenate([pick, A.mirror_index(a)[pick]])  # both signs: 32 angles
    assert len(pick) == 32 and np.all(np.abs(fix["sin_hi"][pick]) > 2.0 ** -30) and np.all(np.abs(fix["cos_hi"][pick]) > 2.0 ** -30)
    rng = np.random.RandomState(20261022)
    i = np.arange(n)
    combo, j = i % 6, (i // 6) % 5
    which = pick[(5 * i + i // 30) % len(pick)]
    mag = lambda lo, hi: rng.uniform(lo, hi, n) * rng.choice([-1.0, 1.0], n)
    cols = np.stack([CLEAR[0] + rng.uniform(-5, 5, n), CLEAR[1] + rng.uniform(-5, 5, n), a[which], mag(0.01, 3.0), mag(0.01, 3.0), mag(0.001, 0.5)])
    prelude = np.array(PRELUDE, dtype=np.int32)[combo].T.copy()
    act = np.array(STEP_ACTIONS, dtype=np.int32)[j]
    return cols, prelude, act, combo, which
