"""body_scenes.restate_step against the oracle, bit for bit, on the lanes tests/test_body_integrator_gpu.py runs.

The GPU suite compares the kernel's columns with a numpy restatement; this ties the restatement to oracle/ssg_oracle.c (the C
statement of the reference's handle_discrete_action and Chipmunk's integrator), without a GPU.  The oracle rotates with libm's
sin / cos, so the restatement is given numpy's (the same libm) here; the arithmetic around the rotation is what is compared, and
it agrees in every bit at every dt and thrust point.
"""
import math

import numpy as np
import pytest

import body_scenes as BS
import sincos_args as A

COLS = ("x", "y", "vx", "vy", "a", "w")  # Batch.peek_all()'s first columns; rudder is column 6


def _constants(native, dt, point):
    c = native.default_config()
    return {"dt": dt, "damp": math.pow(0.4, dt), "m_inv": c.ship_m_inv, "i_inv": c.ship_i_inv, "force_y": c.force_y,
            "px0": point[0], "py0": point[1], "rudder_step": int(c.rudder_step), "rudder_max": int(c.rudder_max)}


def _batch(O, n, dt, point):
    polys, goals = BS.river()
    ob = O.Batch(n, O.default_config(dt=dt, n_beams=10, history=2, n_goals=BS.NG, thrust_px0=point[0], thrust_py0=point[1]), polys, goals,
                 map_ids=np.zeros(n, dtype=np.int32))
    ob.reset()
    return ob


def _state(cols, rudder, bit7):
    return {"x": cols[0], "y": cols[1], "a": cols[2], "vx": cols[3], "vy": cols[4], "w": cols[5], "rudder": rudder.astype(np.int32), "bit7": bit7}


def _same(want, pk, where):
    for c, name in enumerate(COLS):
        bad = ~BS.same_bits(want[name], pk[:, c])
        assert not bad.any(), (where, name, int(bad.sum()), [(int(e), float(want[name][e]).hex(), float(pk[e, c]).hex()) for e in np.nonzero(bad)[0][:6]])
    assert np.array_equal(want["rudder"], pk[:, 6].astype(np.int32)), where


@pytest.mark.parametrize("point", ((0.0, 0.0), (10.0, 22.5)), ids=("px0_0", "px0_bb_centre"))
@pytest.mark.parametrize("speed", BS.SPEEDS)
def test_one_step_is_the_oracles(oracle, native, speed, point):
    cols, prelude, act, combo, _ = BS.step_lanes(A.load())
    n, dt = cols.shape[1], speed * 0.1
    ob = _batch(oracle, n, dt, point)
    for k in range(len(prelude)):
        ob.step(prelude[k], auto_reset=False)
    pk = ob.peek_all()
    assert np.array_equal(pk[:, 6], np.array(BS.PRELUDE_RUDDER)[combo])
    for e in range(n):
        ob.poke_state(e, *cols[:, e])
    ob.step(act, auto_reset=False)
    st = _state(cols, np.array(BS.PRELUDE_RUDDER)[combo], combo != 5)
    want = BS.restate_step(st, act, _constants(native, dt, point), np.sin(cols[2]), np.cos(cols[2]))
    _same(want, ob.peek_all(), "SPEED %d point %r" % (speed, point))


@pytest.mark.parametrize("speed", BS.SPEEDS)
def test_coast_is_the_oracles(oracle, native, speed):
    cols, act, untouched = BS.coast_lanes()
    n, dt = cols.shape[1], speed * 0.1
    ob = _batch(oracle, n, dt, (0.0, 0.0))
    for e in range(n):
        ob.poke_state(e, *cols[:, e])
    kk = _constants(native, dt, (0.0, 0.0))
    st = _state(cols, np.zeros(n), np.zeros(n, dtype=bool))
    for k in range(BS.K):
        ob.step(act[k], auto_reset=False)
        st = BS.restate_step(st, act[k], kk, np.zeros(n), np.ones(n))  # (only the untouched lanes thrust: angle 0 throughout)
        assert np.all(st["a"][untouched] == 0.0) and not st["bit7"][untouched].any() and st["bit7"][~untouched].all()
        _same(st, ob.peek_all(), "SPEED %d step %d" % (speed, k))
