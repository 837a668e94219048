"""HparamSchedule — a hyper-parameter schedule: a piecewise-linear function of a timestep clock, the one definition every trainer reads.

Both reference trainers anneal hyper-parameters: train/stable_baselines/ppo.py:111-119,137 decays each of its three learning rates
linearly to 0 over the run (``make_lr_func(s, 0)``, PPO2's ``learning_rate(frac)``, evaluated once per update; PPO2 takes ``cliprange``
as a callable in the same way), and train/rllib/ppo.py:39 trains with ``lr_schedule: [[0, 1e-3], [5e6, 1e-4], [1e7, 1e-5]]`` (RLlib has
``entropy_coeff_schedule`` of the same form).  Both evaluate their schedules once per update, on the host, and so do the trainers here:
``NativePPO`` / ``DataParallelPPO`` / ``PopulationPPO`` take an ``HparamSchedule`` for ``lr``, ``clip`` and ``ent_coef`` where they take
a float, and ``set_timesteps(t)`` writes the values at ``t`` into the fields every update call already passes.  Nothing runs on the device.

NOT to be confused with the population's *update schedule* — the per-member epochs x minibatches plan of ``pack_schedule``,
``--mutate-schedule`` and ssg_pop_update_sched.  This module is about hyper-parameter schedules only, and says so in every name.

The value at an int ``t >= 0`` over the points ``(t_0 = 0, v_0), ..., (t_last, v_last)``:

    t >= t_last:            v_last                      (RLlib's outside_value; PPO2 holds the stop value the same way)
    t_i <= t < t_{i+1}:     v_i + ((t - t_i) / (t_{i+1} - t_i)) * (v_{i+1} - v_i)

in Python floats, the quotient the true division of the two ints.  The expression is fixed: tests and resumed runs depend on its bits.
RLlib's value before the first end point is a quirk of its own; requiring ``t_0 == 0`` leaves no "before".

Out of scope: schedules of ``vf_clip`` (it decides which entry point runs), ``lam``, ``gamma``, the KL terms (``kl_coef`` is adapted on
the device) and the Adam constants; a clock of wall time; interpolation that is not linear.
"""
import math
from bisect import bisect_right

SCHEDULABLE = ("lr", "clip", "ent_coef")  # the hyper-parameters a trainer takes a schedule for


def _is_int(x):
    return isinstance(x, int) and not isinstance(x, bool)


class HparamSchedule(object):
    """points: a list of (t_i, v_i) — ints t_i, strictly increasing from t_0 == 0, finite floats v_i, at least one.  Anything else is a
    ValueError naming the offending entry."""

    def __init__(self, points):
        if not isinstance(points, (list, tuple)) or len(points) < 1:
            raise ValueError("HparamSchedule: points must be a non-empty list of (t, v) pairs (got %r)" % (points,))
        pts = []
        for i, p in enumerate(points):
            if not isinstance(p, (list, tuple)) or len(p) != 2:
                raise ValueError("HparamSchedule: points[%d] = %r is not a (t, v) pair" % (i, p))
            t, v = p
            if not _is_int(t):
                raise ValueError("HparamSchedule: points[%d] = %r: t must be an int (got a %s)" % (i, p, type(t).__name__))
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError("HparamSchedule: points[%d] = %r: v must be a finite float" % (i, p))
            if i == 0 and t != 0:
                raise ValueError("HparamSchedule: points[0] = %r: the first point must be at t = 0" % (p,))
            if i > 0 and t <= pts[-1][0]:
                raise ValueError("HparamSchedule: points[%d] = %r: t must exceed the point before it (t = %d)" % (i, p, pts[-1][0]))
            pts.append((t, float(v)))
        self.points = tuple(pts)
        self._ts = [t for t, _ in pts]

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def constant(cls, v):
        """The schedule that is v at every t."""
        return cls([(0, v)])

    @classmethod
    def linear(cls, start, stop, total):
        """[(0, start), (total, stop)]: PPO2's linear decay over a run of `total` timesteps, held at `stop` afterwards."""
        return cls([(0, start), (total, stop)])

    @classmethod
    def parse(cls, spec, start, total):
        """A command line's spec: "linear:STOP" runs from `start` to STOP over `total` timesteps; "T0:V0,T1:V1,..." gives absolute
        points, as RLlib writes them.  Malformed text is a ValueError quoting the spec."""
        text = spec.strip() if isinstance(spec, str) else None
        if not text:
            raise ValueError("HparamSchedule.parse: %r is no spec (\"linear:STOP\" or \"T0:V0,T1:V1,...\")" % (spec,))
        try:
            if text.startswith("linear:"):
                return cls.linear(float(start), float(text[len("linear:"):]), total)
            points = []
            for part in text.split(","):
                t, sep, v = part.partition(":")
                if not sep:
                    raise ValueError("%r is not T:V" % part)
                points.append((int(t), float(v)))
            return cls(points)
        except ValueError as ex:
            raise ValueError("HparamSchedule.parse: the spec %r is malformed (\"linear:STOP\" or \"T0:V0,T1:V1,...\"): %s" % (spec, ex))

    # ------------------------------------------------------------------------------------------------
    def value(self, t):
        """The schedule's value at the int t >= 0 (the module's expression)."""
        if not _is_int(t) or t < 0:
            raise ValueError("HparamSchedule.value: t must be an int >= 0 (got %r)" % (t,))
        pts = self.points
        if t >= pts[-1][0]:
            return pts[-1][1]
        i = bisect_right(self._ts, t) - 1
        (t0, v0), (t1, v1) = pts[i], pts[i + 1]
        return v0 + ((t - t0) / (t1 - t0)) * (v1 - v0)

    def values(self):
        """The points' values: a piecewise-linear function stays between them."""
        return [v for _, v in self.points]

    def state(self):
        """Plain data, as a checkpoint holds it: a list of [t, v] lists."""
        return [[t, v] for t, v in self.points]

    @classmethod
    def from_state(cls, state):
        """state() undone."""
        if not isinstance(state, (list, tuple)):
            raise ValueError("HparamSchedule.from_state: a list of [t, v] lists (got %r)" % (state,))
        return cls([tuple(p) if isinstance(p, list) else p for p in state])

    def __eq__(self, other):
        return isinstance(other, HparamSchedule) and self.points == other.points

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.points)

    def __repr__(self):
        return "HparamSchedule(%r)" % (self.state(),)


# ------------------------------------------------------------------------------------------------------------------------------------
# what the trainer classes share
# ------------------------------------------------------------------------------------------------------------------------------------
def check_schedulable(who, name, sched):
    """The refusals of a trainer's constructor and load_state_dict: a clip schedule must be > 0 at every point (the library refuses
    clip <= 0, and a piecewise-linear function over positive points stays positive); lr and ent_coef need only be finite, which every
    schedule is."""
    if name == "clip":
        for i, (t, v) in enumerate(sched.points):
            if not v > 0.0:
                raise ValueError("%s: the clip schedule's points[%d] = (%d, %r) is not > 0" % (who, i, t, v))
    return sched


def split(who, name, given):
    """(the float a trainer starts with, its schedule or None) of one member's argument: a float, or an HparamSchedule (its value at 0)."""
    if isinstance(given, HparamSchedule):
        return check_schedulable(who, name, given).value(0), given
    return float(given), None


def entry_state(sched):
    """One schedule as a state dict holds it: its points, or an empty list for "constant"."""
    return [] if sched is None else sched.state()


def entry_from_state(who, name, entry):
    """entry_state undone and checked: ValueError naming the field for anything malformed."""
    if isinstance(entry, list) and not entry:
        return None
    try:
        return check_schedulable(who, name, HparamSchedule.from_state(entry))
    except ValueError as ex:
        raise ValueError("%s: schedules[%r] is malformed: %s" % (who, name, ex))


def check_clock(who, t):
    if not _is_int(t) or t < 0:
        raise ValueError("%s: timesteps must be an int >= 0 (got %r)" % (who, t))
    return t
