"""The action sampler at its decision boundaries (step 4 of policy_act_body in csrc/shipsim_policy.hip): the case table, the f64 reference,
a numpy float32 restatement of the kernel's formula order with named defects, the scan of u, the bound and the assertions.  No device, no
pytest: tests/test_sampler_edges.py runs the table against the restatement (with the defects switched on) on the host,
tests/test_sampler_edges_gpu.py against every kernel that carries the step.

How a decision becomes observable.  A policy whose Wpi is zero has logits == bpi bit for bit in every env, and u comes from the caller
(policy_act(..., uniforms=u)), so ONE launch over n envs scans n values of u against one fixed logits row: `scan` lays out, per threshold
j < A - 1, the 4097 points k * 2^-24 of Philox's grid around cdf64_j (clipped to [0, 2^24 - 1]), then the ends 0, 2^-24, 1 - 2^-24, then
the values only a caller can pass (1.0, 1.5, -0.0, -1.0, NaN), then 0.5 up to a fixed length.

What is asserted of a scan (`judge_case`; `check_case` raises on the first failures):
  (a) 0 <= act < A on every row.
  (b) act is non-decreasing in u within each window, so threshold j has at most one flip index k_j (the first k with act > j).
  (c) |k_j * 2^-24 - cdf64_j| <= B + 2^-24, B = 4 ulp32(M) + 16 * 2^-24, M = max(max|lg|, |lse|): the roundings of lse and of lg - lse
      scale with M, expf and logf are 1 ulp each of a number <= 1, three f32 additions; the kernel's rule u > cdf puts the flip up to one
      grid step above its own threshold.  A window without a flip needs cdf64_j <= B or cdf64_j >= 1 - 2^-24 - B.
  (d) logp has the same bits on all rows with the same act (so it flips on exactly the row where act flips), at most A values in all,
      each within B of the f64 log-probability of that action (-inf where that is -inf, NaN where the logits hold a NaN or +inf); with
      logp_all (the trainer's dist on the stored x) logp[row] == logp_all[row, act[row]] bitwise (two NaNs count as equal).
  (e) pinned rows, as gpu_support.torch_sample decides them: u = 0, -0.0, -1.0 and NaN give action 0 (u = 0 even where p_0 == 0: what
      tells `>` from `>=`); u = 1.0 gives action 0 where cdf_0 == 1.0f; a NaN or +inf logit gives action 0 on every row; a -inf logit in
      position j > 0 is never chosen on the grid.  The last is where the kernel LEAVES torch_sample's rule: the f32 sum of the other
      probabilities can stop short of 1 - 2^-24, the plain count then draws a masked last action at the top of the grid, and the kernel
      steps back from it (the defect "masked_drawn" is the plain count).

The table's probabilities are at least 1e-3 except where a case is there FOR a tiny or zero one (dominant, saturated, -inf) and in the
spread-8 rows (a spread of 8 is a ratio of exp(-8) = 3.4e-4; the smallest probability there is 3.1e-4): a threshold built from a wrong
partial sum misses by that much or more, while B is 1.7e-5 or less everywhere but where M = 200 (6.2e-5: the offsets of +-200, whose
probabilities are >= 0.06, and the saturated rows, which have one threshold value)."""
from collections import namedtuple

import numpy as np

f32 = np.float32
GRID = 2.0 ** -24
TOP = 2 ** 24 - 1                 # the largest Philox value is TOP * 2^-24
HALF = 2048                       # a window is 2 * HALF + 1 grid points
ENDS = (0.0, GRID, 1.0 - GRID)
CALLER = (1.0, 1.5, -0.0, -1.0, float("nan"))
N_ENVS = 12304                    # 3 windows + ends + caller values = 12 299, padded: 2 x 6152 (a member slice with a tail workgroup)
ACTIONS = (2, 3, 4)
NINF, PINF, NAN = float("-inf"), float("inf"), float("nan")

Case = namedtuple("Case", "name A lg")            # lg: the f32 logits row as python floats
Scan = namedtuple("Scan", "u windows ends caller pad")   # windows: [(j, slice, k int64 [4097])]; the rest: slices of u


# ------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------------------------------------------
_SPREAD2 = {2: (0.0, -2.0), 3: (-2.0, 0.0, -1.0), 4: (-1.0, 0.0, -2.0, -0.5)}
_ROWS = {
    "equal": {2: (0.0, 0.0), 3: (0.0, 0.0, 0.0), 4: (0.0, 0.0, 0.0, 0.0)},
    "spread0.5": {2: (0.0, -0.5), 3: (-0.5, 0.0, -0.25), 4: (-0.25, -0.5, 0.0, -0.125)},
    "spread2": _SPREAD2,
    "spread2/repeated": {2: (0.75, 0.75), 3: (0.0, -2.0, 0.0), 4: (0.0, -2.0, -2.0, -1.0)},
    "spread8": {2: (0.0, -8.0), 3: (-4.0, -8.0, 0.0), 4: (-8.0, -3.0, 0.0, -5.5)},
}
# rows in front of a masked last action whose f32 probabilities add up to 1 - 2^-22 or less: before the kernel stepped back from a
# masked action, an MI355X drew it there for the three largest u of the grid (with two actions the sum is exp(0) = 1)
_SHORT = {3: (0.6302164793014526, 4.13877010345459), 4: (1.1687442064285278, -2.2996838092803955, 1.5198832750320435)}


def cases(A):
    """The table of one action count, in a fixed order."""
    out = [Case("%s/A=%d" % (k, A), A, v[A]) for k, v in _ROWS.items()]
    for off in (50.0, -50.0, 200.0, -200.0):
        out.append(Case("offset%+g/A=%d" % (off, A), A, tuple(x + off for x in _SPREAD2[A])))
    for d in (10.0, 16.0, 17.0, 30.0):                                          # 1 + expf(-d) rounds to 1 from d = 17 on
        out.append(Case("dominant-%g/first/A=%d" % (d, A), A, (0.0,) + (-d,) * (A - 1)))
    for d in (16.0, 17.0):
        out.append(Case("dominant-%g/last/A=%d" % (d, A), A, (-d,) * (A - 1) + (0.0,)))
    out.append(Case("saturated/A=%d" % A, A, (0.0,) + (-200.0,) * (A - 1)))
    out.append(Case("saturated/mirror/A=%d" % A, A, (-200.0,) * (A - 1) + (0.0,)))
    base = _SPREAD2[A]
    for where, j in (("first", 0), ("middle", 1), ("last", A - 1)):
        if where == "middle" and A == 2:
            continue
        out.append(Case("-inf/%s/A=%d" % (where, A), A, base[:j] + (NINF,) + base[j + 1:]))
    if A in _SHORT:
        out.append(Case("-inf/last/short/A=%d" % A, A, _SHORT[A] + (NINF,)))
    out.append(Case("nan/first/A=%d" % A, A, (NAN,) + base[1:]))
    out.append(Case("nan/last/A=%d" % A, A, base[:-1] + (NAN,)))
    out.append(Case("+inf/A=%d" % A, A, base[:1] + (PINF,) + base[2:]))
    for c in out:
        assert len(c.lg) == A and all(x != x or float(f32(x)) == x for x in c.lg), c.name    # every logit IS an f32
    return out


def all_cases():
    return [c for A in ACTIONS for c in cases(A)]


def finite(case):
    """Whether the case has a distribution: no NaN and no +inf logit (-inf is a probability of zero)."""
    return all(x == x and x != PINF for x in case.lg)


# ------------------------------------------------------------------------------------------------------------------------------------
# the f64 reference and the bound
# ------------------------------------------------------------------------------------------------------------------------------------
def reference64(case):
    """(lp64 [A], cdf64 [A - 1], lse64) of a finite case: log_softmax and cumsum(softmax)[:-1] in f64."""
    z = np.asarray(case.lg, dtype=np.float64)
    m = z.max()
    with np.errstate(divide="ignore"):
        e = np.exp(z - m)
        lse = m + np.log(e.sum())
        lp = z - lse
    return lp, np.cumsum(e / e.sum())[:-1], lse


def bound(case):
    """B = 4 ulp32(M) + 16 * 2^-24, M = max(max|lg| over the finite logits, |lse|)."""
    lse = reference64(case)[2]
    M = max(max(abs(x) for x in case.lg if x != NINF), abs(lse))
    return 4.0 * float(np.spacing(f32(M))) + 16.0 * GRID


def min_probability(case):
    return float(np.exp(reference64(case)[0]).min())


# ------------------------------------------------------------------------------------------------------------------------------------
# the scan of u
# ------------------------------------------------------------------------------------------------------------------------------------
def scan(case, n=N_ENVS):
    """The u values of one launch (f32 [n]) and where each group sits.  A case without a distribution gets its windows at (j + 1) / A."""
    A = case.A
    centres = reference64(case)[1] if finite(case) else np.arange(1, A) / A
    parts, windows, at = [], [], 0
    for j in range(A - 1):
        c = int(np.rint(centres[j] * 2.0 ** 24))
        k = np.clip(np.arange(c - HALF, c + HALF + 1, dtype=np.int64), 0, TOP)
        parts.append(k.astype(np.float64) * GRID)
        windows.append((j, slice(at, at + k.size), k))
        at += k.size
    groups = []
    for vals in (ENDS, CALLER):
        parts.append(np.asarray(vals, dtype=np.float64))
        groups.append(slice(at, at + len(vals)))
        at += len(vals)
    assert at <= n
    parts.append(np.full(n - at, 0.5))
    u = np.concatenate(parts).astype(f32)
    assert u.size == n and np.array_equal(u[: groups[0].stop].astype(np.float64), np.concatenate(parts[:-2]))    # every grid point IS an f32
    return Scan(u, windows, groups[0], groups[1], slice(at, n))


# ------------------------------------------------------------------------------------------------------------------------------------
# the float32 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("ge", "m_for_lse", "one_term_short", "one_term_long", "logp_early", "logp_late", "loop_bound_A", "masked_drawn")


def _terms32(lg, A):
    """log_sum_exp's m and lse and the A log-probabilities, the kernel's order in numpy float32 (fmaxf drops a NaN operand)."""
    with np.errstate(all="ignore"):
        m = lg[0]
        for j in range(1, A):
            m = np.fmax(m, lg[j])
        s = f32(0.0)
        for j in range(A):
            s = f32(s + np.exp(f32(lg[j] - m)))
        lse = f32(m + np.log(s))
        return m, lse, np.array([f32(lg[j] - lse) for j in range(A)], dtype=f32)


def _act32(lg, A, u, m, lse, defect):
    sub = m if defect == "m_for_lse" else lse
    with np.errstate(all="ignore"):
        cum, cdf = [f32(0.0)], f32(0.0)                                         # cum[i + 1] = p_0 + ... + p_i, summed as the kernel does
        for j in range(A):
            cdf = f32(cdf + np.exp(f32(lg[j] - sub)))
            cum.append(cdf)
        first = {"one_term_short": 0, "one_term_long": 2}.get(defect, 1)        # threshold j is cum[j + first]
        a = np.zeros(u.shape, dtype=np.int32)
        for j in range(A if defect == "loop_bound_A" else A - 1):
            t = cum[min(j + first, A)]
            a += (u >= t) if defect == "ge" else (u > t)
        if defect != "masked_drawn":                                            # step back from a masked action to the one in front
            for j in range(A - 1, 0, -1):
                if lg[j] == NINF:
                    a[a == j] = j - 1
    return a


def restatement(case, u, defect=None):
    """(act int32 [n], logp f32 [n], logp_all f32 [n, 4]) of step 4 in numpy float32 on the f32 array u.  defect: one of DEFECTS, the rule
    a subtly wrong kernel would follow."""
    A = case.A
    lg = np.asarray(case.lg, dtype=f32)
    u = np.asarray(u, dtype=f32)
    m, lse, lp = _terms32(lg, A)
    a = _act32(lg, A, u, m, lse, defect)
    src = a
    if defect in ("logp_early", "logp_late"):                                   # logp follows the action of the NEXT / the previous grid point
        with np.errstate(invalid="ignore"):
            shifted = (u.astype(np.float64) + (GRID if defect == "logp_early" else -GRID)).astype(f32)
        src = _act32(lg, A, shifted, m, lse, None)
    logp = np.where(src < A, lp[np.minimum(src, A - 1)], lp[0]).astype(f32)     # (a == A: the kernel's select chain keeps lp of action 0)
    la = np.zeros((u.size, 4), dtype=f32)
    la[:, :A] = lp
    return a, logp, la


# ------------------------------------------------------------------------------------------------------------------------------------
# the assertions
# ------------------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def same_float(a, b):
    """Bitwise equality, two NaNs counting as equal (a NaN's payload is not part of any contract)."""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def judge_case(case, sc, act, logp, logp_all=None):
    """What a kernel's results on scan `sc` of `case` must satisfy, (a) to (e) of the module docstring.  Returns (the failures as
    (case, assertion, detail), a record: `ratio` = the largest |k_j * 2^-24 - cdf64_j| / B, `flips` = {j: k_j}, `flipless` = the
    thresholds (c) does not apply to because they lie within B of an end)."""
    A, u = case.A, sc.u
    act = np.asarray(act).astype(np.int64)
    logp = np.asarray(logp, dtype=f32)
    fails, rec = [], dict(ratio=0.0, flips={}, flipless=[], thresholds=0)
    assert act.shape == u.shape == logp.shape, (case.name, act.shape, u.shape, logp.shape)

    def fail(which, detail):
        fails.append((case.name, which, detail))

    # (a)
    bad = np.flatnonzero((act < 0) | (act >= A))
    if bad.size:
        fail("a", "act %s at u %r" % (act[bad[:4]].tolist(), u[bad[:4]].tolist()))
    fin = finite(case)
    grid = np.r_[0: sc.ends.stop, sc.pad]
    # (b), (c)
    if fin:
        lp64, cdf64, _ = reference64(case)
        B = bound(case)
        for j, sl, k in sc.windows:
            rec["thresholds"] += 1
            w = act[sl]
            if (np.diff(w) < 0).any():
                i = int(np.flatnonzero(np.diff(w) < 0)[0])
                fail("b", "threshold %d: act %d at k %d, then %d at k %d" % (j, w[i], k[i], w[i + 1], k[i + 1]))
                continue
            past = w > j
            if past.any() and not past.all():
                kj = int(k[int(np.argmax(past))])
                rec["flips"][j] = kj
                err = abs(kj * GRID - cdf64[j])
                rec["ratio"] = max(rec["ratio"], err / B)
                if not err <= B + GRID:
                    fail("c", "threshold %d flips at k %d = %.9g, cdf64 %.9g: off by %.3e > B + 2^-24 = %.3e" % (j, kj, kj * GRID, cdf64[j], err, B + GRID))
            elif cdf64[j] <= B or cdf64[j] >= 1.0 - GRID - B:
                rec["flipless"].append(j)
            else:
                fail("c", "threshold %d: no flip within %d grid points of cdf64 %.9g (act %d throughout)" % (j, HALF, cdf64[j], w[0]))
    # (d)
    values = {}
    for a in np.unique(act):
        rows = act == a
        b = _bits(logp[rows])
        if not (same_float(logp[rows], logp[rows][:1])).all():
            i = int(np.flatnonzero(b != b[0])[0])
            fail("d", "act %d: logp %r at u %r but %r at u %r" % (a, float(logp[rows][0]), float(u[rows][0]), float(logp[rows][i]), float(u[rows][i])))
        values[int(a)] = logp[rows][0]
    if len(values) > A:
        fail("d", "%d different actions" % len(values))
    for a, v in values.items():
        if not 0 <= a < A:
            continue
        if not fin:
            if not np.isnan(v):
                fail("d", "act %d: logp %r where the logits have no distribution" % (a, float(v)))
        elif lp64[a] == NINF:
            if v != NINF:
                fail("d", "act %d: logp %r, the f64 value is -inf" % (a, float(v)))
        elif not abs(float(v) - lp64[a]) <= B:
            fail("d", "act %d: logp %r, f64 %.9g: off by %.3e > B = %.3e" % (a, float(v), lp64[a], abs(float(v) - lp64[a]), B))
    if logp_all is not None:
        la = np.asarray(logp_all, dtype=f32).reshape(u.size, 4)
        ok = (act >= 0) & (act < A)
        got = la[np.arange(u.size), np.clip(act, 0, 3)]
        bad = np.flatnonzero(ok & ~same_float(logp, got))
        if bad.size:
            fail("d", "logp %r != logp_all[act] %r at u %r" % (float(logp[bad[0]]), float(got[bad[0]]), float(u[bad[0]])))
    # (e)
    un = u.astype(np.float64)
    with np.errstate(invalid="ignore"):
        zero = np.isnan(un) | (un <= 0.0)
    if (act[zero] != 0).any():
        i = int(np.flatnonzero(zero & (act != 0))[0])
        fail("e", "u = %r gives action %d" % (float(u[i]), act[i]))
    if not fin and act.any():
        i = int(np.flatnonzero(act)[0])
        fail("e", "action %d at u %r although the logits hold a NaN or +inf" % (act[i], float(u[i])))
    if fin and cdf64[0] == 1.0 and (act[un == 1.0] != 0).any():
        fail("e", "u = 1.0 against cdf_0 == 1.0f gives action %d" % act[un == 1.0].max())
    for j in range(1, A):
        if case.lg[j] == NINF and (act[grid] == j).any():
            i = int(grid[np.flatnonzero(act[grid] == j)[0]])
            fail("e", "the -inf logit %d is chosen at u = %r = %d * 2^-24" % (j, float(u[i]), int(round(float(u[i]) / GRID))))
    return fails, rec


def check_case(case, u, act, logp, logp_all=None):
    """judge_case on the case's own scan, asserted (u must BE that scan, bit for bit): returns its record."""
    u = np.asarray(u, dtype=f32)
    sc = scan(case, u.size)
    assert np.array_equal(_bits(u), _bits(sc.u)), case.name
    fails, rec = judge_case(case, sc, act, logp, logp_all)
    assert not fails, fails[:6]
    return rec
