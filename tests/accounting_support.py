"""What the accounting domain tests share (tests/test_eval_account_domain_gpu.py, tests/test_episode_stats_domain_gpu.py, tests/
test_exploit_domain_gpu.py and the CPU checks of tests/test_accounting_support.py): the synthetic [T, N] inputs, the exploit copy's
source vectors, the references, and the same references with ONE defect
injected, which the CPU checks run to show that a case's inputs tell the defect from the honest walk.  Nothing here needs a device.

References: the evaluation's is ``ship_sim_gym_amd.evaluate.eval_walk`` as it stands; ``episode_stats_walk`` is the one of
ssg_pop_episode_stats.  ``eval_walk_with`` restates eval_walk in Python integers so that a defect can be switched on; with defect=None
it must give eval_walk's results (tests/test_accounting_support.py asserts it), and no GPU comparison uses it.

Inputs.  Every reward family keeps the f64 walk exact, so the references do not depend on an order of additions that the device could
legitimately choose otherwise (it cannot: one lane walks one env in step order — but the integers would not show it if it did not):
  tie   multiples of 1/8 in [-3/8, 3/8]: every partial sum and its product with 100 is exact, and odd multiples land on x.5
  big   +-2^25 per step: 100 * return exceeds 2^31 after one step, a member's total exceeds 2^32 and stays far below 2^53
  sim   the simulator's {1, -1, -0.01}
Flags are all 256 byte values, on done steps and on the others; done bytes are drawn from {1, 2, 0x80, 0xFF}."""
import math

import numpy as np

TILE = 256
FAMILIES = ("tie", "big", "sim")
DONE_BYTES = np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)
EV_COLLIDING, EV_GOAL, EV_OUT, EV_MAX_STEPS, EV_NO_GOALS = 0x1, 0x2, 0x4, 0x8, 0x10
ENDING_BITS = (EV_COLLIDING, EV_OUT, EV_MAX_STEPS, EV_NO_GOALS)


# ------------------------------------------------------------------------------------------------------------------------------------
# input builders
# ------------------------------------------------------------------------------------------------------------------------------------
def rewards(family, rng, shape):
    """f64 `shape` of one family."""
    if family == "tie":
        return rng.randint(-3, 4, size=shape) / 8.0
    if family == "big":
        return rng.choice([-1.0, 1.0], size=shape) * 2.0 ** 25
    if family == "sim":
        return rng.choice([1.0, -1.0, -0.01], size=shape)
    raise ValueError(family)


def done_mask(pattern, T, n, rng, offsets=None, sizes=None):
    """bool [T, n], or None where the pattern names envs the shape does not have.  Patterns: "p0", "p0.3", "p1"; "last_env" (the
    handle's last env — with offsets / sizes, each member's last env); "envs_255_256" (the last lane of the first 256-env workgroup and
    the first of the second, whichever exist); "last_row" (row T - 1 alone, half of its envs and at least one)."""
    m = np.zeros((T, n), dtype=bool)
    if pattern == "last_env":
        if offsets is None:
            m[:, n - 1] = True
        else:
            for o, s in zip(offsets, sizes):
                m[:, o + s - 1] = True
    elif pattern == "envs_255_256":
        if n < 256:
            return None
        m[:, 255:257] = True
    elif pattern == "last_row":
        m[T - 1] = rng.random_sample(n) < 0.5
        m[T - 1, rng.randint(n)] = True
    else:
        m = rng.random_sample((T, n)) < float(pattern[1:])
    return m


def done_bytes(rng, mask):
    """uint8: a nonzero byte of DONE_BYTES where mask, 0 elsewhere (a done row is a byte the kernels test against 0, not a bool)."""
    return np.where(mask, DONE_BYTES[rng.randint(0, len(DONE_BYTES), size=mask.shape)], 0).astype(np.uint8)


def flag_bytes(rng, mask):
    """uint8 like mask: random bytes, with every value 0..255 placed once among the done cells and once among the others as far as
    each kind has cells for them (flag_coverage reports what a case got)."""
    f = rng.randint(0, 256, size=mask.shape).astype(np.uint8)
    flat = f.reshape(-1)
    for kind in (mask, ~mask):
        cells = rng.permutation(np.flatnonzero(kind.reshape(-1)))[:256]
        flat[cells] = rng.permutation(256)[:len(cells)].astype(np.uint8)
    return f


def flag_coverage(flags, mask):
    """(distinct byte values on the done cells, distinct byte values on the others)."""
    return len(np.unique(flags[mask])), len(np.unique(flags[~mask]))


def inputs(family, pattern, T, n, seed, offsets=None, sizes=None):
    """(rew f64, done u8, flags u8) [T, n] of one case, or None where the pattern does not exist at this shape."""
    rng = np.random.RandomState(seed)
    mask = done_mask(pattern, T, n, rng, offsets, sizes)
    if mask is None:
        return None
    return rewards(family, rng, (T, n)), done_bytes(rng, mask), flag_bytes(rng, mask)


def sign_by_workgroup(rew, offsets, sizes):
    """rew with its signs laid out per member, in place: a member of more than 256 envs gets |r| in its first workgroup's envs and
    -|r| in the others (partial sums of both signs meet in its triple); of the others the odd-numbered ones, and a population's only
    member, get -|r| (a negative total through the unsigned atomics) and the even-numbered ones |r|."""
    for m, (o, s) in enumerate(zip(offsets, sizes)):
        if s > TILE:
            rew[:, o:o + TILE] = np.abs(rew[:, o:o + TILE])
            rew[:, o + TILE:o + s] = -np.abs(rew[:, o + TILE:o + s])
        else:
            rew[:, o:o + s] = np.abs(rew[:, o:o + s]) * (-1.0 if m % 2 == 1 or len(sizes) == 1 else 1.0)
    return rew


def layout(sizes):
    """(offsets, sizes) of contiguous member slices."""
    sizes = [int(s) for s in sizes]
    return [int(o) for o in np.concatenate(([0], np.cumsum(sizes)[:-1]))], sizes


# ------------------------------------------------------------------------------------------------------------------------------------
# rounding
# ------------------------------------------------------------------------------------------------------------------------------------
def round_even(x):
    """llrint in the default rounding mode: to nearest, ties to even.  (A NaN, which only a defective walk ever rounds, gives the
    integer indefinite, -2^63.)"""
    return -2 ** 63 if x != x else int(np.rint(x))


def round_away(x):
    """The defect: to nearest, ties away from zero (llround)."""
    return -2 ** 63 if x != x else int(math.copysign(math.floor(abs(x) + 0.5), x))


def wrap64(v):
    """A Python integer as the int64 it would be on the device."""
    return ((int(v) + 2 ** 63) % 2 ** 64) - 2 ** 63


def wrap32(v):
    """The defect: an integer kept in 32 bits."""
    return ((int(v) + 2 ** 31) % 2 ** 32) - 2 ** 31


def tie_signs(returns):
    """(positive ties, negative ties) among f64 returns: those whose product with 100 has a fractional part of exactly one half."""
    x = np.asarray(returns, dtype=np.float64) * 100.0
    tie = np.abs(x - np.trunc(x)) == 0.5
    return int(np.count_nonzero(tie & (x > 0))), int(np.count_nonzero(tie & (x < 0)))


# ------------------------------------------------------------------------------------------------------------------------------------
# ssg_pop_episode_stats
# ------------------------------------------------------------------------------------------------------------------------------------
EPISODE_DEFECTS = ("half_away", "trunc32", "drop_negative_partial", "drop_tail", "carry_forgotten")


def episode_stats_walk(rew, done, carry_ret, carry_len, offsets, sizes, defect=None, returns=None, partials=None):
    """ssg_pop_episode_stats over rew f64 / done u8 [K, N]: one env after the other walks t = 0 .. K-1 from its carried return and
    length and counts an episode at its done step as (int(np.rint(cum * 100.0)), len, 1) into the row of the member that owns it.
    Returns (int64 [P, 3], (carry_ret f64 [N], carry_len int32 [N])); the carries given are continued, not modified.  `returns`: a list
    that receives every counted f64 return; `partials`: a list that receives (member, the return100 sum of each run of 256 of its envs).
    `defect`: one of EPISODE_DEFECTS, for the CPU checks of the tests' power only."""
    rew, done = np.asarray(rew, dtype=np.float64), np.asarray(done)
    K, N = rew.shape
    cret, clen = np.array(carry_ret, dtype=np.float64), np.array(carry_len, dtype=np.int32)
    rew_e, done_e = rew.T.tolist(), (done != 0).T.tolist()  # (per env: plain Python floats and bools; float + float is the f64 sum)
    cret_l, clen_l = cret.tolist(), clen.tolist()
    rnd = round_away if defect == "half_away" else round_even
    out = [[0, 0, 0] for _ in sizes]
    for m, (o, s) in enumerate(zip(offsets, sizes)):
        last = o + (s - s % TILE if defect == "drop_tail" and s > TILE else s)
        for g in range(o, last, TILE):  # (a run of 256 envs: the defects on partial sums need them apart)
            part = [0, 0, 0]
            for e in range(g, min(g + TILE, last)):
                cum, ln = (0.0, 0) if defect == "carry_forgotten" else (cret_l[e], clen_l[e])
                r_e, d_e = rew_e[e], done_e[e]
                for t in range(K):
                    cum += r_e[t]
                    ln += 1
                    if d_e[t]:
                        if returns is not None:
                            returns.append(cum)
                        r100 = rnd(cum * 100.0)
                        part[0] += wrap32(r100) if defect == "trunc32" else r100
                        part[1] += ln
                        part[2] += 1
                        cum, ln = 0.0, 0
                cret[e], clen[e] = cum, ln
            if partials is not None:
                partials.append((m, part[0]))
            if defect == "drop_negative_partial" and part[0] < 0:
                part[0] = 0
            for c in range(3):
                out[m][c] += part[c]
    return np.array(out, dtype=np.int64).reshape(len(sizes), 3), (cret, clen)


# ------------------------------------------------------------------------------------------------------------------------------------
# ssg_eval_account with one defect
# ------------------------------------------------------------------------------------------------------------------------------------
EVAL_DEFECTS = ("half_away", "unknown_bit", "goal_next_episode", "first_ending_only", "trunc32", "past_quota")


def eval_walk_with(rew, done, flags, episodes, carry=None, defect=None, returns=None):
    """eval_walk's loop with `defect` switched on (None: eval_walk itself, restated): (rows int64 [N, 8], (ret f64 [N], carry int32
    [N, 4])).  `returns`: a list that receives every counted f64 return.
      half_away          the return rounded half away from zero
      unknown_bit        bit 0x20 counted as a collision
      goal_next_episode  a goal event on the done step credited to the episode that starts there
      first_ending_only  of several ending bits on one done step only the lowest counted
      trunc32            llrint(100 * return) kept in 32 bits
      past_quota         an env that has counted E episodes goes on counting"""
    rew, done, flags = np.asarray(rew, dtype=np.float64), np.asarray(done), np.asarray(flags)
    T, n = rew.shape
    E = int(episodes)
    if carry is None:
        ret, ci = np.zeros(n), np.zeros((n, 4), dtype=np.int32)
    else:
        ret, ci = carry[0].copy(), carry[1].copy()
    rows = [[0] * 8 for _ in range(n)]  # (Python integers; wrapped to int64 at the end)
    rnd = round_away if defect == "half_away" else round_even
    for t in range(T):
        for e in range(n):
            if ci[e, 2] >= E and defect != "past_quota":
                continue
            f = int(flags[t, e])
            goal = 1 if f & EV_GOAL else 0
            ret[e] += rew[t, e]
            ci[e, 0] += 1
            if not (defect == "goal_next_episode" and done[t, e]):
                ci[e, 1] += goal
            if done[t, e]:
                if returns is not None:
                    returns.append(float(ret[e]))
                r100 = rnd(ret[e] * 100.0)
                rows[e][0] += 1
                rows[e][1] += wrap32(r100) if defect == "trunc32" else r100
                rows[e][2] += int(ci[e, 0])
                seen = False
                for c, b in enumerate(ENDING_BITS):
                    hit = bool(f & b) or (defect == "unknown_bit" and b == EV_COLLIDING and bool(f & 0x20))
                    if hit and not (defect == "first_ending_only" and seen):
                        rows[e][3 + c] += 1
                    seen = seen or hit
                rows[e][7] += int(ci[e, 1])
                ret[e] = 0.0
                ci[e, 0] = 0
                ci[e, 1] = goal if defect == "goal_next_episode" else 0
                ci[e, 2] += 1
    return np.array([[wrap64(v) for v in row] for row in rows], dtype=np.int64).reshape(n, 8), (ret, ci)


# ------------------------------------------------------------------------------------------------------------------------------------
# ssg_pop_exploit
# ------------------------------------------------------------------------------------------------------------------------------------
def exploit_sources(P, seed=0):
    """{name: src} of the accepted source vectors at P members: the identity; every member from member 0 and from member P - 1;
    disjoint pairs (2j takes 2j + 1); at P >= 256 "upper_half": the members below 128 draw their sources from [128, P), indices a
    signed byte cannot hold."""
    rng = np.random.RandomState(seed + P)
    out = {"identity": list(range(P)), "all_from_0": [0] * P, "all_from_last": [P - 1] * P,
           "pairs": [m + 1 if m % 2 == 0 and m + 1 < P else m for m in range(P)]}
    if P >= 256:
        out["upper_half"] = [int(x) for x in rng.randint(128, P, 128)] + list(range(128, P))
    return out


def refused_sources(P):
    """{name: src} of vectors ssg_pop_exploit refuses: an index out of range on either side, and (from two members on) a source that
    is itself a destination."""
    out = {"above_range": [P] + list(range(1, P)), "negative": list(range(P - 1)) + [-1]}
    if P >= 2:
        out["chained"] = [1, 0] + list(range(2, P)) if P == 2 else [1, 2] + list(range(2, P))
    return out


def exploit_reference(rows, src, defect=None):
    """rows [P, ...] after the exploit: row m is row src[m] as it was.  defect "seven_bits": the source index loses its eighth bit
    (where a signed byte would go negative)."""
    idx = np.asarray(src, dtype=np.int64)
    if defect == "seven_bits":
        idx = idx & 0x7F
    return np.asarray(rows)[idx]


# ------------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ------------------------------------------------------------------------------------------------------------------------------------
def same_bits(got, want):
    """Equal shapes, dtypes and bytes: -0.0 is not 0.0, and a NaN equals itself."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
