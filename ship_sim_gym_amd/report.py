"""The update report — how an update went, reduced on the device (ssg_ppo_report / ssg_pop_report), and the CSV the trainers keep of it.

The reference's Stable-Baselines script runs PPO2 with verbose=1 and a tensorboard_log (train/stable_baselines/ppo.py:88-90), which prints
and logs explained_variance, approxkl, clipfrac, policy_entropy, policy_loss and value_loss per update; RLlib's PPO
(train/rllib/ppo.py:26-41, train/rllib/pbt.py:47-74) reports vf_explained_var, kl, entropy, policy_loss, vf_loss, cur_kl_coeff and cur_lr.
``NativePPO.report`` / ``PopulationPPO.report`` return the same quantities from two launches over the rollout batch (plus one
ssg_ppo_dist / ssg_pop_dist launch with ``post=True``, which measures how far the update moved the policy); ``report_reference`` restates
the launches in numpy in their order of operations, and the device's record is that restatement bit for bit.  ``ProgressWriter`` is the
counterpart of Stable-Baselines' progress.csv.

A data-parallel job's record is taken over the experience of all its ranks, as RLlib's is over its workers' (train/rllib/ppo.py:34-35):
every rank reduces its shard to one sum row (ssg_ppo_report_sums: the walk's nine totals, n, the post flag), the rows are all-gathered,
and every rank forms the same record from the same rows in rank order (ssg_ppo_report_rows).  ``NativePPO.job_report`` does that;
``sums_reference`` / ``rows_reference`` restate the two calls, and one row gives ``report_reference``'s record bit for bit.

The ``lr`` and ``clip`` entries of a record are the trainer's current values: under a hyper-parameter schedule
(ship_sim_gym_amd/hparam_schedule.py) they vary from update to update, and so do ``ProgressWriter``'s two columns.

Out of scope: the episode log or populations across ranks, the
entropy or exact KL of the post-update policy over the whole batch (both need exp), a TensorBoard event writer.
"""
import ctypes as C
import os
import time

import numpy as np

from . import _native as N
from .ppo import _tree256

# the record's f64 columns (include/shipsim.h); 12..19 are named after the stats rows of the update entry points
REPORT_FIELDS = (
    "n", "ret_mean", "ret_var", "err_mean", "err_var", "explained_variance", "value_mean", "adv_mean",
    "post", "approx_kl", "approxkl_ppo2", "clip_fraction",
    "policy_loss", "value_loss", "entropy", "clip_fraction_minibatch", "kl", "grad_norm", "kl_coef", "unused19",
    "stats_rows", "unused21", "unused22", "unused23",
)
assert len(REPORT_FIELDS) == N.REPORT_COLS
REPORT_SUMS = 9  # the walk's sums per lane: ret, ret^2, err, err^2, val, adv, d, d^2, clipped
PROGRESS_FIELDS = tuple(f for f in REPORT_FIELDS if not f.startswith("unused"))
PROGRESS_COLUMNS = ("update", "timesteps", "member") + PROGRESS_FIELDS + ("lr", "clip", "t")


def clip_bounds(clip):
    """ssg_report_clip_bounds: (lo, hi) as np.float32 — (float)log1p(-clip), -inf from clip 1 on, and (float)log1p(clip), formed in
    double by the library, so that the host and the device compare against the same bits."""
    out = (C.c_float * 2)()
    N.call("ssg_report_clip_bounds", float(clip), out)
    return np.float32(out[0]), np.float32(out[1])


def _walk_totals(who, val, ret, adv, act, logp, logp_all_new, clip):
    """The walk and the two reductions behind it, in the device's order of operations: (K, n, post, the nine totals).  Per env the f64
    sums in ascending t, every product and sum separately rounded; the 256-env blocks' halving trees; the blocks' partials added per
    thread (block b, b + 256, ...) and one more tree."""
    f64 = np.float64
    val, ret, adv = (np.asarray(x, dtype=np.float32) for x in (val, ret, adv))
    K, n = val.shape
    post = logp_all_new is not None
    if post != (act is not None) or post != (logp is not None):
        raise ValueError("%s: act, logp and logp_all_new go together" % who)
    nb = -(-n // 256)
    s = np.zeros((nb * 256, REPORT_SUMS))
    if post:
        act, logp = np.asarray(act).astype(np.int64) & 3, np.asarray(logp, dtype=np.float32)
        lpa = np.asarray(logp_all_new, dtype=np.float32).reshape(K, n, 4)
        lo, hi = clip_bounds(clip)
        cols = np.arange(n)
    for t in range(K):
        r, v, a = ret[t].astype(f64), val[t].astype(f64), adv[t].astype(f64)
        err = r - v
        s[:n, 0] += r
        s[:n, 1] += r * r
        s[:n, 2] += err
        s[:n, 3] += err * err
        s[:n, 4] += v
        s[:n, 5] += a
        if post:
            d = lpa[t, cols, act[t]] - logp[t]  # one f32 subtraction
            dd = d.astype(f64)
            s[:n, 6] += dd
            s[:n, 7] += dd * dd
            s[:n, 8] += ((d > hi) | (d < lo)).astype(f64)
    part = np.zeros((-(-nb // 256) * 256, REPORT_SUMS))
    for b in range(nb):
        part[b] = _tree256(s[b * 256: b * 256 + 256].copy())
    acc = np.zeros((256, REPORT_SUMS))
    for r in range(part.shape[0] // 256):  # thread j: partials j, j + 256, ... in that order
        acc += part[r * 256: r * 256 + 256]
    return K, n, post, _tree256(acc)


def report_reference(val, ret, adv, act=None, logp=None, logp_all_new=None, clip=0.2, stats=None, rows=None):
    """ssg_ppo_report restated in numpy, in the device's order of operations: the f64 [24] record of ONE policy (a population member:
    its own columns, bounds and rows).  val / ret / adv f32 [K, n]; the post-update group act i32 [K, n], logp f32 [K, n] and
    logp_all_new f32 [K, n, 4] together or not at all; stats f32 [rows_max, 4 or 8] with rows (None: all of them) used.

    The walk and its reductions (_walk_totals), then the record's formulas (_record_from_sums): the finish kernel's two halves."""
    K, n, post, tot = _walk_totals("report_reference", val, ret, adv, act, logp, logp_all_new, clip)
    return _record_from_sums(tot, np.float64(K) * np.float64(n), int(post), stats, rows, "report_reference")


def sums_reference(val, ret, adv, act=None, logp=None, logp_all_new=None, clip=0.2):
    """ssg_ppo_report_sums restated in numpy, in the device's order of operations: a shard's sum row, f64 [12] = the walk's nine totals
    (report_reference's walk, partials and tree), n = K * n_envs, the post flag, 0.  Without the post group columns 6..8 are 0."""
    K, n, post, tot = _walk_totals("sums_reference", val, ret, adv, act, logp, logp_all_new, clip)
    row = np.zeros(N.REPORT_ROW_COLS)
    row[:REPORT_SUMS] = tot
    row[REPORT_SUMS] = np.float64(K) * np.float64(n)
    row[REPORT_SUMS + 1] = 1.0 if post else 0.0
    return row


def _record_from_sums(tot, cnt, post, stats, rows_used, who="rows_reference"):
    """The record's formulas (the device's form_record) from the nine totals, the count, the post state (1 on, 0 off, else NaN in
    [8..11]) and the stats rows."""
    f64 = np.float64
    out = np.zeros(N.REPORT_COLS)
    with np.errstate(all="ignore"):
        mr = tot[0] / cnt
        vr = (tot[1] - tot[0] * mr) / cnt
        vr = f64(0.0) if vr < 0.0 else vr
        me = tot[2] / cnt
        ve = (tot[3] - tot[2] * me) / cnt
        ve = f64(0.0) if ve < 0.0 else ve
        out[0:5] = cnt, mr, vr, me, ve
        out[5] = np.nan if vr == 0.0 else f64(1.0) - ve / vr
        out[6], out[7] = tot[4] / cnt, tot[5] / cnt
        if post == 1:
            out[8], out[9], out[10], out[11] = 1.0, -(tot[6] / cnt), f64(0.5) * (tot[7] / cnt), tot[8] / cnt
        elif post != 0:
            out[8:12] = np.nan
        if stats is not None:
            st = np.asarray(stats, dtype=np.float32)
            st = st.reshape(-1, st.shape[-1])
            if st.shape[1] not in (4, 8) or st.shape[0] < 1:
                raise ValueError("%s: stats must be f32 [rows >= 1, 4 or 8]" % who)
            used = st.shape[0] if rows_used is None else max(0, min(int(rows_used), st.shape[0]))
            colsum = np.zeros(st.shape[1])
            for j in range(used):  # one thread per column, its rows in row order
                colsum += st[j].astype(f64)
            if used > 0:
                out[N.REPORT_STATS: N.REPORT_STATS + st.shape[1]] = colsum / f64(used)
            out[N.REPORT_ROWS] = used
    return out


def rows_reference(rows, stats=None, rows_used=None, per_shard=False):
    """ssg_ppo_report_rows restated in numpy: the job's record f64 [24] from the sum rows f64 [W, 12] in shard order — column c
    accumulated in row order from row 0's value on, n likewise, then the record's formulas; the post group on when every row's flag is
    1.0, off when every row's is 0.0, NaN in [8..11] otherwise.  stats f32 [rows, 4 or 8] with rows_used (None: all; the device call
    uses all it is given) as in report_reference.  per_shard: [1 + W, 24], record 1 + r formed from row r alone."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, N.REPORT_ROW_COLS)

    def one(block):
        tot = block[0, :REPORT_SUMS + 1].copy()
        for r in block[1:]:
            tot = tot + r[:REPORT_SUMS + 1]
        flags = block[:, REPORT_SUMS + 1]
        post = 1 if np.all(flags == 1.0) else 0 if np.all(flags == 0.0) else -1
        return _record_from_sums(tot[:REPORT_SUMS], tot[REPORT_SUMS], post, stats, rows_used)

    if rows.shape[0] < 1:
        raise ValueError("rows_reference: no rows")
    if not per_shard:
        return one(rows)
    return np.stack([one(rows)] + [one(rows[r: r + 1]) for r in range(rows.shape[0])])


def record_dict(row):
    """A record row (24 numbers) as {field: Python float}."""
    return {k: float(x) for k, x in zip(REPORT_FIELDS, row)}


def scratch_nbytes(n_envs, n_members=1):
    """ssg_ppo_report_workspace_nbytes."""
    return N.nbytes("ssg_ppo_report_workspace_nbytes", int(n_envs), int(n_members))


class ProgressWriter(object):
    """The CSV of the update reports: one row per member per update, ``update, timesteps, member``, then the record's fields (without
    the unused columns), ``lr, clip`` and ``t`` — the host's seconds since the writer was made, the only column that is not
    reproducible (as in ``MonitorWriter``).  Floats are written with %r, so they read back bit for bit.

    resume=False starts the file anew.  resume=True leaves it; ``cut_back(update)`` then keeps the header and the rows whose ``update``
    is at most the checkpoint's and cuts the rest (through FILE.tmp and os.replace), so that a run that is saved, killed and resumed
    leaves the uninterrupted run's file in every column but ``t``."""

    def __init__(self, path, resume=False):
        self.path = os.fspath(path)
        self.t_start = time.time()
        if resume and os.path.exists(self.path):  # (a run resumed with a progress file it did not have before starts one)
            self._read()
        else:
            with open(self.path, "w") as f:
                f.write(",".join(PROGRESS_COLUMNS) + "\n")

    def _read(self):
        try:
            with open(self.path) as f:
                lines = f.read().splitlines(True)
            if not lines or lines[0].strip() != ",".join(PROGRESS_COLUMNS):
                raise ValueError("no progress header")
            return lines
        except (OSError, ValueError) as ex:
            raise ValueError("ProgressWriter: %s is not a progress file of this format (%s)" % (self.path, ex))

    def cut_back(self, update):
        """Keep the header and the rows with ``update`` <= update; returns how many rows were cut."""
        lines = self._read()
        keep = [lines[0]] + [ln for ln in lines[1:] if ln.strip() and int(ln.split(",", 1)[0]) <= int(update)]
        with open(self.path + ".tmp", "w") as f:
            f.writelines(ln if ln.endswith("\n") else ln + "\n" for ln in keep)
        os.replace(self.path + ".tmp", self.path)
        return len(lines) - len(keep)

    def write(self, update, timesteps, records, lr, clip):
        """Append one row per member: records is one record (a dict of REPORT_FIELDS, as NativePPO.report returns) or a dict of arrays
        [P] (PopulationPPO.report); lr / clip are scalars or [P]."""
        t = round(time.time() - self.t_start, 6)
        cols = [np.atleast_1d(np.asarray(records[k], dtype=np.float64)) for k in PROGRESS_FIELDS]
        P = cols[0].shape[0]
        lr, clip = (np.broadcast_to(np.asarray(x, dtype=np.float64), (P,)) for x in (lr, clip))
        with open(self.path, "a") as f:
            for m in range(P):
                f.write("%d,%d,%d,%s,%r,%r,%r\n" % (int(update), int(timesteps), m, ",".join("%r" % float(c[m]) for c in cols),
                                                  float(lr[m]), float(clip[m]), t))
        return P


def read_progress(path):
    """A progress file as {column: numpy array} (int64 for update / timesteps / member, f64 otherwise)."""
    with open(os.fspath(path)) as f:
        names = f.readline().strip().split(",")
        rows = [line.strip().split(",") for line in f if line.strip()]
    ints = ("update", "timesteps", "member")
    return {name: np.array([int(r[i]) if name in ints else float(r[i]) for r in rows], dtype=np.int64 if name in ints else np.float64)
            for i, name in enumerate(names)}
