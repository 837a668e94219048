"""DataParallelPPO — one policy trained from the experience of W env shards (ssg_ppo_adv_moments / ssg_ppo_set_adv_moments /
ssg_ppo_apply_shards).

The RLlib reference scripts collect experience on cpu_count() - 1 workers and train ONE policy from all of it (train/rllib/ppo.py:34-35,
train/rllib/pbt.py:57-58); the Stable-Baselines script does the same over a SubprocVecEnv (train/stable_baselines/ppo.py:122-123).  Here
every rank owns an env shard (sharding.make_sharded_env) and a full copy of the policy.  Per minibatch a rank computes the gradient of
ITS chunk (ssg_ppo_grad / ssg_ppo_grad_ext: the local row), the rows are all-gathered, and every rank applies the same combined
gradient with the same arithmetic (ssg_ppo_apply_shards): the parameters, Adam moments and KL coefficient stay bit-identical on every
rank with no parameter broadcast.  The advantage statistics are job-wide in the same way: gae() gathers the shards' f64 moments.

Rank r shuffles its own samples: ``member`` defaults to the rank, so draw_perm keys the rank's permutation rows by it.  Epoch e's chunk j
of the job is the union of the ranks' chunks j; the shards must make the same number of chunks (ValueError on every rank otherwise).

The two halves of a minibatch are public so that ONE process can replay a W-rank job over the ranks' batches: ``shard_moments`` /
``set_moments`` and ``local_row`` / ``apply_rows`` with torch.stack as the gather.  ``apply_reference`` and ``moments_reference`` restate
the two device steps in numpy, operation for operation.

The observation filter of such a job is ship_sim_gym_amd/obs_filter.py's ``ObsFilter(job=True)``: rank-local during a rollout,
synchronised after it by the same pattern (gathered buffers, the same merge on every rank).

The return filter of such a job is ship_sim_gym_amd/ret_filter.py's ``ReturnFilter(job=True)``: ``gae`` hands it the group, the
ranks gather one [K, 4] block of per-step rows per rollout and chain them alike, which is exact: one filter over all the job's envs.

The update report of such a job is ``job_report`` (ship_sim_gym_amd/report.py): every rank reduces its shard to one f64 sum row, the rows
are all-gathered once per update, and every rank forms the same record from them in rank order, replayable in one process with
``report_row`` / ``report_rows`` and torch.stack.  ``report`` stays the rank's own shard's.

The episode log of such a job is ship_sim_gym_amd/episode_log.py's ``EpisodeLog(job=True)``: every rank packs its shard's finished
episodes of a rollout into one fixed-size block, the blocks are all-gathered once, and every rank merges them into the same ring in the
order one log over all the job's envs would keep, replayable in one process with ``shard_block`` / ``merge_blocks`` and torch.stack.

PPO2's per-minibatch advantage normalisation of such a job is ``DataParallelPPO(job_adv_norm="minibatch")``: the advantages are fixed
once GAE has run and a rank's permutations are known before its first gradient, so every rank sums adv, adv^2 and 1 over EACH minibatch
of the update in one pass (ssg_ppo_minibatch_adv_sums), the [epochs * chunks, 4] blocks are all-gathered once per update, and every rank
forms the same table of stats rows from them in rank order (ssg_ppo_set_minibatch_adv_rows); the per-minibatch loop then only selects
its row.  Replayable in one process with ``shard_minibatch_sums`` / ``set_minibatch_rows`` / ``select_minibatch`` and torch.stack;
``minibatch_sums_reference`` and ``minibatch_rows_reference`` restate the two steps in numpy.  ``adv_norm="minibatch"`` (the
single-handle mode, whose statistics are one shard's) stays refused.

Out of scope: resuming a multi-rank run, populations across ranks, a gather per minibatch, overlapping the gather with the next
gradient, running this loop from C.
"""
import ctypes as C

from . import _native as N
from ._native import _torch
from .ppo import NativePPO, _tree256, adv_stats_row_reference, chunk_split, minibatch_adv_sums_reference
from .sharding import all_gather_rows


def _world(group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def shard_chunks(K, shard_envs, minibatches):
    """[(chunk length, chunks)] per shard for a rollout of K steps: chunk_split of each shard's K * envs samples."""
    return [chunk_split(int(K) * int(e), minibatches) for e in shard_envs]


def chunk_counts(K, shard_envs, minibatches, j):
    """The shards' sample counts M_r of chunk j (the host array ssg_ppo_apply_shards weighs the rows by)."""
    return [min(c, int(K) * int(e) - j * c) for (c, _), e in zip(shard_chunks(K, shard_envs, minibatches), shard_envs)]


# ------------------------------------------------------------------------------------------------------------------------------------
# numpy restatements of the device steps
# ------------------------------------------------------------------------------------------------------------------------------------
def moments_reference(rows, adv_eps):
    """ssg_ppo_set_adv_moments in numpy: rows f64 [W, 4] = {S, Q, n, 0} per shard, summed in row order, then gae_boot_reference's
    formula: the stats row f32 [4] = {mean, std + adv_eps, its inverse, 0} (NaN, NaN, NaN, 0 for fewer than 2 samples)."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
    S = Q = n = 0.0
    for r in rows:
        S, Q, n = S + r[0], Q + r[1], n + r[2]
    if not n >= 2.0:
        return np.array([np.nan, np.nan, np.nan, 0.0], dtype=np.float32)
    mean = S / n
    var = (Q - S * mean) / (n - 1.0)
    if var < 0.0:  # (the device's comparison: a NaN variance stays NaN, which max(0.0, var) would turn into 0)
        var = 0.0
    stdp = np.float32(np.sqrt(var)) + np.float32(adv_eps)
    return np.array([np.float32(mean), stdp, np.float32(1.0) / stdp, 0.0], dtype=np.float32)


def minibatch_sums_reference(adv, perm, chunk, n_samples, partials=False):
    """ssg_ppo_minibatch_adv_sums in numpy, in the device's order of operations: f64 [epochs * C, 4] rows {s, q, c, 0}, C = ceil(n /
    chunk), row e * C + j for the minibatch perm[e][j * chunk: min(n, (j + 1) * chunk)].  adv: f32, flat; perm: int64 [epochs, n]; an
    index outside [0, n_samples) counts for nothing.  partials=True: (rows, the list of every minibatch's f64 [B, 3] partials)."""
    import numpy as np
    adv = np.asarray(adv, dtype=np.float32).reshape(-1)
    perm = np.asarray(perm, dtype=np.int64)
    epochs, n = perm.shape
    C_ = -(-n // int(chunk))
    rows, parts = np.zeros((epochs * C_, 4)), []
    for e in range(epochs):
        for j in range(C_):
            idx = perm[e, j * int(chunk): min(n, (j + 1) * int(chunk))]
            valid = (idx >= 0) & (idx < int(n_samples))
            s, q, cnt, part = minibatch_adv_sums_reference(adv[np.where(valid, idx, 0)], valid)
            rows[e * C_ + j, :3] = s, q, cnt
            parts.append(part)
    return (rows, parts) if partials else rows


def minibatch_rows_reference(rows, adv_eps):
    """ssg_ppo_set_minibatch_adv_rows in numpy: rows f64 [W, n_batches, 4], per minibatch the shards' S, Q and C added in rank order
    starting from rank 0's, then ppo.adv_stats_row_reference's formula: the table f32 [n_batches, 4]."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 3 or rows.shape[2] != 4:
        raise ValueError("minibatch_rows_reference: rows must be f64 [W, n_batches, 4] (got %s)" % (rows.shape,))
    table = np.zeros((rows.shape[1], 4), dtype=np.float32)
    with np.errstate(all="ignore"):
        for b in range(rows.shape[1]):
            S, Q, cnt = rows[0, b, :3]
            for r in range(1, rows.shape[0]):
                S, Q, cnt = S + rows[r, b, 0], Q + rows[r, b, 1], cnt + rows[r, b, 2]
            table[b] = adv_stats_row_reference(S, Q, cnt, adv_eps)
    return table


def shard_weights(counts):
    """w_r = float32(M_r / sum M), the division in double."""
    import numpy as np
    total = float(sum(int(c) for c in counts))
    return np.array([np.float32(float(int(c)) / total) for c in counts], dtype=np.float32)


def adam_reference(g, params, adam_mv, step, hp):
    """One Adam step of ssg_ppo_adam in numpy f32, every product, quotient and sum rounded on its own: (params, adam_mv) after step
    `step` (>= 1) with gradient g.  hp: an object or dict with lr, beta1, beta2, eps."""
    import numpy as np
    f32 = np.float32
    get = (lambda k: hp[k]) if isinstance(hp, dict) else (lambda k: getattr(hp, k))
    lr, b1, b2, eps = (float(get(k)) for k in ("lr", "beta1", "beta2", "eps"))
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    w1 = f32(1.0 - b1)
    omw1, beta2, w2 = f32(1.0) - w1, f32(b2), f32(1.0 - b2)
    bc2_sqrt, epsf, step_size = f32(np.sqrt(bc2)), f32(eps), f32(-(lr / bc1))
    g = np.asarray(g, dtype=f32)
    P = g.size
    p, mv = np.asarray(params, dtype=f32).copy(), np.asarray(adam_mv, dtype=f32).copy()
    m, v = mv[:P], mv[P:]
    m = m + w1 * (g - m) if abs(w1) < 0.5 else g - (g - m) * omw1
    v = v * beta2
    v = v + w2 * (g * g)
    den = np.sqrt(v) / bc2_sqrt + epsf
    p = p + step_size * (m / den)
    return p.astype(f32), np.concatenate([m, v]).astype(f32)


def apply_reference(rows, counts, params, adam_mv, step, hp, max_grad_norm=0.0, ext=False, kl_coef=None, klacc=0.0, first_chunk=True,
                    last_chunk=False, n_chunks=1, kl_target=0.0):
    """ssg_ppo_apply_shards in numpy, in the device's order of operations.  rows f32 [W, P + 8], counts the W sample counts, params f32
    [P], adam_mv f32 [2P], step the Adam step to take.  ext: the extended loss's columns (kl_coef: the coefficient in use or None;
    klacc: the running KL sum before the call).  Returns a dict: g (the combined gradient, unclipped), norm and coef (f32; 0 and 1
    with the clip off), params, adam_mv, stats f32 [8] (columns 4..7 zero under the plain loss), klacc and kl_coef after the call."""
    import numpy as np
    f32 = np.float32
    rows = np.asarray(rows, dtype=f32)
    W, stride = rows.shape
    P = stride - 8
    w = shard_weights(counts)
    s = w[0] * rows[0]
    for r in range(1, W):
        s = s + w[r] * rows[r]  # (f32 arrays: the product and the sum are rounded separately)
    g, tail = s[:P].copy(), s[P:]
    klc = f32(kl_coef) if (ext and kl_coef is not None) else f32(0.0)
    stats = np.zeros(8, dtype=f32)
    ncol = 5 if ext else 4  # (the plain loss has no KL column: whatever the rows hold there, columns 4..7 are zero)
    stats[:ncol] = tail[:ncol]
    stats[6] = klc if klc > 0 else f32(0.0)
    klacc = f32(klacc)
    if ext:
        klacc = f32(tail[4]) if first_chunk else f32(klacc + tail[4])
    norm, coef = f32(0.0), f32(1.0)
    clip = ext and max_grad_norm > 0.0
    if clip:
        nb = -(-stride // 256)
        sq = np.zeros(nb * 256)
        sq[:P] = g.astype(np.float64) ** 2
        total = 0.0
        for b in range(nb):  # the workgroups' trees, then the partials in index order
            total += float(_tree256(sq[b * 256: b * 256 + 256].copy().reshape(256, 1))[0])
        norm = f32(np.sqrt(total))
        coef = min(f32(1.0), f32(max_grad_norm) / (norm + f32(1e-6)))
        stats[5] = norm
    p2, mv2 = adam_reference(g * coef if clip else g, params, adam_mv, step, hp)
    kl_out = None if kl_coef is None else f32(kl_coef)
    if ext and last_chunk and kl_coef is not None and kl_target > 0.0:
        mean, t = f32(klacc / f32(n_chunks)), f32(kl_target)
        if mean > f32(2.0) * t:
            kl_out = f32(kl_out * f32(1.5))
        elif mean < f32(0.5) * t:
            kl_out = f32(kl_out * f32(0.5))
    return {"g": g, "norm": norm, "coef": f32(coef), "params": p2, "adam_mv": mv2, "stats": stats, "klacc": klacc, "kl_coef": kl_out}


def check_return_filter(return_filter, world):
    """Which return filters serve a job of `world` ranks: a job filter any, a plain one only a job of one rank — with more, the
    statistics it divides by would be the rank's own (ValueError, on every rank alike)."""
    if return_filter is not None and int(world) > 1 and not getattr(return_filter, "job", False):
        raise ValueError("DataParallelPPO.gae: a plain ReturnFilter in a job of %d ranks would normalise by this rank's statistics, not "
                         "the job's: make it with ReturnFilter(env, job=True)" % int(world))


JOB_ADV_NORM_MODES = ("batch", "minibatch")


# ------------------------------------------------------------------------------------------------------------------------------------
class DataParallelPPO(NativePPO):
    """NativePPO over this rank's shard of a W-rank job.  group: the process group (None: the default one; with none initialised the
    job is this process alone, W = 1, and every result is NativePPO's bit for bit).  plan=(K, minibatches): check at construction that
    the shards make the same number of chunks for that rollout length and minibatch count (update() checks what it is given).
    ``report`` / ``report_device`` are NativePPO's: the record is then this rank's OWN shard's (its n, means, variances and post-update
    group; the stats rows' means are the job's, since every rank holds the same rows).  ``job_report`` gives the JOB's record: every
    rank's sum row gathered once, the same record formed on every rank (ssg_ppo_report_sums / ssg_ppo_report_rows).
    job_adv_norm="minibatch": PPO2's rule over the job — the advantages of a minibatch are normalised by the statistics of the JOB's
    minibatch, from one gather per update (the module's docstring); "batch" (the default): once per rollout, gae()'s job statistics.
    The clock of the hyper-parameter schedules (``set_timesteps``) is the JOB's — the timesteps collected over all ranks, which the
    caller computes from the job's total env count, the same integer on every rank — so the ranks stay bit-identical with no broadcast."""

    def __init__(self, policy, env, group=None, plan=None, job_adv_norm="batch", **kw):
        if kw.get("adv_norm", "batch") != "batch":
            raise ValueError("DataParallelPPO: adv_norm must be 'batch' (per-minibatch statistics across ranks are out of scope; got %r)"
                             % (kw["adv_norm"],))
        if job_adv_norm not in JOB_ADV_NORM_MODES:
            raise ValueError("DataParallelPPO: job_adv_norm must be 'batch' or 'minibatch' (got %r)" % (job_adv_norm,))
        self.job_adv_norm = job_adv_norm
        self._job_table = None    # f32 [epochs * chunks, 4]: the update's stats rows (set_minibatch_rows)
        self._job_scratch = None  # ssg_ppo_minibatch_adv_sums' partials
        self._job_chunks = 0      # chunks per epoch of the sums last taken: select_minibatch's row stride
        self._job_row = 0
        self.group = group
        self.rank, self.world = _world(group)
        if self.world > N.DP_MAX_SHARDS:
            raise ValueError("DataParallelPPO: %d ranks, ssg_ppo_apply_shards combines at most %d" % (self.world, N.DP_MAX_SHARDS))
        kw.setdefault("member", self.rank)
        super(DataParallelPPO, self).__init__(policy, env, **kw)
        torch = _torch()
        mine = torch.tensor([int(env.num_envs)], dtype=torch.int64, device=policy.device)
        self.shard_envs = [int(v) for v in all_gather_rows(mine, group).reshape(-1).cpu().tolist()]
        self._since_first = 0  # applies since the last first_chunk: the adaptation's divisor
        if plan is not None:
            self.check_chunks(*plan)

    def check_chunks(self, K, minibatches):
        """(chunks, the shards' chunk lengths) for a rollout of K steps; ValueError — on every rank alike, from the gathered shard
        sizes — when the shards would make different numbers of chunks."""
        sc = shard_chunks(K, self.shard_envs, minibatches)
        if len(set(c for _, c in sc)) != 1:
            raise ValueError("DataParallelPPO: with K = %d and %d minibatches the shards of %s envs make %s chunks: every rank must make "
                             "the same number" % (int(K), int(minibatches), self.shard_envs, [c for _, c in sc]))
        return sc[0][1], [c for c, _ in sc]

    def _ws(self, n_samples, max_minibatch):
        """NativePPO's workspace; when it grows, its first 512 bytes are kept: the advantage statistics and, behind them, the
        apply's running KL sum, which lives across the minibatches of an epoch."""
        return self._grow("ssg_ppo_workspace_nbytes", self.policy.to_native(), n_samples, max_minibatch, 512)

    # ------------------------------------------------------------------------------------------------
    # advantage statistics over the job
    # ------------------------------------------------------------------------------------------------
    def shard_moments(self, batch):
        """f64 [4] on the device: {sum adv, sum adv^2, K*N, 0} of the batch gae() has JUST seen (ssg_ppo_adv_moments re-adds GAE's
        partials, which the first gradient call overwrites)."""
        torch = _torch()
        K, n_env = int(batch["adv"].shape[0]), int(batch["adv"].shape[1])
        out = torch.empty(4, dtype=torch.float64, device=self.policy.device)
        self.env.enqueue("ssg_ppo_adv_moments", K, n_env, *self._ws_ptr(), out.data_ptr())
        return out

    def set_moments(self, rows):
        """The job's statistics from the gathered moments rows (f64 [W, 4], shard order) into the workspace, where every gradient call
        reads them (adv_stats() shows them)."""
        torch = _torch()
        rows = rows.to(device=self.policy.device, dtype=torch.float64).contiguous()
        rp = N.arg(rows, torch.float64, (0, 4), "DataParallelPPO.set_moments: rows", self._device, more_rows=True)
        self._ws(1, 1)
        self.env.enqueue("ssg_ppo_set_adv_moments", int(rows.shape[0]), rp, float(self.hp.adv_eps), *self._ws_ptr())

    # ------------------------------------------------------------------------------------------------
    # per-minibatch advantage statistics over the job (job_adv_norm="minibatch")
    # ------------------------------------------------------------------------------------------------
    def _bind_adv_norm(self):
        """(Re)bind this object's source of statistics on the env (host only): the batch mode, which drops a table another trainer
        left, or this object's table and the row it selected last."""
        if self.job_adv_norm != "minibatch":
            return super(DataParallelPPO, self)._bind_adv_norm()
        if self._job_table is None:
            raise ValueError("DataParallelPPO: job_adv_norm='minibatch' and no table yet: call set_minibatch_rows first (update() does)")
        self.env.set_adv_table(self._job_table)
        self.env.select_adv_row(self._job_row)

    def _need_job_mode(self, who):
        if self.job_adv_norm != "minibatch":
            raise ValueError("DataParallelPPO.%s: job_adv_norm is %r" % (who, self.job_adv_norm))

    def shard_minibatch_sums(self, batch, perm, minibatches, partials=False):
        """f64 [epochs * C, 4] on the device: {sum adv, sum adv^2, count, 0} of every minibatch update(batch, perm, epochs, minibatches)
        would cut from THIS shard's samples — row e * C + j for perm[e].chunk(minibatches)[j] (ssg_ppo_minibatch_adv_sums; two launches,
        enqueued only).  perm: int64 [epochs, n] over the batch's n samples.  partials=True: (rows, the f64 [epochs * C, 64, 3] view of
        the scratch, of which a minibatch of M indices wrote its first min(64, ceil(M / 1024)))."""
        torch = _torch()
        self._need_job_mode("shard_minibatch_sums")
        dev = self.policy.device
        adv = self._flat(batch, "adv", torch.float32)
        n = adv.numel()
        perm = perm.to(device=dev, dtype=torch.int64).contiguous()
        if perm.dim() != 2 or int(perm.shape[1]) != n:
            raise ValueError("DataParallelPPO.shard_minibatch_sums: perm must be int64 [epochs, %d] (got %s)" % (n, tuple(perm.shape)))
        epochs = int(perm.shape[0])
        chunk, chunks = chunk_split(n, minibatches)
        nb = epochs * chunks
        need = N.nbytes("ssg_ppo_minibatch_adv_nbytes", nb)
        if self._job_scratch is None or self._job_scratch.numel() < need:
            self._job_scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
        out = torch.empty((nb, 4), dtype=torch.float64, device=dev)
        self.env.enqueue("ssg_ppo_minibatch_adv_sums", n, adv.data_ptr(), perm.data_ptr(), epochs, n, chunk, out.data_ptr(),
                         self._job_scratch.data_ptr(), self._job_scratch.numel())
        self._job_chunks = chunks
        if partials:
            return out, self._job_scratch[:nb * N.ADV_NORM_BLOCKS * 24].view(torch.float64).view(nb, N.ADV_NORM_BLOCKS, 3)
        return out

    def set_minibatch_rows(self, rows):
        """The update's table of stats rows from the gathered sums (f64 [W, epochs * C, 4], shard order), bound to the env with row 0
        selected (ssg_ppo_set_minibatch_adv_rows, one launch; ssg_ppo_set_adv_table).  ``minibatch_table()`` shows it."""
        torch = _torch()
        self._need_job_mode("set_minibatch_rows")
        dev = self.policy.device
        rows = rows.to(device=dev, dtype=torch.float64).contiguous()
        if rows.dim() != 3:
            raise ValueError("DataParallelPPO.set_minibatch_rows: rows must be f64 [W, epochs * chunks, 4] (got %s)" % (tuple(rows.shape),))
        W, nb = int(rows.shape[0]), int(rows.shape[1])
        rp = N.arg(rows, torch.float64, (W, nb, 4), "DataParallelPPO.set_minibatch_rows: rows", dev)
        table = torch.empty((nb, 4), dtype=torch.float32, device=dev)  # (a new one per update: the last one may still be read)
        self.env.enqueue("ssg_ppo_set_minibatch_adv_rows", W, nb, rp, float(self.hp.adv_eps), table.data_ptr())
        self._job_table, self._job_row = table, 0
        self._bind_adv_norm()
        return table

    def select_minibatch(self, e, j):
        """Select the row of minibatch j of epoch e for the next ``local_row`` (host only)."""
        self._need_job_mode("select_minibatch")
        if self._job_table is None:
            raise ValueError("DataParallelPPO.select_minibatch: no table yet: call set_minibatch_rows first")
        row = int(e) * self._job_chunks + int(j)
        if not (0 <= int(j) < self._job_chunks and 0 <= row < int(self._job_table.shape[0])):
            raise ValueError("DataParallelPPO.select_minibatch: (%d, %d) is outside the table's %d rows of %d chunks per epoch"
                             % (int(e), int(j), int(self._job_table.shape[0]), self._job_chunks))
        self._job_row = row

    def minibatch_table(self):
        """f32 [epochs * C, 4] on the device: the table set_minibatch_rows made last, row e * C + j = {mean, std + adv_eps, its
        inverse, 0} of the job's minibatch (e, j)."""
        self._need_job_mode("minibatch_table")
        return self._job_table

    def _apply_return_filter(self, return_filter, batch):
        if getattr(return_filter, "job", False):
            return return_filter.apply(batch, self.group)
        return return_filter.apply(batch)

    def gae(self, batch, gamma=0.99, lam=0.95, return_filter=None):
        """NativePPO.gae on the shard, then the job-wide advantage statistics: the shards' moments gathered and set.  return_filter: a
        job filter (``ReturnFilter(job=True)``) is handed this job's group; a plain one is refused with more than one rank."""
        check_return_filter(return_filter, self.world)
        out = super(DataParallelPPO, self).gae(batch, gamma, lam, return_filter)
        if int(batch["adv"].shape[0]) * sum(self.shard_envs) < 2:
            raise ValueError("DataParallelPPO.gae: the job has fewer than 2 samples: no unbiased std")
        self.set_moments(all_gather_rows(self.shard_moments(batch), self.group))
        return out

    # ------------------------------------------------------------------------------------------------
    # the two halves of a minibatch
    # ------------------------------------------------------------------------------------------------
    def local_row(self, batch, idx):
        """f32 [P + 8]: the gradient of the loss over THIS shard's samples idx (unclipped: the extended loss is taken with
        max_grad_norm = 0), then its stats row (the plain loss's four columns zero-padded)."""
        torch = _torch()
        n, p = self._samples(batch)
        idx = idx.to(device=self.policy.device, dtype=torch.int64).contiguous()
        M = idx.numel()
        self._ws(n, M)
        row = torch.zeros(self.n_params + N.PPO_EXT_STATS, dtype=torch.float32, device=self.policy.device)
        self._bind_adv_norm()
        name, ext = "ssg_ppo_grad", ()
        if self.extended():
            rec = self._ext(batch, n)
            rec.max_grad_norm = 0.0
            name, ext = "ssg_ppo_grad_ext", (C.byref(rec),)
        self.env.enqueue(name, C.byref(self.policy.to_native()), C.byref(self.hp), *ext, n, *p, idx.data_ptr(), M, row.data_ptr(),
                         row[self.n_params:].data_ptr(), *self._ws_ptr())
        return row

    def apply_rows(self, rows, counts, first_chunk, last_chunk, stats=False):
        """One minibatch's second half (ssg_ppo_apply_shards): combine the gathered rows (f32 [W, P + 8], shard order) with the weights
        counts[r] / sum(counts), clip, one Adam step; with last_chunk and kl_target > 0 the KL coefficient is adapted from the mean of
        the applies since the last first_chunk.  stats=True returns the job's stats row (f32 [4], or [8] with an extended term on)."""
        torch = _torch()
        rows = rows.to(device=self.policy.device, dtype=torch.float32).contiguous()
        W = len(counts)
        N.arg(rows, torch.float32, (W, self.n_params + N.PPO_EXT_STATS), "DataParallelPPO.apply_rows: rows", self._device)
        self._since_first = 1 if first_chunk else self._since_first + 1
        cnt = (C.c_int64 * W)(*[int(c) for c in counts])
        sh = N.PpoShards()
        sh.struct_size = C.sizeof(N.PpoShards)
        sh.n_shards, sh.dev_rows, sh.counts = W, rows.data_ptr(), cnt
        sh.first_chunk, sh.last_chunk, sh.n_chunks = int(bool(first_chunk)), int(bool(last_chunk)), self._since_first
        ext = None
        if self.extended():
            rec = N.PpoExt()
            rec.struct_size = C.sizeof(N.PpoExt)
            rec.vf_clip, rec.max_grad_norm, rec.kl_target = self.vf_clip, self.max_grad_norm, self.kl_target
            if self._kl_on:
                rec.dev_kl_coef = self.kl_coef.data_ptr()
            ext = C.byref(rec)
        self._ws(1, 1)
        st = torch.empty(N.PPO_EXT_STATS, dtype=torch.float32, device=self.policy.device) if stats else None
        self._bind_adv_norm()
        self.env.enqueue("ssg_ppo_apply_shards", C.byref(self.policy.to_native()), C.byref(self.hp), ext, C.byref(sh), self.adam_mv.data_ptr(),
                         self.step + 1, N.ptr(st), *self._ws_ptr())
        self.step += 1
        if not stats:
            return None
        return st if self.extended() else st[:4]

    def update(self, batch, perm, epochs, minibatches, stats=False):
        """NativePPO.update over the job: per minibatch the local row, the all-gather of the rows, the apply.  perm: this rank's own
        int64 [epochs, n] over ITS n samples (None: draw_perm's, keyed by the rank).  The shards' counts come from the gathered shard
        sizes: no per-minibatch exchange besides the rows."""
        torch = _torch()
        if perm is None and self.perm_seed is None:
            raise ValueError("DataParallelPPO.update: perm=None needs a perm_seed; else pass the permutations")
        n, _ = self._samples(batch)
        K = int(batch["adv"].shape[0])
        if n != K * self.shard_envs[self.rank]:
            raise ValueError("DataParallelPPO.update: the batch has %d samples, this rank's shard %d x %d" % (n, K, self.shard_envs[self.rank]))
        n_chunks, lens = self.check_chunks(K, minibatches)
        if perm is None:
            perm = self.draw_perm(n, epochs)
        perm = perm.to(device=self.policy.device, dtype=torch.int64).contiguous()
        if tuple(perm.shape) != (int(epochs), n):
            raise ValueError("DataParallelPPO.update: perm must be int64 [epochs, %d] (got %s)" % (n, tuple(perm.shape)))
        if self._kl_on and "logp_all" not in batch:
            self.dist(batch)  # (from the parameters on entry, as NativePPO.update takes it)
        chunk = lens[self.rank]
        self._ws(n, chunk)  # (grown once: the running KL sum lives in it across the minibatches)
        job_rows = self.job_adv_norm == "minibatch"
        if job_rows:  # every minibatch's sums in one pass, one gather, the same table on every rank
            self.set_minibatch_rows(all_gather_rows(self.shard_minibatch_sums(batch, perm, minibatches), self.group))
        out = []
        for e in range(int(epochs)):
            for j in range(n_chunks):
                if job_rows:
                    self.select_minibatch(e, j)
                row = self.local_row(batch, perm[e, j * chunk: min(n, (j + 1) * chunk)])
                rows = all_gather_rows(row, self.group)
                st = self.apply_rows(rows, chunk_counts(K, self.shard_envs, minibatches, j), j == 0,
                                     e == int(epochs) - 1 and j == n_chunks - 1, stats)
                if stats:
                    out.append(st)
        self.updates += 1
        return torch.stack(out) if stats else None

    def job_report(self, batch, stats=None, post=False, group=None, per_shard=False):
        """NativePPO.job_report over this job's group (group=None: ``self.group``): a collective, every rank calls it and gets the same
        bits.  stats: what update(..., stats=True) returned — the job's rows, identical on every rank."""
        return super(DataParallelPPO, self).job_report(batch, stats, post, self.group if group is None else group, per_shard)

    # ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """NativePPO's state plus ``world`` and ``rank``, which load_state_dict checks, and ``job_adv_norm`` (the mode is made at
        construction: it must be the state's; a state without the key is a "batch" one).  The table is not state: every update()
        makes its own before anything reads it."""
        sd = super(DataParallelPPO, self).state_dict()
        sd["world"], sd["rank"], sd["job_adv_norm"] = int(self.world), int(self.rank), self.job_adv_norm
        return sd

    def load_state_dict(self, sd):
        for k, mine in (("world", self.world), ("rank", self.rank)):
            if k not in sd or int(sd[k]) != int(mine):
                raise ValueError("DataParallelPPO.load_state_dict: %s: the state has %r, this object %r" % (k, sd.get(k, "nothing"), mine))
        if sd.get("job_adv_norm", "batch") != self.job_adv_norm:
            raise ValueError("DataParallelPPO.load_state_dict: job_adv_norm: the state has %r, this object %r"
                             % (sd.get("job_adv_norm", "batch"), self.job_adv_norm))
        return super(DataParallelPPO, self).load_state_dict(sd)
