"""Every finished training episode on record: EpisodeLog (ssg_episode_log_append), MonitorWriter and episode_log_reference.

The reference's Stable-Baselines script wraps its envs in ``Monitor`` and reads the per-episode rows back with ``load_results`` /
``ts2xy`` (train/stable_baselines/ppo.py:7-8,38-40): its callback plots return against timesteps and keeps the best model by
``np.mean(y[-100:])``.  ``EpisodeLog`` keeps those rows in a ring on the device: ``append(batch)`` is one library call on a rollout's
[K, N] reward / done / flags buffers, with no host synchronisation; an episode that spans rollouts is carried and recorded once, at
its end.  ``records()`` brings the ring to the host, in append order.  ``MonitorWriter`` writes Stable-Baselines' monitor file from it.
The order of the records, and everything else about a call, is defined in include/shipsim.h (section "Episode log").

``EpisodeLog(..., job=True, rows=K)`` is the log of one rank of a data-parallel job (ship_sim_gym_amd/dp.py): the ring is the JOB's, the
one a single ``EpisodeLog`` over the envs of all ranks would keep — what ``SubprocVecEnv`` + ``Monitor`` + ``load_results`` give the
reference over all its workers (train/stable_baselines/ppo.py:7-8,25-52,122-123).  A rank packs its shard's episodes of a rollout into
one fixed-size block (``shard_block``), the blocks are all-gathered once, and every rank merges them with the same integer arithmetic
(``merge_blocks``), so all ranks hold the same bits; ``job_append`` is the two around the gather.  The halves are public so that one
process can replay a W-rank job with ``torch.stack`` of the shards' blocks as the gather.  The carries stay this rank's envs'.

Out of scope: populations or member bits across ranks, evaluation episodes (``NativeEvaluator`` has its own accounting), a
variable-size gather (it needs a host synchronisation to size), per-episode wall-clock times, a TensorBoard writer.

``episode_log_reference`` is a numpy restatement of the library call, for tests; ``shard_block_reference`` and
``merge_blocks_reference`` restate the two halves of the job's call.
"""
import ctypes as C
import json
import os
import time
import warnings

import numpy as np

from . import _native as N
from ._native import _torch

RECORD_DTYPE = np.dtype([("ret", "<f8"), ("step", "<i8"), ("env", "<i4"), ("length", "<i4"), ("goals", "<i4"), ("end", "<u4")])
RECORD_BYTES = 32
assert RECORD_DTYPE.itemsize == RECORD_BYTES
MONITOR_COLUMNS = ("r", "l", "t", "timesteps", "env", "member", "goals", "end")
# the endings, under evaluate.py's names, and their SSG_EV_* bits
END_BITS = (("collided", N.EV_COLLIDING), ("out_of_bounds", N.EV_OUT_OF_BOUNDS), ("max_steps", N.EV_MAX_STEPS),
            ("no_goals_left", N.EV_NO_GOALS_LEFT))


def record_member(records):
    """The member that owned each record's env when its episode ended (bits 8..15 of ``end``)."""
    return ((np.asarray(records)["end"] >> 8) & 0xff).astype(np.int64)


def record_flags(records):
    """The flags byte of each record's done step (the low byte of ``end``)."""
    return (np.asarray(records)["end"] & 0xff).astype(np.int64)


def member_of_envs(n_envs, n_members=1, slices=None):
    """int64 [n_envs]: the member that owns each env — by the slice sizes when given, else by the equal split."""
    if slices is not None:
        sizes = [int(s) for s in slices]
        if sum(sizes) != int(n_envs) or min(sizes) < 1:
            raise ValueError("member_of_envs: the slices %s do not cover %d envs" % (sizes, n_envs))
        return np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    if int(n_envs) % int(n_members):
        raise ValueError("member_of_envs: %d envs do not split into %d equal member slices" % (n_envs, n_members))
    return np.arange(int(n_envs), dtype=np.int64) // (int(n_envs) // int(n_members))


def episode_log_reference(rew, done, flags, carry_ret, carry, head, ring, step0=0, env_base=0, members=None):
    """What ssg_episode_log_append leaves, in numpy.  rew f64 [K, N], done [K, N], flags u8 [K, N] or None; carry_ret f64 [N], carry
    int32 [N, 2] (length, goal events); head int64 [2]; ring a RECORD_DTYPE array [capacity]; members int [N] or None (all 0).
    Walks t = 0 .. K-1 and, within a row, the envs in ascending order — the order of np.nonzero(done) —, so the episode of rank r meets
    slot (head[0] + r) % capacity; a rank below count - capacity is not written.  Returns new (ring, head, carry_ret, carry)."""
    rew, done = np.asarray(rew, dtype=np.float64), np.asarray(done)
    if rew.ndim != 2 or done.shape != rew.shape or (flags is not None and np.asarray(flags).shape != rew.shape):
        raise ValueError("episode_log_reference: rew, done and flags must be [K, N] alike")
    K, n = rew.shape
    ring, head = np.array(ring, dtype=RECORD_DTYPE), np.array(head, dtype=np.int64).reshape(2)
    cret, c = np.array(carry_ret, dtype=np.float64).reshape(n), np.array(carry, dtype=np.int32).reshape(n, 2)
    cap = ring.shape[0]
    if cap < 1:
        raise ValueError("episode_log_reference: the ring has no slot")
    fl = np.zeros((K, n), dtype=np.uint8) if flags is None else np.asarray(flags).astype(np.uint8)
    mem = np.zeros(n, dtype=np.int64) if members is None else np.asarray(members, dtype=np.int64).reshape(n)
    count = int(np.count_nonzero(done))
    skip, r = max(0, count - cap), 0
    for t in range(K):
        cret = cret + rew[t]
        c[:, 0] += 1
        c[:, 1] += (fl[t] & N.EV_GOAL_REACHED) != 0
        for e in np.nonzero(done[t])[0]:
            if r >= skip:
                ring[(int(head[0]) + r) % cap] = (cret[e], int(step0) + t, int(env_base) + int(e), c[e, 0], c[e, 1],
                                                  int(fl[t, e]) | (int(mem[e]) << 8))
            r += 1
            cret[e] = 0.0
            c[e] = 0
    head[0] += count
    head[1] = count
    return ring, head, cret, c


# the shard block of a job's log (include/shipsim.h, "Job-wide episode log"): a 32-byte header, int32 lb[rows + 1] padded to 16 bytes,
# then `stage` record slots
BLOCK_HEADER_DTYPE = np.dtype([("count", "<i8"), ("step0", "<i8"), ("K", "<i4"), ("stage", "<i4"), ("reserved", "<i8")])
BLOCK_HEADER_BYTES = 32
assert BLOCK_HEADER_DTYPE.itemsize == BLOCK_HEADER_BYTES


def job_stage(capacity, rows, total_envs, world):
    """S, the record slots of a shard block: min(capacity, rows * ceil(total_envs / world)) — the same on every rank."""
    return min(int(capacity), int(rows) * ((int(total_envs) + int(world) - 1) // int(world)))


def block_layout(rows, stage):
    """(lb entries with the padding, offset of the records, bytes of the block) — what ssg_job_episode_log_block_nbytes answers."""
    rows, stage = int(rows), int(stage)
    if rows < 1 or stage < 1:
        raise ValueError("block_layout: rows and stage must be >= 1")
    lb_n = (rows + 1 + 3) // 4 * 4
    rec_off = BLOCK_HEADER_BYTES + 4 * lb_n
    return lb_n, rec_off, rec_off + RECORD_BYTES * stage


def block_views(block, rows, stage):
    """(header [1], lb int32 [padded rows + 1], slots RECORD_DTYPE [stage]): numpy views of one block (a uint8 array of its size)."""
    lb_n, rec_off, nbytes = block_layout(rows, stage)
    block = np.asarray(block)
    if block.dtype != np.uint8 or block.ndim != 1 or block.shape[0] != nbytes:
        raise ValueError("block_views: a block of rows = %d and stage = %d is uint8 [%d] (got %s %s)" % (rows, stage, nbytes, block.dtype, block.shape))
    return (block[:BLOCK_HEADER_BYTES].view(BLOCK_HEADER_DTYPE), block[BLOCK_HEADER_BYTES:rec_off].view("<i4"),
            block[rec_off:].view(RECORD_DTYPE))


def block_owned_slots(count, stage):
    """The slots of a block that the call's episodes own: local rank q lives in slot q % stage, for q in [max(0, count - stage), count)."""
    count, stage = int(count), int(stage)
    return np.sort(np.arange(max(0, count - stage), count, dtype=np.int64) % stage)


def shard_block_reference(rew, done, flags, carry_ret, carry, rows, stage, step0=0, env_base=0):
    """What ssg_job_episode_log_shard leaves, in numpy: episode_log_reference over a staging ring of `stage` slots with head 0, packed with
    the header and lb[t] = the episodes that end on the shard in rows before t (lb[K] = count; zero past K).  Slots that no episode of
    the call owns are zero here and unspecified on the device (block_owned_slots names the others).
    Returns (block uint8 [nbytes], carry_ret, carry)."""
    done = np.asarray(done)
    K = int(done.shape[0])
    if K < 1 or K > int(rows):
        raise ValueError("shard_block_reference: K = %d outside 1..rows = %d" % (K, int(rows)))
    lb_n, rec_off, nbytes = block_layout(rows, stage)
    ring, head, cret, c = episode_log_reference(rew, done, flags, carry_ret, carry, np.zeros(2, dtype=np.int64),
                                                np.zeros(int(stage), dtype=RECORD_DTYPE), step0=step0, env_base=env_base)
    block = np.zeros(nbytes, dtype=np.uint8)
    hdr, lb, slots = block_views(block, rows, stage)
    hdr[0] = (int(head[1]), int(step0), K, int(stage), 0)
    lb[1:K + 1] = np.cumsum(np.count_nonzero(done, axis=1))
    owned = block_owned_slots(int(head[1]), stage)
    slots[owned] = ring[owned]
    return block, cret, c


def merge_blocks_reference(blocks, ring, head, K, step0, rows, stage):
    """What ssg_job_episode_log_merge_blocks leaves, in numpy.  blocks uint8 [W, nbytes], the shards' blocks in rank order; ring a
    RECORD_DTYPE array [capacity]; head int64 [2].  For block r and slot i < min(count_r, stage): q = i, or the one q in
    [count_r - stage, count_r) congruent to i; t = step - step0; the job's rank
        R = (q - lb_r[t]) + sum_{r' < r} lb_r'[t + 1] + sum_{r' >= r} lb_r'[t]
    and total = sum_r lb_r[K] (not below 0).  The record goes to slot (head[0] + R) % capacity unless t is outside [0, K), R outside
    [0, total) or R < total - capacity.  Then head[0] += total, head[1] = total.  Returns new (ring, head)."""
    blocks = np.asarray(blocks)
    K, step0, rows, stage = int(K), int(step0), int(rows), int(stage)
    if blocks.ndim != 2 or blocks.shape[0] < 1 or K < 1 or K > rows:
        raise ValueError("merge_blocks_reference: blocks must be uint8 [W >= 1, nbytes] and K in 1..rows")
    ring, head = np.array(ring, dtype=RECORD_DTYPE), np.array(head, dtype=np.int64).reshape(2)
    cap = int(ring.shape[0])
    views = [block_views(b, rows, stage) for b in blocks]
    lbs = np.stack([v[1].astype(np.int64) for v in views])  # [W, padded rows + 1]
    total = max(0, int(lbs[:, K].sum()))
    head0 = int(head[0])
    for r, (hdr, _, slots) in enumerate(views):
        cnt = max(0, int(hdr["count"][0]))
        for i in range(min(cnt, stage)):
            q = i
            if cnt > stage:
                base = cnt - stage
                q = base + (i - base % stage) % stage
            rec = slots[i]
            t = int(rec["step"]) - step0
            if t < 0 or t >= K:
                continue
            R = (q - int(lbs[r, t])) + int(lbs[:r, t + 1].sum()) + int(lbs[r:, t].sum())
            if R < 0 or R >= total or R < total - cap:
                continue
            ring[(head0 % cap + R) % cap] = rec
    head[0] = head0 + total
    head[1] = total
    return ring, head


class EpisodeLog(object):
    """The episode log of `env` (a ShipVecEnv): owns the ring of `capacity` records with its head, the per-env carries (return f64
    [N]; length and goal events int32 [N, 2]) and the workspace, all on the env's device, and counts the steps it has seen (``steps``:
    step0 of the next call, part of its state).  n_members: 1 for a single policy, P for a population — a record then names the member
    that owned the env when the episode ended (the equal split, or the slices bound to the env).

    Nothing is bound to the env: call ``append(batch)`` after every rollout.  Call ``reset_carry()`` after resetting the envs by hand.

    job=True (one member only), rows=K: the log of one rank of a data-parallel job (include/shipsim.h, "Job-wide episode log").  The ring
    and the head are the JOB's, the same bits on every rank; the carries stay this rank's envs'.  rows is the largest K of one call
    (the rollout length).  The job's size and its total env count come from the process group (`group`; None: the default one; with
    none initialised the job is this process, W = 1), over which the ranks' env counts are gathered once — or from `world` and
    `total_envs`, given together, when one process replays a W-rank job.  Call ``job_append(batch)`` after every rollout."""

    def __init__(self, env, capacity=65536, n_members=1, job=False, rows=None, world=None, total_envs=None, group=None):
        torch = _torch()
        cap, P = int(capacity), int(n_members)
        if cap < 1:
            raise ValueError("EpisodeLog: capacity must be >= 1")
        if P < 1 or P > N.POP_MAX_MEMBERS:
            raise ValueError("EpisodeLog: n_members must be in 1..%d" % N.POP_MAX_MEMBERS)
        self.env, self.capacity, self.n_members = env, cap, P
        dev, n = env.device, int(env.num_envs)
        self.job, self.group = bool(job), group
        self.rows = self.world = self.total_envs = self.stage = self.block_nbytes = None
        self._pending = None    # (K, step0) of a shard_block whose merge_blocks is still to come
        if not self.job and not (rows is None and world is None and total_envs is None and group is None):
            raise ValueError("EpisodeLog: rows, world, total_envs and group belong to a job log (job=True)")
        if self.job:
            if P != 1:
                raise ValueError("EpisodeLog: a job log has one member (populations across ranks are out of scope; got n_members=%d)" % P)
            if rows is None or int(rows) < 1:
                raise ValueError("EpisodeLog: a job log needs rows >= 1, the largest K of one call (got %r)" % (rows,))
            if (world is None) != (total_envs is None):
                raise ValueError("EpisodeLog: world and total_envs go together (both, or neither: then the process group tells)")
            if world is None:
                from .sharding import all_gather_rows
                sizes = all_gather_rows(torch.tensor([n], dtype=torch.int64, device=dev), group).reshape(-1).cpu().tolist()
                world, total_envs = len(sizes), sum(int(v) for v in sizes)
            self.rows, self.world, self.total_envs = int(rows), int(world), int(total_envs)
            if not 1 <= self.world <= N.DP_MAX_SHARDS:
                raise ValueError("EpisodeLog: %d ranks, ssg_job_episode_log_merge_blocks merges at most %d blocks" % (self.world, N.DP_MAX_SHARDS))
            if self.total_envs < self.world or n > (self.total_envs + self.world - 1) // self.world:
                raise ValueError("EpisodeLog: a shard of %d envs is not one of %d envs over %d ranks" % (n, self.total_envs, self.world))
            if self.rows * ((n + 255) // 256) > N.EPISODE_LOG_MAX_CELLS:
                raise ValueError("EpisodeLog: rows * ceil(n_envs / 256) = %d above SSG_EPISODE_LOG_MAX_CELLS = %d"
                                 % (self.rows * ((n + 255) // 256), N.EPISODE_LOG_MAX_CELLS))
            self.stage = job_stage(cap, self.rows, self.total_envs, self.world)
            if self.stage > 2 ** 31 - 1:
                raise ValueError("EpisodeLog: a shard block of %d record slots is more than a call takes" % self.stage)
            self.block_nbytes = N.nbytes("ssg_job_episode_log_block_nbytes", self.rows, self.stage)
        # one buffer, one copy to the host: the head (int64 [2], padded to a record) and then the ring
        self.buffer = torch.zeros((cap + 1) * RECORD_BYTES, dtype=torch.uint8, device=dev)
        self.head = self.buffer[:16].view(torch.int64)
        self.ring = self.buffer[RECORD_BYTES:]
        self.carry_return = torch.zeros(n, dtype=torch.float64, device=dev)
        self.carry = torch.zeros((n, 2), dtype=torch.int32, device=dev)
        self.workspace = torch.zeros(0, dtype=torch.uint8, device=dev)
        self.steps = 0          # rows appended so far
        self.rows_written = 0   # rows a MonitorWriter has written to its file
        self.flushed = 0        # episodes a MonitorWriter has passed (written or found dropped)
        self._writers = []
        self._host_copy = None  # the last copy of the buffer to the host; dropped by whatever changes the ring

    def reset_carry(self):
        """Forget the running episodes (call after an env reset)."""
        self.carry_return.zero_()
        self.carry.zero_()
        return self

    def _ws(self, K):
        need = N.nbytes("ssg_episode_log_workspace_nbytes", int(self.env.num_envs), int(K))
        if self.workspace.numel() < need:
            self.workspace = _torch().zeros(need, dtype=_torch().uint8, device=self.buffer.device)
        return self.workspace

    def to_native(self, K=1):
        """The ssg_episode_log record for calls of up to K rows (the workspace is grown to serve them)."""
        ws = self._ws(K)
        rec = N.EpisodeLogRecord()
        rec.struct_size = C.sizeof(N.EpisodeLogRecord)
        rec.n_members, rec.capacity = self.n_members, self.capacity
        rec.dev_records, rec.dev_head = self.ring.data_ptr(), self.head.data_ptr()
        rec.dev_carry_return, rec.dev_carry = self.carry_return.data_ptr(), self.carry.data_ptr()
        rec.dev_workspace, rec.workspace_nbytes = ws.data_ptr(), ws.numel()
        return rec

    def _check_rows(self, rew, done, flags):
        """(K, row pitch) of a call's [K, N] buffers."""
        torch = _torch()
        env = self.env
        n_env = int(env.num_envs)
        for name, t, dt in (("rew", rew, torch.float64), ("done", done, torch.uint8), ("flags", flags, torch.uint8)):
            if t is None and name == "flags":
                continue
            if t.dtype != dt or t.device != env.device or t.dim() != 2 or int(t.shape[1]) != n_env or int(t.shape[0]) < 1 or \
                    t.stride(1) != 1 or t.stride(0) < n_env:
                raise ValueError("EpisodeLog: %s must be a %s tensor [K, %d] on %s with unit-stride rows (got %s %s, strides %s, on %s)"
                                 % (name, dt, n_env, env.device, t.dtype, tuple(t.shape), tuple(t.stride()), t.device))
        K, pitch = int(rew.shape[0]), int(rew.stride(0))
        if any(int(t.shape[0]) != K or int(t.stride(0)) != pitch for t in (done, flags) if t is not None):
            raise ValueError("EpisodeLog: rew, done and flags must have the same number of rows and the same row pitch")
        return K, pitch

    def append_rows(self, rew, done, flags=None):
        """ssg_episode_log_append on a rollout's buffers: rew f64 / done u8 / flags u8 (or None) [K, N] in the env's row layout, rows of
        unit stride and a common row pitch >= N.  Row t is step ``steps + t``; ``steps`` advances by K.  Blocks beyond the library's
        cap on K * tiles are served in several calls, which leave what one call would.  No host synchronisation."""
        env = self.env
        n_env = int(env.num_envs)
        if self.job:
            raise ValueError("EpisodeLog.append: a job log's ring holds the episodes of all ranks: call job_append (or shard_block and "
                             "merge_blocks)")
        K, pitch = self._check_rows(rew, done, flags)
        per_call = max(1, N.EPISODE_LOG_MAX_CELLS // ((n_env + 255) // 256))
        rec = self.to_native(min(K, per_call))
        for k0 in range(0, K, per_call):
            env.enqueue("ssg_episode_log_append", C.byref(rec), min(K, k0 + per_call) - k0, self.steps + k0, rew[k0].data_ptr(),
                        done[k0].data_ptr(), flags[k0].data_ptr() if flags is not None else None, pitch)
        self.steps += K
        self._host_copy = None
        return self

    def append(self, batch):
        """Record the episodes that ended in a rollout batch (``rollout_policy`` / ``rollout_population``: "rew", "done", "flags")."""
        return self.append_rows(batch["rew"], batch["done"], batch.get("flags"))

    # ------------------------------------------------------------------------------------------------
    # the job's log: the two halves of a call, and the two around the gather
    # ------------------------------------------------------------------------------------------------
    def _job_only(self, who):
        if not self.job:
            raise ValueError("EpisodeLog.%s: this log was not made with job=True (its ring is this handle's: use append)" % who)

    def shard_block(self, batch, out=None):
        """The first half of ``job_append`` (ssg_job_episode_log_shard): walk batch["rew"] / batch["done"] / batch.get("flags") — at most
        `rows` rows — with this rank's carries and pack the shard's episodes into one block.  Returns the block, a uint8 tensor
        [block_nbytes] on the device (`out` when given: contiguous, 16-byte aligned; what it held does not enter the result); the
        ring and the head are not touched.  ``merge_blocks`` must follow before the next one."""
        torch = _torch()
        self._job_only("shard_block")
        if self._pending is not None:
            raise ValueError("EpisodeLog.shard_block: the previous block has not been merged (merge_blocks)")
        env = self.env
        rew, done, flags = batch["rew"], batch["done"], batch.get("flags")
        K, pitch = self._check_rows(rew, done, flags)
        if K > self.rows:
            raise ValueError("EpisodeLog.shard_block: %d rows, this log's calls take %d at most (job_append cuts a batch into pieces)" % (K, self.rows))
        block = torch.empty(self.block_nbytes, dtype=torch.uint8, device=env.device) if out is None else out
        bp = N.arg(block, torch.uint8, (self.block_nbytes,), "EpisodeLog.shard_block: out", self.buffer.device)
        env.enqueue("ssg_job_episode_log_shard", C.byref(self.to_native(K)), K, self.steps, rew.data_ptr(), done.data_ptr(), N.ptr(flags), pitch,
                    self.rows, self.stage, bp, block.numel())
        self._pending = (K, self.steps)
        return block

    def merge_blocks(self, stacked, K=None, step0=None):
        """The second half (ssg_job_episode_log_merge_blocks): stacked uint8 [W, block_nbytes] on the log's device, the ranks'
        ``shard_block`` of this call in rank order.  Every record goes to the slot its job rank decides; the head advances by the
        call's total, and ``steps`` by its rows.  K and step0, given together, merge blocks this log made no ``shard_block`` for
        (blocks made elsewhere: ``steps`` becomes step0 + K)."""
        torch = _torch()
        self._job_only("merge_blocks")
        if (K is None) != (step0 is None):
            raise ValueError("EpisodeLog.merge_blocks: K and step0 go together")
        if K is not None and self._pending is not None:
            raise ValueError("EpisodeLog.merge_blocks: a shard_block is waiting for its merge: call it without K and step0")
        if K is not None and not 1 <= int(K) <= self.rows:
            raise ValueError("EpisodeLog.merge_blocks: K = %d outside 1..rows = %d" % (int(K), self.rows))
        if K is None and self._pending is None:
            raise ValueError("EpisodeLog.merge_blocks: no shard_block is waiting for its merge")
        if (stacked.dtype != torch.uint8 or stacked.device != self.buffer.device or stacked.dim() != 2
                or tuple(stacked.shape) != (self.world, self.block_nbytes)):
            raise ValueError("EpisodeLog.merge_blocks: the blocks must be a uint8 tensor (%d, %d) on %s (got %s %s on %s)"
                             % (self.world, self.block_nbytes, self.buffer.device, stacked.dtype, tuple(stacked.shape), stacked.device))
        stacked = stacked.contiguous()
        K, step0 = self._pending if K is None else (int(K), int(step0))
        self.env.enqueue("ssg_job_episode_log_merge_blocks", C.byref(self.to_native(1)), K, step0, self.rows, self.stage, stacked.data_ptr(),
                         self.world)
        self._pending = None
        self.steps = step0 + K
        self._host_copy = None
        return self

    def job_append(self, batch, group=None):
        """Record the episodes of ALL ranks that ended in this rollout (a collective: every rank calls it with its own batch of the
        same rows): ``shard_block``, one all-gather of the blocks over `group` (None: the log's own), then ``merge_blocks``.  A batch
        of more than `rows` rows goes in pieces of `rows`, which leave what one call would.  No host synchronisation of its own."""
        from .sharding import all_gather_rows
        self._job_only("job_append")
        K = int(batch["rew"].shape[0])
        for k0 in range(0, K, self.rows):
            piece = {k: batch[k][k0:k0 + self.rows] for k in ("rew", "done", "flags") if batch.get(k) is not None}
            self.merge_blocks(all_gather_rows(self.shard_block(piece), self.group if group is None else group))
        return self

    # ------------------------------------------------------------------------------------------------
    # reading (the first read after an append copies the buffer to the host: one device-to-host copy, which waits for the appends before it)
    # ------------------------------------------------------------------------------------------------
    def _host(self):
        if self._host_copy is None:  # (several reads between two appends share one copy)
            raw = self.buffer.cpu().numpy()
            self._host_copy = (raw[:16].view(np.int64).copy(), raw[RECORD_BYTES:].view(RECORD_DTYPE))
        return self._host_copy

    def total(self):
        """Episodes ever appended."""
        return int(self._host()[0][0])

    def records(self, since=None):
        """(records, dropped): the retained records from episode number `since` on (None: all that are retained), a RECORD_DTYPE array
        in append order, and how many episodes between `since` and the oldest retained one were overwritten before they were read."""
        head, ring = self._host()
        total = int(head[0])
        oldest = max(0, total - self.capacity)
        since = oldest if since is None else int(since)
        if since < 0 or since > total:
            raise ValueError("EpisodeLog.records: since = %d outside 0..%d, the episodes appended so far" % (since, total))
        first = max(since, oldest)
        idx = np.arange(first, total, dtype=np.int64) % self.capacity
        return ring[idx].copy(), first - since

    def timesteps(self, records):
        """The x axis of ts2xy(..., 'timesteps'): the env steps the whole batch of envs — a job log: the envs of all ranks — had taken
        when each episode ended."""
        return (np.asarray(records)["step"] + 1) * int(self.total_envs if self.job else self.env.num_envs)

    def mean_last(self, W, member=None):
        """np.mean of the returns of the last min(W, available) retained records (of `member` alone when given); None when there are
        none.  The reference callback's np.mean(y[-100:])."""
        rec, _ = self.records()
        if member is not None:
            rec = rec[record_member(rec) == int(member)]
        if int(W) < 1 or rec.shape[0] == 0:
            return None
        return float(np.mean(rec["ret"][-int(W):]))

    @staticmethod
    def end_counts(records):
        """How the episodes ended, from the SSG_EV_* bits of their done steps (not exclusive of each other), with the episode count."""
        f = record_flags(records)
        out = {"episodes": int(f.shape[0])}
        out.update({name: int(np.count_nonzero(f & bit)) for name, bit in END_BITS})
        return out

    # ------------------------------------------------------------------------------------------------
    # state (ship_sim_gym_amd/checkpoint.py)
    # ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """Plain data: the ring and its head, the carries, the step count, and what a MonitorWriter has written and passed."""
        if self._pending is not None:
            raise ValueError("EpisodeLog.state_dict: a shard_block is waiting for its merge_blocks")
        sd = {"capacity": self.capacity, "n_members": self.n_members, "num_envs": int(self.env.num_envs),
              "ring": self.ring.detach().cpu().clone(), "head": self.head.detach().cpu().clone(),
              "carry_return": self.carry_return.detach().cpu().clone(), "carry": self.carry.detach().cpu().clone(),
              "steps": int(self.steps), "rows_written": int(self.rows_written), "flushed": int(self.flushed)}
        sd.update(self._job_fields())  # (a job log: the ring is the job's, the carries this rank's)
        return sd

    def _job_fields(self):
        if not self.job:
            return {}
        return {"job_world": self.world, "job_total_envs": self.total_envs, "job_rows": self.rows, "job_env_base": int(self.env.env_id_base)}

    def load_state_dict(self, sd):
        """Become the log the state was taken from.  Checked first, all of it: capacity, member count and env count, every tensor's
        shape and dtype, the counters, and that every attached MonitorWriter's file holds the state's rows; a mismatch raises ValueError
        naming the field and leaves this object, and the files, as they were.  Then the files are cut back to the state's rows."""
        from .checkpoint import check_state, check_values
        who = "EpisodeLog.load_state_dict"
        if isinstance(sd, dict) and not self.job and any(k.startswith("job_") for k in sd):
            raise ValueError("%s: the state is a job log's (job_world = %r), this log is one handle's" % (who, sd.get("job_world")))
        if self._pending is not None:
            raise ValueError("%s: a shard_block is waiting for its merge_blocks" % who)
        check_state(who, sd, fields=(("capacity", self.capacity), ("n_members", self.n_members), ("num_envs", int(self.env.num_envs)))
                    + tuple(self._job_fields().items()),
                    tensors=(("ring", self.ring), ("head", self.head), ("carry_return", self.carry_return), ("carry", self.carry)))
        check_values(who, sd, (("steps", int), ("rows_written", int), ("flushed", int)))
        if sd["steps"] < 0 or sd["rows_written"] < 0 or sd["flushed"] < sd["rows_written"] or sd["flushed"] > int(sd["head"][0]):
            raise ValueError("%s: steps %d, rows_written %d and flushed %d do not fit each other or head %d"
                             % (who, sd["steps"], sd["rows_written"], sd["flushed"], int(sd["head"][0])))
        for w in self._writers:
            w.check_rows(sd["rows_written"])
        self.ring.copy_(sd["ring"])
        self.head.copy_(sd["head"])
        self.carry_return.copy_(sd["carry_return"])
        self.carry.copy_(sd["carry"])
        self.steps, self.rows_written, self.flushed = int(sd["steps"]), int(sd["rows_written"]), int(sd["flushed"])
        self._host_copy = None
        for w in self._writers:
            w.cut_back(self.rows_written)
        return self


class MonitorWriter(object):
    """Stable-Baselines' monitor file of an EpisodeLog: ``#`` and a JSON header (t_start, env_id), the column row
    ``r,l,t,timesteps,env,member,goals,end``, then one row per episode — the first three columns are what ``load_results`` reads.
    ``t`` is the host's seconds since t_start at the flush that wrote the row: the only column that is not reproducible.

    resume=False starts the file anew.  resume=True leaves it: ``log.load_state_dict`` then cuts it back to the header and the state's
    rows, so that a run that is saved, killed and resumed leaves the uninterrupted run's file in every column but ``t``."""

    def __init__(self, path, log, env_id="ShipSim", resume=False):
        self.path, self.log, self.warned = os.fspath(path), log, False
        self.t_start = time.time()
        if resume:
            self.t_start = self._read()[0]
        else:
            with open(self.path, "w") as f:
                f.write("#%s\n%s\n" % (json.dumps({"t_start": self.t_start, "env_id": str(env_id)}), ",".join(MONITOR_COLUMNS)))
        log._writers.append(self)

    def _read(self):
        """(t_start, the lines of the file); ValueError unless it starts with this format's two header lines."""
        try:
            with open(self.path) as f:
                lines = f.read().splitlines(True)
            if len(lines) < 2 or not lines[0].startswith("#") or lines[1].strip() != ",".join(MONITOR_COLUMNS):
                raise ValueError("no monitor header")
            return float(json.loads(lines[0][1:])["t_start"]), lines
        except (OSError, ValueError, KeyError, TypeError) as ex:
            raise ValueError("MonitorWriter: %s is not a monitor file of this format (%s)" % (self.path, ex))

    def check_rows(self, rows_written):
        have = len(self._read()[1]) - 2
        if have < int(rows_written):
            raise ValueError("MonitorWriter: rows_written is %d in the state, but %s holds %d rows" % (rows_written, self.path, have))

    def cut_back(self, rows_written):
        """Keep the header and the first rows_written rows."""
        self.t_start, lines = self._read()
        with open(self.path + ".tmp", "w") as f:
            f.writelines(lines[:2 + int(rows_written)])
        os.replace(self.path + ".tmp", self.path)

    def flush(self):
        """Append the records since the last flush; returns how many rows were written.  Warns once, with the count, when records were
        overwritten in the ring before a flush read them (a larger capacity, or a flush more often, keeps them)."""
        log = self.log
        rec, dropped = log.records(since=log.flushed)
        if dropped and not self.warned:
            self.warned = True
            warnings.warn("MonitorWriter: %d episodes were overwritten in the ring (capacity %d) before they were written to %s"
                          % (dropped, log.capacity, self.path), RuntimeWarning, stacklevel=2)
        t = round(time.time() - self.t_start, 6)
        ts, mem, fl = log.timesteps(rec), record_member(rec), record_flags(rec)
        with open(self.path, "a") as f:
            f.write("".join("%r,%d,%r,%d,%d,%d,%d,%d\n" % (float(r["ret"]), r["length"], t, ts[i], r["env"], mem[i], r["goals"], fl[i])
                            for i, r in enumerate(rec)))
        log.flushed += dropped + rec.shape[0]
        log.rows_written += rec.shape[0]
        return int(rec.shape[0])


def read_monitor(path):
    """A monitor file as ({header}, {column: numpy array}): what ``load_results`` would make of it, with the extra columns."""
    with open(os.fspath(path)) as f:
        first, names = f.readline(), f.readline().strip().split(",")
        rows = [line.strip().split(",") for line in f if line.strip()]
    if not first.startswith("#"):
        raise ValueError("read_monitor: %s does not start with a '#' header line" % path)
    cols = {}
    for i, name in enumerate(names):
        cols[name] = np.array([float(r[i]) if name in ("r", "t") else int(r[i]) for r in rows], dtype=np.float64 if name in ("r", "t") else np.int64)
    return json.loads(first[1:]), cols
