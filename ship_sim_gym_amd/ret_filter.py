"""Return normalisation kept and applied on the device: ReturnFilter (ssg_ret_filter_apply) and ret_filter_reference.

Stable-Baselines users wrap the vectorised env of train/stable_baselines/ppo.py:123 in ``VecNormalize``, which by default also
normalises the rewards: it keeps a discounted return per env, updates a running variance with every step's returns and divides the
step's rewards by the running standard deviation (clipped).  For this env — -0.01 per step, +-1 at an event — that brings the value
targets of a 1 000-step episode and of a 20-step one to the same order of magnitude.  ``ReturnFilter`` is that on the device, per member
of a population when there are several, for a whole rollout's [K, N] reward buffer in one library call between the rollout and GAE:
``apply(batch)`` leaves ``batch["rew"]`` alone (episode statistics and evaluation read it) and writes ``batch["rew_norm"]``, which
``NativePPO.gae(batch, ..., return_filter=f)`` / ``PopulationPPO.gae(batch, return_filter=f)`` hand to GAE.  The arithmetic is defined
in include/shipsim.h (section "Return filter") on its own terms; no bit parity with Stable-Baselines is claimed (it uses the
population variance and sqrt(var + eps)).

``ReturnFilter(..., job=True)`` is the filter of one rank of a data-parallel job (ship_sim_gym_amd/dp.py): the statistics are the
job's, those of one ``VecNormalize`` around the envs of all ranks, step by step.  A rank reduces its shard to one (mean, M2, count) row
per step (``shard_rows``), the ranks gather the rows once per rollout, and every rank chains the same rows in the same order
(``apply_rows``), so the states agree bit for bit without a broadcast; with one rank the result is the plain filter's bit for bit
(include/shipsim.h, "Job-wide return filter").

Not covered: the torch-mode trainers, populations across ranks, a frozen job call (a frozen filter needs no rows: ``apply`` serves it).

``ret_filter_reference`` is a numpy restatement of the device's arithmetic, the same walk and reduction order operation for operation,
for tests; ``batch_rows_reference`` and ``job_reference`` restate the two halves of the job-wide call.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import _torch
from .obs_filter import _merge, merge_reference


def _denom(state_rows):
    d = float(np.asarray(state_rows, dtype=np.float64).reshape(N.FILTER_ROWS)[2])
    return 1.0 if d == 0.0 else d


def ret_filter_reference(state_rows, carry, rew, done, gamma, clip=10.0, eps=1e-8, update=True):
    """What ssg_ret_filter_apply leaves for ONE member: state_rows f64 [4] (mean, M2, denom, count; zeros = empty), carry f64 [n], rew
    f64 [K, n] and done [K, n] (the member's columns), gamma a float.  For every k: c = c * gamma + rew[k]; the n values of c are
    merged into the state in the device's order (``obs_filter.merge_reference`` at D = 1); c = 0 where done[k]; out[k] =
    clamp(rew[k] / denom_k, +-clip) with denom_k the merged state's (a denom of 0 divides by 1; clip == 0: no clamp).  update=False
    (frozen): state and carry stay, every row is divided by the state's own denom.  Returns (state [4], carry [n], out [K, n], denoms
    [K]); the square root in a denom is numpy's (the device's may differ in the last bit)."""
    st = np.array(state_rows, dtype=np.float64).reshape(N.FILTER_ROWS, 1)
    c = np.array(carry, dtype=np.float64).reshape(-1)
    rew = np.asarray(rew, dtype=np.float64)
    done = np.asarray(done)
    if rew.ndim != 2 or rew.shape[1] != c.shape[0] or done.shape != rew.shape or rew.shape[1] < 1:
        raise ValueError("ret_filter_reference: rew and done must be [K, n] and carry [n >= 1]")
    g, clip = np.float64(gamma), float(clip)
    K = rew.shape[0]
    out, denoms = np.empty_like(rew), np.empty(K)
    for k in range(K):
        if update:
            prod = c * g
            c = prod + rew[k]
            st = merge_reference(st, c[:, None], eps=eps)
            c = np.where(done[k] != 0, 0.0, c)
        denoms[k] = _denom(st[:, 0])
        out[k] = rew[k] / denoms[k]
    if clip > 0.0:
        out = np.clip(out, -clip, clip)
    return st[:, 0].copy(), c, out, denoms


def batch_rows_reference(carry, rew, done, gamma):
    """What ssg_ret_filter_batches leaves for one rank: carry f64 [n], rew f64 [K, n], done [K, n], gamma a float.  The walk of
    ``ret_filter_reference``; step k's n samples are reduced in the device's order (``obs_filter.merge_reference`` into an empty state
    at D = 1) to the row {mean, M2, 0.0, n}.  Returns (rows f64 [K, 4], carry [n])."""
    c = np.array(carry, dtype=np.float64).reshape(-1)
    rew = np.asarray(rew, dtype=np.float64)
    done = np.asarray(done)
    if rew.ndim != 2 or rew.shape[1] != c.shape[0] or done.shape != rew.shape or rew.shape[1] < 1:
        raise ValueError("batch_rows_reference: rew and done must be [K, n] and carry [n >= 1]")
    g = np.float64(gamma)
    rows = np.zeros((rew.shape[0], N.FILTER_ROWS))
    empty = np.zeros((N.FILTER_ROWS, 1))
    for k in range(rew.shape[0]):
        prod = c * g
        c = prod + rew[k]
        st = merge_reference(empty, c[:, None], eps=0.0)
        rows[k] = st[0, 0], st[1, 0], 0.0, st[3, 0]
        c = np.where(done[k] != 0, 0.0, c)
    return rows, c


def job_reference(state_rows, rows, eps=1e-8):
    """What ssg_ret_filter_apply_rows leaves in the state, and its denoms: state_rows f64 [4] (mean, M2, denom, count), rows f64
    [W, K, 4] (the ranks' rows of ``batch_rows_reference`` in rank order).  For every k: step_k = rows[0][k] merged with rows[1][k],
    ..., rows[W - 1][k] in the header's association, a row of count 0 skipped; state_k = state_{k-1} merged with step_k; denom_k from
    state_k, a denom of 0 dividing by 1.  Returns (state [4], denoms [K]); the square roots are numpy's (the device's may differ in
    the last bit)."""
    st = np.array(state_rows, dtype=np.float64).reshape(N.FILTER_ROWS)
    rows = np.array(rows, dtype=np.float64)
    if rows.ndim != 3 or rows.shape[0] < 1 or rows.shape[1] < 1 or rows.shape[2] != N.FILTER_ROWS:
        raise ValueError("job_reference: rows must be [W >= 1, K >= 1, 4]")
    eps = np.float64(eps)
    s = (np.float64(st[3]), np.float64(st[0]), np.float64(st[1]))
    denoms = np.empty(rows.shape[1])
    den = st[2]
    for k in range(rows.shape[1]):
        a = (np.float64(rows[0, k, 3]), np.float64(rows[0, k, 0]), np.float64(rows[0, k, 1]))
        for r in rows[1:, k]:
            a = _merge(a, (np.float64(r[3]), np.float64(r[0]), np.float64(r[1])))
        s = _merge(s, a)
        den = np.sqrt(s[2] / (s[0] - 1.0)) + eps if s[0] >= 2.0 else np.float64(1.0)
        denoms[k] = 1.0 if den == 0.0 else den
    return np.array([s[1], s[2], den, s[0]], dtype=np.float64), denoms


class ReturnFilter(object):
    """The return filter of `env` (a ShipVecEnv): owns the state tensor f64 [n_members, 4] (mean, M2, denom, count per member; zeros =
    empty, which divides by 1), the per-env carry f64 [N] (the discounted return in flight), the members' discounts on the device and
    the workspace (regrown when a longer rollout arrives).  n_members: 1 for a single policy, P for a population (member m's
    statistics come from its own env slice).  gamma: a float, or a list of P (``PopulationPPO.gamma``); each in [0, 1].  clip: |r| is
    clamped to it (0: no clamp); eps: added to the standard deviation.  update: whether ``apply`` walks the returns and merges them
    (``train(flag)`` changes it later; ``VecNormalize.training``).

    Nothing is bound to the env: call ``apply(batch)`` on a rollout's batch, or hand the filter to ``gae`` of NativePPO /
    PopulationPPO.  Call ``reset_carry()`` after resetting the envs by hand.

    job=True (one member only): the filter of one rank of a data-parallel job (include/shipsim.h, "Job-wide return filter").  The state
    is the job's; the carry stays this rank's envs'.  ``apply(batch, group)`` is ``shard_rows`` (the walk and this shard's row per
    step), one all-gather of the rows, then ``apply_rows`` (the chain over the gathered rows and the division); the two halves are
    public so that one process can replay a W-rank job with ``torch.stack`` of the shards' rows as the gather."""

    def __init__(self, env, n_members=1, gamma=0.99, clip=10.0, eps=1e-8, update=True, job=False):
        torch = _torch()
        P = int(n_members)
        clip, eps = float(clip), float(eps)
        if P < 1 or P > N.POP_MAX_MEMBERS:
            raise ValueError("ReturnFilter: n_members must be in 1..%d" % N.POP_MAX_MEMBERS)
        if not clip >= 0.0 or not eps >= 0.0:
            raise ValueError("ReturnFilter: clip and eps must be >= 0")
        if job and P != 1:
            raise ValueError("ReturnFilter: a job filter has one member (populations across ranks are out of scope; got n_members=%d)" % P)
        self.job = bool(job)
        self.env, self.n_members, self.clip, self.eps, self.updating = env, P, clip, eps, bool(update)
        dev = env.device
        self.state = torch.zeros((P, N.FILTER_ROWS), dtype=torch.float64, device=dev)
        self.carry = torch.zeros(int(env.num_envs), dtype=torch.float64, device=dev)
        self.workspace = torch.zeros(0, dtype=torch.uint8, device=dev)
        self.gamma, self.gamma_dev = None, None
        self.set_gamma(gamma)

    # the state's columns (views of the state tensor; `var` is computed)
    @property
    def mean(self):
        return self.state[:, 0]

    @property
    def M2(self):
        return self.state[:, 1]

    @property
    def denom(self):
        return self.state[:, 2]

    @property
    def count(self):
        return self.state[:, 3]

    @property
    def var(self):
        """The sample variance M2 / (count - 1) of the discounted returns, f64 [n_members]; 1 where count < 2."""
        torch = _torch()
        return torch.where(self.count >= 2.0, self.M2 / (self.count - 1.0).clamp(min=1.0), torch.ones_like(self.M2))

    def set_gamma(self, gamma):
        """The members' discounts: a float for all, or a list of P.  Uploaded only when they changed."""
        torch = _torch()
        g = [float(x) for x in gamma] if isinstance(gamma, (list, tuple)) else [float(gamma)] * self.n_members
        if len(g) != self.n_members:
            raise ValueError("ReturnFilter: gamma has %d entries for %d members" % (len(g), self.n_members))
        if not all(0.0 <= x <= 1.0 for x in g):
            raise ValueError("ReturnFilter: every gamma must be in [0, 1] (got %s)" % (g,))
        if g != self.gamma:
            self.gamma = g
            self.gamma_dev = torch.tensor(g, dtype=torch.float64).to(self.state.device)
        return self

    def train(self, flag=True):
        """Whether ``apply`` updates the statistics and the carry (``VecNormalize.training``)."""
        self.updating = bool(flag)
        return self

    def reset_carry(self):
        """Forget the returns in flight (call after an env reset)."""
        self.carry.zero_()
        return self

    def _ws(self, K):
        need = N.nbytes("ssg_ret_filter_workspace_nbytes", int(self.env.num_envs), int(K), self.n_members)
        if self.workspace.numel() < need:
            self.workspace = _torch().zeros(need, dtype=_torch().uint8, device=self.state.device)
        return self.workspace

    def to_native(self, K=1):
        """The ssg_ret_filter record for calls of up to K steps (the workspace is grown to serve them)."""
        ws = self._ws(K)
        rec = N.RetFilterRecord()
        rec.struct_size = C.sizeof(N.RetFilterRecord)
        rec.flags = N.RET_FILTER_UPDATE if self.updating else 0
        rec.n_members, rec.reserved, rec.clip, rec.eps = self.n_members, 0, self.clip, self.eps
        rec.dev_gamma, rec.dev_state, rec.dev_carry = self.gamma_dev.data_ptr(), self.state.data_ptr(), self.carry.data_ptr()
        rec.dev_workspace, rec.workspace_nbytes = ws.data_ptr(), ws.numel()
        return rec

    def _rows(self, who, rew, done=None):
        """THE check of a call's [K, N] buffers, (K, row pitch): rew f64 / done u8 (None: not taken) in the env's row layout, on its
        device, rows of unit stride and a common row pitch >= N — strided on purpose, so that [:, :N] views of wider buffers serve."""
        torch = _torch()
        env = self.env
        n_env = int(env.num_envs)
        for name, t, dt in (("rew", rew, torch.float64), ("done", done, torch.uint8)):
            if t is None:
                continue
            if t.dtype != dt or t.device != env.device or t.dim() != 2 or int(t.shape[1]) != n_env or int(t.shape[0]) < 1 or \
                    t.stride(1) != 1 or t.stride(0) < n_env:
                raise ValueError("%s: %s must be a %s tensor [K, %d] on %s with unit-stride rows (got %s %s, strides %s, on %s)"
                                 % (who, name, dt, n_env, env.device, t.dtype, tuple(t.shape), tuple(t.stride()), t.device))
        K, pitch = int(rew.shape[0]), int(rew.stride(0))
        if done is not None and (int(done.shape[0]) != K or int(done.stride(0)) != pitch):
            raise ValueError("%s: rew and done must have the same number of rows and the same row pitch" % who)
        return K, pitch

    def _pieces(self, K, call):
        """Serve K steps in pieces of the library's cap: call(record, k0, k1) for each piece [k0, k1); they leave what one call would."""
        rec = self.to_native(min(K, N.RET_FILTER_MAX_STEPS))
        for k0 in range(0, K, N.RET_FILTER_MAX_STEPS):
            call(C.byref(rec), k0, min(K, k0 + N.RET_FILTER_MAX_STEPS))

    def normalise(self, rew, done):
        """ssg_ret_filter_apply on a rollout's buffers: rew f64 / done u8 [K, N] in the env's row layout, rows of unit stride and a
        common row pitch >= N (so [:, :N] views of wider buffers serve).  Returns (out, denom): out f64 [K, N] with rew's row pitch,
        denom f64 [K, n_members], the divisor of every row.  Rollouts longer than the library's cap are served in several calls, which
        leave what one call would."""
        torch = _torch()
        env = self.env
        K, pitch = self._rows("ReturnFilter", rew, done)
        out = torch.empty((K, pitch), dtype=torch.float64, device=env.device)[:, :int(env.num_envs)]
        denom = torch.empty((K, self.n_members), dtype=torch.float64, device=env.device)
        self._pieces(K, lambda rec, k0, k1: env.enqueue("ssg_ret_filter_apply", rec, k1 - k0, rew[k0].data_ptr(), done[k0].data_ptr(), pitch,
                                                        out[k0].data_ptr(), denom[k0].data_ptr()))
        return out, denom

    def _job_rows(self, who, rew, done=None):
        """``_rows`` of a job call's buffers, for an updating job filter only."""
        if not self.job:
            raise ValueError("ReturnFilter.%s: this filter was not made with job=True (its statistics are this handle's: use apply)" % who)
        if not self.updating:
            raise ValueError("ReturnFilter.%s: a frozen filter needs no rows (apply divides by the state's own denom)" % who)
        return self._rows("ReturnFilter." + who, rew, done)

    def shard_rows(self, batch):
        """The first half of a job filter's ``apply`` (ssg_ret_filter_batches): walk batch["rew"] / batch["done"] (the carry is
        updated) and reduce this rank's envs to one row {mean, M2, 0, n} per step.  Returns the rows, f64 [K, 4] on the device; the
        state is neither read nor written.  Rollouts longer than the library's cap are served in several calls."""
        env = self.env
        rew, done = batch["rew"], batch["done"]
        K, pitch = self._job_rows("shard_rows", rew, done)
        rows = _torch().empty((K, N.FILTER_ROWS), dtype=_torch().float64, device=env.device)
        self._pieces(K, lambda rec, k0, k1: env.enqueue("ssg_ret_filter_batches", rec, k1 - k0, rew[k0].data_ptr(), done[k0].data_ptr(), pitch,
                                                        rows[k0].data_ptr()))
        return rows

    def apply_rows(self, batch, rows):
        """The second half (ssg_ret_filter_apply_rows): rows f64 [W, K, 4] on the filter's device, the ranks' ``shard_rows`` of this
        rollout in rank order (W in 1..64).  Every step's W rows are merged in rank order and chained into the state, and
        batch["rew"] is divided by the chain's denoms: writes batch["rew_norm"] (f64 [K, N]) and batch["rew_denom"] (f64 [K, 1]).
        Returns batch["rew_norm"]."""
        torch = _torch()
        env = self.env
        rew = batch["rew"]
        K, pitch = self._job_rows("apply_rows", rew)
        # (any strides serve: every piece is made contiguous below)
        if (rows.dtype != torch.float64 or rows.device != self.state.device or rows.dim() != 3 or not 1 <= int(rows.shape[0]) <= N.DP_MAX_SHARDS
                or tuple(rows.shape[1:]) != (K, N.FILTER_ROWS)):
            raise ValueError("ReturnFilter.apply_rows: rows must be a float64 tensor (W in 1..%d, %d, %d) on %s (got %s %s on %s)"
                             % (N.DP_MAX_SHARDS, K, N.FILTER_ROWS, self.state.device, rows.dtype, tuple(rows.shape), rows.device))
        W = int(rows.shape[0])
        out = torch.empty((K, pitch), dtype=torch.float64, device=env.device)[:, :int(env.num_envs)]
        denom = torch.empty((K, 1), dtype=torch.float64, device=env.device)

        def piece(rec, k0, k1):
            part = rows[:, k0:k1].contiguous()  # (the ranks' rows of this call's steps, [W, k1 - k0, 4]; the whole tensor when K fits)
            env.enqueue("ssg_ret_filter_apply_rows", rec, k1 - k0, part.data_ptr(), W, rew[k0].data_ptr(), pitch, out[k0].data_ptr(),
                        denom[k0].data_ptr())
        self._pieces(K, piece)
        batch["rew_norm"], batch["rew_denom"] = out, denom
        return out

    def apply(self, batch, group=None):
        """Normalise a rollout batch's rewards: writes batch["rew_norm"] (f64 [K, N]) and batch["rew_denom"] (f64 [K, n_members]) and
        leaves batch["rew"] alone.  Returns batch["rew_norm"].  An updating job filter: ``shard_rows``, one all-gather of the rows
        over `group` (None: the default process group; with none initialised the job is this process, W = 1), then ``apply_rows``."""
        if self.job and self.updating:
            from .sharding import all_gather_rows
            return self.apply_rows(batch, all_gather_rows(self.shard_rows(batch), group))
        batch["rew_norm"], batch["rew_denom"] = self.normalise(batch["rew"], batch["done"])
        return batch["rew_norm"]

    def state_dict(self):
        return {"state": self.state.detach().cpu().clone(), "carry": self.carry.detach().cpu().clone(), "gamma": list(self.gamma),
                "clip": self.clip, "eps": self.eps, "n_members": self.n_members}

    def load_state_dict(self, sd):
        """Copy a state_dict's statistics and carry into this filter's tensors (shapes checked), and take its gamma, clip and eps."""
        st, carry = sd["state"], sd["carry"]
        if tuple(st.shape) != tuple(self.state.shape) or tuple(carry.shape) != tuple(self.carry.shape):
            raise ValueError("ReturnFilter.load_state_dict: state %s and carry %s, this filter's are %s and %s"
                             % (tuple(st.shape), tuple(carry.shape), tuple(self.state.shape), tuple(self.carry.shape)))
        self.state.copy_(st.to(self.state.dtype))
        self.carry.copy_(carry.to(self.carry.dtype))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        return self.set_gamma(list(sd["gamma"]))
