"""A running mean / std observation filter kept and applied on the device: ObsFilter (ssg_obs_filter_update / ssg_set_obs_filter) and
merge_reference.

The reference's RLlib trainers run "PPO" with its defaults (train/rllib/pbt.py:50, train/rllib/ppo.py:28), which in the RLlib generation
those scripts are written for include ``observation_filter: "MeanStdFilter"``; Stable-Baselines users wrap the vectorised env of
train/stable_baselines/ppo.py:123 in ``VecNormalize``.  Both keep a running mean and variance per observation column, update them with
every batch of observations and feed the policy ``clip((obs - mean) / std)``.  ``ObsFilter`` is that on the device, per member of a
population when there are several: bound to a ``ShipVecEnv`` (``env.set_obs_filter(f)``), every policy launch on that env forms its
``x`` rows with it, and the rollout loops merge each step's observations ahead of the step's policy launch.  The arithmetic is defined
in include/shipsim.h (section "Observation filter") on its own terms; no bit parity with either library is claimed.

``VecNormalize``'s other half, reward / return normalisation (``norm_reward``), is ship_sim_gym_amd/ret_filter.py's ``ReturnFilter``.
RLlib synchronises its workers' filters after every training iteration; ``ObsFilter(..., job=True)`` with ``sync()`` is that for the ranks
of a data-parallel job (ship_sim_gym_amd/dp.py).  Not covered: statistics merged per step, a per-column clip.

``merge_reference`` is a numpy restatement of the device's reduction, the same tiles and trees operation for operation, for tests;
``merge_rows_reference`` restates the synchronisation's merge of the ranks' buffers.
"""
import ctypes as C

import numpy as np

from . import _native as N
from ._native import _torch


def _halving_tree(x):
    """x[0] + ... + x[255] per column as the device sums them: for h = 128, 64, ..., 1: x[i] = x[i] + x[i + h] for i < h."""
    s = np.array(x, dtype=np.float64)
    h = N.FILTER_TILE // 2
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h >>= 1
    return s[0]


def _merge(a, b):
    """(n, mean [D], M2 [D]) of a merged with b, in the header's association; an empty side leaves the other as it is."""
    if b[0] == 0.0:
        return a
    if a[0] == 0.0:
        return b
    n2 = a[0] + b[0]
    w = b[0] / n2
    delta = b[1] - a[1]
    mean = a[1] + delta * w
    m2 = (a[2] + b[2]) + (delta * delta) * (a[0] * w)
    return n2, mean, m2


def merge_reference(state_rows, batch_rows, eps=1e-8):
    """What ssg_obs_filter_update leaves in one member's state rows: state_rows f64 [4, D] (mean, M2, denom, {count, 0, ...}; zeros =
    empty) merged with batch_rows f64 [n, D], in the device's order (include/shipsim.h: 256-row tiles with two halving trees each,
    eight runs of consecutive tiles merged in tile order, a halving tree over the runs, then the merge into the state).  Returns new
    state rows; denom's square root is numpy's (the device's may differ in the last bit)."""
    st = np.array(state_rows, dtype=np.float64)
    x = np.ascontiguousarray(batch_rows, dtype=np.float64)
    if st.ndim != 2 or st.shape[0] != N.FILTER_ROWS or x.ndim != 2 or x.shape[1] != st.shape[1] or x.shape[0] < 1:
        raise ValueError("merge_reference: state_rows must be [4, D] and batch_rows [n >= 1, D]")
    n, D = x.shape
    tile, runs = N.FILTER_TILE, N.FILTER_RUNS
    T = (n + tile - 1) // tile
    L = (T + runs - 1) // runs
    zero = np.float64(0.0)
    parts = []
    for g in range(runs):
        a = (zero, np.zeros(D), np.zeros(D))
        for t in range(g * L, min((g + 1) * L, T)):
            rows = x[t * tile:(t + 1) * tile]
            nt = rows.shape[0]
            pad = np.zeros((tile, D), dtype=np.float64)
            pad[:nt] = rows
            mu = _halving_tree(pad) / np.float64(nt)
            dev = pad[:nt] - mu
            pad[:nt] = dev * dev
            a = _merge(a, (np.float64(nt), mu, _halving_tree(pad)))
        parts.append(a)
    h = runs // 2
    while h:
        for g in range(h):
            parts[g] = _merge(parts[g], parts[g + h])
        h >>= 1
    cnt, mean, m2 = _merge((np.float64(st[3, 0]), st[0].copy(), st[1].copy()), parts[0])
    out = np.zeros_like(st)
    out[0], out[1] = mean, m2
    out[2] = np.sqrt(m2 / (cnt - 1.0)) + np.float64(eps) if cnt >= 2.0 else 1.0
    out[3, 0] = cnt
    return out


def merge_rows_reference(base_rows, rows, eps=1e-8):
    """What ssg_obs_filter_merge_rows leaves in one member's state rows: base_rows f64 [4, D] merged with rows f64 [W, 4, D] (the ranks'
    buffers of that member) in index order, a row of count 0 skipped, in the header's association ("Job-wide observation filter").
    Returns new state rows; denom's square root is numpy's (the device's may differ in the last bit)."""
    base = np.array(base_rows, dtype=np.float64)
    rows = np.array(rows, dtype=np.float64)
    if base.ndim != 2 or base.shape[0] != N.FILTER_ROWS or rows.ndim != 3 or rows.shape[0] < 1 or rows.shape[1:] != base.shape:
        raise ValueError("merge_rows_reference: base_rows must be [4, D] and rows [W >= 1, 4, D]")
    a = (np.float64(base[3, 0]), base[0].copy(), base[1].copy())
    for r in rows:
        a = _merge(a, (np.float64(r[3, 0]), r[0].copy(), r[1].copy()))
    cnt, mean, m2 = a
    out = np.zeros_like(base)
    out[0], out[1] = mean, m2
    out[2] = np.sqrt(m2 / (cnt - 1.0)) + np.float64(eps) if cnt >= 2.0 else 1.0
    out[3, 0] = cnt
    return out


class ObsFilter(object):
    """The filter of `env` (a ShipVecEnv): owns the state tensor f64 [n_members, 4, D] (mean, M2, denom, {count, 0, ...} per member; zeros
    = empty, which normalises as mean 0, denom 1) and the workspace of the update's partials.  n_members: 1 for a single policy, P for
    a population (member m's statistics come from its own env slice).  clip: |x| is clamped to it (0: no clamp); eps: added to the
    standard deviation.  update: whether the rollout loops of an env this filter is bound to merge each step's observations
    (``train(flag)`` changes it later; ``frozen()`` gives a view that never does).

    Bind it with ``env.set_obs_filter(f)``; then ``policy_act``, ``rollout_policy``, ``population_act``, ``rollout_population`` and
    ``NativeEvaluator`` use it without further arguments, and the policy's ``obs_scale`` is not read.

    job=True: the filter of one rank of a data-parallel job (include/shipsim.h, "Job-wide observation filter").  It also owns ``buffer``
    (this rank's own statistics since the last synchronisation; ``env.set_obs_filter(f)`` binds it too, and every update then merges
    into both) and ``base`` (the state all ranks held right after it).  ``sync(group)`` after each rollout gathers the ranks' buffers
    and merges them into every rank's state, bit-identically; ``merge_rows(rows)`` is its second half, so that one process can replay
    a W-rank job with ``torch.stack`` of the ranks' buffers as the gather."""

    def __init__(self, env, n_members=1, clip=10.0, eps=1e-8, update=True, job=False, _state=None):
        torch = _torch()
        P, D = int(n_members), int(env.states_history)
        clip, eps = float(clip), float(eps)
        if P < 1 or P > N.POP_MAX_MEMBERS:
            raise ValueError("ObsFilter: n_members must be in 1..%d" % N.POP_MAX_MEMBERS)
        if not clip >= 0.0 or not eps >= 0.0:
            raise ValueError("ObsFilter: clip and eps must be >= 0")
        self.env, self.n_members, self.obs_dim, self.clip, self.eps, self.updating = env, P, D, clip, eps, bool(update)
        dev = env.device
        nbytes = N.nbytes("ssg_obs_filter_workspace_nbytes", int(env.num_envs), D, P)
        self.state = _state if _state is not None else torch.zeros((P, N.FILTER_ROWS, D), dtype=torch.float64, device=dev)
        self.workspace = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.job = bool(job)
        self.buffer = torch.zeros_like(self.state) if self.job else None
        self.base = self.state.clone() if self.job else None
        self._bound = []  # the envs this record is bound to: train() re-binds them (a binding is a copy of the record)
        self._views = []  # the frozen() views of this filter: they follow its clip and eps

    # the state's rows (views of the state tensor; `var` is computed)
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
        return self.state[:, 3, 0]

    @property
    def var(self):
        """The sample variance M2 / (count - 1), f64 [n_members, D]; 1 where count < 2."""
        torch = _torch()
        c = self.count[:, None]
        return torch.where(c >= 2.0, self.M2 / (c - 1.0).clamp(min=1.0), torch.ones_like(self.M2))

    def to_native(self):
        rec = N.ObsFilterRecord()
        rec.struct_size = C.sizeof(N.ObsFilterRecord)
        rec.flags = N.FILTER_UPDATE if self.updating else 0
        rec.n_members, rec.obs_dim, rec.clip, rec.eps = self.n_members, self.obs_dim, self.clip, self.eps
        rec.dev_state, rec.dev_workspace, rec.workspace_nbytes = self.state.data_ptr(), self.workspace.data_ptr(), self.workspace.numel()
        return rec

    def update(self, obs=None):
        """Merge a batch of observations into the state (ssg_obs_filter_update, two launches on the current stream), whatever
        ``updating`` says: obs f64 [N, D] in the env's row layout (default: the env's current ``obs``); member m's rows are its slice.
        A job filter merges the batch into its buffer too (ssg_obs_filter_update_buffered: the same two launches)."""
        torch = _torch()
        env = self.env
        obs = env.obs if obs is None else obs
        op = N.arg(obs, torch.float64, (env.num_envs, self.obs_dim), "ObsFilter.update: obs", env.device)
        rec = self.to_native()
        if self.job:
            env.enqueue("ssg_obs_filter_update_buffered", C.byref(rec), self.buffer.data_ptr(), op)
        else:
            env.enqueue("ssg_obs_filter_update", C.byref(rec), op)

    def merge_rows(self, rows):
        """The second half of ``sync``: rows f64 [W, n_members, 4, D] on the filter's device (the ranks' buffers in rank order; W in
        1..64).  state = base merged with rows[0], ..., rows[W - 1] (ssg_obs_filter_merge_rows, one launch on the current stream), then
        base <- state and buffer <- 0."""
        torch = _torch()
        env = self.env
        if not self.job:
            raise ValueError("ObsFilter.merge_rows: this filter was not made with job=True (it has no base and no buffer)")
        rp = N.arg(rows, torch.float64, (1,) + tuple(self.state.shape), "ObsFilter.merge_rows: rows", self.state.device, more_rows=True)
        if rows.shape[0] > N.DP_MAX_SHARDS:
            raise ValueError("ObsFilter.merge_rows: rows holds the buffers of %d ranks, a call merges %d at most" % (rows.shape[0], N.DP_MAX_SHARDS))
        env.enqueue("ssg_obs_filter_merge_rows", C.byref(self.to_native()), self.base.data_ptr(), rp, int(rows.shape[0]))
        self.base.copy_(self.state)
        self.buffer.zero_()
        return self

    def sync(self, group=None):
        """After a rollout, before GAE, on every rank of the job: all-gather the ranks' buffers in rank order and merge them into the
        state (``merge_rows``).  Every rank runs the same arithmetic on the same rows, so the states agree bit for bit without a
        broadcast.  Without a process group it merges this filter's own buffer."""
        from .sharding import all_gather_rows
        return self.merge_rows(all_gather_rows(self.buffer, group))

    def train(self, flag=True):
        """Whether the rollout loops update the statistics (``VecNormalize.training``); re-binds the envs this record is bound to."""
        self.updating = bool(flag)
        for env in list(self._bound):
            env.set_obs_filter(self)
        return self

    def frozen(self, env=None):
        """A second record over the SAME state tensor that never updates, for `env` (default: this filter's env) — what a trainer
        binds to its evaluation env.  It has a workspace of its own, sized for that env, and follows this filter's clip and eps: a
        later ``load_state_dict`` on this filter re-binds the views' envs with the loaded values too."""
        view = ObsFilter(self.env if env is None else env, self.n_members, self.clip, self.eps, update=False, _state=self.state)
        self._views.append(view)
        return view

    def _member_rows(self, n_rows):
        """The member index of each of the env's rows (the env's population slices, else the equal split)."""
        torch = _torch()
        sizes = getattr(self.env, "population_slices", None)
        if sizes is None:
            if n_rows % self.n_members:
                raise ValueError("ObsFilter.normalise: %d rows do not split into %d equal member slices" % (n_rows, self.n_members))
            sizes = [n_rows // self.n_members] * self.n_members
        if len(sizes) != self.n_members or sum(sizes) != n_rows:
            raise ValueError("ObsFilter.normalise: the env's slices %s do not lay out %d rows for %d members" % (sizes, n_rows, self.n_members))
        return torch.repeat_interleave(torch.arange(self.n_members), torch.tensor(sizes)).to(self.state.device)

    def normalise(self, obs, member=None):
        """The torch restatement of what the policy kernel forms: ((obs - mean) / denom).clamp(-clip, +clip).float(), in f64 until the
        last step; a denom entry of 0 (the empty state) divides by 1.  obs: f64 [..., D].  member: the member whose rows to use; None:
        the only member, or — for a population — obs is [N, D] in the env's row layout and every row uses its own member's."""
        torch = _torch()
        obs = obs.to(torch.float64)
        mean, den = self.mean, self.denom
        den = torch.where(den == 0.0, torch.ones_like(den), den)
        if member is not None:
            mean, den = mean[int(member)], den[int(member)]
        elif self.n_members == 1:
            mean, den = mean[0], den[0]
        else:
            idx = self._member_rows(obs.shape[0])
            mean, den = mean[idx], den[idx]
        v = (obs - mean.to(obs.device)) / den.to(obs.device)
        if self.clip > 0.0:
            v = v.clamp(-self.clip, self.clip)
        return v.float()

    def state_dict(self):
        sd = {"state": self.state.detach().cpu().clone(), "clip": self.clip, "eps": self.eps, "n_members": self.n_members,
              "obs_dim": self.obs_dim}
        if self.job:  # (a plain filter's dict stays what it was; a plain filter loads a job's dict and reads its state alone)
            sd.update(base=self.base.detach().cpu().clone(), buffer=self.buffer.detach().cpu().clone())
        return sd

    def load_state_dict(self, sd):
        """Copy a state_dict's statistics into this filter's state tensor (shape checked), and take its clip and eps.  A job filter
        takes base and buffer too; from a plain filter's dict, which has neither, the state becomes the base and the buffer is empty."""
        st = sd["state"]
        if self.job and ("base" in sd) != ("buffer" in sd):
            raise ValueError("ObsFilter.load_state_dict: a job filter's dict holds base and buffer, or neither")
        base, buffer = (sd.get("base", st), sd.get("buffer")) if self.job else (st, None)
        for t in (st, base) + (() if buffer is None else (buffer,)):
            if tuple(t.shape) != tuple(self.state.shape):
                raise ValueError("ObsFilter.load_state_dict: state of shape %s, this filter's is %s" % (tuple(t.shape), tuple(self.state.shape)))
        self.state.copy_(st.to(self.state.dtype))
        if self.job:
            self.base.copy_(base.to(self.state.dtype))
            if buffer is None:
                self.buffer.zero_()
            else:
                self.buffer.copy_(buffer.to(self.state.dtype))
        self.clip, self.eps = float(sd["clip"]), float(sd["eps"])
        for f in [self] + self._views:  # (training and evaluation must normalise alike)
            f.clip, f.eps = self.clip, self.eps
            for env in list(f._bound):
                env.set_obs_filter(f)
        return self
