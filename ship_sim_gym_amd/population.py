"""A population of policies trained on one handle: NativePopulation, PopulationPPO and PBTScheduler (the ssg_pop_* entry points).

Both reference trainers train populations: train/rllib/pbt.py runs 120 PPO trials under ray's PopulationBasedTraining (:29-43 the
scheduler, :47-74 the experiment) and train/stable_baselines/ppo.py:118-137 three PPO2 models, one per learning rate.  A member of such a
population is a small batch, and at small batches the device waits on launches; here the P members share every launch — one policy
launch per rollout step, two launches for GAE, two per minibatch of the update — and each member's results are bit for bit what
``NativePolicy`` / ``NativePPO`` compute for that member alone on its own shard of the envs.

The handle's envs are split into P equal contiguous slices: member m owns envs [m*n, (m+1)*n), n = num_envs / P.  ``params`` is f32
[P, L]; row m is a packed buffer of its own, and ``member(m)`` is a ``NativePolicy`` that shares it.  Hyper-parameters are per member
(plain Python lists on ``PopulationPPO`` that a scheduler may rewrite between updates), and so may the epochs and the minibatch count
of an update be (``update`` with lists: ssg_pop_update_sched — launch j then serves minibatch j of every member that still has one);
so may the batch size, as a member's share of the handle's envs (``ShipVecEnv.set_population_slices``: contiguous slices of unequal
size; ``slices_for_batch_sizes`` turns batch sizes into slices) — every member still rolls out the same K steps on one handle with one
architecture, and an update on unequal slices always runs on the schedule path.  The extended loss terms of
``NativePPO`` — ``vf_clip``, ``max_grad_norm``, ``kl_coef``, ``kl_target`` — are per member as well (``EXT_KEYS``); a member whose value
is 0 has that term off and trains exactly as ``NativePPO`` without it.

``PBTScheduler`` is host-only (``random`` with its own seeded generator, no torch): ray 0.6's PopulationBasedTraining as the reference
configures it, with the interval counted in updates instead of seconds of wall time.
"""
import ctypes as C
import math
import random
from fractions import Fraction

from . import _native as N
from . import hparam_schedule as HS
from ._native import _torch
from .policy import ACTIVATIONS, NativePolicy
from .ppo import DeviceTrainer, adv_norm_mode, adv_norm_scratch, adv_norm_views, chunk_split, load_packed


class NativePopulation(object):
    """members: P ``NativePolicy`` objects of one shape, activation and device (their parameters are copied into row m of ``params`` and
    each member is re-pointed at its row).  obs_scale: f64 [obs_dim] common to the population (default: member 0's)."""

    def __init__(self, members, obs_scale=None):
        torch = _torch()
        members = list(members)
        if not 1 <= len(members) <= N.POP_MAX_MEMBERS:
            raise ValueError("NativePopulation: 1..%d members (got %d)" % (N.POP_MAX_MEMBERS, len(members)))
        first = members[0]
        shape = (first.obs_dim, first.hidden, first.n_hidden_layers, first.n_actions, first.activation, first.device, first.separate_value)
        for m, pol in enumerate(members):
            if (pol.obs_dim, pol.hidden, pol.n_hidden_layers, pol.n_actions, pol.activation, pol.device, pol.separate_value) != shape:
                raise ValueError("NativePopulation: member %d differs from member 0 in shape (shared body or separate value network), "
                                 "activation or device" % m)
        self.obs_dim, self.hidden, self.n_hidden_layers, self.n_actions, self.activation, self.device, self.separate_value = shape
        self.offsets, self.n_params = first.offsets, first.params.numel()
        if obs_scale is None:
            obs_scale = first.obs_scale
        elif not torch.is_tensor(obs_scale):
            obs_scale = torch.full((self.obs_dim,), float(obs_scale), dtype=torch.float64)
        obs_scale = obs_scale.detach().to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        if obs_scale.numel() != self.obs_dim:
            raise ValueError("NativePopulation: obs_scale has %d entries, obs_dim is %d" % (obs_scale.numel(), self.obs_dim))
        self.obs_scale = obs_scale
        with torch.no_grad():
            self.params = torch.stack([pol.params for pol in members]).contiguous()
        self._members = members
        for m, pol in enumerate(members):  # a member IS its row from now on
            pol.params = self.params[m]
            pol.obs_scale = self.obs_scale

    @classmethod
    def from_actor_critics(cls, nets, obs_scale):
        """A population over the parameters OF `nets` (modules shaped like train/ppo_torch.py's ActorCritic — shared body or separate
        value network — all alike)."""
        return cls([NativePolicy.from_actor_critic(net, obs_scale) for net in nets])

    @classmethod
    def from_layers(cls, members, obs_scale, activation="tanh"):
        """members: per member a (layers, pi, v) triple of (W, b) tensors, as NativePolicy's constructor takes them, or a
        (layers, pi, v, value_layers) quadruple for a separate value network."""
        return cls([NativePolicy(m[0], m[1], m[2], obs_scale, activation=activation, value_layers=m[3] if len(m) > 3 else None)
                    for m in members])

    def __len__(self):
        return len(self._members)

    def member(self, m):
        """Member m as a NativePolicy whose ``params`` is row m of this population's (a view: nothing is copied)."""
        return self._members[m]

    def refresh(self):
        """Re-pack every member's source tensors into its row (after an optimiser step on the modules)."""
        for pol in self._members:
            pol.refresh()
        return self.params

    def load_into(self, nets):
        """Copy row m into nets[m] (modules shaped like the members), for checkpoints."""
        nets = list(nets)
        if len(nets) != len(self):
            raise ValueError("NativePopulation.load_into: %d modules for %d members" % (len(nets), len(self)))
        for m, net in enumerate(nets):
            load_packed(self.params[m], net, "NativePopulation.load_into: module %d has %%d parameters, a member %d" % (m, self.n_params))
        return nets

    # ------------------------------------------------------------------------------------------------
    # state (ship_sim_gym_amd/checkpoint.py)
    # ------------------------------------------------------------------------------------------------
    def architecture(self):
        """The member count and the fields that fix a row's layout, as (name, value) pairs: what a state must agree with."""
        return [("n_members", len(self))] + self._members[0].architecture()

    def state_dict(self):
        """The architecture, ``params`` [P, L] and the observation scale (CPU copies; plain data only)."""
        sd = dict(self.architecture())
        sd["params"], sd["obs_scale"] = self.params.detach().cpu().clone(), self.obs_scale.detach().cpu().clone()
        return sd

    def load_state_dict(self, sd):
        """Take a state_dict's rows and observation scale, in place.  Checked first: a member count, an architecture field, a shape or
        a dtype that differs raises ValueError naming the field with both values, and nothing is copied.  The tensors the members
        were built over (the modules' parameters) get the loaded rows, then ``refresh()`` re-packs them: the rows, the members' views
        and the modules agree afterwards."""
        from .checkpoint import check_state
        check_state("NativePopulation.load_state_dict", sd, self.architecture(), [("params", self.params), ("obs_scale", self.obs_scale)])
        with _torch().no_grad():
            self.params.copy_(sd["params"])
            self.obs_scale.copy_(sd["obs_scale"])
            for pol in self._members:
                pol.push_sources()
        self.refresh()
        return self

    @classmethod
    def from_state_dict(cls, sd, device):
        """A NativePopulation on `device` built from a state_dict alone (no modules): the architecture comes from the state."""
        from .checkpoint import check_values
        if not isinstance(sd, dict):
            raise ValueError("NativePopulation.from_state_dict: a state dict is a dict (got a %s)" % type(sd).__name__)
        check_values("NativePopulation.from_state_dict", sd, [("n_members", int)])
        params = sd.get("params")
        if not _torch().is_tensor(params) or params.dim() != 2 or int(params.shape[0]) != sd["n_members"]:
            raise ValueError("NativePopulation.from_state_dict: params must be a tensor [n_members = %d, L]" % sd["n_members"])
        return cls([NativePolicy.from_state_dict(sd, device, row=m) for m in range(sd["n_members"])])

    def to_native(self):
        """The ssg_population record (pointers into this object's tensors: keep it alive while the library uses it)."""
        p = N.Population()
        p.struct_size = C.sizeof(N.Population)
        p.n_members = len(self)
        p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions = self.obs_dim, self.hidden, self.n_hidden_layers, self.n_actions
        p.activation = ACTIVATIONS[self.activation] | (N.POLICY_SEPARATE_VALUE if self.separate_value else 0)
        p.dev_params, p.dev_obs_scale = self.params.data_ptr(), self.obs_scale.data_ptr()
        return p


HPARAM_KEYS = ("gamma", "lam", "clip", "vf_coef", "ent_coef", "lr", "beta1", "beta2", "eps", "adv_eps")
# the extended update's per-member settings: lists like the ones above, except kl_coef, which is a device tensor f32 [P] (the update
# adapts it on the device against kl_target)
EXT_KEYS = ("vf_clip", "max_grad_norm", "kl_target")


class PopulationPPO(DeviceTrainer):
    """GAE and the PPO update of every member of a NativePopulation in shared launches (ssg_pop_gae / ssg_pop_update), the PBT exploit
    copy (ssg_pop_exploit) and per-member episode statistics (ssg_pop_episode_stats).  Owns the Adam moments [P, 2L], the workspace and
    the episode carry columns.  Every hyper-parameter is a list of P floats (``self.lr[m] = ...``); defaults: NativePPO's.  So are
    ``vf_clip``, ``max_grad_norm`` and ``kl_target`` (0 = off); ``kl_coef`` is given as a float or a list and kept as a device tensor
    f32 [P] (``self.kl_coef``), since the update adapts it on the device.  With every extended setting 0 the plain entry points run.
    ``adv_norm="minibatch"`` (one mode for all members) normalises every member's advantages inside each of ITS minibatches, as
    Stable-Baselines' PPO2 does, instead of once per rollout (ssg_ppo_set_adv_norm; ``minibatch_adv_stats()``).
    ``perm_seed``: the library draws the members' minibatch permutations (ssg_pop_perm, one launch): ``update(batch, None, ...)``
    shuffles every member as ``NativePPO(perm_seed=..., member=m)`` shuffles alone, keyed by ``updates``, this object's count of
    update() calls; ``draw_perm`` returns them in the layout the bound state makes ``update`` expect.

    Hyper-parameter schedules (``HparamSchedule``; not the update schedule of epochs x minibatches): each of ``lr``, ``clip`` and
    ``ent_coef`` may be a float, an HparamSchedule, or a list of P of either.  ``self.lr`` / ``self.clip`` / ``self.ent_coef`` stay lists
    of P floats, the CURRENT values; ``set_timesteps`` rewrites a scheduled member's entries from its own clock (members have clocks
    of their own: under unequal slices their batches differ).  So ``ppo.lr[m] = x`` on a scheduled member lasts until the next
    ``set_timesteps``; ``clear_schedule(name, m)`` makes the member's value a constant again.  ``exploit`` leaves schedules and clocks
    where they are: like ``lam``, ``clip`` and ``lr`` themselves they are the scheduler's business, not the weights'."""

    def __init__(self, population, env, gamma=0.99, lam=0.95, clip=0.2, vf_coef=0.5, ent_coef=0.01, lr=3e-4, beta1=0.9, beta2=0.999,
                 eps=1e-8, adv_eps=1e-8, vf_clip=0.0, max_grad_norm=0.0, kl_coef=0.0, kl_target=0.0, adv_norm="batch", perm_seed=None):
        torch = _torch()
        self.population, self.env, self._device = population, env, population.device
        P = len(population)
        self.perm_seed = None if perm_seed is None else int(perm_seed)  # None: the caller brings every perm
        self.updates = 0  # calls of update(); like `step`, load_state_dict() sets it
        # "batch": every member's advantages are normalised once per rollout; "minibatch": inside every minibatch (PPO2's rule), the
        # same mode for all members
        self.adv_norm = adv_norm
        self._adv_mode = adv_norm_mode(adv_norm, "PopulationPPO")
        self._adv_scratch = adv_norm_scratch(P, population.device) if self._adv_mode == N.ADV_NORM_MINIBATCH else None
        if env.states_history != population.obs_dim:
            raise ValueError("PopulationPPO: the env's observation width %d differs from the population's obs_dim %d"
                             % (env.states_history, population.obs_dim))
        env._check_population(population, "PopulationPPO")  # (the env's slices for P members, else an equal split)
        given = dict(gamma=gamma, lam=lam, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, lr=lr, beta1=beta1, beta2=beta2, eps=eps,
                     adv_eps=adv_eps, vf_clip=vf_clip, max_grad_norm=max_grad_norm, kl_target=kl_target, kl_coef=kl_coef)
        # hyper-parameter schedules (hparam_schedule.py), per member: schedules[name][m] is member m's HparamSchedule or None (a
        # constant); timesteps[m] its clock.  The lists of floats below then hold the schedules' values at the clocks (0 for now).
        self.schedules, self.timesteps = {k: [None] * P for k in HS.SCHEDULABLE}, [0] * P
        for k in HPARAM_KEYS + EXT_KEYS + ("kl_coef",):
            v = given[k]
            v = list(v) if isinstance(v, (list, tuple)) else [v] * P
            if len(v) != P:
                raise ValueError("PopulationPPO: %s has %d entries for %d members" % (k, len(v), P))
            if k in HS.SCHEDULABLE:
                pairs = [HS.split("PopulationPPO: member %d" % m, k, x) for m, x in enumerate(v)]
                v, self.schedules[k] = [p[0] for p in pairs], [p[1] for p in pairs]
            setattr(self, k, [float(x) for x in v])
        self.n_members, self.n_params = P, population.n_params
        dev = population.device
        self.adam_mv = torch.zeros((P, 2 * self.n_params), dtype=torch.float32, device=dev)  # per member: m, then v
        self.step = 0  # Adam steps taken (common to the population while every update steps every member alike)
        # Adam steps taken per member.  They differ once an update ran on per-member schedules; while they are all equal, `step` is
        # the count that is used (and may be set by the caller), and member_steps follows it.
        self.member_steps = [0] * P
        self.workspace = torch.zeros(0, dtype=torch.uint8, device=dev)
        self.carry_return = torch.zeros(env.num_envs, dtype=torch.float64, device=dev)
        self.carry_length = torch.zeros(env.num_envs, dtype=torch.int32, device=dev)
        self.kl_coef = torch.tensor(self.kl_coef, dtype=torch.float32).to(dev)  # (the list set above becomes the device tensor)
        self._last_K = 0  # the rollout length of the last batch gae() or update() saw (minibatches_for_size's default)
        self.return_filter = None  # set_return_filter: the ReturnFilter whose state rows travel with an exploit
        self._last_taken = None  # the steps each member took in the last update(): the stats rows report() reads (None: all of them)

    @property
    def member_envs(self):
        """The members' env counts, a list of P ints: the env's slices (``set_population_slices``, read at every call, so the layout
        may change between updates), else the equal split."""
        sizes = self.env.population_slices
        if sizes is None:
            return [self.env.num_envs // self.n_members] * self.n_members
        if len(sizes) != self.n_members:
            raise ValueError("PopulationPPO: slices for %d members are bound to the env, the population has %d" % (len(sizes), self.n_members))
        return sizes

    @property
    def envs_per_member(self):
        """The env count every member has; raises when the env's slices are unequal (``member_envs`` lists them)."""
        sizes = self.member_envs
        if len(set(sizes)) > 1:
            raise ValueError("PopulationPPO.envs_per_member: the members' slices are unequal (%s): see member_envs" % (sizes,))
        return sizes[0]

    # ------------------------------------------------------------------------------------------------
    def set_timesteps(self, t):
        """Set the clocks of the hyper-parameter schedules — t: an int >= 0 for every member, or a list of P of them, member m's own
        timesteps collected before the update that follows — and write every scheduled member's values at its clock into the
        ``lr`` / ``clip`` / ``ent_coef`` lists.  Host only: nothing is launched.  A member without a schedule keeps its value."""
        P, who = self.n_members, "PopulationPPO.set_timesteps"
        ts = list(t) if isinstance(t, (list, tuple)) else [t] * P
        if len(ts) != P:
            raise ValueError("%s: %d clocks for %d members" % (who, len(ts), P))
        self.timesteps = [HS.check_clock(who, x) for x in ts]
        for name, scheds in self.schedules.items():
            for m, sched in enumerate(scheds):
                if sched is not None:
                    getattr(self, name)[m] = sched.value(self.timesteps[m])
        return self

    def clear_schedule(self, name, m):
        """Drop member m's hyper-parameter schedule of `name` ("lr", "clip" or "ent_coef"): its current value stays, as a constant."""
        if name not in HS.SCHEDULABLE:
            raise ValueError("PopulationPPO.clear_schedule: %r is not one of %s" % (name, ", ".join(HS.SCHEDULABLE)))
        self.schedules[name][int(m)] = None
        return self

    def hparams(self):
        """The members' hyper-parameters as a ctypes array of P ssg_ppo_hparams."""
        arr = (N.PpoHparams * self.n_members)()
        for m in range(self.n_members):
            arr[m].struct_size = C.sizeof(N.PpoHparams)
            for k in HPARAM_KEYS:
                setattr(arr[m], k, float(getattr(self, k)[m]))
        return arr

    def diverged(self):
        """True once the members have taken different numbers of Adam steps (an update on unequal schedules, or an exploit after one)."""
        return len(set(self.member_steps)) > 1

    def _steps0(self):
        """The Adam steps every member has taken so far: ``step`` for all while they agree, else ``member_steps``."""
        return list(self.member_steps) if self.diverged() else [int(self.step)] * self.n_members

    def _advance(self, steps0, taken):
        self.member_steps = [s + int(t) for s, t in zip(steps0, taken)]
        self.step = max(self.member_steps)

    def _table(self, n_steps, steps0=None):
        """The members' f32 constants for GAE, the loss and Adam steps self.step + 1 .. + n_steps, derived by the library on the host
        in double (ssg_pop_pack_hparams) and uploaded: a fresh device tensor per call, so the lists may change right after.  steps0: a
        starting step per member (ssg_pop_pack_hparams_steps)."""
        torch = _torch()
        n = N.pop_table_floats(self.n_members, n_steps)
        buf = (C.c_float * n)()
        name, step0 = "ssg_pop_pack_hparams", int(self.step)
        if steps0 is not None:
            name, step0 = "ssg_pop_pack_hparams_steps", (C.c_int64 * self.n_members)(*[int(x) for x in steps0])
        N.call(name, self.n_members, self.hparams(), step0, int(n_steps), buf, n)
        return torch.tensor(list(buf), dtype=torch.float32).to(self.population.device)

    def minibatches_for_size(self, size, samples=None, member=None):
        """The minibatch count that makes minibatches of at most `size` samples out of a member's `samples` (default: the last
        batch's K * envs_per_member, or with member=m K * member_envs[m], that member's own): ceil(samples / size), clamped to [1, samples].  The chunk lengths stay torch.chunk's — every
        chunk ceil(samples / count) long and the last one shorter, so chunks of AT MOST `size` — not RLlib's slicing of exactly
        sgd_minibatch_size samples with a shorter remainder."""
        if samples is None:
            samples = self._last_K * (self.envs_per_member if member is None else self.member_envs[int(member)])
        n = int(samples)
        if n < 1:
            raise ValueError("PopulationPPO.minibatches_for_size: no batch seen yet; pass samples=")
        return max(1, min(n, -(-n // max(1, int(size)))))

    def pack_schedule(self, samples, epochs, minibatches):
        """(int32 host table as a ctypes array, steps per member, launches) of ssg_pop_pack_schedule — or, with `samples` a list of P
        counts, of ssg_pop_pack_schedule_samples."""
        P = self.n_members
        ep, mb = (C.c_int32 * P)(*[int(e) for e in epochs]), (C.c_int32 * P)(*[int(b) for b in minibatches])
        steps, launches = (C.c_int32 * P)(), C.c_int32()
        if isinstance(samples, (list, tuple)):
            name, sm = "ssg_pop_pack_schedule_samples", (C.c_int64 * P)(*[int(x) for x in samples])
        else:
            name, sm = "ssg_pop_pack_schedule", int(samples)

        def pack(buf, n):
            N.call(name, P, sm, ep, mb, buf, n, steps, C.byref(launches))
        pack(None, 0)  # the size query
        n = N.pop_sched_ints(P, launches.value)
        buf = (C.c_int32 * n)()
        pack(buf, n)
        return buf, list(steps), int(launches.value)

    def _ws(self, samples_per_member, max_minibatch):
        """The workspace, grown to serve the sizes (its head — the members' advantage statistics — is kept when it grows)."""
        return self._grow("ssg_pop_workspace_nbytes", self.population.to_native(), samples_per_member, max_minibatch, 16 * self.n_members)

    def _flat(self, batch, key, dtype, shape, who="PopulationPPO"):
        """The address of batch[key], checked (N.arg) as `dtype`, contiguous, on the device and of exactly `shape`."""
        return N.arg(batch[key], dtype, tuple(shape), "%s: batch[%r]" % (who, key), self._device)

    def _KN(self, batch):
        rew = batch["rew"]
        if rew.dim() != 2 or int(rew.shape[1]) != self.env.num_envs:
            raise ValueError("PopulationPPO: batch['rew'] must be [K, %d] (the handle's envs)" % self.env.num_envs)
        return int(rew.shape[0]), self.env.num_envs

    # ------------------------------------------------------------------------------------------------
    def set_return_filter(self, flt):
        """Register a ``ReturnFilter`` of P members (None: none) so that ``exploit`` copies the source member's state rows with its
        weights.  ``gae(batch, return_filter=f)`` applies a filter whether or not it is registered."""
        if flt is not None and flt.n_members != self.n_members:
            raise ValueError("PopulationPPO.set_return_filter: the filter has %d members, the population %d" % (flt.n_members, self.n_members))
        self.return_filter = flt
        return self

    def gae(self, batch, return_filter=None):
        """GAE of every member over its columns of the rollout batch (``rollout_population``'s dict) with its own gamma / lam: returns
        (adv, ret) f32 [K, N], stored in the batch as "adv" / "ret"; leaves the per-member advantage statistics for update().
        return_filter (a ``ReturnFilter`` of P members): it is applied to the batch first and GAE runs on batch["rew_norm"];
        batch["rew"] stays as it is.  With "boot" in the batch (env.set_timeout_bootstrap): ssg_pop_gae_boot — a done sample's one-step
        target is gamma_m * boot instead of 0; boot goes in as it is, with a return filter too."""
        torch = _torch()
        K, n_env = self._KN(batch)
        dev, who = self.population.device, "PopulationPPO.gae"
        if return_filter is not None:
            return_filter.apply(batch)
        p = [self._flat(batch, "rew" if return_filter is None else "rew_norm", torch.float64, (K, n_env), who),
             self._flat(batch, "done", torch.uint8, (K, n_env), who), self._flat(batch, "val", torch.float32, (K, n_env), who),
             self._flat(batch, "last_val", torch.float32, (n_env,), who)]
        name = "ssg_pop_gae"
        if "boot" in batch:
            p.append(self._flat(batch, "boot", torch.float32, (K, n_env), who))
            name = "ssg_pop_gae_boot"
        self._ws(K * max(self.member_envs), 1)
        self._last_K = K
        adv = torch.empty((K, n_env), dtype=torch.float32, device=dev)
        ret = torch.empty_like(adv)
        table = self._table(0)  # (no Adam rows: the step counts do not enter)
        self.env.enqueue(name, C.byref(self.population.to_native()), table.data_ptr(), K, *p, adv.data_ptr(), ret.data_ptr(), *self._ws_ptr())
        batch["adv"], batch["ret"] = adv, ret
        return adv, ret

    def extended(self):
        """True when some member has an extended term on: update() then goes through ssg_pop_update_ext."""
        return any(v > 0.0 for k in EXT_KEYS[:2] for v in getattr(self, k)) or bool((self.kl_coef > 0).any())

    def dist(self, batch):
        """Every member's log-distribution over its columns of the batch's stored observations (ssg_pop_dist, one launch): f32
        [K, N, 4], stored as batch["logp_all"].  With the acting parameters, logp_all.gather(act) is batch["logp"] bitwise."""
        torch = _torch()
        K, n_env = self._KN(batch)
        dev, D = self.population.device, self.population.obs_dim
        x = self._flat(batch, "obs", torch.float32, (K, n_env, D))
        out = torch.empty((K, n_env, 4), dtype=torch.float32, device=dev)
        self.env.enqueue("ssg_pop_dist", C.byref(self.population.to_native()), K, x, out.data_ptr())
        batch["logp_all"] = out
        return out

    def _ext(self, batch, K, n_env):
        """(the ssg_pop_ext record, the tensors it points into)"""
        torch = _torch()
        dev = self.population.device
        rows = [[self.vf_clip[m], self.max_grad_norm[m], self.kl_target[m], 0.0] for m in range(self.n_members)]
        table = torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(dev)  # (rounded from double, as the library rounds)
        ext = N.PopExt()
        ext.struct_size = C.sizeof(N.PopExt)
        ext.dev_ext = table.data_ptr()
        if any(v > 0.0 for v in self.max_grad_norm):
            ext.flags |= N.POP_EXT_GRAD_CLIP
        if any(v > 0.0 for v in self.vf_clip):
            ext.flags |= N.POP_EXT_VF_CLIP
            ext.dev_value_old = self._flat(batch, "val", torch.float32, (K, n_env))
        if bool((self.kl_coef > 0).any()):
            if "logp_all" not in batch:
                self.dist(batch)
            ext.dev_kl_coef = self.kl_coef.data_ptr()
            ext.dev_logp_all = self._flat(batch, "logp_all", torch.float32, (K, n_env, 4))
        return ext, table

    def adv_stats(self):
        """f32 [P, 3] device view: per member the advantage mean, std + adv_eps and its inverse, as the last gae() left them."""
        return self.workspace[:16 * self.n_members].view(_torch().float32).view(self.n_members, 4)[:, :3]

    def _bind_adv_norm(self):
        """(Re)bind this object's mode on the env (host only): two trainers on one env cannot inherit each other's."""
        self.env.set_adv_norm(self._adv_mode, self._adv_scratch, self.n_members)

    def minibatch_adv_stats(self):
        """f32 [P, 4] device view of the scratch: per member {mean, std + adv_eps, its inverse, 0} of the LAST minibatch an update() of
        this object normalised that member by (adv_norm="minibatch" only)."""
        if self._adv_scratch is None:
            raise ValueError("PopulationPPO.minibatch_adv_stats: adv_norm is %r" % (self.adv_norm,))
        return adv_norm_views(self._adv_scratch, self.n_members)[0]

    def draw_perm(self, batch_or_K, epochs, out=None):
        """The permutations update(batch, None, epochs, ...) would use NOW, in the layout update() expects of `perm` in the env's
        current state (ssg_pop_perm, one launch on the current stream): member m's row e is keyed (perm_seed, updates, m, e) over its
        own K * n_m samples — NativePPO(perm_seed=..., member=m).draw_perm's rows bit for bit.  epochs: an int or the members' list
        (max(epochs) rows each).  Equal slices: int64 [P, max(epochs), K*n]; slices bound to the env: the flat int64
        [max(epochs) * K * num_envs] buffer, member after member.  batch_or_K: a batch or its rollout length K; out: a tensor of
        that shape to fill."""
        torch = _torch()
        if self.perm_seed is None:
            raise ValueError("PopulationPPO.draw_perm: no perm_seed was given")
        K = self._KN(batch_or_K)[0] if isinstance(batch_or_K, dict) else int(batch_or_K)
        E = max(int(e) for e in epochs) if isinstance(epochs, (list, tuple)) else int(epochs)
        P, dev = self.n_members, self.population.device
        sizes = self.member_envs
        sliced = self.env.population_slices is not None
        shape = (E * K * sum(sizes),) if sliced else (P, E, K * sizes[0])
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=dev)
        op = N.arg(out, torch.int64, shape, "PopulationPPO.draw_perm: out", dev)
        self.env.enqueue("ssg_pop_perm", self.perm_seed, self.updates, P, K, sizes[0], E, op)
        return out

    def update(self, batch, perm, epochs, minibatches, stats=False):
        """epochs x chunks of {gradient, Adam} for every member from ONE library call.  perm: int64 [P, epochs, K*n] — member m's
        minibatches are perm[m, e].chunk(minibatches), indices into ITS samples (i = t*n + e).  stats=True returns f32
        [P, epochs * chunks, 4] (the minibatch means of the pg loss, (v - ret)^2, the entropy and the clip fraction); with an extended
        term on for some member, 8 columns (NativePPO.grad's) and, at the end, the adaptation of ``kl_coef`` where kl_target > 0.

        epochs and / or minibatches may be lists of P ints: member m then runs epochs[m] epochs of its own chunking into minibatches[m]
        (``minibatches_for_size`` turns a minibatch size into a count), still from ONE library call (ssg_pop_update_sched) whose launch
        j serves minibatch j of every member that has one left.  perm is then int64 [P, max(epochs), K*n] (member m reads its first
        epochs[m] rows), the stats f32 [P, n_launches, cols], zero in a member's rows past its own steps, and each member advances
        ``member_steps`` by its own steps.  Either way member m's results are bitwise NativePPO.update's on its shard.

        With slices bound to the env (``set_population_slices``) the update always runs on the schedule path, scalar epochs /
        minibatches broadcast; member m has K * member_envs[m] samples, and perm is a list of P tensors int64 [max(epochs), K * n_m]
        (or the flat buffer they concatenate to, member after member: nothing is padded to the widest member).

        perm=None (needs a perm_seed): the library draws the permutations, ``draw_perm``'s, in whichever of these layouts applies.  Every
        call counts in ``updates``, the key of those draws."""
        if perm is None:
            if self.perm_seed is None:
                raise ValueError("PopulationPPO.update: perm=None needs a perm_seed (PopulationPPO(..., perm_seed=...)); else pass the "
                                 "permutations")
            perm = self.draw_perm(batch, epochs)
        st = self._update(batch, perm, epochs, minibatches, stats)
        self.updates += 1
        return st

    def _update(self, batch, perm, epochs, minibatches, stats=False):
        """update() with the permutations given: on a common schedule (ssg_pop_update / ssg_pop_update_ext), or — a list among epochs /
        minibatches, or slices bound to the env — on per-member schedules (ssg_pop_update_sched)."""
        torch = _torch()
        K, n_env = self._KN(batch)
        P, dev, D = self.n_members, self.population.device, self.population.obs_dim
        self._last_K = K
        sliced = self.env.population_slices is not None
        n = [K * n_m for n_m in self.member_envs] if sliced else K * self.envs_per_member  # samples per member (sliced: P counts)
        sched = sliced or isinstance(epochs, (list, tuple)) or isinstance(minibatches, (list, tuple))
        if sched:
            epochs = [int(e) for e in epochs] if isinstance(epochs, (list, tuple)) else [int(epochs)] * P
            minibatches = [int(b) for b in minibatches] if isinstance(minibatches, (list, tuple)) else [int(minibatches)] * P
            if len(epochs) != P or len(minibatches) != P:
                raise ValueError("PopulationPPO.update: %d epochs and %d minibatches for %d members" % (len(epochs), len(minibatches), P))
            if min(epochs) < 1 or min(minibatches) < 1:
                raise ValueError("PopulationPPO.update: every member's epochs and minibatches must be >= 1")
        who = "PopulationPPO.update"
        p = [self._flat(batch, "obs", torch.float32, (K, n_env, D), who), self._flat(batch, "act", torch.int32, (K, n_env), who),
             self._flat(batch, "logp", torch.float32, (K, n_env), who), self._flat(batch, "adv", torch.float32, (K, n_env), who),
             self._flat(batch, "ret", torch.float32, (K, n_env), who)]
        if sliced and isinstance(perm, (list, tuple)):
            if len(perm) != P or any(tuple(q.shape) != (max(epochs), n[m]) for m, q in enumerate(perm)):
                raise ValueError("PopulationPPO.update: perm must list %d tensors int64 [max(epochs) = %d, K*n_m] with K*n_m = %s"
                                 % (P, max(epochs), n))
            perm = torch.cat([q.to(device=dev, dtype=torch.int64).reshape(-1) for q in perm])
        perm = perm.to(device=dev, dtype=torch.int64).contiguous()
        if sliced:
            if perm.numel() != max(epochs) * sum(n):
                raise ValueError("PopulationPPO.update: the flat perm must hold max(epochs) * sum(K*n_m) = %d indices (got %d)"
                                 % (max(epochs) * sum(n), perm.numel()))
        elif sched:
            if tuple(perm.shape) != (P, max(epochs), n):
                raise ValueError("PopulationPPO.update: perm must be int64 [%d, %d, %d] = [P, max(epochs), K*n] (got %s)"
                                 % (P, max(epochs), n, tuple(perm.shape)))
        elif tuple(perm.shape) != (P, int(epochs), n):
            raise ValueError("PopulationPPO.update: perm must be int64 [%d, %d, %d] (got %s)" % (P, int(epochs), n, tuple(perm.shape)))
        steps0 = self._steps0()
        if sched:  # launches: the longest member's steps; a stats row past a member's own steps stays zero
            table_sched, taken, launches = self.pack_schedule(n, epochs, minibatches)
            self._ws(max(n) if sliced else n, max(chunk_split(n[m] if sliced else n, minibatches[m])[0] for m in range(P)))
            table_steps0 = steps0
        else:
            chunk, n_chunks = chunk_split(n, minibatches)
            launches = int(epochs) * n_chunks
            taken = [launches] * P
            self._ws(n, chunk)
            table_steps0 = steps0 if self.diverged() else None
        extended = self.extended()
        st = None
        if stats:
            st = (torch.zeros if sched else torch.empty)((P, launches, N.PPO_EXT_STATS if extended else 4), dtype=torch.float32, device=dev)
        self._bind_adv_norm()
        table = self._table(launches, table_steps0)
        ext, ext_table = self._ext(batch, K, n_env) if extended else (None, None)  # (ext_table: kept alive until the call is enqueued)
        if sched:
            dev_sched = torch.frombuffer(table_sched, dtype=torch.int32).to(dev)  # (a copy: the host array is free after the call)
            name = "ssg_pop_update_sched"
            args = (C.byref(ext) if extended else None, table.data_ptr(), launches, dev_sched.data_ptr(), (C.c_int32 * P)(*epochs),
                    (C.c_int32 * P)(*minibatches), max(epochs), K, *p, perm.data_ptr())
        else:
            name = "ssg_pop_update_ext" if extended else "ssg_pop_update"
            args = ((C.byref(ext),) if extended else ()) + (table.data_ptr(), launches, K, *p, perm.data_ptr(), int(epochs), int(minibatches))
        self.env.enqueue(name, C.byref(self.population.to_native()), *args, self.adam_mv.data_ptr(), N.ptr(st), *self._ws_ptr())
        self._advance(steps0, taken)
        self._last_taken = [int(t) for t in taken]  # (report(): the rows of `st` each member wrote)
        return st

    # ------------------------------------------------------------------------------------------------
    # the update report (ship_sim_gym_amd/report.py)
    # ------------------------------------------------------------------------------------------------
    def report_device(self, batch, stats=None, post=False):
        """ssg_pop_report over a batch gae() has seen: every member's record, f64 [P, 24] on the device (report.REPORT_FIELDS; member m's
        row is bit for bit NativePPO.report_device's on its shard with its clip and its rows).  Two launches for all members, no
        synchronisation; on equal slices, per-member schedules and unequal slices alike.  stats: the f32 [P, rows, 4 or 8] tensor
        update(..., stats=True) returned; member m's means are taken over the steps IT took in the last update() (the rows past them,
        which a schedule leaves unwritten, are never read).  post=True: the post-update group under every member's parameters as they
        are NOW and its own clip, which costs one ssg_pop_dist launch into a tensor of its own; batch["logp_all"] is left alone."""
        torch = _torch()
        from . import report as R
        K, n_env = self._KN(batch)
        P, dev, D, who = self.n_members, self.population.device, self.population.obs_dim, "PopulationPPO.report"
        p = [self._flat(batch, k, torch.float32, (K, n_env), who) for k in ("val", "ret", "adv")]
        grp = (None, None, None, None)
        if post:
            act, logp = self._flat(batch, "act", torch.int32, (K, n_env), who), self._flat(batch, "logp", torch.float32, (K, n_env), who)
            self._flat(batch, "obs", torch.float32, (K, n_env, D), who)
            new = self.dist({"rew": batch["rew"], "obs": batch["obs"]})  # (a dict of its own: the batch's logp_all stays the acting policy's)
            bounds = torch.tensor([[float(x) for x in R.clip_bounds(c)] for c in self.clip], dtype=torch.float32).to(dev)
            grp = (act, logp, new.data_ptr(), bounds.data_ptr())
        sp = rows = None
        rows_max = cols = 0
        if stats is not None:
            if stats.dim() != 3:
                raise ValueError("PopulationPPO.report: stats must be [%d, rows, 4 or 8] (update(..., stats=True); got %s)" % (P, tuple(stats.shape)))
            sp = N.arg(stats, torch.float32, (P,) + tuple(stats.shape[1:]), "PopulationPPO.report: stats", dev)  # (P is what is judged)
            rows_max, cols = int(stats.shape[1]), int(stats.shape[2])
            taken = self._last_taken or [rows_max] * P
            rows = torch.tensor([min(int(t), rows_max) for t in taken], dtype=torch.int32).to(dev)
        out = torch.empty((P, N.REPORT_COLS), dtype=torch.float64, device=dev)
        self.env.enqueue("ssg_pop_report", P, K, *p, *grp, sp, rows_max, cols, N.ptr(rows), *self._report_ws(n_env, P), out.data_ptr())
        return out

    def report(self, batch, stats=None, post=False):
        """report_device's records as a dict of numpy arrays [P] (report.REPORT_FIELDS), plus ``lr``, ``clip``, ``step`` (the members'
        Adam steps), ``updates`` and ``kl_coef_now`` (the device's coefficients, read with the same copy): ONE device-to-host copy."""
        torch = _torch()
        import numpy as np
        from .report import REPORT_FIELDS
        out = torch.cat([self.report_device(batch, stats, post), self.kl_coef.to(torch.float64).view(-1, 1)], dim=1).cpu().numpy()
        rec = {k: out[:, i].copy() for i, k in enumerate(REPORT_FIELDS)}
        rec.update(lr=np.array(self.lr, dtype=np.float64), clip=np.array(self.clip, dtype=np.float64),
                   step=np.array(self._steps0(), dtype=np.int64), updates=int(self.updates), kl_coef_now=out[:, N.REPORT_COLS].copy())
        return rec

    def exploit(self, src):
        """PBT's exploit on the device: member m takes the parameters and Adam moments of member src[m] (src[m] == m keeps).  A source
        must not itself be a destination.  The source's ``kl_coef`` travels with its parameters: the coefficient was adapted to THOSE
        parameters (to how far their updates move the distribution), so it belongs to the weights, not to the scheduler's
        hyper-parameters.  Those are the scheduler's business (PBTScheduler returns the new lists).  So does the source's Adam step
        count (``member_steps``): the bias correction belongs to the moments that are copied.  With an observation filter bound to
        the env (``env.set_obs_filter``), the source's filter rows travel too: an exploited member must not keep statistics its new
        weights were never trained on.  So do the state rows of a return filter registered with ``set_return_filter``: the source's
        value head was trained on rewards at the source's scale.  That filter's carries are per env and stay."""
        torch = _torch()
        src = [int(s) for s in src]
        if len(src) != self.n_members:
            raise ValueError("PopulationPPO.exploit: src has %d entries for %d members" % (len(src), self.n_members))
        arr = (C.c_int32 * len(src))(*src)
        flt = getattr(self.env, "obs_filter", None)
        if flt is not None and flt.n_members != self.n_members:  # (judged before anything is copied)
            raise ValueError("PopulationPPO.exploit: the env's observation filter has %d members, the population %d"
                             % (flt.n_members, self.n_members))
        self.env.enqueue("ssg_pop_exploit", C.byref(self.population.to_native()), arr, self.adam_mv.data_ptr())
        with torch.cuda.device(self.population.device):
            self.kl_coef.copy_(self.kl_coef[torch.tensor(src, device=self.population.device)])
            if flt is not None:  # (an indexed copy on the handle's stream; the gather is materialised before the copy writes)
                flt.state.copy_(flt.state[torch.tensor(src, device=flt.state.device)])
            if self.return_filter is not None:
                rf = self.return_filter
                rf.state.copy_(rf.state[torch.tensor(src, device=rf.state.device)])
        steps0 = self._steps0()
        self._advance([steps0[s] for s in src], [0] * self.n_members)

    def reset_episode_carry(self):
        """Forget the running episodes (call after an env reset)."""
        self.carry_return.zero_()
        self.carry_length.zero_()

    def episode_stats(self, batch):
        """int64 [P, 3] device tensor: per member (100 * sum of returns, sum of lengths, episodes) of the episodes that ENDED in this
        rollout batch; episodes spanning batches are carried and counted once, at their end.  The carries are per env: after a
        re-slice an episode in flight is credited to whichever member owns the env when it ends."""
        torch = _torch()
        K, n_env = self._KN(batch)
        who = "PopulationPPO.episode_stats"
        rew, done = self._flat(batch, "rew", torch.float64, (K, n_env), who), self._flat(batch, "done", torch.uint8, (K, n_env), who)
        out = torch.zeros((self.n_members, 3), dtype=torch.int64, device=self.population.device)
        self.env.enqueue("ssg_pop_episode_stats", self.n_members, K, rew, done, self.carry_return.data_ptr(), self.carry_length.data_ptr(),
                         out.data_ptr())
        return out

    # ------------------------------------------------------------------------------------------------
    # state (ship_sim_gym_amd/checkpoint.py)
    # ------------------------------------------------------------------------------------------------
    def state_dict(self):
        """What the next update depends on besides the population and the batch (CPU copies; plain data only): the Adam moments
        [P, 2L], ``step``, ``member_steps``, ``updates``, ``kl_coef`` [P], every per-member hyper-parameter list (HPARAM_KEYS and
        EXT_KEYS), ``adv_norm``, ``perm_seed`` (with ``has_perm_seed``: the state holds no None), the episode carries, ``last_K``, the
        hyper-parameter ``schedules`` ({"lr": P entries, ...}: a member's points, an empty list for a constant) and the clocks ``timesteps``.

        Not state: the workspace (gae() rewrites the statistics at its head before update() reads them, and a checkpoint is taken
        between an update and the next rollout), the per-minibatch scratch, and the env's slices, which belong to the layout the
        caller binds.  A ``ReturnFilter`` registered with ``set_return_filter`` is saved by its owner, not here."""
        sd = {"n_members": self.n_members, "adam_mv": self.adam_mv.detach().cpu().clone(), "step": int(self.step),
              "member_steps": [int(s) for s in self.member_steps], "updates": int(self.updates),
              "kl_coef": self.kl_coef.detach().cpu().clone(), "adv_norm": self.adv_norm,
              "has_perm_seed": self.perm_seed is not None, "perm_seed": int(self.perm_seed or 0),
              "carry_return": self.carry_return.detach().cpu().clone(), "carry_length": self.carry_length.detach().cpu().clone(),
              "last_K": int(self._last_K)}
        for k in HPARAM_KEYS + EXT_KEYS:
            sd[k] = [float(v) for v in getattr(self, k)]
        sd["schedules"] = {k: [HS.entry_state(s) for s in self.schedules[k]] for k in HS.SCHEDULABLE}
        sd["timesteps"] = [int(t) for t in self.timesteps]
        return sd

    def load_state_dict(self, sd):
        """Become the trainer the state was taken from.  Checked first, all of it: the member count, ``adv_norm`` (the mode and its
        scratch are made at construction), every tensor's shape and dtype, every list's length.  A mismatch raises ValueError naming
        the field with both values and leaves this object as it was.  The hyper-parameter schedules and their clocks are taken over
        like the hyper-parameters; a state without ``schedules`` and ``timesteps`` is a constant run's."""
        from .checkpoint import check_state, check_values
        who, P = "PopulationPPO.load_state_dict", self.n_members
        check_state(who, sd, [("n_members", P), ("adv_norm", self.adv_norm)],
                    [("adam_mv", self.adam_mv), ("kl_coef", self.kl_coef), ("carry_return", self.carry_return),
                     ("carry_length", self.carry_length)])
        lists = ("member_steps",) + HPARAM_KEYS + EXT_KEYS
        check_values(who, sd, [("step", int), ("updates", int), ("has_perm_seed", bool), ("perm_seed", int), ("last_K", int)]
                     + [(k, list) for k in lists])
        bad = ["%s lists %d values in the state, this object has %d members" % (k, len(sd[k]), P) for k in lists if len(sd[k]) != P]
        bad += ["%s holds %r" % (k, v) for k in lists for v in sd[k] if isinstance(v, bool) or not isinstance(v, (int, float))]
        if bad:
            raise ValueError("%s: %s" % (who, "; ".join(bad)))
        schedules, timesteps = {k: [None] * P for k in HS.SCHEDULABLE}, [0] * P
        if "schedules" in sd or "timesteps" in sd:
            check_values(who, sd, [("schedules", dict), ("timesteps", list)])
            check_values(who + ": schedules", sd["schedules"], [(k, list) for k in HS.SCHEDULABLE])
            for k in HS.SCHEDULABLE + ("timesteps",):
                n = len(sd[k] if k == "timesteps" else sd["schedules"][k])
                if n != P:
                    raise ValueError("%s: %s lists %d entries in the state, this object has %d members" % (who, k, n, P))
            schedules = {k: [HS.entry_from_state("%s: member %d" % (who, m), k, e) for m, e in enumerate(sd["schedules"][k])]
                         for k in HS.SCHEDULABLE}
            timesteps = [HS.check_clock(who, t) for t in sd["timesteps"]]
        for name in ("adam_mv", "kl_coef", "carry_return", "carry_length"):
            getattr(self, name).copy_(sd[name])
        self.step, self.updates, self._last_K = int(sd["step"]), int(sd["updates"]), int(sd["last_K"])
        self.member_steps = [int(s) for s in sd["member_steps"]]
        self.perm_seed = int(sd["perm_seed"]) if sd["has_perm_seed"] else None
        for k in HPARAM_KEYS + EXT_KEYS:
            setattr(self, k, [float(v) for v in sd[k]])
        self.schedules, self.timesteps = schedules, timesteps
        return self


# ------------------------------------------------------------------------------------------------------------------------------------
# the scheduler (host only)
# ------------------------------------------------------------------------------------------------------------------------------------
LR_CHOICES = [1e-3, 5e-4, 1e-4, 5e-5, 1e-5]


def slices_for_batch_sizes(batch_sizes, n_envs, quantum=64):
    """Slice sizes (P ints summing to n_envs, each a multiple of `quantum`) for members that ask for `batch_sizes` samples per update.

    The handle's K * n_envs samples per update are fixed, so a member's train_batch_size is its SHARE of them, not an absolute
    count: two populations with batch sizes (1, 2) and (10000, 20000) get the same slices.  Deterministic apportionment: n_envs must be
    a multiple of quantum and hold at least one quantum per member; every member gets one quantum, and the remaining quanta are dealt
    by largest remainder in proportion to batch_sizes (ties to the lower index), so no member ends more than one quantum away from
    its exact proportional share of them."""
    sizes = [b if isinstance(b, int) else float(b) for b in batch_sizes]
    P, n_envs, quantum = len(sizes), int(n_envs), int(quantum)
    if P < 1 or quantum < 1 or n_envs < 1:
        raise ValueError("slices_for_batch_sizes: at least one member, quantum >= 1 and n_envs >= 1")
    if any(not (b > 0.0) or b == float("inf") for b in sizes):
        raise ValueError("slices_for_batch_sizes: every batch size must be a positive finite number")
    if n_envs % quantum:
        raise ValueError("slices_for_batch_sizes: n_envs = %d is not a multiple of the quantum %d" % (n_envs, quantum))
    rest = n_envs // quantum - P
    if rest < 0:
        raise ValueError("slices_for_batch_sizes: %d envs hold fewer than one quantum of %d per member (%d members)" % (n_envs, quantum, P))
    sizes = [Fraction(b) for b in sizes]  # (exact, also for floats: the remainders are compared without rounding)
    total = sum(sizes)
    exact = [rest * b / total for b in sizes]
    whole = [int(math.floor(x)) for x in exact]
    order = sorted(range(P), key=lambda m: (-(exact[m] - whole[m]), m))
    for m in order[:rest - sum(whole)]:
        whole[m] += 1
    return [quantum * (1 + w) for w in whole]


def reference_mutations(schedule=False, batch=False):
    """The reference's mutated hyper-parameters (train/rllib/pbt.py:34-42) that can vary per member here: a callable draws a fresh
    value from the generator it is handed; a list is a set of choices.  By default the three that leave the launches alone;
    schedule=True appends the two that set a member's update schedule, num_sgd_iter and sgd_minibatch_size (pbt.py:40-41), which
    ``PopulationPPO.update`` takes per member; batch=True the sixth, train_batch_size (pbt.py:42), which becomes the member's share of
    the handle's envs (``slices_for_batch_sizes``)."""
    out = {
        "lambda": lambda rng: rng.uniform(0.9, 1.0),
        "clip_param": lambda rng: rng.uniform(0.01, 0.5),
        "lr": list(LR_CHOICES),
    }
    if schedule:
        out["num_sgd_iter"] = lambda rng: rng.randint(1, 30)
        out["sgd_minibatch_size"] = lambda rng: rng.randint(128, 16384)
    if batch:
        out["train_batch_size"] = lambda rng: rng.randint(2000, 160000)
    return out


class PBTScheduler(object):
    """ray 0.6's PopulationBasedTraining as train/rllib/pbt.py:29-43 configures it, for a population that trains in lockstep.

    Every `perturbation_interval` UPDATES (the reference counts 600 s of wall time; a lockstep population has no per-trial clock) the
    members are ranked by score.  Each member of the bottom quantile (ceil(P * quantile_fraction), at most P // 2) picks a random member of the
    top quantile as its source and takes that member's hyper-parameters, then explores: for each mutated key, with probability
    `resample_probability` the value is redrawn from the key's generator / list; otherwise a continuous value is multiplied by 1.2 or
    0.8 and a list-valued one steps to the neighbouring entry (staying at an end of the list, as ray clamps it; a value that is not in
    the list is redrawn).  As in ray, a perturbed continuous value is not clamped to the generator's range.  An int stays an int:
    the perturbed value is int(old * 1.2) or int(old * 0.8), truncated — what ray 0.6's explore() does for int-valued entries as far as
    its source is remembered (ray is not installed alongside this project, so that was not checked against it); a resample returns
    whatever the generator returns.
    """

    def __init__(self, n_members, seed=0, perturbation_interval=1, quantile_fraction=0.25, resample_probability=0.33, mutations=None):
        if n_members < 1:
            raise ValueError("PBTScheduler: n_members must be >= 1")
        if perturbation_interval < 1:
            raise ValueError("PBTScheduler: perturbation_interval must be >= 1 (updates)")
        if not 0.0 <= quantile_fraction <= 0.5:
            raise ValueError("PBTScheduler: quantile_fraction must be in [0, 0.5]")
        self.n_members, self.interval = int(n_members), int(perturbation_interval)
        self.quantile_fraction, self.resample_probability = float(quantile_fraction), float(resample_probability)
        self.mutations = reference_mutations() if mutations is None else dict(mutations)
        self.rng = random.Random(seed)

    def due(self, update):
        """True after update number `update` (1, 2, ...) when a perturbation is due."""
        return update > 0 and update % self.interval == 0

    def _arguments(self):
        """The constructor's arguments as plain data, as (name, value) pairs; a mutation that is a list is its values, one that draws
        from the generator is the string "callable" (a function is not data: the scheduler that loads a state brings its own)."""
        return [("n_members", self.n_members), ("perturbation_interval", self.interval), ("quantile_fraction", self.quantile_fraction),
                ("resample_probability", self.resample_probability),
                ("mutations", {str(k): (list(d) if isinstance(d, list) else "callable") for k, d in self.mutations.items()})]

    def state_dict(self):
        """The constructor's arguments and the generator's state, as plain data (ints, floats, strings, lists, dicts: no tuple, no
        torch).  ``due`` reads the interval and the caller's update number, ``perturb`` the generator and its arguments: the scheduler
        keeps no counter of its own, so this is all of it.  After ``load_state_dict`` the next ``perturb(scores, hparams)`` returns
        what the original's next call returns."""
        version, internal, gauss = self.rng.getstate()
        sd = dict(self._arguments())
        sd["rng"] = {"version": int(version), "state": [int(x) for x in internal], "gauss_next": [] if gauss is None else [float(gauss)]}
        return sd

    def load_state_dict(self, sd):
        """Take a state_dict's generator state.  The constructor's arguments must be the state's (a mutated key's list too; a key that
        draws from the generator must be one here as well): ValueError otherwise, naming the field with both values, and nothing
        changes."""
        if not isinstance(sd, dict):
            raise ValueError("PBTScheduler.load_state_dict: a state dict is a dict (got a %s)" % type(sd).__name__)
        bad = ["%s is %r in the state and %r in this object" % (k, sd.get(k, "missing"), v) for k, v in self._arguments() if sd.get(k, None) != v]
        rng = sd.get("rng")
        ok = isinstance(rng, dict) and isinstance(rng.get("version"), int) and isinstance(rng.get("state"), list) and \
            all(isinstance(x, int) for x in rng["state"]) and isinstance(rng.get("gauss_next"), list) and len(rng["gauss_next"]) <= 1
        if not ok:
            bad.append("rng must hold version (int), state (a list of ints) and gauss_next (a list of at most one float)")
        if bad:
            raise ValueError("PBTScheduler.load_state_dict: " + "; ".join(bad))
        probe = random.Random()
        try:  # (a state of the wrong length or version is refused by the generator itself: try it on a scratch one first)
            probe.setstate((rng["version"], tuple(rng["state"]), rng["gauss_next"][0] if rng["gauss_next"] else None))
        except (TypeError, ValueError) as ex:
            raise ValueError("PBTScheduler.load_state_dict: rng is no generator state (%s)" % ex)
        self.rng.setstate(probe.getstate())
        return self

    def quantiles(self, scores):
        """(bottom, top): member indices of the lowest / highest scoring quantile (ties broken by index; disjoint)."""
        order = sorted(range(self.n_members), key=lambda m: (scores[m], m))
        if len(order) <= 1:
            return [], []
        k = int(math.ceil(len(order) * self.quantile_fraction))
        k = min(k, len(order) // 2)
        return (order[:k], order[-k:]) if k else ([], [])

    def explore(self, values):
        """One member's new {key: value} from its source's values; returns (new values, [(key, kind, old, new)])."""
        new, log = dict(values), []
        for key, dist in self.mutations.items():
            old = values[key]
            if isinstance(dist, list):
                if self.rng.random() < self.resample_probability or old not in dist:
                    new[key], kind = self.rng.choice(dist), "resample"
                elif self.rng.random() > 0.5:
                    new[key], kind = dist[max(0, dist.index(old) - 1)], "perturb"
                else:
                    new[key], kind = dist[min(len(dist) - 1, dist.index(old) + 1)], "perturb"
            else:
                if self.rng.random() < self.resample_probability:
                    new[key], kind = dist(self.rng), "resample"
                elif self.rng.random() > 0.5:
                    new[key], kind = int(old * 1.2) if isinstance(old, int) else old * 1.2, "perturb"
                else:
                    new[key], kind = int(old * 0.8) if isinstance(old, int) else old * 0.8, "perturb"
            log.append((key, kind, old, new[key]))
        return new, log

    def perturb(self, scores, hparams):
        """scores: P numbers (higher is better); hparams: {key: list of P values} holding at least the mutated keys.  Returns
        (src, new_hparams, events): src[m] = the member whose weights m takes (m itself = keep), for ``PopulationPPO.exploit``; the new
        lists (copies; only destinations change); events = [{"member", "source", "mutations": [(key, kind, old, new)]}]."""
        if len(scores) != self.n_members:
            raise ValueError("PBTScheduler.perturb: %d scores for %d members" % (len(scores), self.n_members))
        for key in self.mutations:
            if key not in hparams or len(hparams[key]) != self.n_members:
                raise ValueError("PBTScheduler.perturb: hparams[%r] must list %d values" % (key, self.n_members))
        bottom, top = self.quantiles(scores)
        src = list(range(self.n_members))
        new = {k: list(v) for k, v in hparams.items()}
        events = []
        for m in bottom:
            s = self.rng.choice(top)
            values, log = self.explore({k: hparams[k][s] for k in self.mutations})
            src[m] = s
            for k in hparams:  # the source's whole configuration, then the explored keys
                new[k][m] = values[k] if k in values else hparams[k][s]
            events.append({"member": m, "source": s, "mutations": log})
        return src, new, events
