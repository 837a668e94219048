"""ShipVecEnv — the batched, MI355X-resident ShipEnv.

Keeps the reference's gym surface (ship_gym/ship_env.py:16-184: ``action_space = Discrete(3)``,
``observation_space = Box(0, max(bounds), (n_states*H,), uint8)``, ``reset()``, ``step()``) but for N envs at
once, and speaks the two vector-env protocols the reference's trainers use:

* stable-baselines 2.2.0 ``VecEnv`` (train/stable_baselines/ppo.py:122-123 builds a SubprocVecEnv): ``num_envs``,
  ``reset() -> obs[N,D]``, ``step_async(actions)``, ``step_wait() -> (obs, rews, dones, infos)``, ``step``,
  ``close``; a done env is reset inside the step and its returned observation is the reset observation.
* RLlib 0.6.0 ``VectorEnv`` (train/rllib/ppo.py:21-24,43): ``vector_reset()``, ``reset_at(i)``,
  ``vector_step(actions)``, ``get_unwrapped()``.

State for all envs lives in one caller-owned torch-ROCm byte tensor (struct-of-arrays columns, see
include/shipsim.h); PyTorch is only the device-buffer container and stream provider.  All compute goes through
libshipsim.so; there is no CPU path.

Two map modes:
* ``"bank"`` (default): a fixed bank of ``n_maps`` pre-generated worlds lives in HBM (and is staged in LDS by
  the kernel); env e starts on map ``(env_id_base+e) % n_maps`` and every in-kernel auto-reset moves it to the
  next map.  No host involvement per step.
* ``"fresh"``: reference-exact resets — every reset draws a brand-new world from the global ``random`` /
  ``np.random`` streams on the host (game.py:260-277), one bank slot per env.  Needs a host round trip on done.
* ``"fresh_device"``: a brand-new world for EVERY episode of every env, like the reference (ShipGame.reset generates a
  river and a goal path at every reset), but at batch scale and without the host: env e owns a ring of ``ring``
  bank records, episode p lives in record ``e*ring + p % ring`` and is drawn on the device from a Philox stream keyed
  by (map_seed, global env id, p) (ssg_config.map_ring / ssg_refill_worlds).  The in-kernel auto-reset moves an env
  to its next record; the library refills the rings between launches.  Not seed-compatible with the reference's
  Mersenne-Twister draws (use ``"fresh"`` for that); same geometry code as the host path, bit for bit.
"""
import ctypes as C
import inspect
import math
import warnings

import numpy as np

from . import _native as N
from . import config as cfgmod
from . import spaces, worldgen
from ._native import _torch


def _trainer_bases():
    """Base classes for ShipVecEnv: the trainers' own abstract vector-env classes when they are importable, so that
    PPO2's `isinstance(env, VecEnv)` (stable-baselines, train/stable_baselines/ppo.py:88,122-123) and RLlib's
    `isinstance(env, VectorEnv)` (train/rllib/ppo.py:21-24,43) gates accept the batched env; `object` otherwise."""
    bases = []
    for mod, name in (("stable_baselines.common.vec_env", "VecEnv"), ("stable_baselines3.common.vec_env", "VecEnv"),
                      ("ray.rllib.env.vector_env", "VectorEnv")):
        if mod.startswith("stable_baselines3") and bases:
            continue  # one VecEnv flavour is enough
        try:
            cls = getattr(__import__(mod, fromlist=[name]), name)
        except Exception:
            continue
        if isinstance(cls, type) and cls not in bases:
            bases.append(cls)
    return tuple(bases) or (object,)


_BASES = _trainer_bases()


def native_config(num_envs, game_config, env_config, device_index, map_mode="bank", env_id_base=0, auto_reset=True, n_beams=None,
                  fix_collision_reward=False, bank_in_global=False, exact_lidar=False, n_ships=1, rllib=False, ring=32, dyn_memo=True):
    """(ssg_config, auto_reset, rllib_fused) of a ShipVecEnv, from its constructor's arguments alone.

    rllib_fused: the RLlib flow WITHOUT a reset launch (ssg_set_terminal_obs, history <= 2, worlds that live on the device): the step
    kernel resets a done env itself — its row of `obs` is then the reset observation reset_at(i) hands out — and also stores the env's
    TERMINAL observation in `term_obs`, which vector_step reports.  Otherwise (history > 2, host-drawn worlds) the rllib flow runs
    without in-kernel reset and resets its done envs with ONE masked ssg_reset per step."""
    if map_mode not in ("bank", "fresh", "fresh_device"):
        raise ValueError("map_mode must be 'bank', 'fresh' or 'fresh_device'")
    on_device = map_mode in ("bank", "fresh_device")
    rllib_fused = bool(rllib) and env_config.HISTORY_SIZE <= 2 and on_device
    auto_reset = bool(auto_reset) and (not rllib or rllib_fused)
    bounds = tuple(game_config.BOUNDS)
    c = N.default_config()
    c.device_id = int(device_index)
    c.n_envs = int(num_envs)
    c.env_id_base = int(env_id_base)
    if n_beams is None:
        if getattr(env_config, "USE_LIDAR_CONFIG", False):
            lc = env_config.LIDAR_CONFIG
            c.n_beams, c.lidar_spread_deg, c.lidar_dist = lc.N_BEAMS, lc.ANGULAR_SPREAD, lc.DISTANCE
        else:  # the reference ignores LidarConfig: LiDAR() defaults (models.py:29,150)
            c.n_beams = cfgmod.LIDAR_DEFAULT_N_BEAMS
    else:
        c.n_beams = int(n_beams)
    c.history = int(env_config.HISTORY_SIZE)
    c.max_steps = int(env_config.MAX_STEPS)
    c.n_goals = cfgmod.N_GOALS
    c.width, c.height = float(bounds[0]), float(bounds[1])
    c.dt = game_config.SPEED * cfgmod.BASE_DT                 # game.py:194: speed * base_dt
    c.damping_pow_dt = math.pow(cfgmod.SPACE_DAMPING, c.dt)   # cpSpaceStep: pow(space.damping, dt)
    c.spawn_x, c.spawn_y = bounds[0] / 2, 25.0                # game.py:274
    flags = 0
    if auto_reset and on_device:
        flags |= N.FLAG_AUTO_RESET
    if fix_collision_reward:
        flags |= N.FLAG_FIX_COLLISION_REWARD
    if bank_in_global or map_mode == "fresh":
        flags |= N.FLAG_BANK_IN_GLOBAL
    if exact_lidar:
        flags |= N.FLAG_EXACT_LIDAR
    if not dyn_memo:  # config 4 measurement aid: every queued env computes its cpSpaceStep (no memo table look-ups)
        flags |= N.FLAG_DYN_MEMO_OFF
    c.flags = flags
    # n_ships = 4: BASELINE configs[3] — env.game.add_default_traffic() (game.py:279-286) after every reset: three
    # traffic ships, dynamic goal bodies and Chipmunk's contact solver (csrc/shipsim_dynamics.hip)
    c.n_ships = int(n_ships)
    c.map_ring = int(ring) if map_mode == "fresh_device" else 0
    return c, auto_reset, rllib_fused


class EnvHandle(object):
    """One env of a ShipVecEnv, for the per-env calls of the trainers' APIs (`env_method`, `get_attr`, `set_attr`,
    RLlib's `get_unwrapped()`): attribute reads fall through to the batch, `reset()`/`seed()`/`render()` act on
    this env only."""

    def __init__(self, vec, index):
        object.__setattr__(self, "_vec", vec)
        object.__setattr__(self, "index", int(index))
        object.__setattr__(self, "_attrs", {})

    def __getattr__(self, name):
        attrs = object.__getattribute__(self, "_attrs")
        if name in attrs:
            return attrs[name]
        return getattr(object.__getattribute__(self, "_vec"), name)

    def __setattr__(self, name, value):
        self._attrs[name] = value

    def reset(self):
        return self._vec.reset_at(self.index)

    def seed(self, seed=None):
        return self._vec.seed(seed)

    def render(self, mode='human', close=False):
        return self._vec.render(mode=mode, close=close, env=self.index)

    def close(self):
        return None


class ShipVecEnv(*_BASES):
    metadata = {'render.modes': ['human', 'rgb_array']}  # ship_env.py:18
    reward_range = (-1, 1)                                # ship_env.py:20

    def __init__(self, num_envs, game_config=None, env_config=None, device="cuda:0", map_mode="bank", n_maps=64,
                 map_seed=1000, width_frac=0.5, env_id_base=0, auto_reset=True, n_beams=None, bank=None,
                 fix_collision_reward=False, bank_in_global=False, exact_lidar=False, n_ships=1, rllib=False, ring=32,
                 dyn_memo=True, host_slots=4, copy_host_outputs=False):
        torch = _torch()
        if not torch.cuda.is_available():
            raise N.ShipSimError("ShipVecEnv needs a HIP device (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        game_config = game_config if game_config is not None else cfgmod.GameConfig
        env_config = env_config if env_config is not None else cfgmod.EnvConfig
        if env_config.HISTORY_SIZE < 1:  # ship_env.py:46-47
            raise ValueError("history_size must be greater than zero")
        self.num_envs = int(num_envs)
        self._i32, self._cur_stream = torch.int32, torch.cuda.current_stream
        dev = torch.device(device)
        self._dev_index = dev.index if dev.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", self._dev_index)  # (always with its index: tensors report `cuda:N`)
        self.map_mode = map_mode
        self.bounds = tuple(game_config.BOUNDS)
        self.width_frac = float(width_frac)
        # rllib=True: the RLlib VectorEnv flow — vector_step returns the TERMINAL observation of a done env and the
        # caller's reset_at(i) is the one reset it gets (no in-kernel auto-reset underneath, or the fused flow of native_config)
        self.rllib = bool(rllib)
        self.cfg, self.auto_reset, self._rllib_fused = native_config(
            num_envs, game_config, env_config, self._dev_index, map_mode=map_mode, env_id_base=env_id_base, auto_reset=auto_reset,
            n_beams=n_beams, fix_collision_reward=fix_collision_reward, bank_in_global=bank_in_global, exact_lidar=exact_lidar,
            n_ships=n_ships, rllib=rllib, ring=ring, dyn_memo=dyn_memo)
        self.env_id_base, self.n_ships, self.ring = int(env_id_base), int(n_ships), int(self.cfg.map_ring)
        self.game_config, self.env_config = game_config, env_config
        self.n_states = 6 + self.cfg.n_beams                       # ship_env.py:43
        self.states_history = self.n_states * self.cfg.history     # ship_env.py:44
        self.action_space = spaces.Discrete(3)                     # ship_env.py:19
        self.observation_space = spaces.Box(low=0, high=max(self.bounds), shape=(self.states_history,),
                                            dtype=np.uint8)       # ship_env.py:48 (declared uint8; obs are float64)
        self.host_slots = max(2, min(8, int(host_slots)))  # (ssg_step_host has eight completion-event slots)
        self.copy_host_outputs = bool(copy_host_outputs)
        # everything else a ShipVecEnv holds, in its initial state
        self._host = None  # pinned host side of the numpy protocols, made by the first step_async (the tensor API never needs it)
        self.term_obs = None            # enable_terminal_obs
        self._traj_plans = {}           # rollout_tensor(trajectory=True, out=...): launch plans by the obs buffer's address
        self._pop_slices = None         # set_population_slices: (sizes, device table)
        self._timeout_boot = None       # set_timeout_bootstrap: {"term_obs", "boot"}
        self._obs_filter = None         # set_obs_filter
        self._adv_norm_scratch = None   # set_adv_norm
        self._adv_table = None          # set_adv_table
        self._full_reset_done = False   # reset_tensor(mask=None) has run (the handle's first full reset zeroes the blob)
        self._pending = None
        self._closed = False
        self._handles = {}
        self._await_reset = np.zeros(self.num_envs, dtype=bool)  # rllib flow: done envs already re-initialised
        self._reset_obs_h = None
        self._create_handle()
        self._first_bank(bank, n_maps, map_seed)
        if self._rllib_fused:
            self.enable_terminal_obs()
        self._call_base_ctors()

    def _create_handle(self):
        """ssg_create, then the two device blocks: the state blob (bound) and the output block, whose addresses `_out` keeps."""
        torch = _torch()
        self._lib = N.lib()
        self._h = C.c_void_p()
        N.call("ssg_create", C.byref(self.cfg), C.byref(self._h))
        nbytes = C.c_size_t()
        self.call("ssg_state_nbytes", C.byref(nbytes))
        # obs | reward | done | flags are views of ONE device block (256-byte aligned sections), so that the numpy protocols
        # (SB VecEnv / RLlib VectorEnv) bring a whole step to the host with ONE device -> host copy into a pinned block
        n_, D_ = self.num_envs, self.states_history
        up = lambda v: (v + 255) // 256 * 256
        self._o_obs, self._o_rew = 0, up(n_ * D_ * 8)
        self._o_done = self._o_rew + up(n_ * 8)
        self._o_flags = self._o_done + up(n_)
        self._out_nbytes = self._o_flags + up(n_)
        self.state = torch.zeros(nbytes.value, dtype=torch.uint8, device=self.device)
        self._out_blob = torch.zeros(self._out_nbytes, dtype=torch.uint8, device=self.device)
        self.obs, self.reward, self.done, self.flags = self._blob_views(self._out_blob)
        self._actions = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        # the four output addresses as plain integers, for the launch path: the block is allocated once and only ever copied into
        self._out = tuple(t.data_ptr() for t in (self.obs, self.reward, self.done, self.flags))
        self.call("ssg_bind_state", self.state.data_ptr())

    def _first_bank(self, bank, n_maps, map_seed):
        """The constructor's map bank, per map mode."""
        torch = _torch()
        self.bank_polys = self.bank_goals = None
        if self.map_mode == "bank":
            if bank is None:
                bank, self.bank_polys, self.bank_goals = worldgen.build_bank(
                    n_maps, self.bounds, n_goals=self.cfg.n_goals, width_frac=self.width_frac, seed=map_seed)
            self.set_bank(bank)
        elif self.map_mode == "fresh":
            # reference-exact: ShipGame.__init__ ends with self.reset() (game.py:58), so constructing an env already
            # consumes one world's worth of RNG; the user's reset() draws another (App. B-17).
            self.bank_host = np.zeros((self.num_envs, N.MAP_STRIDE), dtype=np.float64)
            self.worlds = [None] * self.num_envs
            for e in range(self.num_envs):
                self._fresh_world(e)
            self.set_bank(self.bank_host)
        else:
            bank = torch.zeros((self.num_envs * self.ring, N.MAP_STRIDE), dtype=torch.float64, device=self.device)
            self.map_seed = int(map_seed)
            self.set_bank(bank)
            self.refill_worlds(self.map_seed)  # fills every ring: episodes 0 .. ring-1 of every env

    def _call_base_ctors(self):
        """The trainers' base-class constructors.  stable-baselines declares VecEnv.__init__(num_envs, observation_space,
        action_space), ray >= 1.x VectorEnv.__init__(observation_space, action_space, num_envs), ray 0.6 (the reference's
        pin) none: each is called with the KEYWORDS its signature names, never positionally, and our own attributes are
        re-asserted afterwards so that no base can have swapped them."""
        mine = {"num_envs": self.num_envs, "observation_space": self.observation_space, "action_space": self.action_space}
        # (the bases of ShipVecEnv itself, not of type(self): for a subclass the latter would list ShipVecEnv and re-enter
        # this constructor)
        for base in ShipVecEnv.__mro__[1:]:
            if base is object or "__init__" not in vars(base):
                continue
            try:
                params = inspect.signature(base.__init__).parameters
                base.__init__(self, **{k: v for k, v in mine.items() if k in params})
            except TypeError as ex:  # a signature this dispatch does not know: say so, keep our own attributes
                warnings.warn("ShipVecEnv: %s.__init__ not called (%s)" % (base.__name__, ex))
        self.num_envs, self.observation_space, self.action_space = mine["num_envs"], mine["observation_space"], mine["action_space"]

    @classmethod
    def from_env_fns(cls, env_fns, **kw):
        """SubprocVecEnv-shaped constructor (train/stable_baselines/ppo.py:122-123: ``SubprocVecEnv([make_env() for i in
        range(num_cpu)])``): one batched env of ``len(env_fns)`` envs instead of one OS process per env.  The first
        thunk is called once to learn the (game_config, env_config) the caller's ``ShipEnv(...)`` line passes."""
        env_fns = list(env_fns)
        if not env_fns:
            raise ValueError("need at least one env thunk")
        probe = env_fns[0]()
        gc, ec = getattr(probe, "game_config", None), getattr(probe, "env_config", None)
        extra = dict(getattr(probe, "_ctor_kw", {}))
        try:
            probe.close()
        except Exception:
            pass
        extra.update(kw)
        return cls(len(env_fns), gc, ec, **extra)

    # ------------------------------------------------------------------------------------------------
    def _stream(self):
        """The current stream's handle on this env's device, a plain integer."""
        return self._cur_stream(self.device).cuda_stream

    def _arg(self, t, dtypes, shape, what, more_rows=False, exc=ValueError):
        """N.arg, THE check of a tensor argument, on this env's device: the tensor's address, or `exc`."""
        return N.arg(t, dtypes, shape, what, self.device, more_rows, exc)

    def call(self, name, *args):
        """THE checked call of a host-only entry point (a setter, a getter): `name`(handle, *args) with this env's device current."""
        with _torch().cuda.device(self.device):
            N.call(name, self._h, *args, handle=self._h)

    def enqueue(self, name, *args):
        """THE checked call of an entry point that launches: ``call`` with the current stream's handle as the last argument."""
        with _torch().cuda.device(self.device):
            N.call(name, self._h, *args, self._cur_stream(self.device).cuda_stream, handle=self._h)

    def _launch(self, what, fn, *args):
        """The step path's form of ``enqueue``: fn, an export bound beforehand, on (handle, *args), the caller appending the stream's
        handle itself, and NO device context on the success path — a non-zero status with another device current: switch to this
        env's and repeat; then N.check.  The arguments are plain integers, so the success case is one ctypes call."""
        rc = fn(self._h, *args)
        if rc:
            torch = _torch()
            if torch.cuda.current_device() != self._dev_index:
                with torch.cuda.device(self.device):
                    rc = fn(self._h, *args)
            N.check(rc, self._h, what)

    def _blob_views(self, blob):
        """(obs [N, D] f64, reward [N] f64, done [N] u8, flags [N] u8) views of an output block (device or pinned host)."""
        torch = _torch()
        n, D = self.num_envs, self.states_history
        return (blob[self._o_obs: self._o_obs + n * D * 8].view(torch.float64).view(n, D),
                blob[self._o_rew: self._o_rew + n * 8].view(torch.float64),
                blob[self._o_done: self._o_done + n], blob[self._o_flags: self._o_flags + n])

    def _host_side(self):
        """The host half of the numpy protocols, made once: `host_slots` pinned output blocks (rotated, so that the arrays of
        one step stay valid while the next steps run), a pinned action buffer and a side stream (the completion events live
        in the handle: ssg_step_host / ssg_wait_host)."""
        if self._host is None:
            torch = _torch()
            with torch.cuda.device(self.device):
                blocks = [torch.empty(self._out_nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(self.host_slots)]
                acts = torch.empty(self.num_envs, dtype=torch.int32, pin_memory=True)
                self._host = {"blocks": blocks,
                              "np": [tuple(v.numpy() for v in self._blob_views(b)) for b in blocks],
                              "acts": acts, "acts_np": acts.numpy(), "acts_ptr": acts.data_ptr(),
                              "block_ptrs": [b.data_ptr() for b in blocks], "stream": torch.cuda.Stream(device=self.device),
                              "step_host": N.lib().ssg_step_host, "wait_host": N.lib().ssg_wait_host, "slot": 0, "inflight": None,
                              "infos": [{} for _ in range(self.num_envs)]}
        return self._host

    def enable_terminal_obs(self, on=True):
        """ssg_set_terminal_obs: from now on every step ALSO stores the terminal observation of each env it auto-resets into that
        env's row of `self.term_obs` ([N, D] float64 device tensor; rows of envs that were not done keep whatever they held).  A
        GPU-resident caller gets both observations of an episode's end from one launch: `obs` (reset observation) and
        `torch.where(done[:, None] != 0, term_obs, obs)` (what RLlib's vector_step reports).  Needs in-kernel auto-reset and
        history <= 2."""
        torch = _torch()
        if on and self.term_obs is None:
            self.term_obs = torch.zeros((self.num_envs, self.states_history), dtype=torch.float64, device=self.device)
        self.call("ssg_set_terminal_obs", N.ptr(self.term_obs if on else None))
        if not on:
            self.term_obs = None
        return self.term_obs

    def _fresh_world(self, e):
        rec, polys, goals = worldgen.generate_world(self.bounds, n_goals=self.cfg.n_goals, width_frac=self.width_frac)
        self.bank_host[e] = rec
        self.worlds[e] = (polys, goals)

    def set_bank(self, bank):
        """Install a map bank (numpy [M, MAP_STRIDE] or a device tensor).  A curriculum lesson change calls this."""
        torch = _torch()
        if isinstance(bank, np.ndarray):
            bank = torch.from_numpy(np.ascontiguousarray(bank, dtype=np.float64)).to(self.device)
        if not bank.is_cuda:
            bank = bank.to(self.device)
        self._arg(bank, torch.float64, (0, N.MAP_STRIDE), "set_bank: bank", more_rows=True, exc=AssertionError)
        self.bank = bank
        self.n_maps = int(bank.shape[0])
        self.call("ssg_set_map_bank", bank.data_ptr(), self.n_maps)

    def regenerate_bank(self, seed, width_frac=None, n_maps=None, return_raw=False):
        """Refresh the map bank ON THE DEVICE (no host geometry, no upload): n_maps brand-new rivers and goal paths
        from a Philox stream keyed by (seed, map index).  Not seed-compatible with the reference's python/numpy RNG —
        use the host `worldgen` path for that.  Envs keep their map ids; the new geometry applies from the next step
        on, so callers normally follow with reset_tensor()."""
        torch = _torch()
        n_maps = self.n_maps if n_maps is None else int(n_maps)
        wf = self.width_frac if width_frac is None else float(width_frac)
        bank = self.bank if n_maps == self.n_maps else torch.empty((n_maps, N.MAP_STRIDE), dtype=torch.float64, device=self.device)
        raw = torch.empty((n_maps, 48 + 3 * self.cfg.n_goals), dtype=torch.float64, device=self.device) if return_raw else None
        self.enqueue("ssg_generate_bank", int(seed), wf, bank.data_ptr(), n_maps, N.ptr(raw))
        self.bank_polys = self.bank_goals = None  # host copies no longer describe the bank
        if bank is not self.bank:
            self.set_bank(bank)
        return raw

    def refill_worlds(self, seed=None, width_frac=None, return_raw=False):
        """map_mode="fresh_device": draw every world the rings are missing (ssg_refill_worlds) and make (seed, width_frac)
        the source of the automatic refills from now on — a curriculum lesson change passes the new width here.  With
        return_raw, returns [num_envs*ring, 48 + 3*n_goals]: rows of the slots drawn by THIS call hold the raw polygons
        and goal draws (rows of other slots are NaN)."""
        torch = _torch()
        if self.map_mode != "fresh_device":
            raise N.ShipSimError("refill_worlds needs map_mode='fresh_device'")
        seed = self.map_seed if seed is None else int(seed)
        self.map_seed = seed
        if width_frac is not None:
            self.width_frac = float(width_frac)
        raw = None
        if return_raw:
            raw = torch.full((self.num_envs * self.ring, 48 + 3 * self.cfg.n_goals), float("nan"), dtype=torch.float64, device=self.device)
        self.enqueue("ssg_refill_worlds", seed, self.width_frac, N.ptr(raw))
        return raw

    def launch_geometry(self):
        """(envs per workgroup, bank staged in LDS?, dynamic LDS bytes per workgroup) of the step kernel for this handle."""
        epw, lds, nb = C.c_int(), C.c_int(), C.c_size_t()
        self.call("ssg_debug_launch_geometry", C.byref(epw), C.byref(lds), C.byref(nb))
        return epw.value, bool(lds.value), nb.value

    def field(self, fid):
        """Typed torch view [n_columns, num_envs] (or [num_envs]) into the state blob.  Config 4 (n_ships = 4): after WRITING
        any column through such a view — the player's pose as much as the traffic / goal bodies — call wake_dynamics():
        which envs the dyn kernels visit next step was decided from the state the last step ended with (ssg_dyn_invalidate)."""
        torch = _torch()
        off, es, nc, stride = C.c_size_t(), C.c_int(), C.c_int(), C.c_size_t()
        self.call("ssg_state_field", fid, C.byref(off), C.byref(es), C.byref(nc), C.byref(stride))
        dt = {8: torch.float64, 4: torch.int32, 1: torch.uint8}[es.value]
        if fid == N.F_DYN_LIVE:
            dt = torch.int64                  # (a 64-bit mask)
        if fid == N.F_STATS:
            return self.state[off.value: off.value + 8 * nc.value].view(torch.int64).view(-1, 4)
        if fid == N.F_DYN_MEMO_STATS:
            return self.state[off.value: off.value + 8 * nc.value].view(torch.int64).view(-1, 16)
        n_pad = stride.value // es.value
        v = self.state[off.value: off.value + nc.value * stride.value].view(dt).view(nc.value, n_pad)[:, :self.num_envs]
        return v[0] if nc.value == 1 else v

    def _mask_arg(self, mask, what):
        """A per-env byte mask (None = all envs), checked: uint8 or bool, one element per env."""
        torch = _torch()
        return None if mask is None else self._arg(mask, (torch.uint8, torch.bool), self.num_envs, what + ": mask")

    def wake_dynamics(self, mask=None):
        """Config 4: call after writing ANY state column through field() — the traffic / goal-body columns (envs whose
        bodies had come to rest are otherwise not stepped; the ships' rotation columns, which the step kernel's collide_ship turns
        their hulls with, are recomputed from the angles — for every env) and the player's own columns (which envs the next full
        cpSpaceStep visits was decided from the state the last step ended with): ssg_dyn_invalidate.  Also after restoring or
        copying the state blob.  mask: uint8 device tensor [num_envs]
        (envs whose rest bit is cleared) or None = all; the next step's queue is rebuilt from the columns either way."""
        self.enqueue("ssg_dyn_invalidate", self._mask_arg(mask, "wake_dynamics"))

    def field_stats_tensor(self):
        """int64 device tensor [4]: sum_return*100, sum_length, episodes, goals_hit of this handle (slots summed)."""
        return self.field(N.F_STATS).sum(dim=0)

    def kernel_times(self, enable):
        """Config 4 measurement aid (ssg_debug_kernel_times): returns (full cpSpaceStep us, step kernel us, steps) averaged over
        the steps since the previous call, and switches the per-launch HIP events on or off for the calls that follow."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self.call("ssg_debug_kernel_times", int(bool(enable)), C.byref(a), C.byref(b), C.byref(n))
        return float(a.value), float(b.value), int(n.value)

    def dyn_counters(self):
        """Config 4: (launches of the full cpSpaceStep, how many of them rebuilt their queue from the per-env flags first)."""
        a, b = C.c_uint64(), C.c_uint64()
        self.call("ssg_debug_dyn_counters", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def dyn_memo_stats(self):
        """Config 4: how the full cpSpaceStep of the queued envs was served so far — looked up in the memo table (`hits`),
        computed (`computed`), results stored (`stored`); SSG_F_DYN_MEMO_STATS."""
        s = self.field(N.F_DYN_MEMO_STATS).sum(dim=0).cpu().numpy()
        return {"hits": int(s[0]), "computed": int(s[1]), "stored": int(s[2]),
                "ship_x_bank_narrowphase": {"hits": int(s[3]), "computed": int(s[4])}}

    def stats(self):
        """Per-handle episode counters accumulated in-kernel: sum_return, sum_length, episodes, goals_hit."""
        s = self.field_stats_tensor().cpu().numpy()
        return {"sum_return": float(s[0]) / 100.0, "sum_length": int(s[1]), "episodes": int(s[2]), "goals_hit": int(s[3])}

    # ------------------------------------------------------------------------------------------------
    # snapshot / restore (ship_sim_gym_amd/checkpoint.py's "env" section)
    # ------------------------------------------------------------------------------------------------
    def fingerprint(self):
        """The configuration a snapshot belongs to, as plain data: a snapshot is restored only into an env of the same fingerprint."""
        c = self.cfg
        return {"num_envs": int(self.num_envs), "history": int(c.history), "n_beams": int(c.n_beams), "n_ships": int(c.n_ships),
                "map_mode": str(self.map_mode), "env_id_base": int(self.env_id_base), "bounds": [float(b) for b in self.bounds],
                "max_steps": int(c.max_steps), "flags": int(c.flags), "n_goals": int(c.n_goals), "dt": float(c.dt),
                "state_nbytes": int(self.state.numel()), "out_nbytes": int(self._out_nbytes)}

    def check_snapshot_supported(self, what):
        """NotImplementedError for the handles whose launches depend on host state inside the library's handle."""
        why = None
        if self.n_ships != 1:
            why = "n_ships = %d: the contact solver's queue, memo generation and bank epoch live in the handle" % self.n_ships
        elif self.map_mode != "bank":
            why = "map_mode = %r: %s" % (self.map_mode, "the rings' refill credit and seed live in the handle" if self.map_mode == "fresh_device"
                                         else "the worlds are drawn on the host from the global random streams")
        elif int(self.cfg.history) > 2:
            why = "history = %d: only handles with history <= 2 launch with constant arguments" % int(self.cfg.history)
        elif self.rllib:
            why = "rllib = True: which envs await their reset_at is kept on the host"
        if why is not None:
            raise NotImplementedError("ShipVecEnv.%s: not supported for this handle (%s); supported: n_ships = 1, map_mode = 'bank', "
                                      "history <= 2, rllib = False" % (what, why))

    def snapshot(self):
        """The env's whole mutable state as plain data (CPU tensors, ints, floats, strings, lists, dicts), taken between two calls:
        ``state`` (the state blob: every column, the episode counters of ``stats()``), ``out`` (the output block: obs | reward | done
        | flags, of which the next policy launch reads obs), ``bank`` with ``n_maps``, and ``fingerprint``.  ``restore`` on an env of
        the same fingerprint makes every later step, rollout and statistic bit for bit what this env goes on to compute.

        Supported: one ship, map_mode="bank", history <= 2, rllib=False — the handles whose launches take constant arguments
        (include/shipsim.h, at ssg_rollout).  Anything else raises NotImplementedError before anything is touched.

        For these handles the blob, the output rows and the bank are all there is.  The host-side fields of ``struct ssg_handle``
        (csrc/shipsim_api.cpp) and why none of them is state here:
        * cfg, dev, layout (n_pad, nbytes, every section's offset), block, lds, lds_bytes: functions of the configuration and of n_maps; ``restore``
          re-installs the bank through ``set_bank``, which derives them again;
        * state, bank, n_maps: pointers and a count; the tensors behind them are what the snapshot holds;
        * prepared, policy_prepared, ppo_prepared, policy_filter_prepared, policy_boot_prepared: "the kernel's LDS limit is set", set
          again on demand;
        * zeroed: "the blob was zeroed by a full reset"; ``restore`` runs the env's first full reset itself when none has happened,
          so that a later ``reset_tensor()`` keeps the restored counters as it keeps the original's;
        * remap_pending: set when a bank shrinks; the remap it asks for takes map ids modulo n_maps, which the restored ids satisfy;
        * dyn, dyn_step (the queue's validity, the launch counters, the memo's generation): config 4 only (n_ships = 4);
        * ring (ready, seed, width_frac, credit, the refill queue's pointers): map_ring only (map_mode="fresh_device");
        * time_kernels, t_dyn_ms, t_step_ms, t_steps: a measurement aid's accumulators;
        * host_ev, host_ev_made: completion events of the numpy protocols' copies; no step may be in flight (checked);
        * pop_sizes, dev_slices, slice_max, slice_min, flt, tob, rec, rec_ids, adv_norm_*: bindings (population slices, observation
          filter, time-out bootstrap, evaluation recorder, advantage normalisation) that their owners bind again; their own state is
          their owners';
        * err: the last error's text.
        Not saved either: ``term_obs`` and the time-out bootstrap's rows, which a step or a rollout writes before anyone reads them."""
        self.check_snapshot_supported("snapshot")
        self._no_step_in_flight("snapshot")
        return {"fingerprint": self.fingerprint(), "state": self.state.detach().cpu().clone(), "out": self._out_blob.detach().cpu().clone(),
                "bank": self.bank.detach().cpu().clone(), "n_maps": int(self.n_maps)}

    def _no_step_in_flight(self, what):
        if self._host is not None and self._host["inflight"] is not None:
            raise N.ShipSimError("ShipVecEnv.%s: a step_async is in flight; call step_wait first" % what)

    def restore(self, snap):
        """Put a ``snapshot()`` back, in place: the state blob, the output block and the bank keep their addresses, so the tensors
        (``obs``, ``reward``, ``done``, ``flags``, ``field()`` views) and the pointers this env handed out stay valid; the bank is
        re-installed through ``set_bank`` (a bank of another n_maps replaces the tensor).  Checked first: NotImplementedError for an
        unsupported handle, ValueError for a snapshot of another fingerprint (every differing key with both values) or with tensors
        of the wrong size — and then nothing has changed."""
        torch = _torch()
        self.check_snapshot_supported("restore")
        self._no_step_in_flight("restore")
        if not isinstance(snap, dict) or not isinstance(snap.get("fingerprint"), dict):
            raise ValueError("ShipVecEnv.restore: not a snapshot (no fingerprint)")
        mine, theirs = self.fingerprint(), snap["fingerprint"]
        bad = ["%s is %r in the snapshot and %r in this env" % (k, theirs.get(k, "missing"), mine.get(k, "missing"))
               for k in sorted(set(mine) | set(theirs)) if k not in theirs or k not in mine or theirs[k] != mine[k]]
        staged = {}  # the snapshot's tensors on the device, checked as what the copies below will read
        for name, dt, shape in (("state", torch.uint8, (self.state.numel(),)), ("out", torch.uint8, (self._out_nbytes,)),
                                ("bank", torch.float64, (1, N.MAP_STRIDE))):
            try:
                if not torch.is_tensor(snap.get(name)):
                    raise ValueError("%s must be a tensor" % name)
                staged[name] = snap[name].to(self.device).contiguous()
                self._arg(staged[name], dt, shape, name, more_rows=name == "bank")
            except ValueError as ex:
                bad.append(str(ex))
        if "bank" in staged and (type(snap.get("n_maps")) is not int or snap["n_maps"] != staged["bank"].shape[0]):
            bad.append("n_maps must be an int, the number of the bank's rows")
        if bad:
            raise ValueError("ShipVecEnv.restore: " + "; ".join(bad))
        with torch.cuda.device(self.device):
            if not self._full_reset_done:
                self.reset_tensor()  # (the handle's first full reset zeroes the blob: let it happen before the blob is written)
            self.state.copy_(staged["state"])
            self._out_blob.copy_(staged["out"])
            new_bank = staged["bank"]
            same_shape = tuple(self.bank.shape) == tuple(new_bank.shape)
            if not (same_shape and torch.equal(self.bank, new_bank)):
                self.bank_polys = self.bank_goals = None  # (host copies, if any, no longer describe the bank)
            if same_shape:
                self.bank.copy_(new_bank)
                new_bank = self.bank
            self.set_bank(new_bank)
        self._pending = None
        return self

    # ------------------------------------------------------------------------------------------------
    # tensor API (zero-copy; what a GPU-resident policy should use)
    # ------------------------------------------------------------------------------------------------
    def reset_tensor(self, mask=None, map_ids=None):
        self._mask_arg(mask, "reset_tensor")
        if map_ids is not None:
            self._arg(map_ids, self._i32, self.num_envs, "reset_tensor: map_ids")
        self._reset_launch(mask, map_ids, self.obs)
        return self.obs

    def _reset_launch(self, mask, map_ids, dest):
        """ssg_reset of the masked envs (None: all of them, a full reset) onto the maps `map_ids` (None: "fresh": env e's own bank
        slot, e; else the library's rule), writing their rows of `dest`."""
        torch = _torch()
        if mask is None:
            self._full_reset_done = True
        own_ids = self.map_mode == "fresh" and map_ids is None
        if own_ids:
            map_ids = torch.arange(self.num_envs, dtype=torch.int32, device=self.device)
        self.enqueue("ssg_reset", N.ptr(mask), N.ptr(map_ids), dest.data_ptr())
        if own_ids:
            torch.cuda.current_stream(self.device).synchronize()  # keep the ids alive until the kernel ran

    def _host_reset(self, envs, dest):
        """THE host-driven reset: `envs` — a host bool array [N], one env index, or None for a full reset — are re-initialised by
        ONE ssg_reset that writes their rows of `dest` (self.obs or a side buffer), and the stream is synchronised.  Where each env
        goes, per map mode: "fresh" draws it a brand-new world on the host (ascending env index, one world per env) and uploads
        the bank; "bank" moves it to the next map modulo n_maps, exactly the sequence the in-kernel auto-reset follows (a full
        reset: to its first map); "fresh_device" passes no ids — the reset kernel moves the env to the next world of its ring."""
        torch = _torch()
        mask_h = envs
        if envs is not None and not isinstance(envs, np.ndarray):
            mask_h = np.arange(self.num_envs) == envs
        with torch.cuda.device(self.device):
            mask = None if mask_h is None else torch.from_numpy(mask_h.astype(np.uint8)).to(self.device)
            ids = None
            if self.map_mode == "fresh":
                for e in (range(self.num_envs) if mask_h is None else np.nonzero(mask_h)[0]):
                    self._fresh_world(int(e))
                self.bank.copy_(torch.from_numpy(self.bank_host))
            elif self.map_mode == "bank" and mask is not None:
                cur = self.field(N.F_MAP_ID)
                ids = torch.where(mask != 0, (cur + 1) % self.n_maps, cur).to(torch.int32).contiguous()
            self._reset_launch(mask, ids, dest)
            torch.cuda.current_stream(self.device).synchronize()

    def _rows_h(self, src, idx):
        """Rows `idx` (a host index array) of the device tensor `src`, as a numpy array."""
        return src[_torch().from_numpy(idx).to(self.device)].cpu().numpy()

    def step_tensor(self, actions):
        """actions: int32 device tensor [N].  Returns (obs, reward, done, flags) device tensors (reused buffers).
        This is the policy-in-the-loop path: one launch per call, so the host side is kept to one ctypes call with plain
        integers (the cached output pointers, the actions' address, the current stream's handle)."""
        # (a tensor of another dtype / size would be read as int32 [N] all the same: wrong steps, or a read past its end)
        a = self._arg(actions, self._i32, self.num_envs, "step_tensor: actions")
        o, r, d, f = self._out
        self._launch("ssg_step", self._lib.ssg_step, a, o, r, d, f, self._cur_stream(self.device).cuda_stream)
        return self.obs, self.reward, self.done, self.flags

    def rollout_tensor(self, actions_kn, trajectory=False, out=None):
        """K back-to-back steps from a pre-generated int32 [K, N] action tensor (random-action throughput run).

        trajectory=False: every step rewrites the env's reused [N, ...] buffers; returns the LAST step's
        (obs, reward, done, flags).  trajectory=True (ssg_rollout_traj): every step's outputs are kept, as the reference's
        rollout loop sees them (train/random.py:14-27) — returns (obs [K, N, D], reward [K, N], done [K, N], flags [K, N])
        device tensors; `out` = a tuple of four such preallocated tensors (first dimension >= K, contiguous) to write
        into instead of allocating.  self.obs / reward / done / flags are left untouched in trajectory mode."""
        n, D = self.num_envs, self.states_history
        a = self._arg(actions_kn, self._i32, (0, n), "rollout_tensor: actions", more_rows=True)
        K = actions_kn.shape[0]
        if not trajectory:
            self._launch("ssg_rollout", self._lib.ssg_rollout, a, K, *self._out, self._cur_stream(self.device).cuda_stream)
            return self.obs, self.reward, self.done, self.flags
        if out is not None:
            # a buffer set seen before: one ctypes call with plain integers, like step_tensor — a 20-step launch is ~140 us, and
            # everything the host does before the launch is GPU idle time inside a caller's timed region.  The cache holds
            # POINTERS and shapes only, never the tensors (a caller's `del bufs` really frees them), and a hit needs all four
            # buffers to sit where they sat when the plan was made, with the shapes checked then.
            po = out[0].data_ptr()
            plan = self._traj_plans.get(po)
            if plan is not None:
                pr, pd, pf, cap, sig = plan
                # (a hit needs the four buffers to be what was checked when the plan was made: addresses AND dtype / shape /
                # strides / device of each — the caching allocator readily hands a freed buffer's address to another tensor)
                if (K <= cap and out[1].data_ptr() == pr and out[2].data_ptr() == pd and out[3].data_ptr() == pf
                        and tuple((t.dtype, tuple(t.shape), t.stride(), t.device.index) for t in out) == sig):
                    self._launch("ssg_rollout_traj", self._lib.ssg_rollout_traj, a, K, po, pr, pd, pf, n,
                                 self._cur_stream(self.device).cuda_stream)
                    return out[0][:K], out[1][:K], out[2][:K], out[3][:K]  # (sliced after the launch: the GPU is already busy)
        torch = _torch()
        specs = ((torch.float64, (K, n, D)), (torch.float64, (K, n)), (torch.uint8, (K, n)), (torch.uint8, (K, n)))
        caller_out = out is not None
        if out is None:
            out = tuple(torch.empty(shape, dtype=dt, device=self.device) for dt, shape in specs)
        to, tr, td, tf = out
        ptrs = [self._arg(t, dt, shape, "rollout_tensor: out[%d]" % j, more_rows=True, exc=AssertionError)
                for j, (t, (dt, shape)) in enumerate(zip(out, specs))]
        self._launch("ssg_rollout_traj", self._lib.ssg_rollout_traj, a, K, *ptrs, n, self._cur_stream(self.device).cuda_stream)
        if caller_out:
            if len(self._traj_plans) >= 8 and ptrs[0] not in self._traj_plans:  # (a handful of rotating buffer sets at most)
                self._traj_plans.pop(next(iter(self._traj_plans)))
            self._traj_plans[ptrs[0]] = (*ptrs[1:], min(int(t.shape[0]) for t in out),
                                         tuple((t.dtype, tuple(t.shape), t.stride(), t.device.index) for t in out))
        return to[:K], tr[:K], td[:K], tf[:K]

    def clear_traj_cache(self):
        """Forget the cached launch plans of rollout_tensor(trajectory=True, out=...).  They hold no tensors (pointers and
        shapes only), so this is never needed to free memory; it exists for callers that recycle addresses deliberately."""
        self._traj_plans.clear()

    # ------------------------------------------------------------------------------------------------
    # the policy in the loop on the device (ABI 9: ssg_policy_act / ssg_rollout_policy; ship_sim_gym_amd/policy.py)
    # ------------------------------------------------------------------------------------------------
    def _check_policy(self, policy, what):
        if self.map_mode == "fresh":
            raise ValueError("%s: map_mode='fresh' draws every new world on the host at each done; use 'bank' or 'fresh_device'" % what)
        if self.rllib:
            raise ValueError("%s: the rllib flow is a numpy protocol (reset_at per done env); construct the env with rllib=False" % what)
        if not self.auto_reset:
            raise ValueError("%s: needs auto_reset=True (a done env is reset inside the step)" % what)
        if policy.obs_dim != self.states_history:
            raise ValueError("%s: the policy's obs_dim %d differs from the env's %d" % (what, policy.obs_dim, self.states_history))
        if policy.params.device != self.device or policy.obs_scale.device != self.device:
            raise ValueError("%s: the policy lives on %s, the env on %s" % (what, policy.params.device, self.device))

    def _f32_rows(self, t, shape, what):
        """A float32 tensor of at least shape[0] rows, checked (None stays None): its address."""
        return None if t is None else self._arg(t, _torch().float32, shape, what, more_rows=True)

    def policy_act(self, policy, seed=0, step=0, uniforms=None, x_out=None, greedy=False):
        """The policy forward + inverse-CDF sampling on the env's current `obs` (ssg_policy_act): returns (act int32 [N], logp [N],
        value [N], x [N, D] float32) device tensors.  uniforms: float32 [N] (e.g. torch.rand) or None = Philox keyed by (seed, step,
        global env id).  x_out: a float32 [N, D] tensor to write the normalised observations into.  greedy=True (ssg_policy_act_greedy):
        the first action with the largest logit instead of a draw, and its logp; value and x are the sampling call's bit for bit, seed
        and step are not used, and `uniforms` with it raises ValueError."""
        return self._act(self._check_policy, policy, "ssg_policy_act", "policy_act", seed, step, uniforms, x_out, greedy)

    def _act(self, check, record, c_name, what, seed, step, uniforms, x_out, greedy):
        """policy_act / population_act: `check` judges the record, c_name is its sampling entry point (c_name + "_greedy": the other)."""
        torch = _torch()
        check(record, what)
        if greedy and uniforms is not None:
            raise ValueError("%s: greedy=True reads no uniforms (pass one or the other)" % what)
        n, D = self.num_envs, self.states_history
        up = self._f32_rows(uniforms, (n,), what + ": uniforms")
        act = torch.empty(n, dtype=torch.int32, device=self.device)
        logp = torch.empty(n, dtype=torch.float32, device=self.device)
        val = torch.empty(n, dtype=torch.float32, device=self.device)
        x = x_out if x_out is not None else torch.empty((n, D), dtype=torch.float32, device=self.device)
        xp = self._f32_rows(x, (n, D), what + ": x_out")
        rec = record.to_native()
        if greedy:
            c_name, draw = c_name + "_greedy", ()
        else:
            draw = (up, int(seed), int(step))
        self.enqueue(c_name, C.byref(rec), self.obs.data_ptr(), *draw, act.data_ptr(), logp.data_ptr(), val.data_ptr(), xp)
        return act, logp, val, x

    def rollout_policy(self, policy, K, seed=0, step0=0, uniforms=None, out=None):
        """K rollout steps with the policy in the loop, enqueued from C on the current stream (ssg_rollout_policy): step k runs the
        policy on the env's current obs, then ssg_step with the sampled actions.  Returns a dict of device tensors — obs f32 [K, N, D]
        (the normalised observation each step's action was drawn from), act i32 / logp f32 / val f32 / rew f64 / done u8 / flags u8
        [K, N], last_val f32 [N] (the value of the observation after the last step).  uniforms: float32 [K, N] or None = Philox keyed
        by (seed, step0 + k, global env id).  out: such a dict, preallocated (first dimension >= K), to write into.  Leaves `obs`
        holding the observation after the last step, like K step_tensor calls."""
        return self._rollout(self._check_policy, policy, "ssg_rollout_policy", "rollout_policy", K, seed, step0, uniforms, out)

    def _rollout(self, check, record, c_name, what, K, seed, step0, uniforms, out):
        """rollout_policy / rollout_population: `check` judges the record, c_name is its entry point."""
        check(record, what)
        K, n = int(K), self.num_envs
        if K < 1:
            raise ValueError("%s: K must be >= 1" % what)
        up = self._f32_rows(uniforms, (K, n), what + ": uniforms")
        boot = self._timeout_rows(K, out, what)
        out, p = self._rollout_buffers(K, out, what)
        rec = record.to_native()
        self.enqueue(c_name, C.byref(rec), K, up, int(seed), int(step0), self.obs.data_ptr(), p["act"], p["logp"], p["val"], p["obs"],
                     p["rew"], p["done"], p["flags"], p["last_val"], n)
        res = {k: (v[:K] if k != "last_val" else v) for k, v in out.items() if k != "boot"}
        if boot is not None:  # (with the bootstrap off a caller's out["boot"] is not part of the batch: nothing wrote it)
            res["boot"] = boot[:K]
        return res

    def _rollout_buffers(self, K, out, what):
        """The out-dict of a policy-in-the-loop rollout of K steps (allocated, or the caller's checked) and its tensors' C pointers."""
        torch = _torch()
        n, D = self.num_envs, self.states_history
        specs = {"obs": ((K, n, D), torch.float32), "act": ((K, n), torch.int32), "logp": ((K, n), torch.float32),
                 "val": ((K, n), torch.float32), "rew": ((K, n), torch.float64), "done": ((K, n), torch.uint8),
                 "flags": ((K, n), torch.uint8), "last_val": ((n,), torch.float32)}
        if out is None:
            out = {k: torch.empty(s, dtype=dt, device=self.device) for k, (s, dt) in specs.items()}
        return out, {k: self._arg(out[k], dt, s, "%s: out[%r]" % (what, k), more_rows=True) for k, (s, dt) in specs.items()}

    # ------------------------------------------------------------------------------------------------
    # a population of policies on this handle (ssg_pop_act / ssg_pop_rollout; ship_sim_gym_amd/population.py)
    # ------------------------------------------------------------------------------------------------
    def _check_population(self, population, what):
        self._check_policy(population, what)
        sizes = self.population_slices
        if sizes is not None:
            if len(sizes) != len(population):
                raise ValueError("%s: %d members, but slices for %d members are bound (set_population_slices)"
                                 % (what, len(population), len(sizes)))
        elif self.num_envs % len(population):
            raise ValueError("%s: %d envs do not split into %d equal member slices" % (what, self.num_envs, len(population)))

    def set_population_slices(self, sizes):
        """Lay a population out over this handle's envs in contiguous slices of unequal size (ssg_pop_set_slices): member m owns
        sizes[m] envs from sum(sizes[:m]) on; every size >= 1, sum(sizes) == num_envs.  While bound, every population call on this env
        (population_act, rollout_population, PopulationPPO, NativeEvaluator) follows the slices and takes a population of len(sizes)
        members only.  None unbinds.  Env state is not touched: envs are fungible, so a layout may be re-bound between updates."""
        torch = _torch()
        if sizes is None:
            self.call("ssg_pop_set_slices", 0, None, None)
            self._pop_slices = None
            return
        sizes = [int(s) for s in sizes]
        P = len(sizes)
        arr = (C.c_int32 * max(P, 1))(*sizes)
        n = N.POP_SLICE_ROW * P
        buf = (C.c_int32 * max(n, 1))()
        N.call("ssg_pop_pack_slices", P, arr, buf, n)
        if sum(sizes) != self.num_envs:
            raise ValueError("set_population_slices: the sizes sum to %d, the handle has %d envs" % (sum(sizes), self.num_envs))
        table = torch.tensor(list(buf), dtype=torch.int32).to(self.device)
        self.call("ssg_pop_set_slices", P, arr, table.data_ptr())
        # (the device table is the caller's memory; an earlier one stays alive until launches that read it have been enqueued AND run:
        # torch's allocator does not hand a freed block to another stream's work before that)
        self._pop_slices = (sizes, table)

    @property
    def population_slices(self):
        """The bound slice sizes (a list of P ints, as the library holds them: ssg_pop_get_slices), or None."""
        if self._pop_slices is None:
            return None
        P = C.c_int()
        self.call("ssg_pop_get_slices", C.byref(P), None)
        out = (C.c_int32 * max(P.value, 1))()
        self.call("ssg_pop_get_slices", C.byref(P), out)
        return [int(out[m]) for m in range(P.value)] or None

    def population_act(self, population, seed=0, step=0, uniforms=None, x_out=None, greedy=False):
        """policy_act with env e evaluated under member e // (N / P) of a NativePopulation — or, with set_population_slices, under the
        member whose slice holds it — (ssg_pop_act, one launch): returns (act
        int32 [N], logp [N], value [N], x [N, D] float32) device tensors.  uniforms / x_out / Philox keying / greedy as policy_act
        (greedy=True: ssg_pop_act_greedy)."""
        return self._act(self._check_population, population, "ssg_pop_act", "population_act", seed, step, uniforms, x_out, greedy)

    def rollout_population(self, population, K, seed=0, step0=0, uniforms=None, out=None):
        """rollout_policy with env e acting under member e // (N / P) of a NativePopulation (ssg_pop_rollout: one policy launch per step
        for the whole population, then ssg_step).  Same out-dict, uniforms, Philox keying and `out` as rollout_policy; member m's
        columns are [m*n, (m+1)*n), n = N / P, or its slice of set_population_slices."""
        return self._rollout(self._check_population, population, "ssg_pop_rollout", "rollout_population", K, seed, step0, uniforms, out)

    # ------------------------------------------------------------------------------------------------
    # the time-out bootstrap (ssg_set_timeout_boot): the value of a timed-out episode's terminal observation, for GAE
    # ------------------------------------------------------------------------------------------------
    def set_timeout_bootstrap(self, on=True, rows=None):
        """Switch the time-out bootstrap on or off.  While it is on, rollout_policy / rollout_population also return batch["boot"]
        (f32 [K, N]): V(terminal observation) where the clock alone ended the episode (EV_MAX_STEPS without EV_COLLIDING,
        EV_OUT_OF_BOUNDS or EV_NO_GOALS_LEFT), +0.0 elsewhere — one more launch per rollout, after the last-value forward; every other
        entry of the batch and the env state stay bit for bit what they are with it off.  NativePPO.gae / PopulationPPO.gae then
        bootstrap those samples from it.  rows: the longest rollout to allocate for now (the buffers grow when a rollout asks for
        more).  The terminal observations take rows * N * D * 8 bytes of device memory (537 MB at 65 536 envs x 32 steps x D = 32,
        67 MB at 4 096 x 64), allocated here, reused by every rollout, freed when switched off.  Needs in-kernel auto-reset and
        history <= 2, like enable_terminal_obs, whose own binding stays in place between rollouts.  A refused call leaves the
        previous state."""
        if not on:
            self.call("ssg_set_timeout_boot", None)
            self._timeout_boot = None
            return
        self._bind_timeout_boot(max(1, int(rows or 1)), None)

    @property
    def timeout_bootstrap(self):
        """The rows the bound time-out buffers serve (ssg_get_timeout_boot), or 0 with the bootstrap off."""
        rec = N.TimeoutBootRecord()
        self.call("ssg_get_timeout_boot", C.byref(rec))
        return int(rec.rows) if rec.struct_size else 0

    def _bind_timeout_boot(self, rows, boot):
        """Bind a record of `rows` rows: the kept terminal-observation rows if they serve that many (else new ones), and `boot` (None:
        the kept or a new f32 [rows, N])."""
        torch = _torch()
        old = self._timeout_boot
        if old is not None and old["term_obs"].shape[0] >= rows:
            term = old["term_obs"]
        else:
            old = None  # (grown: the kept boot rows are too short as well)
            term = torch.empty((rows, self.num_envs, self.states_history), dtype=torch.float64, device=self.device)
        if boot is None:
            boot = old["boot"] if old is not None else torch.empty((term.shape[0], self.num_envs), dtype=torch.float32, device=self.device)
        rec = N.TimeoutBootRecord()
        rec.struct_size, rec.rows = C.sizeof(N.TimeoutBootRecord), min(int(term.shape[0]), int(boot.shape[0]))
        rec.dev_term_obs_KND, rec.dev_boot_KN = term.data_ptr(), boot.data_ptr()
        self.call("ssg_set_timeout_boot", C.byref(rec))
        self._timeout_boot = {"term_obs": term, "boot": boot}

    def timeout_values(self, record, flags, term_obs, out=None):
        """The time-out values of K rows in one launch (ssg_timeout_values for a NativePolicy, ssg_pop_timeout_values for a
        NativePopulation): flags u8 [K, N] (a rollout's), term_obs f64 [K, N, D] (the terminal observations, read only where a wave of
        64 envs holds a time-out) -> f32 [K, N]: the value ``policy_act`` gives for that observation row where N.is_timeout(flags),
        +0.0 elsewhere.  Needs no bootstrap to be switched on; a bound observation filter is read, never updated."""
        torch = _torch()
        from .population import NativePopulation
        pop = isinstance(record, NativePopulation)
        what = "timeout_values"
        (self._check_population if pop else self._check_policy)(record, what)
        n, D = self.num_envs, self.states_history
        fp = self._arg(flags, torch.uint8, (1, n), what + ": flags", more_rows=True)
        K = int(flags.shape[0])
        tp = self._arg(term_obs, torch.float64, (K, n, D), what + ": term_obs")
        if out is None:
            out = torch.empty((K, n), dtype=torch.float32, device=self.device)
        op = self._f32_rows(out, (K, n), what + ": out")
        rec = record.to_native()
        self.enqueue("ssg_pop_timeout_values" if pop else "ssg_timeout_values", C.byref(rec), K, fp, tp, op, n)
        return out[:K]

    def _timeout_rows(self, K, out, what):
        """Ahead of a rollout of K steps: None with the bootstrap off; else the f32 [>= K, N] tensor the rollout writes its time-out
        values into — out["boot"] when the caller's out-dict has one, else a new one per rollout (a batch kept across rollouts keeps
        its values) — bound together with terminal-observation rows that serve K."""
        torch = _torch()
        if self._timeout_boot is None:
            return None
        boot = out.get("boot") if out is not None else None
        if boot is None:
            boot = torch.empty((K, self.num_envs), dtype=torch.float32, device=self.device)
        self._f32_rows(boot, (K, self.num_envs), what + ": out['boot']")
        self._bind_timeout_boot(K, boot)
        return boot

    # ------------------------------------------------------------------------------------------------
    # the observation filter (ssg_set_obs_filter; ship_sim_gym_amd/obs_filter.py)
    # ------------------------------------------------------------------------------------------------
    def set_obs_filter(self, f):
        """Bind an ObsFilter (or one of its frozen() views) to this env: every policy launch on it — policy_act, rollout_policy,
        population_act, rollout_population, NativeEvaluator — then forms x = clamp((obs - mean) / denom) from the filter's state instead
        of obs / obs_scale, a single policy with a filter of 1 member, a population of P members with one of P; the rollout loops
        merge each step's observations first when the filter is updating — a job filter's (``ObsFilter(job=True)``) into its buffer
        too, which is bound with it.  The library keeps a copy of the record, this env a
        reference to the filter (whose tensors the launches read).  None unbinds; a refused binding leaves the old one in place."""
        old = self._obs_filter
        if f is None:
            self.call("ssg_set_obs_filter", None)
        else:
            if f.state.device != self.device:
                raise ValueError("set_obs_filter: the filter lives on %s, the env on %s" % (f.state.device, self.device))
            rec = f.to_native()
            self.call("ssg_set_obs_filter", C.byref(rec))
            if getattr(f, "buffer", None) is not None:  # a job filter: the rollout loops merge into its buffer too (the call above dropped it)
                self.call("ssg_set_obs_filter_buffer", f.buffer.data_ptr())
        if old is not None and old is not f and self in old._bound:
            old._bound.remove(self)
        if f is not None and self not in f._bound:
            f._bound.append(self)
        self._obs_filter = f

    @property
    def obs_filter(self):
        """The bound ObsFilter, or None."""
        return self._obs_filter

    # ------------------------------------------------------------------------------------------------
    # per-minibatch advantage normalisation (ssg_ppo_set_adv_norm; NativePPO / PopulationPPO bind their own before every call)
    # ------------------------------------------------------------------------------------------------
    def set_adv_norm(self, mode, scratch=None, n_members=1):
        """Bind the advantage-normalisation mode of the device PPO update: N.ADV_NORM_BATCH (the default: once per rollout, nothing
        bound) or N.ADV_NORM_MINIBATCH (PPO2's rule) with `scratch`, a uint8 device tensor of ssg_ppo_adv_norm_nbytes(n_members) bytes
        that the caller keeps alive.  Host only; a refused binding leaves the old one in place."""
        nb = scratch.numel() * scratch.element_size() if scratch is not None else 0
        self.call("ssg_ppo_set_adv_norm", int(mode), int(n_members), N.ptr(scratch), nb)
        self._adv_norm_scratch = scratch if int(mode) == N.ADV_NORM_MINIBATCH else None
        self._adv_table = None  # (a successful binding of a mode drops a bound table)

    def adv_norm(self):
        """(mode, n_members) as bound (ssg_ppo_get_adv_norm)."""
        mode, members = C.c_int(), C.c_int()
        self.call("ssg_ppo_get_adv_norm", C.byref(mode), C.byref(members))
        return mode.value, members.value

    def set_adv_table(self, table):
        """Bind the job's table of per-minibatch advantage statistics (ssg_ppo_set_adv_table): a contiguous f32 [rows, 4] device tensor
        that the caller keeps alive, row 0 selected; None unbinds.  While it is bound the gradient calls read the selected row and
        launch no statistics kernel, and the mode is N.ADV_NORM_BATCH.  Host only; a refused binding leaves the old one in place."""
        if table is not None:  # (judged on whichever device it lives on: this call has never asked for the env's)
            N.arg(table, _torch().float32, (0, 4), "ShipVecEnv.set_adv_table: table", table.device, more_rows=True)
        self.call("ssg_ppo_set_adv_table", N.ptr(table), 0 if table is None else int(table.shape[0]))
        self._adv_table = table
        if table is not None:
            self._adv_norm_scratch = None

    def select_adv_row(self, row):
        """The row of the bound table the next gradient call reads (ssg_ppo_select_adv_row).  Host only."""
        self.call("ssg_ppo_select_adv_row", int(row))

    def adv_table(self):
        """(address or None, rows, selected row) as bound (ssg_ppo_get_adv_table)."""
        table, rows, row = C.c_void_p(), C.c_int(), C.c_int()
        self.call("ssg_ppo_get_adv_table", C.byref(table), C.byref(rows), C.byref(row))
        return table.value, rows.value, row.value

    def random_actions(self, seed, step0, K):
        """int32 [K, N] Philox action stream keyed by (seed, step, global env id), generated on the device."""
        torch = _torch()
        out = torch.empty((K, self.num_envs), dtype=torch.int32, device=self.device)
        self.enqueue("ssg_fill_actions", int(seed), int(step0), int(K), out.data_ptr())
        return out

    # ------------------------------------------------------------------------------------------------
    # stable-baselines VecEnv protocol (numpy in / numpy out)
    # ------------------------------------------------------------------------------------------------
    def reset(self):
        self._host_reset(None, self.obs)
        return self.obs.cpu().numpy()

    def step_async(self, actions):
        """VecEnv.step_async: checks the actions, then LAUNCHES the step — actions host -> device from a pinned buffer, ssg_step,
        and ONE device -> host copy of the packed obs | reward | done | flags block into a pinned host block, all on a side
        stream — and returns at once: the step runs while the caller does whatever it does between step_async and step_wait."""
        a = np.asarray(actions)
        # ship_env.py:143 `assert self.action_space.contains(action)` for the whole batch in one range check
        ok = a.dtype.kind in "iu" and a.size == self.num_envs and bool(np.all((a >= 0) & (a < self.action_space.n)))
        assert ok, "%r (%s) invalid" % (a, a.dtype)
        self._pending = a.astype(np.int32).reshape(self.num_envs)
        if self._closed:
            return
        hs = self._host_side()
        np.copyto(hs["acts_np"], self._pending)
        slot = hs["slot"]
        io = hs["stream"]
        io.wait_stream(self._cur_stream(self.device))  # after whatever the tensor API queued (a reset, say)
        # ONE foreign call: actions host -> device, ssg_step, the packed block device -> host, the slot's completion event
        o, r, d, f = self._out
        self._launch("ssg_step_host", hs["step_host"], hs["acts_ptr"], self._actions.data_ptr(), o, r, d, f, self._out_blob.data_ptr(),
                     hs["block_ptrs"][slot], self._out_nbytes, slot, io.cuda_stream)
        hs["inflight"] = slot
        hs["slot"] = (slot + 1) % self.host_slots

    def step_wait(self):
        """VecEnv.step_wait: waits for the event behind step_async's device -> host copy and returns numpy views of that pinned
        block — obs [N, D] float64, rewards [N], dones [N] bool — plus a reused list of N empty info dicts.  The observation
        array is a view of one of `host_slots` rotating blocks: it stays valid until `host_slots - 1` further steps have been
        taken (stable-baselines' runners copy it into their own buffer at once: `self.obs[:] = obs`); rewards and dones are
        fresh small arrays (runners keep them in lists).  `copy_host_outputs=True` returns a fresh observation array too."""
        hs = self._host_side()
        slot = hs["inflight"]
        if slot is None:
            raise N.ShipSimError("step_wait without a step_async")
        hs["inflight"] = None
        # (the step is COMPLETE when this returns — a host-side wait on the slot's event — so later tensor-API calls on any stream see it)
        N.check(hs["wait_host"](self._h, slot), self._h, "ssg_wait_host")
        obs_h, rew_h, done_u8, _ = hs["np"][slot]
        done_h = done_u8.view(np.bool_).copy()
        if self.map_mode == "fresh" and self.auto_reset and done_h.any():
            # host-side auto-reset with brand-new worlds (reference-exact resets)
            self._host_reset(done_h, self.obs)
            obs_h[done_h] = self._rows_h(self.obs, np.nonzero(done_h)[0])  # (the reset observations replace the terminal ones)
        return (obs_h.copy() if self.copy_host_outputs else obs_h), rew_h.copy(), done_h, hs["infos"]

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        self._traj_plans.clear()
        self._timeout_boot = None
        flt, self._obs_filter = self._obs_filter, None
        if flt is not None and self in flt._bound:
            flt._bound.remove(self)
        self._out = (0, 0, 0, 0)  # (no address outlives the handle: a call after close() is refused for its NULL handle)
        hs = self._host
        if hs is not None:
            try:
                hs["stream"].synchronize()  # a step_async still in flight reads and writes the buffers about to go
            except Exception:
                pass
            self._host = None
        if not self._closed and self._h:
            N.lib().ssg_destroy(self._h)
            self._h = None
            self._closed = True

    def seed(self, seed=None):
        """ShipEnv.seed seeds numpy's global generator only (ship_env.py:52-60)."""
        np.random.seed(seed)
        return [seed]

    def get_screen(self, env=0, width=None, height=None, debug=True):
        """ShipGame.render + get_screen (game.py:133-138,197-229) for one env: uint8 [width, height, 3] like
        pygame.surfarray.array3d (x first, screen y down), rasterised on the GPU (csrc/shipsim_render.hip)."""
        torch = _torch()
        width = int(width or self.bounds[0])
        height = int(height or self.bounds[1])
        img = torch.empty((width, height, 3), dtype=torch.uint8, device=self.device)
        self.enqueue("ssg_render", int(env), width, height, img.data_ptr(), 1 if debug else 0)
        return img

    def get_screens(self, envs, width=None, height=None, debug=True):
        """get_screen for several envs in ONE launch (ssg_render_envs): uint8 [len(envs), width, height, 3], frame i bit for bit
        get_screen(envs[i]).  envs: a sequence of env indices, or an int32 device tensor of them; at most RENDER_MAX_ENVS frames and
        2^31 bytes per call.  An index outside 0 .. num_envs-1 leaves its frame unwritten (the ids are only read on the device)."""
        torch = _torch()
        width = int(width or self.bounds[0])
        height = int(height or self.bounds[1])
        with torch.cuda.device(self.device):
            if torch.is_tensor(envs):
                ids = envs.to(device=self.device, dtype=torch.int32).contiguous().reshape(-1)
            else:
                ids = torch.tensor([int(e) for e in envs], dtype=torch.int32, device=self.device)
            out = torch.empty((ids.numel(), width, height, 3), dtype=torch.uint8, device=self.device)
        self.enqueue("ssg_render_envs", ids.data_ptr(), ids.numel(), width, height, out.data_ptr(), 1 if debug else 0)
        return out

    def render(self, mode='human', close=False, env=0):
        """ShipEnv.render (ship_env.py:158-168) only writes a text line (done by the ShipEnv facade); 'rgb_array'
        returns the frame the reference's screen would hold, as a numpy array [H, W, 3]."""
        if mode == 'rgb_array':
            return self.get_screen(env).permute(1, 0, 2).cpu().numpy()
        return None

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        if isinstance(indices, (int, np.integer)):
            return [int(indices)]
        return [int(i) for i in indices]

    def env(self, index):
        """Per-env handle (cached): what `env_method` / `get_attr` / `set_attr` / `get_unwrapped` act on."""
        index = int(index)
        if not 0 <= index < self.num_envs:
            raise IndexError(index)
        h = self._handles.get(index)
        if h is None:
            h = self._handles[index] = EnvHandle(self, index)
        return h

    def get_attr(self, attr_name, indices=None):
        """VecEnv.get_attr: the attribute of each selected env (per-env values set by set_attr win over the batch's)."""
        return [getattr(self.env(i), attr_name) for i in self._indices(indices)]

    def set_attr(self, attr_name, value, indices=None):
        """VecEnv.set_attr: stored per env; the batched physics configuration itself is fixed at construction."""
        for i in self._indices(indices):
            setattr(self.env(i), attr_name, value)

    def env_method(self, method_name, *method_args, **method_kwargs):
        """VecEnv.env_method: call `method_name` on each selected env handle (reset / seed / render / close, or any
        batch method that takes no env index) and return the list of results."""
        indices = method_kwargs.pop("indices", None)
        return [getattr(self.env(i), method_name)(*method_args, **method_kwargs) for i in self._indices(indices)]

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False for _ in self._indices(indices)]

    def get_images(self):
        """render('rgb_array') of every env, as a list of [H, W, 3] arrays: one launch and one device-to-host copy per block of envs
        (get_screens; a block holds at most 64 MiB of frames) instead of one of each per env."""
        frame_bytes = int(self.bounds[0]) * int(self.bounds[1]) * 3
        block = max(1, min(N.RENDER_MAX_ENVS, (64 << 20) // frame_bytes))
        images = []
        for start in range(0, self.num_envs, block):
            frames = self.get_screens(range(start, min(start + block, self.num_envs))).cpu()
            images.extend(frames[i].permute(1, 0, 2).numpy() for i in range(frames.shape[0]))
        return images

    @property
    def unwrapped(self):
        return self

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------
    # RLlib VectorEnv protocol
    # ------------------------------------------------------------------------------------------------
    def vector_reset(self):
        self._await_reset[:] = False
        return list(self.reset())

    def reset_at(self, index):
        """VectorEnv.reset_at: the ONE reset of env `index` (game.py:260-277).  In the rllib flow vector_step has
        already re-initialised every env it reported done, in one masked launch, and cached the reset observations;
        this call hands that observation out instead of resetting (and advancing the map) a second time."""
        index = int(index)
        if self._await_reset[index]:
            self._await_reset[index] = False
            return self._reset_obs_h[index].copy()
        self._host_reset(index, self.obs)
        return self.obs[index].cpu().numpy()

    def _keep_reset_obs(self, idx, rows):
        """rllib flow: `rows`, the reset observations of the done envs `idx`, wait for those envs' reset_at."""
        if self._reset_obs_h is None:
            self._reset_obs_h = np.empty((self.num_envs, self.states_history), dtype=np.float64)
        self._reset_obs_h[idx] = rows
        self._await_reset[idx] = True

    def _reset_done_envs(self, done_h):
        """rllib flow without in-kernel reset: re-initialise all done envs with ONE masked reset launch into a side buffer,
        leaving self.obs = the terminal observations."""
        side = _torch().empty_like(self.obs)
        self._host_reset(done_h, side)
        idx = np.nonzero(done_h)[0]
        self._keep_reset_obs(idx, self._rows_h(side, idx))

    def vector_step(self, actions):
        """VectorEnv.vector_step.  Returns (obs, rewards, dones, infos) as SEQUENCES of per-env items: numpy arrays [N, D] /
        [N] / [N] — RLlib's own adapter only enumerates them (`dict(enumerate(self.new_obs))`), and a per-row `list()` of 65 536
        rows costs more than the step — and the reused list of info dicts.  The observation array is a fresh copy: RLlib's
        sample builders keep the rows by reference."""
        if not self.rllib:
            obs, rew, done, infos = self.step(np.asarray(actions))
            return (obs if self.copy_host_outputs else obs.copy()), rew, done, infos
        if self._await_reset.any():
            raise N.ShipSimError("vector_step: envs %r were reported done and have not been reset_at()"
                                 % (np.nonzero(self._await_reset)[0][:8].tolist(),))
        obs, rew, done, infos = self.step(np.asarray(actions))
        obs = obs if self.copy_host_outputs else obs.copy()
        if done.any():
            if self._rllib_fused:
                # the step kernel has already reset the done envs: their rows of `obs` are the reset observations (kept for
                # reset_at), their terminal observations are in term_obs — no reset launch
                idx = np.nonzero(done)[0]
                self._keep_reset_obs(idx, obs[idx])
                obs[idx] = self._rows_h(self.term_obs, idx)
            else:  # no in-kernel reset underneath: obs rows of done envs are terminal; ONE masked reset for all of them
                self._reset_done_envs(done)
        return obs, rew, done, infos

    def get_unwrapped(self):
        """VectorEnv.get_unwrapped: the underlying envs, as per-env handles."""
        return [self.env(i) for i in range(self.num_envs)]
