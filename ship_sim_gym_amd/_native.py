"""ctypes binding of libshipsim.so (include/shipsim.h) — the only way the Python host reaches the HIP path.

There is no CPU fallback: if the shared library is missing this module raises at import of the symbol table,
and every compute entry point returns an error (raised as ShipSimError) when no MI355X/HIP device is usable.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SSG_LIB_PATH: development override (tools/build_variant.sh builds diagnostic variants next to the product library)
LIB_PATH = os.environ.get("SSG_LIB_PATH") or os.path.join(_HERE, "libshipsim.so")

ABI_VERSION = 9
MAX_BEAMS, MAX_GOALS, MAX_HULL, SHIP_VERTS, N_TRAFFIC = 16, 6, 12, 5, 3
MAP_STRIDE = 145
MAP_OFF_COUNTS, MAP_OFF_AABB, MAP_OFF_GOALS, MAP_OFF_SPAWN_GOAL, MAP_OFF_PLANES, PLANE_DOUBLES = 0, 2, 10, 22, 24, 5
FLAG_AUTO_RESET, FLAG_FIX_COLLISION_REWARD, FLAG_BANK_IN_GLOBAL, FLAG_EXACT_LIDAR, FLAG_DYN_MEMO_OFF = 0x1, 0x2, 0x4, 0x8, 0x10
EV_COLLIDING, EV_GOAL_REACHED, EV_OUT_OF_BOUNDS, EV_MAX_STEPS, EV_NO_GOALS_LEFT = 0x1, 0x2, 0x4, 0x8, 0x10
POLICY_MAX_HIDDEN, POLICY_TANH, POLICY_RELU = 128, 0, 1
POLICY_SEPARATE_VALUE = 0x100  # or-ed into Policy.activation / Population.activation: separate pi / vf towers
POP_MAX_MEMBERS = 256
POP_EXT_GRAD_CLIP, POP_EXT_VF_CLIP = 0x1, 0x2
PPO_EXT_STATS = 8  # stats columns of the _ext entry points
EVAL_STATS, EVAL_GREEDY = 8, 0x1  # columns of an evaluation's stats rows; ssg_eval.flags
# the columns (include/shipsim.h): episodes, llrint(100 * return), length, the four endings (not exclusive), goal events
(EVAL_EPISODES, EVAL_RETURN100, EVAL_LENGTH, EVAL_COLLIDED, EVAL_OUT_OF_BOUNDS, EVAL_MAX_STEPS, EVAL_NO_GOALS_LEFT,
 EVAL_GOALS) = range(8)
FILTER_ROWS, FILTER_UPDATE = 4, 0x1  # state rows per member of an observation filter (mean, M2, denom, count); ssg_obs_filter.flags
FILTER_TILE, FILTER_RUNS = 256, 8  # ssg_obs_filter_update's reduction order: rows per tile, runs of tiles (include/shipsim.h)
RET_FILTER_UPDATE, RET_FILTER_MAX_STEPS = 0x1, 1024  # ssg_ret_filter.flags; the largest K of one ssg_ret_filter_apply call
ADV_NORM_BATCH, ADV_NORM_MINIBATCH = 0, 1  # ssg_ppo_set_adv_norm's modes: once per rollout (the default), PPO2's per minibatch
ADV_NORM_BLOCKS, ADV_NORM_SPAN = 64, 1024  # its reduction order: workgroups at most per member, minibatch positions per workgroup below that
# the minibatch permutations (csrc/shipsim_perm.h): Feistel rounds, the bit-width floor, the cycle walk's cap, the largest row
ADV_TABLE_MAX_ROWS = 65535  # minibatches of one ssg_ppo_minibatch_adv_sums call, rows of one ssg_ppo_set_adv_table table
PERM_ROUNDS, PERM_MIN_BITS, PERM_WALK_CAP, PERM_MAX_N = 8, 8, 256, 1 << 32


def pop_table_floats(n_members, n_steps):
    """SSG_POP_TABLE_FLOATS: the floats ssg_pop_pack_hparams writes for n_members members and n_steps Adam steps."""
    return int(n_members) * 8 * (1 + int(n_steps))


POP_SLICE_ROW = 4  # int32 per member of the slices table (ssg_pop_pack_slices): first env, envs, 256-env blocks, 0
POP_SCHED_ROW = 8  # int32 per member of a schedule table's header, and per member and launch of its records
# a record's fields (include/shipsim.h): the int64 offset takes entries 0 and 1
SCHED_M, SCHED_G, SCHED_FIRST, SCHED_ACTIVE, SCHED_INVM = 2, 3, 4, 5, 6
SCHED_HDR_PREFIX = 4  # a header row's int64 (entries 4, 5) of ssg_pop_pack_schedule_samples: the samples of the members before


def pop_sched_ints(n_members, n_launches):
    """SSG_POP_SCHED_INTS: the int32 ssg_pop_pack_schedule writes for n_members members and n_launches launches."""
    return int(n_members) * POP_SCHED_ROW * (1 + int(n_launches))


(F_X, F_Y, F_VX, F_VY, F_ANGLE, F_W, F_CUM_REWARD, F_LIDAR, F_RUDDER, F_STEP_COUNT, F_MAP_ID, F_GOAL_MASK,
 F_STATS, F_TRAFFIC, F_GOAL_BODIES, F_DYN_FLAGS, F_EPISODES, F_DYN_MEMO_STATS,
 F_DYN_LIVE, F_DYN_ARB_META, F_DYN_ARB_HASH, F_DYN_ARB_IMPULSE) = range(22)
DYN_PAIRS, DYN_POLY_PAIRS = 54, 9  # arbiter rows of F_DYN_ARB_* (pair ids: include/shipsim.h)

# every symbol include/shipsim.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = (
    "ssg_abi_version", "ssg_strerror", "ssg_last_error", "ssg_create", "ssg_destroy", "ssg_default_config",
    "ssg_config_set_ship", "ssg_state_nbytes", "ssg_state_field", "ssg_bind_state", "ssg_set_map_bank", "ssg_reset",
    "ssg_step", "ssg_rollout", "ssg_fill_actions", "ssg_host_convex_hull", "ssg_host_moment_for_poly", "ssg_host_goal_x_range",
    "ssg_host_build_map", "ssg_host_segment_query", "ssg_debug_copy8", "ssg_generate_bank", "ssg_render", "ssg_dyn_invalidate",
    "ssg_init_state", "ssg_refill_worlds", "ssg_debug_launch_geometry", "ssg_rollout_traj", "ssg_debug_dyn_counters", "ssg_debug_kernel_times",
    "ssg_debug_clock_probe", "ssg_debug_launch_clock", "ssg_set_terminal_obs", "ssg_step_host", "ssg_wait_host",
    "ssg_policy_act", "ssg_rollout_policy",
    "ssg_ppo_workspace_nbytes", "ssg_ppo_gae", "ssg_ppo_grad", "ssg_ppo_adam", "ssg_ppo_update",
    "ssg_pop_act", "ssg_pop_rollout", "ssg_pop_pack_hparams", "ssg_pop_workspace_nbytes", "ssg_pop_gae", "ssg_pop_update",
    "ssg_pop_exploit", "ssg_pop_episode_stats",
    "ssg_ppo_dist", "ssg_ppo_grad_ext", "ssg_ppo_update_ext", "ssg_pop_dist", "ssg_pop_update_ext",
    "ssg_pop_pack_schedule", "ssg_pop_pack_hparams_steps", "ssg_pop_update_sched",
    "ssg_policy_act_greedy", "ssg_pop_act_greedy", "ssg_evaluate", "ssg_pop_evaluate", "ssg_eval_reduce", "ssg_eval_account",
    "ssg_pop_pack_slices", "ssg_pop_set_slices", "ssg_pop_get_slices", "ssg_pop_pack_schedule_samples",
    "ssg_obs_filter_workspace_nbytes", "ssg_obs_filter_update", "ssg_set_obs_filter", "ssg_get_obs_filter",
    "ssg_set_obs_filter_buffer", "ssg_get_obs_filter_buffer", "ssg_obs_filter_update_buffered", "ssg_obs_filter_merge_rows",
    "ssg_ret_filter_workspace_nbytes", "ssg_ret_filter_apply", "ssg_ret_filter_batches", "ssg_ret_filter_apply_rows",
    "ssg_ppo_adv_norm_nbytes", "ssg_ppo_set_adv_norm", "ssg_ppo_get_adv_norm",
    "ssg_ppo_minibatch_adv_nbytes", "ssg_ppo_minibatch_adv_sums", "ssg_ppo_set_minibatch_adv_rows",
    "ssg_ppo_set_adv_table", "ssg_ppo_select_adv_row", "ssg_ppo_get_adv_table",
    "ssg_host_perm", "ssg_ppo_perm", "ssg_pop_perm",
    "ssg_set_timeout_boot", "ssg_get_timeout_boot", "ssg_timeout_values", "ssg_pop_timeout_values", "ssg_ppo_gae_boot", "ssg_pop_gae_boot",
    "ssg_ppo_adv_moments", "ssg_ppo_set_adv_moments", "ssg_ppo_apply_shards",
    "ssg_render_envs", "ssg_set_eval_recorder", "ssg_get_eval_recorder",
    "ssg_episode_log_workspace_nbytes", "ssg_episode_log_append",
    "ssg_job_episode_log_block_nbytes", "ssg_job_episode_log_shard", "ssg_job_episode_log_merge_blocks",
    "ssg_report_clip_bounds", "ssg_ppo_report_workspace_nbytes", "ssg_ppo_report", "ssg_pop_report",
    "ssg_ppo_report_sums", "ssg_ppo_report_rows",
)
RENDER_MAX_ENVS = 4096  # frames of one ssg_render_envs launch at most
EVAL_REC_MAX_ENVS = 64  # tracked envs of an evaluation recorder at most
DP_MAX_SHARDS = 64  # ssg_ppo_shards.n_shards at most
EPISODE_LOG_MAX_CELLS = 1 << 22  # K * ceil(n_envs / 256) of one ssg_episode_log_append call at most
# the update report's record (include/shipsim.h): its f64 columns, and where the explained variance, the post-update group's flag, the
# stats rows' means and their row count sit
REPORT_COLS, REPORT_EXPLAINED_VARIANCE, REPORT_POST, REPORT_STATS, REPORT_ROWS = 24, 5, 8, 12, 20
REPORT_ROW_COLS = 12  # a shard's sum row (ssg_ppo_report_sums): the walk's nine sums, n, the post flag, 0


class ShipSimError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("device_id", C.c_int32), ("n_envs", C.c_int32),
        ("env_id_base", C.c_int64),
        ("n_beams", C.c_int32), ("history", C.c_int32), ("max_steps", C.c_int32), ("n_goals", C.c_int32),
        ("lidar_spread_deg", C.c_double), ("lidar_dist", C.c_double), ("goal_radius", C.c_double),
        ("width", C.c_double), ("height", C.c_double), ("dt", C.c_double), ("damping_pow_dt", C.c_double),
        ("spawn_x", C.c_double), ("spawn_y", C.c_double),
        ("ship_hull", C.c_double * (2 * SHIP_VERTS)), ("ship_normals", C.c_double * (2 * SHIP_VERTS)),
        ("ship_m_inv", C.c_double), ("ship_i_inv", C.c_double), ("force_y", C.c_double),
        ("thrust_px0", C.c_double), ("thrust_py0", C.c_double),
        ("rudder_step", C.c_int32), ("rudder_max", C.c_int32),
        ("n_ships", C.c_int32), ("map_ring", C.c_int32),
    ]


class Policy(C.Structure):
    """ssg_policy (ABI 9): an MLP actor-critic the device evaluates for every env (layout of dev_params: include/shipsim.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("obs_dim", C.c_int32), ("hidden", C.c_int32), ("n_hidden_layers", C.c_int32),
        ("n_actions", C.c_int32), ("activation", C.c_int32), ("dev_params", C.c_void_p), ("dev_obs_scale", C.c_void_p),
    ]


class PpoHparams(C.Structure):
    """ssg_ppo_hparams (ABI 9 addition): GAE, loss and Adam hyper-parameters of the device's PPO update."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("gamma", C.c_double), ("lam", C.c_double), ("clip", C.c_double), ("vf_coef", C.c_double),
        ("ent_coef", C.c_double), ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
        ("adv_eps", C.c_double),
    ]


class Population(C.Structure):
    """ssg_population (ABI 9 addition): P policies of one shape on one handle; dev_params is f32 [P][L], row m = member m."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_members", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32),
        ("n_hidden_layers", C.c_int32), ("n_actions", C.c_int32), ("activation", C.c_int32), ("reserved", C.c_int32),
        ("dev_params", C.c_void_p), ("dev_obs_scale", C.c_void_p),
    ]


class PpoExt(C.Structure):
    """ssg_ppo_ext (ABI 9 addition): the value clip, gradient-norm clip and KL penalty of the extended PPO update."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("vf_clip", C.c_double), ("max_grad_norm", C.c_double), ("kl_target", C.c_double),
        ("dev_kl_coef", C.c_void_p), ("dev_logp_all", C.c_void_p), ("dev_value_old", C.c_void_p),
    ]


class PopExt(C.Structure):
    """ssg_pop_ext (ABI 9 addition): the extended update's per-member constants (dev_ext f32 [P][4]) and buffers."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("dev_ext", C.c_void_p), ("dev_kl_coef", C.c_void_p),
        ("dev_logp_all", C.c_void_p), ("dev_value_old", C.c_void_p),
    ]


class Eval(C.Structure):
    """ssg_eval (ABI 9 addition): one call of the evaluation loop — mode, quota, steps, the scratch rows, carries and stats rows."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("episodes_per_env", C.c_int32), ("n_steps", C.c_int32),
        ("seed", C.c_uint64), ("step0", C.c_int64), ("dev_uniform_TN", C.c_void_p), ("dev_obs", C.c_void_p),
        ("dev_act", C.c_void_p), ("dev_logp", C.c_void_p), ("dev_value", C.c_void_p), ("dev_reward", C.c_void_p),
        ("dev_done", C.c_void_p), ("dev_flags", C.c_void_p), ("dev_carry_return", C.c_void_p), ("dev_carry", C.c_void_p),
        ("dev_env_stats", C.c_void_p),
    ]


class ObsFilterRecord(C.Structure):
    """ssg_obs_filter (ABI 9 addition): a running mean / std observation filter — mode, shape, clip / eps, the state rows, the workspace."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_int32), ("obs_dim", C.c_int32),
        ("clip", C.c_double), ("eps", C.c_double), ("dev_state", C.c_void_p), ("dev_workspace", C.c_void_p),
        ("workspace_nbytes", C.c_size_t),
    ]


class RetFilterRecord(C.Structure):
    """ssg_ret_filter (ABI 9 addition): return normalisation — mode, member count, clip / eps, the members' discounts, the state rows,
    the per-env carry, the workspace."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32), ("n_members", C.c_int32), ("reserved", C.c_int32),
        ("clip", C.c_double), ("eps", C.c_double), ("dev_gamma", C.c_void_p), ("dev_state", C.c_void_p), ("dev_carry", C.c_void_p),
        ("dev_workspace", C.c_void_p), ("workspace_nbytes", C.c_size_t),
    ]


class TimeoutBootRecord(C.Structure):
    """ssg_timeout_boot (ABI 9 addition): the time-out bootstrap's buffers — the rows they serve, the terminal observations f64
    [rows][n_envs][D], the values f32 [rows][stride]."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("rows", C.c_int32), ("dev_term_obs_KND", C.c_void_p), ("dev_boot_KN", C.c_void_p),
    ]


class EvalRecorderRecord(C.Structure):
    """ssg_eval_recorder (addition to ABI 9): the tracked envs (a HOST int32 array the library copies), the steps kept per env, the
    frame geometry, and the caller's device buffers — the trajectory rows [R][C](...), cursor / overflow [R], the terminal-observation
    scratch [n_envs][D] and the optional frames [R][ceil(C / S)][W][H][3]."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_tracked", C.c_int32), ("env_ids", C.POINTER(C.c_int32)), ("capacity", C.c_int32),
        ("frame_width", C.c_int32), ("frame_height", C.c_int32), ("frame_every", C.c_int32), ("frame_flags", C.c_uint32),
        ("reserved", C.c_uint32), ("dev_obs", C.c_void_p), ("dev_next_obs", C.c_void_p), ("dev_act", C.c_void_p),
        ("dev_logp", C.c_void_p), ("dev_value", C.c_void_p), ("dev_reward", C.c_void_p), ("dev_done", C.c_void_p),
        ("dev_flags", C.c_void_p), ("dev_cursor", C.c_void_p), ("dev_overflow", C.c_void_p), ("dev_term_obs", C.c_void_p),
        ("dev_frames", C.c_void_p),
    ]


class EpisodeRecord(C.Structure):
    """ssg_episode_record (addition to ABI 9): one finished episode, 32 bytes (episode_log.RECORD_DTYPE is the numpy view of it)."""
    _fields_ = [
        ("ret", C.c_double), ("step", C.c_int64), ("env", C.c_int32), ("length", C.c_int32), ("goals", C.c_int32), ("end", C.c_uint32),
    ]


class EpisodeLogRecord(C.Structure):
    """ssg_episode_log (addition to ABI 9): the ring [capacity] of ssg_episode_record and its head int64 [2], the per-env carries (f64
    [n_envs]; int32 [n_envs][2]) and the workspace — all the caller's, on the device."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_members", C.c_int32), ("capacity", C.c_int64), ("dev_records", C.c_void_p),
        ("dev_head", C.c_void_p), ("dev_carry_return", C.c_void_p), ("dev_carry", C.c_void_p), ("dev_workspace", C.c_void_p),
        ("workspace_nbytes", C.c_size_t),
    ]


class PpoShards(C.Structure):
    """ssg_ppo_shards (ABI 9 addition): the gathered rows of one data-parallel minibatch — W, the device rows f32 [W][P + 8], the HOST
    counts int64 [W], the chunk's place in its epoch and update, and the adaptation's divisor."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_shards", C.c_int32), ("dev_rows", C.c_void_p), ("counts", C.POINTER(C.c_int64)),
        ("first_chunk", C.c_int32), ("last_chunk", C.c_int32), ("n_chunks", C.c_int32), ("reserved", C.c_int32),
    ]


def is_timeout(flags):
    """The time-out predicate of include/shipsim.h on a flags byte (an int, or a numpy / torch integer array): the clock ended the
    episode (EV_MAX_STEPS) and no true terminal did (EV_COLLIDING, EV_OUT_OF_BOUNDS, EV_NO_GOALS_LEFT); EV_GOAL_REACHED does not matter."""
    return ((flags & EV_MAX_STEPS) != 0) & ((flags & (EV_COLLIDING | EV_OUT_OF_BOUNDS | EV_NO_GOALS_LEFT)) == 0)


_lib = None


def lib():
    """Load libshipsim.so (built in-tree by __graft_entry__.build() / csrc/Makefile).  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ShipSimError(
            "libshipsim.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ship_sim_gym_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    # libshipsim.so needs libamdhip64.so.7.  PyTorch-ROCm bundles its own copy of that runtime (same SONAME) and
    # is the owner of the device memory and streams we are handed, so torch must be imported FIRST: the dynamic
    # loader then binds our HIP calls to the runtime already in the process instead of mapping a second one from
    # /opt/rocm (two HIP runtimes in one process cannot share streams and fail at the first hipGetDevice).
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, dp, i32p, u8p, szp, ip = (C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_int))
    L.ssg_abi_version.restype = C.c_int
    L.ssg_strerror.restype = C.c_char_p
    L.ssg_strerror.argtypes = [C.c_int]
    L.ssg_last_error.restype = C.c_char_p
    L.ssg_last_error.argtypes = [vp]
    L.ssg_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.ssg_destroy.argtypes = [vp]
    L.ssg_default_config.argtypes = [C.POINTER(Config)]
    L.ssg_config_set_ship.argtypes = [C.POINTER(Config), C.c_double, C.c_double, C.c_double]
    L.ssg_state_nbytes.argtypes = [vp, szp]
    L.ssg_state_field.argtypes = [vp, C.c_int, szp, ip, ip, szp]
    L.ssg_bind_state.argtypes = [vp, vp]
    L.ssg_init_state.argtypes = [vp, vp]
    L.ssg_debug_launch_geometry.argtypes = [vp, ip, ip, szp]
    L.ssg_debug_kernel_times.argtypes = [vp, C.c_int, dp, dp, C.POINTER(C.c_uint64)]
    L.ssg_debug_dyn_counters.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ssg_refill_worlds.argtypes = [vp, C.c_uint64, C.c_double, vp, vp]
    L.ssg_set_map_bank.argtypes = [vp, vp, C.c_int]
    L.ssg_reset.argtypes = [vp, vp, vp, vp, vp]
    L.ssg_step.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.ssg_rollout.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    L.ssg_rollout_traj.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, C.c_int64, vp]
    L.ssg_fill_actions.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp]
    L.ssg_generate_bank.argtypes = [vp, C.c_uint64, C.c_double, vp, C.c_int, vp, vp]
    L.ssg_debug_copy8.argtypes = [vp, vp, C.c_size_t, vp]
    L.ssg_debug_clock_probe.argtypes = [vp, C.c_int, C.c_int, vp]
    L.ssg_debug_launch_clock.argtypes = [vp, vp]
    L.ssg_set_terminal_obs.argtypes = [vp, vp]
    L.ssg_step_host.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp]
    L.ssg_wait_host.argtypes = [vp, C.c_int]
    L.ssg_policy_act.argtypes = [vp, C.POINTER(Policy), vp, vp, C.c_uint64, C.c_int64, vp, vp, vp, vp, vp]
    L.ssg_rollout_policy.argtypes = [vp, C.POINTER(Policy), C.c_int, vp, C.c_uint64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                     C.c_int64, vp]
    L.ssg_ppo_workspace_nbytes.argtypes = [C.POINTER(Policy), C.c_int64, C.c_int64, szp]
    L.ssg_ppo_gae.argtypes = [vp, C.POINTER(PpoHparams), C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.ssg_ppo_grad.argtypes = [vp, C.POINTER(Policy), C.POINTER(PpoHparams), C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp,
                               C.c_size_t, vp]
    L.ssg_ppo_adam.argtypes = [vp, C.POINTER(Policy), C.POINTER(PpoHparams), vp, vp, C.c_int64, vp]
    L.ssg_ppo_update.argtypes = [vp, C.POINTER(Policy), C.POINTER(PpoHparams), C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp,
                                 C.c_int64, vp, vp, C.c_size_t, vp]
    pp, hp = C.POINTER(Population), C.POINTER(PpoHparams)
    L.ssg_pop_act.argtypes = [vp, pp, vp, vp, C.c_uint64, C.c_int64, vp, vp, vp, vp, vp]
    L.ssg_pop_rollout.argtypes = [vp, pp, C.c_int, vp, C.c_uint64, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp]
    L.ssg_pop_pack_hparams.argtypes = [C.c_int, hp, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    L.ssg_pop_workspace_nbytes.argtypes = [pp, C.c_int64, C.c_int64, szp]
    L.ssg_pop_gae.argtypes = [vp, pp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.ssg_pop_update.argtypes = [vp, pp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_size_t, vp]
    L.ssg_pop_exploit.argtypes = [vp, pp, i32p, vp, vp]
    L.ssg_pop_episode_stats.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    xp, qp = C.POINTER(PpoExt), C.POINTER(PopExt)
    L.ssg_ppo_dist.argtypes = [vp, C.POINTER(Policy), C.c_int64, vp, vp, vp]
    L.ssg_ppo_grad_ext.argtypes = [vp, C.POINTER(Policy), hp, xp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, C.c_size_t, vp]
    L.ssg_ppo_update_ext.argtypes = [vp, C.POINTER(Policy), hp, xp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp,
                                     vp, C.c_size_t, vp]
    L.ssg_pop_dist.argtypes = [vp, pp, C.c_int, vp, vp, vp]
    L.ssg_pop_update_ext.argtypes = [vp, pp, qp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_size_t, vp]
    L.ssg_pop_pack_schedule.argtypes = [C.c_int, C.c_int64, i32p, i32p, i32p, C.c_size_t, i32p, i32p]
    L.ssg_pop_pack_hparams_steps.argtypes = [C.c_int, hp, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_float), C.c_size_t]
    L.ssg_pop_update_sched.argtypes = [vp, pp, qp, vp, C.c_int, vp, i32p, i32p, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                       C.c_size_t, vp]
    L.ssg_pop_pack_slices.argtypes = [C.c_int, i32p, i32p, C.c_size_t]
    L.ssg_pop_set_slices.argtypes = [vp, C.c_int, i32p, vp]
    L.ssg_pop_get_slices.argtypes = [vp, ip, i32p]
    L.ssg_pop_pack_schedule_samples.argtypes = [C.c_int, C.POINTER(C.c_int64), i32p, i32p, i32p, C.c_size_t, i32p, i32p]
    L.ssg_policy_act_greedy.argtypes = [vp, C.POINTER(Policy), vp, vp, vp, vp, vp, vp]
    L.ssg_pop_act_greedy.argtypes = [vp, pp, vp, vp, vp, vp, vp, vp]
    L.ssg_evaluate.argtypes = [vp, C.POINTER(Policy), C.POINTER(Eval), vp]
    L.ssg_pop_evaluate.argtypes = [vp, pp, C.POINTER(Eval), vp]
    L.ssg_eval_reduce.argtypes = [vp, C.c_int, vp, vp, vp]
    L.ssg_eval_account.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.ssg_obs_filter_workspace_nbytes.argtypes = [C.c_int, C.c_int, C.c_int, szp]
    L.ssg_obs_filter_update.argtypes = [vp, C.POINTER(ObsFilterRecord), vp, vp]
    L.ssg_set_obs_filter.argtypes = [vp, C.POINTER(ObsFilterRecord)]
    L.ssg_get_obs_filter.argtypes = [vp, C.POINTER(ObsFilterRecord)]
    L.ssg_set_obs_filter_buffer.argtypes = [vp, vp]
    L.ssg_get_obs_filter_buffer.argtypes = [vp, C.POINTER(vp)]
    L.ssg_obs_filter_update_buffered.argtypes = [vp, C.POINTER(ObsFilterRecord), vp, vp, vp]
    L.ssg_obs_filter_merge_rows.argtypes = [vp, C.POINTER(ObsFilterRecord), vp, vp, C.c_int, vp]
    L.ssg_ret_filter_workspace_nbytes.argtypes = [C.c_int, C.c_int, C.c_int, szp]
    L.ssg_ret_filter_apply.argtypes = [vp, C.POINTER(RetFilterRecord), C.c_int, vp, vp, C.c_int64, vp, vp, vp]
    L.ssg_ret_filter_batches.argtypes = [vp, C.POINTER(RetFilterRecord), C.c_int, vp, vp, C.c_int64, vp, vp]
    L.ssg_ret_filter_apply_rows.argtypes = [vp, C.POINTER(RetFilterRecord), C.c_int, vp, C.c_int, vp, C.c_int64, vp, vp, vp]
    L.ssg_ppo_adv_norm_nbytes.argtypes = [C.c_int, szp]
    L.ssg_ppo_set_adv_norm.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t]
    L.ssg_ppo_get_adv_norm.argtypes = [vp, ip, ip]
    L.ssg_ppo_minibatch_adv_nbytes.argtypes = [C.c_int, szp]
    L.ssg_ppo_minibatch_adv_sums.argtypes = [vp, C.c_int64, vp, vp, C.c_int, C.c_int64, C.c_int64, vp, vp, C.c_size_t, vp]
    L.ssg_ppo_set_minibatch_adv_rows.argtypes = [vp, C.c_int, C.c_int, vp, C.c_double, vp, vp]
    L.ssg_ppo_set_adv_table.argtypes = [vp, vp, C.c_int]
    L.ssg_ppo_select_adv_row.argtypes = [vp, C.c_int]
    L.ssg_ppo_get_adv_table.argtypes = [vp, C.POINTER(vp), ip, ip]
    L.ssg_host_perm.argtypes = [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    L.ssg_ppo_perm.argtypes = [vp, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int64, vp, vp]
    L.ssg_pop_perm.argtypes = [vp, C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.ssg_set_timeout_boot.argtypes = [vp, C.POINTER(TimeoutBootRecord)]
    L.ssg_get_timeout_boot.argtypes = [vp, C.POINTER(TimeoutBootRecord)]
    L.ssg_timeout_values.argtypes = [vp, C.POINTER(Policy), C.c_int, vp, vp, vp, C.c_int64, vp]
    L.ssg_pop_timeout_values.argtypes = [vp, pp, C.c_int, vp, vp, vp, C.c_int64, vp]
    L.ssg_ppo_gae_boot.argtypes = [vp, C.POINTER(PpoHparams), C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.ssg_pop_gae_boot.argtypes = [vp, pp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.ssg_ppo_adv_moments.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    L.ssg_ppo_set_adv_moments.argtypes = [vp, C.c_int, vp, C.c_double, vp, C.c_size_t, vp]
    L.ssg_ppo_apply_shards.argtypes = [vp, C.POINTER(Policy), hp, xp, C.POINTER(PpoShards), vp, C.c_int64, vp, vp, C.c_size_t, vp]
    L.ssg_render.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, vp]
    L.ssg_render_envs.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, vp]
    L.ssg_set_eval_recorder.argtypes = [vp, C.POINTER(EvalRecorderRecord)]
    L.ssg_get_eval_recorder.argtypes = [vp, C.POINTER(EvalRecorderRecord)]
    L.ssg_episode_log_workspace_nbytes.argtypes = [C.c_int, C.c_int, szp]
    L.ssg_episode_log_append.argtypes = [vp, C.POINTER(EpisodeLogRecord), C.c_int, C.c_int64, vp, vp, vp, C.c_int64, vp]
    L.ssg_job_episode_log_block_nbytes.argtypes = [C.c_int, C.c_int, szp]
    L.ssg_job_episode_log_shard.argtypes = [vp, C.POINTER(EpisodeLogRecord), C.c_int, C.c_int64, vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp,
                                            C.c_size_t, vp]
    L.ssg_job_episode_log_merge_blocks.argtypes = [vp, C.POINTER(EpisodeLogRecord), C.c_int, C.c_int64, C.c_int, C.c_int, vp, C.c_int, vp]
    L.ssg_report_clip_bounds.argtypes = [C.c_double, C.POINTER(C.c_float)]
    L.ssg_ppo_report_workspace_nbytes.argtypes = [C.c_int, C.c_int, szp]
    L.ssg_ppo_report.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp]
    L.ssg_pop_report.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_size_t, vp, vp]
    L.ssg_ppo_report_sums.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, vp, C.c_size_t, vp, vp]
    L.ssg_ppo_report_rows.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.ssg_dyn_invalidate.argtypes = [vp, vp, vp]
    L.ssg_host_convex_hull.argtypes = [C.c_int, dp, dp, ip]
    L.ssg_host_moment_for_poly.argtypes = [C.c_double, C.c_int, dp, dp]
    L.ssg_host_goal_x_range.argtypes = [dp, C.c_double, C.c_double, dp, dp, ip]
    L.ssg_host_build_map.argtypes = [dp, C.c_int, dp, C.c_int, dp, C.c_int, C.c_double, C.c_double, dp]
    L.ssg_host_segment_query.argtypes = [dp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, ip,
                                         dp, dp, dp]
    for name in EXPORTS:
        getattr(L, name)  # AttributeError here = a declared entry point is not exported
    if L.ssg_abi_version() != ABI_VERSION:
        raise ShipSimError("libshipsim.so ABI %d != binding ABI %d" % (L.ssg_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc, handle=None, what=""):
    if rc != 0:
        L = lib()
        msg = L.ssg_last_error(handle).decode() if handle is not None else L.ssg_last_error(None).decode()
        raise ShipSimError("%s failed: %s (%s)" % (what or "libshipsim call", L.ssg_strerror(rc).decode(), msg))


def call(name, *args, handle=None):
    """THE checked library call: the export `name` on `args`, then check(rc, handle, name).  Every export has its argtypes declared
    (lib(); tests/test_abi.py), pointers as c_void_p, so an address goes in as a plain integer (``t.data_ptr()``) and None as NULL.
    As it stands it serves the queries that take no handle; ShipVecEnv.call / ShipVecEnv.enqueue put the handle in front."""
    check(getattr(lib(), name)(*args), handle, name)


def nbytes(name, *args):
    """A ``*_nbytes`` query: `name` on `args` and a size_t out-parameter, whose value is returned."""
    need = C.c_size_t()
    call(name, *args, C.byref(need))
    return need.value


def ptr(t):
    """A tensor's address as a pointer argument of a C call; None stays None (NULL)."""
    return None if t is None else t.data_ptr()


def _torch():
    """THE import point of torch for the host layer: at first use, so that the host-only parts import without it."""
    import torch
    return torch


def arg(t, dtypes, shape, what, device, more_rows=False, exc=ValueError):
    """THE check of a tensor argument: `t` is what the C call will read it as — of `dtypes` (one dtype or a tuple of them), of `shape`
    (an int: that many elements, in any shape; a tuple: exactly that shape, or with more_rows a first dimension of at least shape[0]),
    contiguous and on `device` — or `exc` is raised, naming the call and the argument (`what`), what was expected and what was got.
    Returns the tensor's address, a plain integer."""
    if ((t.dtype is dtypes or (type(dtypes) is tuple and t.dtype in dtypes)) and t.device == device and t.is_contiguous()
            and (t.numel() == shape if type(shape) is int else
                 t.dim() == len(shape) and tuple(t.shape[1:]) == tuple(shape[1:])
                 and (t.shape[0] >= shape[0] if more_rows else t.shape[0] == shape[0]))):
        return t.data_ptr()
    want = "%d elements" % shape if type(shape) is int else "shape [%s]" % ", ".join(
        [(">= %d" if more_rows else "%d") % shape[0]] + ["%d" % s for s in shape[1:]])
    names = " / ".join(str(d) for d in (dtypes if type(dtypes) is tuple else (dtypes,)))
    raise exc("%s must be a contiguous %s tensor of %s on %s (got %s %s on %s, strides %s)"
              % (what, names, want, device, t.dtype, tuple(t.shape), t.device, tuple(t.stride())))


def default_config():
    c = Config()
    call("ssg_default_config", C.byref(c))
    return c
