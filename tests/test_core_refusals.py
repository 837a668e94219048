"""Every refusal, needing no device, of the handle's core — ssg_create (every limit), ssg_bind_state, ssg_set_map_bank, ssg_init_state,
ssg_reset, ssg_step, ssg_rollout, ssg_rollout_traj, ssg_step_host, ssg_wait_host, ssg_refill_worlds, ssg_dyn_invalidate,
ssg_generate_bank (bad arguments only), ssg_set_terminal_obs, ssg_state_field, ssg_state_nbytes and the three ssg_debug_* getters —
pinned, together with their valid calls that run on the host alone.  CASES is a table in the form of test_layout_refusals.py: the
call, the return code, the whole ssg_last_error text, and for the getters what they wrote into their outputs (each starts as -7, so a
refused call shows that it wrote nothing).  The literals were recorded from the library as it was before the handle's blob layout, dyn
queue, memo and ring state each came to live behind one type; the file passes unchanged against both.

The handle is test_update_refusals.handle's kind: a made-up bound blob and made-up device addresses, here 256 envs and 8 beams.  Its
state is a "+"-joined list: "null" | "unbound", or config words ("ring": map_ring 2, "cfg4": n_ships 4, "hist3": history 3,
"noreset": no SSG_FLAG_AUTO_RESET, "device1": the handle's device is 1, the current one 0) followed by "bound" (the blob) and "bank"
(4 records; n_envs * 2 of them in ring mode).  Only rows refused before hipGetDevice is asked, plus the host-only valid calls: nothing
ever reaches a device.  What lies behind check_ready is in test_core_refusals_gpu.py, which runs this file's machinery.  No GPU."""
import ctypes as C

import pytest

import test_update_refusals as R

Q = R.Q
N_ENVS, BEAMS, RING = 256, 8, 2
UNSET = -7  # what every output of a getter holds before the call

CONFIG_WORDS = {"ring": ("map_ring", RING), "cfg4": ("n_ships", 4), "hist3": ("history", 3), "noreset": ("flags", 0), "device1": ("device_id", 1)}


def config(native, overrides=()):
    c = native.default_config()
    c.n_envs, c.n_beams = N_ENVS, BEAMS
    for k, v in dict(overrides).items():
        setattr(c, k, float(v) if isinstance(v, str) else v)
    return c


def handle(native, state, base=Q):
    words = state.split("+")
    if words[0] in ("null", "create"):  # ("create": ssg_create's own rows take no handle)
        return None
    L = native.lib()
    h = C.c_void_p()
    c = config(native, dict(CONFIG_WORDS[w] for w in words if w in CONFIG_WORDS))
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if "bound" in words:  # (host only: the addresses are recorded, never touched before a launch)
        native.check(L.ssg_bind_state(h, C.c_void_p(base)), h)
    if "bank" in words:
        native.check(L.ssg_set_map_bank(h, C.c_void_p(base), N_ENVS * RING if "ring" in words else 4), h)
    assert set(words) <= set(CONFIG_WORDS) | {"unbound", "bound", "bank"}, state
    return h


def call(native, entry, h, base=Q, **a):
    """(return code, outputs) of `entry` on handle h.  A pointer of the call: 0 = NULL, absent = the base address (the reset's mask and
    map ids, the invalidate's mask and the raw-draw buffers: absent = NULL); the getters' outputs: absent = a variable holding UNSET."""
    L = native.lib()

    def ptr(name, default=base):
        v = a.get(name, default)
        return C.c_void_p(v) if v else None
    outs = []

    def out(name, ctype):
        if a.get(name, 1) == 0:
            return None
        outs.append(ctype(UNSET))
        return C.byref(outs[-1])
    step_out = lambda: [ptr(k) for k in ("obs", "rew", "done", "flags")]  # noqa: E731
    if entry == "ssg_create":
        c, made = config(native, a.get("cfg") or {}), C.c_void_p()
        rc = L.ssg_create(C.byref(c) if a.get("cfg", {}) is not None else None, C.byref(made) if a.get("out", 1) else None)
        if rc == 0:
            L.ssg_destroy(made)
    elif entry == "ssg_bind_state":
        rc = L.ssg_bind_state(h, ptr("state"))
    elif entry == "ssg_set_map_bank":
        rc = L.ssg_set_map_bank(h, ptr("bank"), a.get("n_maps", 4))
    elif entry == "ssg_init_state":
        rc = L.ssg_init_state(h, None)
    elif entry == "ssg_reset":
        rc = L.ssg_reset(h, ptr("mask", 0), ptr("map_ids", 0), ptr("obs"), None)
    elif entry == "ssg_step":
        rc = L.ssg_step(h, ptr("act"), *step_out(), None)
    elif entry == "ssg_rollout":
        rc = L.ssg_rollout(h, ptr("act"), a.get("K", 2), *step_out(), None)
    elif entry == "ssg_rollout_traj":
        rc = L.ssg_rollout_traj(h, ptr("act"), a.get("K", 2), *step_out(), a.get("stride", N_ENVS), None)
    elif entry == "ssg_step_host":
        host_act, host_block = (C.c_int32 * N_ENVS)(), (C.c_uint8 * 64)()
        rc = L.ssg_step_host(h, host_act if a.get("host_act", 1) else None, ptr("act"), *step_out(), ptr("block"),
                             host_block if a.get("host_block", 1) else None, a.get("block_bytes", 64), a.get("slot", 0), None)
    elif entry == "ssg_wait_host":
        rc = L.ssg_wait_host(h, a.get("slot", 0))
    elif entry == "ssg_refill_worlds":
        rc = L.ssg_refill_worlds(h, 1, float(a.get("width_frac", 0.5)), ptr("raw", 0), None)
    elif entry == "ssg_dyn_invalidate":
        rc = L.ssg_dyn_invalidate(h, ptr("mask", 0), None)
    elif entry == "ssg_generate_bank":
        rc = L.ssg_generate_bank(h, 1, float(a.get("width_frac", 0.5)), ptr("bank"), a.get("n_maps", 4), ptr("raw", 0), None)
    elif entry == "ssg_set_terminal_obs":
        rc = L.ssg_set_terminal_obs(h, ptr("term"))
    elif entry == "ssg_rollout_policy":  # (the GPU twin's: it consults the device first)
        pol = R.policy(native, base, {"obs_dim": 2 * (6 + BEAMS)})
        rc = L.ssg_rollout_policy(h, pol, a.get("K", 2), ptr("uniform"), 7, 0, ptr("obs"), ptr("act"), ptr("logp"), ptr("value"), ptr("x"),
                                  ptr("rew"), ptr("done"), ptr("flags"), ptr("last"), a.get("stride", N_ENVS), None)
    elif entry == "ssg_state_nbytes":
        rc = L.ssg_state_nbytes(h, out("nbytes", C.c_size_t))
    elif entry == "ssg_state_field":
        rc = L.ssg_state_field(h, a.get("field", 0), out("offset", C.c_size_t), out("elem_size", C.c_int), out("n_columns", C.c_int),
                               out("stride_bytes", C.c_size_t))
    elif entry == "ssg_debug_launch_geometry":
        rc = L.ssg_debug_launch_geometry(h, out("epw", C.c_int), out("in_lds", C.c_int), out("lds_bytes", C.c_size_t))
    elif entry == "ssg_debug_kernel_times":
        rc = L.ssg_debug_kernel_times(h, a.get("enable", 0), out("dyn_us", C.c_double), out("step_us", C.c_double), out("steps", C.c_uint64))
    else:
        assert entry == "ssg_debug_dyn_counters", entry
        rc = L.ssg_debug_dyn_counters(h, out("full_steps", C.c_uint64), out("rebuilds", C.c_uint64))
    return rc, [C.c_int64(int(o.value)).value if not isinstance(o, C.c_double) else o.value for o in outs]


def outcome(native, entry, state, kw, base=Q):
    """(return code, ssg_last_error text, outputs) of one case.  As in test_layout_refusals.outcome a refusal of something else is made
    first: a call that leaves no message of its own shows that one's text ("ssg_ppo_set_adv_norm: ...") and never a stale one."""
    L = native.lib()
    h = handle(native, state, base)
    try:
        assert L.ssg_ppo_set_adv_norm(h, 9, 0, None, 0) == -1
        rc, outs = call(native, entry, h, base, **kw)
        return rc, L.ssg_last_error(h).decode(), outs
    finally:
        if h is not None:
            L.ssg_destroy(h)


HOST_ONLY = ("ssg_create", "ssg_bind_state", "ssg_set_map_bank", "ssg_set_terminal_obs", "ssg_state_field", "ssg_state_nbytes",
             "ssg_debug_launch_geometry", "ssg_debug_kernel_times", "ssg_debug_dyn_counters")  # a valid call of these launches nothing
SUBJECTS = HOST_ONLY + ("ssg_init_state", "ssg_reset", "ssg_step", "ssg_rollout", "ssg_rollout_traj", "ssg_step_host", "ssg_wait_host",
                        "ssg_refill_worlds", "ssg_dyn_invalidate", "ssg_generate_bank")

# (entry point, the handle's state, what the call is made with, return code, ssg_last_error, the getters' outputs)
CASES = [
    ('ssg_create', 'create', {'cfg': None}, -1, 'ssg_create: NULL argument', []),
    ('ssg_create', 'create', {'out': 0}, -1, 'ssg_create: NULL argument', []),
    ('ssg_create', 'create', {'cfg': None, 'out': 0}, -1, 'ssg_create: NULL argument', []),
    ('ssg_create', 'create', {'cfg': {'struct_size': 8}}, -1, 'ssg_create: struct_size mismatch', []),
    ('ssg_create', 'create', {'cfg': {'struct_size': 0}}, -1, 'ssg_create: struct_size mismatch', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': 0}}, -1, 'ssg_create: n_envs must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': -5}}, -1, 'ssg_create: n_envs must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'n_beams': 0}}, -4, 'ssg_create: n_beams must be in 1..16', []),
    ('ssg_create', 'create', {'cfg': {'n_beams': 17}}, -4, 'ssg_create: n_beams must be in 1..16', []),
    ('ssg_create', 'create', {'cfg': {'n_beams': -1}}, -4, 'ssg_create: n_beams must be in 1..16', []),
    ('ssg_create', 'create', {'cfg': {'history': 0}}, -1, 'history_size must be greater than zero', []),
    ('ssg_create', 'create', {'cfg': {'history': -1}}, -1, 'history_size must be greater than zero', []),
    ('ssg_create', 'create', {'cfg': {'history': 9}}, -4, 'ssg_create: history must be <= 8', []),
    ('ssg_create', 'create', {'cfg': {'n_goals': 0}}, -4, 'ssg_create: n_goals must be in 1..6', []),
    ('ssg_create', 'create', {'cfg': {'n_goals': 7}}, -4, 'ssg_create: n_goals must be in 1..6', []),
    ('ssg_create', 'create', {'cfg': {'dt': 0.0}}, -1, 'ssg_create: dt must be > 0', []),
    ('ssg_create', 'create', {'cfg': {'dt': -1.0}}, -1, 'ssg_create: dt must be > 0', []),
    ('ssg_create', 'create', {'cfg': {'dt': 'nan'}}, -1, 'ssg_create: dt must be > 0', []),
    ('ssg_create', 'create', {'cfg': {'max_steps': 0}}, -1, 'ssg_create: max_steps must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'max_steps': -3}}, -1, 'ssg_create: max_steps must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 2}}, -4, 'ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 3}}, -4, 'ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 5}}, -4, 'ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': -1}}, -4, 'ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 1}}, -4, 'ssg_create: map_ring must be 0 or in 2..128', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 129}}, -4, 'ssg_create: map_ring must be 0 or in 2..128', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': -1}}, -4, 'ssg_create: map_ring must be 0 or in 2..128', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': -128}}, -4, 'ssg_create: map_ring must be 0 or in 2..128', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': 200000, 'map_ring': 128}}, -4, 'ssg_create: n_envs * map_ring * SSG_MAP_STRIDE must be < 2^31 (use a smaller ring, or shard the envs over more handles)', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': 115705, 'map_ring': 128}}, -4, 'ssg_create: n_envs * map_ring * SSG_MAP_STRIDE must be < 2^31 (use a smaller ring, or shard the envs over more handles)', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': 115704, 'map_ring': 128, 'history': 3}}, -4, 'ssg_create: map_ring needs history <= 2', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 2, 'history': 3}}, -4, 'ssg_create: map_ring needs history <= 2', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 128, 'history': 8}}, -4, 'ssg_create: map_ring needs history <= 2', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 4, 'flags': 9}}, -4, 'ssg_create: SSG_FLAG_EXACT_LIDAR is not built for n_ships = 4', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 1, 'flags': 9}}, 0, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_create', 'create', {'cfg': {'struct_size': 8, 'n_envs': 0}}, -1, 'ssg_create: struct_size mismatch', []),
    ('ssg_create', 'create', {'cfg': {'n_envs': 0, 'n_beams': 17}}, -1, 'ssg_create: n_envs must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'n_beams': 17, 'history': 0}}, -4, 'ssg_create: n_beams must be in 1..16', []),
    ('ssg_create', 'create', {'cfg': {'history': 0, 'n_goals': 7}}, -1, 'history_size must be greater than zero', []),
    ('ssg_create', 'create', {'cfg': {'history': 9, 'n_goals': 7}}, -4, 'ssg_create: history must be <= 8', []),
    ('ssg_create', 'create', {'cfg': {'n_goals': 7, 'dt': 0.0}}, -4, 'ssg_create: n_goals must be in 1..6', []),
    ('ssg_create', 'create', {'cfg': {'dt': 0.0, 'max_steps': 0}}, -1, 'ssg_create: dt must be > 0', []),
    ('ssg_create', 'create', {'cfg': {'max_steps': 0, 'n_ships': 2}}, -1, 'ssg_create: max_steps must be >= 1', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 2, 'map_ring': 1}}, -4, 'ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 129, 'history': 3}}, -4, 'ssg_create: map_ring must be 0 or in 2..128', []),
    ('ssg_create', 'create', {'cfg': {'map_ring': 2, 'history': 3, 'n_ships': 4, 'flags': 9}}, -4, 'ssg_create: map_ring needs history <= 2', []),
    ('ssg_create', 'create', {}, 0, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 0}}, 0, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_create', 'create', {'cfg': {'n_ships': 4, 'map_ring': 128, 'history': 2, 'n_beams': 16, 'n_goals': 6}}, 0, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_create', 'create', {'cfg': {'history': 8, 'n_beams': 1, 'n_goals': 1, 'max_steps': 1}}, 0, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_bind_state', 'null', {}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'null', {'state': 0}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'null', {'state': 196624}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'null', {'state': 196736}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_bind_state', 'unbound', {'state': 0}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'unbound', {'state': 196624}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_bind_state', 'unbound', {'state': 196736}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_bind_state', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_bind_state', 'bound+bank', {'state': 0}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'bound+bank', {'state': 196624}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_bind_state', 'bound+bank', {'state': 196736}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_bind_state', 'cfg4+bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_bind_state', 'cfg4+bound', {'state': 0}, -1, 'ssg_bind_state: NULL argument', []),
    ('ssg_bind_state', 'cfg4+bound', {'state': 196624}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_bind_state', 'cfg4+bound', {'state': 196736}, -1, 'ssg_bind_state: state blob must be 256-byte aligned', []),
    ('ssg_set_map_bank', 'null', {}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'bank': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'n_maps': -1}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'bank': 0, 'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'n_maps': 14810233}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'n_maps': 14810232}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'bank': 196616}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'bank': 196616, 'n_maps': 14810233}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'null', {'bank': 196624}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'unbound', {'bank': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'unbound', {'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'unbound', {'n_maps': -1}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'unbound', {'bank': 0, 'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'unbound', {'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'unbound', {'n_maps': 14810232}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'unbound', {'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'unbound', {'bank': 196616, 'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'unbound', {'bank': 196624}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound', {'bank': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound', {'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound', {'n_maps': -1}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound', {'bank': 0, 'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound', {'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'bound', {'n_maps': 14810232}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound', {'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'bound', {'bank': 196616, 'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'bound', {'bank': 196624}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound+bank', {'bank': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound+bank', {'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound+bank', {'n_maps': -1}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound+bank', {'bank': 0, 'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'bound+bank', {'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'bound+bank', {'n_maps': 14810232}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'bound+bank', {'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'bound+bank', {'bank': 196616, 'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'bound+bank', {'bank': 196624}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'cfg4+bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'bank': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'n_maps': -1}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'bank': 0, 'n_maps': 0}, -1, 'ssg_set_map_bank: bad argument', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'n_maps': 14810232}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'bank': 196616, 'n_maps': 14810233}, -4, 'ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31', []),
    ('ssg_set_map_bank', 'cfg4+bound', {'bank': 196624}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'ring+unbound', {'n_maps': 4}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+unbound', {'n_maps': 512}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'ring+unbound', {'n_maps': 513}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+unbound', {'n_maps': 512, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+unbound', {'n_maps': 4, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+bound', {'n_maps': 4}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+bound', {'n_maps': 512}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'ring+bound', {'n_maps': 513}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+bound', {'n_maps': 512, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+bound', {'n_maps': 4, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+bound+bank', {'n_maps': 4}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+bound+bank', {'n_maps': 512}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'ring+bound+bank', {'n_maps': 513}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+bound+bank', {'n_maps': 512, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+bound+bank', {'n_maps': 4, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+cfg4+bound', {'n_maps': 4}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+cfg4+bound', {'n_maps': 512}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_map_bank', 'ring+cfg4+bound', {'n_maps': 513}, -1, 'ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring', []),
    ('ssg_set_map_bank', 'ring+cfg4+bound', {'n_maps': 512, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_set_map_bank', 'ring+cfg4+bound', {'n_maps': 4, 'bank': 196616}, -1, 'ssg_set_map_bank: bank must be 16-byte aligned', []),
    ('ssg_init_state', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_init_state', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_init_state', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_init_state', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_reset', 'null', {'obs': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_reset', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'unbound', {'obs': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'cfg4+unbound', {'obs': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'ring+unbound', {'obs': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'bound', {'obs': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'cfg4+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'cfg4+bound', {'obs': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'ring+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'ring+bound', {'obs': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'hist3+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'hist3+bound', {'obs': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'null', {'map_ids': 196608}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_reset', 'unbound', {'map_ids': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'cfg4+unbound', {'map_ids': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'ring+unbound', {'map_ids': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_reset', 'bound', {'map_ids': 196608}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'cfg4+bound', {'map_ids': 196608}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'ring+bound', {'map_ids': 196608}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_reset', 'hist3+bound', {'map_ids': 196608}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_step', 'null', {'act': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_step', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'unbound', {'act': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'cfg4+unbound', {'act': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'ring+unbound', {'act': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step', 'bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'bound', {'act': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'cfg4+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'cfg4+bound', {'act': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'ring+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'ring+bound', {'act': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'hist3+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'hist3+bound', {'act': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_rollout', 'null', {'K': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_rollout', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'unbound', {'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'cfg4+unbound', {'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'ring+unbound', {'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout', 'bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'bound', {'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'cfg4+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'cfg4+bound', {'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'ring+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'ring+bound', {'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'hist3+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'hist3+bound', {'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_rollout_traj', 'null', {'stride': 1}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_rollout_traj', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'unbound', {'stride': 1}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'cfg4+unbound', {'stride': 1}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'ring+unbound', {'stride': 1}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'bound', {'stride': 1}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'cfg4+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'cfg4+bound', {'stride': 1}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'ring+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'ring+bound', {'stride': 1}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'hist3+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'hist3+bound', {'stride': 1}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'null', {'obs': 0, 'K': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_rollout_traj', 'unbound', {'obs': 0, 'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'cfg4+unbound', {'obs': 0, 'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'ring+unbound', {'obs': 0, 'K': 0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_rollout_traj', 'bound', {'obs': 0, 'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'cfg4+bound', {'obs': 0, 'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'ring+bound', {'obs': 0, 'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'hist3+bound', {'obs': 0, 'K': 0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_refill_worlds', 'null', {'width_frac': 0.0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_refill_worlds', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'unbound', {'width_frac': 0.0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'cfg4+unbound', {'width_frac': 0.0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'ring+unbound', {'width_frac': 0.0}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_refill_worlds', 'bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'bound', {'width_frac': 0.0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'cfg4+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'cfg4+bound', {'width_frac': 0.0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'ring+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'ring+bound', {'width_frac': 0.0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'hist3+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'hist3+bound', {'width_frac': 0.0}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_dyn_invalidate', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_dyn_invalidate', 'null', {'mask': 196608}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_dyn_invalidate', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_dyn_invalidate', 'unbound', {'mask': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_dyn_invalidate', 'cfg4+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_dyn_invalidate', 'cfg4+unbound', {'mask': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_dyn_invalidate', 'ring+unbound', {}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_dyn_invalidate', 'ring+unbound', {'mask': 196608}, -3, 'no state blob bound: call ssg_bind_state first', []),
    ('ssg_step_host', 'null', {}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'host_act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'host_block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'block_bytes': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'slot': -1}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'slot': 8, 'obs': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'null', {'host_act': 0, 'slot': 9}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'host_act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'host_block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'block_bytes': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'slot': -1}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'slot': 8, 'obs': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'unbound', {'host_act': 0, 'slot': 9}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'host_act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'host_block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'block_bytes': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'slot': -1}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'slot': 8, 'obs': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound', {'host_act': 0, 'slot': 9}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'host_act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'act': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'host_block': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'block_bytes': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'slot': -1}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'slot': 8, 'obs': 0}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_step_host', 'bound+bank', {'host_act': 0, 'slot': 9}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_wait_host', 'null', {'slot': 0}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'null', {'slot': 7}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'null', {'slot': -1}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'null', {'slot': 8}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'unbound', {'slot': 0}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'unbound', {'slot': 7}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'unbound', {'slot': -1}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'unbound', {'slot': 8}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'bound+bank', {'slot': 0}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'bound+bank', {'slot': 7}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'bound+bank', {'slot': -1}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'bound+bank', {'slot': 8}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'cfg4+bound+bank', {'slot': 0}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'cfg4+bound+bank', {'slot': 7}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'cfg4+bound+bank', {'slot': -1}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_wait_host', 'cfg4+bound+bank', {'slot': 8}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_generate_bank', 'null', {}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'bank': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'n_maps': -4}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'width_frac': 0.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'width_frac': -0.5}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'width_frac': 1.0000001}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'width_frac': 'nan'}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'bank': 0, 'width_frac': 2.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'null', {'n_maps': 0, 'raw': 196608}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'bank': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'n_maps': -4}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'width_frac': 0.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'width_frac': -0.5}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'width_frac': 1.0000001}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'width_frac': 'nan'}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'bank': 0, 'width_frac': 2.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'unbound', {'n_maps': 0, 'raw': 196608}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'bank': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'n_maps': -4}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'width_frac': 0.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'width_frac': -0.5}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'width_frac': 1.0000001}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'width_frac': 'nan'}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'bank': 0, 'width_frac': 2.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'bound+bank', {'n_maps': 0, 'raw': 196608}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'bank': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'n_maps': -4}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'width_frac': 0.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'width_frac': -0.5}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'width_frac': 1.0000001}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'width_frac': 'nan'}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'bank': 0, 'width_frac': 2.0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_generate_bank', 'ring+bound+bank', {'n_maps': 0, 'raw': 196608}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_set_terminal_obs', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_set_terminal_obs', 'null', {'term': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_set_terminal_obs', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'unbound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'bound+bank', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'hist3+unbound', {}, -4, 'ssg_set_terminal_obs: history > 2 builds its rows in the frame-shift kernel (reset the done envs with a masked ssg_reset instead)', []),
    ('ssg_set_terminal_obs', 'hist3+unbound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'hist3+bound+bank', {}, -4, 'ssg_set_terminal_obs: history > 2 builds its rows in the frame-shift kernel (reset the done envs with a masked ssg_reset instead)', []),
    ('ssg_set_terminal_obs', 'hist3+bound+bank', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'noreset+bound', {}, -1, 'ssg_set_terminal_obs: only a handle that resets its done envs in-kernel (SSG_FLAG_AUTO_RESET) replaces terminal observations', []),
    ('ssg_set_terminal_obs', 'noreset+bound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'hist3+noreset+unbound', {}, -4, 'ssg_set_terminal_obs: history > 2 builds its rows in the frame-shift kernel (reset the done envs with a masked ssg_reset instead)', []),
    ('ssg_set_terminal_obs', 'hist3+noreset+unbound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'cfg4+bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'cfg4+bound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'ring+bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_set_terminal_obs', 'ring+bound', {'term': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_state_nbytes', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7]),
    ('ssg_state_nbytes', 'null', {'nbytes': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_state_field', 'null', {'field': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 7}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 12}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 13}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 17}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 21}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': -1}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 22}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 1000}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7, -7]),
    ('ssg_state_field', 'null', {'offset': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_field', 'null', {'elem_size': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_field', 'null', {'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_field', 'null', {'stride_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_field', 'null', {'field': -1, 'offset': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_field', 'null', {'field': 13, 'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_state_nbytes', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [44288]),
    ('ssg_state_nbytes', 'unbound', {'nbytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_state_field', 'unbound', {'field': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [8192, 8, 1, 2048]),
    ('ssg_state_field', 'unbound', {'field': 7}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [22528, 8, 8, 2048]),
    ('ssg_state_field', 'unbound', {'field': 12}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 8, 1024, 8]),
    ('ssg_state_field', 'unbound', {'field': 13}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': 17}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': 21}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': -1}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': 22}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': 1000}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'unbound', {'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'unbound', {'elem_size': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'unbound', {'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'unbound', {'stride_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': -1, 'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'unbound', {'field': 13, 'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_nbytes', 'cfg4+unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [36443648]),
    ('ssg_state_nbytes', 'cfg4+unbound', {'nbytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_state_field', 'cfg4+unbound', {'field': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [8192, 8, 1, 2048]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 7}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [22528, 8, 8, 2048]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 12}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 8, 1024, 8]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 13}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [44288, 8, 27, 2048]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 17}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [1544704, 8, 4096, 8]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 21}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [197888, 8, 216, 2048]),
    ('ssg_state_field', 'cfg4+unbound', {'field': -1}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 22}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 1000}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'elem_size': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'stride_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'field': -1, 'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'cfg4+unbound', {'field': 13, 'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_nbytes', 'ring+cfg4+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [36448000]),
    ('ssg_state_nbytes', 'ring+cfg4+bound+bank', {'nbytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [8192, 8, 1, 2048]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 7}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [22528, 8, 8, 2048]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 12}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 8, 1024, 8]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 13}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [48640, 8, 27, 2048]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 17}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [1549056, 8, 4096, 8]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 21}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [202240, 8, 216, 2048]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': -1}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 22}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 1000}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'elem_size': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'stride_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': -1, 'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'ring+cfg4+bound+bank', {'field': 13, 'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_nbytes', 'hist3+bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [187648]),
    ('ssg_state_nbytes', 'hist3+bound', {'nbytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_state_field', 'hist3+bound', {'field': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [8192, 8, 1, 2048]),
    ('ssg_state_field', 'hist3+bound', {'field': 7}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [22528, 8, 8, 2048]),
    ('ssg_state_field', 'hist3+bound', {'field': 12}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 8, 1024, 8]),
    ('ssg_state_field', 'hist3+bound', {'field': 13}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': 17}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': 21}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': -1}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': 22}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': 1000}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'elem_size': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'stride_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': -1, 'offset': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_state_field', 'hist3+bound', {'field': 13, 'n_columns': 0}, -1, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [-7, -7, -7]),
    ('ssg_debug_launch_geometry', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7, -7]),
    ('ssg_debug_launch_geometry', 'null', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_debug_launch_geometry', 'null', {'in_lds': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7]),
    ('ssg_debug_kernel_times', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7.0, -7.0, -7]),
    ('ssg_debug_kernel_times', 'null', {'enable': 1}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7.0, -7.0, -7]),
    ('ssg_debug_kernel_times', 'null', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_debug_kernel_times', 'null', {'step_us': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7.0, -7]),
    ('ssg_debug_dyn_counters', 'null', {}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7, -7]),
    ('ssg_debug_dyn_counters', 'null', {'full_steps': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', [-7]),
    ('ssg_debug_dyn_counters', 'null', {'full_steps': 0, 'rebuilds': 0}, -1, 'ssg_ppo_set_adv_norm: NULL handle', []),
    ('ssg_debug_launch_geometry', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 0, 0]),
    ('ssg_debug_launch_geometry', 'unbound', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'unbound', {'in_lds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 0]),
    ('ssg_debug_kernel_times', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'unbound', {'enable': 1}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'unbound', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_kernel_times', 'unbound', {'step_us': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0]),
    ('ssg_debug_dyn_counters', 'unbound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 0]),
    ('ssg_debug_dyn_counters', 'unbound', {'full_steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0]),
    ('ssg_debug_dyn_counters', 'unbound', {'full_steps': 0, 'rebuilds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 0, 0]),
    ('ssg_debug_launch_geometry', 'bound', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'bound', {'in_lds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 0]),
    ('ssg_debug_kernel_times', 'bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'bound', {'enable': 1}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'bound', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_kernel_times', 'bound', {'step_us': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0]),
    ('ssg_debug_dyn_counters', 'bound', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 0]),
    ('ssg_debug_dyn_counters', 'bound', {'full_steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0]),
    ('ssg_debug_dyn_counters', 'bound', {'full_steps': 0, 'rebuilds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 1, 21936]),
    ('ssg_debug_launch_geometry', 'bound+bank', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'bound+bank', {'in_lds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 21936]),
    ('ssg_debug_kernel_times', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'bound+bank', {'enable': 1}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'bound+bank', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_kernel_times', 'bound+bank', {'step_us': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0]),
    ('ssg_debug_dyn_counters', 'bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 0]),
    ('ssg_debug_dyn_counters', 'bound+bank', {'full_steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0]),
    ('ssg_debug_dyn_counters', 'bound+bank', {'full_steps': 0, 'rebuilds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'cfg4+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 1, 23856]),
    ('ssg_debug_launch_geometry', 'cfg4+bound+bank', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'cfg4+bound+bank', {'in_lds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 23856]),
    ('ssg_debug_kernel_times', 'cfg4+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'cfg4+bound+bank', {'enable': 1}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'cfg4+bound+bank', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_kernel_times', 'cfg4+bound+bank', {'step_us': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0]),
    ('ssg_debug_dyn_counters', 'cfg4+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 0]),
    ('ssg_debug_dyn_counters', 'cfg4+bound+bank', {'full_steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0]),
    ('ssg_debug_dyn_counters', 'cfg4+bound+bank', {'full_steps': 0, 'rebuilds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'ring+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 0, 43920]),
    ('ssg_debug_launch_geometry', 'ring+bound+bank', {'epw': 0, 'in_lds': 0, 'lds_bytes': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_launch_geometry', 'ring+bound+bank', {'in_lds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [64, 43920]),
    ('ssg_debug_kernel_times', 'ring+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'ring+bound+bank', {'enable': 1}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0.0, 0]),
    ('ssg_debug_kernel_times', 'ring+bound+bank', {'enable': 1, 'dyn_us': 0, 'step_us': 0, 'steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
    ('ssg_debug_kernel_times', 'ring+bound+bank', {'step_us': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0.0, 0]),
    ('ssg_debug_dyn_counters', 'ring+bound+bank', {}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0, 0]),
    ('ssg_debug_dyn_counters', 'ring+bound+bank', {'full_steps': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', [0]),
    ('ssg_debug_dyn_counters', 'ring+bound+bank', {'full_steps': 0, 'rebuilds': 0}, 0, 'ssg_ppo_set_adv_norm: unknown mode 9 (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)', []),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_is_the_recorded_one(native, case):
    entry, state, kw, rc, text, outs = CASES[case]
    assert outcome(native, entry, state, kw) == (rc, text, outs), (entry, state, kw)


def test_the_table_covers_every_subject_and_state():
    assert {c[0] for c in CASES} == set(SUBJECTS)
    words = set().union(*(c[1].split("+") for c in CASES))
    assert {"null", "unbound", "bound", "bank", "ring", "cfg4", "hist3", "noreset"} <= words
    for e in SUBJECTS:  # every subject on a NULL handle (ssg_create: a NULL argument)
        assert any(c[0] == e and (c[1] == "null" or e == "ssg_create") for c in CASES), e
    assert sum(c[0] == "ssg_create" and c[3] < 0 for c in CASES) >= 20
    # (no VALID call of a launching entry point: with a device present it would be launched on these made-up addresses)
    assert all(c[3] < 0 for c in CASES if c[0] not in HOST_ONLY)
