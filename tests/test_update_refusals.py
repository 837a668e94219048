"""Every refusal of the gradient / update entry points that needs no device, pinned: ssg_ppo_grad, ssg_ppo_grad_ext, ssg_ppo_update,
ssg_ppo_update_ext, ssg_pop_update, ssg_pop_update_ext, ssg_pop_update_sched and the four pack functions (ssg_pop_pack_hparams[_steps],
ssg_pop_pack_schedule[_samples]).  CASES is a table of calls with the return code and the whole ssg_last_error text each must leave,
also where several things are wrong at once: the order of the refusals is part of the interface.  The literals were recorded from the
library as it was before the entry points came to share one record, two fillers and one tail; the file passes unchanged against both.

A handle with a made-up bound blob and made-up device addresses, as in test_ppo_ext.py: every call is refused on the host, nothing is
ever touched.  64 envs, obs_dim 8 (history 1, 2 beams), hidden 16, one layer, 3 actions; a population of 2.  What lies behind the device
for ssg_ppo_grad / ssg_ppo_update (they consult it first) is in test_update_refusals_gpu.py, which runs this file's machinery.  No GPU."""
import ctypes as C

import pytest

Q = 0x30000      # a plausible device address (256-byte aligned; never dereferenced on the host)
BIG = 1 << 40
N_ENVS, D, H, P = 64, 8, 16, 2

# what a call is made with unless its case says otherwise (a pointer: 0 = NULL, absent = the base address)
DEFAULTS = dict(n_samples=256, M=64, epochs=2, minibatches=3, step0=0, K=4, table_steps=6, perm_epochs=2, nbytes=BIG, stats=0,
                sched_epochs=(1, 2), sched_minibatches=(1, 3))


def handle(native, state, base=Q):
    """A handle in `state`: "null" (None), "unbound", "bound", "slices" (bound; slices (24, 40)), "advnorm1" (bound; the per-minibatch
    normalisation scratch of ONE member), "device1" (bound; the handle's device is 1, the current one 0)."""
    if state == "null":
        return None
    L = native.lib()
    c = native.default_config()
    c.n_envs, c.history, c.n_beams = N_ENVS, 1, 2
    if state == "device1":
        c.device_id = 1
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if state != "unbound":  # (host only: the address is recorded, never touched before a launch)
        native.check(L.ssg_bind_state(h, C.c_void_p(base)), h)
    if state == "slices":
        native.check(L.ssg_pop_set_slices(h, 2, (C.c_int32 * 2)(24, 40), C.c_void_p(base)), h)
    if state == "advnorm1":
        nb = C.c_size_t()
        native.check(L.ssg_ppo_adv_norm_nbytes(1, C.byref(nb)))
        native.check(L.ssg_ppo_set_adv_norm(h, native.ADV_NORM_MINIBATCH, 1, C.c_void_p(base), nb.value), h)
    return h


def _record(rec, spec):
    """byref(rec) with the fields of spec overwritten ("nan" / "inf": those floats); spec None: a NULL record."""
    if spec is None:
        return None
    for k, v in spec.items():
        setattr(rec, k, float(v) if isinstance(v, str) else v)
    return C.byref(rec)


def policy(native, base, spec):
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = D, H, 1, 3, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = base, base
    return _record(p, spec)


def population(native, base, spec):
    p = native.Population()
    p.struct_size = C.sizeof(native.Population)
    p.n_members, p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = P, D, H, 1, 3, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = base, base
    return _record(p, spec)


def _hp(native, hp, spec):
    hp.struct_size = C.sizeof(native.PpoHparams)
    hp.gamma, hp.lam, hp.clip, hp.vf_coef, hp.ent_coef = 0.99, 0.95, 0.2, 0.5, 0.01
    hp.lr, hp.beta1, hp.beta2, hp.eps, hp.adv_eps = 3e-4, 0.9, 0.999, 1e-8, 1e-8
    return _record(hp, spec)


def ppo_ext(native, spec):
    e = native.PpoExt()
    e.struct_size = C.sizeof(native.PpoExt)
    return _record(e, spec)


def pop_ext(native, base, spec):
    e = native.PopExt()
    e.struct_size = C.sizeof(native.PopExt)
    e.dev_ext = base
    return _record(e, spec)


def _i32(v):
    return None if v is None else (C.c_int32 * len(v))(*v)


def call(native, entry, h, base=Q, **kw):
    """The return code of `entry` on handle h with DEFAULTS, the records and the pointers as kw overrides them."""
    a = dict(DEFAULTS, **kw)

    def ptr(name):
        v = a.get(name, base)
        return C.c_void_p(v) if v else None
    fn = getattr(native.lib(), entry)
    batch = [ptr(k) for k in ("x", "act", "logp", "adv", "ret", "idx")]
    tail = [ptr("stats"), ptr("ws"), a["nbytes"], None]
    if entry.startswith("ssg_ppo_"):
        head = [h, policy(native, base, a.get("pol", {})), _hp(native, native.PpoHparams(), a.get("hp", {}))]
        if entry.endswith("_ext"):
            head.append(ppo_ext(native, a.get("ext", {})))
        if "grad" in entry:
            return fn(*head, a["n_samples"], *batch, a["M"], ptr("grad"), *tail)
        return fn(*head, a["n_samples"], *batch, a["epochs"], a["minibatches"], ptr("mv"), a["step0"], *tail)
    head = [h, population(native, base, a.get("pop", {}))]
    if entry == "ssg_pop_update_sched":
        return fn(*head, pop_ext(native, base, a.get("ext")), ptr("table"), a["table_steps"], ptr("sched"), _i32(a["sched_epochs"]),
                  _i32(a["sched_minibatches"]), a["perm_epochs"], a["K"], *batch, ptr("mv"), *tail)
    if entry == "ssg_pop_update_ext":
        head.append(pop_ext(native, base, a.get("ext", {})))
    return fn(*head, ptr("table"), a["table_steps"], a["K"], *batch, a["epochs"], a["minibatches"], ptr("mv"), *tail)


def pack(native, entry, n_members=P, hp=({}, {}), step0=0, steps0=(0, 0), n_steps=6, out=True, out_size=None, samples=128,
         epochs=(1, 2), minibatches=(1, 3), launches_out=True):
    """The return code of a pack function.  hp: per member the overrides of a good ssg_ppo_hparams (None: a NULL array); out False: NULL;
    out_size None: what the call needs."""
    L = native.lib()
    if "hparams" in entry:
        arr = None
        if hp is not None:
            arr = (native.PpoHparams * len(hp))()
            for m, spec in enumerate(hp):
                _hp(native, arr[m], spec)
        n = native.pop_table_floats(max(n_members, 1), max(n_steps, 0)) if out_size is None else out_size
        buf = (C.c_float * max(n, 1))() if out else None
        if entry.endswith("_steps"):
            return L.ssg_pop_pack_hparams_steps(n_members, arr, None if steps0 is None else (C.c_int64 * len(steps0))(*steps0), n_steps, buf, n)
        return L.ssg_pop_pack_hparams(n_members, arr, step0, n_steps, buf, n)
    n = native.pop_sched_ints(max(n_members, 1), 6) if out_size is None else out_size
    buf = (C.c_int32 * max(n, 1))() if out else None
    steps, launches = (C.c_int32 * 256)(), C.c_int32()
    if entry.endswith("_samples") and samples is not None:
        samples = (samples,) * max(n_members, 1) if isinstance(samples, int) else samples
        samples = (C.c_int64 * len(samples))(*samples)
    return getattr(L, entry)(n_members, samples, _i32(epochs), _i32(minibatches), buf, n, steps, C.byref(launches) if launches_out else None)


def outcome(native, entry, state, kw, base=Q):
    """(return code, ssg_last_error text) of one case.  A refusal of something else is made first, so that a call which leaves no
    message of its own shows that refusal's text ("ssg_pop_set_slices: ...") and never a stale one."""
    L = native.lib()
    h = handle(native, state, base) if state != "pack" else None
    try:
        assert L.ssg_pop_set_slices(h, 300, (C.c_int32 * 1)(1), C.c_void_p(base)) == -1
        rc = pack(native, entry, **kw) if state == "pack" else call(native, entry, h, base, **kw)
        return rc, L.ssg_last_error(h).decode()
    finally:
        if h is not None:
            L.ssg_destroy(h)


# (entry point, the handle's state — "pack": a pack function, no handle —, what the call is made with, return code, ssg_last_error)
CASES = [
    ('ssg_ppo_grad', 'null', {}, -1, 'ssg_pop_set_slices: NULL handle'),
    ('ssg_ppo_grad', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_grad', 'null', {'pol': None}, -1, 'ssg_pop_set_slices: NULL handle'),
    ('ssg_ppo_grad', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_grad_ext', 'null', {}, -1, 'ssg_pop: NULL handle'),
    ('ssg_ppo_grad_ext', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_grad_ext', 'null', {'pol': None}, -1, 'ssg_pop: NULL handle'),
    ('ssg_ppo_grad_ext', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_update', 'null', {}, -1, 'ssg_pop_set_slices: NULL handle'),
    ('ssg_ppo_update', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_update', 'null', {'pol': None}, -1, 'ssg_pop_set_slices: NULL handle'),
    ('ssg_ppo_update', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_update_ext', 'null', {}, -1, 'ssg_pop: NULL handle'),
    ('ssg_ppo_update_ext', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_update_ext', 'null', {'pol': None}, -1, 'ssg_pop: NULL handle'),
    ('ssg_ppo_update_ext', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update', 'null', {}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update', 'null', {'pop': None}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update_ext', 'null', {}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update_ext', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update_ext', 'null', {'pop': None}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update_ext', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update_sched', 'null', {}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update_sched', 'unbound', {}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_pop_update_sched', 'null', {'pop': None}, -1, 'ssg_pop: NULL handle'),
    ('ssg_pop_update_sched', 'unbound', {'x': 0}, -3, 'no state blob bound: call ssg_bind_state first'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': None}, -1, 'ssg_ppo_grad_ext: NULL policy'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'struct_size': 8}}, -1, 'ssg_ppo_grad_ext: ssg_policy.struct_size != sizeof(ssg_policy)'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'obs_dim': 9}}, -1, "ssg_ppo_grad_ext: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'hidden': 24}}, -1, 'ssg_ppo_grad_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'hidden': 0}}, -1, 'ssg_ppo_grad_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'n_hidden_layers': 3}}, -1, 'ssg_ppo_grad_ext: n_hidden_layers must be 1 or 2'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'n_actions': 5}}, -1, 'ssg_ppo_grad_ext: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'activation': 7}}, -1, 'ssg_ppo_grad_ext: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'dev_params': 0}}, -1, 'ssg_ppo_grad_ext: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'dev_obs_scale': 0}}, -1, 'ssg_ppo_grad_ext: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': None}, -1, 'ssg_ppo_grad_ext: NULL hparams'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'struct_size': 8}}, -1, 'ssg_ppo_grad_ext: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'lr': 'nan'}}, -1, 'ssg_ppo_grad_ext: a hyper-parameter is not finite'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'gamma': 'inf'}}, -1, 'ssg_ppo_grad_ext: a hyper-parameter is not finite'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'clip': 0.0}}, -1, 'ssg_ppo_grad_ext: clip must be > 0'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'beta1': 1.0}}, -1, 'ssg_ppo_grad_ext: betas must be in [0, 1)'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'beta2': -0.5}}, -1, 'ssg_ppo_grad_ext: betas must be in [0, 1)'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': None}, -1, 'ssg_ppo_grad_ext: NULL ssg_ppo_ext'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'struct_size': 8}}, -1, 'ssg_ppo_grad_ext: ssg_ppo_ext.struct_size != sizeof(ssg_ppo_ext)'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'vf_clip': 'nan'}}, -1, 'ssg_ppo_grad_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'max_grad_norm': 'inf'}}, -1, 'ssg_ppo_grad_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'kl_target': 'nan'}}, -1, 'ssg_ppo_grad_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'dev_kl_coef': 196608}}, -1, 'ssg_ppo_grad_ext: dev_kl_coef without dev_logp_all (ssg_ppo_dist)'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'vf_clip': 0.2}}, -1, 'ssg_ppo_grad_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'vf_clip': 0.2, 'dev_kl_coef': 196608, 'dev_logp_all': 196608}}, -1, 'ssg_ppo_grad_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_grad_ext', 'bound', {'n_samples': 0}, -1, 'ssg_ppo_grad_ext: n_samples < 1'),
    ('ssg_ppo_grad_ext', 'bound', {'x': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'act': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'logp': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'adv': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'ret': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'idx': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'grad': 0}, -1, 'ssg_ppo_grad_ext: NULL dev_grad'),
    ('ssg_ppo_grad_ext', 'bound', {'M': 0}, -1, 'ssg_ppo_grad_ext: M < 1'),
    ('ssg_ppo_grad_ext', 'bound', {'ws': 0}, -1, 'ssg_ppo_grad_ext: NULL workspace'),
    ('ssg_ppo_grad_ext', 'bound', {'ws': 196624}, -1, 'ssg_ppo_grad_ext: the workspace must be 256-byte aligned'),
    ('ssg_ppo_grad_ext', 'bound', {'nbytes': 0}, -1, 'ssg_ppo_grad_ext: workspace of 0 bytes, this call needs 2672 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_grad_ext', 'bound', {'nbytes': 2671}, -1, 'ssg_ppo_grad_ext: workspace of 2671 bytes, this call needs 2672 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': None, 'hp': None}, -1, 'ssg_ppo_grad_ext: NULL policy'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': None, 'x': 0}, -1, 'ssg_ppo_grad_ext: NULL hparams'),
    ('ssg_ppo_grad_ext', 'bound', {'x': 0, 'n_samples': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'idx': 0, 'ws': 0}, -1, 'ssg_ppo_grad_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad_ext', 'bound', {'n_samples': 0, 'nbytes': 0}, -1, 'ssg_ppo_grad_ext: n_samples < 1'),
    ('ssg_ppo_grad_ext', 'bound', {'grad': 0, 'M': 0}, -1, 'ssg_ppo_grad_ext: NULL dev_grad'),
    ('ssg_ppo_grad_ext', 'bound', {'M': 0, 'ws': 0}, -1, 'ssg_ppo_grad_ext: M < 1'),
    ('ssg_ppo_grad_ext', 'bound', {'hp': {'clip': 0.0}, 'ext': None}, -1, 'ssg_ppo_grad_ext: clip must be > 0'),
    ('ssg_ppo_grad_ext', 'bound', {'ext': {'vf_clip': 0.2}, 'x': 0}, -1, 'ssg_ppo_grad_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_grad_ext', 'bound', {'pol': {'hidden': 24}, 'ext': {'struct_size': 8}}, -1, 'ssg_ppo_grad_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_update_ext', 'bound', {'pol': None}, -1, 'ssg_ppo_update_ext: NULL policy'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'struct_size': 8}}, -1, 'ssg_ppo_update_ext: ssg_policy.struct_size != sizeof(ssg_policy)'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'obs_dim': 9}}, -1, "ssg_ppo_update_ext: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'hidden': 24}}, -1, 'ssg_ppo_update_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'hidden': 0}}, -1, 'ssg_ppo_update_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'n_hidden_layers': 3}}, -1, 'ssg_ppo_update_ext: n_hidden_layers must be 1 or 2'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'n_actions': 5}}, -1, 'ssg_ppo_update_ext: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'activation': 7}}, -1, 'ssg_ppo_update_ext: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'dev_params': 0}}, -1, 'ssg_ppo_update_ext: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'dev_obs_scale': 0}}, -1, 'ssg_ppo_update_ext: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_update_ext', 'bound', {'hp': None}, -1, 'ssg_ppo_update_ext: NULL hparams'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'struct_size': 8}}, -1, 'ssg_ppo_update_ext: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'lr': 'nan'}}, -1, 'ssg_ppo_update_ext: a hyper-parameter is not finite'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'gamma': 'inf'}}, -1, 'ssg_ppo_update_ext: a hyper-parameter is not finite'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'clip': 0.0}}, -1, 'ssg_ppo_update_ext: clip must be > 0'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'beta1': 1.0}}, -1, 'ssg_ppo_update_ext: betas must be in [0, 1)'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'beta2': -0.5}}, -1, 'ssg_ppo_update_ext: betas must be in [0, 1)'),
    ('ssg_ppo_update_ext', 'bound', {'ext': None}, -1, 'ssg_ppo_update_ext: NULL ssg_ppo_ext'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'struct_size': 8}}, -1, 'ssg_ppo_update_ext: ssg_ppo_ext.struct_size != sizeof(ssg_ppo_ext)'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'vf_clip': 'nan'}}, -1, 'ssg_ppo_update_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'max_grad_norm': 'inf'}}, -1, 'ssg_ppo_update_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'kl_target': 'nan'}}, -1, 'ssg_ppo_update_ext: vf_clip, max_grad_norm or kl_target is not finite'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'dev_kl_coef': 196608}}, -1, 'ssg_ppo_update_ext: dev_kl_coef without dev_logp_all (ssg_ppo_dist)'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'vf_clip': 0.2}}, -1, 'ssg_ppo_update_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'vf_clip': 0.2, 'dev_kl_coef': 196608, 'dev_logp_all': 196608}}, -1, 'ssg_ppo_update_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_update_ext', 'bound', {'n_samples': 0}, -1, 'ssg_ppo_update_ext: n_samples < 1'),
    ('ssg_ppo_update_ext', 'bound', {'x': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'act': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'logp': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'adv': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'ret': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'idx': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'mv': 0}, -1, 'ssg_ppo_update_ext: NULL dev_adam_mv'),
    ('ssg_ppo_update_ext', 'bound', {'epochs': 0}, -1, 'ssg_ppo_update_ext: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update_ext', 'bound', {'minibatches': 0}, -1, 'ssg_ppo_update_ext: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update_ext', 'bound', {'step0': -1}, -1, 'ssg_ppo_update_ext: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update_ext', 'bound', {'ws': 0}, -1, 'ssg_ppo_update_ext: NULL workspace'),
    ('ssg_ppo_update_ext', 'bound', {'ws': 196624}, -1, 'ssg_ppo_update_ext: the workspace must be 256-byte aligned'),
    ('ssg_ppo_update_ext', 'bound', {'nbytes': 0}, -1, 'ssg_ppo_update_ext: workspace of 0 bytes, this call needs 3552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update_ext', 'bound', {'nbytes': 3551}, -1, 'ssg_ppo_update_ext: workspace of 3551 bytes, this call needs 3552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update_ext', 'bound', {'pol': None, 'hp': None}, -1, 'ssg_ppo_update_ext: NULL policy'),
    ('ssg_ppo_update_ext', 'bound', {'hp': None, 'x': 0}, -1, 'ssg_ppo_update_ext: NULL hparams'),
    ('ssg_ppo_update_ext', 'bound', {'x': 0, 'n_samples': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'idx': 0, 'ws': 0}, -1, 'ssg_ppo_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update_ext', 'bound', {'n_samples': 0, 'nbytes': 0}, -1, 'ssg_ppo_update_ext: n_samples < 1'),
    ('ssg_ppo_update_ext', 'bound', {'mv': 0, 'epochs': 0}, -1, 'ssg_ppo_update_ext: NULL dev_adam_mv'),
    ('ssg_ppo_update_ext', 'bound', {'epochs': 0, 'ws': 196624}, -1, 'ssg_ppo_update_ext: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update_ext', 'bound', {'step0': -1, 'nbytes': 0}, -1, 'ssg_ppo_update_ext: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update_ext', 'bound', {'hp': {'clip': 0.0}, 'ext': None}, -1, 'ssg_ppo_update_ext: clip must be > 0'),
    ('ssg_ppo_update_ext', 'bound', {'ext': {'vf_clip': 0.2}, 'x': 0}, -1, 'ssg_ppo_update_ext: vf_clip > 0 without dev_value_old'),
    ('ssg_ppo_update_ext', 'bound', {'pol': {'hidden': 24}, 'ext': {'struct_size': 8}}, -1, 'ssg_ppo_update_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_pop_update', 'bound', {'pop': None}, -1, 'ssg_pop_update: NULL population'),
    ('ssg_pop_update', 'bound', {'pop': {'struct_size': 8}}, -1, 'ssg_pop_update: ssg_population.struct_size != sizeof(ssg_population)'),
    ('ssg_pop_update', 'bound', {'pop': {'n_members': 0}}, -1, 'ssg_pop_update: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update', 'bound', {'pop': {'n_members': 257}}, -1, 'ssg_pop_update: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update', 'bound', {'pop': {'n_members': 3}}, -1, "ssg_pop_update: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update', 'bound', {'pop': {'obs_dim': 9}}, -1, "ssg_pop_update: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_pop_update', 'bound', {'pop': {'hidden': 24}}, -1, 'ssg_pop_update: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_pop_update', 'bound', {'pop': {'n_hidden_layers': 0}}, -1, 'ssg_pop_update: n_hidden_layers must be 1 or 2'),
    ('ssg_pop_update', 'bound', {'pop': {'n_actions': 1}}, -1, 'ssg_pop_update: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_pop_update', 'bound', {'pop': {'activation': 7}}, -1, 'ssg_pop_update: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_pop_update', 'bound', {'pop': {'dev_params': 0}}, -1, 'ssg_pop_update: NULL dev_params or dev_obs_scale'),
    ('ssg_pop_update', 'bound', {'K': 0}, -1, 'ssg_pop_update: K < 1'),
    ('ssg_pop_update', 'bound', {'table': 0}, -1, 'ssg_pop_update: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update', 'bound', {'table_steps': 5}, -1, 'ssg_pop_update: the table holds fewer Adam steps than epochs * chunks'),
    ('ssg_pop_update', 'bound', {'x': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'act': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'logp': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'adv': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'ret': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'idx': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'mv': 0}, -1, 'ssg_pop_update: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update', 'bound', {'epochs': 0}, -1, 'ssg_pop_update: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update', 'bound', {'minibatches': 0}, -1, 'ssg_pop_update: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update', 'bound', {'ws': 0}, -1, 'ssg_pop_update: NULL workspace'),
    ('ssg_pop_update', 'bound', {'ws': 196624}, -1, 'ssg_pop_update: the workspace must be 256-byte aligned'),
    ('ssg_pop_update', 'bound', {'nbytes': 0}, -1, 'ssg_pop_update: workspace of 0 bytes, this call needs 5824 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update', 'bound', {'nbytes': 5823}, -1, 'ssg_pop_update: workspace of 5823 bytes, this call needs 5824 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update', 'bound', {'pop': {'n_members': 3}, 'K': 0}, -1, "ssg_pop_update: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update', 'bound', {'K': 0, 'x': 0}, -1, 'ssg_pop_update: K < 1'),
    ('ssg_pop_update', 'bound', {'x': 0, 'table': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'bound', {'table': 0, 'ws': 0}, -1, 'ssg_pop_update: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update', 'bound', {'table_steps': 5, 'nbytes': 0}, -1, 'ssg_pop_update: the table holds fewer Adam steps than epochs * chunks'),
    ('ssg_pop_update', 'bound', {'mv': 0, 'epochs': 0}, -1, 'ssg_pop_update: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update', 'bound', {'minibatches': 0, 'table_steps': 0}, -1, 'ssg_pop_update: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update', 'bound', {'epochs': 0, 'ws': 0}, -1, 'ssg_pop_update: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update_ext', 'bound', {'pop': None}, -1, 'ssg_pop_update_ext: NULL population'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'struct_size': 8}}, -1, 'ssg_pop_update_ext: ssg_population.struct_size != sizeof(ssg_population)'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_members': 0}}, -1, 'ssg_pop_update_ext: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_members': 257}}, -1, 'ssg_pop_update_ext: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_members': 3}}, -1, "ssg_pop_update_ext: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update_ext', 'bound', {'pop': {'obs_dim': 9}}, -1, "ssg_pop_update_ext: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_pop_update_ext', 'bound', {'pop': {'hidden': 24}}, -1, 'ssg_pop_update_ext: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_hidden_layers': 0}}, -1, 'ssg_pop_update_ext: n_hidden_layers must be 1 or 2'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_actions': 1}}, -1, 'ssg_pop_update_ext: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'activation': 7}}, -1, 'ssg_pop_update_ext: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'dev_params': 0}}, -1, 'ssg_pop_update_ext: NULL dev_params or dev_obs_scale'),
    ('ssg_pop_update_ext', 'bound', {'ext': None}, -1, 'ssg_pop_update_ext: NULL ssg_pop_ext'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'struct_size': 8}}, -1, 'ssg_pop_update_ext: ssg_pop_ext.struct_size != sizeof(ssg_pop_ext)'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'flags': 4}}, -1, 'ssg_pop_update_ext: unknown ssg_pop_ext.flags bits'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'dev_ext': 0}}, -1, 'ssg_pop_update_ext: NULL dev_ext'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'dev_kl_coef': 196608}}, -1, 'ssg_pop_update_ext: dev_kl_coef without dev_logp_all (ssg_pop_dist)'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'flags': 2}}, -1, 'ssg_pop_update_ext: SSG_POP_EXT_VF_CLIP without dev_value_old'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'flags': 2, 'dev_kl_coef': 196608, 'dev_logp_all': 196608}}, -1, 'ssg_pop_update_ext: SSG_POP_EXT_VF_CLIP without dev_value_old'),
    ('ssg_pop_update_ext', 'bound', {'K': 0}, -1, 'ssg_pop_update_ext: K < 1'),
    ('ssg_pop_update_ext', 'bound', {'table': 0}, -1, 'ssg_pop_update_ext: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_ext', 'bound', {'table_steps': 5}, -1, 'ssg_pop_update_ext: the table holds fewer Adam steps than epochs * chunks'),
    ('ssg_pop_update_ext', 'bound', {'x': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'act': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'logp': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'adv': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'ret': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'idx': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'mv': 0}, -1, 'ssg_pop_update_ext: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_ext', 'bound', {'epochs': 0}, -1, 'ssg_pop_update_ext: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update_ext', 'bound', {'minibatches': 0}, -1, 'ssg_pop_update_ext: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update_ext', 'bound', {'ws': 0}, -1, 'ssg_pop_update_ext: NULL workspace'),
    ('ssg_pop_update_ext', 'bound', {'ws': 196624}, -1, 'ssg_pop_update_ext: the workspace must be 256-byte aligned'),
    ('ssg_pop_update_ext', 'bound', {'nbytes': 0}, -1, 'ssg_pop_update_ext: workspace of 0 bytes, this call needs 8928 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_ext', 'bound', {'nbytes': 8927}, -1, 'ssg_pop_update_ext: workspace of 8927 bytes, this call needs 8928 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_ext', 'bound', {'pop': {'n_members': 3}, 'K': 0}, -1, "ssg_pop_update_ext: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update_ext', 'bound', {'K': 0, 'x': 0}, -1, 'ssg_pop_update_ext: K < 1'),
    ('ssg_pop_update_ext', 'bound', {'x': 0, 'table': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'bound', {'table': 0, 'ws': 0}, -1, 'ssg_pop_update_ext: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_ext', 'bound', {'table_steps': 5, 'nbytes': 0}, -1, 'ssg_pop_update_ext: the table holds fewer Adam steps than epochs * chunks'),
    ('ssg_pop_update_ext', 'bound', {'pop': None, 'ext': None}, -1, 'ssg_pop_update_ext: NULL population'),
    ('ssg_pop_update_ext', 'bound', {'ext': {'flags': 4}, 'K': 0}, -1, 'ssg_pop_update_ext: unknown ssg_pop_ext.flags bits'),
    ('ssg_pop_update_ext', 'bound', {'mv': 0, 'epochs': 0}, -1, 'ssg_pop_update_ext: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_ext', 'bound', {'minibatches': 0, 'table_steps': 0}, -1, 'ssg_pop_update_ext: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update_ext', 'bound', {'epochs': 0, 'ws': 0}, -1, 'ssg_pop_update_ext: epochs < 1 or minibatches < 1'),
    ('ssg_pop_update_sched', 'bound', {'pop': None}, -1, 'ssg_pop_update_sched: NULL population'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'struct_size': 8}}, -1, 'ssg_pop_update_sched: ssg_population.struct_size != sizeof(ssg_population)'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_members': 0}}, -1, 'ssg_pop_update_sched: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_members': 257}}, -1, 'ssg_pop_update_sched: n_members must be in 1..SSG_POP_MAX_MEMBERS'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_members': 3}}, -1, "ssg_pop_update_sched: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update_sched', 'bound', {'pop': {'obs_dim': 9}}, -1, "ssg_pop_update_sched: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_pop_update_sched', 'bound', {'pop': {'hidden': 24}}, -1, 'ssg_pop_update_sched: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_hidden_layers': 0}}, -1, 'ssg_pop_update_sched: n_hidden_layers must be 1 or 2'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_actions': 1}}, -1, 'ssg_pop_update_sched: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'activation': 7}}, -1, 'ssg_pop_update_sched: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'dev_params': 0}}, -1, 'ssg_pop_update_sched: NULL dev_params or dev_obs_scale'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'struct_size': 8}}, -1, 'ssg_pop_update_sched: ssg_pop_ext.struct_size != sizeof(ssg_pop_ext)'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'flags': 4}}, -1, 'ssg_pop_update_sched: unknown ssg_pop_ext.flags bits'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'dev_ext': 0}}, -1, 'ssg_pop_update_sched: NULL dev_ext'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'dev_kl_coef': 196608}}, -1, 'ssg_pop_update_sched: dev_kl_coef without dev_logp_all (ssg_pop_dist)'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'flags': 2}}, -1, 'ssg_pop_update_sched: SSG_POP_EXT_VF_CLIP without dev_value_old'),
    ('ssg_pop_update_sched', 'bound', {'ext': {'flags': 2, 'dev_kl_coef': 196608, 'dev_logp_all': 196608}}, -1, 'ssg_pop_update_sched: SSG_POP_EXT_VF_CLIP without dev_value_old'),
    ('ssg_pop_update_sched', 'bound', {'K': 0}, -1, 'ssg_pop_update_sched: K < 1'),
    ('ssg_pop_update_sched', 'bound', {'table': 0}, -1, 'ssg_pop_update_sched: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_sched', 'bound', {'table_steps': 5}, -1, "ssg_pop_update_sched: the table holds fewer Adam steps than the schedule's launches (max epochs * chunks)"),
    ('ssg_pop_update_sched', 'bound', {'x': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'act': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'logp': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'adv': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'ret': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'idx': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'mv': 0}, -1, 'ssg_pop_update_sched: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_sched', 'bound', {'sched_epochs': None}, -1, 'ssg_pop_update_sched: NULL epochs or minibatches'),
    ('ssg_pop_update_sched', 'bound', {'sched_minibatches': None}, -1, 'ssg_pop_update_sched: NULL epochs or minibatches'),
    ('ssg_pop_update_sched', 'bound', {'sched': 0}, -1, 'ssg_pop_update_sched: NULL dev_sched'),
    ('ssg_pop_update_sched', 'bound', {'sched_epochs': (1, 0)}, -1, "ssg_pop_update_sched: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_update_sched', 'bound', {'sched_minibatches': (0, 3)}, -1, "ssg_pop_update_sched: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_update_sched', 'bound', {'perm_epochs': 1}, -1, 'ssg_pop_update_sched: perm_epochs < the largest epochs of a member'),
    ('ssg_pop_update_sched', 'bound', {'sched_epochs': (3, 2)}, -1, 'ssg_pop_update_sched: perm_epochs < the largest epochs of a member'),
    ('ssg_pop_update_sched', 'bound', {'ext': {}, 'table_steps': 5}, -1, "ssg_pop_update_sched: the table holds fewer Adam steps than the schedule's launches (max epochs * chunks)"),
    ('ssg_pop_update_sched', 'bound', {'ws': 0}, -1, 'ssg_pop_update_sched: NULL workspace'),
    ('ssg_pop_update_sched', 'bound', {'ws': 196624}, -1, 'ssg_pop_update_sched: the workspace must be 256-byte aligned'),
    ('ssg_pop_update_sched', 'bound', {'nbytes': 0}, -1, 'ssg_pop_update_sched: workspace of 0 bytes, this call needs 7552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'bound', {'nbytes': 7551}, -1, 'ssg_pop_update_sched: workspace of 7551 bytes, this call needs 7552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'bound', {'ext': {}, 'nbytes': 0}, -1, 'ssg_pop_update_sched: workspace of 0 bytes, this call needs 10688 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'bound', {'ext': {}, 'nbytes': 10687}, -1, 'ssg_pop_update_sched: workspace of 10687 bytes, this call needs 10688 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'bound', {'ext': {}, 'ws': 0}, -1, 'ssg_pop_update_sched: NULL workspace'),
    ('ssg_pop_update_sched', 'bound', {'pop': {'n_members': 3}, 'K': 0}, -1, "ssg_pop_update_sched: the handle's 64 envs do not split into 3 equal member slices"),
    ('ssg_pop_update_sched', 'bound', {'K': 0, 'x': 0}, -1, 'ssg_pop_update_sched: K < 1'),
    ('ssg_pop_update_sched', 'bound', {'x': 0, 'table': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'bound', {'table': 0, 'ws': 0}, -1, 'ssg_pop_update_sched: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_sched', 'bound', {'table_steps': 5, 'nbytes': 0}, -1, "ssg_pop_update_sched: the table holds fewer Adam steps than the schedule's launches (max epochs * chunks)"),
    ('ssg_pop_update_sched', 'bound', {'ext': {'dev_ext': 0}, 'K': 0}, -1, 'ssg_pop_update_sched: NULL dev_ext'),
    ('ssg_pop_update_sched', 'bound', {'mv': 0, 'sched': 0}, -1, 'ssg_pop_update_sched: NULL dev_table or dev_adam_mv'),
    ('ssg_pop_update_sched', 'bound', {'sched': 0, 'sched_epochs': (1, 0)}, -1, 'ssg_pop_update_sched: NULL dev_sched'),
    ('ssg_pop_update_sched', 'bound', {'perm_epochs': 1, 'table_steps': 5}, -1, 'ssg_pop_update_sched: perm_epochs < the largest epochs of a member'),
    ('ssg_pop_update_sched', 'bound', {'sched_epochs': None, 'ws': 0}, -1, 'ssg_pop_update_sched: NULL epochs or minibatches'),
    ('ssg_ppo_grad_ext', 'bound', {'M': 1000, 'nbytes': 0}, -1, 'ssg_ppo_grad_ext: workspace of 0 bytes, this call needs 15872 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_grad_ext', 'bound', {'M': 1000, 'nbytes': 15871}, -1, 'ssg_ppo_grad_ext: workspace of 15871 bytes, this call needs 15872 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update_ext', 'bound', {'minibatches': 1, 'nbytes': 0}, -1, 'ssg_ppo_update_ext: workspace of 0 bytes, this call needs 5312 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update_ext', 'bound', {'minibatches': 1, 'nbytes': 5311}, -1, 'ssg_ppo_update_ext: workspace of 5311 bytes, this call needs 5312 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update', 'slices', {}, -1, 'ssg_pop_update: slices are bound to the handle (ssg_pop_set_slices): the update runs through ssg_pop_update_sched'),
    ('ssg_pop_update', 'slices', {'K': 0}, -1, 'ssg_pop_update: K < 1'),
    ('ssg_pop_update', 'slices', {'x': 0}, -1, 'ssg_pop_update: slices are bound to the handle (ssg_pop_set_slices): the update runs through ssg_pop_update_sched'),
    ('ssg_pop_update', 'slices', {'pop': {'n_members': 4}}, -1, 'ssg_pop_update: 4 members, but slices for 2 members are bound to the handle (ssg_pop_set_slices)'),
    ('ssg_pop_update', 'advnorm1', {}, -1, 'ssg_pop_update: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_pop_update', 'advnorm1', {'x': 0}, -1, 'ssg_pop_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update', 'advnorm1', {'table': 0}, -1, 'ssg_pop_update: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_pop_update_ext', 'slices', {}, -1, 'ssg_pop_update_ext: slices are bound to the handle (ssg_pop_set_slices): the update runs through ssg_pop_update_sched'),
    ('ssg_pop_update_ext', 'slices', {'K': 0}, -1, 'ssg_pop_update_ext: K < 1'),
    ('ssg_pop_update_ext', 'slices', {'x': 0}, -1, 'ssg_pop_update_ext: slices are bound to the handle (ssg_pop_set_slices): the update runs through ssg_pop_update_sched'),
    ('ssg_pop_update_ext', 'slices', {'pop': {'n_members': 4}}, -1, 'ssg_pop_update_ext: 4 members, but slices for 2 members are bound to the handle (ssg_pop_set_slices)'),
    ('ssg_pop_update_ext', 'advnorm1', {}, -1, 'ssg_pop_update_ext: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_pop_update_ext', 'advnorm1', {'x': 0}, -1, 'ssg_pop_update_ext: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_ext', 'advnorm1', {'table': 0}, -1, 'ssg_pop_update_ext: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_pop_update_sched', 'slices', {'K': 0}, -1, 'ssg_pop_update_sched: K < 1'),
    ('ssg_pop_update_sched', 'slices', {'x': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'slices', {'pop': {'n_members': 4}}, -1, 'ssg_pop_update_sched: 4 members, but slices for 2 members are bound to the handle (ssg_pop_set_slices)'),
    ('ssg_pop_update_sched', 'advnorm1', {}, -1, 'ssg_pop_update_sched: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_pop_update_sched', 'advnorm1', {'x': 0}, -1, 'ssg_pop_update_sched: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_pop_update_sched', 'advnorm1', {'table': 0}, -1, 'ssg_pop_update_sched: 2 members, but the bound advantage-normalisation scratch serves n_members = 1 (ssg_ppo_set_adv_norm)'),
    ('ssg_ppo_grad_ext', 'advnorm1', {'ws': 0}, -1, 'ssg_ppo_grad_ext: NULL workspace'),
    ('ssg_ppo_update_ext', 'advnorm1', {'ws': 0}, -1, 'ssg_ppo_update_ext: NULL workspace'),
    ('ssg_pop_update_sched', 'slices', {'nbytes': 0}, -1, 'ssg_pop_update_sched: workspace of 0 bytes, this call needs 7552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'slices', {'nbytes': 7551}, -1, 'ssg_pop_update_sched: workspace of 7551 bytes, this call needs 7552 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'slices', {'ext': {}, 'nbytes': 0}, -1, 'ssg_pop_update_sched: workspace of 0 bytes, this call needs 10688 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'slices', {'ext': {}, 'nbytes': 10687}, -1, 'ssg_pop_update_sched: workspace of 10687 bytes, this call needs 10688 (ssg_ppo_workspace_nbytes)'),
    ('ssg_pop_update_sched', 'slices', {'table_steps': 5}, -1, "ssg_pop_update_sched: the table holds fewer Adam steps than the schedule's launches (max epochs * chunks)"),
    ('ssg_pop_update_sched', 'slices', {'perm_epochs': 1}, -1, 'ssg_pop_update_sched: perm_epochs < the largest epochs of a member'),
    ('ssg_pop_update_sched', 'slices', {'sched_minibatches': (1, 0)}, -1, "ssg_pop_update_sched: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_hparams', 'pack', {'hp': None}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'out': False}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'n_members': 0}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'n_members': 257}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'n_steps': -1}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'out_size': 35}, -1, 'ssg_pop_pack_hparams: out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps)'),
    ('ssg_pop_pack_hparams', 'pack', {'hp': ({}, {'clip': 0.0})}, -1, 'ssg_pop_pack_hparams: clip must be > 0'),
    ('ssg_pop_pack_hparams', 'pack', {'hp': ({'struct_size': 8}, {})}, -1, 'ssg_pop_pack_hparams: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_pop_pack_hparams', 'pack', {'hp': ({}, {'lr': 'nan'})}, -1, 'ssg_pop_pack_hparams: a hyper-parameter is not finite'),
    ('ssg_pop_pack_hparams', 'pack', {'hp': ({'beta1': 1.0}, {})}, -1, 'ssg_pop_pack_hparams: betas must be in [0, 1)'),
    ('ssg_pop_pack_hparams', 'pack', {'hp': None, 'out_size': 0}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'out_size': 0, 'hp': ({}, {'clip': 0.0})}, -1, 'ssg_pop_pack_hparams: out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps)'),
    ('ssg_pop_pack_hparams', 'pack', {'n_members': 0, 'n_steps': -1}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': None}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'out': False}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'n_members': 0}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'n_members': 257}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'n_steps': -1}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'out_size': 35}, -1, 'ssg_pop_pack_hparams_steps: out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps)'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': ({}, {'clip': 0.0})}, -1, 'ssg_pop_pack_hparams_steps: clip must be > 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': ({'struct_size': 8}, {})}, -1, 'ssg_pop_pack_hparams_steps: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': ({}, {'lr': 'nan'})}, -1, 'ssg_pop_pack_hparams_steps: a hyper-parameter is not finite'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': ({'beta1': 1.0}, {})}, -1, 'ssg_pop_pack_hparams_steps: betas must be in [0, 1)'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'hp': None, 'out_size': 0}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'out_size': 0, 'hp': ({}, {'clip': 0.0})}, -1, 'ssg_pop_pack_hparams_steps: out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps)'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'n_members': 0, 'n_steps': -1}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'step0': -1}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams', 'pack', {'step0': -1, 'out_size': 0}, -1, 'ssg_pop_pack_hparams: NULL pointer, n_members out of range, n_steps < 0 or step0 < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'steps0': None}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_hparams_steps', 'pack', {'steps0': (0, -1)}, -1, "ssg_pop_pack_hparams_steps: a member's step0 is < 0"),
    ('ssg_pop_pack_hparams_steps', 'pack', {'steps0': (0, -1), 'out_size': 0}, -1, "ssg_pop_pack_hparams_steps: a member's step0 is < 0"),
    ('ssg_pop_pack_hparams_steps', 'pack', {'steps0': None, 'n_steps': -1}, -1, 'ssg_pop_pack_hparams_steps: NULL pointer, n_members out of range or n_steps < 0'),
    ('ssg_pop_pack_schedule', 'pack', {'epochs': None}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'minibatches': None}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'launches_out': False}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'n_members': 0}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'n_members': 257}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'epochs': (1, 0)}, -1, "ssg_pop_pack_schedule: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule', 'pack', {'minibatches': (0, 3)}, -1, "ssg_pop_pack_schedule: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule', 'pack', {'out_size': 17}, -1, 'ssg_pop_pack_schedule: out_ints < SSG_POP_SCHED_INTS(n_members, n_launches)'),
    ('ssg_pop_pack_schedule', 'pack', {'epochs': (1, 0), 'out_size': 0}, -1, "ssg_pop_pack_schedule: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule', 'pack', {'epochs': None, 'n_members': 0}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'epochs': None}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'minibatches': None}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'launches_out': False}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'n_members': 0}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'n_members': 257}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'epochs': (1, 0)}, -1, "ssg_pop_pack_schedule_samples: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule_samples', 'pack', {'minibatches': (0, 3)}, -1, "ssg_pop_pack_schedule_samples: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule_samples', 'pack', {'out_size': 17}, -1, 'ssg_pop_pack_schedule_samples: out_ints < SSG_POP_SCHED_INTS(n_members, n_launches)'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'epochs': (1, 0), 'out_size': 0}, -1, "ssg_pop_pack_schedule_samples: a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)"),
    ('ssg_pop_pack_schedule_samples', 'pack', {'epochs': None, 'n_members': 0}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule', 'pack', {'samples': 0}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule', 'pack', {'samples': 0, 'epochs': (0, 0)}, -1, 'ssg_pop_pack_schedule: NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'samples': None}, -1, 'ssg_pop_pack_schedule_samples: NULL samples, epochs, minibatches or n_launches_out, or n_members out of range'),
    ('ssg_pop_pack_schedule_samples', 'pack', {'samples': (128, 0)}, -1, "ssg_pop_pack_schedule_samples: a member's sample count is < 1"),
    ('ssg_pop_pack_schedule_samples', 'pack', {'samples': (0, 128), 'epochs': (0, 1)}, -1, "ssg_pop_pack_schedule_samples: a member's sample count is < 1"),
    ('ssg_pop_pack_schedule_samples', 'pack', {'samples': (24, 40), 'out_size': 17}, -1, 'ssg_pop_pack_schedule_samples: out_ints < SSG_POP_SCHED_INTS(n_members, n_launches)'),
]


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_is_the_recorded_one(native, case):
    entry, state, kw, rc, text = CASES[case]
    assert outcome(native, entry, state, kw) == (rc, text), (entry, state, kw)


def test_the_table_covers_every_entry_point_and_precedence(native):
    entries = {c[0] for c in CASES}
    assert entries == {"ssg_ppo_grad", "ssg_ppo_grad_ext", "ssg_ppo_update", "ssg_ppo_update_ext", "ssg_pop_update", "ssg_pop_update_ext",
                       "ssg_pop_update_sched", "ssg_pop_pack_hparams", "ssg_pop_pack_hparams_steps", "ssg_pop_pack_schedule",
                       "ssg_pop_pack_schedule_samples"}
    for e in entries:  # at least one case per entry point with two things wrong at once (a handle's state can be one of them)
        assert any(c[0] == e and len(c[2]) + (c[1] not in ("bound", "pack")) >= 2 for c in CASES), e
    assert all(c[3] < 0 for c in CASES)  # (no VALID call: with a device present it would be launched on these made-up addresses)
