"""CPU-side checks of the extended PPO update (value clipping, KL penalty, gradient-norm clipping: ssg_ppo_dist, ssg_ppo_grad_ext,
ssg_ppo_update_ext, ssg_pop_dist, ssg_pop_update_ext): the symbols in the header and the binding, the ssg_ppo_ext / ssg_pop_ext records
against ctypes, every refusal before any device work, the workspace size, and the PBT trainer's switches.  No GPU."""
import ctypes as C
import os
import re

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_SYMBOLS = ("ssg_ppo_dist", "ssg_ppo_grad_ext", "ssg_ppo_update_ext", "ssg_pop_dist", "ssg_pop_update_ext")
PTR = C.sizeof(C.c_void_p)


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_ext_symbols_are_declared_exported_bound_and_abi_stays_9(native):
    text = _header()
    L = native.lib()
    for name in EXT_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in native.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes, name                     # bound with its argument types
    assert native.ABI_VERSION == 9 and L.ssg_abi_version() == 9
    assert re.search(r"#define\s+SSG_ABI_VERSION\s+9\b", text)
    assert C.sizeof(native.PpoHparams) == 88                        # the new constants have a record of their own
    flags = dict(re.findall(r"#define\s+(SSG_POP_EXT_[A-Z_]+)\s+(0x[0-9a-fA-F]+)u", text))
    assert int(flags["SSG_POP_EXT_GRAD_CLIP"], 0) == native.POP_EXT_GRAD_CLIP == 1
    assert int(flags["SSG_POP_EXT_VF_CLIP"], 0) == native.POP_EXT_VF_CLIP == 2


def _record_fields(name):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    names = []
    for ctype, decl in re.findall(r"(uint32_t|double|const float \*|float \*)\s*([\w\s,]+);", body):
        names += [(ctype.strip(), n.strip()) for n in decl.split(",")]
    return names


def _check_record(names, struct, size):
    assert [n for _, n in names] == [f for f, _ in struct._fields_]
    size_of = {"uint32_t": 4, "double": 8, "const float *": PTR, "float *": PTR}
    off = 0
    for ctype, name in names:
        sz = size_of[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(struct, name).offset == off, name
        off += sz
    assert C.sizeof(struct) == (off + 7) // 8 * 8 == size


def test_ext_records_match_the_header(native):
    ppo = _record_fields("ssg_ppo_ext")
    assert [n for _, n in ppo] == ["struct_size", "vf_clip", "max_grad_norm", "kl_target", "dev_kl_coef", "dev_logp_all", "dev_value_old"]
    _check_record(ppo, native.PpoExt, 32 + 3 * PTR)
    pop = _record_fields("ssg_pop_ext")
    assert [n for _, n in pop] == ["struct_size", "flags", "dev_ext", "dev_kl_coef", "dev_logp_all", "dev_value_old"]
    _check_record(pop, native.PopExt, 8 + 4 * PTR)


def _handle(native, n_envs, bound):
    L = native.lib()
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    if bound:  # (host only: the address is recorded, never touched before a launch — and every call below is refused before one)
        native.check(L.ssg_bind_state(h, C.c_void_p(0x100000)), h)
    return h


def _policy(native, D=32, H=64, L=2, A=3, params=0x10000, scale=0x20000):
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = D, H, L, A, native.POLICY_TANH
    p.dev_params, p.dev_obs_scale = params, scale
    return p


def _population(native, P=4, **kw):
    pol = _policy(native, **kw)
    p = native.Population()
    p.struct_size = C.sizeof(native.Population)
    p.n_members = P
    for k in ("obs_dim", "hidden", "n_hidden_layers", "n_actions", "activation", "dev_params", "dev_obs_scale"):
        setattr(p, k, getattr(pol, k))
    return p


def _hparams(native):
    hp = native.PpoHparams()
    hp.struct_size = C.sizeof(native.PpoHparams)
    hp.gamma, hp.lam, hp.clip, hp.vf_coef, hp.ent_coef = 0.99, 0.95, 0.2, 0.5, 0.01
    hp.lr, hp.beta1, hp.beta2, hp.eps, hp.adv_eps = 3e-4, 0.9, 0.999, 1e-8, 1e-8
    return hp


def _ext(native, vf_clip=0.0, max_grad_norm=0.0, kl_target=0.0, kl=0, la=0, vo=0):
    e = native.PpoExt()
    e.struct_size = C.sizeof(native.PpoExt)
    e.vf_clip, e.max_grad_norm, e.kl_target = vf_clip, max_grad_norm, kl_target
    e.dev_kl_coef, e.dev_logp_all, e.dev_value_old = kl or None, la or None, vo or None
    return e


def _pop_ext(native, flags=0, table=0x40000, kl=0, la=0, vo=0):
    e = native.PopExt()
    e.struct_size = C.sizeof(native.PopExt)
    e.flags = flags
    e.dev_ext, e.dev_kl_coef, e.dev_logp_all, e.dev_value_old = table or None, kl or None, la or None, vo or None
    return e


Q = 0x30000     # a plausible device address (256-byte aligned; never dereferenced on the host)
BIG = 1 << 40


def _grad(native, h, pol, hp, ext, M=64, ws=Q, nbytes=BIG, grad=Q, x=Q):
    q = C.c_void_p(Q)
    return native.lib().ssg_ppo_grad_ext(h, pol, hp, ext, 4000, C.c_void_p(x) if x else None, q, q, q, q, q, M,
                                         C.c_void_p(grad) if grad else None, None, C.c_void_p(ws) if ws else None, nbytes, None)


def _update(native, h, pol, hp, ext, epochs=2, minibatches=4, ws=Q, nbytes=BIG, mv=Q, step0=0, perm=Q):
    q = C.c_void_p(Q)
    return native.lib().ssg_ppo_update_ext(h, pol, hp, ext, 4000, q, q, q, q, q, C.c_void_p(perm) if perm else None, epochs, minibatches,
                                           C.c_void_p(mv) if mv else None, step0, None, C.c_void_p(ws) if ws else None, nbytes, None)


def _pop_update(native, h, pop, ext, table_steps=8, K=4, epochs=2, minibatches=4, ws=Q, nbytes=BIG, mv=Q, table=Q):
    q = C.c_void_p(Q)
    return native.lib().ssg_pop_update_ext(h, pop, ext, C.c_void_p(table) if table else None, table_steps, K, q, q, q, q, q, q, epochs,
                                           minibatches, C.c_void_p(mv) if mv else None, None, C.c_void_p(ws) if ws else None, nbytes, None)


def test_ext_entry_points_refuse_without_a_handle_or_a_blob(native):
    L = native.lib()
    pol, hp, ext = C.byref(_policy(native)), C.byref(_hparams(native)), C.byref(_ext(native))
    pop, pext = C.byref(_population(native)), C.byref(_pop_ext(native))
    q = C.c_void_p(Q)
    calls = lambda h: {
        "dist": L.ssg_ppo_dist(h, pol, 4000, q, q, None), "grad": _grad(native, h, pol, hp, ext), "update": _update(native, h, pol, hp, ext),
        "pop_dist": L.ssg_pop_dist(h, pop, 4, q, q, None), "pop_update": _pop_update(native, h, pop, pext)}
    assert set(calls(None).values()) == {-1}                          # SSG_ERR_BAD_ARG without a handle
    h = _handle(native, 1000, bound=False)
    try:
        assert set(calls(h).values()) == {-3}                         # SSG_ERR_NOT_BOUND without a bound blob
    finally:
        L.ssg_destroy(h)


def test_single_policy_ext_refusals_before_any_device_work(native):
    """With a (host-recorded) blob every bad record, missing pointer or short workspace is SSG_ERR_BAD_ARG, judged on the host before
    the device is asked for anything — so this runs without one."""
    L = native.lib()
    h = _handle(native, 1000, bound=True)
    try:
        good_pol, good_hp, good_ext = _policy(native), _hparams(native), _ext(native)
        pol, hp, ext = C.byref(good_pol), C.byref(good_hp), C.byref(good_ext)
        q = C.c_void_p(Q)
        # bad ssg_ppo_ext records, and pointers a switched-on term needs
        short = _ext(native)
        short.struct_size -= 8
        bad_ext = {"NULL": None, "struct_size": C.byref(short), "nan": C.byref(_ext(native, vf_clip=float("nan"))),
                   "inf": C.byref(_ext(native, max_grad_norm=float("inf"))), "nan target": C.byref(_ext(native, kl_target=float("nan"))),
                   "kl without logp_all": C.byref(_ext(native, kl=Q)), "vf_clip without value_old": C.byref(_ext(native, vf_clip=0.2)),
                   "vf_clip with only the kl buffers": C.byref(_ext(native, vf_clip=0.2, kl=Q, la=Q))}
        for what, e in bad_ext.items():
            assert _grad(native, h, pol, hp, e) == -1, what
            assert _update(native, h, pol, hp, e) == -1, what
        assert b"dev_logp_all" in L.ssg_last_error(h) or b"dev_value_old" in L.ssg_last_error(h)
        # bad policy / hparams records
        for bad in (_policy(native, H=40), _policy(native, D=31), _policy(native, params=0), _policy(native, A=5)):
            assert _grad(native, h, C.byref(bad), hp, ext) == -1 and _update(native, h, C.byref(bad), hp, ext) == -1
            assert L.ssg_ppo_dist(h, C.byref(bad), 4000, q, q, None) == -1
        bad_hp = _hparams(native)
        bad_hp.clip = 0.0
        assert _grad(native, h, pol, C.byref(bad_hp), ext) == -1 and _update(native, h, pol, C.byref(bad_hp), ext) == -1
        assert _grad(native, h, None, hp, ext) == -1 and _grad(native, h, pol, None, ext) == -1
        # arguments: NULL buffers, M / epochs / minibatches / step0 out of range
        assert _grad(native, h, pol, hp, ext, x=0) == -1 and _grad(native, h, pol, hp, ext, grad=0) == -1
        assert _grad(native, h, pol, hp, ext, M=0) == -1
        assert _update(native, h, pol, hp, ext, epochs=0) == -1 and _update(native, h, pol, hp, ext, minibatches=0) == -1
        assert _update(native, h, pol, hp, ext, step0=-1) == -1 and _update(native, h, pol, hp, ext, mv=0) == -1
        assert _update(native, h, pol, hp, ext, perm=0) == -1
        # the workspace: NULL, misaligned, one byte short of what ssg_ppo_workspace_nbytes asks for
        nb = C.c_size_t()
        assert L.ssg_ppo_workspace_nbytes(pol, 4000, 1000, C.byref(nb)) == 0
        plen = 64 * 32 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 64 + 1
        assert nb.value >= 256 + 16 * (plen + 8) * 4 + plen * 4    # 16 slots of P + 8 floats, and the clip sequence's vector
        for e in (good_ext, _ext(native, vf_clip=0.2, max_grad_norm=0.5, kl_target=0.01, kl=Q, la=Q, vo=Q)):
            er = C.byref(e)
            assert _grad(native, h, pol, hp, er, M=1000, ws=0) == -1 and _update(native, h, pol, hp, er, ws=0) == -1
            assert _grad(native, h, pol, hp, er, M=1000, ws=Q + 16) == -1 and _update(native, h, pol, hp, er, ws=Q + 16) == -1
            assert _grad(native, h, pol, hp, er, M=1000, nbytes=4096) == -1 and b"workspace" in L.ssg_last_error(h)
            assert _update(native, h, pol, hp, er, nbytes=4096) == -1 and b"workspace" in L.ssg_last_error(h)
        # ssg_ppo_dist: NULL buffers, sample counts outside 1..2^31-1
        assert L.ssg_ppo_dist(h, pol, 4000, None, q, None) == -1 and L.ssg_ppo_dist(h, pol, 4000, q, None, None) == -1
        assert L.ssg_ppo_dist(h, pol, 0, q, q, None) == -1 and L.ssg_ppo_dist(h, pol, 1 << 31, q, q, None) == -1
        assert L.ssg_ppo_dist(h, None, 4000, q, q, None) == -1
        # (no VALID call is made here: with a device present it would be launched on these made-up addresses)
    finally:
        L.ssg_destroy(h)


def test_population_ext_refusals_before_any_device_work(native):
    L = native.lib()
    h = _handle(native, 1000, bound=True)
    try:
        good_pop, good_ext = _population(native), _pop_ext(native)
        pop, ext = C.byref(good_pop), C.byref(good_ext)
        q = C.c_void_p(Q)
        short = _pop_ext(native)
        short.struct_size -= 8
        bad_ext = {"NULL": None, "struct_size": C.byref(short), "no table": C.byref(_pop_ext(native, table=0)),
                   "unknown flag": C.byref(_pop_ext(native, flags=4)), "kl without logp_all": C.byref(_pop_ext(native, kl=Q)),
                   "vf clip flag without value_old": C.byref(_pop_ext(native, flags=native.POP_EXT_VF_CLIP))}
        for what, e in bad_ext.items():
            assert _pop_update(native, h, pop, e) == -1, what
        for bad in (_population(native, P=0), _population(native, P=257), _population(native, P=3), _population(native, H=40),
                    _population(native, params=0)):
            assert _pop_update(native, h, C.byref(bad), ext) == -1 and L.ssg_pop_dist(h, C.byref(bad), 4, q, q, None) == -1
        assert _pop_update(native, h, None, ext) == -1 and L.ssg_pop_dist(h, None, 4, q, q, None) == -1
        assert _pop_update(native, h, pop, ext, K=0) == -1 and _pop_update(native, h, pop, ext, epochs=0) == -1
        assert _pop_update(native, h, pop, ext, minibatches=0) == -1 and _pop_update(native, h, pop, ext, mv=0) == -1
        assert _pop_update(native, h, pop, ext, table=0) == -1
        assert _pop_update(native, h, pop, ext, table_steps=7) == -1 and b"Adam steps" in L.ssg_last_error(h)
        full = C.byref(_pop_ext(native, flags=3, kl=Q, la=Q, vo=Q))
        for e in (ext, full):
            assert _pop_update(native, h, pop, e, ws=0) == -1 and _pop_update(native, h, pop, e, ws=Q + 16) == -1
            assert _pop_update(native, h, pop, e, nbytes=8192) == -1 and b"workspace" in L.ssg_last_error(h)
        assert L.ssg_pop_dist(h, pop, 4, None, q, None) == -1 and L.ssg_pop_dist(h, pop, 4, q, None, None) == -1
        assert L.ssg_pop_dist(h, pop, 0, q, q, None) == -1 and L.ssg_pop_dist(h, pop, 65536, q, q, None) == -1
    finally:
        L.ssg_destroy(h)


def test_pbt_trainer_leaves_the_extended_terms_off_by_default():
    import inspect
    import pytest
    mod = load_script("train/pbt_native.py")
    a = mod.parse_args([])
    assert (a.kl_coeff, a.kl_target, a.vf_clip, a.max_grad_norm) == (0.0, 0.01, 0.0, 0.0)   # kl_target alone switches nothing on
    sig = inspect.signature(mod.train).parameters
    assert [sig[k].default for k in ("kl_coeff", "kl_target", "vf_clip", "max_grad_norm")] == [0.0, 0.01, 0.0, 0.0]
    a = mod.parse_args(["--kl-coeff", "1.0", "--kl-target", "0.02", "--vf-clip", "10", "--max-grad-norm", "0.5"])
    assert (a.kl_coeff, a.kl_target, a.vf_clip, a.max_grad_norm) == (1.0, 0.02, 10.0, 0.5)
    with pytest.raises(SystemExit):
        mod.parse_args(["--kl-coeff", "-1"])
    assert "no kl_coeff" not in mod.__doc__ and "--kl-coeff 1.0" in mod.__doc__
