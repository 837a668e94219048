"""CPU checks of per-minibatch advantage normalisation (ssg_ppo_adv_norm_nbytes / ssg_ppo_set_adv_norm / ssg_ppo_get_adv_norm;
ship_sim_gym_amd/ppo.py's minibatch_adv_reference; --adv-norm of the trainers): the ABI surface, the scratch formula, every refusal of
the binding with the argument named, the numpy restatement against plain numpy, and the trainers' flags.  Nothing touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ssg_ppo_adv_norm_nbytes", "ssg_ppo_set_adv_norm", "ssg_ppo_get_adv_norm")


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_symbols_are_exported_declared_and_cite_the_reference(native):
    text, L = _header(), native.lib()
    decls = [(m.start(), m.group(1)) for m in re.finditer(r'^\s*(?:int|const char\s*\*)\s+(ssg_\w+)\s*\(', text, flags=re.M)]
    for name in SYMBOLS:
        assert name in native.EXPORTS and hasattr(L, name), name
        i = [d[1] for d in decls].index(name)                                # declared, as a function returning int
        comment = text[decls[i - 1][0]: decls[i][0]]                         # what tests/test_abi.py reads for this declaration
        assert "train/stable_baselines/ppo.py:90" in comment, name
    assert L.ssg_abi_version() == native.ABI_VERSION == 9                    # additive: the version stays


def test_constants_header_equals_binding(native):
    consts = dict(re.findall(r"#define\s+(SSG_ADV_NORM_[A-Z]+)\s+(\d+)", _header()))
    assert consts == {"SSG_ADV_NORM_BATCH": "0", "SSG_ADV_NORM_MINIBATCH": "1"}
    assert (native.ADV_NORM_BATCH, native.ADV_NORM_MINIBATCH) == (0, 1)


def _nbytes(native, P):
    out = C.c_size_t(0)
    return native.lib().ssg_ppo_adv_norm_nbytes(P, C.byref(out)), out.value


def _formula(P):
    r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
    return r256(P * 4 * 4) + r256(P * 64 * 3 * 8)  # f32 [P][4] statistics, then f64 [P][64][3] partials


def test_scratch_formula_and_refusals(native):
    for P in (1, 16, 256):
        assert _nbytes(native, P) == (0, _formula(P)), P
    assert _formula(1) == 256 + 1536
    for bad in (0, 257):
        assert _nbytes(native, bad)[0] == -1, bad
        assert b"n_members" in native.lib().ssg_last_error(None)
    assert native.lib().ssg_ppo_adv_norm_nbytes(1, None) == -1
    assert b"nbytes" in native.lib().ssg_last_error(None)


def _handle(native, n_envs=256):
    c = native.default_config()
    c.n_envs = n_envs
    h = C.c_void_p()
    native.check(native.lib().ssg_create(C.byref(c), C.byref(h)))
    return h


def _bound(native, h):
    mode, members = C.c_int(-1), C.c_int(-1)
    assert native.lib().ssg_ppo_get_adv_norm(h, C.byref(mode), C.byref(members)) == 0
    return mode.value, members.value


SCRATCH = 0x100000  # (256-byte aligned; the host never dereferences it)


def test_binding_refusals_name_the_argument_and_leave_the_binding(native):
    L = native.lib()
    MB, B = native.ADV_NORM_MINIBATCH, native.ADV_NORM_BATCH
    assert L.ssg_ppo_set_adv_norm(None, MB, 1, C.c_void_p(SCRATCH), _formula(1)) == -1
    assert b"NULL handle" in L.ssg_last_error(None)
    assert L.ssg_ppo_get_adv_norm(None, None, None) == -1
    h = _handle(native)
    try:
        assert _bound(native, h) == (B, 0)                                   # a fresh handle: batch mode, nothing bound
        # a good binding needs no state blob and no device: it is host only
        assert L.ssg_ppo_set_adv_norm(h, MB, 4, C.c_void_p(SCRATCH), _formula(4)) == 0
        assert _bound(native, h) == (MB, 4)
        refusals = (
            ((2, 4, SCRATCH, _formula(4)), b"mode"),                         # an unknown mode
            ((-1, 4, SCRATCH, _formula(4)), b"mode"),
            ((MB, 4, None, _formula(4)), b"dev_scratch"),                    # mode 1 with NULL scratch
            ((MB, 4, SCRATCH + 128, _formula(4)), b"dev_scratch"),           # misaligned
            ((MB, 4, SCRATCH, _formula(4) - 1), b"scratch_nbytes"),          # too small
            ((MB, 4, SCRATCH, _formula(3)), b"scratch_nbytes"),
            ((MB, 0, SCRATCH, _formula(4)), b"n_members"),                   # n_members outside 1..SSG_POP_MAX_MEMBERS
            ((MB, 257, SCRATCH, _formula(256)), b"n_members"),
            ((MB, -3, SCRATCH, _formula(4)), b"n_members"),
        )
        for (mode, members, ptr, nb), word in refusals:
            rc = L.ssg_ppo_set_adv_norm(h, mode, members, C.c_void_p(ptr) if ptr is not None else None, nb)
            assert rc == -1 and word in L.ssg_last_error(h), (mode, members, ptr, nb, L.ssg_last_error(h))
            assert _bound(native, h) == (MB, 4)                              # the binding stays as it was
        assert L.ssg_ppo_set_adv_norm(h, MB, 256, C.c_void_p(SCRATCH), _formula(256)) == 0 and _bound(native, h) == (MB, 256)
        # mode 0 unbinds, with or without a scratch
        assert L.ssg_ppo_set_adv_norm(h, B, 1, C.c_void_p(SCRATCH), _formula(1)) == 0 and _bound(native, h) == (B, 0)
        assert L.ssg_ppo_set_adv_norm(h, MB, 1, C.c_void_p(SCRATCH), _formula(1)) == 0 and _bound(native, h) == (MB, 1)
        assert L.ssg_ppo_set_adv_norm(h, B, 0, None, 0) == 0 and _bound(native, h) == (B, 0)
    finally:
        L.ssg_destroy(h)


def test_reference_against_plain_numpy():
    from ship_sim_gym_amd.ppo import minibatch_adv_reference as ref
    rng = np.random.RandomState(3)
    a = (rng.standard_normal(10000) * 2.5 + 0.75).astype(np.float32)
    eps = 1e-8
    row = ref(a, np.ones(a.size, dtype=bool), eps)
    assert row.dtype == np.float32 and row.shape == (4,)
    a64 = a.astype(np.float64)
    mean, std = a64.mean(), a64.std(ddof=1)
    assert abs(row[0] - mean) <= 1e-6 * abs(mean) and abs(row[1] - (std + eps)) <= 1e-6 * std
    assert abs(row[2] - 1.0 / (std + eps)) <= 1e-6 / std and row[3] == 0.0
    # invalid positions count for nothing, whatever they hold
    valid = rng.uniform(size=a.size) > 0.05
    junk = np.where(valid, a, np.float32(1e30))
    row = ref(junk, valid, eps)
    mean, std = a64[valid].mean(), a64[valid].std(ddof=1)
    assert abs(row[0] - mean) <= 1e-6 * abs(mean) and abs(row[1] - (std + eps)) <= 1e-6 * std
    # one sample: var = 0 (numpy's std of one sample, not torch's NaN); none: {0, 1, 1, 0}
    one = ref(np.array([1.75], dtype=np.float32), np.array([True]), eps)
    assert one.tolist() == [1.75, np.float32(eps), np.float32(1.0) / np.float32(eps), 0.0]
    one_of_three = ref(np.array([9.0, 1.75, 9.0], dtype=np.float32), np.array([False, True, False]), eps)
    assert one_of_three.tolist() == one.tolist()
    row, part = ref(a, np.ones(a.size, dtype=bool), eps, partials=True)      # 10 workgroups, rounds of 2 560: the last round ends in workgroup 9
    assert part.shape == (10, 3) and part.dtype == np.float64 and part[:, 2].tolist() == [1024.0] * 9 + [784.0]
    assert abs(part[:, 0].sum() - a64.sum()) <= 1e-9 * np.abs(a64).sum() and row.tolist() == ref(a, np.ones(a.size, dtype=bool), eps).tolist()
    for empty in (ref(np.zeros(0, dtype=np.float32), np.zeros(0, dtype=bool), eps), ref(np.ones(5, dtype=np.float32), np.zeros(5, dtype=bool), eps)):
        assert empty.tolist() == [0.0, 1.0, 1.0, 0.0] and empty.dtype == np.float32
    # the order is a function of M alone: the same samples at other positions may round differently, the same positions never do
    assert ref(a, np.ones(a.size, dtype=bool), eps).tolist() == ref(a.copy(), np.ones(a.size, dtype=bool), eps).tolist()


def test_trainers_parse_adv_norm():
    ppo = load_script("train/ppo_torch.py")
    assert ppo.parse_args([]).adv_norm == "batch"
    assert ppo.parse_args(["--adv-norm", "minibatch"]).adv_norm == "minibatch"                      # the torch update takes it too
    assert ppo.parse_args(["--mode", "native", "--update", "native", "--adv-norm", "minibatch"]).adv_norm == "minibatch"
    assert ppo.parse_args(["--adv-norm", "batch"]).adv_norm == "batch"
    pbt = load_script("train/pbt_native.py")
    assert pbt.parse_args([]).adv_norm == "batch" and pbt.parse_args(["--adv-norm", "minibatch"]).adv_norm == "minibatch"
    for mod in (ppo, pbt):
        for bad in ("none", "population", ""):
            with pytest.raises(SystemExit):
                mod.parse_args(["--adv-norm", bad])
    with pytest.raises(ValueError):
        ppo.train(adv_norm="none")                                                                  # refused before any device is touched
