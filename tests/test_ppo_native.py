"""CPU-side checks of the device PPO update (GAE + gradient + Adam, ABI 9 additions): the new symbols in the header and the binding,
the ssg_ppo_hparams record against ctypes, argument refusals before any device work, and the trainer's --update option.  No GPU."""
import ctypes as C
import os
import re

import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PPO_SYMBOLS = ("ssg_ppo_workspace_nbytes", "ssg_ppo_gae", "ssg_ppo_grad", "ssg_ppo_adam", "ssg_ppo_update")


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def test_ppo_symbols_are_declared_exported_and_abi_stays_9(native):
    text = _header()
    L = native.lib()
    for name in PPO_SYMBOLS:
        assert re.search(r"^int\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in native.EXPORTS and hasattr(L, name), name
    assert native.ABI_VERSION == 9 and L.ssg_abi_version() == 9


def test_hparams_record_matches_the_header(native):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct ssg_ppo_hparams \{(.*?)\} ssg_ppo_hparams;", text, flags=re.S).group(1)
    names = []
    for ctype, decl in re.findall(r"(uint32_t|double)\s+([\w\s,]+);", body):
        names += [(ctype, n.strip()) for n in decl.split(",")]
    assert [n for _, n in names] == [f for f, _ in native.PpoHparams._fields_]
    size_of = {"uint32_t": 4, "double": 8}
    off = 0
    for ctype, name in names:
        sz = size_of[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(native.PpoHparams, name).offset == off, name
        off += sz
    assert C.sizeof(native.PpoHparams) == (off + 7) // 8 * 8 == 88


def _policy_record(native, D=32, H=64, L=2, A=3):
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = D, H, L, A, native.POLICY_TANH
    return p


def test_workspace_size_and_its_refusals(native):
    L = native.lib()
    pol = _policy_record(native)
    nb = C.c_size_t()
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 4096 * 32, 32768, C.byref(nb)) == 0
    P = 64 * 32 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 64 + 1
    assert nb.value >= 256 + 512 * (P + 4) * 4           # 512 workgroup slots of P + 4 floats at 32768 samples
    small = C.c_size_t()
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 100, 100, C.byref(small)) == 0 and small.value < nb.value
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 0, 1, C.byref(nb)) == -1
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 1, 0, C.byref(nb)) == -1
    assert L.ssg_ppo_workspace_nbytes(C.byref(pol), 1, 1, None) == -1
    assert L.ssg_ppo_workspace_nbytes(None, 1, 1, C.byref(nb)) == -1
    bad = _policy_record(native, H=40)
    assert L.ssg_ppo_workspace_nbytes(C.byref(bad), 1, 1, C.byref(nb)) == -1


def test_ppo_entry_points_refuse_before_touching_a_device(native):
    """Without a bound state blob every compute entry point returns SSG_ERR_NOT_BOUND (nothing enqueued); no handle: BAD_ARG."""
    L = native.lib()
    c = native.default_config()
    c.n_envs = 64
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    pol, hp = native.Policy(), native.PpoHparams()
    try:
        assert L.ssg_ppo_gae(h, C.byref(hp), 1, 64, None, None, None, None, None, None, None, 0, None) == -3
        assert L.ssg_ppo_grad(h, C.byref(pol), C.byref(hp), 64, None, None, None, None, None, None, 64, None, None, None, 0, None) == -3
        assert L.ssg_ppo_adam(h, C.byref(pol), C.byref(hp), None, None, 1, None) == -3
        assert L.ssg_ppo_update(h, C.byref(pol), C.byref(hp), 64, None, None, None, None, None, None, 2, 4, None, 0, None, None, 0,
                                None) == -3
        assert L.ssg_ppo_gae(None, C.byref(hp), 1, 64, None, None, None, None, None, None, None, 0, None) == -1
        assert L.ssg_ppo_adam(None, C.byref(pol), C.byref(hp), None, None, 1, None) == -1
    finally:
        L.ssg_destroy(h)


def test_trainer_offers_native_update_only_with_native_mode():
    mod = load_script("train/ppo_torch.py")
    assert mod.parse_args(["--mode", "native", "--update", "native"]).update == "native"
    assert mod.parse_args([]).update == "torch" and mod.make_arg_parser().parse_args([]).update == "torch"
    for m in ("eager", "graph", "pingpong"):
        assert mod.parse_args(["--mode", m]).update == "torch"
        with pytest.raises(SystemExit):
            mod.parse_args(["--mode", m, "--update", "native"])
        with pytest.raises(ValueError, match="mode='native'"):
            mod.train(envs=64, updates=1, mode=m, update="native", device="cpu")
    with pytest.raises(ValueError):
        mod.train(envs=64, updates=1, mode="native", update="adam", device="cpu")


def test_update_chunks_are_torch_chunks():
    """NativePPO.update's chunk count (its stats rows and its Adam step advance, epochs x chunks) is torch.chunk's, also where
    torch.chunk makes fewer chunks than asked (n = 10 into 6 gives 5)."""
    import torch
    from ship_sim_gym_amd.ppo import chunk_split
    for n in range(1, 301):
        r = torch.arange(n)
        for m in range(1, 41):
            chunks = r.chunk(m)
            chunk, n_chunks = chunk_split(n, m)
            assert n_chunks == len(chunks) and chunk == len(chunks[0]), (n, m)
            assert [len(c) for c in chunks] == [min(chunk, n - i * chunk) for i in range(n_chunks)], (n, m)
    assert chunk_split(10, 6) == (2, 5)
