"""CPU-side checks of the policy in the loop (ABI 9): the packed parameter layout include/shipsim.h documents, the module checks of
NativePolicy.from_actor_critic, the ctypes record against the header, and the trainer's `native` mode.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


class _AC(nn.Module):
    """ppo_torch.ActorCritic's shape with the knobs the native policy accepts."""

    def __init__(self, D, A, H=64, layers=2, act=nn.Tanh):
        super().__init__()
        mods = [nn.Linear(D, H), act()]
        for _ in range(layers - 1):
            mods += [nn.Linear(H, H), act()]
        self.body = nn.Sequential(*mods)
        self.pi = nn.Linear(H, A)
        self.v = nn.Linear(H, 1)

    def forward(self, x):
        h = self.body(x)
        return self.pi(h), self.v(h).squeeze(-1)


def _header_offsets(D, H, L, A):
    """The layout as the header's comment states it, restated from its formulas (o1, oh, total)."""
    o1 = H * D + H
    oh = o1 + (H * H + H if L == 2 else 0)
    offs = {"W0": (0, (H, D)), "b0": (H * D, (H,))}
    if L == 2:
        offs.update({"W1": (o1, (H, H)), "b1": (o1 + H * H, (H,))})
    offs.update({"Wpi": (oh, (A, H)), "bpi": (oh + A * H, (A,)), "Wv": (oh + A * H + A, (1, H)), "bv": (oh + A * H + A + H, (1,))})
    total = H * D + H + (L - 1) * (H * H + H) + A * H + A + H + 1
    return offs, total


def _numpy_forward(buf, D, H, L, A, act, x):
    """A forward that reads ONLY the packed buffer, at the header's offsets."""
    offs, total = _header_offsets(D, H, L, A)
    assert buf.shape == (total,)
    g = lambda k: buf[offs[k][0]: offs[k][0] + int(np.prod(offs[k][1]))].reshape(offs[k][1]).astype(np.float64)
    f = np.tanh if act == "tanh" else (lambda z: np.maximum(z, 0.0))
    h = f(x @ g("W0").T + g("b0"))
    if L == 2:
        h = f(h @ g("W1").T + g("b1"))
    return h @ g("Wpi").T + g("bpi"), (h @ g("Wv").T + g("bv"))[:, 0]


def test_packing_is_torch_cat_of_the_actor_critic_parameters():
    from ship_sim_gym_amd.policy import NativePolicy, packed_offsets
    mod = load_script("train/ppo_torch.py")
    torch.manual_seed(0)
    net = mod.ActorCritic(32, 3)
    pol = NativePolicy.from_actor_critic(net, torch.full((32,), 600.0, dtype=torch.float64))
    assert torch.equal(pol.params, torch.cat([p.detach().flatten() for p in net.parameters()]))
    assert (pol.obs_dim, pol.hidden, pol.n_hidden_layers, pol.n_actions, pol.activation) == (32, 64, 2, 3, "tanh")
    offs, total = _header_offsets(32, 64, 2, 3)
    assert packed_offsets(32, 64, 2, 3) == (offs, total)
    # refresh() re-packs in place: same storage, the new values
    addr = pol.params.data_ptr()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.25)
    pol.refresh()
    assert pol.params.data_ptr() == addr
    assert torch.equal(pol.params, torch.cat([p.detach().flatten() for p in net.parameters()]))


@pytest.mark.parametrize("D,H,L,A,act", [(32, 64, 2, 3, "tanh"), (14, 16, 1, 2, "relu"), (176, 128, 2, 4, "tanh"), (48, 32, 1, 3, "relu")])
def test_numpy_forward_over_the_packed_buffer_matches_torch(D, H, L, A, act):
    from ship_sim_gym_amd.policy import NativePolicy
    torch.manual_seed(D + H)
    net = _AC(D, A, H, L, nn.Tanh if act == "tanh" else nn.ReLU)
    scale = torch.linspace(200.0, 600.0, D, dtype=torch.float64)
    pol = NativePolicy.from_actor_critic(net, scale)
    obs = torch.rand((257, D), dtype=torch.float64) * 600.0 - 1.0
    x = (obs / scale).float()
    with torch.no_grad():
        logits, value = net(x)
    lg, v = _numpy_forward(pol.params.numpy(), D, H, L, A, act, x.numpy().astype(np.float64))
    np.testing.assert_allclose(lg, logits.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(v, value.numpy(), atol=1e-6, rtol=0)
    xr, lr, vr = pol.forward_reference(obs)
    assert torch.equal(xr, x)
    np.testing.assert_allclose(lr.numpy(), logits.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(vr.numpy(), value.numpy(), atol=1e-6, rtol=0)


def test_from_actor_critic_rejects_what_the_kernel_cannot_run():
    from ship_sim_gym_amd.policy import NativePolicy
    s = 600.0
    NativePolicy.from_actor_critic(_AC(32, 3, 128, 2), s)                    # the limits themselves pass
    NativePolicy.from_actor_critic(_AC(32, 4, 16, 1, nn.ReLU), s)
    for bad in (_AC(32, 3, 130, 2), _AC(32, 3, 40, 2), _AC(32, 3, 144, 1), _AC(32, 3, 64, 3), _AC(32, 5, 64, 2), _AC(32, 1, 64, 2)):
        with pytest.raises(ValueError):
            NativePolicy.from_actor_critic(bad, s)
    mixed = _AC(32, 3, 64, 2)
    mixed.body[3] = nn.ReLU()
    wrong_act = _AC(32, 3, 64, 1)
    wrong_act.body[1] = nn.Sigmoid()
    no_bias = _AC(32, 3, 64, 1)
    no_bias.body[0] = nn.Linear(32, 64, bias=False)
    two_values = _AC(32, 3, 64, 1)
    two_values.v = nn.Linear(64, 2)
    not_seq = _AC(32, 3, 64, 1)
    not_seq.body = nn.ModuleList(list(not_seq.body))
    for bad in (mixed, wrong_act, no_bias, two_values, not_seq, nn.Linear(3, 3)):
        with pytest.raises(ValueError):
            NativePolicy.from_actor_critic(bad, s)
    with pytest.raises(ValueError):
        NativePolicy.from_actor_critic(_AC(32, 3, 64, 2), torch.ones(31, dtype=torch.float64))  # obs_scale of the wrong length
    with pytest.raises(ValueError):
        NativePolicy.from_actor_critic(_AC(32, 3, 64, 2).double(), s)                           # f32 parameters only


def test_policy_record_matches_the_header(native):
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct ssg_policy \{(.*?)\} ssg_policy;", text, flags=re.S).group(1)
    fields = re.findall(r"(uint32_t|int32_t|const float \*|const double \*)\s*(\w+);", body)
    names = [f for _, f in fields]
    assert names == [f for f, _ in native.Policy._fields_]
    size_of = {"uint32_t": 4, "int32_t": 4, "const float *": 8, "const double *": 8}
    off = 0
    for (ctype, name), (pname, ptype) in zip(fields, native.Policy._fields_):
        sz = size_of[ctype]
        off = (off + sz - 1) // sz * sz
        assert getattr(native.Policy, name).offset == off, name
        assert C.sizeof(ptype) == sz, name
        off += sz
    assert C.sizeof(native.Policy) == (off + 7) // 8 * 8 == 40
    consts = dict(re.findall(r"#define\s+(SSG_POLICY_[A-Z_]+)\s+(\d+)", _header()))
    assert int(consts["SSG_POLICY_MAX_HIDDEN"]) == native.POLICY_MAX_HIDDEN == 128
    assert (int(consts["SSG_POLICY_TANH"]), int(consts["SSG_POLICY_RELU"])) == (native.POLICY_TANH, native.POLICY_RELU)


def test_abi9_symbols_are_exported(native):
    assert native.ABI_VERSION == 9
    L = native.lib()
    assert L.ssg_abi_version() == 9
    for name in ("ssg_policy_act", "ssg_rollout_policy"):
        assert name in native.EXPORTS and hasattr(L, name)


def test_policy_entry_points_refuse_before_touching_a_device(native):
    """Without a bound state blob both entry points return an error code (nothing enqueued), like every compute entry point."""
    L = native.lib()
    c = native.default_config()
    c.n_envs = 64
    h = C.c_void_p()
    native.check(L.ssg_create(C.byref(c), C.byref(h)))
    pol = native.Policy()
    assert L.ssg_policy_act(h, C.byref(pol), None, None, 0, 0, None, None, None, None, None) == -3
    assert L.ssg_rollout_policy(h, C.byref(pol), 1, None, 0, 0, None, None, None, None, None, None, None, None, None, 64, None) == -3
    assert L.ssg_policy_act(None, C.byref(pol), None, None, 0, 0, None, None, None, None, None) == -1
    L.ssg_destroy(h)


def test_trainer_offers_native_mode():
    mod = load_script("train/ppo_torch.py")
    ap = mod.make_arg_parser()
    assert ap.parse_args(["--mode", "native"]).mode == "native"
    for m in ("eager", "graph", "pingpong"):
        assert ap.parse_args(["--mode", m]).mode == m
    assert ap.parse_args([]).mode == "graph"
