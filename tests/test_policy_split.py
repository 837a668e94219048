"""CPU-side checks of the separate value network (SSG_POLICY_SEPARATE_VALUE): the flag in the header and the binding with the pinned
record sizes, the workspace sizes for the longer packed row and their refusals of other flag bits, the packed layout against torch.cat
of a separate-tower module, what from_actor_critic accepts and refuses, and the trainers' --separate-value option.  No GPU."""
import ctypes as C
import itertools
import os
import re

import pytest

from gpu_support import load_script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "shipsim.h")).read()


def split_len(D, H, L, A):
    return 2 * (H * D + H + (L - 1) * (H * H + H)) + A * H + A + H + 1


def test_flag_in_header_and_binding_and_pinned_sizes(native):
    m = re.search(r"#define\s+SSG_POLICY_SEPARATE_VALUE\s+(0x[0-9a-fA-F]+|\d+)", _header())
    assert m and int(m.group(1), 0) == 0x100 == native.POLICY_SEPARATE_VALUE
    assert C.sizeof(native.Policy) == 40 and C.sizeof(native.Population) == 48
    assert native.ABI_VERSION == 9 and native.lib().ssg_abi_version() == 9
    assert int(re.search(r"#define\s+SSG_ABI_VERSION\s+(\d+)", _header()).group(1)) == 9


def _policy_record(native, activation, D=32, H=64, L=2, A=3):
    p = native.Policy()
    p.struct_size = C.sizeof(native.Policy)
    p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = D, H, L, A, activation
    return p


def _pop_record(native, activation, P=4, D=32, H=64, L=2, A=3):
    p = native.Population()
    p.struct_size = C.sizeof(native.Population)
    p.n_members, p.obs_dim, p.hidden, p.n_hidden_layers, p.n_actions, p.activation = P, D, H, L, A, activation
    return p


BAD_FLAGS = (0x200, 0x102, 0x100 | 0xff, 2, -1, 0x100 | 0x200, 0x10100)


def test_workspace_sizes_take_the_flag_and_refuse_other_bits(native):
    L = native.lib()
    P_shared = 64 * 32 + 64 + 64 * 64 + 64 + 3 * 64 + 3 + 64 + 1
    P_split = split_len(32, 64, 2, 3)
    assert P_split == P_shared + 64 * 32 + 64 + 64 * 64 + 64
    for kind in (native.POLICY_TANH, native.POLICY_RELU):
        shared, split = C.c_size_t(), C.c_size_t()
        assert L.ssg_ppo_workspace_nbytes(C.byref(_policy_record(native, kind)), 4096 * 32, 32768, C.byref(shared)) == 0
        assert L.ssg_ppo_workspace_nbytes(C.byref(_policy_record(native, kind | 0x100)), 4096 * 32, 32768, C.byref(split)) == 0
        assert split.value >= 256 + 512 * (P_split + 4) * 4     # 512 workgroup slots of P + 4 floats at 32768 samples
        assert split.value > shared.value
        pshared, psplit = C.c_size_t(), C.c_size_t()
        assert L.ssg_pop_workspace_nbytes(C.byref(_pop_record(native, kind)), 32768, 32768, C.byref(pshared)) == 0
        assert L.ssg_pop_workspace_nbytes(C.byref(_pop_record(native, kind | 0x100)), 32768, 32768, C.byref(psplit)) == 0
        assert psplit.value >= 4096 + 4 * 512 * (P_split + 4) * 4
        assert psplit.value > pshared.value
        assert psplit.value - 4096 == 4 * (split.value - 256)   # P times the single policy's slots, as for the shared shape
    out = C.c_size_t(12345)
    for bad in BAD_FLAGS:
        assert L.ssg_ppo_workspace_nbytes(C.byref(_policy_record(native, bad)), 4096 * 32, 32768, C.byref(out)) == -1, hex(bad)
        assert L.ssg_pop_workspace_nbytes(C.byref(_pop_record(native, bad)), 32768, 32768, C.byref(out)) == -1, hex(bad)
    assert out.value == 12345


def _towers(torch, D, H, L, A, act=None, H_vf=None, L_vf=None, act_vf=None):
    nn = torch.nn
    act = act or nn.Tanh

    def tower(h, l, a):
        mods = [nn.Linear(D, h), a()]
        if l == 2:
            mods += [nn.Linear(h, h), a()]
        return nn.Sequential(*mods)

    class Split(nn.Module):
        def __init__(self):
            super().__init__()
            self.pi_body = tower(H, L, act)
            self.pi = nn.Linear(H, A)
            self.vf_body = tower(H_vf or H, L_vf or L, act_vf or act)
            self.v = nn.Linear(H_vf or H, 1)

    return Split()


@pytest.mark.parametrize("D,H,L,A", list(itertools.product((7, 32), (16, 64), (1, 2), (2, 3, 4))))
def test_packed_offsets_are_torch_cat_of_a_separate_tower_module(D, H, L, A):
    import torch
    from ship_sim_gym_amd.policy import packed_offsets
    torch.manual_seed(D * 1000 + H * 10 + L * 5 + A)
    net = _towers(torch, D, H, L, A)
    flat = torch.cat([p.detach().flatten() for p in net.parameters()])
    offsets, total = packed_offsets(D, H, L, A, separate_value=True)
    assert total == flat.numel() == split_len(D, H, L, A)
    names = ["W0", "b0"] + (["W1", "b1"] if L == 2 else []) + ["Wpi", "bpi", "V0", "c0"] + (["V1", "c1"] if L == 2 else []) + ["Wv", "bv"]
    assert list(offsets) == names
    o = 0
    for name, p in zip(names, net.parameters()):
        off, shape = offsets[name]
        assert off == o and tuple(shape) == tuple(p.shape), name
        assert torch.equal(flat[off: off + p.numel()].view(*shape), p.detach()), name
        o += p.numel()
    # the flag off: today's layout, and the default
    shared, n_shared = packed_offsets(D, H, L, A)
    assert (shared, n_shared) == packed_offsets(D, H, L, A, separate_value=False)
    assert "V0" not in shared and n_shared == H * D + H + (L - 1) * (H * H + H) + A * H + A + H + 1


@pytest.mark.parametrize("L,act", [(1, "Tanh"), (2, "ReLU")])
def test_from_actor_critic_takes_the_separate_module_on_cpu(native, L, act):
    import torch
    from ship_sim_gym_amd.policy import NativePolicy
    torch.manual_seed(3)
    D, H, A = 7, 16, 3
    net = _towers(torch, D, H, L, A, act=getattr(torch.nn, act))
    pol = NativePolicy.from_actor_critic(net, 2.0)
    assert pol.separate_value and (pol.obs_dim, pol.hidden, pol.n_hidden_layers, pol.n_actions, pol.activation) == (D, H, L, A, act.lower())
    assert torch.equal(pol.params, torch.cat([p.detach().flatten() for p in net.parameters()]))
    rec = pol.to_native()
    assert rec.activation == (native.POLICY_SEPARATE_VALUE | (native.POLICY_RELU if act == "ReLU" else native.POLICY_TANH))
    assert set(pol.unpack()) >= {"V0", "c0", "Wv", "bv"}
    # forward_reference is the module's forward
    obs = torch.randn(5, D, dtype=torch.float64)
    x, logits, value = pol.forward_reference(obs)
    with torch.no_grad():
        assert torch.allclose(logits, net.pi(net.pi_body(x)), atol=1e-6)
        assert torch.allclose(value, net.v(net.vf_body(x)).squeeze(-1), atol=1e-6)
        # refresh() follows the module, both towers
        net.vf_body[0].weight.add_(1.0)
        net.pi_body[0].bias.sub_(1.0)
    pol.refresh()
    assert torch.equal(pol.unpack()["V0"], net.vf_body[0].weight.detach()) and torch.equal(pol.unpack()["b0"], net.pi_body[0].bias.detach())
    # a shared module still gives the shared record
    mod = load_script("train/ppo_torch.py")
    shared = NativePolicy.from_actor_critic(mod.ActorCritic(D, A, hidden=H), 2.0)
    assert not shared.separate_value and shared.to_native().activation == native.POLICY_TANH


def test_from_actor_critic_refuses_unequal_towers_and_mixed_modules():
    import torch
    from ship_sim_gym_amd.policy import NativePolicy
    nn = torch.nn
    D, H, A = 7, 16, 3
    for kw in (dict(L_vf=1), dict(H_vf=32), dict(act_vf=nn.ReLU)):
        with pytest.raises(ValueError, match="pi_body"):
            NativePolicy.from_actor_critic(_towers(torch, D, H, 2, A, **kw), 2.0)
    both = _towers(torch, D, H, 2, A)
    both.body = nn.Sequential(nn.Linear(D, H), nn.Tanh())
    with pytest.raises(ValueError, match="both body and pi_body"):
        NativePolicy.from_actor_critic(both, 2.0)
    half = _towers(torch, D, H, 2, A)
    del half.vf_body
    with pytest.raises(ValueError, match="body = nn.Sequential.*pi_body"):
        NativePolicy.from_actor_critic(half, 2.0)
    with pytest.raises(ValueError, match="body = nn.Sequential.*pi_body"):
        NativePolicy.from_actor_critic(nn.Linear(D, A), 2.0)
    # the constructor's own check: towers of another depth or width
    pol_layers = [(torch.zeros(H, D), torch.zeros(H))]
    heads = ((torch.zeros(A, H), torch.zeros(A)), (torch.zeros(1, H), torch.zeros(1)))
    with pytest.raises(ValueError, match="depth"):
        NativePolicy(pol_layers, heads[0], heads[1], 2.0, value_layers=pol_layers + [(torch.zeros(H, H), torch.zeros(H))])
    with pytest.raises(ValueError):
        NativePolicy(pol_layers, heads[0], (torch.zeros(1, 32), torch.zeros(1)), 2.0, value_layers=[(torch.zeros(32, D), torch.zeros(32))])


def test_population_refuses_mixed_shapes():
    import torch
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.population import NativePopulation
    D, H, A = 7, 16, 3
    mod = load_script("train/ppo_torch.py")
    split = NativePolicy.from_actor_critic(_towers(torch, D, H, 2, A), 2.0)
    shared = NativePolicy.from_actor_critic(mod.ActorCritic(D, A, hidden=H), 2.0)
    with pytest.raises(ValueError, match="member 1"):
        NativePopulation([split, shared])
    pop = NativePopulation([split, NativePolicy.from_actor_critic(_towers(torch, D, H, 2, A), 2.0)])
    assert pop.separate_value and pop.n_params == split_len(D, H, 2, A)
    assert pop.to_native().activation == 0x100


def test_trainers_offer_separate_value_and_keep_the_shared_module():
    import torch
    mod = load_script("train/ppo_torch.py")
    assert mod.parse_args([]).separate_value is False
    for m in ("eager", "graph", "pingpong", "native"):
        assert mod.parse_args(["--mode", m, "--separate-value"]).separate_value is True
    assert mod.parse_args(["--mode", "native", "--update", "native", "--separate-value"]).separate_value is True
    keys = ["body.0.weight", "body.0.bias", "body.2.weight", "body.2.bias", "pi.weight", "pi.bias", "v.weight", "v.bias"]
    assert list(mod.ActorCritic(32, 3).state_dict()) == keys == list(mod.ActorCritic(32, 3, separate_value=False).state_dict())
    # the shared module's initial values are what they were: the same draws in the same order
    torch.manual_seed(5)
    a = mod.ActorCritic(32, 3)
    torch.manual_seed(5)
    nn = torch.nn
    body = nn.Sequential(nn.Linear(32, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh())
    pi, v = nn.Linear(64, 3), nn.Linear(64, 1)
    for p, q in zip(a.parameters(), list(body.parameters()) + list(pi.parameters()) + list(v.parameters())):
        assert torch.equal(p, q)
    sep = mod.ActorCritic(32, 3, separate_value=True)
    assert [n for n, _ in sep.named_children()] == ["pi_body", "pi", "vf_body", "v"]
    logits, value = sep(torch.zeros(5, 32))
    assert tuple(logits.shape) == (5, 3) and tuple(value.shape) == (5,)
    pbt = load_script("train/pbt_native.py")
    assert pbt.parse_args([]).separate_value is False and pbt.parse_args(["--separate-value"]).separate_value is True
