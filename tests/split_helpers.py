"""Shared by the separate-value-network GPU tests: seeded separate-tower modules and their NativePolicy, the shared policy over one
tower, small handles per obs_dim, synthetic rollout-shaped batches, and the extended PPO loss on a separate-tower packed buffer."""
import numpy as np

DEV = "cuda:0"
# obs_dim D = history * (6 + n_beams)
HIST_BEAMS = {7: (1, 1), 22: (1, 16), 176: (8, 16)}


def env_config(history):
    from ship_sim_gym_amd.config import EnvConfig

    class E(EnvConfig):
        HISTORY_SIZE = history
    return E


def vec(n, D, base=0, n_maps=4):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    history, n_beams = HIST_BEAMS[D]
    env = ShipVecEnv(n, n_maps=n_maps, n_beams=n_beams, env_config=env_config(history), env_id_base=base)
    assert env.states_history == D
    return env


def split_module(torch, D, H=64, layers=2, act="tanh", A=3, seed=0, same_towers=False, device=DEV):
    """A module declaring pi_body, pi, vf_body, v with seeded uniform weights (helpers.actor_critic_policy's scaling); same_towers: the
    vf tower holds the pi tower's numbers."""
    nn = torch.nn
    g = torch.Generator().manual_seed(seed)

    def tower():
        mods = [nn.Linear(D, H), nn.Tanh() if act == "tanh" else nn.ReLU()]
        if layers == 2:
            mods += [nn.Linear(H, H), nn.Tanh() if act == "tanh" else nn.ReLU()]
        return nn.Sequential(*mods)

    net = nn.Module()
    net.pi_body, net.pi, net.vf_body, net.v = tower(), nn.Linear(H, A), tower(), nn.Linear(H, 1)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2 - 1).mul_(1.5 / p.shape[-1] ** 0.5)
        if same_towers:
            for p, q in zip(net.vf_body.parameters(), net.pi_body.parameters()):
                p.copy_(q)
    return net.to(device)


def split_policy(torch, D, H=64, layers=2, act="tanh", A=3, seed=0, same_towers=False, device=DEV):
    from ship_sim_gym_amd.policy import NativePolicy
    net = split_module(torch, D, H, layers, act, A, seed, same_towers, device)
    pol = NativePolicy.from_actor_critic(net, torch.full((D,), 600.0, dtype=torch.float64, device=device))
    assert pol.separate_value
    return net, pol


def shared_over_pi_tower(torch, net, pol):
    """The shared NativePolicy over `net`'s pi tower and both heads (its own copy of the numbers)."""
    from ship_sim_gym_amd.policy import NativePolicy
    mods = list(net.pi_body)
    layers = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in mods[0::2]]
    heads = [(m.weight.detach().clone(), m.bias.detach().clone()) for m in (net.pi, net.v)]
    out = NativePolicy(layers, heads[0], heads[1], pol.obs_scale, activation=pol.activation)
    assert not out.separate_value
    return out


def unpack(p, offsets):
    return {k: p[o: o + int(np.prod(s))].view(*s) for k, (o, s) in offsets.items()}


def split_forward(torch, p, offsets, L, act, x):
    """(logits, value) of a separate-tower packed buffer p (any dtype)."""
    t = unpack(p, offsets)
    f = torch.tanh if act == "tanh" else torch.relu
    h = f(x @ t["W0"].T + t["b0"])
    hv = f(x @ t["V0"].T + t["c0"])
    if L == 2:
        h = f(h @ t["W1"].T + t["b1"])
        hv = f(hv @ t["V1"].T + t["c1"])
    return h @ t["Wpi"].T + t["bpi"], (hv @ t["Wv"].T + t["bv"]).squeeze(-1)


def split_loss(torch, p, offsets, L, act, x, a, logp_old, advn, ret, v_old, lpa_old, clip=0.2, vf_coef=0.5, ent_coef=0.01, vf_clip=0.0,
               kl_coef=0.0):
    """tests/test_ppo_ext_gpu.py's ext_loss over separate towers: (loss, pg, mean VL, entropy mean, clip fraction, mean KL)."""
    logits, v = split_forward(torch, p, offsets, L, act, x)
    lpa = torch.log_softmax(logits, -1)
    ratio = torch.exp(lpa.gather(-1, a.unsqueeze(-1)).squeeze(-1) - logp_old)
    pg = -torch.min(ratio * advn, torch.clamp(ratio, 1 - clip, 1 + clip) * advn).mean()
    l1 = (v - ret).pow(2)
    l2 = (v_old + torch.clamp(v - v_old, -vf_clip, vf_clip) - ret).pow(2)
    vl = torch.max(l1, l2).mean() if vf_clip > 0 else l1.mean()
    ent = -(lpa.exp() * lpa).sum(-1).mean()
    kl = (lpa_old.exp() * (lpa_old - lpa)).sum(-1).mean()
    cf = ((ratio - 1).abs() > clip).to(x.dtype).mean()
    loss = pg + vf_coef * vl - ent_coef * ent
    if kl_coef > 0:
        loss = loss + kl_coef * kl
    return loss, pg, vl, ent, cf, kl


def synthetic_batch(torch, pol, K, N, seed):
    """A rollout-shaped batch with controlled extremes (tests/test_ppo_domain_gpu.py's): rows at the real scale, reset rows (obs = -1),
    ~5 % of rows scaled x50; logp_old = the current policy's logp + U(-0.4, 0.4) (ratios clipped on both sides, ties inside),
    logp_all_old a perturbed copy of the current distribution, val = the current value + U(-0.2, 0.2)."""
    D, A = pol.obs_dim, pol.n_actions
    g = torch.Generator(device=DEV).manual_seed(seed)

    def u(*shape):
        return torch.rand(shape, generator=g, device=DEV, dtype=torch.float64)

    obs = u(K, N, D) * 600.0
    obs[u(K, N) < 0.1] = -1.0
    x = (obs / pol.obs_scale).float()
    x[u(K, N) < 0.05] *= 50.0
    act = (u(K, N) * A).long().clamp_(max=A - 1)
    with torch.no_grad():
        fwd = split_forward if pol.separate_value else shared_forward
        logits, v = fwd(torch, pol.params.detach().double(), pol.offsets, pol.n_hidden_layers, pol.activation, x.double())
        old = torch.log_softmax(torch.log_softmax(logits, -1) + 0.5 * torch.randn(logits.shape, generator=g, device=DEV, dtype=torch.float64), -1)
    logp_all = torch.zeros((K, N, 4), device=DEV)
    logp_all[..., :A] = old.float()
    logp = logp_all.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    return dict(obs=x.contiguous(), act=act.to(torch.int32).contiguous(), logp=logp.contiguous(), logp_all=logp_all.contiguous(),
                rew=torch.randn((K, N), generator=g, device=DEV, dtype=torch.float64), done=(u(K, N) < 0.05).to(torch.uint8),
                val=(v + (u(K, N) - 0.5) * 0.4).float().contiguous(), last_val=torch.randn((N,), generator=g, device=DEV))


def shared_forward(torch, p, offsets, L, act, x):
    t = unpack(p, offsets)
    f = torch.tanh if act == "tanh" else torch.relu
    h = f(x @ t["W0"].T + t["b0"])
    if L == 2:
        h = f(h @ t["W1"].T + t["b1"])
    return h @ t["Wpi"].T + t["bpi"], (h @ t["Wv"].T + t["bv"]).squeeze(-1)


def nan_fill(ppo, head=256):
    """Fill the workspace past the advantage statistics with NaN bytes: every slot entry must be written before it is read."""
    ppo.workspace[head:].fill_(0xFF)


def check_per_tensor(torch, pol, mine, ref64, ref32, what):
    """helpers.check_per_tensor (the project's bound), printing each figure before it asserts."""
    for k, (o, s) in pol.offsets.items():
        n = int(np.prod(s))
        g64 = ref64[o: o + n].double()
        e_mine = float((mine[o: o + n].double() - g64).abs().max())
        e_t32 = float((ref32[o: o + n].double() - g64).abs().max())
        bound = 4 * e_t32 + 1e-6 * float(g64.abs().max())
        print("%s %s: |mine - f64| %.3e  |torch f32 - f64| %.3e  bound %.3e" % (what, k, e_mine, e_t32, bound))
        assert e_mine <= bound, (what, k, e_mine, e_t32, bound)
