"""GPU checks of GAE and the PPO update on the device (ship_sim_gym_amd/ppo.py, ssg_ppo_*): GAE bitwise against train/ppo_torch.py's
loop, the minibatch gradient against an f64 autograd reference, Adam against torch.optim.Adam, a whole update against the f64
reference of the same update (and run to run bitwise), and ppo_torch's --update native."""
import numpy as np
import pytest

from gpu_support import load_script, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _policy, check_per_tensor as _check_per_tensor, forward as _forward, \
    ref_grad as _ref_grad, ref_update as _ref_update, torch_gae as _torch_gae

pytestmark = pytest.mark.gpu


def _vec(n):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64)


def _rollout(torch, env, pol, K, seed=1):
    env.reset_tensor()
    return dict(env.rollout_policy(pol, K, seed=seed))


@pytest.mark.parametrize("n,K", [(1000, 16), (4097, 8), (512, 1)])
def test_gae_is_bitwise_the_trainers_loop(torch_cuda, n, K):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec(n)
    _, pol = _policy(torch, env.states_history)
    b = _rollout(torch, env, pol, K)
    # real dones, plus forced ones so that every K sees terminations mid-rollout
    g = torch.Generator(device="cuda:0").manual_seed(n + K)
    b["done"] = (b["done"] | (torch.rand(b["done"].shape, generator=g, device="cuda:0") < 0.05)).to(torch.uint8).contiguous()
    assert int(b["done"].sum()) > 0
    ppo = NativePPO(pol, env)
    adv, ret = ppo.gae(b, 0.99, 0.95)
    ref_adv, ref_ret = _torch_gae(torch, b)
    assert torch.equal(adv, ref_adv) and torch.equal(ret, ref_ret)
    flat = ref_adv.reshape(-1)
    ref_norm = (flat - flat.mean()) / (flat.std() + 1e-8)
    st = ppo.adv_stats()
    mine = (adv.reshape(-1) - st[0]) / st[1]
    assert float((mine - ref_norm).abs().max()) <= 1e-5
    env.close()


def _batch_for(torch, H, L, act, A, n=4096, K=10, seed=0):
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec(n)
    _, pol = _policy(torch, env.states_history, H, L, act, A, seed=seed)
    b = _rollout(torch, env, pol, K, seed=seed + 7)
    ppo = NativePPO(pol, env)
    ppo.gae(b)
    # logp of an older policy: ratios clipped on both sides, and (where |log r| is small) ties of min() inside the clip range
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    b["logp"] = (b["logp"] + (torch.rand(b["logp"].shape, generator=g, device="cuda:0") - 0.5) * 0.8).contiguous()
    st = ppo.adv_stats()
    advn = (b["adv"].reshape(-1) - st[0]) / st[1]
    return env, pol, ppo, b, advn


@pytest.mark.parametrize("H,L,act,A", [(16, 1, "relu", 2), (64, 2, "tanh", 3), (128, 2, "relu", 4), (128, 1, "tanh", 3),
                                       (64, 1, "relu", 4), (16, 2, "tanh", 4)])
def test_grad_matches_f64_autograd(torch_cuda, H, L, act, A):
    torch = torch_cuda
    env, pol, ppo, b, advn = _batch_for(torch, H, L, act, A, seed=H + L + A)
    n = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(5)
    perm = torch.randperm(n, device="cuda:0", generator=g)
    sizes = [3000, n] if (H, L) == (64, 2) else [3000]
    for M in sizes:
        idx = perm[:M]
        mine, st = ppo.grad(b, idx, stats=True)
        again = ppo.grad(b, idx)
        assert torch.equal(mine, again)                      # bitwise run to run
        r64, terms64 = _ref_grad(torch, pol, b, idx, advn, torch.float64)
        r32, terms32 = _ref_grad(torch, pol, b, idx, advn, torch.float32)
        _check_per_tensor(torch, pol, mine, r64, r32, (H, L, act, A, M))
        ratio_inside = terms64[3] < 1.0
        assert ratio_inside and terms64[3] > 0.0, terms64      # clipped samples exist, and so do ties inside the range
        for got, want in zip(st.tolist(), terms32):
            assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, (st.tolist(), terms32)
    env.close()


def test_clipped_on_both_sides_and_ties(torch_cuda):
    """The default network's batch has ratios below 1-clip, above 1+clip, and inside (min() ties)."""
    torch = torch_cuda
    env, pol, ppo, b, advn = _batch_for(torch, 64, 2, "tanh", 3)
    with torch.no_grad():
        logits, _ = _forward(torch, pol.params, pol.offsets, pol.n_hidden_layers, pol.activation, b["obs"].reshape(-1, pol.obs_dim))
        lp = torch.log_softmax(logits, -1).gather(-1, b["act"].reshape(-1, 1).long()).squeeze(-1)
        r = torch.exp(lp - b["logp"].reshape(-1))
    assert int((r < 0.8).sum()) > 0 and int((r > 1.2).sum()) > 0 and int(((r >= 0.8) & (r <= 1.2)).sum()) > 0
    env.close()


def test_adam_matches_torch_optim(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env = _vec(64)
    _, pol = _policy(torch, env.states_history)
    ppo = NativePPO(pol, env, lr=3e-4)
    ref = pol.params.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=3e-4)
    g = torch.Generator(device="cuda:0").manual_seed(3)
    for _ in range(10):
        grad = torch.randn(ref.shape, generator=g, device="cuda:0") * 0.1
        ppo.adam_step(grad)
        ref.grad = grad.clone()
        opt.step()
    torch.testing.assert_close(pol.params, ref.detach(), rtol=1e-6, atol=1e-7)
    env.close()


def test_whole_update_against_f64_and_run_to_run(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env, pol, ppo, b, advn = _batch_for(torch, 64, 2, "tanh", 3, n=2048, K=8)
    n = b["act"].numel()
    g = torch.Generator(device="cuda:0").manual_seed(11)
    perm = torch.stack([torch.randperm(n, device="cuda:0", generator=g) for _ in range(2)])
    p0 = pol.params.detach().clone()
    r64 = _ref_update(torch, pol, b, advn, perm, 4, torch.float64)[0]
    r32 = _ref_update(torch, pol, b, advn, perm, 4, torch.float32)[0]
    st = ppo.update(b, perm, 2, 4, stats=True)
    assert st.shape == (8, 4) and bool(torch.isfinite(st).all())
    first = pol.params.detach().clone()
    _check_per_tensor(torch, pol, first, r64, r32, "update")
    # again from the same start: bitwise the same parameters
    stats = ppo.adv_stats().clone()
    pol.params.copy_(p0)
    ppo2 = NativePPO(pol, env)
    ppo2._ws(n, -(-n // 4))
    ppo2.workspace[:12].view(torch.float32).copy_(stats)
    ppo2.update(b, perm, 2, 4)
    assert torch.equal(pol.params, first)
    env.close()


def test_trainer_native_update(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/ppo_torch.py")
    hist, det = mod.train(envs=4096, updates=3, horizon=32, log=lambda s: None, mode="native", update="native", return_details=True)
    assert len(hist) == 3 and all(np.isfinite(h[1]) and np.isfinite(h[3]) for h in hist)
    assert det["update_seconds"] > 0 and all(bool(torch.isfinite(p).all()) for p in det["params"])
    # the first update sees the same first rollout and the same minibatches in both update paths
    _, nat = mod.train(envs=4096, updates=1, horizon=32, log=lambda s: None, mode="native", update="native", return_details=True)
    _, ref = mod.train(envs=4096, updates=1, horizon=32, log=lambda s: None, mode="native", update="torch", return_details=True)
    for a, b in zip(nat["snapshots"][0].values(), ref["snapshots"][0].values()):
        assert torch.equal(a, b)
    torch.manual_seed(0)  # train()'s own start: the seed, the probe env, then the module (its initial parameters)
    probe = mod.ShipVecEnv(1, mod.GameConfig, mod.EnvConfig, device="cuda:0", n_maps=1)
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    net0 = mod.ActorCritic(D, A)
    for pn, pr, p0 in zip(nat["params"], ref["params"], net0.parameters()):
        dn, dr = pn.cpu() - p0.detach(), pr.cpu() - p0.detach()
        assert float((dn - dr).norm()) <= 0.02 * float(dr.norm()) + 1e-7, (float((dn - dr).norm()), float(dr.norm()))
    # load_into round-trips the packed buffer into a module
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.policy import NativePolicy
    env = _vec(64)
    net, pol = _policy(torch, env.states_history)
    ppo = NativePPO(pol, env)
    ppo.adam_step(torch.ones(pol.params.numel(), device="cuda:0"))
    other, _ = _policy(torch, env.states_history, seed=9)
    ppo.load_into(other)
    assert torch.equal(NativePolicy.from_actor_critic(other, 600.0).params, pol.params)
    env.close()
