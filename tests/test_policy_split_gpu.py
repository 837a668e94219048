"""GPU checks of the policy forward with a separate value network (SSG_POLICY_SEPARATE_VALUE; ssg_policy_act, ssg_rollout_policy,
ssg_ppo_dist).  A separate policy whose vf tower holds its pi tower's numbers runs the chains the shared policy runs, so its outputs are
the shared policy's bit for bit; with different towers the outputs follow forward_reference within the bounds of
tests/test_policy_native_gpu.py, the logits depend on the pi tower alone and the value on the vf tower alone, and an env's outputs do
not depend on the sharding.  Records with other flag bits are refused before anything is launched."""
import ctypes as C

import pytest

from gpu_support import DEV, check_near_rows as _check_near, torch_cuda, torch_sample as _torch_sample, vec  # noqa: F401
from ppo_reference import assert_same_rollout, shared_over_pi_tower, split_policy, stepwise_rollout

pytestmark = pytest.mark.gpu

# (n envs, D, H, L, A, act): n = one full wave / one wave plus a tail; every D, H, L, A and activation, and every pair (L, H), (L, A),
# (act, L) among them; the last case is the largest LDS footprint (three activation buffers at D = 176, H = 128)
CASES = [(64, 7, 16, 1, 2, "tanh"), (100, 22, 48, 2, 3, "relu"), (100, 7, 128, 2, 4, "tanh"), (64, 22, 16, 2, 4, "relu"),
         (100, 22, 128, 1, 3, "tanh"), (64, 7, 48, 1, 4, "relu"), (100, 7, 48, 2, 2, "tanh"), (64, 22, 128, 1, 2, "relu"),
         (100, 22, 16, 1, 3, "relu"), (100, 176, 128, 2, 3, "tanh")]


def _warm(env, steps=6):
    env.reset_tensor()
    acts = env.random_actions(5, 0, steps)
    for k in range(steps):
        env.step_tensor(acts[k])


@pytest.mark.parametrize("n,D,H,L,A,act", CASES)
def test_identical_towers_are_the_shared_policy_bitwise(torch_cuda, n, D, H, L, A, act):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    net, split = split_policy(torch, D, H, L, act, A, seed=n + D + H, same_towers=True)
    shared = shared_over_pi_tower(torch, net, split)
    a, b = vec(n, D), vec(n, D)
    _warm(a)
    _warm(b)
    assert torch.equal(a.obs, b.obs)
    u = torch.rand(n, generator=torch.Generator(device=DEV).manual_seed(D + H), device=DEV)
    # one forward, caller uniforms
    got, want = a.policy_act(split, uniforms=u), b.policy_act(shared, uniforms=u)
    for name, g, w in zip(("act", "logp", "value", "x"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), name
    # the fused rollout under the separate policy = the step-by-step loop under the shared one, dev_last_value included
    K = 5
    U = torch.rand((K, n), generator=torch.Generator(device=DEV).manual_seed(n), device=DEV)
    fused = a.rollout_policy(split, K, uniforms=U)
    step = stepwise_rollout(b, shared, K, 0, 0, uniforms=U)
    assert_same_rollout(torch, fused, step, "fused split = stepwise shared")
    assert torch.equal(a.obs, b.obs)
    # and its own step-by-step loop (Philox): the value-only forward is the full forward's value
    _warm(a)
    _warm(b)
    fused = a.rollout_policy(split, K, seed=9, step0=2)
    assert_same_rollout(torch, fused, stepwise_rollout(b, split, K, 9, 2), "fused split = stepwise split")
    # the whole log-distribution over the stored rows
    la_split, la_shared = NativePPO(split, a).dist(dict(fused)), NativePPO(shared, a).dist(dict(fused))
    assert torch.equal(la_split, la_shared)
    assert torch.equal(la_split.gather(-1, fused["act"].long().unsqueeze(-1)).squeeze(-1), fused["logp"])
    assert bool((la_split[..., A:] == 0).all())
    a.close()
    b.close()


@pytest.mark.parametrize("n,D,H,L,A,act", CASES)
def test_independent_towers_follow_the_reference_and_do_not_mix(torch_cuda, n, D, H, L, A, act):
    torch = torch_cuda
    net, pol = split_policy(torch, D, H, L, act, A, seed=3 * n + D + H)
    env = vec(n, D)
    _warm(env)
    obs = env.obs.clone()
    u = torch.rand(n, generator=torch.Generator(device=DEV).manual_seed(D * H), device=DEV)
    a, logp, val, x = env.policy_act(pol, uniforms=u)
    xr, logits, vr = pol.forward_reference(obs)
    assert torch.equal(x, (obs / pol.obs_scale).float()) and torch.equal(xr, x)
    ar, lpr, cdf = _torch_sample(torch, logits, u)
    near = (u.unsqueeze(-1) - cdf[:, :-1]).abs().min(dim=-1).values < 1e-5
    assert int(near.sum()) <= 1
    ok = ~near
    print("max |logp - ref| %.3e  max |value - ref| %.3e" % (float((logp - lpr)[ok].abs().max()), float((val - vr).abs().max())))
    assert torch.equal(a.long()[ok], ar[ok])
    assert float((logp - lpr)[ok].abs().max()) <= 1e-4
    _check_near(torch, near, u, cdf, a, logp, torch.log_softmax(logits.double(), -1), 1e-4)   # the f64 logp of the action stored
    assert bool(((val - vr).abs() <= 1e-5 * (1 + vr.abs())).all()), float((val - vr).abs().max())
    assert torch.equal(env.obs, obs)
    # the towers really differ: the value is not the shared policy's over the pi tower
    assert not torch.equal(val, env.policy_act(shared_over_pi_tower(torch, net, pol), uniforms=u)[2])
    # only the vf tower (and its head) moves: act and logp keep their bits, the value moves
    p0 = pol.params.clone()
    o = pol.offsets
    vf0, vf1 = o["V0"][0], pol.params.numel()
    g = torch.Generator(device=DEV).manual_seed(1)
    pol.params[vf0:vf1] += 0.05 * torch.randn(vf1 - vf0, generator=g, device=DEV)
    a2, logp2, val2, _ = env.policy_act(pol, uniforms=u)
    assert torch.equal(a2, a) and torch.equal(logp2, logp) and not torch.equal(val2, val)
    # only the pi tower (and its head) moves: the value keeps its bits
    pol.params.copy_(p0)
    pol.params[:vf0] += 0.05 * torch.randn(vf0, generator=g, device=DEV)
    a3, logp3, val3, _ = env.policy_act(pol, uniforms=u)
    assert torch.equal(val3, val) and not torch.equal(logp3, logp)
    env.close()


def test_shard_invariance(torch_cuda):
    """2048 envs = 1024 + 1024, Philox keyed by the global env id (default env: D = 32; H = 64, L = 2)."""
    torch = torch_cuda
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    K = 8
    whole = ShipVecEnv(2048, n_maps=64)
    halves = [ShipVecEnv(1024, n_maps=64, env_id_base=0), ShipVecEnv(1024, n_maps=64, env_id_base=1024)]
    for e in [whole] + halves:
        e.reset_tensor()
    _, pol = split_policy(torch, whole.states_history)
    w = whole.rollout_policy(pol, K, seed=3, step0=7)
    hs = [h.rollout_policy(pol, K, seed=3, step0=7) for h in halves]
    for k in w:
        assert torch.equal(w[k], torch.cat([h[k] for h in hs], dim=0 if k == "last_val" else 1)), k
    a, lp, v, x = whole.policy_act(pol, seed=3, step=7 + K)
    parts = [h.policy_act(pol, seed=3, step=7 + K) for h in halves]
    for i, t in enumerate((a, lp, v, x)):
        assert torch.equal(t, torch.cat([p[i] for p in parts])), i
    assert torch.equal(v, w["last_val"])
    assert len(set(w["act"].reshape(-1).tolist())) == 3
    for e in [whole] + halves:
        e.close()


BAD_FLAGS = (0x200, 0x102, 0x100 | 0xff, 0x300, 2, -1)


def test_bad_flag_bits_are_refused_and_launch_nothing(torch_cuda):
    """ssg_policy_act, ssg_rollout_policy and ssg_ppo_dist through their ctypes signatures, on pre-filled outputs."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    n, K, D = 100, 3, 22
    env = vec(n, D)
    _warm(env)
    _, pol = split_policy(torch, D, 48, 2, "tanh", 3)
    bufs = {"act": torch.full((K, n), 7, dtype=torch.int32, device=DEV), "logp": torch.full((K, n), 7.0, device=DEV),
            "val": torch.full((K, n), 7.0, device=DEV), "x": torch.full((K, n, D), 7.0, device=DEV),
            "rew": torch.full((K, n), 7.0, dtype=torch.float64, device=DEV), "done": torch.full((K, n), 7, dtype=torch.uint8, device=DEV),
            "flags": torch.full((K, n), 7, dtype=torch.uint8, device=DEV), "last": torch.full((n,), 7.0, device=DEV),
            "logp_all": torch.full((K, n, 4), 7.0, device=DEV)}
    torch.cuda.synchronize()
    state0, obs0, params0 = env.state.clone(), env.obs.clone(), pol.params.clone()
    L, P, stream = N.lib(), (lambda t: C.c_void_p(t.data_ptr())), env._stream()
    good = pol.to_native()
    assert good.activation == 0x100
    for flag in BAD_FLAGS:
        p = pol.to_native()
        p.activation = flag
        assert L.ssg_policy_act(env._h, C.byref(p), P(env.obs), None, 0, 0, P(bufs["act"]), P(bufs["logp"]), P(bufs["val"]), P(bufs["x"]),
                                stream) == -1, hex(flag)
        assert L.ssg_rollout_policy(env._h, C.byref(p), K, None, 0, 0, P(env.obs), P(bufs["act"]), P(bufs["logp"]), P(bufs["val"]),
                                    P(bufs["x"]), P(bufs["rew"]), P(bufs["done"]), P(bufs["flags"]), P(bufs["last"]), n, stream) == -1, hex(flag)
        assert L.ssg_ppo_dist(env._h, C.byref(p), K * n, P(bufs["x"]), P(bufs["logp_all"]), stream) == -1, hex(flag)
    torch.cuda.synchronize()
    assert torch.equal(env.state, state0) and torch.equal(env.obs, obs0) and torch.equal(pol.params, params0)
    for k, t in bufs.items():
        assert bool((t == 7).all()), k
    # the good record launches
    assert L.ssg_ppo_dist(env._h, C.byref(good), K * n, P(bufs["x"]), P(bufs["logp_all"]), stream) == 0
    torch.cuda.synchronize()
    assert not bool((bufs["logp_all"] == 7).any())
    env.close()
