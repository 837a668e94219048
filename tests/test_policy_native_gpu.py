"""GPU checks of the policy in the loop (ABI 9: ssg_policy_act / ssg_rollout_policy, ship_sim_gym_amd/policy.py): the device's forward
against torch on the env's real observations, its Philox uniforms, the fused rollout against its own step-by-step loop, shard
invariance, the env stepping exactly as it does under rollout_tensor, the other handle kinds, argument errors, and ppo_torch's
`native` mode against its eager mode."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import check_near_rows as _check_near, env_config as _env_config, load_script, same_columns as _same_columns
from gpu_support import torch_sample as _torch_sample
from gpu_support import torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _policy, assert_same_rollout as _assert_same, stepwise_rollout as _stepwise

pytestmark = pytest.mark.gpu


def _vec(n, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    kw.setdefault("n_maps", 64)
    return ShipVecEnv(n, **kw)


def test_forward_matches_torch_on_real_observations(torch_cuda):
    torch = torch_cuda
    n = 1000  # not a multiple of 64: the tail workgroup's lanes store nothing
    for nb in (8, 10):
        for hist in (1, 2, 3):
            env = _vec(n, n_beams=nb, env_config=_env_config(hist))
            env.reset_tensor()
            acts = env.random_actions(5, 0, 20)
            for k in range(20):                       # real observations, reset rows (with their -1 entries) included
                env.step_tensor(acts[k])
            obs = env.obs.clone()
            D = env.states_history
            assert bool((obs == -1).any())
            u = torch.rand(n, generator=torch.Generator(device=env.device).manual_seed(nb * 10 + hist), device=env.device)
            for H in (32, 64, 128):
                for layers in (1, 2):
                    for act in ("tanh", "relu"):
                        net, pol = _policy(torch, D, H, layers, act, seed=H + layers)
                        a, logp, val, x = env.policy_act(pol, uniforms=u)
                        xr, logits, vr = pol.forward_reference(obs)
                        tag = (nb, hist, H, layers, act)
                        assert torch.equal(x, (obs / pol.obs_scale).float()) and torch.equal(xr, x), tag
                        ar, lpr, cdf = _torch_sample(torch, logits, u)
                        near = (u.unsqueeze(-1) - cdf[:, :-1]).abs().min(dim=-1).values < 1e-5
                        assert int(near.sum()) <= n // 1000, tag
                        ok = ~near
                        assert torch.equal(a.long()[ok], ar[ok]), tag
                        assert float((logp - lpr)[ok].abs().max()) <= 1e-4, tag
                        _check_near(torch, near, u, cdf, a, logp, torch.log_softmax(logits.double(), -1), 1e-4)   # f64: the action's own
                        assert bool(((val - vr).abs() <= 1e-5 * (1 + vr.abs())).all()), (tag, float((val - vr).abs().max()))
                        assert torch.equal(env.obs, obs)  # the forward reads the observation, never writes it
            env.close()


def _philox_u(seed, step, env_ids, word0=None):
    """Philox4x32-10, counter (env_lo, env_hi, step_lo, step_hi), key = seed; u = (word 1 >> 8) * 2^-24 (include/shipsim.h).
    word0: a list that receives output word 0 (what ssg_fill_actions turns into its actions)."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    mask = 0xFFFFFFFF
    out = np.empty(len(env_ids), dtype=np.float32)
    for i, e in enumerate(env_ids):
        c = [e & mask, e >> 32, step & mask, step >> 32]
        k = [seed & mask, seed >> 32]
        for r in range(10):
            if r:
                k = [(k[0] + W0) & mask, (k[1] + W1) & mask]
            p0, p1 = M0 * c[0], M1 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & mask, (p0 >> 32) ^ c[3] ^ k[1], p0 & mask]
        out[i] = np.float32(c[1] >> 8) * np.float32(2.0 ** -24)
        if word0 is not None:
            word0.append(c[0])
    return out


def test_philox_uniforms_are_the_documented_stream(torch_cuda):
    """uniforms=None draws u from Philox keyed by (seed, step, GLOBAL env id).  u is seen through the actions it selects: a policy with
    zero weights has the same CDF for every env (its bias), and over many random CDFs the in-kernel draw and the numpy restatement
    passed in as `uniforms` must choose identical actions everywhere (a different u would cross some boundary)."""
    torch = torch_cuda
    n = 1000
    for base in (0, 123457):
        env = _vec(n, env_id_base=base)
        env.reset_tensor()
        D = env.states_history
        net, pol = _policy(torch, D, 16, 1, A=4)
        g = torch.Generator().manual_seed(base)
        seen = set()
        for trial in range(24):
            seed, step = (2 ** 40 + 17 * trial) if trial % 2 else trial, trial * 1000003 + (2 ** 33 if trial % 3 == 0 else 0)
            with torch.no_grad():
                for p in net.parameters():
                    p.zero_()
                net.pi.bias.copy_(torch.randn(4, generator=g) * 2)
            pol.refresh()
            a0, lp0, v0, _ = env.policy_act(pol, seed=seed, step=step)
            w0 = []
            u = torch.from_numpy(_philox_u(seed, step, range(base, base + n), w0)).to(env.device)
            if trial < 4:  # the restatement is the library's stream: word 0 gives ssg_fill_actions' actions
                assert env.random_actions(seed, step, 1)[0].tolist() == [(w * 3) >> 32 for w in w0]
            a1, lp1, v1, _ = env.policy_act(pol, uniforms=u)
            assert torch.equal(a0, a1) and torch.equal(lp0, lp1) and torch.equal(v0, v1), (base, trial)
            seen |= set(a0.tolist())
        assert seen == {0, 1, 2, 3}
        env.close()


# config4: every step is the full cpSpaceStep's launch and the step kernel's, the dyn queue handed from step to step; ring4: a world per
# episode, three episode starts between two refills and episodes of 3 steps, so both 7-step rollouts refill inside the loop
FUSED_KINDS = {"bank": (1000, 64, {}),
               "config4": (256, 64, dict(n_ships=4, n_beams=8, n_maps=4, env_config=_env_config(2, 20))),
               "ring4": (256, 7, dict(map_mode="fresh_device", ring=4, n_beams=8, env_config=_env_config(2, 3)))}


@pytest.mark.parametrize("kind", list(FUSED_KINDS))
def test_fused_rollout_equals_stepwise_loop(torch_cuda, kind):
    torch = torch_cuda
    n, K, kw = FUSED_KINDS[kind]
    a, b = _vec(n, **kw), _vec(n, **kw)
    a.reset_tensor(); b.reset_tensor()

    def same_state():
        from ship_sim_gym_amd import _native as N
        bodies = (N.F_TRAFFIC, N.F_GOAL_BODIES) if kind == "config4" else ()
        return torch.equal(a.obs, b.obs) and _same_columns(torch, a, b) and all(torch.equal(a.field(f), b.field(f)) for f in bodies)
    net, pol = _policy(torch, a.states_history)
    fused = a.rollout_policy(pol, K, seed=11, step0=500)
    step = _stepwise(b, pol, K, 11, 500)
    _assert_same(torch, fused, step, "philox")
    assert same_state()
    assert int(fused["done"].sum()) > 0 or int(fused["flags"].sum()) > 0
    # caller uniforms and a preallocated `out` (first dimension longer than K)
    u = torch.rand((K, n), device=a.device)
    out = {k: torch.full((K + 2,) + tuple(v.shape[1:]), 3, dtype=v.dtype, device=a.device) if k != "last_val" else torch.empty_like(v)
           for k, v in fused.items()}
    fused2 = a.rollout_policy(pol, K, uniforms=u, out=out)
    step2 = _stepwise(b, pol, K, 0, 0, uniforms=u)
    _assert_same(torch, fused2, step2, "uniforms")
    assert fused2["obs"].data_ptr() == out["obs"].data_ptr() and int(out["act"][K:].eq(3).all()) == 1
    assert same_state()
    a.close(); b.close()


def test_shard_invariance(torch_cuda):
    torch = torch_cuda
    K = 32
    whole = _vec(2048)
    halves = [_vec(1024, env_id_base=0), _vec(1024, env_id_base=1024)]
    for e in [whole] + halves:
        e.reset_tensor()
    net, pol = _policy(torch, whole.states_history)
    w = whole.rollout_policy(pol, K, seed=3, step0=7)
    hs = [h.rollout_policy(pol, K, seed=3, step0=7) for h in halves]
    for k in w:
        cat = torch.cat([h[k] for h in hs], dim=0 if k == "last_val" else 1)
        assert torch.equal(w[k], cat), k
    # and the single forward: the same bits as inside the rollout
    a, lp, v, x = whole.policy_act(pol, seed=3, step=7 + K)
    parts = [h.policy_act(pol, seed=3, step=7 + K) for h in halves]
    for i, t in enumerate((a, lp, v, x)):
        assert torch.equal(t, torch.cat([p[i] for p in parts])), i
    assert torch.equal(v, w["last_val"])
    for e in [whole] + halves:
        e.close()


def test_native_rollout_steps_the_env_as_rollout_tensor_does(torch_cuda):
    torch = torch_cuda
    n, K = 2048, 48
    a, b = _vec(n), _vec(n)
    a.reset_tensor()
    obs0 = b.reset_tensor().clone()
    net, pol = _policy(torch, a.states_history)
    r = a.rollout_policy(pol, K, seed=21)
    to, tr, td, tf = b.rollout_tensor(r["act"].contiguous(), trajectory=True)
    assert torch.equal(tr, r["rew"]) and torch.equal(td, r["done"]) and torch.equal(tf, r["flags"])
    scale = pol.obs_scale
    prev = torch.cat([obs0.unsqueeze(0), to[:-1]])
    for k in range(K):
        assert torch.equal(r["obs"][k], (prev[k] / scale).float()), k
    assert torch.equal(a.obs, to[-1])
    assert int(r["done"].sum()) > 0
    a.close(); b.close()


@pytest.mark.parametrize("kind", ["n_ships4", "fresh_device", "history3"])
def test_other_handle_kinds_fused_equals_stepwise(torch_cuda, kind):
    torch = torch_cuda
    kw = {"n_ships4": dict(n_ships=4, n_maps=16), "fresh_device": dict(map_mode="fresh_device", ring=8),
          "history3": dict(env_config=_env_config(3))}[kind]
    n = 256 if kind == "n_ships4" else 1000
    K = 40
    a, b = _vec(n, **kw), _vec(n, **kw)
    a.reset_tensor(); b.reset_tensor()
    net, pol = _policy(torch, a.states_history, act="relu")
    fused = a.rollout_policy(pol, K, seed=5, step0=1)
    step = _stepwise(b, pol, K, 5, 1)
    _assert_same(torch, fused, step, kind)
    assert torch.equal(a.obs, b.obs) and _same_columns(torch, a, b)
    a.close(); b.close()


def test_bad_arguments_raise_and_launch_nothing(torch_cuda):
    from ship_sim_gym_amd import _native as N
    torch = torch_cuda
    n, K = 512, 4
    env = _vec(n)
    env.reset_tensor()
    acts = env.random_actions(1, 0, 3)
    for k in range(3):
        env.step_tensor(acts[k])
    D = env.states_history
    net, pol = _policy(torch, D)
    dev = env.device
    bufs = {"act": torch.zeros((K, n), dtype=torch.int32, device=dev), "logp": torch.zeros((K, n), device=dev),
            "val": torch.zeros((K, n), device=dev), "x": torch.zeros((K, n, D), device=dev),
            "rew": torch.zeros((K, n), dtype=torch.float64, device=dev), "done": torch.zeros((K, n), dtype=torch.uint8, device=dev),
            "flags": torch.zeros((K, n), dtype=torch.uint8, device=dev), "last": torch.zeros(n, device=dev)}
    torch.cuda.synchronize()
    state0, obs0 = env.state.clone(), env.obs.clone()
    L = N.lib()
    P = lambda t: C.c_void_p(t.data_ptr())
    stream = env._stream()

    def roll(p, K=K, stride=n, drop=None):
        a = dict(obs=P(env.obs), act=P(bufs["act"]), logp=P(bufs["logp"]), val=P(bufs["val"]), rew=P(bufs["rew"]), done=P(bufs["done"]))
        if drop:
            a[drop] = None
        return L.ssg_rollout_policy(env._h, C.byref(p), K, None, 0, 0, a["obs"], a["act"], a["logp"], a["val"], P(bufs["x"]), a["rew"],
                                    a["done"], P(bufs["flags"]), P(bufs["last"]), stride, stream)

    def act1(p, drop=None):
        a = dict(obs=P(env.obs), act=P(bufs["act"]), logp=P(bufs["logp"]), val=P(bufs["val"]))
        if drop:
            a[drop] = None
        return L.ssg_policy_act(env._h, C.byref(p), a["obs"], None, 0, 0, a["act"], a["logp"], a["val"], P(bufs["x"]), stream)

    def bad(**kw):
        p = pol.to_native()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    bad_records = [bad(struct_size=C.sizeof(N.Policy) - 8), bad(struct_size=0), bad(obs_dim=D + 1), bad(hidden=8), bad(hidden=0),
                   bad(hidden=130), bad(hidden=40), bad(hidden=144), bad(n_hidden_layers=0), bad(n_hidden_layers=3), bad(n_actions=1),
                   bad(n_actions=5), bad(activation=2), bad(activation=-1), bad(dev_params=None), bad(dev_obs_scale=None)]
    for p in bad_records:
        assert roll(p) == -1
        assert act1(p) == -1
    good = pol.to_native()
    for drop in ("obs", "act", "logp", "val", "rew", "done"):
        assert roll(good, drop=drop) == -1, drop
    for drop in ("obs", "act", "logp", "val"):
        assert act1(good, drop=drop) == -1, drop
    assert roll(good, K=0) == -1 and roll(good, K=-3) == -1
    assert roll(good, stride=n - 1) == -1 and roll(good, stride=0) == -1
    assert L.ssg_rollout_policy(env._h, None, K, None, 0, 0, P(env.obs), P(bufs["act"]), P(bufs["logp"]), P(bufs["val"]), None, P(bufs["rew"]),
                                P(bufs["done"]), None, None, n, stream) == -1
    # the Python layer refuses before the library is reached
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 0)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, K, uniforms=torch.rand((K, n + 1), device=dev))
    with pytest.raises(ValueError):
        env.policy_act(_policy(torch, D + 1)[1])
    torch.cuda.synchronize()
    assert torch.equal(env.state, state0) and torch.equal(env.obs, obs0)
    assert int(bufs["act"].abs().sum()) == 0 and int(bufs["done"].sum()) == 0 and float(bufs["last"].abs().sum()) == 0.0
    env.close()
    for kw in (dict(map_mode="fresh"), dict(rllib=True), dict(auto_reset=False)):
        e = _vec(64, **kw)
        e.reset_tensor()
        torch.cuda.synchronize()
        s0 = e.state.clone()
        with pytest.raises(ValueError):
            e.rollout_policy(pol, 2)
        with pytest.raises(ValueError):
            e.policy_act(pol)
        torch.cuda.synchronize()
        assert torch.equal(e.state, s0), kw
        e.close()


def test_ppo_native_mode_trains_and_matches_eager_rollouts(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/ppo_torch.py")
    n, H = 4096, 32
    hist, got = mod.train(envs=n, updates=3, horizon=H, log=lambda s: None, mode="native", return_details=True)
    assert len(hist) == 3 and all(np.isfinite(h[1]) and np.isfinite(h[3]) for h in hist)
    assert got["rollout_us_per_step"] > 0 and all(int(s["done"].sum()) > 0 for s in got["snapshots"][:1])
    assert sum(int(s["done"].sum()) for s in got["snapshots"]) > 0
    _, ref = mod.train(envs=n, updates=1, horizon=H, log=lambda s: None, mode="eager", return_details=True)
    a, b = got["snapshots"][0], ref["snapshots"][0]
    assert set(a) == set(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape for k in a)
    same = torch.ones(n, dtype=torch.bool, device=a["act"].device)
    for k in ("act", "rew", "done"):
        same &= (a[k] == b[k]).all(dim=0)
    same &= (a["obs"] == b["obs"]).all(dim=2).all(dim=0)
    assert int(same.sum()) >= int(0.999 * n), int(same.sum())
    assert float((a["logp"] - b["logp"])[:, same].abs().max()) <= 1e-4
    va, vb = a["val"][:, same], b["val"][:, same]
    assert bool(((va - vb).abs() <= 1e-5 * (1 + vb.abs())).all()), float((va - vb).abs().max())
