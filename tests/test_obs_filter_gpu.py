"""GPU checks of the observation filter (ssg_obs_filter_update / ssg_set_obs_filter; ship_sim_gym_amd/obs_filter.py).  The references:
``merge_reference`` (the numpy restatement of the device's reduction order) for the statistics, a CPU torch restatement of the formula
for the normalised rows, hand loops of ``filter.update()`` / ``policy_act`` / ``step_tensor`` for the rollout loops, and — for a
population — the single-policy path on a handle of n_m envs with env_id_base + o_m.  Every comparison is bitwise except the device's
square root (2 ulp).

Shapes: n in {1, 2, 255, 256, 257, 769} (one row, below / at / above the 256-row tile, four tiles of which one a tail) and D in
{7, 28, 48} (history 1 with 1 beam; history 2 with 8 beams; history 3 with 10 beams: the frame-shift path, and two column chunks).
Everything above T = 4 tiles and D = 48 — runs of several tiles, empty runs, the second and third prefetch group, the column chunks
up to D = 176, populations at the member limit and on slices with surplus workgroups, counts past 2^31, the filtered policy kernels at
the extreme widths — is in tests/test_obs_filter_domain_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, env_config, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, assert_same_rollout, split_policy, stepwise_rollout

pytestmark = pytest.mark.gpu

HIST_BEAMS = {7: (1, 1), 28: (2, 8), 48: (3, 10)}
SIZES = (1, 2, 255, 256, 257, 769)
KEYS = ("obs", "act", "logp", "val", "rew", "done", "flags", "last_val")


def _vec(n, D, base=0, max_steps=None):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    history, beams = HIST_BEAMS[D]
    cfg = env_config(history)
    if max_steps is not None:
        cfg.MAX_STEPS = max_steps
    env = ShipVecEnv(n, n_maps=64, n_beams=beams, env_config=cfg, env_id_base=base)
    assert env.states_history == D
    return env


def _steps(env, k, seed=5):
    for a in env.random_actions(seed, 0, k):
        env.step_tensor(a)


def _filter(env, **kw):
    from ship_sim_gym_amd.obs_filter import ObsFilter
    return ObsFilter(env, **kw)


def _check_state(flt, prev_rows, batch, member=0):
    """The member's state rows against merge_reference(prev_rows, batch): count, mean and M2 bit for bit, denom within 2 ulp of
    sqrt(M2 / (count - 1)) + eps formed from the device's own M2 (1 below two rows).  Returns the device's rows (numpy)."""
    from ship_sim_gym_amd.obs_filter import merge_reference
    got = flt.state[member].cpu().numpy()
    want = merge_reference(prev_rows, batch.cpu().numpy(), eps=flt.eps)
    assert got[3, 0] == want[3, 0] and not got[3, 1:].any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    cnt = got[3, 0]
    den = np.sqrt(got[1] / (cnt - 1.0)) + flt.eps if cnt >= 2 else np.ones_like(got[1])
    assert np.all(np.abs(got[2] - den) <= 2 * np.spacing(den)), np.abs(got[2] - den).max()
    return got


@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
def test_update_is_the_restatement_bit_for_bit(torch_cuda, D):
    torch = torch_cuda
    for n in SIZES:
        env = _vec(n, D)
        env.reset_tensor()
        flt = _filter(env)
        zero = np.zeros((4, D))
        flt.update()                                                   # the env's own observations after a reset
        rows = _check_state(flt, zero, env.obs)
        if n == 1:
            assert np.array_equal(rows[2], np.ones(D))                 # one row: denom == 1
        _steps(env, 3)
        before = flt.state.clone()
        flt.update()                                                   # ... and after a few random steps
        rows2 = _check_state(flt, rows, env.obs)
        assert rows2[3, 0] == 2 * n
        # the same update on a cloned state: identical bits
        twin = _filter(env)
        twin.state.copy_(before)
        twin.update()
        assert torch.equal(twin.state, flt.state)
        # a caller-made tensor, five successive merges
        g = torch.Generator(device=DEV).manual_seed(n * 100 + D)
        mine = _filter(env, eps=1e-3)
        prev = zero
        for t in range(5):
            batch = (torch.rand((n, D), generator=g, device=DEV, dtype=torch.float64) - 0.3) * (10.0 ** (t - 1))
            batch[:, D - 1] = -1.0
            mine.update(batch)
            prev = _check_state(mine, prev, batch)
        assert prev[3, 0] == 5 * n and prev[0, D - 1] == -1.0 and prev[1, D - 1] == 0.0
        env.close()


def _norm_cpu(torch, flt, obs, member=0):
    st = flt.state[member].cpu()
    den = torch.where(st[2] == 0.0, torch.ones_like(st[2]), st[2])
    v = (obs.cpu() - st[0]) / den
    if flt.clip > 0.0:
        v = v.clamp(-flt.clip, flt.clip)
    return v.float()


def _policies(torch, D):
    return {"shared": actor_critic_policy(torch, D, seed=D)[1], "split": split_policy(torch, D, H=48, seed=D + 1)[1]}


@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
def test_policy_act_normalises_with_the_published_state(torch_cuda, D):
    torch = torch_cuda
    n = 257
    env = _vec(n, D)
    env.reset_tensor()
    flt = _filter(env)
    flt.update()
    _steps(env, 4)
    flt.update()
    for name, pol in _policies(torch, D).items():
        env.set_obs_filter(None)
        plain = {g: env.policy_act(pol, seed=3, step=5, greedy=g) for g in (False, True)}
        env.set_obs_filter(flt)
        assert env.obs_filter is flt
        want = _norm_cpu(torch, flt, env.obs)
        assert torch.equal(want, flt.normalise(env.obs).cpu())
        for greedy in (False, True):
            a, lp, v, x = env.policy_act(pol, seed=3, step=5, greedy=greedy)
            assert torch.equal(x.cpu(), want), (name, greedy)
            assert torch.isfinite(lp).all() and torch.isfinite(v).all() and int(a.min()) >= 0 and int(a.max()) < pol.n_actions
            assert not torch.equal(x, plain[greedy][3])
        # policy_act never updates
        assert flt.count.item() == 2 * n
        # mean = 0, denom = obs_scale, clip = 0 written into the state: every output is the unbound call's
        ident = _filter(env, clip=0.0)
        ident.state[0, 2] = pol.obs_scale
        env.set_obs_filter(ident)
        for greedy in (False, True):
            got = env.policy_act(pol, seed=3, step=5, greedy=greedy)
            for t, (p, q) in enumerate(zip(got, plain[greedy])):
                assert p.dtype == q.dtype and torch.equal(p, q), (name, greedy, t)
        # after unbinding: what it was before binding
        env.set_obs_filter(None)
        assert env.obs_filter is None
        for greedy in (False, True):
            assert all(torch.equal(p, q) for p, q in zip(env.policy_act(pol, seed=3, step=5, greedy=greedy), plain[greedy]))
    env.close()


def test_clipping(torch_cuda):
    torch = torch_cuda
    D, n = 28, 70
    env = _vec(n, D)
    env.reset_tensor()
    pol = actor_critic_policy(torch, D, seed=1)[1]
    flt = _filter(env, clip=10.0)
    flt.update()                                       # reset rows: every column constant but the map-dependent ones
    const = (flt.M2[0] == 0.0).cpu()
    assert int(const.sum()) >= D // 2                  # (the history half is -1 everywhere)
    env.set_obs_filter(flt)
    x = env.policy_act(pol)[3].cpu()
    assert not x[:, const].any()                       # a constant column gives x == 0
    obs0 = env.obs.clone()
    env.obs[:, 0], env.obs[:, 1] = 1e9, -1e9
    x = env.policy_act(pol)[3].cpu()
    assert (x[:, 0] == 10.0).all() and (x[:, 1] == -10.0).all() and torch.equal(x[:, 2:], _norm_cpu(torch, flt, obs0)[:, 2:])
    wide = _filter(env, clip=0.0)
    wide.state.copy_(flt.state)
    env.set_obs_filter(wide)
    x = env.policy_act(pol)[3].cpu()
    assert torch.equal(x, _norm_cpu(torch, wide, env.obs)) and (x[:, 0] > 1e6).all() and (x[:, 1] < -1e6).all()
    env.close()


def _hand_rollout(env, flt, pol, K, seed, step0, update):
    """ssg_rollout_policy with a filter bound, restated: K x {filter.update(), policy_act, step_tensor}, then the bootstrap value."""
    import torch
    rows = {k: [] for k in KEYS[:-1]}
    for k in range(K):
        if update:
            flt.update()
        a, lp, v, x = env.policy_act(pol, seed=seed, step=step0 + k)
        rows["obs"].append(x); rows["act"].append(a); rows["logp"].append(lp); rows["val"].append(v)
        _, r, d, f = env.step_tensor(a)
        rows["rew"].append(r.clone()); rows["done"].append(d.clone()); rows["flags"].append(f.clone())
    out = {k: torch.stack(v) for k, v in rows.items()}
    out["last_val"] = env.policy_act(pol, seed=seed, step=step0 + K)[2]
    return out


@pytest.mark.parametrize("n,D", [(257, 28), (769, 48), (2, 7)])
def test_rollout_updates_then_normalises(torch_cuda, n, D):
    torch = torch_cuda
    K = 4
    pol = _policies(torch, D)["split" if D == 48 else "shared"]
    a, b = _vec(n, D), _vec(n, D)
    fa, fb = _filter(a), _filter(b)
    a.set_obs_filter(fa); b.set_obs_filter(fb)
    a.reset_tensor(); b.reset_tensor()
    ra = a.rollout_policy(pol, K, seed=9, step0=2)
    rb = _hand_rollout(b, fb, pol, K, 9, 2, update=True)
    assert_same_rollout(torch, ra, rb, "updating")
    assert torch.equal(fa.state, fb.state) and torch.equal(a.obs, b.obs)
    assert fa.count.item() == K * n                    # the bootstrap forward merged nothing
    assert torch.equal(ra["obs"][K - 1].cpu(), ra["obs"][K - 1].cpu().clamp(-10.0, 10.0))
    # last_val: a frozen policy_act on the final observations
    assert torch.equal(ra["last_val"], a.policy_act(pol, seed=0, step=0)[2]) and fa.count.item() == K * n
    # frozen: the state does not move, and the buffers are the hand loop's without updates
    keep = fa.state.clone()
    a.set_obs_filter(fa.frozen()); b.set_obs_filter(fb.frozen())
    ra = a.rollout_policy(pol, K, seed=9, step0=2 + K)
    rb = stepwise_rollout(b, pol, K, 9, 2 + K)
    assert_same_rollout(torch, ra, rb, "frozen")
    assert torch.equal(fa.state, keep) and torch.equal(fb.state, keep)
    # train(False) on the bound filter re-binds it frozen
    a.set_obs_filter(fa)
    fa.train(False)
    a.rollout_policy(pol, 1, seed=1)
    assert torch.equal(fa.state, keep)
    fa.train(True)
    a.rollout_policy(pol, 1, seed=1)
    assert fa.count.item() == (K + 1) * n
    a.close(); b.close()


@pytest.mark.parametrize("sizes", [None, (64, 320, 192)])
def test_population_members_are_single_policy_filters(torch_cuda, sizes):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    P, N, D, K = 3, 576, 28, 3
    env = _vec(N, D)
    if sizes is not None:
        env.set_population_slices(sizes)
    sz = list(sizes) if sizes is not None else [N // P] * P
    offs = [sum(sz[:m]) for m in range(P)]
    members = [actor_critic_policy(torch, D, seed=40 + m)[1] for m in range(P)]
    pop = NativePopulation([actor_critic_policy(torch, D, seed=40 + m)[1] for m in range(P)])
    flt = _filter(env, n_members=P)
    env.set_obs_filter(flt)
    env.reset_tensor()
    rb = env.rollout_population(pop, K, seed=7)
    assert flt.count.tolist() == [float(K * s) for s in sz]
    for m, (o, n) in enumerate(zip(offs, sz)):
        sh = _vec(n, D, base=o)
        fs = _filter(sh)
        sh.set_obs_filter(fs)
        sh.reset_tensor()
        rs = sh.rollout_policy(members[m], K, seed=7)
        for k in KEYS[:-1]:
            assert rb[k].dtype == rs[k].dtype and torch.equal(rb[k][:, o:o + n], rs[k]), (m, k)
        assert torch.equal(rb["last_val"][o:o + n], rs["last_val"]) and torch.equal(env.obs[o:o + n], sh.obs), m
        assert torch.equal(flt.state[m], fs.state[0]), m
        # population_act and the greedy launch read the member's own rows
        for greedy in (False, True):
            pa = env.population_act(pop, seed=3, step=1, greedy=greedy)
            sa = sh.policy_act(members[m], seed=3, step=1, greedy=greedy)
            assert all(torch.equal(p[o:o + n], q) for p, q in zip(pa, sa)), (m, greedy)
        sh.close()
    # a single-policy call against the population's filter, and a population against a single filter: refused
    from ship_sim_gym_amd._native import ShipSimError
    with pytest.raises(ShipSimError):
        env.policy_act(members[0])
    one = _vec(N, D)
    one.set_obs_filter(_filter(one))
    one.reset_tensor()
    with pytest.raises(ShipSimError):
        one.rollout_population(pop, 1)
    with pytest.raises(ShipSimError):
        one.population_act(pop)
    keep = pop.params.clone()                                          # ... and exploit refuses before it copies anything
    with pytest.raises(ValueError):
        PopulationPPO(pop, one).exploit([1, 1, 2])
    assert torch.equal(pop.params, keep)
    one.close()
    # exploit: the source's filter rows travel with its weights
    ppo = PopulationPPO(pop, env)
    before = flt.state.clone()
    ppo.exploit([1, 1, 2])
    assert torch.equal(flt.state[0], before[1]) and torch.equal(flt.state[1], before[1]) and torch.equal(flt.state[2], before[2])
    assert not torch.equal(before[0], before[1])
    env.close()


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("sizes", [None, (1, 63, 128)], ids=["equal", "sliced"])
def test_separate_value_population_members_are_single_policy_filters(torch_cuda, sizes, layers):
    """The FILTER kernels of a population whose members have a separate value network — on equal slices and on a slices table, sampled,
    greedy and the value-only bootstrap forward — against the single-policy path with a filter of its own on each member's shard
    (test_policy_act_normalises_with_the_published_state checks that path for a separate value network).  The smallest shapes that
    still tell the kernels, grids and LDS sizes apart: D = 8, hidden 16, one and two layers (two: the third activation buffer), and
    slices of one env, a partial wave and two workgroups."""
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    P, N, D, H, K = 3, 192, 8, 16, 3

    def vec(n, base=0):
        env = ShipVecEnv(n, n_maps=64, n_beams=2, env_config=env_config(1), env_id_base=base)
        assert env.states_history == D
        return env

    def members():
        return [split_policy(torch, D, H, layers, seed=60 + m)[1] for m in range(P)]

    env = vec(N)
    if sizes is not None:
        env.set_population_slices(sizes)
    sz = list(sizes) if sizes is not None else [N // P] * P
    offs = [sum(sz[:m]) for m in range(P)]
    refs, pop = members(), NativePopulation(members())
    flt = _filter(env, n_members=P)
    env.set_obs_filter(flt)
    env.reset_tensor()
    rb = env.rollout_population(pop, K, seed=7)
    assert flt.count.tolist() == [float(K * s) for s in sz]
    acts = {greedy: env.population_act(pop, seed=3, step=1, greedy=greedy) for greedy in (False, True)}
    assert not torch.equal(acts[False][0], acts[True][0])
    for m, (o, n) in enumerate(zip(offs, sz)):
        sh = vec(n, base=o)
        fs = _filter(sh)
        sh.set_obs_filter(fs)
        sh.reset_tensor()
        rs = sh.rollout_policy(refs[m], K, seed=7)
        for k in KEYS:
            got = rb[k][o:o + n] if k == "last_val" else rb[k][:, o:o + n]
            assert got.dtype == rs[k].dtype and torch.equal(got, rs[k]), (m, k)
        assert torch.equal(env.obs[o:o + n], sh.obs) and torch.equal(flt.state[m], fs.state[0]), m
        for greedy, pa in acts.items():
            sa = sh.policy_act(refs[m], seed=3, step=1, greedy=greedy)
            assert all(p.dtype == q.dtype and torch.equal(p[o:o + n], q) for p, q in zip(pa, sa)), (m, greedy)
        sh.close()
    env.close()


def test_evaluation_is_frozen(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator, eval_walk
    n, D, T, E = 256, 28, 48, 2
    a, b = _vec(n, D, max_steps=20), _vec(n, D, max_steps=20)
    pol = actor_critic_policy(torch, D, seed=8)[1]
    train = _filter(a)
    a.reset_tensor()
    g = torch.Generator(device=DEV).manual_seed(1)
    for scale in (1.0, 300.0):                         # some statistics (the envs themselves stay fresh)
        train.update(a.obs + scale * torch.rand((n, D), generator=g, device=DEV, dtype=torch.float64))
    keep = train.state.clone()
    a.set_obs_filter(train.frozen())
    fb = _filter(b, update=False)
    fb.state.copy_(keep)
    b.set_obs_filter(fb)
    ev = NativeEvaluator(a)
    r = ev.evaluate(pol, E, greedy=False, max_steps=T, seed=11, chunk=T)
    assert torch.equal(train.state, keep) and r["steps"] == T
    b.reset_tensor()
    rb = b.rollout_policy(pol, T, seed=11, step0=0)
    want, _ = eval_walk(rb["rew"].cpu().numpy(), rb["done"].cpu().numpy(), rb["flags"].cpu().numpy(), E)
    assert np.array_equal(r["per_env"].cpu().numpy(), want) and int(want[:, 0].min()) >= 1
    assert torch.equal(fb.state, keep)
    # an updating filter bound to the evaluated env is not updated either
    a.set_obs_filter(train)
    ev.evaluate(pol, 1, greedy=True, max_steps=8, chunk=8)
    assert torch.equal(train.state, keep)
    a.close(); b.close()


def test_refusals_on_a_live_handle(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    env = _vec(300, 28)
    env.reset_tensor()
    pol = actor_critic_policy(torch, 28, seed=2)[1]
    plain = env.policy_act(pol, seed=4, step=1)
    flt = _filter(env, clip=5.0)
    flt.update()
    env.set_obs_filter(flt)
    bound = env.policy_act(pol, seed=4, step=1)
    L, h = N.lib(), env._h
    bad = [dict(struct_size=8), dict(obs_dim=27), dict(n_members=0), dict(n_members=257), dict(dev_state=None), dict(dev_workspace=None),
           dict(workspace_nbytes=flt.workspace.numel() - 1), dict(flags=2), dict(clip=-1.0), dict(eps=-1.0), dict(clip=float("nan")),
           dict(eps=float("nan"))]
    for kw in bad:
        rec = flt.to_native()
        for k, v in kw.items():
            setattr(rec, k, v)
        assert L.ssg_set_obs_filter(h, C.byref(rec)) == -1, kw
        assert L.ssg_obs_filter_update(h, C.byref(rec), C.c_void_p(env.obs.data_ptr()), env._stream()) == -1, kw
        got = N.ObsFilterRecord()
        assert L.ssg_get_obs_filter(h, C.byref(got)) == 0 and (got.clip, got.dev_state, got.n_members) == (5.0, flt.state.data_ptr(), 1), kw
    assert L.ssg_obs_filter_update(h, C.byref(flt.to_native()), None, env._stream()) == -1
    two = flt.to_native()
    two.n_members, two.workspace_nbytes = 7, 1 << 30    # 300 envs do not split into 7 members
    assert L.ssg_obs_filter_update(h, C.byref(two), C.c_void_p(env.obs.data_ptr()), env._stream()) == -1
    torch.cuda.synchronize()
    assert flt.count.item() == 300                      # nothing was launched by a refused call
    with pytest.raises(ValueError):
        flt.update(env.obs.float())
    # the binding survived every refusal ...
    assert all(torch.equal(p, q) for p, q in zip(env.policy_act(pol, seed=4, step=1), bound))
    # ... and after unbinding policy_act is what it was before binding
    env.set_obs_filter(None)
    assert all(torch.equal(p, q) for p, q in zip(env.policy_act(pol, seed=4, step=1), plain))
    env.close()


def _run(args, timeout):
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_ppo_script_runs_with_the_filter(torch_cuda, tmp_path):
    import re
    torch = torch_cuda
    f = str(tmp_path / "filter.pt")
    out = _run([os.path.join(ROOT, "train", "ppo_torch.py"), "--mode", "native", "--update", "native", "--obs-filter", "--envs", "256",
                "--updates", "2", "--horizon", "8", "--save-obs-filter", f], 300)
    assert out.returncode == 0, out.stderr[-2000:]
    losses = re.findall(r"policy loss (\S+)\s+value loss (\S+)\s+entropy (\S+)\s+\(obs filter: (\d+) rows", out.stdout)
    assert len(losses) == 2 and all(np.isfinite(float(v)) for row in losses for v in row[:3]), out.stdout
    assert [int(row[3]) for row in losses] == [256 * 8, 2 * 256 * 8]
    sd = torch.load(f, map_location="cpu")
    assert sd["state"].shape == (1, 4, sd["obs_dim"]) and sd["state"][0, 3, 0] == 2 * 256 * 8 and torch.isfinite(sd["state"]).all()


def test_evaluate_script_reads_a_saved_filter(torch_cuda, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    env = ShipVecEnv(64)                                # the scripts' env: the default 10 beams, history 2
    env.reset_tensor()
    flt = _filter(env)
    flt.update()
    _steps(env, 5)
    flt.update()
    f = str(tmp_path / "filter.pt")
    torch.save(flt.state_dict(), f)
    env.close()
    out = _run([os.path.join(ROOT, "train", "evaluate_native.py"), "--envs", "256", "--episodes", "1", "--obs-filter", f], 300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert lines[0].split()[:2] == ["policy", "episodes"] and len(lines) == 2 and int(lines[1].split()[1]) == 256, out.stdout


def test_pbt_script_runs_with_the_filter(torch_cuda):
    out = _run([os.path.join(ROOT, "train", "pbt_native.py"), "--members", "3", "--envs-per-member", "64", "--updates", "2", "--horizon", "8",
                "--perturb-every", "1", "--obs-filter", "--eval-every", "2"], 300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "update 2  episode_reward_mean" in out.stdout and "greedy evaluation" in out.stdout, out.stdout
    assert "observation filter: rows merged per member" in out.stdout, out.stdout
