"""Evaluation on the device (ssg_policy_act_greedy / ssg_pop_act_greedy, ssg_evaluate / ssg_pop_evaluate / ssg_eval_reduce,
ship_sim_gym_amd/evaluate.py): the greedy action against the policy's own log-distribution, ties, populations; the evaluation loop
against its own step-by-step restatement (rollout_policy / policy_act + step_tensor, walked by eval_walk); the quota and the carry;
populations against their members alone; other handle kinds; the script.  Everything is integers or bitwise: no tolerances."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, env_config as _env_config, same_columns as _same_columns, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy as _shared_policy, split_policy as _split_policy

pytestmark = pytest.mark.gpu


def _vec(n, history=2, max_steps=1000, **kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    kw.setdefault("n_maps", 64)
    return ShipVecEnv(n, env_config=_env_config(history, max_steps), **kw)


def _policy(torch, D, H=64, layers=2, act="tanh", A=3, seed=0, split=False):
    return (_split_policy if split else _shared_policy)(torch, D, H, layers, act, A, seed)[1]


def _constant_policy(torch, D, bias, H=16):
    """Zero weights: the logits are `bias` for every observation (equal entries = uniform over the actions)."""
    from ship_sim_gym_amd.policy import NativePolicy
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    b = torch.tensor(bias, dtype=torch.float32, device=DEV)
    return NativePolicy([(z(H, D), z(H))], (z(len(bias), H), b), (z(1, H), z(1)), 600.0)


def _walk(r, E, carry=None):
    from ship_sim_gym_amd.evaluate import eval_walk
    return eval_walk(r["rew"].cpu().numpy(), r["done"].cpu().numpy(), r["flags"].cpu().numpy(), E, carry)


def _rows(ev):
    return ev.env_stats.cpu().numpy().copy()


def _carry(ev):
    return ev.carry_return.cpu().numpy().copy(), ev.carry.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------------------------------
# greedy acting
# ------------------------------------------------------------------------------------------------------------------------------------
N_ACT = 200  # three full waves and a tail of 8


@pytest.fixture(scope="module")
def stepped_envs(torch_cuda):
    """Per history: 200 envs with 8 beams after 20 random steps, so that reset rows (their -1 history entries) are in."""
    envs = {}
    for history in (1, 2):
        env = _vec(N_ACT, history=history, n_beams=8)
        env.reset_tensor()
        acts = env.random_actions(11, 0, 20)
        for k in range(20):
            env.step_tensor(acts[k])
        envs[history] = env
    assert bool((envs[2].obs == -1).any())
    yield envs
    for env in envs.values():
        env.close()


@pytest.mark.parametrize("history,H,layers,act,split", list(itertools.product((1, 2), (32, 64), (1, 2), ("tanh", "relu"), (False, True))))
def test_greedy_act_is_the_first_maximum_of_the_policys_own_distribution(torch_cuda, stepped_envs, history, H, layers, act, split):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env = stepped_envs[history]
    pol = _policy(torch, env.states_history, H, layers, act, seed=3 + H + layers, split=split)
    a_s, lp_s, v_s, x_s = env.policy_act(pol, seed=1, step=2)
    a, lp, v, x = env.policy_act(pol, greedy=True)
    assert a.dtype == torch.int32 and torch.equal(v, v_s) and torch.equal(x, x_s)      # value and x: the sampling launch's, bit for bit
    logp_all = NativePPO(pol, env).dist({"obs": x})                                     # [n, 4], columns >= A zero
    A = pol.n_actions
    best = logp_all[:, :A].max(dim=1).values
    idx = a.long().unsqueeze(1)
    assert int(a.min()) >= 0 and int(a.max()) < A
    assert torch.equal(logp_all.gather(1, idx).squeeze(1), best)                        # the action attains the row's maximum ...
    first = (logp_all[:, :A] == best.unsqueeze(1)).float().argmax(dim=1)
    assert torch.equal(a.long(), first)                                                 # ... and is the first that does
    assert torch.equal(lp, logp_all.gather(1, idx).squeeze(1))                          # logp bitwise
    _, logits, _ = pol.forward_reference(env.obs)
    top = logits.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5
    assert int(clear.sum()) > N_ACT // 2
    assert torch.equal(a.long()[clear], logits.argmax(dim=1)[clear])                    # against plain torch where the maximum is clear
    a2, lp2, v2, x2 = env.policy_act(pol, seed=99, step=7, greedy=True)                 # no seed, no step
    assert torch.equal(a, a2) and torch.equal(lp, lp2) and torch.equal(v, v2) and torch.equal(x, x2)
    with pytest.raises(ValueError):
        env.policy_act(pol, greedy=True, uniforms=torch.rand(N_ACT, device=DEV))


@pytest.mark.parametrize("bias,want", [((0.0, 1.0, 1.0), 1), ((2.0, 2.0, 2.0), 0), ((0.0, 0.0, 3.0, 3.0), 2), ((1.0, 1.0), 0)])
def test_greedy_ties_go_to_the_smallest_index(torch_cuda, stepped_envs, bias, want):
    torch = torch_cuda
    env = stepped_envs[1]
    pol = _constant_policy(torch, env.states_history, bias)
    from ship_sim_gym_amd.ppo import NativePPO
    a, lp, _, x = env.policy_act(pol, greedy=True)
    assert torch.equal(a, torch.full((N_ACT,), want, dtype=torch.int32, device=DEV))
    assert torch.equal(lp, NativePPO(pol, env).dist({"obs": x})[:, want])


@pytest.mark.parametrize("split", [False, True])
def test_population_greedy_is_each_members_own_greedy_call(torch_cuda, stepped_envs, split):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation
    env = stepped_envs[2]
    P, n = 4, N_ACT // 4                                                                # 50 per member: a tail workgroup each
    pop = NativePopulation([_policy(torch, env.states_history, 64, 2, "tanh", seed=20 + m, split=split) for m in range(P)])
    a, lp, v, x = env.population_act(pop, greedy=True)
    a_s, _, v_s, x_s = env.population_act(pop, seed=4, step=5)
    assert torch.equal(v, v_s) and torch.equal(x, x_s) and not torch.equal(a, a_s)
    one = _vec(n, history=2, n_beams=8)
    for m in range(P):
        sl = slice(m * n, (m + 1) * n)
        one.obs.copy_(env.obs[sl])
        am, lpm, vm, xm = one.policy_act(pop.member(m), greedy=True)
        assert torch.equal(a[sl], am) and torch.equal(lp[sl], lpm) and torch.equal(v[sl], vm) and torch.equal(x[sl], xm), m
    one.close()
    assert len({tuple(a[m * n:(m + 1) * n].tolist()) for m in range(P)}) > 1          # (the members do differ)
    with pytest.raises(ValueError):
        env.population_act(pop, greedy=True, uniforms=torch.rand(N_ACT, device=DEV))


# ------------------------------------------------------------------------------------------------------------------------------------
# the evaluation loop against its own step-by-step restatement
# ------------------------------------------------------------------------------------------------------------------------------------
N_EV, MAX_STEPS, E, T = 256, 40, 2, 100


@pytest.fixture(scope="module")
def sampled_run(torch_cuda):
    """(a): a uniform policy over 3 actions, explicit uniforms [T, N]; the evaluation on one env, rollout_policy on its twin."""
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    a, b = _vec(N_EV, max_steps=MAX_STEPS), _vec(N_EV, max_steps=MAX_STEPS)
    pol = _constant_policy(torch, a.states_history, (0.5, 0.5, 0.5))
    u = torch.rand((T, N_EV), generator=torch.Generator().manual_seed(7)).to(DEV)
    ev = NativeEvaluator(a)
    a.reset_tensor(); b.reset_tensor()
    ev.run(pol, E, T, greedy=False, uniforms=u)
    r = b.rollout_policy(pol, T, uniforms=u)
    out = {"pol": pol, "u": u, "rows": _rows(ev), "carry": _carry(ev), "rollout": r, "same_state": torch.equal(a.obs, b.obs) and _same_columns(torch, a, b)}
    a.close(); b.close()
    return out


def test_sampled_evaluation_equals_the_walk_over_rollout_policy(torch_cuda, sampled_run, native):
    s = sampled_run
    want, (ret, ci) = _walk(s["rollout"], E)
    print("episodes %d  collided %d  out of bounds %d  timed out %d  no goals left %d  goal events %d" % tuple(s["rows"][:, c].sum() for c in (0, 3, 4, 5, 6, 7)))
    assert np.array_equal(s["rows"], want)
    assert np.array_equal(s["carry"][0], ret) and np.array_equal(s["carry"][1], ci)
    assert s["same_state"]                                                              # both envs were stepped alike
    rows = s["rows"]
    assert (rows[:, 0] == E).all()                                                      # conditions on the inputs (the CPU test's regime)
    assert rows[:, native.EVAL_COLLIDED].sum() > 0 and rows[:, native.EVAL_OUT_OF_BOUNDS].sum() > 0 and rows[:, native.EVAL_MAX_STEPS].sum() > 0
    assert rows[:, native.EVAL_GOALS].sum() > 0


def test_greedy_evaluation_equals_the_walk_over_a_python_loop(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    a, b = _vec(N_EV, max_steps=MAX_STEPS), _vec(N_EV, max_steps=MAX_STEPS)
    pol = _policy(torch, a.states_history, seed=5)
    ev = NativeEvaluator(a)
    a.reset_tensor(); b.reset_tensor()
    ev.run(pol, E, T, greedy=True)
    rows = {"rew": [], "done": [], "flags": []}
    ev_b = NativeEvaluator(b)                                                           # the accounting launch alone, after each own step
    for _ in range(T):
        act = b.policy_act(pol, greedy=True)[0]
        _, r, d, f = b.step_tensor(act)
        ev_b.account(E)
        rows["rew"].append(r.clone()); rows["done"].append(d.clone()); rows["flags"].append(f.clone())
    want, (ret, ci) = _walk({k: torch.stack(v) for k, v in rows.items()}, E)
    assert np.array_equal(_rows(ev), want) and int(want[:, 0].sum()) > 0
    got = _carry(ev)
    assert np.array_equal(got[0], ret) and np.array_equal(got[1], ci)
    assert torch.equal(a.obs, b.obs) and _same_columns(torch, a, b)
    assert torch.equal(ev.act, act)                                                     # the scratch rows hold the last step's
    assert np.array_equal(_rows(ev_b), want) and np.array_equal(_carry(ev_b)[1], ci) and ev_b.steps == T
    a.close(); b.close()


def test_quota_and_carry(torch_cuda, sampled_run):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    s = sampled_run
    env = _vec(N_EV, max_steps=MAX_STEPS)
    ev = NativeEvaluator(env)
    env.reset_tensor()
    ev.run(s["pol"], E, 37, greedy=False, uniforms=s["u"][:37])
    mid = _rows(ev)
    ev.run(s["pol"], E, 63, greedy=False, uniforms=s["u"][37:])
    assert not np.array_equal(mid, s["rows"])                                           # (the second call did add episodes)
    assert np.array_equal(_rows(ev), s["rows"])                                         # 37 + 63 = one call of 100: rows ...
    got = _carry(ev)
    assert np.array_equal(got[0], s["carry"][0]) and np.array_equal(got[1], s["carry"][1])   # ... and carries
    ev.run(s["pol"], E, 60, greedy=False, seed=3, step0=100)                            # past the quota: neither changes
    got = _carry(ev)
    assert np.array_equal(_rows(ev), s["rows"]) and np.array_equal(got[0], s["carry"][0]) and np.array_equal(got[1], s["carry"][1])
    assert ev.steps == 160
    # too few steps for two episodes of 40: incomplete; the default max_steps always suffices
    r = ev.evaluate(s["pol"], E, greedy=False, seed=1, max_steps=30)
    assert r["complete"] is False and r["steps"] == 30 and int(r["per_env"][:, 0].min()) < E
    r = ev.evaluate(s["pol"], E, greedy=False, seed=1, chunk=32)
    assert r["complete"] is True and r["steps"] <= E * MAX_STEPS and r["steps"] % 32 in (0, E * MAX_STEPS % 32)
    pe = r["per_env"].cpu().numpy()
    assert (pe[:, 0] == E).all() and np.array_equal(r["per_member"].cpu().numpy(), pe.sum(0, keepdims=True))
    assert r["return_mean"][0] == pe[:, 1].sum() / 100.0 / pe[:, 0].sum() and r["length_mean"][0] == pe[:, 2].sum() / pe[:, 0].sum()
    assert 0.0 < r["length_mean"][0] <= MAX_STEPS
    for k in ("collision_rate", "out_of_bounds_rate", "max_steps_rate", "no_goals_left_rate"):
        assert 0.0 <= r[k][0] <= 1.0
    assert r["collision_rate"][0] + r["out_of_bounds_rate"][0] + r["max_steps_rate"][0] + r["no_goals_left_rate"][0] >= 1.0
    with pytest.raises(ValueError):
        ev.evaluate(s["pol"], E, greedy=True, uniforms=s["u"])
    env.close()


@pytest.mark.parametrize("split", [False, True])
def test_population_evaluation_is_each_member_alone(torch_cuda, split):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    from ship_sim_gym_amd.population import NativePopulation
    P, n = 4, 64
    env = _vec(P * n, max_steps=MAX_STEPS)
    pop = NativePopulation([_policy(torch, env.states_history, seed=40 + m, split=split) for m in range(P)])
    ev = NativeEvaluator(env)
    env.reset_tensor()
    ev.run(pop, E, T, greedy=False, seed=9, step0=3)                                    # Philox over the GLOBAL env id
    rows = _rows(ev)
    assert int(rows[:, 0].sum()) > 0
    for m in range(P):
        one = _vec(n, max_steps=MAX_STEPS, env_id_base=m * n)
        ev1 = NativeEvaluator(one)
        one.reset_tensor()
        ev1.run(pop.member(m), E, T, greedy=False, seed=9, step0=3)
        assert np.array_equal(rows[m * n:(m + 1) * n], _rows(ev1)), m
        assert np.array_equal(ev1.reduce(1).cpu().numpy(), _rows(ev1).sum(0, keepdims=True)), m   # P = 1
        assert torch.equal(env.obs[m * n:(m + 1) * n], one.obs), m
        one.close()
    assert np.array_equal(ev.reduce(P).cpu().numpy(), rows.reshape(P, n, 8).sum(1))
    assert np.array_equal(ev.reduce(1).cpu().numpy(), rows.sum(0, keepdims=True))
    ev.member_stats.fill_(-7)                                                           # written, not accumulated
    assert np.array_equal(ev.reduce(2).cpu().numpy(), rows.reshape(2, 2 * n, 8).sum(1))
    env.close()


@pytest.mark.parametrize("kind", ["history3", "n_ships4", "ring4"])
def test_other_handle_kinds(torch_cuda, kind):
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    # (ring4: a world per episode out of rings of 4 — three episode starts between two refills, episodes of at most 40 steps)
    kw = {"history3": dict(history=3), "n_ships4": dict(n_ships=4, n_maps=16), "ring4": dict(map_mode="fresh_device", ring=4)}[kind]
    a, b = _vec(128, max_steps=MAX_STEPS, **kw), _vec(128, max_steps=MAX_STEPS, **kw)
    pol = _policy(torch, a.states_history, act="relu", seed=2)
    ev = NativeEvaluator(a)
    a.reset_tensor(); b.reset_tensor()
    ev.run(pol, E, T, greedy=False, seed=5, step0=1)
    r = b.rollout_policy(pol, T, seed=5, step0=1)
    want, _ = _walk(r, E)
    assert np.array_equal(_rows(ev), want) and int(want[:, 0].min()) >= 1
    assert torch.equal(a.obs, b.obs) and _same_columns(torch, a, b)
    a.close(); b.close()


def test_evaluate_script_prints_one_row_per_policy(torch_cuda):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train", "evaluate_native.py"), "--envs", "256", "--episodes", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert lines[0].split()[:2] == ["policy", "episodes"] and len(lines) == 2, out.stdout
    assert lines[1].split()[0] == "policy" and int(lines[1].split()[1]) == 256         # every env counted its one episode
