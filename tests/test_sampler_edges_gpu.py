"""GPU checks of the action sampler AT its decision boundaries (step 4 of policy_act_body in csrc/shipsim_policy.hip): the threshold each
action flips at, that logp flips on the same row, monotonicity, u = 0 and u = 1 - 2^-24, logits with large offsets, -inf, NaN and +inf
logits.  tests/sampler_edges.py has the idea (zero Wpi makes the logits bpi bit for bit, so one launch over 12 304 envs scans 12 304
values of u against one logits row), the table, the f64 reference, the bound B and the assertions; tests/test_sampler_edges.py shows on
the host that every defect these tests are there for fails a named case.

Every kernel that carries the step runs the whole table (70 logits rows: 22, 24 and 24 for A = 2, 3 and 4): the shared body (L = 1 and 2, tanh and
relu, H = 16 and 48), the separate-value body, a population on equal and on unequal slices, the observation-filter kernels and the fused
rollout; each must also return the plain shared launch's act and logp bit for bit.

Measured on the MI355X (each sweep prints its own figures, test_every_instantiation_was_scanned the tally): 70 cases, 1 120 scans of
12 304 envs over 42 sweeps (14 kernels / layouts x 3 action counts, the fused rollout two scans per case); the largest
|k_j * 2^-24 - cdf64_j| / B is 0.108 (A = 3; 0.089 for A = 2 and 4), the same in every sweep and 0.089 in numpy's restatement.  B is the
condition, the ratio only recorded.  Per table, 4 of 19 (A = 2), 8 of 42 (A = 3) and 11 of 63 (A = 4) thresholds lie within B of 0 or of
1 - 2^-24 and are not asked for a flip.  The module takes about 5 s.

What the tests found.  No case of the table failed on the device, but numpy's restatement drew the masked action of "-inf/last/A=3" at
u = 1 - 2^-24: the f32 sum of the other probabilities stopped at 1 - 2^-23.  The device's expf rounds that row the other way, yet the
formula admits it: over 12 304 rows with random logits and a masked last action the kernel drew the masked action on 2 005 (A = 3) and
1 699 (A = 4) of them at u = 1 - 2^-24, with logp = -inf.  policy_act_body now steps back from a masked action;
test_a_masked_action_is_never_drawn is that measurement as a test, and two of the rows it found are in the table ("-inf/last/short").
"""
import numpy as np
import pytest

import sampler_edges as E
from gpu_support import DEV, torch_cuda, vec  # noqa: F401
from ppo_reference import actor_critic_policy, split_policy

pytestmark = pytest.mark.gpu

D = 7
SLICES = (2049, 4100, 6155)         # member 0 ends on the centre row of window 0; 1, 4 and 11 rows in the tail workgroups


@pytest.fixture(scope="module")
def env(torch_cuda):
    e = vec(E.N_ENVS, D)
    e.reset_tensor()
    yield e
    _PLAIN.clear()
    _U.clear()
    e.close()


_SCANS, _U, _PLAIN, _SEEN = {}, {}, {}, {}


def _scan(case):
    if case.name not in _SCANS:
        _SCANS[case.name] = E.scan(case)
    return _SCANS[case.name]


def _u(torch, case):
    if case.name not in _U:
        _U[case.name] = torch.tensor(_scan(case).u, device=DEV)
    return _U[case.name]


def _policy(torch, mode, H, L, act, A, seed):
    """A policy whose Wpi is zero: logits == bpi whatever the trunk computes."""
    _, pol = (actor_critic_policy if mode == "shared" else split_policy)(torch, D, H, L, act, A, seed=seed)
    assert pol.separate_value == (mode == "split")
    o, s = pol.offsets["Wpi"]
    pol.params[o: o + int(np.prod(s))].zero_()
    return pol


def _set_logits(torch, params, pol, case):
    """bpi = the case's row, in `params` ([P] or [members, P])."""
    o, s = pol.offsets["bpi"]
    assert s == (case.A,)
    params[..., o: o + case.A] = torch.tensor(case.lg, dtype=torch.float32, device=DEV)


def _plain(torch, env, case):
    """The case through the plain shared launch (L = 1, tanh, H = 16): (act, logp) numpy, kept per module."""
    if case.name not in _PLAIN:
        key = ("plain", case.A)
        if key not in _PLAIN:
            _PLAIN[key] = _policy(torch, "shared", 16, 1, "tanh", case.A, seed=case.A)
        pol = _PLAIN[key]
        _set_logits(torch, pol.params, pol, case)
        a, lp, _, _ = env.policy_act(pol, uniforms=_u(torch, case))
        _PLAIN[case.name] = (a.cpu().numpy(), lp.cpu().numpy())
    return _PLAIN[case.name]


def _sweep(torch, env, tag, A, launch):
    """Every case of A through launch(case, u) -> [(act, logp, logp_all or None)] (one entry per scan the launch made): check_case on
    each, and the plain shared launch's bits.  Prints what was measured."""
    worst, flipless, thresholds, scans = 0.0, 0, 0, 0
    for case in E.cases(A):
        sc = _scan(case)
        pa, pl = _plain(torch, env, case)
        for act, logp, la in launch(case, _u(torch, case)):
            act, logp = act.cpu().numpy(), logp.cpu().numpy()
            rec = E.check_case(case, sc.u, act, logp, None if la is None else la.cpu().numpy())
            assert np.array_equal(act, pa), (tag, case.name, np.flatnonzero(act != pa)[:4], sc.u[act != pa][:4])
            assert E.same_float(logp, pl).all(), (tag, case.name)
            worst, flipless, thresholds, scans = max(worst, rec["ratio"]), flipless + len(rec["flipless"]), thresholds + rec["thresholds"], scans + 1
    print("%s A=%d: %d scans of %d envs, %d thresholds, %d of them within B of an end (no flip asked for); the largest |k_j * 2^-24 - cdf64_j| / B is %.4f"
          % (tag, A, scans, E.N_ENVS, thresholds, flipless, worst))
    _SEEN[tag, A] = (scans, worst)                                              # (B is check_case's condition; the ratio is only recorded)


def _with_dist(torch, env, pol):
    """launch(case, u) of policy_act under `pol`, logp_all from the trainer's dist on the stored x."""
    from ship_sim_gym_amd.ppo import NativePPO
    ppo = NativePPO(pol, env)

    def launch(case, u):
        _set_logits(torch, pol.params, pol, case)
        a, lp, _, x = env.policy_act(pol, uniforms=u)
        return [(a, lp, ppo.dist({"obs": x}))]
    return launch


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("L,act,H", [(1, "tanh", 16), (2, "relu", 16), (1, "relu", 48), (2, "tanh", 48)])
def test_shared_body(torch_cuda, env, L, act, H, A):
    torch = torch_cuda
    pol = _policy(torch, "shared", H, L, act, A, seed=H + L + A)
    _sweep(torch, env, "shared L=%d %s H=%d" % (L, act, H), A, _with_dist(torch, env, pol))


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("L,act,H", [(2, "tanh", 16), (1, "relu", 48)])
def test_separate_value_body(torch_cuda, env, L, act, H, A):
    torch = torch_cuda
    pol = _policy(torch, "split", H, L, act, A, seed=H + L + A)
    _sweep(torch, env, "split L=%d %s H=%d" % (L, act, H), A, _with_dist(torch, env, pol))


def _population(torch, mode, n_members, A):
    """Members with different trunks and zero Wpi."""
    from ship_sim_gym_amd.population import NativePopulation
    members = [_policy(torch, mode, 16, 2, "tanh", A, seed=10 * m + A) for m in range(n_members)]
    pop = NativePopulation(members)
    assert not torch.equal(pop.params[0], pop.params[-1])
    return pop, members[0]


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("mode", ["shared", "split"])
def test_population_on_equal_slices(torch_cuda, env, mode, A):
    torch = torch_cuda
    pop, first = _population(torch, mode, 2, A)
    assert (E.N_ENVS // 2) % 64 != 0

    def launch(case, u):
        _set_logits(torch, pop.params, first, case)
        a, lp, _, _ = env.population_act(pop, uniforms=u)
        return [(a, lp, None)]
    _sweep(torch, env, "population %s, 2 equal slices" % mode, A, launch)


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("mode", ["shared", "split"])
def test_population_on_unequal_slices(torch_cuda, env, mode, A):
    """A window straddles a member boundary and a tail workgroup: member 0's last row is the centre row of window 0."""
    torch = torch_cuda
    pop, first = _population(torch, mode, len(SLICES), A)
    assert sum(SLICES) == E.N_ENVS and all(s % 64 for s in SLICES) and SLICES[0] == E.HALF + 1
    env.set_population_slices(SLICES)
    try:
        def launch(case, u):
            _set_logits(torch, pop.params, first, case)
            a, lp, _, _ = env.population_act(pop, uniforms=u)
            return [(a, lp, None)]
        _sweep(torch, env, "population %s, slices %s" % (mode, SLICES), A, launch)
    finally:
        env.set_population_slices(None)


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("mode", ["shared", "split"])
def test_with_an_observation_filter_bound(torch_cuda, env, mode, A):
    torch = torch_cuda
    from ship_sim_gym_amd.obs_filter import ObsFilter
    pol = _policy(torch, mode, 16, 1, "tanh", A, seed=A)
    flt = ObsFilter(env, clip=5.0, update=False)
    flt.update()
    env.set_obs_filter(flt)
    try:
        x0 = env.policy_act(pol, uniforms=_u(torch, E.cases(A)[0]))[3]
        assert not torch.equal(x0, (env.obs / pol.obs_scale).float())               # the filter kernels ran
        _sweep(torch, env, "%s, filter bound" % mode, A, _with_dist(torch, env, pol))
    finally:
        env.set_obs_filter(None)


@pytest.mark.parametrize("A", E.ACTIONS)
@pytest.mark.parametrize("mode", ["shared", "split"])
def test_fused_rollout(torch_cuda, env, mode, A):
    """rollout_policy with uniforms [2, N]: each row is its own scan (the envs have moved on between them; the logits have not)."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    pol = _policy(torch, mode, 16, 2, "relu", A, seed=A + 1)
    ppo = NativePPO(pol, env)
    K = 2

    def launch(case, u):
        _set_logits(torch, pol.params, pol, case)
        b = dict(env.rollout_policy(pol, K, uniforms=u.repeat(K, 1).contiguous()))
        la = ppo.dist(b)
        assert not torch.equal(b["obs"][0], b["obs"][1])
        return [(b["act"][k], b["logp"][k], la[k]) for k in range(K)]
    _sweep(torch, env, "%s, fused rollout K=%d" % (mode, K), A, launch)


@pytest.mark.parametrize("A,masked", [(2, (1,)), (3, (2,)), (3, (1, 2)), (4, (3,)), (4, (1, 3)), (4, (2, 3))])
@pytest.mark.parametrize("mode", ["shared", "split"])
def test_a_masked_action_is_never_drawn(torch_cuda, env, mode, A, masked):
    """Every env its own logits row (Wpi is NOT zero here), the logits in `masked` at -inf, u at the three largest values of the grid
    and at 0.5: no masked action, a finite logp that is the distribution's entry for the stored action, and no action below the f64
    choice for u - 1e-5 (so at the top it is the last action that has a probability, tiny ones aside).  (The plain count drew the masked last action on 2 005 of 12 304 rows at u = 1 - 2^-24.)"""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    _, pol = (actor_critic_policy if mode == "shared" else split_policy)(torch, D, 16, 1, "tanh", A, seed=A)
    (o, s), (ob, _) = pol.offsets["Wpi"], pol.offsets["bpi"]
    pol.params[o: o + int(np.prod(s))] *= 6.0
    for j in masked:
        pol.params[ob + j] = float("-inf")
    ppo = NativePPO(pol, env)
    acts = env.random_actions(7, 0, 30)                                         # apart from each other: most envs get a row of their own
    for k in range(30):
        env.step_tensor(acts[k])
    _, logits, _ = pol.forward_reference(env.obs)
    lp64 = torch.log_softmax(logits.double(), -1)
    assert len(torch.unique(logits[:, 0])) > E.N_ENVS // 4 and bool(torch.isinf(logits[:, list(masked)]).all())
    free = [j for j in range(A) if j not in masked]
    assert free[0] == 0
    for k in (E.TOP, E.TOP - 1, E.TOP - 2, 2 ** 23):
        u = torch.full((E.N_ENVS,), k * E.GRID, dtype=torch.float32, device=DEV)
        a, lp, _, x = env.policy_act(pol, uniforms=u)
        al = a.long().unsqueeze(-1)
        assert bool(((a >= 0) & (a < A)).all()) and not bool(torch.isin(a, torch.tensor(masked, device=DEV)).any()), (k, masked)
        assert bool(torch.isfinite(lp).all()) and torch.equal(lp, ppo.dist({"obs": x}).gather(-1, al).squeeze(-1))
        assert float((lp - lp64.gather(-1, al).squeeze(-1)).abs().max()) <= 1e-4
        lo = (k * E.GRID - 1e-5 > lp64.exp().cumsum(-1)[:, :-1]).sum(-1)        # the f64 choice a rounding band below u: never above act
        assert bool((a >= lo).all()) and (k < E.TOP or int((a == free[-1]).sum()) > E.N_ENVS // 2), (k, masked)


def test_every_instantiation_was_scanned(torch_cuda, env):
    """Runs last: the tally of the sweeps that ran in this session (42 when the whole module did)."""
    assert _SEEN
    scans, worst = sum(s for s, _ in _SEEN.values()), max(w for _, w in _SEEN.values())
    print("%d logits rows, %d scans over %d instantiation x action-count sweeps; the largest |k_j * 2^-24 - cdf64_j| / B overall is %.4f"
          % (len(E.all_cases()), scans, len(_SEEN), worst))
