"""GPU checks of the KL coefficient's adaptation AT its decision boundaries (ppo_kl_adapt_kernel, the last launch of ssg_ppo_update_ext,
ssg_pop_update_ext and ssg_pop_update_sched).  The kernel compares the f32 mean of the last epoch's per-minibatch mean(KL) with
kl_target: x 1.5 above 2 x target, x 0.5 below 0.5 x target, else nothing, both inequalities strict.  Four things feed that comparison —
the reduce kernel's running sum klacc[m], the first_chunk flag that restarts it, the divisor (the chunks MADE, per member on schedules)
and the per-member targets — and every one of them is reproducible on the host: the stats rows hold the device's own minibatch means
in column 4, ppo_reference.kl_adapt restates the f32 sum in chunk order and the comparison.  So nothing here has a tolerance.

The pattern of every test: a probe update with the KL term on and no target; from ITS stats rows the four targets of
ppo_reference.kl_boundary_targets (one float32 below mean / 2, mean / 2, 2 x mean, one float32 above 2 x mean: factors 1.5, 1, 1,
0.5); then the same update from the same parameters once per target.  The target must change nothing but the coefficient (stats,
parameters and moments are the probe's, torch.equal), and the coefficient is kl_adapt's and the named factor, ==.  Populations rotate
the four targets over their members, so every member meets every side, and compare with NativePPO on the member's shard as well.

Before it uses the targets every test asserts that they can tell the right mean from the plausible wrong ones (_targets): the last
chunk's mean over the chunk count, the sum that was never restarted between epochs, the sum over the minibatches ASKED FOR, and
for populations the sum over another member's chunk count."""
import numpy as np
import pytest

from gpu_support import DEV, vec
from gpu_support import torch_cuda  # noqa: F401
from population_harness import age, cached, member_hparams, perms_per_member, shard_reference, shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import KL_BOUNDARY_FACTORS, actor_critic_policy, kl_adapt, kl_boundary_targets, kl_factor, kl_mean, split_policy, \
    synthetic_batch

pytestmark = pytest.mark.gpu

D = 22
KL_COEF = 1.0
TERMS = dict(vf_clip=0.05, max_grad_norm=0.05, kl_coef=KL_COEF)
F32 = np.float32

_ENVS, _SINGLE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()
    _SINGLE.clear()


def _env():
    """One small handle for every single-policy test (the PPO calls take their own K and N)."""
    if D not in _ENVS:
        _ENVS[D] = vec(64, D)
    return _ENVS[D]


def _targets(kls_last, kls_all, chunks, epochs, asked, other_chunks=(), also=None):
    """kl_boundary_targets of the probe's last-epoch means, after asserting that the mean is finite and positive and that the four
    targets tell it from every wrong mean that applies — each computed in f32 as kl_adapt computes the right one:
    (a) the last chunk alone over the chunk count (first_chunk always set), with more than one chunk;
    (b) every epoch's chunks over the chunk count (first_chunk never set), with more than one epoch;
    (c) the sum over the minibatches asked for, where fewer chunks were made;
    (d) the sum over another member's chunk count, where the counts differ;
    and whatever `also` names.  A condition on the batch, not a measurement: a seed that violates it is to be replaced."""
    kls_last = np.asarray(kls_last, dtype=F32)
    assert len(kls_last) == chunks and len(kls_all) == epochs * chunks
    mean = kl_mean(kls_last)
    assert mean.dtype == F32 and np.isfinite(mean) and mean > 0 and bool((kls_last > 0).all())
    pairs = kl_boundary_targets(kls_last)
    assert tuple(f for _, f in pairs) == KL_BOUNDARY_FACTORS
    assert all(float(F32(t)) == t and t > 0 for t, _ in pairs) and len({t for t, _ in pairs}) == 4
    wrong = dict(also or {})
    if chunks > 1:
        wrong["(a) last chunk / chunks"] = kl_mean(kls_last[-1:], chunks)
    if epochs > 1:
        wrong["(b) every epoch / chunks"] = kl_mean(kls_all, chunks)
    if asked != chunks:
        wrong["(c) sum / minibatches asked for"] = kl_mean(kls_last, asked)
    for c in sorted(set(other_chunks) - {chunks}):
        wrong["(d) sum / %d chunks of another member" % c] = kl_mean(kls_last, c)
    for name, w in wrong.items():
        assert [kl_factor(w, t) for t, _ in pairs] != list(KL_BOUNDARY_FACTORS), (name, float(w), float(mean))
    return pairs


def _adapted(coef, factor):
    return F32(F32(coef) * F32(factor))


# ------------------------------------------------------------------------------------------------------------------------------------
# one policy
# ------------------------------------------------------------------------------------------------------------------------------------
def _single(torch, K, envs, split=False):
    """(policy, batch) per shape, computed once: D = 22, two layers (64 wide, or separate towers of 48), a synthetic rollout batch whose
    acting policy is an older one, so the KL is alive."""
    key = (K, envs, split)
    if key not in _SINGLE:
        make = split_policy if split else actor_critic_policy
        _, pol = make(torch, D, 48 if split else 64, 2, "tanh", 3, seed=K + envs)
        _SINGLE[key] = (pol, synthetic_batch(torch, pol, K, envs, 100 + K + envs))
    return _SINGLE[key]


def _perm(torch, n, epochs, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(epochs)])


def _check_single(torch, K, envs, epochs, minibatches, chunks, split=False, **ppo_kw):
    """The four targets, with and without a stats buffer, against the probe of (K, envs, epochs, minibatches)."""
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    pol, b = _single(torch, K, envs, split)
    assert pol.separate_value == split
    n = K * envs
    assert chunk_split(n, minibatches)[1] == chunks
    perm = _perm(torch, n, epochs, minibatches)
    p0 = pol.params.detach().clone()

    def run(target, stats):
        pol.params.copy_(p0)
        ppo = NativePPO(pol, _env(), kl_target=target, **TERMS, **ppo_kw)
        ppo.gae(b)
        return ppo, ppo.update(b, perm, epochs, minibatches, stats=stats)

    try:
        probe, s_probe = run(0.0, True)
        assert s_probe.shape == (epochs * chunks, 8) and bool(torch.isfinite(s_probe).all())
        assert probe.kl_coef.tolist() == [KL_COEF] and bool((s_probe[:, 6] == KL_COEF).all())
        first, mv = pol.params.detach().clone(), probe.adam_mv.clone()
        assert not torch.equal(first, p0)
        kls_all = s_probe[:, 4].cpu().numpy()
        kls = kls_all[-chunks:]
        # (one epoch of one chunk is exempt from (a) to (c) by construction: the last chunk IS the epoch, and 1 minibatch makes 1 chunk)
        pairs = _targets(kls, kls_all, chunks, epochs, minibatches)
        print("%s: mean KL %.9g, targets %s" % ((K, envs, epochs, minibatches), float(kl_mean(kls)), [t for t, _ in pairs]))
        for target, factor in pairs:
            for stats in (True, False):                                      # klacc is written whether or not a stats row is
                ppo, st = run(target, stats)
                assert (st is None) == (not stats) and (st is None or torch.equal(st, s_probe)), (target, stats)
                # the target changes nothing but the coefficient
                assert torch.equal(pol.params, first) and torch.equal(ppo.adam_mv, mv) and ppo.step == epochs * chunks, (target, stats)
                got, want = ppo.kl_coef.cpu().numpy()[0], kl_adapt(KL_COEF, kls, target)
                assert got.dtype == F32 and got == want == _adapted(KL_COEF, factor), (target, stats, got, want, factor)
    finally:
        pol.params.copy_(p0)


@pytest.mark.parametrize("K,envs,epochs,minibatches,chunks", [(8, 125, 2, 4, 4), (8, 125, 2, 3, 3), (2, 5, 2, 6, 5), (8, 125, 1, 1, 1)],
                         ids=["even", "short-last-chunk", "fewer-chunks-than-asked", "single-chunk"])
def test_one_policy_at_the_boundaries(torch_cuda, K, envs, epochs, minibatches, chunks):
    """An even split (4 x 250), a short last chunk (334, 334, 332), fewer chunks than asked (5 of 2 samples for 6) and a single chunk
    that is both the first and the last of its epoch; each with a stats buffer and with dev_stats NULL."""
    _check_single(torch_cuda, K, envs, epochs, minibatches, chunks)


def test_one_policy_with_per_minibatch_advantage_normalisation(torch_cuda):
    _check_single(torch_cuda, 8, 125, 2, 3, 3, adv_norm="minibatch")


def test_one_policy_with_a_separate_value_network(torch_cuda):
    _check_single(torch_cuda, 8, 125, 2, 3, 3, split=True)


def test_second_update_on_the_same_workspace_starts_its_own_sum(torch_cuda):
    """A 5-chunk update, then a 2-chunk one on the same NativePPO and the same workspace bytes: the second update's four targets come
    from ITS probe rows, and nothing of the first call's sum (nor its chunk count) may enter."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO, chunk_split
    K, envs, epochs = 2, 5, 2
    pol, b = _single(torch, K, envs)
    n = K * envs
    assert chunk_split(n, 6)[1] == 5 and chunk_split(n, 2) == (5, 2)
    perm_a, perm_b = _perm(torch, n, epochs, 1), _perm(torch, n, epochs, 2)
    p0 = pol.params.detach().clone()

    def run(target):
        pol.params.copy_(p0)
        ppo = NativePPO(pol, _env(), **TERMS)
        ppo.gae(b)
        ppo._ws(n, n)                                                        # room for either chunking: the workspace never grows below
        ws = ppo.workspace.data_ptr()
        s_a = ppo.update(b, perm_a, epochs, 6, stats=True)
        assert ppo.kl_coef.tolist() == [KL_COEF]                            # no target: the first update leaves the coefficient alone
        ppo.kl_target = target
        s_b = ppo.update(b, perm_b, epochs, 2, stats=True)
        assert ppo.workspace.data_ptr() == ws and ppo.step == epochs * (5 + 2)
        return ppo, s_a, s_b

    try:
        probe, a_probe, b_probe = run(0.0)
        assert a_probe.shape == (10, 8) and b_probe.shape == (4, 8) and bool(torch.isfinite(b_probe).all())
        last, mv = pol.params.detach().clone(), probe.adam_mv.clone()
        a_all, b_all = a_probe[:, 4].cpu().numpy(), b_probe[:, 4].cpu().numpy()
        carried = {"the first call's last epoch carried over": kl_mean(np.concatenate([a_all[-5:], b_all[-2:]]), 2),
                   "everything since the object was made": kl_mean(np.concatenate([a_all, b_all]), 2),
                   "the first call's chunk count": kl_mean(b_all[-2:], 5)}
        pairs = _targets(b_all[-2:], b_all, 2, epochs, 2, also=carried)
        for target, factor in pairs:
            ppo, s_a, s_b = run(target)
            assert torch.equal(s_a, a_probe) and torch.equal(s_b, b_probe) and torch.equal(pol.params, last) and torch.equal(ppo.adam_mv, mv)
            got, want = ppo.kl_coef.cpu().numpy()[0], kl_adapt(KL_COEF, b_all[-2:], target)
            assert got.dtype == F32 and got == want == _adapted(KL_COEF, factor), (target, got, want, factor)
    finally:
        pol.params.copy_(p0)


# ------------------------------------------------------------------------------------------------------------------------------------
# populations
# ------------------------------------------------------------------------------------------------------------------------------------
def _ext_terms(P):
    """RLlib's loss, PPO2's, the KL term alone, everything on — every member with its own coefficient > 0."""
    pick = lambda row: [row[m % 4] for m in range(P)]  # noqa: E731
    return {"vf_clip": pick((10.0, 0.05, 0.0, 0.2)), "max_grad_norm": pick((0.0, 0.03, 0.0, 0.5)), "kl_coef": pick((1.0, 0.5, 0.3, 2.0))}


def _sharded(torch, sizes, K, bind):
    """(env, pop, batch, shard envs, reference policies, shard batches) of population_harness.shard_rollouts at D = 22, aged with forced
    dones; bind: `sizes` bound to the population's handle as slices.  Computed once per layout and left unchanged."""
    sizes = list(sizes)

    def make_env(n, base):
        env = vec(n, D, base=base)
        if bind and n == sum(sizes):
            env.set_population_slices(sizes)
        return env

    def make():
        P = len(sizes)
        setup = shard_rollouts(torch, make_env, lambda d: [actor_critic_policy(torch, d, seed=100 + m)[1] for m in range(P)], sizes, K, 7)
        env, pop, b, shards, refs, sbs = setup
        age(torch, b, sbs, sizes, pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(P * 1000 + sum(sizes) + K), True)
        return setup
    return cached((tuple(sizes), K, bind), make)


def _unsharded(torch, P, n, K):
    """The same six for P members of n envs WITHOUT shard envs (one-layer policies 16 wide): the host restatement is the reference."""
    def make():
        from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
        env = vec(P * n, D)
        pop = NativePopulation([actor_critic_policy(torch, D, 16, 1, "tanh", 3, seed=300 + m)[1] for m in range(P)])
        env.reset_tensor()
        b = dict(env.rollout_population(pop, K, seed=7))
        la = PopulationPPO(pop, env).dist(b)
        age(torch, b, [], [n] * P, pop.n_actions, la, torch.Generator(device=DEV).manual_seed(P + n + K), False)
        return env, pop, b, [], [], []
    return cached((P, n, K, "unsharded"), make)


def _check_population(torch, setup, sizes, K, epochs, minibatches, zero_member=None):
    """Four rounds from the same parameters: member m at target number (m + r) % 4 of ITS four in round r, against the host restatement
    from the probe's rows st[m, steps_m - chunks_m : steps_m, 4] and, where the set-up has shard envs, bit for bit against NativePPO on
    the shard at that same target.  zero_member: one more round in which that member's target is 0 — its coefficient stays."""
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import chunk_split
    env, pop, b, shards, refs, sbs = setup
    sizes = list(sizes)
    P = len(sizes)
    assert len(pop) == P and env.num_envs == sum(sizes)
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    ep = list(epochs) if isinstance(epochs, list) else [epochs] * P
    mb = list(minibatches) if isinstance(minibatches, list) else [minibatches] * P
    samples = [K * s for s in sizes]
    chunks = [chunk_split(s, c)[1] for s, c in zip(samples, mb)]
    steps = [e * c for e, c in zip(ep, chunks)]
    g = torch.Generator(device=DEV).manual_seed(11)
    perm = perms_per_member(torch, g, max(ep), samples) if env.population_slices is not None else stacked_perms(torch, g, P, max(ep), samples[0])
    hp, terms = member_hparams(P), _ext_terms(P)
    coef0 = np.asarray(terms["kl_coef"], dtype=F32)
    saved = pop.params.clone(), [r.params.clone() for r in refs]

    def run(targets):
        pop.params.copy_(saved[0])
        ppo = PopulationPPO(pop, env, **hp, kl_target=targets, **terms)
        ppo.gae(b)
        st = ppo.update(b, perm, epochs, minibatches, stats=True)
        assert st.shape == (P, max(steps), 8) and ppo.member_steps == steps
        return ppo, st

    try:
        probe, st0 = run([0.0] * P)
        assert bool(torch.isfinite(st0).all()) and probe.extended() and np.array_equal(probe.kl_coef.cpu().numpy(), coef0)
        first, mv = pop.params.clone(), probe.adam_mv.clone()
        rows = st0[:, :, 4].cpu().numpy()
        kls = [rows[m, steps[m] - chunks[m]:steps[m]] for m in range(P)]   # member m's LAST epoch ends where its own steps end
        pairs = [_targets(kls[m], rows[m, :steps[m]], chunks[m], ep[m], mb[m], other_chunks=chunks) for m in range(P)]
        rounds = [[(m + r) % 4 for m in range(P)] for r in range(4)]
        if zero_member is not None:
            rounds.append([None if m == zero_member else k for m, k in enumerate(rounds[0])])
        for r, kinds in enumerate(rounds):
            targets = [0.0 if k is None else pairs[m][k][0] for m, k in enumerate(kinds)]
            ppo, st = run(targets)
            assert torch.equal(st, st0) and torch.equal(pop.params, first) and torch.equal(ppo.adam_mv, mv), r
            got = ppo.kl_coef.cpu().numpy()
            assert got.dtype == F32
            for m, k in enumerate(kinds):
                if k is None:
                    assert got[m] == coef0[m], (r, m, got[m])               # a target of 0 keeps the coefficient, whatever klacc holds
                else:
                    want = kl_adapt(coef0[m], kls[m], targets[m])
                    assert got[m] == want == _adapted(coef0[m], pairs[m][k][1]), (r, m, k, got[m], want, targets[m])
            for m in range(P if shards else 0):
                refs[m].params.copy_(saved[1][m])
                ref = shard_reference(torch, m, hp, dict(terms, kl_target=targets), refs, shards, sbs)
                r_st = ref.update(sbs[m], perm[m][:ep[m]].contiguous(), ep[m], mb[m], stats=True)
                assert torch.equal(st[m, :steps[m]], r_st) and torch.equal(pop.params[m], refs[m].params), (r, m)
                assert torch.equal(ppo.kl_coef[m:m + 1], ref.kl_coef), (r, m, ppo.kl_coef.tolist(), ref.kl_coef.tolist())
        return pairs
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)


def test_population_common_entry_at_the_boundaries(torch_cuda):
    """ssg_pop_update_ext: 4 members of 800 samples, two epochs of chunks 267, 267, 266; member 1 also with a target of 0."""
    torch = torch_cuda
    sizes = [100] * 4
    _check_population(torch, _sharded(torch, sizes, 8, False), sizes, 8, 2, 3, zero_member=1)


def test_population_schedules_at_the_boundaries(torch_cuda):
    """ssg_pop_update_sched on the shapes of test_extended_loss_on_uneven_schedules: 800 samples per member, chunk counts 4, 1, 5, 3 and
    steps 8, 1, 15, 6 of 15 launches — three members are adapted from a sum they stopped touching launches ago, each over ITS count."""
    torch = torch_cuda
    sizes = [100] * 4
    _check_population(torch, _sharded(torch, sizes, 8, False), sizes, 8, [2, 1, 3, 2], [4, 1, 5, 3], zero_member=1)


def test_population_on_unequal_slices_at_the_boundaries(torch_cuda):
    """ssg_pop_set_slices: 41 / 80 / 123 envs (bases 41 and 121, unaligned), 328 / 640 / 984 samples in chunks 110, 110, 108; 640; and
    4 x 197, 196 — three chunk counts, two short last chunks, and no member beyond the file's largest shape of 8 x 125 samples."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import chunk_split
    sizes = [41, 80, 123]
    assert [chunk_split(8 * s, c) for s, c in zip(sizes, [3, 1, 5])] == [(110, 3), (640, 1), (197, 5)]
    _check_population(torch, _sharded(torch, sizes, 8, True), sizes, 8, [2, 1, 2], [3, 1, 5])


@pytest.mark.parametrize("P,n,lists", [(70, 16, False), (70, 16, True), (256, 8, False)], ids=["70-common", "70-schedules", "max-members"])
def test_more_members_than_one_wave(torch_cuda, P, n, lists):
    """The adaptation kernel maps member m to lane m of one 256-lane workgroup: 70 members are more than one wave of 64,
    SSG_POP_MAX_MEMBERS fill it.  K = 4; two epochs of two chunks, or on schedules 1, 2 and 3 chunks (22, 22, 20 of 64 samples).
    No shard envs: the host restatement alone.  Member 65, a lane of the second wave, also runs a round with a target of 0."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    assert P in (70, N.POP_MAX_MEMBERS)
    epochs, minibatches = ([(2, 1)[m % 2] for m in range(P)], [(1, 2, 3)[m % 3] for m in range(P)]) if lists else (2, 2)
    _check_population(torch, _unsharded(torch, P, n, 4), [n] * P, 4, epochs, minibatches, zero_member=65)
