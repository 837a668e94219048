"""GPU checks of per-member update schedules (ssg_pop_update_sched; PopulationPPO.update with lists of epochs / minibatches;
train/pbt_native.py --mutate-schedule).  The reference of every check is the single-policy path: member m's update is
``NativePPO.update(batch_m, perm[m, :epochs[m]], epochs[m], minibatches[m])`` on a ``ShipVecEnv(n, env_id_base=m*n)`` shard with that
member's settings and Adam step count, and every comparison is torch.equal — parameters, moments, stats rows, the adapted KL coefficient.
The idiom is tests/test_population_gpu.py's and tests/test_population_split_gpu.py's: one population rollout and the P shard rollouts
asserted equal, then the same forced dones and the same older acting policy (noise on its log-distribution and value) in both."""
import ctypes as C
import math

import pytest

from gpu_support import DEV, load_script, vec as split_vec
from gpu_support import torch_cuda  # noqa: F401
from population_harness import age, cached, member_hparams as _hp, shard_reference as _reference, shard_rollouts, stacked_perms as _perm
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy, split_policy

pytestmark = pytest.mark.gpu

SPLIT_SHAPE = (22, 48, 2, 3, "tanh")  # D, H, layers, A, activation of the separate-value population


def _vec(n, base=0, split=False):
    if split:
        return split_vec(n, SPLIT_SHAPE[0], base=base)
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    return ShipVecEnv(n, n_maps=64, env_id_base=base)


def _members(torch, D, P, split, seed=100):
    if split:
        _, H, L, A, act = SPLIT_SHAPE
        return [split_policy(torch, D, H, L, act, A, seed=seed + m)[1] for m in range(P)]
    return [actor_critic_policy(torch, D, seed=seed + m)[1] for m in range(P)]


def _setup(torch, P, n, K, split=False):
    """(env, pop, batch, shard envs, reference policies, shard batches), computed once per shape and left unchanged: every test works
    on copies of the dicts and restores the parameters."""
    def make():
        setup = shard_rollouts(torch, lambda n, base: _vec(n, base, split), lambda D: _members(torch, D, P, split), [n] * P, K, 7)
        env, pop, b, shards, refs, sbs = setup
        age(torch, b, sbs, [n] * P, pop.n_actions, b["logp_all"], torch.Generator(device=DEV).manual_seed(P * 1000 + n + K), True)
        return setup
    return cached((P, n, K, split), make)


def _expected_steps(samples, epochs, minibatches):
    from ship_sim_gym_amd.ppo import chunk_split
    return [e * chunk_split(samples, b)[1] for e, b in zip(epochs, minibatches)]


def _check_rounds(torch, setup, K, ext, rounds, after_round=None):
    """PopulationPPO.update on the schedules of `rounds` ((epochs, minibatches) lists, one update each, each continuing the last)
    against P NativePPO updates.  Returns (ppo, the reference objects, the last stats) with the parameters restored."""
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = setup
    P = len(pop)
    n = env.num_envs // P
    samples = K * n
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    hp = _hp(P)
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, **hp, **ext)
        ppo.gae(b)
        ref_ppos = [_reference(torch, m, hp, ext, refs, shards, sbs) for m in range(P)]
        cols = 8 if ppo.extended() else 4
        g = torch.Generator(device=DEV).manual_seed(11)
        st = None
        for r, (epochs, minibatches) in enumerate(rounds):
            steps = _expected_steps(samples, epochs, minibatches)
            launches = max(steps)
            perm = _perm(torch, g, P, max(epochs), samples)
            before = list(ppo.member_steps)
            st = ppo.update(b, perm, epochs, minibatches, stats=True)
            assert st.shape == (P, launches, cols) and bool(torch.isfinite(st).all())
            assert ppo.member_steps == [s0 + s for s0, s in zip(before, steps)]
            for m in range(P):
                ref = ref_ppos[m]
                assert ref.step == before[m], (r, m)                             # the same starting Adam step, per member
                r_st = ref.update(sbs[m], perm[m, :epochs[m]].contiguous(), epochs[m], minibatches[m], stats=True)
                assert r_st.shape[0] == steps[m] and ref.step == ppo.member_steps[m], (r, m)
                assert torch.equal(pop.params[m], refs[m].params), (r, m, "params")
                assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (r, m, "moments")
                assert torch.equal(st[m, :steps[m], :r_st.shape[1]], r_st), (r, m, "stats")
                assert bool((st[m, :steps[m], r_st.shape[1]:] == 0).all()), (r, m, "columns of terms that are off")
                assert bool((st[m, steps[m]:] == 0).all()), (r, m, "rows past the member's steps")
                assert torch.equal(ppo.kl_coef[m:m + 1], ref.kl_coef), (r, m, "coefficient", ppo.kl_coef.tolist(), ref.kl_coef.tolist())
            if after_round:
                after_round(r, ppo, ref_ppos)
        return ppo, ref_ppos, st
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)


def test_uneven_schedules_are_bitwise_each_members_own(torch_cuda):
    """616 samples per member: 44 chunks of 14 (M below one tile), 9 chunks of 69 (last 64: a ragged second tile) and one chunk of 616
    (ten tiles) in the same launches; the members go idle after 2, 27 and 44 launches.  The second update permutes the schedules, so it
    starts from unequal per-member Adam step counts."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import chunk_split
    assert [chunk_split(616, b) for b in (45, 9, 1)] == [(14, 44), (69, 9), (616, 1)] and 616 - 8 * 69 == 64
    assert _expected_steps(616, [1, 3, 2], [45, 9, 1]) == [44, 27, 2]
    setup = _setup(torch, 3, 77, 8)
    ppo, refs, _ = _check_rounds(torch, setup, 8, {}, [([1, 3, 2], [45, 9, 1]), ([2, 1, 3], [1, 45, 9])])
    assert ppo.member_steps == [44 + 2, 27 + 44, 2 + 27] and ppo.diverged() and not ppo.extended()


def test_capped_grid_next_to_a_small_member(torch_cuda):
    """33 600 samples per member: member 0's single minibatch has 525 tiles on the capped grid of 512 workgroups (the grid-stride
    wrap); member 1's chunks of 4 800 have 75 tiles in the same 512-wide launch, so 437 of its workgroups leave at once."""
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import chunk_split
    assert chunk_split(33600, 7) == (4800, 7) and -(-33600 // 64) == 525 and 4800 // 64 == 75
    _check_rounds(torch, _setup(torch, 2, 4200, 8), 8, {}, [([1, 2], [1, 7])])


EXT4 = {"vf_clip": [10.0, 0.05, 0.0, 0.2], "max_grad_norm": [0.0, 0.03, 0.0, 0.5], "kl_coef": [1.0, 0.0, 0.0, 0.5],
        "kl_target": [1e-4, 0.0, 0.0, 10.0]}     # RLlib's loss; PPO2's; everything off; everything on with a target far above the KL


def test_extended_loss_on_uneven_schedules(torch_cuda):
    """800 samples per member; steps 8 / 1 / 15 / 6 (chunks of 200, 800, 160 and 267, 267, 266).  Each member's coefficient is adapted
    from ITS last epoch's chunks: member 0's mean KL is far above 2 x 1e-4 (x 1.5), member 3's far below 0.5 x 10 (x 0.5).
    (Targets AT the decision's boundaries, which tell the epoch's mean from a wrong sum or divisor: tests/test_kl_adapt_gpu.py.)"""
    torch = torch_cuda
    assert _expected_steps(800, [2, 1, 3, 2], [4, 1, 5, 3]) == [8, 1, 15, 6]
    ppo, refs, st = _check_rounds(torch, _setup(torch, 4, 100, 8), 8, EXT4, [([2, 1, 3, 2], [4, 1, 5, 3])])
    assert ppo.extended() and [r.extended() for r in refs] == [True, True, False, True]
    assert ppo.kl_coef.tolist() == [1.5, 0.0, 0.0, 0.25]
    assert bool((st[0, :8, 4] > 1e-3).all()) and bool((st[1, :1, 5] > 0).all()) and bool((st[3, :6, 5] > 0).all())
    assert bool((st[2, :, 4:] == 0).all())


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_separate_value_network_on_uneven_schedules(torch_cuda, ext):
    torch = torch_cuda
    terms = {k: v[:2] for k, v in EXT4.items()} if ext else {}
    setup = _setup(torch, 2, 77, 8, split=True)
    assert setup[1].separate_value
    ppo, refs, _ = _check_rounds(torch, setup, 8, terms, [([2, 1], [9, 45]), ([1, 3], [1, 9])])
    assert ppo.member_steps == [18 + 1, 44 + 27]


@pytest.mark.parametrize("ext", [False, True], ids=["plain", "ext"])
def test_uniform_schedule_equals_the_common_entry_points(torch_cuda, ext):
    """The list path with equal entries against the int path (ssg_pop_update / ssg_pop_update_ext), two updates each."""
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _setup(torch, 4, 100, 8)
    P, samples = 4, 800
    terms = EXT4 if ext else {}
    saved = pop.params.clone()
    g = torch.Generator(device=DEV).manual_seed(5)
    perms = [_perm(torch, g, P, 2, samples), _perm(torch, g, P, 2, samples)]
    results = []
    try:
        for lists in (False, True):
            pop.params.copy_(saved)
            bb = dict(b)
            ppo = PopulationPPO(pop, env, **_hp(P), **terms)
            ppo.gae(bb)
            sts = []
            for perm, mb in zip(perms, (3, 4)):                                 # chunks of 267, 267, 266; then of 200
                sts.append(ppo.update(bb, perm, [2] * P if lists else 2, [mb] * P if lists else mb, stats=True))
            assert ppo.step == 2 * 3 + 2 * 4 and ppo.member_steps == [14] * P and not ppo.diverged()
            results.append((pop.params.clone(), ppo.adam_mv.clone(), sts, ppo.kl_coef.clone()))
    finally:
        pop.params.copy_(saved)
    (p0, mv0, st0, kl0), (p1, mv1, st1, kl1) = results
    assert not torch.equal(p0, saved)
    assert torch.equal(p0, p1) and torch.equal(mv0, mv1) and torch.equal(kl0, kl1)
    assert all(a.shape == c.shape and torch.equal(a, c) for a, c in zip(st0, st1))
    assert st0[0].shape == (P, 6, 8 if ext else 4)
    if ext:
        assert kl1.tolist() != EXT4["kl_coef"]                                  # the coefficients were adapted


def test_exploit_after_an_uneven_update_takes_the_sources_steps(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env, pop, b, shards, refs, sbs = _setup(torch, 3, 77, 8)
    P, samples = 3, 616
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    hp = _hp(P)
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, **hp)
        ppo.gae(b)
        g = torch.Generator(device=DEV).manual_seed(3)
        ppo.update(b, _perm(torch, g, P, 2, samples), [1, 2, 2], [4, 9, 1])
        assert ppo.member_steps == [4, 18, 2]
        src = [1, 1, 2]                                                         # member 0 <- member 1
        ppo.exploit(src)
        assert ppo.member_steps == [18, 18, 2]
        assert torch.equal(pop.params[0], pop.params[1]) and torch.equal(ppo.adam_mv[0], ppo.adam_mv[1])
        # the references continue from what each member now holds: parameters, moments and Adam step of its source, its OWN constants
        ref_ppos = []
        for m in range(P):
            refs[m].params.copy_(pop.params[m])
            ref = _reference(torch, m, hp, {}, refs, shards, sbs)
            ref.adam_mv.copy_(ppo.adam_mv[m])
            ref.step = ppo.member_steps[m]
            ref_ppos.append(ref)
        perm = _perm(torch, g, P, 2, samples)
        for lists in (True, False):                                             # per-member schedules, then the common entry point
            epochs, mbs = ([2, 1, 1], [2, 3, 9]) if lists else ([2] * P, [3] * P)
            st = ppo.update(b, perm, epochs if lists else 2, mbs if lists else 3, stats=True)
            for m in range(P):
                r_st = ref_ppos[m].update(sbs[m], perm[m, :epochs[m]].contiguous(), epochs[m], mbs[m], stats=True)
                assert torch.equal(pop.params[m], refs[m].params), (lists, m, "params")
                assert torch.equal(ppo.adam_mv[m], ref_ppos[m].adam_mv), (lists, m, "moments")
                assert torch.equal(st[m, :r_st.shape[0]], r_st), (lists, m, "stats")
                assert ppo.member_steps[m] == ref_ppos[m].step
        assert ppo.member_steps == [18 + 4 + 6, 18 + 3 + 6, 2 + 9 + 6] and ppo.step == 28
    finally:
        pop.params.copy_(saved[0])
        for q, p0 in zip(refs, saved[1]):
            q.params.copy_(p0)


def test_update_sched_refuses_bad_arguments(torch_cuda):
    """Through ctypes, one argument wrong at a time: SSG_ERR_BAD_ARG with its message, and nothing is launched."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _setup(torch, 3, 77, 8)
    P, K, samples = 3, 8, 616
    b = dict(b)
    ppo = PopulationPPO(pop, env, vf_clip=[0.2, 0.0, 0.0], kl_coef=[1.0, 0.0, 0.0])
    ppo.gae(b)
    epochs, mbs = [1, 3, 2], [4, 9, 1]
    sched, steps, launches = ppo.pack_schedule(samples, epochs, mbs)
    assert (steps, launches) == ([4, 27, 2], 27)
    ppo._ws(samples, samples)
    table = ppo._table(launches, [0] * P)
    dev_sched = torch.tensor(list(sched), dtype=torch.int32).to(DEV)
    perm = _perm(torch, torch.Generator(device=DEV).manual_seed(1), P, 3, samples)
    ext, ext_table = ppo._ext(b, K, P * 77)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    L, h = N.lib(), env._h
    good = dict(h=h, pop=C.byref(pop.to_native()), ext=None, table=ptr(table), table_steps=launches, sched=ptr(dev_sched),
                epochs=(C.c_int32 * P)(*epochs), mbs=(C.c_int32 * P)(*mbs), perm_epochs=3, K=K, x=ptr(b["obs"]), act=ptr(b["act"]),
                logp=ptr(b["logp"]), adv=ptr(b["adv"]), ret=ptr(b["ret"]), perm=ptr(perm), mv=ptr(ppo.adam_mv), stats=None,
                ws=ptr(ppo.workspace), nbytes=ppo.workspace.numel(), stream=None)
    order = list(good)
    p0, mv0 = pop.params.clone(), ppo.adam_mv.clone()

    def call(**change):
        a = dict(good, **change)
        rc = L.ssg_pop_update_sched(*[a[k] for k in order])
        return rc, L.ssg_last_error(h).decode()

    def bad_ext(**kw):
        e = N.PopExt()
        C.memmove(C.byref(e), C.byref(ext), C.sizeof(N.PopExt))
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(e)

    cases = [
        (dict(epochs=(C.c_int32 * P)(1, 0, 2)), "epochs or minibatches is < 1"),
        (dict(mbs=(C.c_int32 * P)(4, 9, -1)), "epochs or minibatches is < 1"),
        (dict(perm_epochs=2), "perm_epochs < the largest epochs"),
        (dict(table_steps=launches - 1), "fewer Adam steps than the schedule's launches"),
        (dict(epochs=None), "NULL epochs or minibatches"),
        (dict(mbs=None), "NULL epochs or minibatches"),
        (dict(sched=None), "NULL dev_sched"),
        (dict(table=None), "NULL dev_table or dev_adam_mv"),
        (dict(mv=None), "NULL dev_table or dev_adam_mv"),
        (dict(perm=None), "NULL x, act, logp, adv, ret or index buffer"),
        (dict(x=None), "NULL x, act, logp, adv, ret or index buffer"),
        (dict(pop=None), "NULL population"),
        (dict(K=0), "K < 1"),
        (dict(ws=None), "NULL workspace"),
        (dict(nbytes=4096), "this call needs"),
        (dict(ext=bad_ext(struct_size=8)), "ssg_pop_ext.struct_size"),
        (dict(ext=bad_ext(flags=0x8)), "unknown ssg_pop_ext.flags bits"),
        (dict(ext=bad_ext(dev_ext=None)), "NULL dev_ext"),
        (dict(ext=bad_ext(dev_logp_all=None)), "dev_kl_coef without dev_logp_all"),
        (dict(ext=bad_ext(dev_value_old=None)), "SSG_POP_EXT_VF_CLIP without dev_value_old"),
    ]
    for change, text in cases:
        rc, msg = call(**change)
        assert rc == -1 and "ssg_pop_update_sched" in msg and text in msg, (sorted(change), rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(pop.params, p0) and torch.equal(ppo.adam_mv, mv0)          # nothing was launched
    assert ext_table is not None


def test_trainer_mutates_and_exploits_schedules_reproducibly(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/pbt_native.py")
    lines = []
    kw = dict(members=4, envs_per_member=64, horizon=8, updates=4, perturb_every=2, mutate_schedule=True, seed=0, return_details=True)
    hist, det = mod.train(log=lines.append, **kw)
    print("scores: %s" % hist)
    print("schedules: %s %s  member_steps %s" % (det["hparams"]["num_sgd_iter"], det["hparams"]["sgd_minibatch_size"], det["member_steps"]))
    assert len(hist) == 4 and all(len(row) == 4 for row in hist)
    assert all(math.isfinite(s) for s in hist[-1])
    samples = 8 * 64
    logged = [det["hparams"]] + [ev["schedule"] for ev in det["exploits"] if "schedule" in ev]
    for rec in logged:
        its, szs = rec["num_sgd_iter"], rec["sgd_minibatch_size"]
        for it, sz in zip(its if isinstance(its, list) else [its], szs if isinstance(szs, list) else [szs]):
            assert type(it) is int and type(sz) is int and 1 <= it <= 30 and 128 <= sz <= samples, rec
    assert len(det["exploits"]) >= 1 and any("schedule" in ev for ev in det["exploits"])
    assert any("schedule: member" in s for s in lines) and any(s.startswith("schedule: num_sgd_iter") for s in lines)
    assert len(det["member_steps"]) == 4 and min(det["member_steps"]) >= 4
    assert bool(torch.isfinite(det["params"]).all())
    _, again = mod.train(log=lambda s: None, **kw)
    assert torch.equal(det["params"], again["params"]) and det["hparams"] == again["hparams"] and det["member_steps"] == again["member_steps"]
