"""Hyper-parameter schedules on the device trainers (ship_sim_gym_amd/hparam_schedule.py; NativePPO / PopulationPPO / DataParallelPPO
``set_timesteps``; train/ppo_torch.py --lr-schedule / --clip-schedule / --ent-schedule): a scheduled run is bit for bit the run whose
constants were set by hand before every update.

Every comparison is torch.equal, or == on Python values: a schedule is evaluated on the host and written into the fields every update
call already passes, so there is no tolerance anywhere.  The expected values are the module's expression restated here (_expr).
Shapes: hidden 16, 4 beams and history 2 (D = 20), K = 4; a step limit of 11 for the trainer script's runs, as
tests/test_checkpoint_gpu.py sets it, so that episodes end on both sides of a save point."""
import pytest

from gpu_support import DEV, env_config, load_script, torch_cuda  # noqa: F401
from population_harness import cached, member_hparams, perms_per_member, shard_reference, shard_rollouts, stacked_perms
from population_harness import close_cached  # noqa: F401
from ppo_reference import actor_critic_policy
from ship_sim_gym_amd.hparam_schedule import HparamSchedule

pytestmark = pytest.mark.gpu

BEAMS, D, HIDDEN, K, MAX_STEPS = 4, 20, 16, 4, 11
QUIET = lambda *a, **k: None  # noqa: E731


def _expr(points, t):
    """v_i + ((t - t_i) / (t_{i+1} - t_i)) * (v_{i+1} - v_i), the last value from the last point on: evaluated in the test."""
    if t >= points[-1][0]:
        return float(points[-1][1])
    for (t0, v0), (t1, v1) in zip(points, points[1:]):
        if t0 <= t < t1:
            return v0 + ((t - t0) / (t1 - t0)) * (v1 - v0)
    raise AssertionError(t)


def _env(n, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    env = ShipVecEnv(n, n_maps=8, n_beams=BEAMS, env_config=env_config(2), env_id_base=base)
    assert env.states_history == D
    return env


def _policy(torch, seed=3):
    return actor_critic_policy(torch, D, HIDDEN, 2, "tanh", 3, seed=seed)[1]


def _clone(batch):
    return {k: v.clone() for k, v in batch.items()}


def _perms(torch, g, rows, n):
    return torch.stack([torch.randperm(n, device=DEV, generator=g) for _ in range(rows)])


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. NativePPO on a schedule against its twin
# ------------------------------------------------------------------------------------------------------------------------------------
N1 = 128
POINTS = {"lr": [(0, 1e-3), (3 * K * N1, 0.0)],                           # PPO2's decay to 0 over the 3 updates
          "clip": [(0, 0.2), (700, 0.1), (3 * K * N1, 0.05)],              # three points: update 1 on the first segment, update 2 on the second
          "ent_coef": [(0, 0.01), (2 * K * N1, 0.0)]}                      # ends at update 2's clock exactly: the stop value


@pytest.mark.parametrize("case", ["plain", "grad_clip"])
def test_native_ppo_on_schedules_is_its_twin_with_constants_set_by_hand(torch_cuda, case):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    ext = dict(max_grad_norm=0.5) if case == "grad_clip" else {}
    env = _env(N1)
    env.reset_tensor()
    pols = [_policy(torch), _policy(torch)]
    sched = NativePPO(pols[0], env, **{k: HparamSchedule(p) for k, p in POINTS.items()}, **ext)
    twin = NativePPO(pols[1], env, lr=POINTS["lr"][0][1], clip=POINTS["clip"][0][1], ent_coef=POINTS["ent_coef"][0][1], **ext)
    assert sched.extended() == (case == "grad_clip") and sched.timesteps == 0
    assert all(getattr(sched.hp, k) == POINTS[k][0][1] for k in POINTS)       # until set_timesteps: the values at 0
    g = torch.Generator(device=DEV).manual_seed(5)
    seen = []
    for u in range(3):
        t = u * K * N1
        want = {k: _expr(p, t) for k, p in POINTS.items()}
        seen.append(want)
        b0 = dict(env.rollout_policy(pols[0], K, seed=21, step0=K * u))
        b1 = _clone(b0)
        perm = _perms(torch, g, 2, K * N1)
        mv, ws = sched.adam_mv.clone(), sched.workspace.clone()
        assert sched.set_timesteps(t) is sched and sched.timesteps == t
        assert torch.equal(sched.adam_mv, mv) and torch.equal(sched.workspace, ws)   # (host only)
        twin.hp.lr, twin.hp.clip, twin.hp.ent_coef = want["lr"], want["clip"], want["ent_coef"]
        assert all(getattr(sched.hp, k) == want[k] for k in want), (u, want)
        out = []
        for ppo, b in ((sched, b0), (twin, b1)):
            ppo.gae(b)
            st = ppo.update(b, perm, 2, 2, stats=True)
            out.append((st, ppo.report(b, stats=st)))
        (s0, r0), (s1, r1) = out
        assert s0.shape == (4, 8 if ext else 4) and torch.equal(s0, s1), u
        assert torch.equal(pols[0].params, pols[1].params) and torch.equal(sched.adam_mv, twin.adam_mv), u
        assert r0["lr"] == r1["lr"] == want["lr"] and r0["clip"] == r1["clip"] == want["clip"], (u, r0["lr"], r0["clip"])
        assert r0 == r1
    # the schedules were in use: three different learning rates and clips, the entropy coefficient at its stop value at last
    assert len({w["lr"] for w in seen}) == 3 and len({w["clip"] for w in seen}) == 3 and seen[2]["ent_coef"] == 0.0 and seen[2]["lr"] > 0.0
    assert seen[1]["clip"] == 0.2 + ((512 - 0) / (700 - 0)) * (0.1 - 0.2) and seen[2]["clip"] == 0.1 + ((1024 - 700) / (1536 - 700)) * (0.05 - 0.1)
    sd = sched.state_dict()
    assert sd["schedules"] == {k: [list(p) for p in POINTS[k]] for k in POINTS} and sd["timesteps"] == 2 * K * N1
    assert twin.state_dict()["schedules"] == {"lr": [], "clip": [], "ent_coef": []} and twin.state_dict()["timesteps"] == 0
    assert sd["hp"] == twin.state_dict()["hp"]
    # refusals: a clip schedule that reaches 0, at construction; a clock that is no int >= 0
    with pytest.raises(ValueError, match=r"clip schedule's points\[1\]"):
        NativePPO(pols[0], env, clip=HparamSchedule([(0, 0.2), (64, 0.0)]))
    with pytest.raises(ValueError, match="int >= 0"):
        sched.set_timesteps(-1)
    assert sched.timesteps == 2 * K * N1
    env.close()


def test_constant_schedules_are_the_floats_and_no_schedule_only_records_the_clock(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    env = _env(N1)
    env.reset_tensor()
    vals = dict(lr=7e-4, clip=0.15, ent_coef=0.003)
    pols = [_policy(torch), _policy(torch)]
    const = NativePPO(pols[0], env, **{k: HparamSchedule.constant(v) for k, v in vals.items()})
    plain = NativePPO(pols[1], env, **vals)
    g = torch.Generator(device=DEV).manual_seed(6)
    for u in range(2):
        b0 = dict(env.rollout_policy(pols[0], K, seed=22, step0=K * u))
        b1 = _clone(b0)
        perm = _perms(torch, g, 2, K * N1)
        hp_before = {k: getattr(plain.hp, k) for k in vals}
        for ppo, b in ((const, b0), (plain, b1)):
            ppo.set_timesteps(u * K * N1 + 17)
            ppo.gae(b)
            ppo.update(b, perm, 2, 2)
        assert {k: getattr(plain.hp, k) for k in vals} == hp_before == vals and plain.timesteps == const.timesteps == u * K * N1 + 17
        assert all(getattr(const.hp, k) == vals[k] for k in vals)
        assert torch.equal(pols[0].params, pols[1].params) and torch.equal(const.adam_mv, plain.adam_mv), u
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the population: every member against NativePPO(member) on its shard with the same schedule
# ------------------------------------------------------------------------------------------------------------------------------------
def _pop_setup(torch, sizes):
    def make_env(n, base):
        env = _env(n, base)
        if n == sum(sizes) and len(set(sizes)) > 1:                         # the population's handle, on unequal slices
            env.set_population_slices(list(sizes))
        return env
    return cached(tuple(sizes), lambda: shard_rollouts(torch, make_env, lambda d: [_policy(torch, seed=100 + m) for m in range(len(sizes))],
                                                       sizes, K, 7))


def _pop_hparams(sizes, updates=2):
    """lrs 1e-3, 1e-4, 1e-5 as the reference sweeps them, members 0 and 1 each decaying to 0 over their OWN run; member 1's clip and
    member 0's entropy coefficient scheduled; the last member all floats."""
    P = len(sizes)
    lrs = [1e-3, 1e-4, 1e-5][:P]
    hp = member_hparams(P)
    points = {"lr": [[(0, lrs[m]), (updates * K * sizes[m], 0.0)] if m < P - 1 else None for m in range(P)],
              "clip": [[(0, 0.2), (K * sizes[1] // 2, 0.12), (3 * K * sizes[1], 0.1)] if m == 1 else None for m in range(P)],
              "ent_coef": [[(0, 0.01), (K * sizes[0], 0.002)] if m == 0 else None for m in range(P)]}
    const = {"lr": lrs, "clip": hp["clip"], "ent_coef": hp["ent_coef"]}
    for k, pts in points.items():
        hp[k] = [HparamSchedule(p) if p is not None else const[k][m] for m, p in enumerate(pts)]
    return hp, points, const


@pytest.mark.parametrize("sizes", [(64, 64, 64), (64, 128)], ids=["equal", "unequal"])
def test_population_members_follow_their_own_schedules_and_clocks(torch_cuda, sizes):
    torch = torch_cuda
    from ship_sim_gym_amd.population import PopulationPPO
    env, pop, b, shards, refs, sbs = _pop_setup(torch, sizes)
    P = len(sizes)
    b, sbs = dict(b), [dict(sb) for sb in sbs]
    hp, points, const = _pop_hparams(sizes)
    saved = pop.params.clone(), [r.params.clone() for r in refs]
    try:
        ppo = PopulationPPO(pop, env, **hp)
        assert ppo.member_envs == list(sizes)
        for k in points:                                                    # lists of P floats, the values at 0
            assert getattr(ppo, k) == [pts[0][1] if pts is not None else const[k][m] for m, pts in enumerate(points[k])]
            assert [s is not None for s in ppo.schedules[k]] == [pts is not None for pts in points[k]]
        ppo.gae(b)
        ref_ppos = [shard_reference(torch, m, hp, {}, refs, shards, sbs) for m in range(P)]
        g = torch.Generator(device=DEV).manual_seed(11)
        samples = [K * n for n in sizes]
        for u in range(2):
            clocks = [u * s for s in samples]                               # members have clocks of their own
            want = {k: [_expr(pts, clocks[m]) if pts is not None else const[k][m] for m, pts in enumerate(points[k])] for k in points}
            ppo.set_timesteps(clocks if len(set(sizes)) > 1 else (clocks if u else 0))   # (an int serves every member)
            assert ppo.timesteps == clocks and all(getattr(ppo, k) == want[k] for k in want), (u, want)
            perm = perms_per_member(torch, g, 2, samples) if len(set(sizes)) > 1 else stacked_perms(torch, g, P, 2, samples[0])
            st = ppo.update(b, perm, 2, 2, stats=True)
            rec = ppo.report(b, stats=st)
            assert rec["lr"].tolist() == want["lr"] and rec["clip"].tolist() == want["clip"]
            for m, ref in enumerate(ref_ppos):
                ref.set_timesteps(clocks[m])
                assert (ref.hp.lr, ref.hp.clip, ref.hp.ent_coef) == (want["lr"][m], want["clip"][m], want["ent_coef"][m])
                rst = ref.update(sbs[m], perm[m], 2, 2, stats=True)
                assert torch.equal(st[m], rst), (u, m)
                assert torch.equal(pop.params[m], refs[m].params) and torch.equal(ppo.adam_mv[m], ref.adam_mv), (u, m)
        assert want["lr"][0] == const["lr"][0] + ((samples[0]) / (2 * samples[0])) * (0.0 - const["lr"][0]) and want["lr"][-1] == const["lr"][-1]
        sd = ppo.state_dict()
        assert sd["timesteps"] == clocks and sd["schedules"] == {k: [[list(p) for p in pts] if pts is not None else [] for pts in points[k]] for k in points}
        if P == 3:
            # an assignment to a scheduled member lasts until the next set_timesteps; clear_schedule makes the value a constant
            ppo.lr[0], ppo.lr[2] = 0.5, 0.25
            ppo.set_timesteps(clocks)
            assert ppo.lr == [want["lr"][0], want["lr"][1], 0.25]
            ppo.lr[2] = const["lr"][2]
            # exploit leaves the schedules and the clocks where they are
            before = {k: list(v) for k, v in ppo.schedules.items()}
            params1 = pop.params[1].clone()
            ppo.exploit([1, 1, 2])
            assert torch.equal(pop.params[0], params1)
            assert all(a is c for k in before for a, c in zip(before[k], ppo.schedules[k])) and ppo.timesteps == clocks
            nxt = [2 * s for s in samples]
            ppo.set_timesteps(nxt)
            for k in points:
                assert getattr(ppo, k) == [_expr(pts, nxt[m]) if pts is not None else const[k][m] for m, pts in enumerate(points[k])], k
            ppo.clear_schedule("clip", 1)
            held = ppo.clip[1]
            ppo.set_timesteps([3 * s for s in samples])
            assert ppo.clip[1] == held and ppo.schedules["clip"][1] is None and ppo.lr[0] == 0.0
            with pytest.raises(ValueError, match="vf_clip"):
                ppo.clear_schedule("vf_clip", 0)
            with pytest.raises(ValueError, match="2 clocks for 3 members"):
                ppo.set_timesteps([0, 0])
            # the state round-trips through a fresh trainer; a malformed entry names its field and member
            fresh = PopulationPPO(pop, env)
            fresh.load_state_dict(ppo.state_dict())
            assert fresh.schedules == ppo.schedules and fresh.timesteps == ppo.timesteps and fresh.lr == ppo.lr and fresh.clip == ppo.clip
            bad = ppo.state_dict()
            bad["schedules"]["clip"][2] = [[0, 0.2], [5, 0.0]]
            with pytest.raises(ValueError, match=r"member 2: schedules\['clip'\]"):
                PopulationPPO(pop, env).load_state_dict(bad)
            old = {k: v for k, v in ppo.state_dict().items() if k not in ("schedules", "timesteps")}
            fresh.load_state_dict(old)
            assert fresh.schedules == {k: [None] * 3 for k in points} and fresh.timesteps == [0, 0, 0] and fresh.lr == ppo.lr
        with pytest.raises(ValueError, match=r"member 1: the clip schedule's points\[1\]"):
            PopulationPPO(pop, env, clip=[0.2, HparamSchedule([(0, 0.2), (9, -0.1)])] + [0.2] * (P - 2))
    finally:
        pop.params.copy_(saved[0])
        for r, p in zip(refs, saved[1]):
            r.params.copy_(p)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. data parallel: the clock is the job's
# ------------------------------------------------------------------------------------------------------------------------------------
def test_one_rank_data_parallel_on_schedules_is_native_ppo(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.dp import DataParallelPPO
    from ship_sim_gym_amd.ppo import NativePPO
    env = _env(N1)
    env.reset_tensor()
    pols = [_policy(torch), _policy(torch)]
    kw = {k: HparamSchedule(p) for k, p in POINTS.items()}
    tr = [NativePPO(pols[0], env, perm_seed=11, **kw), DataParallelPPO(pols[1], env, perm_seed=11, **kw)]
    assert (tr[1].rank, tr[1].world, tr[1].member) == (0, 1, 0)
    for u in range(3):
        b0 = dict(env.rollout_policy(pols[0], K, seed=21, step0=K * u))
        out = []
        for t, b in zip(tr, (b0, _clone(b0))):
            t.set_timesteps(u * K * N1)
            t.gae(b)
            out.append(t.update(b, None, 2, 2, stats=True))
        assert tr[0].hp.lr == tr[1].hp.lr == _expr(POINTS["lr"], u * K * N1) and tr[0].hp.clip == tr[1].hp.clip == _expr(POINTS["clip"], u * K * N1)
        assert torch.equal(out[0], out[1]) and torch.equal(pols[0].params, pols[1].params) and torch.equal(tr[0].adam_mv, tr[1].adam_mv), u
    sd = tr[1].state_dict()
    assert sd["timesteps"] == 2 * K * N1 and sd["schedules"]["lr"] == [list(p) for p in POINTS["lr"]]
    fresh = DataParallelPPO(_policy(torch), env).load_state_dict(sd)
    assert fresh.schedules == tr[1].schedules and fresh.timesteps == tr[1].timesteps and fresh.hp.lr == tr[1].hp.lr
    env.close()


SHARDS = (128, 64)  # unequal: each shard's own count is a clock of its own, and both differ from the job's


def test_two_shards_replayed_stay_identical_on_the_jobs_clock(torch_cuda):
    """A two-shard job replayed in one process, one replica per shard (local_row / apply_rows, torch.stack as the gather): with the job's
    timestep count on both replicas their parameters stay bit-identical; with each replica's own shard count they do not, and neither
    is the job's result: the clock is the job's."""
    torch = torch_cuda
    from ship_sim_gym_amd.dp import DataParallelPPO, chunk_counts, shard_chunks
    from ship_sim_gym_amd.ppo import NativePPO
    envs = [_env(SHARDS[0], 0), _env(SHARDS[1], SHARDS[0])]
    for env in envs:
        env.reset_tensor()
    acting = _policy(torch)
    batches = [dict(env.rollout_policy(acting, K, seed=9)) for env in envs]
    total, epochs, minibatches, updates = sum(SHARDS), 2, 2, 2
    points = {"lr": [(0, 1e-3), (updates * K * total, 0.0)], "clip": [(0, 0.2), (K * total, 0.1)]}
    g = torch.Generator(device=DEV).manual_seed(4)
    perms = [[_perms(torch, g, epochs, K * n) for n in SHARDS] for _ in range(updates)]
    sc = shard_chunks(K, SHARDS, minibatches)
    n_chunks = sc[0][1]
    assert all(c == n_chunks for _, c in sc)

    def replay(clock):
        """clock(u, r): the timesteps replica r sets before update u.  Returns the replicas' parameters and the learning rates they used."""
        pols = [_policy(torch), _policy(torch)]
        trs = [DataParallelPPO(pol, env, member=r, **{k: HparamSchedule(p) for k, p in points.items()}) for r, (pol, env) in enumerate(zip(pols, envs))]
        lrs = []
        for u in range(updates):
            bs = [dict(b) for b in batches]
            for r, tr in enumerate(trs):
                tr.set_timesteps(clock(u, r))
            lrs.append([tr.hp.lr for tr in trs])
            moments = []
            for tr, b in zip(trs, bs):
                NativePPO.gae(tr, b)
                moments.append(tr.shard_moments(b))
            for tr in trs:
                tr.set_moments(torch.stack(moments))
            for e in range(epochs):
                for j in range(n_chunks):
                    rows = torch.stack([tr.local_row(b, perms[u][r][e, j * sc[r][0]: min(K * SHARDS[r], (j + 1) * sc[r][0])])
                                        for r, (tr, b) in enumerate(zip(trs, bs))])
                    for tr in trs:
                        tr.apply_rows(rows, chunk_counts(K, SHARDS, minibatches, j), j == 0, e == epochs - 1 and j == n_chunks - 1)
            for tr in trs:
                tr.updates += 1
        return [pol.params.clone() for pol in pols], lrs

    job, job_lrs = replay(lambda u, r: u * K * total)
    assert torch.equal(job[0], job[1]) and bool(torch.isfinite(job[0]).all()) and not torch.equal(job[0], acting.params)
    assert job_lrs == [[_expr(points["lr"], u * K * total)] * 2 for u in range(updates)] and job_lrs[1][0] == 1e-3 + ((K * total) / (updates * K * total)) * (0.0 - 1e-3)
    own, own_lrs = replay(lambda u, r: u * K * SHARDS[r])
    assert own_lrs[0] == job_lrs[0] and own_lrs[1] == [_expr(points["lr"], K * n) for n in SHARDS] and len(set(own_lrs[1] + job_lrs[1])) == 3
    assert not torch.equal(own[0], own[1])                                   # the replicas drift apart
    assert not torch.equal(own[0], job[0]) and not torch.equal(own[1], job[0])
    for env in envs:
        env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. train/ppo_torch.py: a resumed run, and 5. the torch update follows
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def short_episodes():
    """MAX_STEPS = 11 for the trainer script's envs (they read the config class), as tests/test_checkpoint_gpu.py sets it."""
    from ship_sim_gym_amd.config import EnvConfig
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(EnvConfig, "MAX_STEPS", MAX_STEPS)
        yield


ENVS, HORIZON = 128, 4
RUN = dict(envs=ENVS, horizon=HORIZON, hidden=HIDDEN, env_kw={"n_beams": BEAMS}, seed=3, return_details=True, log=QUIET,
           lr_schedule="linear:0", clip_schedule="0:0.2,1024:0.1", total_timesteps=4 * ENVS * HORIZON)  # the span: the 4-update run's own length
LR_POINTS, CLIP_POINTS = [(0, 3e-4), (4 * ENVS * HORIZON, 0.0)], [(0, 0.2), (1024, 0.1)]


def _same(a, b):
    import torch
    if torch.is_tensor(a) or torch.is_tensor(b):
        return torch.is_tensor(a) and torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu())
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_a_scheduled_run_resumed_is_the_uninterrupted_run(torch_cuda, short_episodes, tmp_path):
    torch = torch_cuda
    from ship_sim_gym_amd import checkpoint
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.ppo import NativePPO
    from ship_sim_gym_amd.report import read_progress
    mod = load_script("train/ppo_torch.py")
    kw = dict(RUN, mode="native", update="native")
    p = {k: str(tmp_path / k) for k in ("full.ckpt", "half.ckpt", "resumed.ckpt", "full.csv", "resumed.csv")}
    lines = []
    _, d_full = mod.train(updates=4, save=p["full.ckpt"], progress=p["full.csv"], **dict(kw, log=lambda *a: lines.append(" ".join(str(x) for x in a))))
    mod.train(updates=2, save=p["half.ckpt"], progress=p["resumed.csv"], **kw)            # saved after update 1 ...
    _, d_res = mod.train(updates=4, resume=p["half.ckpt"], save=p["resumed.ckpt"], progress=p["resumed.csv"], **kw)   # ... and resumed
    assert len(d_full["params"]) == len(d_res["params"]) and all(torch.equal(a, c) for a, c in zip(d_full["params"], d_res["params"]))
    full, half, res = (checkpoint.load(p[k]) for k in ("full.ckpt", "half.ckpt", "resumed.ckpt"))
    assert _same(res["trainer"], full["trainer"]) and _same(res["policy"], full["policy"]) and _same(res["loop"], full["loop"])
    clocks = [u * ENVS * HORIZON for u in range(4)]
    want_lr, want_clip = [_expr(LR_POINTS, t) for t in clocks], [_expr(CLIP_POINTS, t) for t in clocks]
    assert full["trainer"]["schedules"] == {"lr": [list(q) for q in LR_POINTS], "clip": [list(q) for q in CLIP_POINTS], "ent_coef": []}
    assert (half["trainer"]["timesteps"], full["trainer"]["timesteps"]) == (clocks[1], clocks[3])
    assert (full["trainer"]["hp"]["lr"], full["trainer"]["hp"]["clip"], full["trainer"]["hp"]["ent_coef"]) == (want_lr[3], want_clip[3], 0.01)
    assert full["config"]["lr_schedule"] == "linear:0" and full["config"]["clip_schedule"] == "0:0.2,1024:0.1" and full["config"]["ent_schedule"] == "None"
    # the --progress columns now vary, and a resumed run reproduces them like the others, apart from t
    prog_full, prog_res = read_progress(p["full.csv"]), read_progress(p["resumed.csv"])
    assert prog_full["lr"].tolist() == prog_res["lr"].tolist() == want_lr and prog_full["clip"].tolist() == prog_res["clip"].tolist() == want_clip
    assert len(set(want_lr)) == 4 and want_clip[2:] == [0.1, 0.1] and want_clip[1] == 0.2 + ((512 - 0) / (1024 - 0)) * (0.1 - 0.2)
    assert all(prog_full[c].tolist() == prog_res[c].tolist() for c in prog_full if c != "t")
    # an update's log line names the current values; the span is logged once
    assert sum("hyper-parameter schedule of lr" in ln for ln in lines) == 1 and sum("hyper-parameter schedules at" in ln for ln in lines) == 4
    assert any("at 512 timesteps: lr %.6g  clip %.6g" % (want_lr[1], want_clip[1]) in ln for ln in lines)
    # the specs are the run's configuration: another one is refused with both values
    with pytest.raises(ValueError, match=r"lr_schedule \(the file has 'linear:0', this run 'linear:1e-5'\)"):
        mod.train(updates=4, resume=p["half.ckpt"], **dict(kw, lr_schedule="linear:1e-5"))
    # a trainer section from before there were schedules (the two keys deleted) loads as a constant run; a malformed entry is refused
    env = _env(8)
    pol = NativePolicy.from_state_dict(half["policy"], DEV)
    old = {k: v for k, v in half["trainer"].items() if k not in ("schedules", "timesteps")}
    ppo = NativePPO(pol, env, lr=HparamSchedule.linear(1.0, 0.5, 10)).load_state_dict(old)
    assert ppo.schedules == {"lr": None, "clip": None, "ent_coef": None} and ppo.timesteps == 0
    assert (ppo.hp.lr, ppo.hp.clip, ppo.step) == (want_lr[1], want_clip[1], half["trainer"]["step"])
    ppo.set_timesteps(4096)
    assert (ppo.hp.lr, ppo.hp.clip) == (want_lr[1], want_clip[1])
    ppo = NativePPO(pol, env).load_state_dict(half["trainer"])
    assert ppo.schedules["lr"] == HparamSchedule(LR_POINTS) and ppo.timesteps == clocks[1]
    mv = ppo.adam_mv.clone()
    bad = dict(half["trainer"], adam_mv=torch.zeros_like(half["trainer"]["adam_mv"]), schedules=dict(half["trainer"]["schedules"], clip=[[0, 0.2], [0, 0.1]]))
    with pytest.raises(ValueError, match=r"schedules\['clip'\]"):
        ppo.load_state_dict(bad)
    assert torch.equal(ppo.adam_mv, mv) and ppo.schedules["clip"] == HparamSchedule(CLIP_POINTS)   # (raised before anything was copied)
    env.close()


def test_the_torch_update_follows_the_schedules(torch_cuda, short_episodes, monkeypatch):
    import inspect
    mod = load_script("train/ppo_torch.py")
    inner, seen = mod.torch_update, []
    params = list(inspect.signature(inner).parameters)

    def recording(*args, **kwargs):
        bound = dict(zip(params, args), **kwargs)
        seen.append((bound["opt"].param_groups[0]["lr"], bound["clip"], bound["ent_coef"], len(bound["opt"].param_groups)))
        return inner(*args, **kwargs)
    monkeypatch.setattr(mod, "torch_update", recording)
    mod.train(updates=2, mode="eager", update="torch", **dict(RUN, ent_schedule="0:0.01,512:0.004"))
    clocks = [0, ENVS * HORIZON]
    assert seen == [(_expr(LR_POINTS, t), _expr(CLIP_POINTS, t), _expr([(0, 0.01), (512, 0.004)], t), 1) for t in clocks]
    assert seen[1][:3] == (3e-4 + ((512) / (2048)) * (0.0 - 3e-4), 0.2 + ((512) / (1024)) * (0.1 - 0.2), 0.004)
