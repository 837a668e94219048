#!/usr/bin/env python3
"""A population sharing its launches against what the single-policy path offers, in one process and one run.

For each (members x envs per member) — default 16x4096 and 120x512; default env (D = 32), ActorCritic hidden 64, 2 layers, 3 actions;
K = 32 rollout steps, 2 epochs x 4 minibatches — on one handle of members * envs envs:

(a) the rollout step: ``rollout_population`` (one policy launch per step for all members) against ``rollout_policy`` with ONE policy
    on the same handle (the same launches with one parameter row), both K steps from a fresh reset with the same uniforms; microseconds
    per step.  ``single_step_spread`` is (max - min) / median over the single-policy repeats: the population figure is expected
    within it (the work per workgroup is identical).
(b) GAE + update: ``PopulationPPO.gae`` + ``.update`` against a loop over the members of ``NativePPO.gae`` + ``.update`` on each
    member's own slice of the same batch (contiguous copies made beforehand) — what training the members one after another costs;
    milliseconds per update of the whole population.  Both start every repeat from the same parameters and zero moments and use the
    same pre-drawn permutations (drawing them is not timed).

With ``--sched`` (per-member schedules, ssg_pop_update_sched), instead, per configuration:

(c) a UNIFORM schedule (2 epochs x 4 minibatches for everyone) through the per-member entry (lists) against the common entry
    (``ssg_pop_update``, the code path that existed before per-member schedules: the yardstick), update only, alternating in the same
    run; ``uniform_spread`` is (max - min) / median over the common entry's repeats.
(d) a SKEWED schedule — epochs 1..4 cycling over the members, minibatches cycling over 1, 4, 16 — through the per-member entry
    against a loop of the members' ``NativePPO.update`` with the same schedules.

With ``--slices`` (per-member batch sizes: unequal env slices, ssg_pop_set_slices), instead, per configuration, on ONE handle whose
layout is re-bound between the runs (binding is not timed):

(e) EQUAL slices bound against nothing bound: the rollout step, and GAE + update (bound: the schedule path, which a sliced update
    always takes; unbound: the common entry, whose code the slices do not touch: the yardstick).  ``*_spread`` is (max - min) / median
    over the unbound path's repeats.
(f) a SKEWED layout — batch shares cycling 1 : 2 : 4 : 8 over the members through ``slices_for_batch_sizes`` (quantum 64) — against
    the equal layout at the same N: the rollout step; and its GAE + update against a loop of the members' ``NativePPO.gae`` +
    ``.update`` on shards of those sizes.

With ``--adv-norm`` (per-minibatch advantage normalisation, ssg_ppo_set_adv_norm), instead, per configuration:

(g) GAE + update of the population with ``adv_norm="minibatch"`` against the same with ``adv_norm="batch"`` (the yardstick: the code
    path that existed before), two PopulationPPO objects on one handle, alternating; ``batch_spread`` is (max - min) / median over
    the batch-mode repeats.

With ``--perm`` (the minibatch permutations drawn by the library, ssg_pop_perm), instead, per configuration and for perm_epochs 2 and 30
(the rows a trainer draws per member: the epochs, or --max-epochs of train/pbt_native.py --mutate-schedule):

(h) the draw alone — torch's (``torch.rand((P, perm_epochs, samples)).argsort(-1)``, what the trainers and the figures above use)
    against ``PopulationPPO.draw_perm`` (one launch into a fresh tensor) — with each draw's peak device memory above what was
    allocated before it (torch's allocator statistics; the result included); and GAE + update (2 epochs x 4 minibatches, reading the
    first 2 rows) with each draw of all perm_epochs rows INSIDE the timed region, all four alternating.

With ``--report`` (the update report, ssg_pop_report), instead, per configuration:

(i) ``PopulationPPO.report_device`` alone without and with the post-update group (two launches; one ssg_pop_dist launch more), GAE alone
    (the yardstick) and GAE + update without and with a report (no post group; the update then writes its stats rows) behind it, all
    alternating; ``update_spread`` is (max - min) / median over the plain GAE + update's repeats.

Each figure: 2 warm-up runs, then the median of ``--repeats`` (5) runs, alternating the two paths, each bracketed by a synchronize and
timed with HIP events.  One JSON line on stdout.

    python tools/population_timing.py [--configs 16x4096,120x512] [--horizon 32] [--repeats 5] [--sched | --slices | --adv-norm | --perm | --report]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _ppo():
    spec = importlib.util.spec_from_file_location("ppo_torch", os.path.join(ROOT, "train", "ppo_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)  # ms


def _alternate(paths, repeats, before=None):
    times = {k: [] for k, _ in paths}
    for i in range(2 + repeats):
        for k, f in paths:
            if before:
                before(k)
            t = _timed(f)
            if i >= 2:
                times[k].append(t)
    return times


def measure(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4):
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    nets = [mod.ActorCritic(D, A).to(dev) for _ in range(P)]
    pop = NativePopulation.from_actor_critics(nets, scale)
    seq = NativePopulation.from_actor_critics(nets, scale)       # the sequential loop's own copy of the same parameters
    single = NativePolicy.from_actor_critic(nets[0], scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    U = torch.rand((horizon, N), generator=gen, device=dev)
    out = {}

    # (a) the rollout step
    bufs = {}

    def roll_pop():
        bufs["pop"] = env.rollout_population(pop, horizon, uniforms=U, out=bufs.get("pop"))

    def roll_single():
        bufs["single"] = env.rollout_policy(single, horizon, uniforms=U, out=bufs.get("single"))

    t = _alternate([("single", roll_single), ("pop", roll_pop)], repeats, before=lambda k: env.reset_tensor())
    for k in ("single", "pop"):
        out[k + "_step_us"] = statistics.median(t[k]) * 1e3 / horizon
        out[k + "_step_us_all"] = [round(x * 1e3 / horizon, 2) for x in t[k]]
    out["single_step_spread"] = (max(t["single"]) - min(t["single"])) / statistics.median(t["single"])
    out["pop_step_over_single"] = out["pop_step_us"] / out["single_step_us"]

    # (b) GAE + update
    env.reset_tensor()
    b = dict(env.rollout_population(pop, horizon, uniforms=U))
    samples = horizon * n
    perm = torch.rand((P, epochs, samples), generator=gen, device=dev).argsort(dim=-1)
    ppo = PopulationPPO(pop, env)
    slices = [{k: (v[:, m * n:(m + 1) * n] if k != "last_val" else v[m * n:(m + 1) * n]).contiguous() for k, v in b.items()}
              for m in range(P)]
    seq_ppos = [NativePPO(seq.member(m), env) for m in range(P)]

    def restore(k):
        if k == "pop":
            pop.params.copy_(p0)
            ppo.adam_mv.zero_()
            ppo.step = 0
        else:
            seq.params.copy_(p0)
            for q in seq_ppos:
                q.adam_mv.zero_()
                q.step = 0

    def upd_pop():
        nb = dict(b)
        ppo.gae(nb)
        ppo.update(nb, perm, epochs, minibatches)

    def upd_seq():
        for m in range(P):
            nb = dict(slices[m])
            seq_ppos[m].gae(nb)
            seq_ppos[m].update(nb, perm[m], epochs, minibatches)

    t = _alternate([("seq", upd_seq), ("pop", upd_pop)], repeats, before=restore)
    same = bool(torch.equal(pop.params, seq.params))             # both paths computed the same update, bit for bit
    for k in ("seq", "pop"):
        out[k + "_update_ms"] = statistics.median(t[k])
        out[k + "_update_ms_all"] = [round(x, 3) for x in t[k]]
    out["update_speedup"] = out["seq_update_ms"] / out["pop_update_ms"]
    out["updates_bitwise_equal"] = same
    env.close()
    out.update({"members": P, "envs_per_member": n, "horizon": horizon, "epochs": epochs, "minibatches": minibatches,
                "samples_per_minibatch": -(-samples // minibatches)})
    return out


def measure_sched(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4):
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    nets = [mod.ActorCritic(D, A).to(dev) for _ in range(P)]
    pop = NativePopulation.from_actor_critics(nets, scale)
    seq = NativePopulation.from_actor_critics(nets, scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    U = torch.rand((horizon, N), generator=gen, device=dev)
    env.reset_tensor()
    b = dict(env.rollout_population(pop, horizon, uniforms=U))
    samples = horizon * n
    sk_epochs = [1 + m % 4 for m in range(P)]
    sk_mbs = [(1, 4, 16)[m % 3] for m in range(P)]
    perm = torch.rand((P, max(sk_epochs), samples), generator=gen, device=dev).argsort(dim=-1)
    perm_u = perm[:, :epochs].contiguous()
    ppo = PopulationPPO(pop, env)
    ppo.gae(b)
    slices = [{k: (v[:, m * n:(m + 1) * n] if k != "last_val" else v[m * n:(m + 1) * n]).contiguous() for k, v in b.items()}
              for m in range(P)]
    seq_ppos = [NativePPO(seq.member(m), env) for m in range(P)]
    for m in range(P):
        seq_ppos[m].gae(slices[m])
    perm_m = [perm[m, :sk_epochs[m]].contiguous() for m in range(P)]
    finals = {}

    def restore(k):
        if k == "seq":
            seq.params.copy_(p0)
            for q in seq_ppos:
                q.adam_mv.zero_()
                q.step = 0
        else:
            pop.params.copy_(p0)
            ppo.adam_mv.zero_()
            ppo.step, ppo.member_steps = 0, [0] * P

    def common():
        ppo.update(b, perm_u, epochs, minibatches)
        finals["common"] = pop.params.clone()

    def lists():
        ppo.update(b, perm_u, [epochs] * P, [minibatches] * P)
        finals["lists"] = pop.params.clone()

    def skew_pop():
        ppo.update(b, perm, sk_epochs, sk_mbs)
        finals["skew_pop"] = pop.params.clone()

    def skew_seq():
        for m in range(P):
            seq_ppos[m].update(slices[m], perm_m[m], sk_epochs[m], sk_mbs[m])
        finals["seq"] = seq.params.clone()

    out = {"members": P, "envs_per_member": n, "horizon": horizon, "uniform_epochs": epochs, "uniform_minibatches": minibatches,
           "skew_epochs": "1..4 cycling", "skew_minibatches": "1, 4, 16 cycling"}
    t = _alternate([("common", common), ("lists", lists)], repeats, before=restore)
    for k in ("common", "lists"):
        out["uniform_%s_ms" % k] = statistics.median(t[k])
        out["uniform_%s_ms_all" % k] = [round(x, 3) for x in t[k]]
    out["uniform_spread"] = (max(t["common"]) - min(t["common"])) / statistics.median(t["common"])
    out["uniform_lists_over_common"] = out["uniform_lists_ms"] / out["uniform_common_ms"]
    out["uniform_bitwise_equal"] = bool(torch.equal(finals["common"], finals["lists"]))
    t = _alternate([("seq", skew_seq), ("skew_pop", skew_pop)], repeats, before=restore)
    out["skew_seq_ms"], out["skew_pop_ms"] = statistics.median(t["seq"]), statistics.median(t["skew_pop"])
    out["skew_seq_ms_all"], out["skew_pop_ms_all"] = [round(x, 3) for x in t["seq"]], [round(x, 3) for x in t["skew_pop"]]
    out["skew_speedup"] = out["skew_seq_ms"] / out["skew_pop_ms"]
    out["skew_bitwise_equal"] = bool(torch.equal(finals["seq"], finals["skew_pop"]))
    env.close()
    return out


def measure_slices(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4):
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO, slices_for_batch_sizes
    from ship_sim_gym_amd.ppo import NativePPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    nets = [mod.ActorCritic(D, A).to(dev) for _ in range(P)]
    pop = NativePopulation.from_actor_critics(nets, scale)
    seq = NativePopulation.from_actor_critics(nets, scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    U = torch.rand((horizon, N), generator=gen, device=dev)
    skew = slices_for_batch_sizes([(1, 2, 4, 8)[m % 4] for m in range(P)], N, 64)
    offs = [sum(skew[:m]) for m in range(P)]
    layouts = {"unbound": None, "equal": [n] * P, "skew": skew}
    out = {"members": P, "envs": N, "horizon": horizon, "epochs": epochs, "minibatches": minibatches, "skew_shares": "1, 2, 4, 8 cycling",
           "skew_min_envs": min(skew), "skew_max_envs": max(skew)}

    # the rollout step under the three layouts
    bufs = {}

    def bind(k):
        env.set_population_slices(layouts[k])
        env.reset_tensor()

    def roll(k):
        def f():
            bufs[k] = env.rollout_population(pop, horizon, uniforms=U, out=bufs.get(k))
        return f

    t = _alternate([(k, roll(k)) for k in layouts], repeats, before=bind)
    for k in layouts:
        out[k + "_step_us"] = statistics.median(t[k]) * 1e3 / horizon
        out[k + "_step_us_all"] = [round(x * 1e3 / horizon, 2) for x in t[k]]
    out["step_spread"] = (max(t["unbound"]) - min(t["unbound"])) / statistics.median(t["unbound"])
    out["equal_step_over_unbound"] = out["equal_step_us"] / out["unbound_step_us"]
    out["skew_step_over_equal"] = out["skew_step_us"] / out["equal_step_us"]
    out["equal_rollout_bitwise_equal"] = all(bool(torch.equal(bufs["unbound"][k], bufs["equal"][k])) for k in bufs["unbound"])

    # GAE + update: equal slices bound against nothing bound
    ppo = PopulationPPO(pop, env)
    samples = horizon * n
    perm = torch.rand((P, epochs, samples), generator=gen, device=dev).argsort(dim=-1)
    perm_list = [perm[m] for m in range(P)]
    b_eq = {k: v.clone() for k, v in bufs["unbound"].items()}
    finals = {}

    def restore(k):
        env.set_population_slices(layouts[k])
        pop.params.copy_(p0)
        ppo.adam_mv.zero_()
        ppo.step, ppo.member_steps = 0, [0] * P

    def upd(k):
        def f():
            nb = dict(b_eq)
            ppo.gae(nb)
            ppo.update(nb, perm_list if k == "equal" else perm, epochs, minibatches)
            finals[k] = pop.params.clone()
        return f

    t = _alternate([(k, upd(k)) for k in ("unbound", "equal")], repeats, before=restore)
    for k in ("unbound", "equal"):
        out[k + "_update_ms"] = statistics.median(t[k])
        out[k + "_update_ms_all"] = [round(x, 3) for x in t[k]]
    out["update_spread"] = (max(t["unbound"]) - min(t["unbound"])) / statistics.median(t["unbound"])
    out["equal_update_over_unbound"] = out["equal_update_ms"] / out["unbound_update_ms"]
    out["equal_update_bitwise_equal"] = bool(torch.equal(finals["unbound"], finals["equal"]))

    # GAE + update on the skewed layout against a loop over shards of those sizes
    b_sk = {k: v.clone() for k, v in bufs["skew"].items()}
    perm_sk = [torch.rand((epochs, horizon * s), generator=gen, device=dev).argsort(dim=-1) for s in skew]
    shards = [{k: (v[:, o:o + s] if k != "last_val" else v[o:o + s]).contiguous() for k, v in b_sk.items()} for o, s in zip(offs, skew)]
    seq_ppos = [NativePPO(seq.member(m), env) for m in range(P)]

    def restore_sk(k):
        if k == "skew_pop":
            restore("skew")
        else:
            seq.params.copy_(p0)
            for q in seq_ppos:
                q.adam_mv.zero_()
                q.step = 0

    def skew_pop():
        nb = dict(b_sk)
        ppo.gae(nb)
        ppo.update(nb, perm_sk, epochs, minibatches)
        finals["skew_pop"] = pop.params.clone()

    def skew_seq():
        for m in range(P):
            nb = dict(shards[m])
            seq_ppos[m].gae(nb)
            seq_ppos[m].update(nb, perm_sk[m], epochs, minibatches)
        finals["skew_seq"] = seq.params.clone()

    t = _alternate([("skew_seq", skew_seq), ("skew_pop", skew_pop)], repeats, before=restore_sk)
    for k in ("skew_seq", "skew_pop"):
        out[k + "_update_ms"] = statistics.median(t[k])
        out[k + "_update_ms_all"] = [round(x, 3) for x in t[k]]
    out["skew_update_speedup"] = out["skew_seq_update_ms"] / out["skew_pop_update_ms"]
    out["skew_update_bitwise_equal"] = bool(torch.equal(finals["skew_seq"], finals["skew_pop"]))
    env.set_population_slices(None)
    env.close()
    return out


def measure_adv_norm(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4):
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    pop = NativePopulation.from_actor_critics([mod.ActorCritic(D, A).to(dev) for _ in range(P)], scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    env.reset_tensor()
    b = dict(env.rollout_population(pop, horizon, uniforms=torch.rand((horizon, N), generator=gen, device=dev)))
    samples = horizon * n
    perm = torch.rand((P, epochs, samples), generator=gen, device=dev).argsort(dim=-1)
    ppos = {"batch": PopulationPPO(pop, env), "minibatch": PopulationPPO(pop, env, adv_norm="minibatch")}  # (each call binds its own mode)

    def restore(k):
        pop.params.copy_(p0)
        ppos[k].adam_mv.zero_()
        ppos[k].step = 0
        ppos[k].member_steps = [0] * P

    def upd(k):
        def run():
            nb = dict(b)
            ppos[k].gae(nb)
            ppos[k].update(nb, perm, epochs, minibatches)
        return run

    t = _alternate([("batch", upd("batch")), ("minibatch", upd("minibatch"))], repeats, before=restore)
    out = {}
    for k in ("batch", "minibatch"):
        out[k + "_update_ms"] = statistics.median(t[k])
        out[k + "_update_ms_all"] = [round(x, 3) for x in t[k]]
    out["batch_spread"] = (max(t["batch"]) - min(t["batch"])) / statistics.median(t["batch"])
    out["minibatch_over_batch"] = out["minibatch_update_ms"] / out["batch_update_ms"]
    env.close()
    out.update({"members": P, "envs_per_member": n, "horizon": horizon, "epochs": epochs, "minibatches": minibatches,
                "samples_per_minibatch": -(-samples // minibatches)})
    return out


def measure_report(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4):
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    pop = NativePopulation.from_actor_critics([mod.ActorCritic(D, A).to(dev) for _ in range(P)], scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    env.reset_tensor()
    b = dict(env.rollout_population(pop, horizon, uniforms=torch.rand((horizon, N), generator=gen, device=dev)))
    samples = horizon * n
    perm = torch.rand((P, epochs, samples), generator=gen, device=dev).argsort(dim=-1)
    ppo = PopulationPPO(pop, env)
    nb_r = dict(b)
    ppo.gae(nb_r)
    st_r = torch.randn((P, epochs * minibatches, 4), device=dev)

    def restore(k):
        pop.params.copy_(p0)
        ppo.adam_mv.zero_()
        ppo.step = 0
        ppo.member_steps = [0] * P

    def upd(with_report):
        def run():
            nb = dict(b)
            ppo.gae(nb)
            st = ppo.update(nb, perm, epochs, minibatches, stats=with_report)
            if with_report:
                ppo.report_device(nb, stats=st)
        return run

    t = _alternate([("report", lambda: ppo.report_device(nb_r, stats=st_r)), ("report_post", lambda: ppo.report_device(nb_r, stats=st_r, post=True)),
                    ("gae", lambda: ppo.gae(dict(b))), ("update", upd(False)), ("update_report", upd(True))], repeats, before=restore)
    out = {"members": P, "envs_per_member": n, "horizon": horizon, "epochs": epochs, "minibatches": minibatches}
    for k, v in t.items():
        out[k + "_ms"] = statistics.median(v)
        out[k + "_ms_all"] = [round(x, 4) for x in v]
    out["update_spread"] = (max(t["update"]) - min(t["update"])) / statistics.median(t["update"])
    env.close()
    return out


def _peak_bytes(fn):
    """Peak device memory during fn() above what was allocated before it (the result included)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def measure_perm(mod, members, n, horizon, repeats, dev, epochs=2, minibatches=4, perm_epochs_list=(2, 30)):
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    torch.manual_seed(0)
    P, N = members, members * n
    env = mod.ShipVecEnv(N, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    pop = NativePopulation.from_actor_critics([mod.ActorCritic(D, A).to(dev) for _ in range(P)], scale)
    p0 = pop.params.clone()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    env.reset_tensor()
    b = dict(env.rollout_population(pop, horizon, uniforms=torch.rand((horizon, N), generator=gen, device=dev)))
    samples = horizon * n
    ppo = PopulationPPO(pop, env, perm_seed=1)
    out = {"members": P, "envs_per_member": n, "horizon": horizon, "epochs": epochs, "minibatches": minibatches, "by_perm_epochs": []}

    def restore(k):
        pop.params.copy_(p0)
        ppo.adam_mv.zero_()
        ppo.step = 0
        ppo.member_steps = [0] * P

    for E in perm_epochs_list:
        def draw_torch():
            return torch.rand((P, E, samples), generator=gen, device=dev).argsort(dim=-1)

        def draw_native():
            return ppo.draw_perm(horizon, E)

        def upd(draw):
            def run():
                nb = dict(b)
                ppo.gae(nb)
                ppo.update(nb, draw()[:, :epochs].contiguous(), epochs, minibatches)
            return run

        t = _alternate([("draw_torch", draw_torch), ("draw_native", draw_native), ("update_torch_draw", upd(draw_torch)),
                        ("update_native_draw", upd(draw_native))], repeats, before=restore)
        rec = {"perm_epochs": E, "indices": P * E * samples}
        for k, v in t.items():
            rec[k + "_ms"] = statistics.median(v)
            rec[k + "_ms_all"] = [round(x, 4) for x in v]
        rec["draw_torch_peak_bytes"], rec["draw_native_peak_bytes"] = _peak_bytes(draw_torch), _peak_bytes(draw_native)
        out["by_perm_epochs"].append(rec)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="16x4096,120x512")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sched", action="store_true", help="time per-member schedules (ssg_pop_update_sched) instead")
    ap.add_argument("--slices", action="store_true", help="time unequal env slices (ssg_pop_set_slices) instead")
    ap.add_argument("--adv-norm", action="store_true", help="time per-minibatch advantage normalisation against batch mode instead")
    ap.add_argument("--perm", action="store_true", help="time the permutation draws (torch's against the library's) and GAE + update with each instead")
    ap.add_argument("--report", action="store_true", help="time the update report alone, GAE alone and GAE + update with and without a report instead")
    a = ap.parse_args()
    mod = _ppo()
    if a.report:
        res = [measure_report(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
        print(json.dumps({"population_report_timing": res}))
        return
    if a.perm:
        res = [measure_perm(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
        print(json.dumps({"population_perm_timing": res}))
        return
    if a.adv_norm:
        res = [measure_adv_norm(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
        print(json.dumps({"population_adv_norm_timing": res}))
        return
    if a.slices:
        res = [measure_slices(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
        print(json.dumps({"population_slices_timing": res}))
        return
    if a.sched:
        res = [measure_sched(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
        print(json.dumps({"population_sched_timing": res}))
        return
    res = [measure(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
    print(json.dumps({"population_timing": res}))


if __name__ == "__main__":
    main()
