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

Each figure: 2 warm-up runs, then the median of ``--repeats`` (5) runs, alternating the two paths, each bracketed by a synchronize and
timed with HIP events.  One JSON line on stdout.

    python tools/population_timing.py [--configs 16x4096,120x512] [--horizon 32] [--repeats 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="16x4096,120x512")
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    mod = _ppo()
    res = [measure(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.horizon, a.repeats, "cuda:0") for c in a.configs.split(",")]
    print(json.dumps({"population_timing": res}))


if __name__ == "__main__":
    main()
