#!/usr/bin/env python3
"""Evaluation step (ssg_evaluate: policy launch + ssg_step + the accounting launch, enqueued from C) against rollout_policy's step
(ssg_rollout_policy: policy launch + ssg_step) at the same env count, in one process.

For each env count (65 536 and 4 096; default env: 10 beams, history 2 -> D = 32; ActorCritic hidden 64, 2 layers, 3 actions): an
evaluation env and a rollout env are set up and warmed up, then calls of `steps` steps are timed with HIP events that end in a
synchronize, `repeats` times alternating rollout, sampled evaluation and greedy evaluation; the median per kind in us per step.  Both
sampled paths draw with Philox (no uniforms buffer), and rollout_policy writes into preallocated buffers.  The quota is set out of reach,
so every env is counted at every step (the accounting launch's most expensive case).  The accounting launch alone (ssg_eval_account)
and the reduction (ssg_eval_reduce): HIP events around 50 back-to-back launches on the evaluator's own buffers — a launch-bound upper
bound where the kernel is shorter than the host call (`rocprofv3 --kernel-trace --stats` gives the kernel alone, see tools/README.md).
One JSON line on stdout.

    python tools/eval_timing.py [--envs 65536,4096] [--steps 64] [--repeats 5]

``--record R [--frame-size WxH]`` times the evaluation recorder (ssg_set_eval_recorder) instead: the greedy evaluation step with
nothing bound, with R tracked envs, and with R tracked envs and WxH frames (default 64x64), alternating in one process
(measure_record).
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

from ship_sim_gym_amd.evaluate import NativeEvaluator  # noqa: E402


def _ppo():
    spec = importlib.util.spec_from_file_location("ppo_torch", os.path.join(ROOT, "train", "ppo_torch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def measure(mod, n, steps, repeats, dev):
    torch.manual_seed(0)
    r_env = mod.ShipVecEnv(n, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    e_env = mod.ShipVecEnv(n, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = r_env.states_history, r_env.action_space.n
    net = mod.ActorCritic(D, A).to(dev)
    scale = torch.full((D,), float(max(r_env.bounds)), dtype=torch.float64, device=dev)
    policy = mod.NativePolicy.from_actor_critic(net, scale)
    r_env.reset_tensor(); e_env.reset_tensor()
    ev = NativeEvaluator(e_env)
    out = {}
    quota = 1 << 30  # out of reach: every env is counted at every step
    step = [0]

    def rollout():
        out["b"] = r_env.rollout_policy(policy, steps, seed=1, step0=step[0], out=out.get("b_full"))
        out.setdefault("b_full", out["b"])

    run = {"rollout": rollout,
           "eval_sampled": lambda: ev.run(policy, quota, steps, greedy=False, seed=1, step0=step[0]),
           "eval_greedy": lambda: ev.run(policy, quota, steps, greedy=True)}
    for _ in range(2):  # warm-up: two calls each
        for k in run:
            run[k]()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    for _ in range(repeats):
        for k in run:
            step[0] += steps
            times[k].append(_timed(run[k]) / steps)
    # the accounting launch and the reduction alone: back-to-back launches on the evaluator's own buffers (the last step's rows)
    account_us = statistics.median(_timed(lambda: [ev.account(quota, ev.reward, ev.done, ev.flags) for _ in range(50)]) / 50 for _ in range(repeats))
    reduce_us = statistics.median(_timed(lambda: [ev.reduce(1) for _ in range(50)]) / 50 for _ in range(repeats))
    med = {k: statistics.median(v) for k, v in times.items()}
    r_env.close(); e_env.close()
    return {"envs": n, "obs_dim": D, "hidden": 64, "layers": 2, "n_actions": A, "steps": steps,
            "rollout_us_per_step": round(med["rollout"], 2), "eval_sampled_us_per_step": round(med["eval_sampled"], 2),
            "eval_greedy_us_per_step": round(med["eval_greedy"], 2),
            "eval_sampled_minus_rollout_us": round(med["eval_sampled"] - med["rollout"], 2),
            "eval_greedy_minus_rollout_us": round(med["eval_greedy"] - med["rollout"], 2),
            "eval_account_us": round(account_us, 2), "eval_reduce_us": round(reduce_us, 2),
            "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}}


def measure_record(mod, n, steps, repeats, dev, R, size):
    """The greedy evaluation step with nothing bound, with R tracked envs (evenly spaced over the handle) and with R tracked envs
    and frames of `size`, alternating, on ONE env; the capacity is the call's step count and the cursors are zeroed ahead of every
    call (outside the timed region), so every slot writes a row — and a frame, S = 1 — at every step: the recorder's most expensive
    case.  Median us per step per case and every repeat."""
    from ship_sim_gym_amd.evaluate import EvalRecorder
    torch.manual_seed(0)
    env = mod.ShipVecEnv(n, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    net = mod.ActorCritic(D, A).to(dev)
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    policy = mod.NativePolicy.from_actor_critic(net, scale)
    env.reset_tensor()
    ev = NativeEvaluator(env)
    ids = [i * n // R for i in range(R)]
    recorders = {"nothing_bound": None, "tracked": EvalRecorder(env, ids, steps), "tracked_frames": EvalRecorder(env, ids, steps, frames=size)}
    quota = 1 << 30

    def call(rec):
        if rec is not None:
            rec.reset()
        torch.cuda.synchronize()
        return _timed(lambda: ev.run(policy, quota, steps, greedy=True, recorder=rec)) / steps

    for _ in range(2):
        for rec in recorders.values():
            call(rec)
    times = {k: [] for k in recorders}
    for _ in range(repeats):
        for k, rec in recorders.items():
            times[k].append(call(rec))
    assert all(int(c) == steps for k in ("tracked", "tracked_frames") for c in recorders[k].steps)  # every slot wrote every step
    med = {k: statistics.median(v) for k, v in times.items()}
    env.close()
    return {"envs": n, "obs_dim": D, "steps": steps, "tracked": R, "frame_size": list(size),
            "nothing_bound_us_per_step": round(med["nothing_bound"], 2), "tracked_us_per_step": round(med["tracked"], 2),
            "tracked_frames_us_per_step": round(med["tracked_frames"], 2),
            "tracked_minus_nothing_us": round(med["tracked"] - med["nothing_bound"], 2),
            "frames_minus_tracked_us": round(med["tracked_frames"] - med["tracked"], 2),
            "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="65536,4096")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--record", type=int, default=0, metavar="R",
                    help="time the evaluation step with nothing bound, with R tracked envs and with R tracked envs and frames instead")
    ap.add_argument("--frame-size", default="64x64", metavar="WxH", help="of --record's frames")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    mod = _ppo()
    if a.record:
        size = tuple(int(t) for t in a.frame_size.lower().split("x"))
        res = [measure_record(mod, int(n), a.steps, a.repeats, "cuda:0", a.record, size) for n in a.envs.split(",")]
        print(json.dumps({"tool": "eval_timing --record", "device": torch.cuda.get_device_name(0), "results": res}))
        return
    res = [measure(mod, int(n), a.steps, a.repeats, "cuda:0") for n in a.envs.split(",")]
    print(json.dumps({"tool": "eval_timing", "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
