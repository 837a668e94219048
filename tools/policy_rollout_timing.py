#!/usr/bin/env python3
"""Rollout step with the policy in the loop: train/ppo_torch.py's `graph` mode (policy in PyTorch, the whole step one HIP graph)
against its `native` mode (ssg_rollout_policy: policy kernel + ssg_step per step, enqueued from C), in one process.

For each env count (65 536 and 4 096; default env: 10 beams, history 2 -> D = 32; ActorCritic hidden 64, 2 layers, 3 actions): both
modes are set up on their own envs and warmed up, then whole rollouts (horizon 64, ppo_torch.rollout() — the same uniforms draw and
buffer conversions the trainer does) are timed with HIP events that end in a synchronize, 5 repeats alternating the two modes;
the median per mode in us per rollout step.  The policy kernel's own time: HIP events around 50 back-to-back ssg_policy_act launches
on preallocated buffers (a launch-bound upper bound where the kernel is shorter than the host call; `rocprofv3 --kernel-trace --stats`
gives the kernel alone, see tools/README.md).  One JSON line on stdout.

    python tools/policy_rollout_timing.py [--envs 65536,4096] [--horizon 64] [--repeats 5] [--separate-value]

--separate-value measures, after each env count's shared-body figures and in the same process, the same things for ActorCritic with a
value network of its own (two 64-64 towers: SSG_POLICY_SEPARATE_VALUE); its results carry "separate_value": true.

    python tools/policy_rollout_timing.py --obs-filter [--beams 8] [--envs 65536,4096] [--horizon 64] [--repeats 7]

--obs-filter measures the observation filter (ship_sim_gym_amd/obs_filter.py) instead: on ONE native env per env count (--beams 8,
history 2 -> D = 28) whole rollouts are timed with nothing bound, with a filter bound and updating, and with it bound frozen, the
three alternating in every repeat; and the filter's two launches alone (50 back-to-back ssg_obs_filter_update calls).  Medians and
every repeat in us per rollout step; the shader clock as rocm-smi reports it before and after (null when it cannot be read).  The
unbound figure of two builds of the library is compared by running this mode alternately with SSG_LIB_PATH set to each.

    python tools/policy_rollout_timing.py --obs-filter-job [--beams 8] [--envs 65536,4096] [--horizon 64] [--repeats 7]

--obs-filter-job measures the job-wide filter (``ObsFilter(job=True)``) instead: on ONE native env per env count whole rollouts are
timed with an updating filter bound and with a job filter bound (its buffer too: the dual finalise kernel), the two alternating in every
repeat; then, alone and back to back, the update's two launches both ways (50 calls) and the rows-merge launch at W = 1, 2 and 8 rows.

    python tools/policy_rollout_timing.py --timeout-bootstrap [--envs 65536,4096] [--horizon 32,64] [--repeats 7]

--timeout-bootstrap measures the time-out bootstrap (ShipVecEnv.set_timeout_bootstrap) instead: on ONE native env per env count (the
default env, D = 32; --horizon lists one rollout length per env count) whole rollouts are timed with nothing bound and with the
record bound, alternating in every repeat (the bound figure includes the one ssg_timeout_values launch, spread over the horizon);
then, alone and back to back, that launch over the horizon's rows with no time-out in the batch ("none"), with every env timing out
on one row ("one_row": the start of training, when every episode runs into the clock together) and with every sample a time-out
("all_rows"), and ssg_ppo_dist over the same number of rows (a forward of every row, to set "all_rows" against).  Medians and every
repeat; rollouts in us per step, launches in us per launch.
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ship_sim_gym_amd import _native as N  # noqa: E402


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


def measure(mod, n, horizon, repeats, dev, separate_value=False):
    torch.manual_seed(0)
    probe = mod.ShipVecEnv(1, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=1)
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    net = mod.ActorCritic(D, A, separate_value=separate_value).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    # graph mode, set up as train() does: reset, one eager warm-up step, reset, capture
    g_shards = mod.make_shards(n, "graph", net, dev, horizon)
    sh = g_shards[0]
    sh.env.reset_tensor()
    sh.step()
    sh.env.reset_tensor()
    sh.t.zero_()
    torch.cuda.synchronize()
    sh.capture(torch.cuda.Stream(device=dev))
    torch.cuda.synchronize()
    # native mode
    n_shards = mod.make_shards(n, "native", net, dev, horizon)
    n_shards[0].env.reset_tensor()
    policy = mod.NativePolicy.from_actor_critic(net, n_shards[0].scale)
    run = {"graph": lambda: mod.rollout(g_shards, horizon, "graph", gen),
           "native": lambda: mod.rollout(n_shards, horizon, "native", gen, policy)}
    for m in ("graph", "native", "graph", "native"):  # warm-up: two rollouts each
        run[m]()
    torch.cuda.synchronize()
    times = {"graph": [], "native": []}
    for _ in range(repeats):
        for m in ("graph", "native"):
            times[m].append(_timed(run[m]) / horizon)
    # the policy kernel alone: back-to-back launches on preallocated buffers
    env = n_shards[0].env
    bufs = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev),
            torch.empty((n, D), device=dev)]
    pol = policy.to_native()
    L, h, st = N.lib(), env._h, env._stream()
    obs, act, logp, val, x = (C.c_void_p(t.data_ptr()) for t in [env.obs] + bufs)

    def launches(k):
        for i in range(k):
            N.check(L.ssg_policy_act(h, C.byref(pol), obs, None, 1, i, act, logp, val, x, st), h, "ssg_policy_act")
    launches(5)
    torch.cuda.synchronize()
    kernel_us = statistics.median(_timed(lambda: launches(50)) / 50 for _ in range(repeats))
    for s in g_shards + n_shards:
        s.graph = None
        s.env.close()
    g = statistics.median(times["graph"])
    nat = statistics.median(times["native"])
    return {"envs": n, "separate_value": bool(separate_value), "obs_dim": D, "hidden": 64, "layers": 2, "n_actions": A, "horizon": horizon,
            "graph_us_per_step": round(g, 2), "native_us_per_step": round(nat, 2), "speedup": round(g / nat, 2),
            "native_env_steps_per_s": round(n / nat * 1e6), "policy_act_us": round(kernel_us, 2),
            "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}}


def _sclk():
    """The shader clock line(s) of `rocm-smi --showclocks` for the first device (read only), or None."""
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
    except Exception:
        return None
    lines = [ln.strip() for ln in out.splitlines() if "sclk" in ln.lower()]
    return lines or None


def measure_filter(mod, n, horizon, repeats, dev, beams):
    from ship_sim_gym_amd.obs_filter import ObsFilter
    torch.manual_seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    probe = mod.ShipVecEnv(1, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=1, n_beams=beams)
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    net = mod.ActorCritic(D, A).to(dev)
    shards = mod.make_shards(n, "native", net, dev, horizon, env_kw={"n_beams": beams})
    env = shards[0].env
    env.reset_tensor()
    policy = mod.NativePolicy.from_actor_critic(net, shards[0].scale)
    flt = ObsFilter(env)
    frozen = flt.frozen()
    bind = {"unbound": None, "updating": flt, "frozen": frozen}

    def run(m):
        env.set_obs_filter(bind[m])
        mod.rollout(shards, horizon, "native", gen, policy)
    clock0 = _sclk()
    for m in ("unbound", "updating", "frozen") * 2:  # warm-up: two rollouts each
        run(m)
    torch.cuda.synchronize()
    times = {m: [] for m in bind}
    for _ in range(repeats):
        for m in bind:
            env.set_obs_filter(bind[m])
            times[m].append(_timed(lambda: mod.rollout(shards, horizon, "native", gen, policy)) / horizon)
    env.set_obs_filter(None)
    rec = flt.to_native()
    L, h, st, obs = N.lib(), env._h, env._stream(), C.c_void_p(env.obs.data_ptr())

    def launches(k):
        for _ in range(k):
            N.check(L.ssg_obs_filter_update(h, C.byref(rec), obs, st), h, "ssg_obs_filter_update")
    launches(5)
    torch.cuda.synchronize()
    update_us = [_timed(lambda: launches(50)) / 50 for _ in range(repeats)]
    clock1 = _sclk()
    env.close()
    med = {m: statistics.median(v) for m, v in times.items()}
    return {"envs": n, "obs_dim": D, "hidden": 64, "layers": 2, "n_actions": A, "horizon": horizon,
            "unbound_us_per_step": round(med["unbound"], 2), "updating_us_per_step": round(med["updating"], 2),
            "frozen_us_per_step": round(med["frozen"], 2), "filter_update_us": round(statistics.median(update_us), 2),
            "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}, "filter_update_repeats_us": [round(t, 2) for t in update_us],
            "sclk_before": clock0, "sclk_after": clock1}


def measure_filter_job(mod, n, horizon, repeats, dev, beams):
    """The job-wide filter's cost: the rollout step with an updating filter bound and its buffer bound too (the dual finalise kernel)
    against the same filter without a buffer, alternating on ONE env; the update's two launches alone, both ways; and the rows-merge
    launch alone at W = 1, 2 and 8 rows (ssg_obs_filter_merge_rows without the copies ObsFilter.merge_rows adds)."""
    from ship_sim_gym_amd.obs_filter import ObsFilter
    torch.manual_seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    probe = mod.ShipVecEnv(1, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=1, n_beams=beams)
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    net = mod.ActorCritic(D, A).to(dev)
    shards = mod.make_shards(n, "native", net, dev, horizon, env_kw={"n_beams": beams})
    env = shards[0].env
    env.reset_tensor()
    policy = mod.NativePolicy.from_actor_critic(net, shards[0].scale)
    bind = {"unbuffered": ObsFilter(env), "buffered": ObsFilter(env, job=True)}
    clock0 = _sclk()
    for m in ("unbuffered", "buffered") * 2:  # warm-up: two rollouts each
        env.set_obs_filter(bind[m])
        mod.rollout(shards, horizon, "native", gen, policy)
    torch.cuda.synchronize()
    times = {m: [] for m in bind}
    for _ in range(repeats):
        for m in bind:
            env.set_obs_filter(bind[m])
            times[m].append(_timed(lambda: mod.rollout(shards, horizon, "native", gen, policy)) / horizon)
    env.set_obs_filter(None)
    L, h, st, obs = N.lib(), env._h, env._stream(), C.c_void_p(env.obs.data_ptr())
    job = bind["buffered"]
    rec, buf = job.to_native(), C.c_void_p(job.buffer.data_ptr())

    def plain(k):
        for _ in range(k):
            N.check(L.ssg_obs_filter_update(h, C.byref(rec), obs, st), h, "ssg_obs_filter_update")

    def dual(k):
        for _ in range(k):
            N.check(L.ssg_obs_filter_update_buffered(h, C.byref(rec), buf, obs, st), h, "ssg_obs_filter_update_buffered")
    update_us = {}
    for name, fn in (("unbuffered", plain), ("buffered", dual)):
        fn(5)
        torch.cuda.synchronize()
        update_us[name] = [_timed(lambda: fn(50)) / 50 for _ in range(repeats)]
    merge_us = {}
    base = C.c_void_p(job.base.data_ptr())
    for W in (1, 2, 8):
        rows = job.buffer.clone()[None].repeat(W, 1, 1, 1).contiguous()

        def merges(k):
            for _ in range(k):
                N.check(L.ssg_obs_filter_merge_rows(h, C.byref(rec), base, C.c_void_p(rows.data_ptr()), W, st), h, "ssg_obs_filter_merge_rows")
        merges(5)
        torch.cuda.synchronize()
        merge_us[W] = [_timed(lambda: merges(50)) / 50 for _ in range(repeats)]
    clock1 = _sclk()
    env.close()
    res = {"envs": n, "obs_dim": D, "hidden": 64, "layers": 2, "n_actions": A, "horizon": horizon,
           "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}, "sclk_before": clock0, "sclk_after": clock1}
    for m in bind:
        res["%s_us_per_step" % m] = round(statistics.median(times[m]), 2)
        res["update_%s_us" % m] = round(statistics.median(update_us[m]), 2)
        res["update_%s_repeats_us" % m] = [round(t, 2) for t in update_us[m]]
    for W, v in merge_us.items():
        res["merge_rows_%d_us" % W] = round(statistics.median(v), 2)
        res["merge_rows_%d_repeats_us" % W] = [round(t, 2) for t in v]
    return res


def measure_timeout(mod, n, horizon, repeats, dev):
    torch.manual_seed(0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    probe = mod.ShipVecEnv(1, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=1)
    D, A = probe.states_history, probe.action_space.n
    probe.close()
    net = mod.ActorCritic(D, A).to(dev)
    shards = mod.make_shards(n, "native", net, dev, horizon)
    env = shards[0].env
    env.reset_tensor()
    policy = mod.NativePolicy.from_actor_critic(net, shards[0].scale)

    def run(bound):
        if bool(env.timeout_bootstrap) != bound:
            env.set_timeout_bootstrap(bound, rows=horizon)
        mod.rollout(shards, horizon, "native", gen, policy)
    clock0 = _sclk()
    for m in (False, True) * 2:  # warm-up: two rollouts each
        run(m)
    torch.cuda.synchronize()
    times = {"unbound": [], "bound": []}
    for _ in range(repeats):
        for name, m in (("unbound", False), ("bound", True)):
            if bool(env.timeout_bootstrap) != m:
                env.set_timeout_bootstrap(m, rows=horizon)
            times[name].append(_timed(lambda: mod.rollout(shards, horizon, "native", gen, policy)) / horizon)
    env.set_timeout_bootstrap(False)
    # the launch alone, on rows of its own: real observations everywhere, so that a forward runs on what a rollout would hand it
    rows = env.obs.unsqueeze(0).expand(horizon, n, D).contiguous()
    out = torch.empty((horizon, n), dtype=torch.float32, device=dev)
    flags = {"none": torch.zeros((horizon, n), dtype=torch.uint8, device=dev), "one_row": torch.zeros((horizon, n), dtype=torch.uint8, device=dev),
             "all_rows": torch.full((horizon, n), N.EV_MAX_STEPS, dtype=torch.uint8, device=dev)}
    flags["one_row"][horizon // 2] = N.EV_MAX_STEPS
    x = torch.zeros((horizon * n, D), dtype=torch.float32, device=dev)
    logp_all = torch.empty((horizon * n, 4), dtype=torch.float32, device=dev)
    pol = policy.to_native()
    L, h, st = N.lib(), env._h, env._stream()

    def dist(k):
        for _ in range(k):
            N.check(L.ssg_ppo_dist(h, C.byref(pol), horizon * n, C.c_void_p(x.data_ptr()), C.c_void_p(logp_all.data_ptr()), st), h, "ssg_ppo_dist")

    def values(f, k):
        for _ in range(k):
            env.timeout_values(policy, f, rows, out=out)
    launch = {}
    for name, f in flags.items():
        values(f, 3)
        torch.cuda.synchronize()
        launch[name] = [_timed(lambda: values(f, 20)) / 20 for _ in range(repeats)]
    dist(3)
    torch.cuda.synchronize()
    launch["ppo_dist"] = [_timed(lambda: dist(20)) / 20 for _ in range(repeats)]
    clock1 = _sclk()
    env.close()
    res = {"envs": n, "obs_dim": D, "hidden": 64, "layers": 2, "n_actions": A, "horizon": horizon,
           "term_obs_bytes": horizon * n * D * 8,
           "unbound_us_per_step": round(statistics.median(times["unbound"]), 2), "bound_us_per_step": round(statistics.median(times["bound"]), 2),
           "repeats_us": {k: [round(t, 2) for t in v] for k, v in times.items()}, "sclk_before": clock0, "sclk_after": clock1}
    for name, v in launch.items():
        res["launch_%s_us" % name] = round(statistics.median(v), 2)
        res["launch_%s_repeats_us" % name] = [round(t, 2) for t in v]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="65536,4096")
    ap.add_argument("--horizon", default="64", help="rollout steps; with --timeout-bootstrap a comma-separated list, one per env count")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--separate-value", action="store_true", help="also measure the separate-value-network shape, in the same process")
    ap.add_argument("--obs-filter", action="store_true", help="measure the observation filter instead (unbound / updating / frozen rollouts)")
    ap.add_argument("--obs-filter-job", action="store_true",
                    help="measure the job-wide filter instead (updating rollouts with and without the buffer bound, the rows merge alone)")
    ap.add_argument("--beams", type=int, default=8, help="lidar beams of the --obs-filter / --obs-filter-job env (8 -> D = 28)")
    ap.add_argument("--timeout-bootstrap", action="store_true",
                    help="measure the time-out bootstrap instead (unbound / bound rollouts, the one launch alone)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    mod = _ppo()
    dev = "cuda:0"
    horizons = [int(x) for x in a.horizon.split(",")]
    a.horizon = horizons[0]
    if a.timeout_bootstrap:
        envs = [int(n) for n in a.envs.split(",")]
        if len(horizons) == 1:
            horizons = horizons * len(envs)
        res = [measure_timeout(mod, n, k, a.repeats, dev) for n, k in zip(envs, horizons)]
        print(json.dumps({"tool": "policy_rollout_timing", "mode": "timeout_bootstrap", "lib": N.LIB_PATH,
                          "device": torch.cuda.get_device_name(0), "results": res}))
        return
    if a.obs_filter_job:
        res = [measure_filter_job(mod, int(n), a.horizon, a.repeats, dev, a.beams) for n in a.envs.split(",")]
        print(json.dumps({"tool": "policy_rollout_timing", "mode": "obs_filter_job", "lib": N.LIB_PATH, "device": torch.cuda.get_device_name(0),
                          "results": res}))
        return
    if a.obs_filter:
        res = [measure_filter(mod, int(n), a.horizon, a.repeats, dev, a.beams) for n in a.envs.split(",")]
        print(json.dumps({"tool": "policy_rollout_timing", "mode": "obs_filter", "lib": N.LIB_PATH, "device": torch.cuda.get_device_name(0),
                          "results": res}))
        return
    res = [measure(mod, int(n), a.horizon, a.repeats, dev, sep) for n in a.envs.split(",") for sep in ([False, True] if a.separate_value else [False])]
    print(json.dumps({"tool": "policy_rollout_timing", "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
