#!/usr/bin/env python3
"""GAE + PPO update after one rollout: train/ppo_torch.py's torch update (the GAE loop, autograd, torch.optim.Adam) against the native
one (NativePPO: ssg_ppo_gae + ssg_ppo_update, ship_sim_gym_amd/ppo.py), in one process, on the same native rollout batch.

For each (envs, horizon) — default 65 536 x 32 and 4 096 x 64; default env (D = 32), ActorCritic hidden 64, 2 layers, 3 actions;
2 epochs x 4 minibatches — one rollout_policy batch is collected, then each path runs 2 warm-up updates and `--repeats` timed ones
(alternating), each bracketed by a synchronize and timed with HIP events; the median per path in ms per update.  Both paths start
every update from the same parameters' values (their own copies) and draw their permutations from generators seeded alike.  One JSON
line on stdout.  The kernels alone: `rocprofv3 --kernel-trace --stats -- python tools/ppo_update_timing.py --only native` (tools/README.md).

    python tools/ppo_update_timing.py [--configs 65536x32,4096x64] [--repeats 7] [--only torch|native] [--ext] [--separate-value] [--ret-filter]
                                      [--adv-norm] [--perm] [--timeout-bootstrap] [--checkpoint] [--dp] [--episode-log] [--report]
                                      [--ret-filter-job] [--report-job] [--episode-log-job] [--adv-norm-job]

--ext adds, in the same run, the extended update (NativePPO with vf_clip 0.2, max_grad_norm 0.5, kl_coef 1.0, kl_target 0.01: GAE, the
ssg_ppo_dist launch, ssg_ppo_update_ext) as the path "native_ext", and the ssg_ppo_dist launch alone as "dist".
--separate-value measures, after each configuration's shared-body figures and in the same process, the same paths for ActorCritic with
a value network of its own (two 64-64 towers: SSG_POLICY_SEPARATE_VALUE); its results carry "separate_value": true.
--ret-filter adds, in the same run and alternating with the others, return normalisation (ship_sim_gym_amd/ret_filter.py): "gae" (ssg_ppo_gae
alone), "ret_gae" (ssg_ret_filter_apply updating, then GAE on its output), "ret_frozen" (the frozen apply alone: one launch), "ret_apply"
(the updating apply alone: three launches) and "native_ret" (the whole GAE + update with the filter, to set against "native").
--adv-norm adds, in the same run and alternating with the others, "native_mbnorm": the whole GAE + update of a NativePPO with
adv_norm="minibatch" (two more launches ahead of every minibatch's gradient launch), to set against "native" (batch mode).
--perm adds, in the same run and alternating with the others: "perm_torch" (the draw "native" makes inside its timed region, alone:
torch.randperm per epoch, stacked), "perm_native" (NativePPO.draw_perm alone: ssg_ppo_perm, one launch into a fresh tensor) and
"native_permnative" (the whole GAE + update with update(perm=None), the library drawing), to set against "native"; and each draw's
peak device memory above what was allocated before it (torch's allocator statistics; the result tensor included), in bytes.
--timeout-bootstrap adds, in the same run and alternating with the others: "gae_plain" (ssg_ppo_gae alone) and "gae_boot"
(ssg_ppo_gae_boot alone, on the same batch plus a "boot" buffer that holds a value at a tenth of the samples and marks them done).
--checkpoint adds, in the same run and alternating with the others, "checkpoint_save": one ship_sim_gym_amd/checkpoint.py save of what
train/ppo_torch.py --save writes between two updates (the policy, the trainer, the env's snapshot, an observation and a return filter, a
loop section), host wall-clock milliseconds from the first state_dict() to the renamed file (device-to-host copies, pickling and the
file system; the path is under --checkpoint-dir, default the system's temporary directory), to set against "native", the GAE + update
of the same process; and the file's size in bytes.  What --save-every 1 costs per update is the first against the second.
--dp adds, in the same run and alternating with the others, "native_dp": the whole GAE + update through DataParallelPPO
(ship_sim_gym_amd/dp.py) on ONE rank, to set against "native" — what leaving the C loop costs: a Python iteration per minibatch, a
gather that is a no-op, the moments launches and the apply launch in place of the reduction; and "apply_rows_w1" / "_w2" / "_w8":
ssg_ppo_apply_shards alone on 1, 2 and 8 gathered rows (the plain loss: one launch).
--episode-log adds, in the same run and alternating with the others: "eplog_append" (EpisodeLog.append alone: ssg_episode_log_append, three
launches), "episode_stats" (ssg_pop_episode_stats alone with one member: the closest existing walk, one launch), "gae_alone" (ssg_ppo_gae
alone) and "native_eplog" (the append, then the whole GAE + update), to set against "native".
--report adds, in the same run and alternating with the others: "report" (NativePPO.report_device alone without the post-update group:
ssg_ppo_report, two launches, with the stats rows of an update), "report_post" (the same with the post-update group: one ssg_ppo_dist
launch more), "gae_only" (ssg_ppo_gae alone, the yardstick) and "native_report" (the whole GAE + update with stats rows, then the report
without the post group), to set against "native".
--ret-filter-job adds, in the same run and alternating with the others, the job-wide return filter (``ReturnFilter(job=True)``) on one
device: "ret_apply_plain" (ssg_ret_filter_apply updating: three launches) against "ret_apply_split" (the split call at W = 1: shard_rows,
a gather that is a no-op, apply_rows: four launches); "ret_apply_rows_w1" / "_w2" / "_w8" (apply_rows alone on 1, 2 and 8 stacked
rows: two launches); and the whole GAE + update with each filter, "native_ret_plain" and "native_ret_job".  With this flag every timed
path follows one untimed GAE over the batch, so that all have the same predecessor.  The gather over real links is not part of
any of them.
--report-job adds, in the same run and alternating with the others, the job's update report on one device: "report_device"
(NativePPO.report_device with the stats rows of an update: ssg_ppo_report, two launches) against "report_split" (the split call at W = 1:
report_row, then report_rows on its one row: three launches); "report_rows_w1" / "_w2" / "_w8" (report_rows alone on 1, 2 and 8 stacked
rows: one launch); and the whole GAE + update with each report behind it, one copy to the host included, "native_report_own"
(NativePPO.report) and "native_report_job" (NativePPO.job_report, whose gather is a no-op here).  Every timed path follows one untimed
GAE, as with --ret-filter-job.  The gather over real links is not part of any of them.
--episode-log-job adds, in the same run and alternating with the others, the job-wide episode log (``EpisodeLog(job=True)``) on one
device, capacity 65 536, rows = the horizon: "eplog_plain" (EpisodeLog.append: ssg_episode_log_append, three launches) against
"eplog_split" (the split call at W = 1: shard_block, a gather that is a no-op, merge_blocks: six launches); "eplog_merge_w1" / "_w2" /
"_w8" (merge_blocks alone on 1, 2 and 8 stacked copies of this device's block: two launches); and the whole GAE + update with each log
ahead of it, "native_eplog_plain" and "native_eplog_job"; and the block's size in bytes.  Every timed path follows one untimed GAE, as
with --ret-filter-job.  The gather over real links is not part of any of them.
--adv-norm-job adds, in the same run and alternating with the others, the job-wide per-minibatch advantage normalisation
(``DataParallelPPO(job_adv_norm="minibatch")``) on one rank: the whole GAE + update of that trainer, "native_dp_mbjob" (the sums' two
launches, a gather that is a no-op and the rows launch once per update, then a host-side select per minibatch), against the same
trainer in batch mode, "native_dp_batch", and against "native_mbnorm_single" (NativePPO with adv_norm="minibatch": two launches ahead
of every minibatch's gradient launch, inside the C loop); "mb_sums" (shard_minibatch_sums alone: ssg_ppo_minibatch_adv_sums, two
launches) and "mb_rows_w1" / "_w2" / "_w8" (ssg_ppo_set_minibatch_adv_rows and the binding alone on 1, 2 and 8 stacked blocks: one
launch).  Every timed path follows one untimed GAE, as with --ret-filter-job.  The gather over real links is not part of any of them.
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


def _wall_ms(fn):
    """Host wall-clock milliseconds of fn() between two synchronizes (for work that is mostly on the host)."""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(mod, envs, horizon, repeats, only, dev, epochs=2, minibatches=4, ext=False, separate_value=False, ret_filter=False,
            adv_norm=False, perm=False, timeout_bootstrap=False, checkpoint=False, checkpoint_dir=None, dp=False, episode_log=False,
            report=False, ret_filter_job=False, report_job=False, episode_log_job=False, adv_norm_job=False):
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.ppo import NativePPO
    torch.manual_seed(0)
    env = mod.ShipVecEnv(envs, mod.GameConfig, mod.EnvConfig, device=dev, n_maps=64)
    D, A = env.states_history, env.action_space.n
    net = mod.ActorCritic(D, A, separate_value=separate_value).to(dev)
    scale = torch.full((D,), float(max(env.bounds)), dtype=torch.float64, device=dev)
    env.reset_tensor()
    pol_roll = NativePolicy.from_actor_critic(net, scale)
    b = dict(env.rollout_policy(pol_roll, horizon, seed=1))
    p0 = [p.detach().clone() for p in net.parameters()]
    # the torch path trains `net`; the native path a second module's packed parameters
    net_n = mod.ActorCritic(D, A, separate_value=separate_value).to(dev)
    pol = NativePolicy.from_actor_critic(net_n, scale)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    ppo = NativePPO(pol, env)
    n = horizon * envs

    def seeded():
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        return g
    g_t, g_n, g_p = seeded(), seeded(), seeded()

    def run_torch():
        with torch.no_grad():
            for p, q in zip(net.parameters(), p0):
                p.copy_(q)
        # train/ppo_torch.py's update, as it runs after a native rollout (rew / done / act converted as rollout() does, inside the timing)
        mod.torch_update(net, opt, dict(b, rew=b["rew"].float(), done=b["done"].float(), act=b["act"].long()), b["last_val"], epochs,
                         minibatches, g_t)

    def native_path(trainer, gen, before=None, after=None, **gae_kw):
        """The whole GAE + update of `trainer` from the start parameters, its permutations drawn from gen (None: by the library)."""
        def run():
            with torch.no_grad():
                for p, q in zip(net_n.parameters(), p0):
                    p.copy_(q)
            pol.refresh()
            if before is not None:
                before()
            nb = dict(b)
            trainer.gae(nb, **gae_kw)
            rows = None if gen is None else torch.stack([torch.randperm(n, device=dev, generator=gen) for _ in range(epochs)])
            if after is None:
                trainer.update(nb, rows, epochs, minibatches)
            else:
                after(nb, trainer.update(nb, rows, epochs, minibatches, stats=True))
        return run

    from ship_sim_gym_amd.ret_filter import ReturnFilter
    rflt, rfrozen = ReturnFilter(env), ReturnFilter(env, update=False)
    ppo_x = NativePPO(pol, env, vf_clip=0.2, max_grad_norm=0.5, kl_coef=1.0, kl_target=0.01)
    ppo_m = NativePPO(pol, env, adv_norm="minibatch") if adv_norm else None  # (every call binds its object's own mode on the env)
    ppo_p = NativePPO(pol, env, perm_seed=1) if perm else None
    run_native, run_native_ret = native_path(ppo, g_n), native_path(ppo, seeded(), return_filter=rflt)
    run_native_ext = native_path(ppo_x, seeded(), before=lambda: ppo_x.kl_coef.fill_(1.0))
    run_native_mbnorm, run_native_permnative = native_path(ppo_m, seeded()), native_path(ppo_p, None)

    run_dist = lambda: ppo_x.dist(dict(b))  # noqa: E731
    draw_torch = lambda: torch.stack([torch.randperm(n, device=dev, generator=g_p) for _ in range(epochs)])  # noqa: E731
    draw_native = lambda: ppo_p.draw_perm(n, epochs)  # noqa: E731

    if dp:  # one rank of a data-parallel job: the Python loop, a gather that is a no-op, and the apply launch in place of the reduction
        from ship_sim_gym_amd.dp import DataParallelPPO
        ppo_d = DataParallelPPO(pol, env)
        run_native_dp = native_path(ppo_d, seeded())

        def apply_alone(W):
            rows = torch.randn((W, ppo_d.n_params + 8), device=dev) * 1e-3
            counts = [-(-n // minibatches)] * W
            return lambda: ppo_d.apply_rows(rows, counts, True, False)

    ckpt_path = None
    if checkpoint:
        import tempfile
        from ship_sim_gym_amd import checkpoint as ckpt_mod
        from ship_sim_gym_amd.obs_filter import ObsFilter
        oflt = ObsFilter(env)  # (not bound: its state is saved, whatever it holds)
        ckpt_path = os.path.join(checkpoint_dir or tempfile.gettempdir(), "ppo_update_timing_%d_%dx%d.ckpt" % (os.getpid(), envs, horizon))
        g_c = torch.Generator(device=dev)
        g_c.manual_seed(1)

        def run_checkpoint_save():
            ckpt_mod.save(ckpt_path, {"policy": pol.state_dict(), "trainer": ppo.state_dict(), "env": env.snapshot(),
                                      "obs_filter": oflt.state_dict(), "ret_filter": rflt.state_dict(),
                                      "loop": {"update": 0, "gen_state": g_c.get_state().cpu().clone(), "history": [], "best": float("-inf")},
                                      "config": {"envs": envs, "horizon": horizon}})

    paths = [(k, f) for k, f in (("torch", run_torch), ("native", run_native)) if only in (None, k)]
    if episode_log:  # the append reads the rollout's own rows; the carries and the ring keep running from call to call, as in training
        import ctypes as C
        from ship_sim_gym_amd import _native as N
        from ship_sim_gym_amd.episode_log import EpisodeLog
        eplog = EpisodeLog(env)
        st_ret, st_len = torch.zeros(envs, dtype=torch.float64, device=dev), torch.zeros(envs, dtype=torch.int32, device=dev)
        st_out = torch.zeros((1, 3), dtype=torch.int64, device=dev)

        def run_episode_stats():
            N.check(N.lib().ssg_pop_episode_stats(env._h, 1, horizon, C.c_void_p(b["rew"].data_ptr()), C.c_void_p(b["done"].data_ptr()),
                                                  C.c_void_p(st_ret.data_ptr()), C.c_void_p(st_len.data_ptr()), C.c_void_p(st_out.data_ptr()),
                                                  env._stream()), env._h, "ssg_pop_episode_stats")
        paths += [("eplog_append", lambda: eplog.append(b)), ("episode_stats", run_episode_stats), ("gae_alone", lambda: ppo.gae(dict(b))),
                  ("native_eplog", native_path(ppo, seeded(), before=lambda: eplog.append(b)))]
    if report:  # the report reads a batch GAE has seen and the stats rows of an update; it changes neither
        nb_r = dict(b)
        ppo.gae(nb_r)
        st_r = torch.randn((epochs * minibatches, 4), device=dev)
        paths += [("report", lambda: ppo.report_device(nb_r, stats=st_r)), ("report_post", lambda: ppo.report_device(nb_r, stats=st_r, post=True)),
                  ("gae_only", lambda: ppo.gae(dict(b))),
                  ("native_report", native_path(ppo, seeded(), after=lambda nb, st: ppo.report_device(nb, stats=st)))]
    if checkpoint:
        paths.append(("checkpoint_save", run_checkpoint_save))
    if dp:
        paths += [("native_dp", run_native_dp)] + [("apply_rows_w%d" % W, apply_alone(W)) for W in (1, 2, 8)]
    if adv_norm:
        paths.append(("native_mbnorm", run_native_mbnorm))
    if perm:
        paths += [("perm_torch", draw_torch), ("perm_native", draw_native), ("native_permnative", run_native_permnative)]
    if ext:
        paths += [("native_ext", run_native_ext), ("dist", run_dist)]
    if timeout_bootstrap:  # the same rows, a tenth of them done with a value to bootstrap from (GAE's cost does not depend on how many)
        hit = torch.rand((horizon, envs), generator=g_n, device=dev) < 0.1
        b_boot = dict(b, done=(b["done"] | hit).to(torch.uint8).contiguous(), boot=torch.where(hit, torch.ones_like(b["val"]), torch.zeros_like(b["val"])))
        b_plain = {k: v for k, v in b_boot.items() if k != "boot"}
        paths += [("gae_plain", lambda: ppo.gae(dict(b_plain))), ("gae_boot", lambda: ppo.gae(dict(b_boot)))]
    if ret_filter:
        rfrozen.state.copy_(rflt.state)  # (whatever it holds: the frozen call's cost does not depend on it)
        paths += [("gae", lambda: ppo.gae(dict(b))), ("ret_gae", lambda: ppo.gae(dict(b), return_filter=rflt)),
                  ("ret_frozen", lambda: rfrozen.apply(dict(b))), ("ret_apply", lambda: rflt.apply(dict(b))), ("native_ret", run_native_ret)]
    if ret_filter_job:  # (the filters' states keep running from call to call, as in training: the cost does not depend on them)
        rplain, rjob = ReturnFilter(env), ReturnFilter(env, job=True)
        own = rjob.shard_rows(dict(b))

        def rows_alone(W):
            f, rows = ReturnFilter(env, job=True), torch.stack([own] * W)
            return lambda: f.apply_rows(dict(b), rows)
        paths += [("ret_apply_plain", lambda: rplain.apply(dict(b))), ("ret_apply_split", lambda: rjob.apply(dict(b)))]
        paths += [("ret_apply_rows_w%d" % W, rows_alone(W)) for W in (1, 2, 8)]
        paths += [("native_ret_plain", native_path(ppo, seeded(), return_filter=rplain)), ("native_ret_job", native_path(ppo, seeded(), return_filter=rjob))]
        # What ran before a path shows in it: the path after a whole update, whichever it is, measured 15 .. 40 us more.  So here every
        # path follows one untimed GAE over the batch; the two whole updates still differ by their order (profiles/ret_filter_job/).
    if report_job:  # the report calls read a batch GAE has seen and the stats rows of an update; they change neither
        nb_j = dict(b)
        ppo.gae(nb_j)
        st_j = torch.randn((epochs * minibatches, 4), device=dev)
        own_row = ppo.report_row(nb_j)

        def report_rows_alone(W):
            rows = torch.stack([own_row] * W)
            return lambda: ppo.report_rows(rows, st_j)
        paths += [("report_device", lambda: ppo.report_device(nb_j, stats=st_j)),
                  ("report_split", lambda: ppo.report_rows(ppo.report_row(nb_j)[None], st_j))]
        paths += [("report_rows_w%d" % W, report_rows_alone(W)) for W in (1, 2, 8)]
        paths += [("native_report_own", native_path(ppo, seeded(), after=lambda nb, st: ppo.report(nb, stats=st))),
                  ("native_report_job", native_path(ppo, seeded(), after=lambda nb, st: ppo.job_report(nb, stats=st)))]
    if episode_log_job:  # (the carries and the rings keep running from call to call, as in training: the cost does not depend on them)
        from ship_sim_gym_amd.episode_log import EpisodeLog
        ep_plain, ep_job = EpisodeLog(env), EpisodeLog(env, job=True, rows=horizon)
        own_block = EpisodeLog(env, job=True, rows=horizon).shard_block(b)

        def merge_alone(W):
            log, stacked = EpisodeLog(env, job=True, rows=horizon, world=W, total_envs=W * envs), torch.stack([own_block] * W)
            return lambda: log.merge_blocks(stacked, K=horizon, step0=0)
        paths += [("eplog_plain", lambda: ep_plain.append(b)), ("eplog_split", lambda: ep_job.job_append(b))]
        paths += [("eplog_merge_w%d" % W, merge_alone(W)) for W in (1, 2, 8)]
        paths += [("native_eplog_plain", native_path(ppo, seeded(), before=lambda: ep_plain.append(b))),
                  ("native_eplog_job", native_path(ppo, seeded(), before=lambda: ep_job.job_append(b)))]
    if adv_norm_job:  # (each trainer rebinds its own source of statistics on the env before every call)
        from ship_sim_gym_amd.dp import DataParallelPPO
        ppo_jb, ppo_jm = DataParallelPPO(pol, env), DataParallelPPO(pol, env, job_adv_norm="minibatch")
        ppo_sm = NativePPO(pol, env, adv_norm="minibatch")
        nb_a = dict(b)
        ppo.gae(nb_a)
        perm_a = torch.stack([torch.randperm(n, device=dev, generator=seeded()) for _ in range(epochs)])
        own_sums = ppo_jm.shard_minibatch_sums(nb_a, perm_a, minibatches)

        def mb_rows_alone(W):
            stacked = torch.stack([own_sums] * W)
            return lambda: ppo_jm.set_minibatch_rows(stacked)
        paths += [("native_dp_batch", native_path(ppo_jb, seeded())), ("native_dp_mbjob", native_path(ppo_jm, seeded())),
                  ("native_mbnorm_single", native_path(ppo_sm, seeded())),
                  ("mb_sums", lambda: ppo_jm.shard_minibatch_sums(nb_a, perm_a, minibatches))]
        paths += [("mb_rows_w%d" % W, mb_rows_alone(W)) for W in (1, 2, 8)]
    if ret_filter_job or report_job or episode_log_job or adv_norm_job:
        spacer = lambda: ppo.gae(dict(b))  # noqa: E731
    else:
        spacer = lambda: None  # noqa: E731
    times = {k: [] for k, _ in paths}
    timer = {"checkpoint_save": _wall_ms}  # (a save is host work: HIP events would bracket only its copies)
    for _ in range(2):
        for k, f in paths:
            spacer()
            timer.get(k, _timed)(f)
    for _ in range(repeats):
        for k, f in paths:
            spacer()
            times[k].append(timer.get(k, _timed)(f))
    peaks = {"perm_torch_peak_bytes": _peak_bytes(draw_torch), "perm_native_peak_bytes": _peak_bytes(draw_native)} if perm else {}
    env.close()
    out = {"envs": envs, "separate_value": bool(separate_value), "horizon": horizon, "epochs": epochs, "minibatches": minibatches, "samples_per_minibatch": -(-n // minibatches)}
    for k, v in times.items():
        out[k + "_ms_per_update"] = statistics.median(v)
        out[k + "_ms_all"] = [round(x, 3) for x in v]
    out.update(peaks)
    if episode_log or episode_log_job:
        out["episodes_per_append"] = int(b["done"].ne(0).sum().item())
    if episode_log_job:
        out["eplog_block_bytes"], out["eplog_stage"] = int(ep_job.block_nbytes), int(ep_job.stage)
    if ckpt_path is not None:
        out["checkpoint_file_bytes"] = os.path.getsize(ckpt_path)
        os.remove(ckpt_path)
    if "torch" in times and "native" in times:
        out["speedup"] = out["torch_ms_per_update"] / out["native_ms_per_update"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="65536x32,4096x64")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only", choices=("torch", "native"), default=None)
    ap.add_argument("--ext", action="store_true", help="also time the extended update (all three terms on) and ssg_ppo_dist alone")
    ap.add_argument("--separate-value", action="store_true", help="also measure the separate-value-network shape, in the same process")
    ap.add_argument("--ret-filter", action="store_true", help="also time return normalisation: GAE alone, apply + GAE, the frozen apply, "
                                                              "the updating apply, and the whole GAE + update with the filter")
    ap.add_argument("--adv-norm", action="store_true", help="also time the whole GAE + update with per-minibatch advantage normalisation")
    ap.add_argument("--perm", action="store_true", help="also time the permutation draws alone (torch's and the library's), the whole GAE + "
                                                        "update with the library drawing, and each draw's peak memory")
    ap.add_argument("--timeout-bootstrap", action="store_true", help="also time ssg_ppo_gae_boot against ssg_ppo_gae, each alone")
    ap.add_argument("--checkpoint", action="store_true", help="also time one checkpoint save (policy, trainer, env, both filters) and report "
                                                              "the file's size, next to the GAE + update of the same process")
    ap.add_argument("--checkpoint-dir", default=None, help="where --checkpoint writes its file (default: the system's temporary directory)")
    ap.add_argument("--dp", action="store_true", help="also time the whole GAE + update through DataParallelPPO on one rank, and the apply "
                                                      "launch alone on 1, 2 and 8 rows")
    ap.add_argument("--episode-log", action="store_true", help="also time the episode log's append alone, ssg_pop_episode_stats alone, GAE "
                                                               "alone, and the whole GAE + update with the append ahead of it")
    ap.add_argument("--report", action="store_true", help="also time the update report alone (without and with the post-update group), GAE "
                                                          "alone, and the whole GAE + update with the report behind it")
    ap.add_argument("--ret-filter-job", action="store_true", help="also time the job-wide return filter on one device: the split call at "
                                                                  "W = 1 against ssg_ret_filter_apply, apply_rows alone on 1, 2 and 8 "
                                                                  "stacked rows, and the whole GAE + update with each")
    ap.add_argument("--report-job", action="store_true", help="also time the job's update report on one device: the split call at W = 1 "
                                                              "against ssg_ppo_report, report_rows alone on 1, 2 and 8 stacked rows, and "
                                                              "the whole GAE + update with report() and with job_report() behind it")
    ap.add_argument("--episode-log-job", action="store_true", help="also time the job-wide episode log on one device: the split call at "
                                                                   "W = 1 against ssg_episode_log_append, merge_blocks alone on 1, 2 and "
                                                                   "8 stacked blocks, and the whole GAE + update with each log ahead of it")
    ap.add_argument("--adv-norm-job", action="store_true", help="also time the job-wide per-minibatch advantage normalisation on one rank: "
                                                                "the whole GAE + update of DataParallelPPO in that mode, in batch mode, "
                                                                "and of NativePPO(adv_norm='minibatch'); the sums call and the rows "
                                                                "call alone (1, 2 and 8 stacked blocks)")
    a = ap.parse_args()
    mod = _ppo()
    res = [measure(mod, int(c.split("x")[0]), int(c.split("x")[1]), a.repeats, a.only, "cuda:0", ext=a.ext, separate_value=sep, ret_filter=a.ret_filter,
                   adv_norm=a.adv_norm, perm=a.perm, timeout_bootstrap=a.timeout_bootstrap, checkpoint=a.checkpoint,
                   checkpoint_dir=a.checkpoint_dir, dp=a.dp, episode_log=a.episode_log, report=a.report, ret_filter_job=a.ret_filter_job, report_job=a.report_job,
                   episode_log_job=a.episode_log_job, adv_norm_job=a.adv_norm_job)
           for c in a.configs.split(",") for sep in ([False, True] if a.separate_value else [False])]
    print(json.dumps({"ppo_update_timing": res}))


if __name__ == "__main__":
    main()
