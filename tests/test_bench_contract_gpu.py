"""The driver's contract for bench.py (one JSON line on stdout at N = 1), checked on a small, quick run."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_carries_the_contract_fields():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--envs-per-gpu", "8192", "--no-other-configs", "--full"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                       # exactly one line on stdout
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 20 and j["warmup"] == 5 and j["higher_is_better"] is True
    assert j["unit"] == "env-steps/s" and j["dtype"] == "f64" and j["scaling"] == "weak" and j["vs_baseline"] is None
    assert j["data"] == "synthetic" and "workload" in j["config"] and "model" not in j["config"]
    # value = envs x steps / the timed region, whole job
    assert abs(j["value"] - 8192 * 20 / (j["ms_per_step"] * 20 * 1e-3)) <= 1e-6 * j["value"]
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["algorithmic_bytes_per_env_step"] == 675 and r["avg_launch_us"] > 0
    # what binds, without fractions above 1: the 675 B formula over the wall time `value` uses, and the bytes the FUSED API
    # must move (outputs 234 + action 4 + the state columns once per 20-step launch)
    for k in ("frac_wall", "fused_compulsory_bytes_per_env_step", "frac_fused_compulsory", "measured_copy_GBps"):
        assert k in r, k
    assert "frac_of_measured_copy" not in r
    assert abs(r["frac_wall"] - 675 * j["value"] / 1e9 / 8000.0) < 1e-9
    assert abs(r["fused_compulsory_bytes_per_env_step"] - (234 + 4 + 2 * ((7 + 8) * 8 + 17) / 20.0)) < 1e-9
    assert 0 < r["frac_fused_compulsory"] < 1 and r["frac_wall"] <= r["frac"] * 1.0001
    cb = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["single_thread"]["cores"] == 1
    assert j["single_step_launch_us"] > 0 and len(j["single_step_launch_us_repeats"]) >= 5
    # the timed repeats: spread, the shader clock the step kernel recorded in each, and what preceded them (all untimed, all declared)
    assert len(j["repeats_ms"]) == j["repeats"] == len(j["repeats_shader_clock_ghz"]) == len(j["repeats_event_ms"])
    assert j["repeats_min_ms"] <= j["repeats_median_ms"] <= j["repeats_max_ms"]
    assert abs(j["repeats_median_ms"] - j["ms_per_step"] * 20) < 1e-9 and j["value_min"] <= j["value"] <= j["value_max"]
    assert all(0.5 < g < 3.0 for g in j["repeats_shader_clock_ghz"]), j["repeats_shader_clock_ghz"]   # GHz, from s_memtime / s_memrealtime
    assert j["preconditioning_ms"] >= 300.0 and j["burn_in_steps"] == 1000 and "scratch" in j["preconditioning"]


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _direct_last_step(n, W, K, R, burn_in, rows=None):
    """What bench.py's timed path computes, stepped directly on a fresh env of the headline workload: reset, burn-in, then the W
    warm-up and R x K timed steps as one trajectory rollout (step g takes action row g % rows).  Returns the last step's outputs."""
    import torch
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    vec = ShipVecEnv(n, device="cuda:0", map_mode="bank", n_maps=64, map_seed=1000, n_beams=8)
    vec.reset_tensor()
    for b0 in range(0, burn_in, 200):
        vec.rollout_tensor(vec.random_actions(777, b0, min(200, burn_in - b0)))
    T = W + K * R
    acts = vec.random_actions(12345, 0, rows or T)
    if rows:
        acts = acts[torch.arange(T, device=acts.device) % rows].contiguous()
    last = [t[-1].cpu().numpy() for t in vec.rollout_tensor(acts, trajectory=True)]
    vec.close()
    return last


def test_plain_run_times_exactly_the_steps_asked_and_dumps_its_last_step(tmp_path):
    """A plain run (no --full): one timed region of exactly --steps steps, nothing else measured, and --dump-outputs writes what the
    last timed step returned, bit for bit what the same steps give when taken directly."""
    import numpy as np
    n, K, W = 8192, 150, 30
    j = _bench("--gpus", "1", "--steps", str(K), "--warmup", str(W), "--envs-per-gpu", str(n), "--burn-in-steps", "200",
               "--dump-outputs", str(tmp_path))
    assert j["steps"] == K and j["warmup"] == W and j["repeats"] == 1 and len(j["repeats_ms"]) == 1
    assert abs(j["repeats_ms"][0] - j["ms_per_step"] * K) < 1e-9
    assert abs(j["value"] - n * K / (j["ms_per_step"] * K * 1e-3)) <= 1e-6 * j["value"]
    assert j["metric"] == "env steps/sec (batched ShipEnv)" and j["unit"] == "env-steps/s" and j["dtype"] == "f64"
    assert j["higher_is_better"] is True
    assert j["cpu_baseline"] is None and j["other_configs"] is None and j["single_step_launch_us"] is None
    assert j["roofline"]["measured_copy_GBps"] is None
    names = ("obs", "reward", "done", "flags")
    got = [np.load(tmp_path / (k + ".npy")) for k in names]
    assert [g.dtype for g in got] == [np.float64, np.float64, np.float32, np.float32]
    assert got[0].shape[0] == n and all(g.shape == (n,) for g in got[1:])
    for k, g, w in zip(names, got, _direct_last_step(n, W, K, 1, 200)):
        np.testing.assert_array_equal(g, w.astype(g.dtype), err_msg=k)


def test_long_repeat_streams_through_bounded_buffers(monkeypatch):
    """A repeat longer than one trajectory buffer set (TRAJ_RING_BYTES) with more actions than ACT_RING_BYTES holds — both shrunk
    here to a few launches: the repeat streams through the set in whole launches, the action rows wrap, and the last timed step is
    still bit for bit the direct rollout's."""
    import torch
    import bench
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    n, K, W, R = 4096, 450, 30, 2
    vec = ShipVecEnv(n, device="cuda:0", map_mode="bank", n_maps=64, map_seed=1000, n_beams=8)
    monkeypatch.setattr(bench, "TRAJ_RING_BYTES", bench.traj_bytes_per_step(n, vec.states_history) * 250)
    monkeypatch.setattr(bench, "ACT_RING_BYTES", 4 * n * 700)
    walls, evs, n_bufs, set_steps, clocks, pre, last = bench.timed_rollouts(vec, K, W, R, False, torch.device("cuda", 0),
                                                                            burn_in=200, keep_last=True)
    vec.close()
    assert set_steps == 200 and n_bufs == 1 and len(walls) == R and all(w > 0 for w in walls)
    for k, g, w in zip(("obs", "reward", "done", "flags"), last, _direct_last_step(n, W, K, R, 200, rows=600)):
        assert (g == w).all(), k
