"""The device world generator (csrc/shipsim_worldgen.hip) over its domain: the law of its draws and its geometry.

GEOMETRY.  Every record of ``regenerate_bank(return_raw=True)`` — and of a ``map_mode="fresh_device"`` ring refilled after
stepping — is rebuilt from the raw polygons and goal draws the kernel emitted by the ORACLE alone (cpConvexHull,
cpPolyShapeSetVerts / CacheData, cpPolyShapeSegmentQuery as restated in oracle/ssg_oracle.c; not the library's ssg_host_*
path) and compared bit for bit: hull vertices and their order, plane normals and offsets, boxes, counts, goals, the spawn
goal, the zeroed unused slots and the pad double.  The sweep (worldgen_law.SWEEP, 22 517 worlds) varies width_frac over
{0.05 .. 1.0}, the bounds (square, wide, tall, flat), n_goals 1..SSG_MAX_GOALS and n_maps over {1, 63, 65, 4097} (partial
last workgroups).  COVERAGE IS A CONDITION: the census of the device's own worlds must count at least 50 rays answered at
alpha 0 (the point-query path), on an edge, on a vertex circle, left-going rays answered by the right bank's pass and
right-going ones by the left bank's, 50 box early-out misses, and four distinct hull sizes — the classes
tests/test_worldgen_law.py already reaches on Mersenne-Twister-drawn worlds of the same configurations.

Reached beyond what was asked: the ``x = fallback`` arm.  In every world whose goal rows stay within 10 of the map
(height / (n_goals + 1) >= 10: all but the flat one) the corner vertices put a hull under every ray's end, and the test
asserts that no ray misses there; the flat world's rows leave the map, its rays do miss both banks (at least 50 must), and
the fallback's value in the record is checked like every other double.

NOT covered, because the generator cannot reach them:
* ``convex_hull``'s ``n <= 2`` exit: the two corners and at least one of ten continuous draws are three distinct points (with
  ten normal y deviates no hull had fewer than 4 vertices in any run);
* its exact-duplicate filter: two vertices agree in both coordinates only if two 53-bit draws repeat;
* candidate-filter ties at the ``1e-6`` pad and collinear triples in the hull's ``<= 0`` pop: measure-zero events of
  continuous draws (tests/test_abi.py holds the host's copy of this arithmetic to the oracle on constructed cases).

LAW.  65 536 maps per seed at the default bounds for width_frac 0.5, 0.1 and 0.8: the checks of worldgen_law (KS per side
pooled and per vertex index, x-y correlation within a vertex, lag-1 correlation across vertices and across maps m, m+1,
chi-square on both randints with every value present, KS on u with u < 1, exact corners, finiteness), each at alpha = 1e-6,
seeds fixed below.  tests/test_worldgen_law.py shows that the reference's own algorithm passes them and that six planted
errors do not.

TRY CAP.  One run at width_frac 4e-5 (strip 0.012 wide): most vertices reach try 1000.  The kernel returns, every x is finite
and <= x_max (the device's capped vertex is folded; the reference's is not — include/shipsim.h), and the
share of vertices left outside the strip is the one the device's law predicts.
"""
import time

import numpy as np
import pytest

from gpu_support import torch_cuda  # noqa: F401

import worldgen_law as W

pytestmark = pytest.mark.gpu

LAW_SEEDS = {0.5: (20260501, 20260502), 0.1: (20260503,), 0.8: (20260504,)}   # width_frac -> seeds, fixed before the first run
N_LAW = 65536
SWEEP_SEED0, RING_SEED, CAP_SEED, N_CAP = 7100, 7200, 7300, 4096


def _vec(monkeypatch, n_envs, bounds, n_goals, **kw):
    """A ShipVecEnv of the given bounds and number of goals (config.N_GOALS is the package's one source of ssg_config.n_goals)."""
    from ship_sim_gym_amd import config as cfgmod
    from ship_sim_gym_amd.vec_env import ShipVecEnv

    class G(cfgmod.GameConfig):
        BOUNDS = bounds

    monkeypatch.setattr(cfgmod, "N_GOALS", n_goals)
    v = ShipVecEnv(n_envs, game_config=G, n_beams=8, **kw)
    assert v.cfg.n_goals == n_goals and (v.cfg.width, v.cfg.height) == bounds
    return v


def _check_records(oracle, native, bank, raw, width, height, n_goals, width_frac, census, what):
    """bank [M, stride], raw [M, 48 + 3 n_goals] -> every record against the oracle's, bit for bit; the raw draws' domain."""
    assert np.all(np.isfinite(raw)) and np.all(np.isfinite(bank)), what
    polys = raw[:, :48].reshape(-1, 2, 12, 2)
    goal_raw = raw[:, 48:].reshape(-1, n_goals, 3)
    assert np.array_equal(polys[:, :, W.N_SEG:], np.broadcast_to(W.corners(width, height), (len(polys), 2, 2, 2))), what
    t, _ = W.standardise_banks(polys, width, height, width_frac)
    assert t.min() >= 0.0 and t.max() <= W.strip_width(width, width_frac) / W.X_SIGMA, what
    assert np.all((goal_raw[:, :, 1] >= 0.0) & (goal_raw[:, :, 1] < 1.0)), what
    world = oracle.World(oracle.default_config(width=float(width), height=float(height), n_goals=n_goals))
    spawn = (width / 2, 25.0)
    for m in range(len(bank)):
        rec = W.oracle_record(oracle, native, world, polys[m], goal_raw[m], width, spawn, census)
        if bank[m].tobytes() != rec.tobytes():
            np.testing.assert_array_equal(bank[m], rec, err_msg="%s, record %d" % (what, m))
            bad = np.nonzero(bank[m].view(np.uint64) != rec.view(np.uint64))[0]
            raise AssertionError("%s, record %d: doubles %s differ in their bits (sign of zero)" % (what, m, bad.tolist()))


def test_every_record_of_the_sweep_is_the_oracles_and_the_census_is_met(torch_cuda, oracle, native, monkeypatch):
    t0 = time.time()
    total, vecs, n_worlds = W.Census(), {}, 0
    for k, (width, height, n_goals, width_frac, n_maps) in enumerate(W.SWEEP):
        key = (width, height, n_goals)
        if key not in vecs:
            vecs[key] = _vec(monkeypatch, 64, (width, height), n_goals, n_maps=1)
        v = vecs[key]
        raw = v.regenerate_bank(SWEEP_SEED0 + k, width_frac=width_frac, n_maps=n_maps, return_raw=True).cpu().numpy()
        bank = v.bank.cpu().numpy()
        assert bank.shape == (n_maps, native.MAP_STRIDE) and raw.shape == (n_maps, 48 + 3 * n_goals)
        c = W.Census()
        _check_records(oracle, native, bank, raw, width, height, n_goals, width_frac, c, "config %r" % (W.SWEEP[k],))
        print(W.SWEEP[k], c)
        if W.corners_within_reach(height, n_goals):
            assert c.rays["ray_miss"] == 0, W.SWEEP[k]
        total.add(c)
        n_worlds += n_maps
    for v in vecs.values():
        v.close()
    print("sweep:", total)
    print("sweep wall time: %.1f s" % (time.time() - t0))
    assert n_worlds >= 20000 and total.worlds == n_worlds
    assert total.shortfalls() == []
    assert total.rays["ray_miss"] >= 50   # gen_goal_path's fallback arm (the flat world)


def test_a_fresh_device_ring_refilled_after_stepping_is_the_oracles(torch_cuda, oracle, native, monkeypatch):
    """map_mode="fresh_device" at width_frac 0.8 with three goals and one-step episodes (MAX_STEPS = 1: every env consumes one
    world per step, so the rings wrap many times and the automatic refills run inside the rollout).  The library refills
    lazily, before a launch that has no credit left, so at least one step has run since the last refill when the rollout
    returns: the refill with raw capture that follows draws at least one world for every env, and every slot it drew is
    held to the oracle."""
    from ship_sim_gym_amd.config import EnvConfig

    class E(EnvConfig):
        MAX_STEPS = 1

    n, R, n_goals, wf = 96, 4, 3, 0.8
    v = _vec(monkeypatch, n, (600, 600), n_goals, map_mode="fresh_device", ring=R, map_seed=RING_SEED, width_frac=wf, env_config=E)
    v.reset_tensor()
    v.rollout_tensor(v.random_actions(5, 0, 60))
    assert int(v.field(native.F_EPISODES).min()) == 61     # the ring of 4 wrapped fifteen times
    raw = v.refill_worlds(return_raw=True).cpu().numpy()
    bank = v.bank.cpu().numpy()
    drawn = np.nonzero(~np.isnan(raw[:, 0]))[0]
    assert len(drawn) >= n, len(drawn)
    assert len(set((drawn // R).tolist())) == n            # at least one slot of every env's ring
    c = W.Census()
    _check_records(oracle, native, bank[drawn], raw[drawn], 600, 600, n_goals, wf, c, "ring slots")
    print("ring:", c)
    assert c.rays["ray_miss"] == 0 and c.worlds == len(drawn)
    v.close()


@pytest.mark.parametrize("width_frac", [0.5, 0.1, 0.8])
def test_the_law_of_the_device_draws(torch_cuda, native, monkeypatch, width_frac):
    t0 = time.time()
    v = _vec(monkeypatch, 64, (600, 600), 5, n_maps=1)
    seen = None
    for seed in LAW_SEEDS[width_frac]:
        raw = v.regenerate_bank(seed, width_frac=width_frac, n_maps=N_LAW, return_raw=True).cpu().numpy()
        assert raw.shape == (N_LAW, 63) and np.all(np.isfinite(raw)) and bool(torch_cuda.isfinite(v.bank).all())
        polys, g = raw[:, :48].reshape(N_LAW, 2, 12, 2), raw[:, 48:].reshape(N_LAW, 5, 3)
        checks = W.bank_law_checks(polys, 600.0, 600.0, width_frac)
        checks += W.goal_law_checks(g[:, :, 0], g[:, :, 1], g[:, :, 2], 600.0, 600.0, 5)
        print("\nwidth_frac %g, seed %d, %d checks\n%s" % (width_frac, seed, len(checks), W.describe(checks)))
        for c in W.failures(checks):
            print("  FAILED %-60s %.6g against %.6g" % c[:3])
        assert W.failures(checks) == []
        rows = {r.tobytes() for r in raw}
        assert len(rows) == N_LAW                      # the counter-keyed streams of one seed do not repeat
        if seen is not None:
            assert not (rows & seen)                   # and two seeds share no record
        seen = rows
    v.close()
    print("law wall time: %.1f s" % (time.time() - t0))


def test_the_try_cap_run_returns_folded_vertices_in_the_predicted_share(torch_cuda, native, monkeypatch):
    wf = W.CAP_WIDTH_FRAC
    s_w = W.strip_width(600.0, wf)
    v = _vec(monkeypatch, 64, (600, 600), 5, n_maps=1)
    raw = v.regenerate_bank(CAP_SEED, width_frac=wf, n_maps=N_CAP, return_raw=True)
    torch_cuda.cuda.synchronize()                       # the kernel returns: 1000 tries x 20 vertices in most lanes
    raw = raw.cpu().numpy()
    assert np.all(np.isfinite(raw)) and bool(torch_cuda.isfinite(v.bank).all())
    x = raw[:, :48].reshape(N_CAP, 2, 12, 2)[:, :, :W.N_SEG, 0]
    x_min, x_max = np.array([0.0, 600.0 - s_w])[None, :, None], np.array([s_w, 600.0])[None, :, None]
    assert np.all(x <= x_max)                           # folded: never above x_max (the reference's capped vertex may be)
    share = float(np.mean(x < x_min))
    at_cap, outside = W.cap_share(s_w)
    print("try cap: share outside the strip %.6f; (1 - 2q)^999 = %.6f, (1 - 2q)^1000 = %.6f" % (share, at_cap, outside))
    assert at_cap > 0.5
    for p in (at_cap, outside):                         # (the two differ by 2q = 1.9e-4 of their value)
        lo, hi = W.proportion_bounds(p, x.size)
        assert lo < share < hi, (share, lo, hi)
    # the vertices at the cap follow the half-normal beyond the strip: t = (x_max - x) / 50 given t > s_w / 50
    t = ((x_max - x) / W.X_SIGMA)[x < x_min]
    tail0 = 2.0 * (1.0 - float(W.phi(s_w / W.X_SIGMA)))
    c = W.ks_check("KS x at the cap", 1.0 - 2.0 * (1.0 - W.phi(t)) / tail0)
    print(c)
    assert c.ok
    v.close()
