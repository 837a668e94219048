"""The observation filter over its whole domain (ship_sim_gym_amd/csrc/shipsim_filter.hip, the FILTER instantiations of shipsim_policy.hip;
include/shipsim.h "Observation filter").  tests/test_obs_filter_gpu.py stops at four tiles and D = 48; this module runs the shapes at which
the kernels take another path (profiles/obs_filter/README.md lists, per case, T, L, the runs, the column chunks and the passes of the
finalise loop):

* the two update kernels against ``merge_reference`` — count, mean and M2 bit for bit, denom within 2 ulp of the square root formed from
  the device's own M2 — at runs of more than one tile, empty runs, a one-row tail tile, a second and third group of the eight-tile
  prefetch, every column-chunk pattern up to D = 176 and counts past 2^31.  Batches are caller-made; each holds columns of different
  scales, a constant column (mean exact, M2 == 0.0) and an ill-conditioned column of exact values k 2^-10 + 2^20, for which
  tests/test_obs_filter.py states what the reduction order delivers.  Before every update the workspace is filled with NaN bytes, and
  the same update on a cloned state with a zeroed workspace must leave the same bits: finalise reads no partial that was not written.
* populations: 256 members of three rows each, every member checked; unequal slices of 9, 2 and 19 tiles (surplus workgroups for two
  members) against merge_reference and against a single-policy filter on a handle of the member's size; one fused rollout at nine tiles.
* the filtered policy kernels at D = 176 / hidden 16 and D = 7 / hidden 128 and at the wave tails: x bit for bit ObsFilter.normalise, and
  action, logp and value bit for bit those of the UNFILTERED kernel fed x (obs := x.double(), obs_scale = 1: (float)(x / 1.0) == x), the
  kernel tests/test_ppo_domain_gpu.py::test_policy_forward_domain checks against an f64 forward."""
import numpy as np
import pytest

from gpu_support import DEV, env_config, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, assert_same_rollout, split_module

pytestmark = pytest.mark.gpu

HIST_BEAMS = {7: (1, 1), 32: (2, 10), 33: (3, 5), 63: (7, 3), 64: (4, 10), 176: (8, 16)}
TILE, RUNS = 256, 8
KEYS = ("obs", "act", "logp", "val", "rew", "done", "flags")


def _vec(n, D, base=0):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    history, beams = HIST_BEAMS[D]
    env = ShipVecEnv(n, n_maps=16, n_beams=beams, env_config=env_config(history), env_id_base=base)
    assert env.states_history == D
    return env


def _filter(env, **kw):
    from ship_sim_gym_amd.obs_filter import ObsFilter
    return ObsFilter(env, **kw)


def _steps(env, k, seed=5):
    for a in env.random_actions(seed, 0, k):
        env.step_tensor(a)


def _batch(rng, n, D, t):
    """n rows for merge t (numpy f64): column c at scale 10^(t - 1) * 10^(c % 4 - 1) (test_obs_filter_gpu.py's mixture, per column as
    well as per merge), the last column constant, the one before it k 2^-10 + 2^20 with k a uniform integer in -1024..1024, and the one
    before that a noisy ramp over the rows: the tiles' means then lie far apart against the spread inside a tile, so the
    delta * delta * (n * (n_b / n')) term carries M2 at every merge and the last bit of its weight shows."""
    x = (rng.random_sample((n, D)) - 0.3) * (10.0 ** (t - 1) * 10.0 ** (np.arange(D) % 4 - 1))
    x[:, D - 3] = 0.37 * np.arange(n) + 1000.0 * t + rng.random_sample(n)
    x[:, D - 2] = rng.randint(-1024, 1025, n) * 2.0 ** -10 + 2.0 ** 20
    x[:, D - 1] = -1.0
    return x


def _check_rows(got, prev, x, eps):
    """One member's state rows (numpy [4, D]) against merge_reference(prev, x): test_obs_filter_gpu.py's _check_state rule."""
    from ship_sim_gym_amd.obs_filter import merge_reference
    want = merge_reference(prev, x, eps=eps)
    assert np.isfinite(got).all()
    assert got[3, 0] == want[3, 0] and not got[3, 1:].any()
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])
    cnt = got[3, 0]
    den = np.sqrt(got[1] / (cnt - 1.0)) + eps if cnt >= 2 else np.ones_like(got[1])
    assert np.all(np.abs(got[2] - den) <= 2 * np.spacing(den)), np.abs(got[2] - den).max()
    return got


def _poisoned_update(torch, flt, twin, batch):
    """flt.update(batch) on a workspace of NaN bytes; then the same update from the same state on `twin`'s zeroed workspace: same bits."""
    twin.state.copy_(flt.state)
    twin.workspace.zero_()
    flt.workspace.fill_(0xFF)
    flt.update(batch)
    twin.update(batch)
    assert torch.isfinite(flt.state).all() and torch.equal(twin.state, flt.state)


def _merge_case(torch, env, seed, state0=None, merges=2):
    """`merges` successive updates of a single-member filter on `env` with caller-made batches, each checked; returns the last rows."""
    n, D = env.num_envs, env.states_history
    rng = np.random.RandomState(seed)
    flt, twin = _filter(env), _filter(env)
    prev = np.zeros((4, D))
    if state0 is not None:
        prev = state0
        flt.state[0].copy_(torch.from_numpy(state0))
    for t in range(merges):
        x = _batch(rng, n, D, t)
        _poisoned_update(torch, flt, twin, torch.from_numpy(x).to(DEV))
        prev = _check_rows(flt.state[0].cpu().numpy(), prev, x, flt.eps)
        assert prev[0, D - 1] == -1.0 and prev[1, D - 1] == 0.0        # the constant column
    return prev


def _geometry(n):
    T = -(-n // TILE)
    return T, -(-T // RUNS)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the update kernels
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,L", [(2048, 8, 1), (2049, 9, 2), (4097, 17, 3), (16384, 64, 8), (16385, 65, 9), (35000, 137, 18)])
def test_update_at_every_run_and_prefetch_shape(torch_cuda, n, T, L):
    """Eight runs of exactly one tile; runs of 2,2,2,2,1,0,0,0 and of 3,3,3,3,3,2,0,0 tiles with a one-row last tile; one exact prefetch
    group per run; a second group of one tile; three groups (8, 8, 2) with a last run of 11 tiles."""
    assert _geometry(n) == (T, L)
    env = _vec(n, 7)
    rows = _merge_case(torch_cuda, env, seed=n)
    assert rows[3, 0] == 2 * n
    env.close()


@pytest.mark.parametrize("D", sorted(HIST_BEAMS))
def test_update_at_every_column_chunk_pattern(torch_cuda, D):
    """Column chunks of 7; 31 + 1 (the one-column remainder: LDS stride 1, 256 rows per pass); 31 + 2; 31 + 31 + 1; 31 + 31 + 2; and
    5 x 31 + 21 at the widest observation, where the finalise loop's 8 D work items take six passes — each at two tiles of which one
    a one-row tail, at nine tiles in runs of two, and the widest at 65 tiles as well."""
    for n in (257, 2049) + ((16385,) if D == 176 else ()):
        env = _vec(n, D)
        rows = _merge_case(torch_cuda, env, seed=1000 * D + n)
        assert rows[3, 0] == 2 * n
        env.close()


def _count_state(D, count):
    """State rows of `count` rows so far with arbitrary means; M2 = U(1, 100) * count in the even columns (a spread of a few units) and
    U(1, 100) in the odd ones (next to none: there the merged M2 is the delta * delta term, weight and all)."""
    rng = np.random.RandomState(D)
    st = np.zeros((4, D))
    st[0] = rng.uniform(-5.0, 5.0, D)
    st[1] = rng.uniform(1.0, 100.0, D) * np.where(np.arange(D) % 2 == 0, float(count), 1.0)
    st[0, D - 1], st[1, D - 1] = -1.0, 0.0                             # (the batches' constant column, so that it stays checkable)
    st[2] = np.sqrt(st[1] / (count - 1.0)) + 1e-8
    st[3, 0] = float(count)
    assert int(st[3, 0]) == count
    return st


@pytest.mark.parametrize("n,D,count", [(4097, 7, 2 ** 31 + 12345), (4097, 33, 2 ** 40)])
def test_update_into_a_count_past_2_31(torch_cuda, n, D, count):
    """A hand-written state of `count` rows with arbitrary mean and M2, three merges of 17 tiles: the merged count is exact, mean and M2
    the restatement's.  (At these n the weight n * (n_b / n') differs in its last bit from n_b * (n / n') in the second merge of
    the first case and the third of the second, so the association of the weight is checked here too.)"""
    state0 = _count_state(D, count)
    env = _vec(n, D)
    rows = _merge_case(torch_cuda, env, seed=count % 9973, state0=state0, merges=3)
    assert int(rows[3, 0]) == count + 3 * n and rows[3, 0] != state0[3, 0]
    env.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. populations
# ------------------------------------------------------------------------------------------------------------------------------------
def test_population_at_the_member_limit(torch_cuda):
    """POP_MAX_MEMBERS members of three rows each: EVERY member is the single-member restatement of its own rows."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    P, rows, D = N.POP_MAX_MEMBERS, 3, 7
    assert P == 256
    env = _vec(P * rows, D)
    flt, twin = _filter(env, n_members=P), _filter(env, n_members=P)
    rng = np.random.RandomState(256)
    prev = np.zeros((P, 4, D))
    for t in range(2):
        x = _batch(rng, P * rows, D, t)
        _poisoned_update(torch, flt, twin, torch.from_numpy(x).to(DEV))
        got = flt.state.cpu().numpy()
        for m in range(P):
            _check_rows(got[m], prev[m], x[m * rows:(m + 1) * rows], flt.eps)
        prev = got
    assert (prev[:, 3, 0] == 2 * rows).all() and (prev[:, 0, D - 1] == -1.0).all() and not prev[:, 1, D - 1].any()
    assert len({prev[m, 0, 0] for m in range(P)}) == P                 # (the members' rows differ, so a misplaced slice shows)
    env.close()


def test_sliced_population_with_surplus_workgroups(torch_cuda):
    """Slices of 2049, 300 and 4700 rows (T = 9, 2, 19; L = 2, 1, 3): the widest sets the tile stride, so the other two members have
    surplus workgroups that write no partials.  Each member is merge_reference on its rows and, bit for bit, a single-policy filter
    on a handle of its size fed the same rows."""
    torch = torch_cuda
    sizes, D = (2049, 300, 4700), 32
    assert [_geometry(n) for n in sizes] == [(9, 2), (2, 1), (19, 3)]
    offs = [sum(sizes[:m]) for m in range(3)]
    env = _vec(sum(sizes), D)
    env.set_population_slices(sizes)
    flt, twin = _filter(env, n_members=3), _filter(env, n_members=3)
    singles = []
    for o, n in zip(offs, sizes):
        sh = _vec(n, D, base=o)
        singles.append((sh, _filter(sh), _filter(sh)))
    rng = np.random.RandomState(32)
    prev = np.zeros((3, 4, D))
    for t in range(2):
        x = _batch(rng, sum(sizes), D, t)
        batch = torch.from_numpy(x).to(DEV)
        _poisoned_update(torch, flt, twin, batch)
        got = flt.state.cpu().numpy()
        for m, (o, n) in enumerate(zip(offs, sizes)):
            _check_rows(got[m], prev[m], x[o:o + n], flt.eps)
            sh, fs, ft = singles[m]
            _poisoned_update(torch, fs, ft, batch[o:o + n].contiguous())
            assert torch.equal(flt.state[m], fs.state[0]), (t, m)
        prev = got
    assert prev[:, 3, 0].tolist() == [2.0 * n for n in sizes]
    for sh, _, _ in singles:
        sh.close()
    env.close()


def test_fused_rollout_updates_at_nine_tiles(torch_cuda):
    """rollout_policy's own enqueue of the two launches at a multi-run shape (n = 2049, D = 32, K = 2) against the hand loop of
    update() / policy_act / step_tensor (test_obs_filter_gpu.py::test_rollout_updates_then_normalises at four tiles)."""
    torch = torch_cuda
    n, D, K = 2049, 32, 2
    pol = actor_critic_policy(torch, D, seed=D)[1]
    a, b = _vec(n, D), _vec(n, D)
    fa, fb = _filter(a), _filter(b)
    a.set_obs_filter(fa); b.set_obs_filter(fb)
    a.reset_tensor(); b.reset_tensor()
    fa.workspace.fill_(0xFF)
    ra = a.rollout_policy(pol, K, seed=9, step0=2)
    rows = {k: [] for k in KEYS}
    prev = np.zeros((4, D))
    for k in range(K):
        obs = b.obs.cpu().numpy()
        fb.workspace.fill_(0xFF)
        fb.update()
        prev = _check_rows(fb.state[0].cpu().numpy(), prev, obs, fb.eps)
        act, lp, v, x = b.policy_act(pol, seed=9, step=2 + k)
        rows["obs"].append(x); rows["act"].append(act); rows["logp"].append(lp); rows["val"].append(v)
        _, r, d, f = b.step_tensor(act)
        rows["rew"].append(r.clone()); rows["done"].append(d.clone()); rows["flags"].append(f.clone())
    rb = {k: torch.stack(v) for k, v in rows.items()}
    rb["last_val"] = b.policy_act(pol, seed=9, step=2 + K)[2]
    assert_same_rollout(torch, ra, rb, "updating")
    assert torch.equal(fa.state, fb.state) and torch.equal(a.obs, b.obs) and torch.isfinite(fa.state).all()
    assert fa.count.item() == K * n
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the filtered policy kernels
# ------------------------------------------------------------------------------------------------------------------------------------
CLIPS = (0.0, 0.1, 10.0)   # 0.1 is not an f32 number: the clamp is in f64, then one rounding


def _unit_scale_policies(torch, D, H, seed):
    """A shared and a separate-value policy whose obs_scale is all ones (a bound filter does not read it)."""
    from ship_sim_gym_amd.policy import NativePolicy
    ones = torch.ones(D, dtype=torch.float64, device=DEV)
    shared = NativePolicy.from_actor_critic(actor_critic_policy(torch, D, H, seed=seed)[0], ones)
    split = NativePolicy.from_actor_critic(split_module(torch, D, H, seed=seed + 1), ones)
    assert split.separate_value and not shared.separate_value
    return {"shared": shared, "split": split}


def _real_state(env, flt):
    """Statistics from two real updates around a few random steps (eps = 0 filters: a constant column gets denom == 0.0)."""
    env.reset_tensor()
    _steps(env, 3)
    flt.update()
    _steps(env, 2)
    flt.update()


def _edit_denoms(torch, rows):
    """Hand edits of one member's state rows [4, D]: the column with the largest M2 gets a denom a millionth of its own (most rows
    clip), its neighbour denom == 0.0 (divides by 1).  Returns the two columns.  (A lone env that only turned its rudder has seen one
    observation twice, M2 == 0 everywhere: its small denom is 1e-6, and nothing clips.)"""
    small = int(torch.argmax(rows[1]))
    zero = (small + 1) % rows.shape[1]
    rows[2, small] = 1e-6 * (float(rows[2, small]) if float(rows[1, small]) > 0.0 else 1.0)
    rows[2, zero] = 0.0
    return small, zero


def _filtered_equals_unfiltered(torch, env, flt, act_fn, member, rows, small, zero, tag):
    """For every clip and both draws: x is ObsFilter.normalise(obs), and (act, logp, value) are the unfiltered launch's on obs := x.
    act_fn(greedy) runs the launch on env.obs.  `rows`: member `member`'s rows of the env, whose columns `small` and `zero` were edited."""
    obs0 = env.obs.clone()
    for clip in CLIPS:
        flt.clip = clip
        want = flt.normalise(obs0)
        for greedy in (False, True):
            env.obs.copy_(obs0)
            env.set_obs_filter(flt)                                    # (a binding is a copy of the record: re-bind for the clip)
            a, lp, v, x = act_fn(greedy)
            assert torch.equal(x, want), (tag, clip, greedy)
            assert torch.isfinite(x).all() and torch.isfinite(lp).all() and torch.isfinite(v).all(), (tag, clip, greedy)
            env.set_obs_filter(None)
            env.obs.copy_(x.double())
            a2, lp2, v2, x2 = act_fn(greedy)
            assert torch.equal(x2, x), (tag, clip, greedy)
            for name, p, q in (("act", a, a2), ("logp", lp, lp2), ("value", v, v2)):
                assert p.dtype == q.dtype and torch.equal(p, q), (tag, clip, greedy, name)
        env.obs.copy_(obs0)
        xs = want[rows]
        d0 = obs0[rows][:, zero] - flt.mean[member, zero]              # denom == 0.0 divides by 1
        assert torch.equal(xs[:, zero], (d0.clamp(-clip, clip) if clip > 0.0 else d0).float()), (tag, clip)
        if clip > 0.0 and xs.shape[0] >= 63:                           # most rows of the small-denom column sit on the clip
            c32 = torch.tensor(clip, dtype=torch.float64).float().item()
            assert float((xs[:, small].abs() == c32).float().mean()) > 0.5 and float(xs.abs().max()) == c32, (tag, clip)


@pytest.mark.parametrize("D,H", [(176, 16), (7, 128)])
def test_filtered_policy_kernels_at_the_extreme_widths_and_wave_tails(torch_cuda, D, H):
    """D = 176 > hidden 16 (the obs width sizes the LDS rows the mean / denom doubles are staged in) and D = 7 under hidden 128; one
    env, a wave less one, a full wave, a wave and one, two waves and one; shared and separate value; sampled and greedy; no clamp, a
    clip that is no f32 number, and the default."""
    torch = torch_cuda
    pols = _unit_scale_policies(torch, D, H, seed=D + H)
    for n in (1, 63, 64, 65, 129):
        env = _vec(n, D)
        flt = _filter(env, eps=0.0)
        _real_state(env, flt)
        small, zero = _edit_denoms(torch, flt.state[0])
        for name, pol in pols.items():
            _filtered_equals_unfiltered(torch, env, flt, lambda g: env.policy_act(pol, seed=3, step=5, greedy=g), 0, slice(None), small,
                                        zero, (D, H, n, name))
        env.close()


def test_filtered_population_kernels_on_slices_at_the_widest_observation(torch_cuda):
    """The sliced FILTER kernels at D = 176 on slices of one env, a wave less one and two waves and one: each member normalises with
    its own edited rows, and the rest of the launch is the unfiltered sliced launch's on those x."""
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation
    D, H, sizes = 176, 16, (1, 63, 129)
    offs = [sum(sizes[:m]) for m in range(3)]
    env = _vec(sum(sizes), D)
    env.set_population_slices(sizes)
    flt = _filter(env, n_members=3, eps=0.0)
    _real_state(env, flt)
    for kind in ("shared", "split"):
        pop = NativePopulation([_unit_scale_policies(torch, D, H, seed=70 + 2 * m)[kind] for m in range(3)])
        for m, (o, n) in enumerate(zip(offs, sizes)):
            keep = flt.state.clone()
            small, zero = _edit_denoms(torch, flt.state[m])
            _filtered_equals_unfiltered(torch, env, flt, lambda g: env.population_act(pop, seed=3, step=5, greedy=g), m,
                                        slice(o, o + n), small, zero, (kind, m))
            flt.state.copy_(keep)
    env.close()
