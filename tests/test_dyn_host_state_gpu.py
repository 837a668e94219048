"""The host's half of the config-4 step as a table of events against ssg_debug_dyn_counters: which host-side events make the next full
cpSpaceStep rebuild its queue from the per-env flags (`queue_rebuilds`), and which leave the queue the step kernel handed over in use.
A stale queue is no crash: it is an env stepped twice, or not at all.

One handle (config 4, 256 envs, 8 beams, a 4-record bank: the one-record-per-wave kernel) walks TABLE in order; after each event it
takes one step (rollout_traj_5: five, in one ssg_rollout_traj) and the counters' growth is compared.  A twin handle takes every step and
every event except the four that must change nothing but the queue (the same bank or blob bound again, both kinds of
ssg_dyn_invalidate): after those rows the step's outputs and the player, traffic and goal-body columns are the twin's bit for bit.
Two more handles: a 65-record bank (the per-lane-planes kernel, where every reset rebuilds) and map_ring = 4 (refills rebuild
nothing).  The amounts were read from the library's code as it was before this state came to live behind one type, and the table
recorded from that library on an MI355X is this one."""
import ctypes as C

import pytest

from gpu_support import DEV, env_config, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

N_ENVS, BEAMS = 256, 8
TWIN_SKIPS = ("same_bank", "same_blob", "invalidate_zero_mask", "invalidate_null")

# (event before the step, steps taken after it, queue_rebuilds grows by)
TABLE = [
    ("first_step_after_full_reset", 1, 1),
    ("step_after_step", 1, 0),
    ("one_masked_reset", 1, 0),
    ("two_masked_resets", 1, 1),
    ("full_reset", 1, 1),
    ("same_bank", 1, 1),
    ("same_blob", 1, 1),
    ("invalidate_zero_mask", 1, 1),
    ("invalidate_null", 1, 1),
    ("generate_into_bound_bank", 1, 1),
    ("generate_into_another_buffer", 1, 0),
    ("set_terminal_obs", 1, 0),
    ("rollout_traj_5", 5, 0),
    ("one_masked_reset_again", 1, 0),  # (a step forgets the reset that joined its queue: the next one joins again)
]


def _vec(**kw):
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    kw.setdefault("n_maps", 4)
    return ShipVecEnv(N_ENVS, device=DEV, n_beams=BEAMS, n_ships=4, env_config=env_config(2, 6), **kw)


def _mask(torch, k):
    return (torch.arange(N_ENVS, device=DEV) % 3 == k).to(torch.uint8)


def _event(torch, vec, name, spare):
    from ship_sim_gym_amd import _native as N
    L = N.lib()
    if name in ("one_masked_reset", "one_masked_reset_again"):
        vec.reset_tensor(mask=_mask(torch, 0))
    elif name == "two_masked_resets":
        vec.reset_tensor(mask=_mask(torch, 1))
        vec.reset_tensor(mask=_mask(torch, 2))
    elif name == "full_reset":
        vec.reset_tensor()
    elif name == "same_bank":
        vec.set_bank(vec.bank)
    elif name == "same_blob":
        N.check(L.ssg_bind_state(vec._h, C.c_void_p(vec.state.data_ptr())), vec._h)
    elif name == "invalidate_zero_mask":
        vec.wake_dynamics(torch.zeros(N_ENVS, dtype=torch.uint8, device=DEV))
    elif name == "invalidate_null":
        vec.wake_dynamics()
    elif name == "generate_into_bound_bank":
        vec.regenerate_bank(seed=5)
    elif name == "generate_into_another_buffer":
        N.check(L.ssg_generate_bank(vec._h, 6, 0.5, C.c_void_p(spare.data_ptr()), vec.n_maps, None, vec._stream()), vec._h)
    elif name == "set_terminal_obs":
        vec.enable_terminal_obs()
    else:
        assert name in ("first_step_after_full_reset", "step_after_step", "rollout_traj_5"), name


def _steps(vec, acts):
    """The outputs of len(acts) steps: one ssg_step, or one ssg_rollout_traj."""
    if len(acts) == 1:
        return [t.clone() for t in vec.step_tensor(acts[0])]
    return list(vec.rollout_tensor(acts, trajectory=True))


def _same(torch, a, b, out_a, out_b):
    from ship_sim_gym_amd import _native as N
    return (all(torch.equal(x, y) for x, y in zip(out_a, out_b)) and
            all(torch.equal(a.field(f), b.field(f)) for f in (N.F_X, N.F_TRAFFIC, N.F_GOAL_BODIES)))


def run_table(torch):
    """[(event, growth of full_steps, growth of queue_rebuilds, outputs and columns equal the twin's)] for TABLE, then the two other handles'
    rows."""
    main, twin = _vec(), _vec()
    spare = torch.zeros_like(main.bank)
    main.reset_tensor(); twin.reset_tensor()
    acts = main.random_actions(3, 0, len(TABLE) + 4)  # (the five-step row takes four more)
    rows, k = [], 0
    for name, n_steps, _ in TABLE:
        _event(torch, main, name, spare)
        if name not in TWIN_SKIPS:
            _event(torch, twin, name, spare)
        before = main.dyn_counters()
        out_m, out_t = _steps(main, acts[k:k + n_steps]), _steps(twin, acts[k:k + n_steps])
        after = main.dyn_counters()
        k += n_steps
        rows.append((name, after[0] - before[0], after[1] - before[1], _same(torch, main, twin, out_m, out_t)))
    main.close(); twin.close()
    # the per-lane-planes kernel (more than 64 records): a masked reset cannot join the queue
    big = _vec(n_maps=65)
    big.reset_tensor()
    big.step_tensor(acts[0]); big.step_tensor(acts[1])
    big.reset_tensor(mask=_mask(torch, 0))
    before = big.dyn_counters()
    big.step_tensor(acts[2])
    after = big.dyn_counters()
    rows.append(("65_records_one_masked_reset", after[0] - before[0], after[1] - before[1], True))
    big.close()
    # map_ring = 4: seven steps hold two refills (the reset took one of the three episode starts a filled ring allows)
    ring = _vec(map_mode="fresh_device", ring=4)
    ring.reset_tensor()
    ring.step_tensor(acts[0])
    before = ring.dyn_counters()
    for i in range(1, 7):
        ring.step_tensor(acts[i])
    after = ring.dyn_counters()
    rows.append(("ring4_six_more_steps", after[0] - before[0], after[1] - before[1], True))
    ring.close()
    torch.cuda.synchronize()
    return rows


@pytest.fixture(scope="module")
def table(torch_cuda):
    return {r[0]: r for r in run_table(torch_cuda)}


@pytest.mark.parametrize("event,n_steps,rebuilds", TABLE)
def test_event_rebuilds_the_queue_or_not(table, event, n_steps, rebuilds):
    _, d_full, d_rebuilds, same = table[event]
    print(event, d_full, d_rebuilds, same)
    assert (d_full, d_rebuilds) == (n_steps, rebuilds)
    assert same  # (for TWIN_SKIPS: the event changed nothing but the queue; for the others: both handles saw it)


def test_the_per_lane_planes_kernel_rebuilds_after_one_masked_reset(table):
    assert table["65_records_one_masked_reset"][1:3] == (1, 1)


def test_ring_refills_rebuild_nothing(table):
    assert table["ring4_six_more_steps"][1:3] == (6, 0)
