"""The refusals of test_core_refusals.py that lie behind the device (check_ready): the NULL-buffer, K < 1 and stride refusals of
ssg_rollout_traj (and of ssg_step / ssg_rollout through it) on every kind of handle, ssg_reset with map ids on a ring handle and before
the first ssg_refill_worlds, the ring-not-ready refusal of ssg_step, ssg_rollout, ssg_rollout_traj and ssg_rollout_policy,
ssg_refill_worlds on a bank handle and with a bad width_frac, and the wrong-current-device refusal of every subject that asks for the
device ("device1": the handle's device is 1, the current one 0, so no second GPU is needed), with and without something else wrong.
Same table form, same machinery, literals recorded on an MI355X from the same earlier library.

Nothing is launched but what a refused call issues before it refuses: a full ssg_reset of a freshly bound blob zeroes the blob first,
and ssg_step_host copies its actions in before it steps.  So every pointer of a call points into one zeroed 8 MiB device buffer
(256 envs, 8 beams: the ring handle's blob is well under 1 MiB; rows that would zero a config-4 blob, 36 MiB, are not in the table)."""
import pytest

import test_core_refusals as T
from gpu_support import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

BUFFER_BYTES = 8 << 20

# as test_core_refusals.CASES; "BASE": the buffer's address
CASES = [
    ('ssg_rollout_traj', 'bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'K': -1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'stride': 1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'bound+bank', {'stride': 255}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'bound+bank', {'stride': -1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'bound+bank', {'act': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'K': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'bound+bank', {'done': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'bound+bank', {'K': -2}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'bound+bank', {'rew': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'K': -1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'stride': 1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'stride': 255}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'stride': -1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'act': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'K': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'cfg4+bound+bank', {'done': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'cfg4+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'cfg4+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'cfg4+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'cfg4+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'cfg4+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'cfg4+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'cfg4+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'cfg4+bound+bank', {'K': -2}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'cfg4+bound+bank', {'rew': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'K': -1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'stride': 1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'stride': 255}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'stride': -1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'act': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'K': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'hist3+bound+bank', {'done': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'hist3+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'hist3+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'hist3+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'hist3+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'hist3+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'hist3+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'hist3+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'hist3+bound+bank', {'K': -2}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'hist3+bound+bank', {'rew': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'K': -1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'stride': 1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'stride': 255}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'stride': -1}, -1, 'ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'act': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'K': 0, 'stride': 1}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {'done': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'ring+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'ring+bound+bank', {'obs': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'ring+bound+bank', {'rew': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_step', 'ring+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'ring+bound+bank', {'act': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'ring+bound+bank', {'done': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'ring+bound+bank', {'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'ring+bound+bank', {'K': -2}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_rollout', 'ring+bound+bank', {'rew': 0, 'K': 0}, -1, 'ssg_step/ssg_rollout: NULL buffer or K < 1', []),
    ('ssg_reset', 'ring+bound+bank', {'map_ids': 'BASE', 'mask': 'BASE'}, -1, "ssg_reset: dev_map_ids must be NULL in map_ring mode (an env's records are its own ring)", []),
    ('ssg_reset', 'ring+bound+bank', {'mask': 'BASE'}, -3, 'map_ring mode: call ssg_refill_worlds before the first ssg_reset', []),
    ('ssg_reset', 'ring+bound+bank', {'map_ids': 'BASE'}, -1, "ssg_reset: dev_map_ids must be NULL in map_ring mode (an env's records are its own ring)", []),
    ('ssg_reset', 'ring+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds before the first ssg_reset', []),
    ('ssg_step', 'ring+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout', 'ring+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout', 'ring+bound+bank', {'K': 5}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_traj', 'ring+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_policy', 'ring+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_policy', 'ring+bound+bank', {'K': 0}, -1, 'ssg_rollout_policy: K < 1', []),
    ('ssg_rollout_policy', 'ring+bound+bank', {'obs': 0}, -1, 'ssg_rollout_policy: NULL dev_obs, act, logp, value, reward or done buffer', []),
    ('ssg_rollout_policy', 'ring+bound+bank', {'stride': 1}, -1, 'ssg_rollout_policy: step_stride_envs < n_envs (steps would overlap)', []),
    ('ssg_reset', 'ring+cfg4+bound+bank', {'map_ids': 'BASE', 'mask': 'BASE'}, -1, "ssg_reset: dev_map_ids must be NULL in map_ring mode (an env's records are its own ring)", []),
    ('ssg_reset', 'ring+cfg4+bound+bank', {'mask': 'BASE'}, -3, 'map_ring mode: call ssg_refill_worlds before the first ssg_reset', []),
    ('ssg_step', 'ring+cfg4+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout', 'ring+cfg4+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout', 'ring+cfg4+bound+bank', {'K': 5}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_traj', 'ring+cfg4+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_policy', 'ring+cfg4+bound+bank', {}, -3, 'map_ring mode: call ssg_refill_worlds first', []),
    ('ssg_rollout_policy', 'ring+cfg4+bound+bank', {'K': 0}, -1, 'ssg_rollout_policy: K < 1', []),
    ('ssg_rollout_policy', 'ring+cfg4+bound+bank', {'obs': 0}, -1, 'ssg_rollout_policy: NULL dev_obs, act, logp, value, reward or done buffer', []),
    ('ssg_rollout_policy', 'ring+cfg4+bound+bank', {'stride': 1}, -1, 'ssg_rollout_policy: step_stride_envs < n_envs (steps would overlap)', []),
    ('ssg_refill_worlds', 'bound+bank', {}, -1, 'ssg_refill_worlds: the handle was not created with map_ring', []),
    ('ssg_refill_worlds', 'bound+bank', {'width_frac': 0.0}, -1, 'ssg_refill_worlds: the handle was not created with map_ring', []),
    ('ssg_refill_worlds', 'cfg4+bound+bank', {}, -1, 'ssg_refill_worlds: the handle was not created with map_ring', []),
    ('ssg_refill_worlds', 'cfg4+bound+bank', {'width_frac': 0.0}, -1, 'ssg_refill_worlds: the handle was not created with map_ring', []),
    ('ssg_refill_worlds', 'ring+bound+bank', {'width_frac': 0.0}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+bound+bank', {'width_frac': -1.0}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+bound+bank', {'width_frac': 1.5}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+bound+bank', {'width_frac': 'nan'}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+cfg4+bound+bank', {'width_frac': 0.0}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+cfg4+bound+bank', {'width_frac': -1.0}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+cfg4+bound+bank', {'width_frac': 1.5}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_refill_worlds', 'ring+cfg4+bound+bank', {'width_frac': 'nan'}, -1, 'ssg_refill_worlds: bad width_frac', []),
    ('ssg_init_state', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_init_state', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_init_state', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_init_state', 'device1+bound', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+bound+bank', {'map_ids': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+cfg4+bound+bank', {'map_ids': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+ring+bound+bank', {'map_ids': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_reset', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+bound+bank', {'act': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+cfg4+bound+bank', {'act': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+ring+bound+bank', {'act': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+cfg4+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+ring+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_rollout_traj', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+bound+bank', {'stride': 1}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+cfg4+bound+bank', {'stride': 1}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+ring+bound+bank', {'stride': 1}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_traj', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step_host', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+bound+bank', {'obs': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+cfg4+bound+bank', {'obs': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+ring+bound+bank', {'obs': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_step_host', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_refill_worlds', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+bound+bank', {'width_frac': 0.0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+cfg4+bound+bank', {'width_frac': 0.0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+ring+bound+bank', {'width_frac': 0.0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_refill_worlds', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_dyn_invalidate', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+bound+bank', {'mask': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+cfg4+bound+bank', {'mask': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+ring+bound+bank', {'mask': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+bound', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_dyn_invalidate', 'device1+bound', {'mask': 'BASE'}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+cfg4+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+cfg4+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+ring+bound+bank', {}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+ring+bound+bank', {'K': 0}, -1, "current HIP device 0 differs from the handle's device 1", []),
    ('ssg_rollout_policy', 'device1+bound', {}, -3, 'no map bank set: call ssg_set_map_bank first', []),
    ('ssg_step_host', 'device1+bound+bank', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_generate_bank', 'device1+bound+bank', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_wait_host', 'device1+bound+bank', {}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
    ('ssg_step_host', 'device1+ring+bound+bank', {'slot': 8}, -1, 'ssg_step_host: NULL buffer, empty block or slot out of range', []),
    ('ssg_generate_bank', 'device1+ring+bound+bank', {'n_maps': 0}, -1, 'ssg_generate_bank: bad argument', []),
    ('ssg_wait_host', 'device1+ring+bound+bank', {}, -1, 'ssg_wait_host: no ssg_step_host was issued into this slot', []),
]


@pytest.fixture(scope="module")
def base(torch_cuda, native):
    torch = torch_cuda
    buf = torch.zeros(BUFFER_BYTES, dtype=torch.uint8, device="cuda:0")
    h = T.handle(native, "ring+bound+bank", buf.data_ptr())  # the one blob a row of the table zeroes
    rc, outs = T.call(native, "ssg_state_nbytes", h)
    native.lib().ssg_destroy(h)
    assert rc == 0 and outs[0] <= BUFFER_BYTES
    torch.cuda.synchronize()
    yield buf.data_ptr()
    torch.cuda.synchronize()
    del buf


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_behind_the_device_is_the_recorded_one(native, base, case):
    entry, state, kw, rc, text, outs = CASES[case]
    kw = {k: (base if v == "BASE" else v) for k, v in kw.items()}
    assert T.outcome(native, entry, state, kw, base) == (rc, text, outs), (entry, state, kw)


def test_the_table_covers_the_device_mismatch_of_every_subject_that_asks_for_the_device():
    asks = {"ssg_init_state", "ssg_reset", "ssg_step", "ssg_rollout", "ssg_rollout_traj", "ssg_step_host", "ssg_refill_worlds",
            "ssg_dyn_invalidate", "ssg_rollout_policy"}
    for e in asks:
        mismatch = [c for c in CASES if c[0] == e and c[1].startswith("device1")]
        assert any(not c[2] for c in mismatch) and (e == "ssg_init_state" or any(c[2] for c in mismatch)), e
    assert all(c[3] < 0 for c in CASES)  # (nothing in the table passes)
    for needle in ("call ssg_refill_worlds first", "call ssg_refill_worlds before the first ssg_reset", "dev_map_ids must be NULL",
                   "NULL buffer or K < 1", "step_stride_envs must be 0 or >= n_envs", "not created with map_ring", "bad width_frac",
                   "differs from the handle's device"):
        assert any(needle in c[4] for c in CASES), needle
