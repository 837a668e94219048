"""The refusals of test_update_refusals.py that lie behind the device: ssg_ppo_grad and ssg_ppo_update consult it FIRST (check_ready), so
everything they refuse about their arguments needs one; and all seven entry points refuse a handle of another device than the current
one — the five newer ones only after everything the host can judge.  Same table form, same machinery, literals recorded from the same
earlier library.  Nothing is launched: every call is refused.  Should one ever pass, it would run on a zeroed 4 MiB device buffer that
every pointer of the call points into (64 envs, obs_dim 8, hidden 16, one layer, P = 2: every extent is a few KiB), not on made-up
addresses."""
import pytest

import test_update_refusals as R
from gpu_support import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

# as test_update_refusals.CASES; "BASE+16": a misaligned address inside the buffer
CASES = [
    ('ssg_ppo_grad', 'bound', {'pol': None}, -1, 'ssg_ppo_grad: NULL policy'),
    ('ssg_ppo_grad', 'bound', {'pol': {'struct_size': 8}}, -1, 'ssg_ppo_grad: ssg_policy.struct_size != sizeof(ssg_policy)'),
    ('ssg_ppo_grad', 'bound', {'pol': {'obs_dim': 9}}, -1, "ssg_ppo_grad: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_ppo_grad', 'bound', {'pol': {'hidden': 24}}, -1, 'ssg_ppo_grad: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_grad', 'bound', {'pol': {'hidden': 0}}, -1, 'ssg_ppo_grad: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_grad', 'bound', {'pol': {'n_hidden_layers': 3}}, -1, 'ssg_ppo_grad: n_hidden_layers must be 1 or 2'),
    ('ssg_ppo_grad', 'bound', {'pol': {'n_actions': 5}}, -1, 'ssg_ppo_grad: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_ppo_grad', 'bound', {'pol': {'activation': 7}}, -1, 'ssg_ppo_grad: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_ppo_grad', 'bound', {'pol': {'dev_params': 0}}, -1, 'ssg_ppo_grad: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_grad', 'bound', {'pol': {'dev_obs_scale': 0}}, -1, 'ssg_ppo_grad: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_grad', 'bound', {'hp': None}, -1, 'ssg_ppo_grad: NULL hparams'),
    ('ssg_ppo_grad', 'bound', {'hp': {'struct_size': 8}}, -1, 'ssg_ppo_grad: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_ppo_grad', 'bound', {'hp': {'lr': 'nan'}}, -1, 'ssg_ppo_grad: a hyper-parameter is not finite'),
    ('ssg_ppo_grad', 'bound', {'hp': {'gamma': 'inf'}}, -1, 'ssg_ppo_grad: a hyper-parameter is not finite'),
    ('ssg_ppo_grad', 'bound', {'hp': {'clip': 0.0}}, -1, 'ssg_ppo_grad: clip must be > 0'),
    ('ssg_ppo_grad', 'bound', {'hp': {'beta1': 1.0}}, -1, 'ssg_ppo_grad: betas must be in [0, 1)'),
    ('ssg_ppo_grad', 'bound', {'hp': {'beta2': -0.5}}, -1, 'ssg_ppo_grad: betas must be in [0, 1)'),
    ('ssg_ppo_grad', 'bound', {'n_samples': 0}, -1, 'ssg_ppo_grad: n_samples < 1'),
    ('ssg_ppo_grad', 'bound', {'x': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'act': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'logp': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'adv': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'ret': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'idx': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'grad': 0}, -1, 'ssg_ppo_grad: NULL dev_grad'),
    ('ssg_ppo_grad', 'bound', {'M': 0}, -1, 'ssg_ppo_grad: M < 1'),
    ('ssg_ppo_grad', 'bound', {'ws': 0}, -1, 'ssg_ppo_grad: NULL workspace'),
    ('ssg_ppo_grad', 'bound', {'ws': 'BASE+16'}, -1, 'ssg_ppo_grad: the workspace must be 256-byte aligned'),
    ('ssg_ppo_grad', 'bound', {'nbytes': 0}, -1, 'ssg_ppo_grad: workspace of 0 bytes, this call needs 1120 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_grad', 'bound', {'nbytes': 1119}, -1, 'ssg_ppo_grad: workspace of 1119 bytes, this call needs 1120 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_grad', 'bound', {'pol': None, 'hp': None}, -1, 'ssg_ppo_grad: NULL policy'),
    ('ssg_ppo_grad', 'bound', {'hp': None, 'x': 0}, -1, 'ssg_ppo_grad: NULL hparams'),
    ('ssg_ppo_grad', 'bound', {'x': 0, 'n_samples': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'idx': 0, 'ws': 0}, -1, 'ssg_ppo_grad: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_grad', 'bound', {'n_samples': 0, 'nbytes': 0}, -1, 'ssg_ppo_grad: n_samples < 1'),
    ('ssg_ppo_grad', 'bound', {'grad': 0, 'M': 0}, -1, 'ssg_ppo_grad: NULL dev_grad'),
    ('ssg_ppo_grad', 'bound', {'M': 0, 'ws': 0}, -1, 'ssg_ppo_grad: M < 1'),
    ('ssg_ppo_grad', 'advnorm1', {'ws': 0}, -1, 'ssg_ppo_grad: NULL workspace'),
    ('ssg_ppo_update', 'bound', {'pol': None}, -1, 'ssg_ppo_update: NULL policy'),
    ('ssg_ppo_update', 'bound', {'pol': {'struct_size': 8}}, -1, 'ssg_ppo_update: ssg_policy.struct_size != sizeof(ssg_policy)'),
    ('ssg_ppo_update', 'bound', {'pol': {'obs_dim': 9}}, -1, "ssg_ppo_update: obs_dim 9 differs from the handle's history*(6+n_beams) = 8"),
    ('ssg_ppo_update', 'bound', {'pol': {'hidden': 24}}, -1, 'ssg_ppo_update: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_update', 'bound', {'pol': {'hidden': 0}}, -1, 'ssg_ppo_update: hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN'),
    ('ssg_ppo_update', 'bound', {'pol': {'n_hidden_layers': 3}}, -1, 'ssg_ppo_update: n_hidden_layers must be 1 or 2'),
    ('ssg_ppo_update', 'bound', {'pol': {'n_actions': 5}}, -1, 'ssg_ppo_update: n_actions must be in 2..4 (ssg_step accepts actions 0..3)'),
    ('ssg_ppo_update', 'bound', {'pol': {'activation': 7}}, -1, 'ssg_ppo_update: activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE'),
    ('ssg_ppo_update', 'bound', {'pol': {'dev_params': 0}}, -1, 'ssg_ppo_update: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_update', 'bound', {'pol': {'dev_obs_scale': 0}}, -1, 'ssg_ppo_update: NULL dev_params or dev_obs_scale'),
    ('ssg_ppo_update', 'bound', {'hp': None}, -1, 'ssg_ppo_update: NULL hparams'),
    ('ssg_ppo_update', 'bound', {'hp': {'struct_size': 8}}, -1, 'ssg_ppo_update: ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)'),
    ('ssg_ppo_update', 'bound', {'hp': {'lr': 'nan'}}, -1, 'ssg_ppo_update: a hyper-parameter is not finite'),
    ('ssg_ppo_update', 'bound', {'hp': {'gamma': 'inf'}}, -1, 'ssg_ppo_update: a hyper-parameter is not finite'),
    ('ssg_ppo_update', 'bound', {'hp': {'clip': 0.0}}, -1, 'ssg_ppo_update: clip must be > 0'),
    ('ssg_ppo_update', 'bound', {'hp': {'beta1': 1.0}}, -1, 'ssg_ppo_update: betas must be in [0, 1)'),
    ('ssg_ppo_update', 'bound', {'hp': {'beta2': -0.5}}, -1, 'ssg_ppo_update: betas must be in [0, 1)'),
    ('ssg_ppo_update', 'bound', {'n_samples': 0}, -1, 'ssg_ppo_update: n_samples < 1'),
    ('ssg_ppo_update', 'bound', {'x': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'act': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'logp': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'adv': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'ret': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'idx': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'mv': 0}, -1, 'ssg_ppo_update: NULL dev_adam_mv'),
    ('ssg_ppo_update', 'bound', {'epochs': 0}, -1, 'ssg_ppo_update: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update', 'bound', {'minibatches': 0}, -1, 'ssg_ppo_update: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update', 'bound', {'step0': -1}, -1, 'ssg_ppo_update: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update', 'bound', {'ws': 0}, -1, 'ssg_ppo_update: NULL workspace'),
    ('ssg_ppo_update', 'bound', {'ws': 'BASE+16'}, -1, 'ssg_ppo_update: the workspace must be 256-byte aligned'),
    ('ssg_ppo_update', 'bound', {'nbytes': 0}, -1, 'ssg_ppo_update: workspace of 0 bytes, this call needs 1984 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update', 'bound', {'nbytes': 1983}, -1, 'ssg_ppo_update: workspace of 1983 bytes, this call needs 1984 (ssg_ppo_workspace_nbytes)'),
    ('ssg_ppo_update', 'bound', {'pol': None, 'hp': None}, -1, 'ssg_ppo_update: NULL policy'),
    ('ssg_ppo_update', 'bound', {'hp': None, 'x': 0}, -1, 'ssg_ppo_update: NULL hparams'),
    ('ssg_ppo_update', 'bound', {'x': 0, 'n_samples': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'idx': 0, 'ws': 0}, -1, 'ssg_ppo_update: NULL x, act, logp, adv, ret or index buffer'),
    ('ssg_ppo_update', 'bound', {'n_samples': 0, 'nbytes': 0}, -1, 'ssg_ppo_update: n_samples < 1'),
    ('ssg_ppo_update', 'bound', {'mv': 0, 'epochs': 0}, -1, 'ssg_ppo_update: NULL dev_adam_mv'),
    ('ssg_ppo_update', 'bound', {'epochs': 0, 'ws': 'BASE+16'}, -1, 'ssg_ppo_update: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update', 'bound', {'step0': -1, 'nbytes': 0}, -1, 'ssg_ppo_update: epochs < 1, minibatches < 1 or step0 < 0'),
    ('ssg_ppo_update', 'advnorm1', {'ws': 0}, -1, 'ssg_ppo_update: NULL workspace'),
    ('ssg_ppo_grad', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_grad', 'device1', {'ws': 0}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_grad_ext', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_grad_ext', 'device1', {'ws': 0}, -1, 'ssg_ppo_grad_ext: NULL workspace'),
    ('ssg_ppo_update', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_update', 'device1', {'ws': 0}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_update_ext', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_ppo_update_ext', 'device1', {'ws': 0}, -1, 'ssg_ppo_update_ext: NULL workspace'),
    ('ssg_pop_update', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_pop_update', 'device1', {'ws': 0}, -1, 'ssg_pop_update: NULL workspace'),
    ('ssg_pop_update_ext', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_pop_update_ext', 'device1', {'ws': 0}, -1, 'ssg_pop_update_ext: NULL workspace'),
    ('ssg_pop_update_sched', 'device1', {}, -1, "current HIP device 0 differs from the handle's device 1"),
    ('ssg_pop_update_sched', 'device1', {'ws': 0}, -1, 'ssg_pop_update_sched: NULL workspace'),
]


@pytest.fixture(scope="module")
def base(torch_cuda):
    buf = torch_cuda.zeros(1 << 22, dtype=torch_cuda.uint8, device="cuda:0")
    assert buf.data_ptr() % 256 == 0
    yield buf.data_ptr()
    torch_cuda.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0                                     # nothing ran


@pytest.mark.parametrize("case", range(len(CASES)), ids=["%s-%d" % (c[0], i) for i, c in enumerate(CASES)])
def test_refusal_behind_the_device_is_the_recorded_one(native, base, case):
    entry, state, kw, rc, text = CASES[case]
    kw = {k: (base + 16 if v == "BASE+16" else v) for k, v in kw.items()}
    assert R.outcome(native, entry, state, kw, base) == (rc, text), (entry, state, kw)


def test_the_table_covers_both_device_first_entry_points_and_the_mismatch_of_all_seven():
    assert {c[0] for c in CASES if c[1] == "device1"} == {"ssg_ppo_grad", "ssg_ppo_grad_ext", "ssg_ppo_update", "ssg_ppo_update_ext",
                                                          "ssg_pop_update", "ssg_pop_update_ext", "ssg_pop_update_sched"}
    for e in ("ssg_ppo_grad", "ssg_ppo_update"):
        assert sum(c[0] == e and c[1] == "bound" for c in CASES) >= 30, e
        assert any(c[0] == e and len(c[2]) >= 2 for c in CASES), e
    assert all(c[3] < 0 for c in CASES)
