"""CPU checks of ppo_reference.kl_boundary_targets, the helper tests/test_kl_adapt_gpu.py takes its targets from: on any list of
minibatch means the four targets are distinct positive float32 values and kl_adapt's decision on them is exactly coef x (1.5, 1, 1,
0.5) — and one float32 step further from the boundary on either side changes nothing, so the four sit AT the two boundaries.  No GPU."""
import numpy as np
import pytest

from ppo_reference import KL_BOUNDARY_FACTORS, kl_adapt, kl_boundary_targets, kl_factor, kl_mean


@pytest.mark.parametrize("scale", [1e-6, 1e-2, 10.0])
@pytest.mark.parametrize("count", [1, 2, 5, 44])
def test_boundary_targets_sit_on_both_sides_of_both_boundaries(count, scale):
    rng = np.random.RandomState(count * 1000 + int(-np.log10(scale)) + 7)
    for draw in range(20):
        kls = (rng.uniform(0.25, 4.0, size=count) * scale).astype(np.float32)
        mean = kl_mean(kls)
        assert mean.dtype == np.float32 and np.isfinite(mean) and mean > 0
        pairs = kl_boundary_targets(kls)
        targets = [t for t, _ in pairs]
        assert tuple(f for _, f in pairs) == KL_BOUNDARY_FACTORS == (1.5, 1.0, 1.0, 0.5)
        assert all(type(t) is float and float(np.float32(t)) == t and t > 0.0 for t in targets)   # float32 values, unchanged by (float)
        assert targets[0] < targets[1] < targets[2] < targets[3]
        assert np.float32(targets[1]) * np.float32(2.0) == mean and np.float32(targets[2]) * np.float32(0.5) == mean
        assert np.nextafter(np.float32(targets[0]), np.float32(np.inf)) == np.float32(targets[1])
        assert np.nextafter(np.float32(targets[2]), np.float32(np.inf)) == np.float32(targets[3])
        for coef in (1.0, 0.3, 2.25):
            c = np.float32(coef)
            got = [kl_adapt(coef, kls, t) for t in targets]
            want = [np.float32(c * np.float32(1.5)), c, c, np.float32(c * np.float32(0.5))]
            assert all(g.dtype == np.float32 for g in got) and got == want, (draw, coef, got, want)
        assert [kl_factor(mean, t) for t in targets] == list(KL_BOUNDARY_FACTORS)
        # a mean that is off by one float32 step is told from the right one by at least one of the four
        for wrong in (np.nextafter(mean, np.float32(0.0)), np.nextafter(mean, np.float32(np.inf))):
            assert [kl_factor(wrong, t) for t in targets] != list(KL_BOUNDARY_FACTORS)


def test_the_mean_is_the_float32_sum_in_order_over_the_count():
    kls = np.array([1e-3, 1.0, 3e-8, 2.5e-1, 7e-4], dtype=np.float32)
    s = np.float32(0.0)
    for k in kls:
        s = np.float32(s + k)
    assert kl_mean(kls) == np.float32(s / np.float32(5.0)) and kl_mean(kls, 6) == np.float32(s / np.float32(6.0))
    assert kl_mean(kls[:1]) == kls[0]
