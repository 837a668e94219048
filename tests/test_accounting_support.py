"""CPU checks of tests/accounting_support.py and of the power of the GPU domain tests built on it: the input builders give what they
promise, ``eval_walk_with`` without a defect is ``eval_walk``, and every defect the GPU tests are there to catch — switched on in the
numpy reference, one at a time — changes the expected result on inputs those tests really use (their own case generators are run
here).  A kernel with that defect would therefore fail the named test.  Nothing here touches a device."""
import numpy as np
import pytest

import test_episode_stats_domain_gpu as stats_cases
import test_eval_account_domain_gpu as eval_cases
from accounting_support import (DONE_BYTES, EPISODE_DEFECTS, EVAL_DEFECTS, FAMILIES, TILE, episode_stats_walk, eval_walk_with, exploit_reference,
                                exploit_sources, flag_coverage, inputs, layout, refused_sources, rewards, round_away, round_even, wrap32)


def test_the_reward_families_keep_the_walk_exact():
    rng = np.random.RandomState(0)
    tie = rewards("tie", rng, (12, 513))
    assert set(np.unique(tie * 8)) == set(range(-3, 4))
    sums = np.cumsum(tie, axis=0)
    assert np.array_equal(sums * 800.0, np.rint(sums * 800.0))              # every partial sum is a multiple of 1/8, 100 x exact
    assert (np.abs(sums * 100.0 - np.trunc(sums * 100.0)) == 0.5).any()
    big = rewards("big", rng, (12, 513))
    assert set(np.unique(big)) == {-2.0 ** 25, 2.0 ** 25} and 100 * 2.0 ** 25 > 2 ** 31 and 513 * 12 * 100 * 2.0 ** 25 < 2 ** 53
    assert set(np.unique(rewards("sim", rng, (12, 513)))) == {1.0, -1.0, -0.01}


def test_flags_hold_every_byte_on_done_steps_and_on_the_others():
    rew, done, flags = inputs("sim", "p0.3", 12, 513, seed=1)
    mask = done != 0
    assert flag_coverage(flags, mask) == (256, 256)
    assert set(np.unique(done)) == {0} | set(int(b) for b in DONE_BYTES)
    on_done = flags[mask]
    assert any(f & 0xE0 for f in on_done) and any(bin(int(f) & 0x1D).count("1") >= 2 for f in on_done) and any(f & 0x2 for f in on_done)
    assert inputs("sim", "envs_255_256", 2, 255, seed=1) is None and inputs("sim", "envs_255_256", 2, 256, seed=1)[1][:, 255].all()
    assert inputs("sim", "envs_255_256", 2, 257, seed=1)[1][:, :255].sum() == 0


def test_roundings_disagree_exactly_on_ties():
    xs = (0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 37.5, 0.49, -0.51, 3.0)
    assert [round_even(x) for x in xs] == [0, 2, 2, 0, -2, -2, 38, 0, -1, 3]
    assert [round_away(x) for x in xs] == [1, 2, 3, -1, -2, -3, 38, 0, -1, 3]
    assert wrap32(2 ** 31) == -2 ** 31 and wrap32(-2 ** 31 - 1) == 2 ** 31 - 1 and wrap32(12345) == 12345


@pytest.mark.parametrize("family", FAMILIES)
def test_eval_walk_with_no_defect_is_eval_walk(family):
    from ship_sim_gym_amd.evaluate import eval_walk
    for n, pattern, E in ((65, "p0.3", 1), (257, "p1", 3), (64, "last_env", 2 ** 31 - 1)):
        case = inputs(family, pattern, 12, n, seed=n)
        carry = (np.arange(n) / 8.0, np.tile(np.array([3, 1, 0, -9], dtype=np.int32), (n, 1)))
        want, got = eval_walk(*case, E, carry=carry), eval_walk_with(*case, E, carry=carry)
        assert np.array_equal(want[0], got[0]) and want[1][0].tobytes() == got[1][0].tobytes() and np.array_equal(want[1][1], got[1][1])


def _told_apart(cases, walk):
    """The number of `cases` (honest result, arguments of the defective walk) on which the defective walk gives another result."""
    return sum(0 if np.array_equal(walk(*args), honest) else 1 for honest, args in cases)


# defect -> the (env count, reward family) of test_account_equals_eval_walk_after_the_first_row_and_the_last that must tell it
EVAL_CATCHES = {"half_away": (64, "tie"), "unknown_bit": (1, "sim"), "goal_next_episode": (63, "sim"), "first_ending_only": (65, "big"),
                "trunc32": (257, "big")}


@pytest.mark.parametrize("defect", EVAL_DEFECTS)
def test_every_accounting_defect_changes_what_the_gpu_test_expects(defect):
    if defect == "past_quota":  # test_an_env_at_its_quota_touches_nothing: every one of its cases, at every env count
        for n in eval_cases.NS:
            for what, E, case, rows, (want, carry) in eval_cases._quota_cases(n):
                if n < 63 and what[-1] == "mixed":
                    continue  # (so few envs need not hold one that is through before the last row)
                rows_bad, carry_bad = eval_walk_with(*case, E, carry=eval_cases._fresh(n), defect=defect)
                assert not np.array_equal(rows_bad, want) and not np.array_equal(carry_bad[1], carry[1]), what
        return
    n, family = EVAL_CATCHES[defect]
    cases = [(total, (case, E)) for what, E, case, first, (total, carry) in eval_cases._walk_cases(n, family)]
    told = _told_apart(cases, lambda case, E: eval_walk_with(*case, E, carry=eval_cases._fresh(n), defect=defect)[0])
    assert told >= len(cases) // 4, (defect, told, len(cases))


# defect -> the layout of test_episode_stats_equal_the_walk_call_after_call that must tell it
EPISODE_CATCHES = {"half_away": "N255-P5", "trunc32": "N256-P256", "drop_negative_partial": "N1026-P2", "drop_tail": "slices",
                   "carry_forgotten": "N1-P1"}


@pytest.mark.parametrize("defect", EPISODE_DEFECTS)
def test_every_episode_stats_defect_changes_what_the_gpu_test_expects(defect):
    sizes = {name: sizes for name, sizes, _ in stats_cases.LAYOUTS}[EPISODE_CATCHES[defect]]
    offsets, sizes = layout(sizes)
    n = sum(sizes)
    told = total = 0
    for what, a, (rows_a, carry_a), b, (rows_b, carry_b) in stats_cases._cases(sizes):
        bad_a = episode_stats_walk(*a, np.zeros(n), np.zeros(n, dtype=np.int32), offsets, sizes, defect=defect)
        bad_b = episode_stats_walk(*b, *bad_a[1], offsets, sizes, defect=defect)
        same = np.array_equal(bad_a[0], rows_a) and np.array_equal(bad_b[0], rows_b)
        same = same and bad_b[1][0].tobytes() == carry_b[0].tobytes() and np.array_equal(bad_b[1][1], carry_b[1])
        told, total = told + (not same), total + 1
    assert told >= 3, (defect, told, total)


def test_reduce_cases_tell_a_narrow_sum_and_a_dropped_tail():
    for n_envs, P in eval_cases.EQUAL:
        offsets, sizes = layout([n_envs // P] * P)
        stats, want = eval_cases._reduce_case(n_envs, offsets, sizes, seed=n_envs + P)
        assert not np.array_equal(want, want.astype(np.int32))              # a sum kept in 32 bits
        if sizes[0] > TILE:  # a lane that took one row instead of striding over the member's rows
            assert not np.array_equal(want, np.stack([stats[o:o + TILE].sum(axis=0) for o in offsets]))
        if P > 1:            # a member that summed its neighbour's rows
            assert len({row.tobytes() for row in want}) == P


def test_source_vectors_are_what_the_library_accepts_and_refuses():
    for P in (1, 2, 6, 256):
        for name, src in exploit_sources(P).items():
            assert len(src) == P and all(0 <= s < P and src[s] == s for s in src), (P, name)
        for name, src in refused_sources(P).items():
            assert len(src) == P and (any(not 0 <= s < P for s in src) or any(src[s] != s for s in src)), (P, name)
    src = exploit_sources(256)["upper_half"]
    rows = np.arange(256)
    assert min(src[:128]) >= 128 and not np.array_equal(exploit_reference(rows, src, defect="seven_bits"), exploit_reference(rows, src))
    assert exploit_sources(256)["all_from_last"] == [255] * 256 and np.array_equal(exploit_reference(rows, [255] * 256), [255] * 256)
