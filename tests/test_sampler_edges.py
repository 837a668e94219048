"""Host checks of tests/sampler_edges.py: the float32 restatement of the sampler passes every case, every defect the GPU tests are there
for fails a NAMED case on a named assertion, the table holds what it promises, and the windows hold the flips."""
import numpy as np
import pytest

import sampler_edges as E

CASES = E.all_cases()
BY_NAME = {c.name: c for c in CASES}

# defect -> (a case that must catch it, the assertion that must fail there)
CAUGHT_BY = {
    "ge": ("saturated/mirror/A=3", "e"),                  # u = 0 against cdf_0 == 0: `>=` leaves action 0
    "m_for_lse": ("equal/A=3", "c"),                      # exp(lg - m) = 1: every threshold >= 1
    "one_term_short": ("spread2/A=4", "c"),               # threshold 0 is 0: the flip is at k = 1
    "one_term_long": ("spread0.5/A=2", "c"),              # threshold 0 is 1
    "logp_early": ("spread2/repeated/A=3", "d"),          # the row below the flip already carries the next action's logp
    "logp_late": ("offset-200/A=4", "d"),
    "loop_bound_A": ("dominant-10/first/A=2", "a"),       # u = 1.5 counts a third threshold: action 2 of 2
    "masked_drawn": ("-inf/last/short/A=3", "e"),         # the f32 cdf in front of the masked action is below 1 - 2^-24
}


def _run(case, defect=None):
    sc = E.scan(case)
    act, logp, la = E.restatement(case, sc.u, defect)
    return sc, act, logp, la


def test_the_table_holds_what_it_promises():
    names = set(BY_NAME)
    assert len(names) == len(CASES)
    for A in E.ACTIONS:
        for stem in ("equal", "spread0.5", "spread2", "spread8", "spread2/repeated", "offset+50", "offset-50", "offset+200", "offset-200",
                     "dominant-10/first", "dominant-16/first", "dominant-17/first", "dominant-30/first", "dominant-16/last", "dominant-17/last",
                     "saturated", "saturated/mirror", "-inf/first", "-inf/last", "nan/first", "nan/last", "+inf"):
            assert "%s/A=%d" % (stem, A) in names, (stem, A)
        assert ("-inf/middle/A=%d" % A in names) == (A > 2) and ("-inf/last/short/A=%d" % A in names) == (A > 2)
        rep = BY_NAME["spread2/repeated/A=%d" % A].lg
        assert len(set(rep)) < A
        assert E.reference64(BY_NAME["saturated/mirror/A=%d" % A])[1][0] < 1e-80          # cdf_0 == 0 in f32
        assert E.reference64(BY_NAME["saturated/A=%d" % A])[1][0] == 1.0
        # 1 + expf(d) rounds to 1 between d = -16 and d = -17
        assert np.float32(1.0) + np.exp(np.float32(-16.0)) > 1.0 and np.float32(1.0) + np.exp(np.float32(-17.0)) == 1.0
    tiny = ("dominant", "saturated", "-inf")
    for c in CASES:
        if not E.finite(c):
            assert any(x != x or x == E.PINF for x in c.lg)
            continue
        B = E.bound(c)
        assert B <= 6.2e-5 and (B <= 1.7e-5 or max(abs(x) for x in c.lg if x != E.NINF) >= 198.0), (c.name, B)
        if not c.name.startswith(tiny):
            assert E.min_probability(c) >= (3.1e-4 if c.name.startswith("spread8") else 1e-3), (c.name, E.min_probability(c))
            assert E.min_probability(c) >= 5 * B, c.name                                # a wrong partial sum is far outside the bound
    for off in (200.0, -200.0):                                                          # ulp(lse) dominates B there
        c = BY_NAME["offset%+g/A=3" % off]
        assert 4 * float(np.spacing(np.float32(200.0))) > 60 * 16 * E.GRID and E.bound(c) > 6e-5


def test_the_scan_is_the_promised_one():
    for c in CASES:
        sc = E.scan(c)
        assert sc.u.dtype == np.float32 and sc.u.size == E.N_ENVS and len(sc.windows) == c.A - 1
        for j, sl, k in sc.windows:
            assert k.size == 2 * E.HALF + 1 and k.min() >= 0 and k.max() <= E.TOP and (np.diff(k) >= 0).all()
            assert np.array_equal(sc.u[sl].astype(np.float64) * 2.0 ** 24, k.astype(np.float64))
            if E.finite(c):
                cdf = E.reference64(c)[1][j]
                assert abs(np.clip(np.rint(cdf * 2.0 ** 24), 0, E.TOP) - k[E.HALF]) <= 0 or k[0] == 0 or k[-1] == E.TOP
        assert sc.u[sc.ends].tolist() == [0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
        cal = sc.u[sc.caller]
        assert cal[:2].tolist() == [1.0, 1.5] and cal[2] == 0.0 and np.signbit(cal[2]) and cal[3] == -1.0 and np.isnan(cal[4])
        assert (sc.u[sc.pad] == 0.5).all() and sc.pad.stop == E.N_ENVS
    assert E.N_ENVS >= 3 * (2 * E.HALF + 1) + 8 and E.N_ENVS % 2 == 0 and (E.N_ENVS // 2) % 64 != 0


def test_the_restatement_passes_every_case():
    worst, thresholds, flipless = 0.0, 0, 0
    for c in CASES:
        sc, act, logp, la = _run(c)
        rec = E.check_case(c, sc.u, act, logp, la)
        worst, thresholds, flipless = max(worst, rec["ratio"]), thresholds + rec["thresholds"], flipless + len(rec["flipless"])
    print("%d cases, %d thresholds, %d of them within B of an end; the largest |k_j * 2^-24 - cdf64_j| / B is %.3f" % (len(CASES), thresholds, flipless, worst))
    assert worst <= 1.0


def test_the_windows_hold_the_flip_of_every_finite_case():
    for c in CASES:
        if not E.finite(c):
            continue
        sc, act, logp, la = _run(c)
        _, rec = E.judge_case(c, sc, act, logp, la)
        cdf, B = E.reference64(c)[1], E.bound(c)
        for j in range(c.A - 1):
            if B < cdf[j] < 1.0 - E.GRID - B:
                k = rec["flips"][j]
                _, sl, ks = sc.windows[j]
                assert ks[0] < k <= ks[-1] and act[sl][np.searchsorted(ks, k)] > j >= act[sl][np.searchsorted(ks, k) - 1], (c.name, j, k)
            else:
                assert j in rec["flipless"] or j in rec["flips"], (c.name, j)


@pytest.mark.parametrize("defect", E.DEFECTS)
def test_every_defect_fails_a_named_case(defect):
    name, which = CAUGHT_BY[defect]
    c = BY_NAME[name]
    sc, act, logp, la = _run(c, defect)
    fails, _ = E.judge_case(c, sc, act, logp)
    assert fails and {w for _, w, _ in fails} >= {which}, (defect, name, fails[:3])
    with pytest.raises(AssertionError):
        E.check_case(c, sc.u, act, logp)
    caught = [x.name for x in CASES if E.judge_case(x, *_run(x, defect)[:3])[0]]
    print("%s: fails %s on (%s); %d of %d cases catch it" % (defect, name, which, len(caught), len(CASES)))
    assert name in caught


def test_defects_table_is_complete():
    assert set(CAUGHT_BY) == set(E.DEFECTS)


def test_check_case_wants_its_own_scan_and_the_distribution_row():
    c = BY_NAME["spread2/A=3"]
    sc, act, logp, la = _run(c)
    with pytest.raises(AssertionError):
        E.check_case(c, sc.u[::-1].copy(), act, logp)
    wrong = la.copy()
    wrong[7, act[7]] = np.nextafter(wrong[7, act[7]], np.float32(0.0))
    with pytest.raises(AssertionError):
        E.check_case(c, sc.u, act, logp, wrong)
    bent = act.copy()                                                           # a non-monotone act(u): one row back to the previous action
    _, sl, ks = sc.windows[1]
    bent[sl.stop - 5] -= 1
    fails, _ = E.judge_case(c, sc, bent, logp)
    assert {w for _, w, _ in fails} >= {"b"}
