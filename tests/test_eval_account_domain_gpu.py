"""The evaluation's accounting and reduce kernels over their domain (eval_account_kernel, eval_reduce_kernel, eval_reduce_sliced_kernel;
ssg_eval_account / ssg_eval_reduce, ship_sim_gym_amd/evaluate.py NativeEvaluator.account / reduce).  The inputs are synthetic (tests/
accounting_support.py): one ``account()`` call per row of [T, N] arrays, an env serving as the handle only.  The reference of the
accounting is ``eval_walk`` as it stands, the reference of the reduce numpy's column sums; every comparison is of integers or of bytes.

Accounting shapes: N in {1, 63, 64, 65, 255, 256, 257, 513} (one env; below / at / above a wave; below / at / above the 256-lane
workgroup; two workgroups and a one-env tail) x T in {1, 2, 12} x E in {1, 3, 2^31 - 1}; done patterns p = 0, 0.3, 1, only the last
env, only envs 255 and 256; the reward families tie / big / sim, each with all 256 flag bytes on done steps and on the others.

The ``_..._cases`` generators build a test's inputs and references and assert, on the host, what the inputs must hold for the case to
mean anything (ties of both signs, integers wider than 32 bits, envs on both sides of the quota); the tests put each case on the device."""
import numpy as np
import pytest

from accounting_support import FAMILIES, eval_walk_with, flag_coverage, inputs, layout, same_bits, tie_signs
from gpu_support import DEV, torch_cuda  # noqa: F401
from ret_filter_support import handles  # noqa: F401

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 255, 256, 257, 513)
TS = (1, 2, 12)
ES = (1, 3, 2 ** 31 - 1)
PATTERNS = ("p0", "p0.3", "p1", "last_env", "envs_255_256")
SENT = -0x5EED5EED  # carry[:, 3] before a case: a negative int32 no count reaches


def _fresh(n):
    """A zero carry whose fourth word holds the sentinel."""
    ci = np.zeros((n, 4), dtype=np.int32)
    ci[:, 3] = SENT
    return np.zeros(n), ci


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases (host only)
# ------------------------------------------------------------------------------------------------------------------------------------
def _walk_cases(n, family):
    """Yields (what, E, case, (rows, carry) after row 0, (rows, carry) after the last row), from _fresh(n)."""
    from ship_sim_gym_amd.evaluate import eval_walk
    ties, wide, covered = [0, 0], False, False
    for ti, T in enumerate(TS):
        for ei, E in enumerate(ES):
            for pi, pattern in enumerate(PATTERNS):
                case = inputs(family, pattern, T, n, seed=100000 * n + 1000 * ti + 100 * ei + 10 * pi + FAMILIES.index(family))
                if case is None:
                    continue
                what = (n, family, T, E, pattern)
                mask = case[1] != 0
                if min(np.count_nonzero(mask), np.count_nonzero(~mask)) >= 256:
                    assert flag_coverage(case[2], mask) == (256, 256), what
                    covered = True
                first, carry1 = eval_walk(case[0][:1], case[1][:1], case[2][:1], E, carry=_fresh(n))
                rest, carry2 = (eval_walk(case[0][1:], case[1][1:], case[2][1:], E, carry=carry1) if T > 1
                                else (np.zeros_like(first), carry1))
                total = first + rest
                if family == "tie":
                    returns = []
                    assert np.array_equal(eval_walk_with(*case, E, carry=_fresh(n), returns=returns)[0], total), what
                    pos, neg = tie_signs(returns)
                    ties = [ties[0] + pos, ties[1] + neg]
                    if len(returns) >= 64:  # ties of each sign, and rounding them half away from zero gives other rows
                        assert pos > 0 and neg > 0, (what, pos, neg)
                        assert not np.array_equal(eval_walk_with(*case, E, carry=_fresh(n), defect="half_away")[0], total), what
                wide = wide or bool(np.abs(total[:, 1]).max() > 2 ** 32)
                yield what, E, case, (first, carry1), (total, carry2)
    assert family != "tie" or (ties[0] > 0 and ties[1] > 0), ties
    assert family != "big" or wide       # some env's return100 leaves 32 bits
    assert n < 513 or covered            # the largest shape does place every flag byte on both kinds of step


def _quota_cases(n, T=12):
    """Yields (what, E, case, rows the state must equal from, (rows, carry)): after the first `rows` rows the state is the last
    element, and it must still be after all T."""
    from ship_sim_gym_amd.evaluate import eval_walk
    for fi, family in enumerate(FAMILIES):
        case = list(inputs(family, "p1", T, n, seed=7000 * n + fi))
        case[0][1:], case[1][1:], case[2][1:] = np.nan, 0xFF, 0xFF
        first, carry1 = eval_walk(case[0][:1], case[1][:1], case[2][:1], 1, carry=_fresh(n))
        assert (first[:, 0] == 1).all() and (carry1[1][:, 2] == 1).all() and carry1[0].tobytes() == np.zeros(n).tobytes()
        yield (n, family, "all through after row 0"), 1, case, 1, (first, carry1)
        for E in (1, 3):
            case = list(inputs(family, "p0.3", T, n, seed=7000 * n + 10 * E + fi))
            ends = np.cumsum(case[1] != 0, axis=0)
            counted = np.zeros((T, n), dtype=np.int64)  # episodes that ended BEFORE row t
            counted[1:] = ends[:-1]
            full = counted >= E
            case[0][full], case[1][full], case[2][full] = np.nan, 0xFF, 0xFF
            want, carry = eval_walk(*case, E, carry=_fresh(n))
            assert np.array_equal(carry[1][:, 2], np.minimum(ends[-1], E)) and not np.isnan(carry[0]).any()
            if n >= 63:  # cells past the quota exist; at E = 3 some envs are through and some still count at the end
                assert full.any() and (E == 1 or ((ends[-1] >= E).any() and (ends[-1] < E).any())), (n, family, E)
            yield (n, family, E, "mixed"), E, case, T, (want, carry)


def _continuation_cases(n, E, T=12):
    """Yields (what, case, (ret0, ci0, stats0), (stats, carry) after T rows)."""
    from ship_sim_gym_amd.evaluate import eval_walk
    for fi, family in enumerate(FAMILIES):
        rng = np.random.RandomState(31 * n + fi)
        case = inputs(family, "p0.3", T, n, seed=9000 * n + fi)
        ret0 = {"tie": rng.randint(-40, 41, n) / 8.0, "big": rng.randint(-5, 6, n) * 2.0 ** 25, "sim": rng.randint(-300, 301, n) * 0.01}[family]
        ci0 = np.zeros((n, 4), dtype=np.int32)
        ci0[:, 0], ci0[:, 1], ci0[:, 3] = rng.randint(1, 1000, n), rng.randint(0, 6, n), SENT
        ci0[rng.permutation(n)[:(n + 1) // 2], 2] = E - 1
        stats0 = ((rng.randint(0, 2, (n, 8)) * 2 - 1) * (2 ** 40 + rng.randint(0, 1000, (n, 8)))).astype(np.int64)
        add, carry = eval_walk(*case, E, carry=(ret0, ci0))
        if n >= 63:
            assert (carry[1][:, 2] == E).any() and (carry[1][:, 2] < E).any() and add[:, 7].any(), (n, family, E)
        yield (n, family, E), case, (ret0, ci0, stats0), (stats0 + add, carry)


# ------------------------------------------------------------------------------------------------------------------------------------
# the device side
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def evaluators(handles):
    """One NativeEvaluator per env count of the module."""
    from ship_sim_gym_amd.evaluate import NativeEvaluator
    made = {}

    def get(n):
        if n not in made:
            made[n] = NativeEvaluator(handles(n))
        return made[n]
    return get


def _load(torch, ev, ret, ci, stats=None):
    """Put carries (and stats rows, default zero) on the device."""
    ev.carry_return.copy_(torch.from_numpy(ret))
    ev.carry.copy_(torch.from_numpy(ci))
    if stats is None:
        ev.env_stats.zero_()
    else:
        ev.env_stats.copy_(torch.from_numpy(stats))


def _account(torch, ev, E, case, rows):
    """One account() call per row of `rows` (a range) of the case's device arrays."""
    for t in rows:
        ev.account(E, case[0][t], case[1][t], case[2][t])


def _dev(torch, case):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in case]


def _assert_state(ev, stats, ret, ci, what):
    got = ev.env_stats.cpu().numpy(), ev.carry_return.cpu().numpy(), ev.carry.cpu().numpy()
    assert same_bits(got[0], stats), ("env_stats", what, np.argwhere(got[0] != stats)[:4].tolist())
    assert same_bits(got[1], ret), ("carry_return", what)
    assert same_bits(got[2], ci), ("carry", what, np.argwhere(got[2] != ci)[:4].tolist())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", NS)
def test_account_equals_eval_walk_after_the_first_row_and_the_last(torch_cuda, evaluators, n, family):
    """Every (T, E, done pattern) of the module's docstring at one env count and one reward family, from a zero carry.  With tie
    rewards, a case that counts 64 episodes or more holds a tie of each sign and tells rounding half away from zero from llrint; with
    big rewards some env's return100 leaves 32 bits (_walk_cases asserts both on the inputs)."""
    torch = torch_cuda
    ev = evaluators(n)
    for what, E, case, (first, carry1), (total, carry2) in _walk_cases(n, family):
        d = _dev(torch, case)
        _load(torch, ev, *_fresh(n))
        _account(torch, ev, E, d, range(1))
        _assert_state(ev, first, *carry1, what + ("after row 0",))
        _account(torch, ev, E, d, range(1, len(case[0])))
        _assert_state(ev, total, *carry2, what + ("after the last row",))


@pytest.mark.parametrize("n", NS)
def test_an_env_at_its_quota_touches_nothing(torch_cuda, evaluators, n):
    """E = 1 and every env done in row 0: rows 1 .. 11 hold NaN rewards, done = 0xFF and flags = 0xFF, and stats and both carries must
    be bitwise what they were after row 0 — carry_return 0.0, not NaN.  Then the mixed case, E in {1, 3} with p = 0.3: every cell of an
    env that had reached E before that row is poisoned the same way, and the result is eval_walk's, which never reads such a cell."""
    torch = torch_cuda
    ev = evaluators(n)
    for what, E, case, rows, (want, carry) in _quota_cases(n):
        d = _dev(torch, case)
        _load(torch, ev, *_fresh(n))
        _account(torch, ev, E, d, range(rows))
        _assert_state(ev, want, *carry, what + ("before the poisoned rows",))
        _account(torch, ev, E, d, range(rows, len(case[0])))
        _assert_state(ev, want, *carry, what + ("after them",))
        assert not np.isnan(ev.carry_return.cpu().numpy()).any()


@pytest.mark.parametrize("E", ES[1:])
@pytest.mark.parametrize("n", NS)
def test_account_continues_carries_and_adds_to_the_rows(torch_cuda, evaluators, n, E):
    """From a state in flight: half the envs have counted E - 1 episodes (one more and they stop), every env carries a length, goal
    events and a return, and env_stats holds a nonzero pattern of integers above 2^40.  The kernel ADDS to the rows: the result is the
    pattern plus eval_walk's additions from that carry."""
    torch = torch_cuda
    ev = evaluators(n)
    for what, case, (ret0, ci0, stats0), (stats, carry) in _continuation_cases(n, E):
        _load(torch, ev, ret0, ci0, stats0)
        _account(torch, ev, E, _dev(torch, case), range(len(case[0])))
        _assert_state(ev, stats, *carry, what)


def test_the_fourth_carry_word_keeps_the_callers_value(torch_cuda, evaluators):
    """Finding: the accounting neither reads nor computes the fourth word of an env's carry.  An env below its quota stores the int4 it
    loaded, an env at its quota stores nothing, so whatever the caller put there stays — for every env, done or not, counting or
    through; here a distinct value per env, negative ones included.  (include/shipsim.h says so since this test; it used to list the
    word as 0, which is what a caller who zeroes the carry finds.)  The sentinel of every other case of this module checks the same."""
    torch = torch_cuda
    from ship_sim_gym_amd.evaluate import eval_walk
    n, T, E = 257, 12, 2
    ev = evaluators(n)
    case = inputs("sim", "p0.3", T, n, seed=77)
    ret0, ci0 = np.zeros(n), np.zeros((n, 4), dtype=np.int32)
    ci0[:, 3] = np.arange(n) * 16807 - 2 ** 21
    want, carry = eval_walk(*case, E, carry=(ret0, ci0))
    assert (carry[1][:, 2] == E).any() and (carry[1][:, 2] < E).any() and np.array_equal(carry[1][:, 3], ci0[:, 3])
    _load(torch, ev, ret0, ci0)
    _account(torch, ev, E, _dev(torch, case), range(T))
    _assert_state(ev, want, *carry, "fourth word")
    assert np.array_equal(ev.carry.cpu().numpy()[:, 3], ci0[:, 3])


# ------------------------------------------------------------------------------------------------------------------------------------
# the reduce
# ------------------------------------------------------------------------------------------------------------------------------------
EQUAL = ((1, 1), (256, 256), (257, 1), (255, 5), (512, 2), (771, 3), (1026, 2))   # envs per member: 1, 1, 257, 51, 256, 257, 513
SLICES = (1, 255, 256, 257, 513, 7)


def _reduce_case(n_envs, offsets, sizes, seed):
    """(stats int64 [N, 8] of +-(2^40 + small), the members' column sums).  Per (member, column) 15 rows in 16 share one sign, so a
    member's sums do not cancel: at 513 rows they need more than 48 bits."""
    rng = np.random.RandomState(seed)
    stats = np.empty((n_envs, 8), dtype=np.int64)
    for o, k in zip(offsets, sizes):
        sign = (rng.randint(0, 2, 8) * 2 - 1) * np.where(rng.randint(0, 16, (k, 8)) == 0, -1, 1)
        stats[o:o + k] = sign * (2 ** 40 + rng.randint(0, 4096, (k, 8)))
    want = np.stack([stats[o:o + k].sum(axis=0) for o, k in zip(offsets, sizes)])
    assert max(sizes) < 513 or np.abs(want).max() >= 2 ** 48
    assert (want < 0).any() and (want > 0).any() and not np.array_equal(want, want.astype(np.int32).astype(np.int64))
    return stats, want


def _check_reduce(torch, ev, P, offsets, sizes, seed):
    stats, want = _reduce_case(ev.env.num_envs, offsets, sizes, seed)
    ev.env_stats.copy_(torch.from_numpy(stats))
    ev.member_stats.fill_(-7)
    got = ev.reduce(P)
    assert tuple(got.shape) == (P, 8) and got.data_ptr() == ev.member_stats.data_ptr()
    assert same_bits(got.cpu().numpy(), want), (P, sizes, np.argwhere(got.cpu().numpy() != want)[:4].tolist())
    assert bool((ev.member_stats[P:] == -7).all())                         # written, not accumulated; no row past P touched
    assert torch.equal(ev.env_stats, torch.from_numpy(stats).to(DEV))      # (the input is read only)


@pytest.mark.parametrize("n_envs,P", EQUAL, ids=["N%d-P%d" % c for c in EQUAL])
def test_reduce_of_equal_slices_is_the_column_sum(torch_cuda, evaluators, n_envs, P):
    offsets, sizes = layout([n_envs // P] * P)
    _check_reduce(torch_cuda, evaluators(n_envs), P, offsets, sizes, seed=n_envs + P)


@pytest.mark.parametrize("order", ["as_listed", "reversed"])
def test_reduce_of_bound_slices_is_each_slices_column_sum(torch_cuda, evaluators, order):
    sizes = list(SLICES if order == "as_listed" else SLICES[::-1])
    ev = evaluators(sum(sizes))
    env = ev.env
    env.set_population_slices(sizes)
    try:
        offsets, sizes = layout(sizes)
        _check_reduce(torch_cuda, ev, len(sizes), offsets, sizes, seed=len(order))
        _check_reduce(torch_cuda, ev, 1, [0], [env.num_envs], seed=len(order) + 1)   # one policy: the whole handle, whatever is bound
    finally:
        env.set_population_slices(None)
