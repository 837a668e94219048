"""The return filter over its whole domain (ssg_ret_filter_apply: ship_sim_gym_amd/csrc/shipsim_retfilter.hip, ship_sim_gym_amd/ret_filter.py;
include/shipsim.h "Return filter").  tests/test_ret_filter_gpu.py stops at K = 9 steps and at n = 4097 envs for one member, 7049 for a
population; this module runs the shapes at which the three launches take another loop trip, and the value edges the header states
(profiles/ret_filter/README.md lists, per case, n, T, L, K and the pass counts of the three launches):

* pass counts, n = 257 (two tiles, the second of one row) and n = 1: K from 3 to 1024 around every multiple of the walk's four-step
  staging (its third and later passes, both LDS halves reused many times), of the division's eight steps per blockIdx.z group (up to
  128 groups) and of the chain kernel's 32 steps per pass (a second trip at K = 33, 32 trips and the whole of its two LDS arrays at
  1024); K = 33 and 1024 also on a padded row pitch.
* run and prefetch geometry at K = 5: eight runs of one tile, runs of two with empty runs and a one-row tail, one exact group of the
  eight-tile prefetch (16384), a second group of one tile (16385), three groups with a short last run (35000); 16385 also at K = 33,
  where both multi-trip loops of the chain kernel run in one launch.  The last step's rewards are a noisy ramp over the envs, and each
  case first shows on the CPU that these inputs tell the documented association of the merges from one sequential run over the tiles.
* continuation: K1 + K2 rows in one call against two calls, split at and around the chain kernel's 32 and the walk's 4, and 1 + 1023;
  ``ReturnFilter.normalise`` beyond the library's 1024-step cap against explicit library calls and the restatement.
* value edges: the discounts 0 and 1, done bytes other than 1, ill-conditioned returns, constant returns at eps = 0 (a denom of 0.0
  divides by 1), counts past 2^31, one sample; frozen calls on NaN, +-inf, -0.0, the smallest subnormal and 1e308 at every clip.
* populations: 256 members of three envs at K = 33 and 1024; unequal slices of 1, 16385, 257 and 2049 envs with surplus workgroups.

The rule everywhere is ret_filter_support._check's: count, mean, M2 and the carry bit for bit ``ret_filter_reference``'s, every denom_k
within 2 ulp of the restatement's, the state's denom within 2 ulp of the value formed from the device's own M2 and equal to the last
denom_k, out bit for bit clamp(rew / denom_k) formed from the device's own denom_k.  Before every updating call the workspace is filled
with 0xFF bytes, and the same call from a cloned state and carry on a zeroed workspace must leave the same bits: no launch reads a
partial or a denom that was not written.  That the restatement itself is right is tests/test_ret_filter.py's business
(test_reference_against_exact_arithmetic, at these shapes reduced)."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, torch_cuda, vec  # noqa: F401
from ret_filter_support import (D, _check, _dev, _filter, _geometry, _ill_inputs, _inputs, _ramp_inputs, _same_bits,  # noqa: F401
                                _samples, _sequential_m2, _ulp_close, handles)

pytestmark = pytest.mark.gpu


def _pair(env, **kw):
    """The filter under test and the twin that repeats its calls on a zeroed workspace."""
    return _filter(env, **kw), _filter(env, **kw)


def _same(torch, a, b):
    """Equal as bit patterns (an int64 view: -0.0 is not 0.0, a NaN equals itself)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _apply(torch, flt, twin, r, d):
    """flt.normalise(r, d) on a workspace of 0xFF bytes; then the same call from a clone of its state and carry on `twin`'s zeroed
    workspace: state, carry, out and denom hold the same bits.  Returns flt's (out, denom)."""
    from ship_sim_gym_amd import _native as N
    K = min(int(r.shape[0]), N.RET_FILTER_MAX_STEPS)
    twin.state.copy_(flt.state)
    twin.carry.copy_(flt.carry)
    flt.to_native(K)
    twin.to_native(K)
    flt.workspace.fill_(0xFF)
    twin.workspace.zero_()
    out, den = flt.normalise(r, d)
    out2, den2 = twin.normalise(r, d)
    for name, a, b in (("state", flt.state, twin.state), ("carry", flt.carry, twin.carry), ("out", out, out2), ("denom", den, den2)):
        assert _same(torch, a, b), name
    return out, den


def _lib_apply(env, flt, K, r, d, pitch, out, den=None):
    """One ssg_ret_filter_apply call on caller-made buffers (ReturnFilter.normalise allocates its own)."""
    from ship_sim_gym_amd import _native as N
    rec = flt.to_native(K)
    N.check(N.lib().ssg_ret_filter_apply(env._h, C.byref(rec), K, C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), pitch,
                                         C.c_void_p(out.data_ptr()), C.c_void_p(den.data_ptr()) if den is not None else None,
                                         env._stream()), env._h, "ssg_ret_filter_apply")


def _two_applies(torch, env, make, K, n, seed, pad=0, **kw):
    """Two successive applies of a fresh filter, each checked against the restatement: make(K, n, seed) from the empty state, then
    make(K, n, seed + 500) with the rewards scaled by 3 on the running state and carry.  Returns (flt, first out, r, d)."""
    flt, twin = _pair(env, **kw)
    rew, done = make(K, n, seed)
    r, d = _dev(torch, rew, done, pad)
    out, den = _apply(torch, flt, twin, r, d)
    assert out.stride(0) == n + pad and den.shape == (K, 1)
    st, carry = _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    rew2, done2 = make(K, n, seed + 500)
    rew2 = rew2 * 3.0
    r2, d2 = _dev(torch, rew2, done2, pad)
    out2, den2 = _apply(torch, flt, twin, r2, d2)
    _check(flt, st, carry, rew2, done2, out2, den2)
    assert torch.equal(r.cpu(), torch.from_numpy(rew))                 # the raw rewards stay
    return flt, out, r, d


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. pass counts of the three launches
# ------------------------------------------------------------------------------------------------------------------------------------
#          K   walk passes (4 steps)  division groups (8 steps)  chain passes (32 steps)
PASSES = [(3, 1, 1, 1), (4, 1, 1, 1), (5, 2, 1, 1), (7, 2, 1, 1), (8, 2, 1, 1), (9, 3, 2, 1), (16, 4, 2, 1), (17, 5, 3, 1), (31, 8, 4, 1),
          (32, 8, 4, 1), (33, 9, 5, 2), (63, 16, 8, 2), (64, 16, 8, 2), (65, 17, 9, 3), (1023, 256, 128, 32), (1024, 256, 128, 32)]
PASS_CASES = [(257,) + p + (0,) for p in PASSES] + [(257, 33, 9, 5, 2, 5), (257, 1024, 256, 128, 32, 5), (1, 33, 9, 5, 2, 0),
                                                     (1, 1024, 256, 128, 32, 0)]


@pytest.mark.parametrize("n,K,walk,groups,chain,pad", PASS_CASES,
                         ids=["n%d-K%d%s" % (c[0], c[1], "-pad%d" % c[5] if c[5] else "") for c in PASS_CASES])
def test_apply_at_every_pass_count(torch_cuda, handles, n, K, walk, groups, chain, pad):
    """K below, at and above the multiples of 4, 8 and 32 the three launches work in, up to the cap: the walk's LDS halves alternate
    `walk` times, the division runs `groups` blockIdx.z groups with a partial last one, the chain kernel takes `chain` trips of its
    pass loop and fills bat_mean / bat_m2 up to entry K - 1."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    assert (-(-K // 4), -(-K // 8), -(-K // 32)) == (walk, groups, chain) and K <= N.RET_FILTER_MAX_STEPS == 1024
    env = handles(n)
    flt, out, r, d = _two_applies(torch, env, _inputs, K, n, seed=1000 * n + K, pad=pad, gamma=0.99, clip=10.0, eps=1e-8)
    assert flt.count.item() == 2 * K * n
    if pad:                                                            # the padding columns were neither read into anything nor written
        base = torch.full((K, n + pad), -7.0, dtype=torch.float64, device=DEV)
        fresh = _filter(env, gamma=0.99, clip=10.0, eps=1e-8)
        fresh.to_native(K)
        fresh.workspace.fill_(0xFF)
        _lib_apply(env, fresh, K, r, d, n + pad, base)
        assert (base[:, n:] == -7.0).all() and _same(torch, base[:, :n], out)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. run and prefetch geometry
# ------------------------------------------------------------------------------------------------------------------------------------
#            n      T    L   K   seed (the first of 1000 n + K + 0 .. 19 at which the inputs discriminate; chosen on the CPU)
GEOMETRY = [(2048, 8, 1, 5, 2048005), (2049, 9, 2, 5, 2049005), (16384, 64, 8, 5, 16384007), (16385, 65, 9, 5, 16385005),
            (16385, 65, 9, 33, 16385033), (35000, 137, 18, 5, 35000005)]


@pytest.mark.parametrize("n,T,L,K,seed", GEOMETRY, ids=["n%d-K%d" % (c[0], c[3]) for c in GEOMETRY])
def test_apply_at_every_run_and_prefetch_shape(torch_cuda, handles, n, T, L, K, seed):
    """Eight runs of exactly one tile; runs of 2, 2, 2, 2, 1, 0, 0, 0 tiles with a one-row last tile; one exact prefetch group per run;
    a second group of one tile; three groups (8, 8, 2) with a last run of 11 tiles.  K = 5 is a full walk pass and a partial one; at
    K = 33 the chain kernel's pass loop and its prefetch loop both take a second trip in one launch."""
    torch = torch_cuda
    from ship_sim_gym_amd.obs_filter import merge_reference
    assert _geometry(n) == (T, L)
    # the inputs discriminate: the last step's batch M2 with all tiles merged in one sequential run differs from the restatement's
    rew, done = _ramp_inputs(K, n, seed)
    batch = _samples(np.zeros(n), rew, done, 0.99)[0][K - 1]
    restated = merge_reference(np.zeros((4, 1)), batch[:, None])[1, 0]
    assert not _same_bits(np.float64(_sequential_m2(batch)), restated), "these inputs do not tell the run merges' association"
    flt, _, _, _ = _two_applies(torch, handles(n), _ramp_inputs, K, n, seed=seed, gamma=0.99, clip=10.0, eps=1e-8)
    assert flt.count.item() == 2 * K * n


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. continuation
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K1,K2", [(257, 32, 1), (257, 31, 2), (257, 4, 29), (257, 1, 1023), (16385, 5, 4)])
def test_two_applies_continue_as_one_at_the_pass_boundaries(torch_cuda, handles, n, K1, K2):
    """One filter over K1 + K2 rows against a second over K1 and then K2 rows: a split exactly at the chain kernel's 32 steps, one
    before it, at the walk's four steps, one row and then the cap less one; and at 65 tiles with a split inside the second walk pass."""
    torch = torch_cuda
    env = handles(n)
    rew, done = _inputs(K1 + K2, n, seed=77 + n + K1)
    r, d = _dev(torch, rew, done)
    one, twin = _pair(env, gamma=0.95, clip=1.0)
    out, den = _apply(torch, one, twin, r, d)
    two = _filter(env, gamma=0.95, clip=1.0)
    oa, da = _apply(torch, two, twin, r[:K1], d[:K1])
    ob, db = _apply(torch, two, twin, r[K1:], d[K1:])
    assert torch.equal(one.state, two.state) and torch.equal(one.carry, two.carry)
    assert torch.equal(out, torch.cat([oa, ob])) and torch.equal(den, torch.cat([da, db]))
    assert torch.isfinite(out).all() and torch.isfinite(one.state).all() and one.count.item() == (K1 + K2) * n
    assert (out.abs() == 1.0).any() and (out.abs() < 1.0).any()       # (the clip bites at the events: the denom is below 1)


@pytest.mark.parametrize("K,calls", [(1025, [1024, 1]), (2049, [1024, 1024, 1])])
def test_normalise_splits_rollouts_beyond_the_cap(torch_cuda, handles, K, calls):
    """ReturnFilter.normalise cuts a rollout longer than SSG_RET_FILTER_MAX_STEPS into several library calls: the result is the
    restatement's over all rows, and bit for bit that of explicit library calls of 1024 (+ 1024) + 1 rows."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    n = 3
    env = handles(n)
    rew, done = _inputs(K, n, seed=K)
    r, d = _dev(torch, rew, done)
    flt, twin = _pair(env, gamma=0.99)
    out, den = _apply(torch, flt, twin, r, d)
    assert out.shape == (K, n) and den.shape == (K, 1)
    _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    lib = _filter(env, gamma=0.99)
    o = torch.full((K, n), -7.0, dtype=torch.float64, device=DEV)
    dn = torch.full((K, 1), -7.0, dtype=torch.float64, device=DEV)
    lib.to_native(N.RET_FILTER_MAX_STEPS)
    lib.workspace.fill_(0xFF)
    made = []
    for k0 in range(0, K, N.RET_FILTER_MAX_STEPS):
        k1 = min(K, k0 + N.RET_FILTER_MAX_STEPS)
        _lib_apply(env, lib, k1 - k0, r[k0:], d[k0:], n, o[k0:], dn[k0:])
        made.append(k1 - k0)
    assert made == calls
    for name, a, b in (("state", flt.state, lib.state), ("carry", flt.carry, lib.carry), ("out", out, o), ("denom", den, dn)):
        assert _same(torch, a, b), name


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. value edges of the updating call
# ------------------------------------------------------------------------------------------------------------------------------------
def test_gamma_zero_samples_are_the_rewards(torch_cuda, handles):
    """gamma = 0.0: c * 0 + rew[k] is rew[k], so the samples are the rewards and the carry holds the last reward, or 0 where done."""
    torch = torch_cuda
    n, K = 257, 33
    rew, done = _inputs(K, n, seed=40)
    assert _same_bits(_samples(np.zeros(n), rew, done, 0.0)[0], rew)
    flt, twin = _pair(handles(n), gamma=0.0, clip=10.0)
    r, d = _dev(torch, rew, done)
    out, den = _apply(torch, flt, twin, r, d)
    _, carry = _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    assert _same_bits(carry, np.where(done[K - 1] != 0, 0.0, rew[K - 1])) and carry[n - 1] == 0.0 and carry[0] == rew[K - 1, 0]


def test_gamma_one_returns_grow_over_the_whole_call(torch_cuda, handles):
    """gamma = 1.0 at K = 1024: the even columns never finish, so their returns are the running sums of 1024 rewards (c * 1.0 is c:
    the carry is numpy's sequential cumulative sum, bit for bit).  The count is exact and the state the restatement's."""
    torch = torch_cuda
    n, K = 257, 1024
    rew, done = _inputs(K, n, seed=41)
    done[:, 0::2] = 0
    flt, twin = _pair(handles(n), gamma=1.0, clip=10.0)
    r, d = _dev(torch, rew, done)
    out, den = _apply(torch, flt, twin, r, d)
    st, carry = _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    assert st[3] == K * n
    assert _same_bits(carry[0::2], np.cumsum(rew[:, 0::2], axis=0)[K - 1]) and np.abs(carry[0::2]).max() > 20.0


def test_any_non_zero_done_byte_resets_the_carry(torch_cuda, handles):
    """done != 0 for bytes other than 1: 2, 0x80 and 0xFF reset the carry as 1 does."""
    torch = torch_cuda
    n, K = 257, 9
    rng = np.random.RandomState(42)
    rew = _inputs(K, n, seed=42)[0]
    done = rng.choice(np.array([0, 1, 2, 0x80, 0xFF], dtype=np.uint8), size=(K, n), p=[0.8, 0.05, 0.05, 0.05, 0.05])
    done[K - 1, :10] = [0, 1, 2, 0x80, 0xFF, 0xFF, 0x80, 2, 1, 0]
    assert all((done == b).any() for b in (0, 1, 2, 0x80, 0xFF))
    flt, twin = _pair(handles(n), gamma=0.99, clip=10.0)
    r, d = _dev(torch, rew, done)
    out, den = _apply(torch, flt, twin, r, d)
    _, carry = _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    assert _same_bits(carry[done[K - 1] != 0], np.zeros(int((done[K - 1] != 0).sum()))) and (carry[done[K - 1] == 0] != 0.0).all()
    # ... and within the call: the same rows with every non-zero byte written as 1 leave the same bits
    ones = _filter(handles(n), gamma=0.99, clip=10.0)
    out1, den1 = _apply(torch, ones, twin, *_dev(torch, rew, (done != 0).astype(np.uint8)))
    assert _same(torch, ones.state, flt.state) and _same(torch, ones.carry, flt.carry) and _same(torch, out1, out) and _same(torch, den1, den)


@pytest.mark.parametrize("n,K", [(4097, 5), (300, 40)])
def test_ill_conditioned_returns(torch_cuda, handles, n, K):
    """gamma = 0 with rewards j 2^-10 + 2^20: a spread of about one against a mean of a million (kappa^2 about 3e12).  The match with
    the restatement is bit for bit as always; what the order delivers against the exact values is in tests/test_ret_filter.py."""
    torch = torch_cuda
    flt, _, _, _ = _two_applies(torch, handles(n), _ill_inputs, K, n, seed=1000 * n + K, gamma=0.0, clip=0.0, eps=1e-8)
    assert flt.count.item() == 2 * K * n and 2.0 ** 20 - 1.0 < flt.mean.item() < 3.0 * 2.0 ** 20


def test_constant_returns_at_eps_zero_divide_by_one(torch_cuda, handles):
    """Constant rewards of 0.5 at gamma = 0, clip = 0 and eps = 0: M2 is exactly 0.0 and so is the state's denom, the call divides by 1
    and says so in dev_denom_KP.  With eps = 1e-8 and clip = 10 the denom is 1e-8 and every out is the clip."""
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    n, K = 257, 5
    rew, done = np.full((K, n), 0.5), _inputs(K, n, seed=43)[1]
    r, d = _dev(torch, rew, done)
    flt, twin = _pair(handles(n), gamma=0.0, clip=0.0, eps=0.0)
    out, den = _apply(torch, flt, twin, r, d)
    st, carry = flt.state[0].cpu().numpy(), flt.carry.cpu().numpy()
    assert _same_bits(st, np.array([0.5, 0.0, 0.0, K * n]))
    assert _same_bits(den.cpu().numpy(), np.ones((K, 1))) and _same(torch, out, r)
    want = ret_filter_reference(np.zeros(4), np.zeros(n), rew, done, 0.0, 0.0, 0.0)
    assert _same_bits(st, want[0]) and _same_bits(carry, want[1]) and _same_bits(out.cpu().numpy(), want[2])
    assert _same_bits(carry, np.where(done[K - 1] != 0, 0.0, 0.5))
    flt, twin = _pair(handles(n), gamma=0.0, clip=10.0, eps=1e-8)
    out, den = _apply(torch, flt, twin, r, d)
    _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
    assert _same_bits(flt.state[0].cpu().numpy(), np.array([0.5, 0.0, 1e-8, K * n]))
    assert (den == 1e-8).all() and (out == 10.0).all()
    rn, _ = _dev(torch, -rew, done)                                    # (frozen on the same state: the other sign)
    out, den = flt.train(False).normalise(rn, d)
    assert (den == 1e-8).all() and (out == -10.0).all()


def _count_state(count, spread):
    """State rows of `count` samples so far with an arbitrary mean; M2 = 37.25 count (a spread of a few units) or 37.25 (next to none:
    there the merged M2 is the delta * delta term, weight and all)."""
    m2 = 37.25 * (float(count) if spread else 1.0)
    st = np.array([-3.125, m2, np.sqrt(m2 / (count - 1.0)) + 1e-8, float(count)])
    assert int(st[3]) == count
    return st


@pytest.mark.parametrize("count,spread", [(2 ** 31 + 12345, True), (2 ** 40, False)], ids=["2^31+12345", "2^40"])
def test_apply_into_a_count_past_2_31(torch_cuda, handles, count, spread):
    """A hand-written state of `count` samples, three applies of 3 x 4097: the count after is exact and differs from the one before,
    mean and M2 are the restatement's."""
    torch = torch_cuda
    n, K = 4097, 3
    state0 = _count_state(count, spread)
    flt, twin = _pair(handles(n), gamma=0.99, clip=10.0)
    flt.state[0].copy_(torch.from_numpy(state0))
    st, carry = state0, np.zeros(n)
    for t in range(3):
        rew, done = _inputs(K, n, seed=count % 9973 + t)
        rew = rew * 3.0 ** t
        r, d = _dev(torch, rew, done)
        out, den = _apply(torch, flt, twin, r, d)
        before = st[3]
        st, carry = _check(flt, st, carry, rew, done, out, den)
        assert st[3] != before
    assert int(st[3]) == count + 3 * K * n and st[3] != state0[3]


def test_one_sample_then_two(torch_cuda, handles):
    """n = 1, K = 1 from the empty state: count 1, denom 1.0, out is rew.  A second such apply: count 2 and a finite denom."""
    torch = torch_cuda
    env = handles(1)
    flt, twin = _pair(env, gamma=0.99, clip=0.0)
    rew, done = np.array([[0.75]]), np.zeros((1, 1), dtype=np.uint8)
    r, d = _dev(torch, rew, done)
    out, den = _apply(torch, flt, twin, r, d)
    st, carry = _check(flt, np.zeros(4), np.zeros(1), rew, done, out, den)
    assert _same_bits(st, np.array([0.75, 0.0, 1.0, 1.0])) and den.item() == 1.0 and _same(torch, out, r) and carry[0] == 0.75
    rew2 = np.array([[-0.25]])
    r2, _ = _dev(torch, rew2, done)
    out2, den2 = _apply(torch, flt, twin, r2, d)
    st, _ = _check(flt, st, carry, rew2, done, out2, den2)
    assert st[3] == 2.0 and np.isfinite(st[2]) and st[2] > 0.0 and st[2] != 1.0 and den2.item() == st[2]


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the frozen call and the clamp's special values
# ------------------------------------------------------------------------------------------------------------------------------------
TINY = 5e-324                                                          # the smallest subnormal
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, TINY, 1e308])
CLIPS = (0.0, 0.1, 10.0)


def _special_inputs(K, n, seed):
    """_inputs with the six special values in the first and the last row, at the first and the last envs of each (env 0 and env n - 1
    get a different one in the two rows; at K = 1 the last row's placement stands)."""
    rew, done = _inputs(K, n, seed)
    for row, shift in ((0, 0), (K - 1, 2)):
        rew[row, :6] = np.roll(SPECIALS, shift)
        rew[row, n - 6:] = np.roll(SPECIALS, shift + 3)
    return rew, done


def _frozen_case(torch, flt, rew, r, d, divisor):
    """Frozen calls at every clip on a state whose denom divides as `divisor`: out is numpy's rew / divisor, then np.clip, on the same
    f64 values, as bit patterns except for NaN-ness; dev_denom_KP reports the divisor; state and carry bytes stay."""
    K, n = rew.shape
    state, carry = flt.state.cpu().numpy().tobytes(), flt.carry.cpu().numpy().tobytes()
    nan = np.isnan(rew)
    assert nan.sum() == (2 if K > 1 else 1) * 2
    for clip in CLIPS:
        flt.clip = clip
        flt.to_native(K)
        flt.workspace.fill_(0xFF)
        out, den = flt.normalise(r, d)
        got = out.cpu().numpy()
        with np.errstate(all="ignore"):
            want = rew / divisor
            if clip > 0.0:
                want = np.clip(want, -clip, clip)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(want), nan), clip
        assert _same_bits(np.where(nan, 0.0, got), np.where(nan, 0.0, want)), clip
        assert den.shape == (K, 1) and (den == divisor).all(), clip
        assert flt.state.cpu().numpy().tobytes() == state and flt.carry.cpu().numpy().tobytes() == carry, clip
        # what that means for the special values, spelled out
        top = clip if clip > 0.0 else np.inf
        huge = min(np.inf if divisor < 0.5 else 1e308, top)             # (1e308 over a denom below 0.55 overflows)
        for value, expect in ((np.inf, top), (-np.inf, -top), (1e308, huge)):
            assert (got[rew == value] == expect).all() and (rew == value).any(), (clip, value)
        zeros = got[rew == 0.0]
        assert zeros.size and _same_bits(zeros, np.full(zeros.size, -0.0)), clip
        tiny = got[rew == TINY]
        assert tiny.size and (tiny >= TINY).all() and (tiny < 1e-300).all(), clip


@pytest.mark.parametrize("n", [257, 2049])
@pytest.mark.parametrize("K", [1, 8, 9, 1024])
def test_frozen_call_and_the_clamp_on_special_values(torch_cuda, handles, n, K):
    """K = 1, 8, 9 and 1024: one partial blockIdx.z group, one full, a second of one step, 128.  NaN stays NaN; +-inf becomes +-clip,
    or stays at clip 0; 1e308 over a denom below 0.5 overflows to inf and becomes +clip; -0.0 stays -0.0; the smallest subnormal
    over such a denom is a (larger) subnormal."""
    torch = torch_cuda
    env = handles(n)
    flt = _filter(env, gamma=0.99, clip=10.0)
    rew0, done0 = _inputs(5, n, seed=n)
    flt.normalise(*_dev(torch, 0.5 * rew0, done0))                     # a state with statistics, then frozen
    flt.train(False)
    divisor = flt.denom.item()
    assert 0.0 < divisor < 0.5 and 1e308 / divisor == np.inf and flt.carry.any()
    rew, done = _special_inputs(K, n, seed=n + K)
    r, d = _dev(torch, rew, done)
    _frozen_case(torch, flt, rew, r, d, divisor)
    # a hand-written state of count 5 and denom 0.0 divides by 1 and says so
    flt.state[0].copy_(torch.tensor([0.5, 0.0, 0.0, 5.0], dtype=torch.float64))
    _frozen_case(torch, flt, rew, r, d, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. populations
# ------------------------------------------------------------------------------------------------------------------------------------
def _three_row_chains(rew, done, gammas, eps):
    """All members of a population of three-env slices at once, from the empty state: a tile of three rows sums as (x0 + x2) + x1 (the
    halving tree meets zeros until h = 2), one tile is one run, and a run tree of one non-empty run leaves it as it is; then the
    header's merge into the state.  rew / done [K, 3 P].  Returns (count, mean [P], M2 [P], denoms [K, P])."""
    K, P = rew.shape[0], len(gammas)
    g = np.asarray(gammas, dtype=np.float64)[:, None]
    c = np.zeros((P, 3))
    cnt, mean, m2 = 0.0, np.zeros(P), np.zeros(P)
    dens = np.empty((K, P))
    for k in range(K):
        prod = c * g
        c = prod + rew[k].reshape(P, 3)
        mu = ((c[:, 0] + c[:, 2]) + c[:, 1]) / 3.0
        sq = c - mu[:, None]
        sq = sq * sq
        q = (sq[:, 0] + sq[:, 2]) + sq[:, 1]
        if cnt == 0.0:
            cnt, mean, m2 = 3.0, mu, q
        else:
            n2 = cnt + 3.0
            w = 3.0 / n2
            delta = mu - mean
            mean, m2, cnt = mean + delta * w, (m2 + q) + (delta * delta) * (cnt * w), n2
        dens[k] = np.sqrt(m2 / (cnt - 1.0)) + eps
        c = np.where(done[k].reshape(P, 3) != 0, 0.0, c)
    return cnt, mean, m2, dens


@pytest.mark.parametrize("K", [33, 1024])
def test_population_at_the_member_limit(torch_cuda, handles, K):
    """256 members of three envs with 256 different discounts.  K = 33: EVERY member against the restatement.  K = 1024 (the largest
    workspace: 1024 x 256 partials and denoms): eight members against the restatement, and every member's count, mean and M2 bit
    for bit, and its row of dev_denom_KP within 2 ulp, against the three-row chains above — which the eight members tie to the
    restatement."""
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    P, rows = N.POP_MAX_MEMBERS, 3
    assert P == 256
    env = handles(P * rows)
    gammas = [0.9 + 0.1 * m / P for m in range(P)]
    rew, done = _inputs(K, P * rows, seed=256 + K)
    r, d = _dev(torch, rew, done)
    flt, twin = _pair(env, n_members=P, gamma=gammas, clip=4.0)
    out, den = _apply(torch, flt, twin, r, d)
    assert den.shape == (K, P) and flt.count.tolist() == [float(K * rows)] * P
    members = range(P) if K == 33 else (0, 1, 100, 127, 128, 200, 254, 255)
    for m in members:
        cols = slice(m * rows, (m + 1) * rows)
        _check(flt, np.zeros(4), np.zeros(rows), rew[:, cols], done[:, cols], out, den, member=m, cols=cols)
    cnt, mean, m2, dens = _three_row_chains(rew, done, gammas, flt.eps)
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    for m in (0, 127, 255):                                            # (the chains are the restatement's, bit for bit)
        cols = slice(m * rows, (m + 1) * rows)
        st, _, _, want = ret_filter_reference(np.zeros(4), np.zeros(rows), rew[:, cols], done[:, cols], gammas[m], 4.0, flt.eps)
        assert _same_bits(dens[:, m], want) and _same_bits(st[:2], np.array([mean[m], m2[m]])) and st[3] == cnt
    state = flt.state.cpu().numpy()
    assert _same_bits(state[:, 0], mean) and _same_bits(state[:, 1], m2) and (state[:, 3] == cnt).all()
    got = den.cpu().numpy()
    assert _ulp_close(got, dens), np.abs(got - dens).max()
    assert _same_bits(state[:, 2], got[K - 1])
    assert len(set(state[:, 0].tolist())) == P                         # (the members' rows differ, so a misplaced slice shows)


def test_sliced_population_with_surplus_workgroups(torch_cuda, handles):
    """Slices of 1, 16385, 257 and 2049 envs (T = 1, 65, 2, 9; L = 1, 9, 1, 2) at K = 37 with the discounts 0, 0.9, 1 and 0.99: the
    widest slice sets the grid, so three members have surplus workgroups that write no partials; one member has runs of nine tiles
    (a second prefetch group) over two chain passes, one a single row.  Each member is the restatement on its columns and, bit for
    bit, a single-member filter on a handle of its own size fed its columns."""
    torch = torch_cuda
    sizes, gammas, K = (1, 16385, 257, 2049), (0.0, 0.9, 1.0, 0.99), 37
    assert [_geometry(n) for n in sizes] == [(1, 1), (65, 9), (2, 1), (9, 2)] and sum(sizes) == 18692
    offs = [sum(sizes[:m]) for m in range(4)]
    env = vec(sum(sizes), D)
    env.set_population_slices(sizes)
    rew, done = _inputs(K, sum(sizes), seed=37)
    r, d = _dev(torch, rew, done)
    flt, twin = _pair(env, n_members=4, gamma=list(gammas), clip=4.0)
    out, den = _apply(torch, flt, twin, r, d)
    assert den.shape == (K, 4) and flt.count.tolist() == [float(K * n) for n in sizes]
    for m, (o, n) in enumerate(zip(offs, sizes)):
        cols = slice(o, o + n)
        _check(flt, np.zeros(4), np.zeros(n), rew[:, cols], done[:, cols], out, den, member=m, cols=cols)
        sh = handles(n)
        one, single_twin = _pair(sh, gamma=gammas[m], clip=4.0)
        so, sd = _apply(torch, one, single_twin, r[:, cols].contiguous(), d[:, cols].contiguous())
        assert torch.equal(flt.state[m], one.state[0]) and torch.equal(flt.carry[cols], one.carry), m
        assert torch.equal(out[:, cols], so) and torch.equal(den[:, m], sd[:, 0]), m
    env.close()
