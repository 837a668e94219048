"""GPU checks of the minibatch permutations drawn on the device (ssg_ppo_perm / ssg_pop_perm; NativePPO / PopulationPPO with perm_seed;
--perm native of the trainers): every row bit for bit the numpy restatement and an exact permutation, nothing written outside the
buffer, the keying, the population layouts on equal and unequal slices against the single call per member, the refusal of a member
count the bound slices do not have, update(perm=None) against update(draw_perm()) on twins, and the trainers run to run."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, load_script, vec
from gpu_support import torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy, synthetic_batch

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -0x5EED5EED
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 100003)
_ENVS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_envs():
    yield
    for env in _ENVS.values():
        env.close()
    _ENVS.clear()


def _env(n, tag=""):
    """One handle per env count (and tag) at obs_dim 7."""
    if (n, tag) not in _ENVS:
        _ENVS[(n, tag)] = vec(n, 7)
    return _ENVS[(n, tag)]


def _guarded(torch, entries):
    """(the whole buffer, its inner `entries` entries): int64, 64 guard entries of a sentinel on each side, the inside sentinel too."""
    buf = torch.full((entries + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    return buf, buf[GUARD: GUARD + entries]


def _guards_untouched(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _stream_ptr(torch, stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream(DEV)).cuda_stream)


def _ppo_perm(torch, env, seed, update, member, epochs, n, stream=None):
    """ssg_ppo_perm into a guarded buffer: numpy int64 [epochs, n]; asserts the guards."""
    from ship_sim_gym_amd import _native as N
    buf, inner = _guarded(torch, epochs * n)
    with torch.cuda.device(DEV):
        N.check(N.lib().ssg_ppo_perm(env._h, seed, update, member, epochs, n, C.c_void_p(inner.data_ptr()), _stream_ptr(torch, stream)),
                env._h, "ssg_ppo_perm")
    torch.cuda.synchronize()
    assert _guards_untouched(buf), (n, epochs)
    return inner.view(epochs, n).cpu().numpy()


def _pop_perm(torch, env, seed, update, members, K, n, perm_epochs, entries):
    from ship_sim_gym_amd import _native as N
    buf, inner = _guarded(torch, entries)
    with torch.cuda.device(DEV):
        N.check(N.lib().ssg_pop_perm(env._h, seed, update, members, K, n, perm_epochs, C.c_void_p(inner.data_ptr()), _stream_ptr(torch)),
                env._h, "ssg_pop_perm")
    torch.cuda.synchronize()
    assert _guards_untouched(buf)
    return inner.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. one policy's rows
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epochs", (1, 3))
@pytest.mark.parametrize("n", SIZES)
def test_rows_are_bitwise_the_restatement_and_exact_permutations(torch_cuda, n, epochs):
    """A lane takes 2 elements, a wave 128, a block 512: one lane and a lone tail element (1, 3), a wave's edge (127 .. 129), a block's
    edge (511 .. 513), 8 blocks and a ninth (4 095 .. 4 097), 196 blocks (100 003), and the sizes in between.  Odd n with 3 epochs puts
    rows at addresses that are no multiple of 16 bytes, where the kernel stores 8 bytes at a time."""
    from ship_sim_gym_amd.ppo import perm_reference
    torch = torch_cuda
    seed, update, member = 0xC0FFEE + n, 5, 2
    rows = _ppo_perm(torch, _env(256), seed, update, member, epochs, n)
    assert rows.dtype == np.int64 and rows.shape == (epochs, n)
    assert rows.min() >= 0                                                   # no -1: the walk's cap was never reached
    for e in range(epochs):
        assert np.array_equal(rows[e], perm_reference(seed, update, member, e, n)), (n, e)
        assert np.array_equal(np.sort(rows[e]), np.arange(n)), (n, e)


def test_rows_follow_their_key_and_nothing_else(torch_cuda):
    from ship_sim_gym_amd.ppo import perm_reference
    torch = torch_cuda
    env, n, epochs = _env(256), 4097, 2
    base = _ppo_perm(torch, env, 9, 1, 0, epochs, n)
    side = torch.cuda.Stream(device=DEV)
    assert np.array_equal(_ppo_perm(torch, env, 9, 1, 0, epochs, n, stream=side), base)         # another stream: the same rows
    assert np.array_equal(_ppo_perm(torch, _env(384), 9, 1, 0, epochs, n), base)                 # another handle: the same rows
    assert np.array_equal(_ppo_perm(torch, env, 9, 1, 0, 1, n)[0], base[0])                      # fewer epochs: a prefix
    for key in ((9, 1, 1), (9, 2, 0), (10, 1, 0)):                                               # member, update, seed
        other = _ppo_perm(torch, env, key[0], key[1], key[2], epochs, n)
        assert not np.array_equal(other[0], base[0]) and int((other[0] == base[0]).sum()) <= 12, key
        assert np.array_equal(other[1], perm_reference(key[0], key[1], key[2], 1, n)), key
    assert not np.array_equal(base[0], base[1])                                                  # the epoch


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. a population's layouts
# ------------------------------------------------------------------------------------------------------------------------------------
def test_population_layout_on_equal_slices(torch_cuda):
    torch = torch_cuda
    env, P, K, n, E = _env(384), 3, 3, 130, 2
    flat = _pop_perm(torch, env, 21, 4, P, K, n, E, P * E * K * n).reshape(P, E, K * n)
    for m in range(P):
        assert np.array_equal(flat[m], _ppo_perm(torch, env, 21, 4, m, E, K * n)), m


def test_population_layout_on_unequal_slices_and_the_member_refusal(torch_cuda):
    from ship_sim_gym_amd import _native as N
    torch = torch_cuda
    env, sizes, K, E = _env(384), (64, 192, 128), 3, 2
    env.set_population_slices(list(sizes))
    try:
        flat = _pop_perm(torch, env, 21, 4, 3, K, 999, E, E * K * 384)        # (n is not read with slices bound)
        for m, n_m in enumerate(sizes):
            start = E * K * sum(sizes[:m])                                   # perm_epochs x the samples of the members before
            block = flat[start: start + E * K * n_m].reshape(E, K * n_m)
            assert np.array_equal(block, _ppo_perm(torch, env, 21, 4, m, E, K * n_m)), m
        buf, inner = _guarded(torch, E * K * 384)
        for members in (2, 4):
            rc = N.lib().ssg_pop_perm(env._h, 21, 4, members, K, 128, E, C.c_void_p(inner.data_ptr()), _stream_ptr(torch))
            assert rc == -1 and b"slices for 3 members" in N.lib().ssg_last_error(env._h), members
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())                                 # nothing was launched
    finally:
        env.set_population_slices(None)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. plumbing: update(perm=None) is update(draw_perm())
# ------------------------------------------------------------------------------------------------------------------------------------
K4, N4, EPOCHS, MINIBATCHES, SEED = 4, 256, 2, 2, 1234


def _single(torch, perm_seed, batch_seed=3, member=0, env_tag=""):
    from ship_sim_gym_amd.ppo import NativePPO
    _, pol = actor_critic_policy(torch, 7, 16, 1, "tanh", 3, seed=1)
    ppo = NativePPO(pol, _env(N4, env_tag), perm_seed=perm_seed, member=member)
    b = synthetic_batch(torch, pol, K4, N4, batch_seed)
    ppo.gae(b)
    return pol, ppo, b


def test_native_ppo_draws_its_own_permutations(torch_cuda):
    from ship_sim_gym_amd.ppo import perm_reference
    torch = torch_cuda
    n = K4 * N4
    pol_a, a, ba = _single(torch, SEED)
    pol_b, b, bb = _single(torch, SEED)
    pol_c, c, bc = _single(torch, SEED + 1)
    drawn = b.draw_perm(bb, EPOCHS)
    assert drawn.shape == (EPOCHS, n) and drawn.dtype == torch.int64
    assert np.array_equal(drawn.cpu().numpy(), np.stack([perm_reference(SEED, 0, 0, e, n) for e in range(EPOCHS)]))
    assert torch.equal(b.draw_perm(n, EPOCHS, out=torch.empty_like(drawn)), drawn)
    a.update(ba, None, EPOCHS, MINIBATCHES)
    b.update(bb, drawn, EPOCHS, MINIBATCHES)
    c.update(bc, None, EPOCHS, MINIBATCHES)
    assert (a.updates, b.updates, a.step) == (1, 1, EPOCHS * MINIBATCHES)
    assert torch.equal(pol_a.params, pol_b.params) and torch.equal(a.adam_mv, b.adam_mv)
    assert not torch.equal(pol_a.params, pol_c.params)                       # another seed, other minibatches
    second = b.draw_perm(bb, EPOCHS)                                          # the second update's rows are others
    assert not torch.equal(second, drawn)
    assert np.array_equal(second[1].cpu().numpy(), perm_reference(SEED, 1, 0, 1, n))
    a.update(ba, None, EPOCHS, MINIBATCHES)
    b.update(bb, second, EPOCHS, MINIBATCHES)
    assert torch.equal(pol_a.params, pol_b.params) and torch.equal(a.adam_mv, b.adam_mv) and a.updates == 2
    a.updates = 0                                                            # a checkpoint may set the count: the first rows again
    assert torch.equal(a.draw_perm(n, EPOCHS), drawn)
    with pytest.raises(ValueError, match="perm_seed"):
        _single(torch, None)[1].update(ba, None, EPOCHS, MINIBATCHES)


def _population(torch, sizes, perm_seed):
    """(env, PopulationPPO, batch, member twins [(policy, NativePPO, shard batch)]) on the 256-env handle, gae done on both sides."""
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    P = len(sizes)
    members = lambda: [actor_critic_policy(torch, 7, 16, 1, "tanh", 3, seed=100 + m)[1] for m in range(P)]  # noqa: E731
    env = _env(N4, "population")
    env.set_population_slices(list(sizes) if len(set(sizes)) > 1 else None)
    pop, refs = NativePopulation(members()), members()
    b = synthetic_batch(torch, refs[0], K4, N4, 8)
    ppo = PopulationPPO(pop, env, perm_seed=perm_seed)
    ppo.gae(b)
    twins = []
    for m in range(P):
        o = sum(sizes[:m])
        sb = {k: (v[o:o + sizes[m]] if v.dim() == 1 else v[:, o:o + sizes[m]]).contiguous() for k, v in b.items() if k not in ("adv", "ret")}
        ref = NativePPO(refs[m], _env(N4), perm_seed=perm_seed, member=m)
        ref.gae(sb)
        twins.append((refs[m], ref, sb))
    return env, pop, ppo, b, twins


@pytest.mark.parametrize("sizes", ((64, 64, 64, 64), (64, 128, 64)), ids=("equal", "unequal"))
def test_population_draws_every_members_own_permutations(torch_cuda, sizes):
    torch = torch_cuda
    P = len(sizes)
    env, pop, ppo, b, twins = _population(torch, sizes, SEED)
    try:
        drawn = ppo.draw_perm(b, EPOCHS)
        if len(set(sizes)) == 1:
            assert drawn.shape == (P, EPOCHS, K4 * sizes[0])
            blocks = [drawn[m] for m in range(P)]
        else:
            assert drawn.shape == (EPOCHS * K4 * N4,)
            starts = [EPOCHS * K4 * sum(sizes[:m]) for m in range(P)]
            blocks = [drawn[s: s + EPOCHS * K4 * n_m].view(EPOCHS, K4 * n_m) for s, n_m in zip(starts, sizes)]
        for m, (pol, ref, sb) in enumerate(twins):
            assert torch.equal(blocks[m], ref.draw_perm(sb, EPOCHS)), m
        ppo.update(b, None, EPOCHS, MINIBATCHES)
        for m, (pol, ref, sb) in enumerate(twins):
            ref.update(sb, None, EPOCHS, MINIBATCHES)
            assert torch.equal(pop.params[m], pol.params), (m, "params")
            assert torch.equal(ppo.adam_mv[m], ref.adam_mv), (m, "moments")
        assert ppo.updates == 1
        again = ppo.draw_perm(b, EPOCHS)                                       # the second update's permutations are others
        assert again.shape == drawn.shape and not torch.equal(again, drawn)
        if len(set(sizes)) > 1:                                              # a re-slice between updates: draw_perm follows the env
            env.set_population_slices([128, 64, 64])
            moved = ppo.draw_perm(b, EPOCHS)
            assert torch.equal(moved[:EPOCHS * K4 * 128].view(EPOCHS, K4 * 128), twins[0][1].draw_perm(K4 * 128, EPOCHS))
        first = pop.params.clone()
        env2, pop2, ppo2, b2, _ = _population(torch, sizes, SEED + 1)        # another seed: other minibatches, other parameters
        ppo2.update(b2, None, EPOCHS, MINIBATCHES)
        assert not torch.equal(pop2.params, first)
    finally:
        env.set_population_slices(None)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the trainers
# ------------------------------------------------------------------------------------------------------------------------------------
def test_ppo_torch_with_native_permutations_is_reproducible(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/ppo_torch.py")
    kw = dict(envs=256, updates=2, horizon=8, mode="native", update="native", perm="native", return_details=True, log=lambda s: None)
    _, one = mod.train(**kw)
    _, two = mod.train(**kw)
    assert all(bool(torch.isfinite(p).all()) for p in one["params"])
    assert all(torch.equal(p, q) for p, q in zip(one["params"], two["params"]))
    _, other = mod.train(**dict(kw, perm="torch"))
    assert any(not torch.equal(p, q) for p, q in zip(one["params"], other["params"]))           # the flag reaches the update


def test_pbt_native_with_native_permutations_is_reproducible(torch_cuda):
    torch = torch_cuda
    mod = load_script("train/pbt_native.py")
    kw = dict(members=4, envs_per_member=64, updates=2, horizon=8, perturb_every=1, perm="native", return_details=True, log=lambda s: None)
    _, one = mod.train(**kw)
    _, two = mod.train(**kw)
    assert bool(torch.isfinite(one["params"]).all()) and torch.equal(one["params"], two["params"])
