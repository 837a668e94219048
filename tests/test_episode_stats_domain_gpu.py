"""pop_episode_stats_kernel and pop_episode_stats_sliced_kernel over their domain (ssg_pop_episode_stats; ship_sim_gym_amd/population.py
PopulationPPO.episode_stats) on synthetic [K, N] batches (tests/accounting_support.py), the env serving as the handle only.  The
reference is ``episode_stats_walk``; the triples are compared as integers, carry_return as bytes, carry_length as integers.  Every
case calls twice, on different inputs, so the second call starts from carries in flight.

Shapes: K in {1, 2, 9}; equal layouts (N, P) = (1, 1), (256, 256), (255, 5), (771, 3), (1026, 2) — 1, 1, 51, 257 and 513 envs per
member, so one lane of one workgroup, one-lane members up to the member limit, a part of a workgroup, and two and three workgroups with
a one-env tail — and the unequal slices (1, 255, 256, 257, 513, 7).  Done patterns: p = 0 (the triple stays zero: no workgroup has an
episode to add), 0.3, 1, only each member's last env (at 513 envs the member's only episodes sit in its third workgroup), only row K - 1.
Rewards: tie (multiples of 1/8) and big (+-2^25 per step, the signs laid out by sign_by_workgroup: members with a negative total,
and members whose workgroups' partial sums have opposite signs)."""
import numpy as np
import pytest

from accounting_support import TILE, episode_stats_walk, inputs, layout, same_bits, sign_by_workgroup, tie_signs
from gpu_support import DEV, torch_cuda  # noqa: F401
from ret_filter_support import D, handles  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 2, 9)
PATTERNS = ("p0", "p0.3", "p1", "last_env", "last_row")
EQUAL = ((1, 1), (256, 256), (255, 5), (771, 3), (1026, 2))
SLICES = (1, 255, 256, 257, 513, 7)
LAYOUTS = [("N%d-P%d" % (n, p), [n // p] * p, False) for n, p in EQUAL] + [("slices", list(SLICES), True)]


def _cases(sizes):
    """Yields (what, first call's (rew, done), its (rows, carries), second call's (rew, done), its (rows, carries)) and asserts on the
    host what the inputs must hold: see the module's docstring."""
    offsets, sizes = layout(sizes)
    n_envs, P = sum(sizes), len(sizes)
    seen = {"negative": False, "wide": False, "mixed": False, "ties": [0, 0]}
    for ki, K in enumerate(KS):
        for pi, pattern in enumerate(PATTERNS):
            for fi, family in enumerate(("tie", "big")):
                what = (tuple(sizes) if P <= 6 else (sizes[0], P), K, pattern, family)
                calls, carries = [], (np.zeros(n_envs), np.zeros(n_envs, dtype=np.int32))
                returns, partials = [], []
                for call in range(2):
                    rew, done, _ = inputs(family, pattern, K, n_envs, seed=1000 * n_envs + 100 * ki + 10 * pi + 2 * fi + call + 7 * P,
                                          offsets=offsets, sizes=sizes)
                    if family == "big":
                        sign_by_workgroup(rew, offsets, sizes)
                    parts = []
                    rows, carries = episode_stats_walk(rew, done, *carries, offsets, sizes, returns=returns, partials=parts)
                    partials += [((call, m), part) for m, part in parts]
                    calls.append(((rew, done), (rows, carries)))
                total = calls[0][1][0] + calls[1][1][0]
                if pattern == "p0":
                    assert not total.any() and (carries[1] == 2 * K).all(), what
                elif pattern != "p0.3" or n_envs * K >= 64:
                    assert total[:, 2].sum() > 0, what
                if pattern in ("p1", "last_env"):
                    assert (total[:, 2] > 0).all(), what  # every member counts episodes
                if family == "tie":
                    pos, neg = tie_signs(returns)
                    seen["ties"] = [seen["ties"][0] + pos, seen["ties"][1] + neg]
                    if len(returns) >= 64:  # ties of each sign, and rounding them half away from zero gives another triple
                        assert pos > 0 and neg > 0, (what, pos, neg)
                        c0 = (np.zeros(n_envs), np.zeros(n_envs, dtype=np.int32))
                        away = episode_stats_walk(*calls[0][0], *c0, offsets, sizes, defect="half_away")
                        away2 = episode_stats_walk(*calls[1][0], *away[1], offsets, sizes, defect="half_away")
                        assert not np.array_equal(away[0] + away2[0], total), what
                if family == "big" and pattern == "p1":
                    by_member = {}
                    for m, part in partials:
                        by_member.setdefault(m, []).append(part)
                    mixed = any(min(p) < 0 < max(p) for p in by_member.values())  # within one call, the partial sums of one member
                    assert mixed == (max(sizes) > TILE), what
                    seen["mixed"] = seen["mixed"] or mixed
                    seen["negative"] = seen["negative"] or bool((total[:, 0] < 0).any())
                    if K >= 2:  # 100 * 2^25 per step: two steps of one env leave 32 bits
                        assert (np.abs(total[:, 0]) > 2 ** 32).all(), what
                        seen["wide"] = True
                yield what, calls[0][0], calls[0][1], calls[1][0], calls[1][1]
    assert seen["wide"] and seen["ties"][0] > 0 and seen["ties"][1] > 0, seen
    assert seen["mixed"] == (max(sizes) > TILE)
    # a member with a negative total: every layout but three members of 257 envs, whose 256 positive envs outweigh the one negative
    assert seen["negative"] == (set(sizes) != {257}), seen


@pytest.fixture(scope="module")
def trainers(torch_cuda, handles):
    """(env, PopulationPPO) per layout: the smallest policy the library takes (one hidden layer of 16, two actions), P members."""
    torch = torch_cuda
    from ship_sim_gym_amd.policy import NativePolicy
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    made = {}
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    src = ([(z(16, D), z(16))], (z(2, 16), z(2)), (z(1, 16), z(1)))

    def get(sizes, sliced):
        key = (tuple(sizes), sliced)
        if key not in made:
            env = handles(sum(sizes))
            env.set_population_slices(sizes if sliced else None)
            pop = NativePopulation([NativePolicy(src[0], src[1], src[2], 600.0) for _ in sizes])
            made[key] = (env, PopulationPPO(pop, env))
        return made[key]
    return get


def _batch(torch, rew, done):
    return {"rew": torch.from_numpy(np.ascontiguousarray(rew)).to(DEV), "done": torch.from_numpy(np.ascontiguousarray(done)).to(DEV)}


def _assert_call(ppo, got, rows, carries, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, rows), (what, np.argwhere(got != rows)[:4].tolist(), got[:4].tolist(), rows[:4].tolist())
    assert same_bits(ppo.carry_return.cpu().numpy(), carries[0]), ("carry_return", what)
    assert same_bits(ppo.carry_length.cpu().numpy(), carries[1]), ("carry_length", what)


@pytest.mark.parametrize("name,sizes,sliced", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_episode_stats_equal_the_walk_call_after_call(torch_cuda, trainers, name, sizes, sliced):
    torch = torch_cuda
    env, ppo = trainers(sizes, sliced)
    try:
        assert (env.population_slices == sizes) if sliced else (env.population_slices is None)
        for what, a, want_a, b, want_b in _cases(sizes):
            ppo.reset_episode_carry()
            _assert_call(ppo, ppo.episode_stats(_batch(torch, *a)), *want_a, what + ("first call",))
            _assert_call(ppo, ppo.episode_stats(_batch(torch, *b)), *want_b, what + ("second call",))
    finally:
        if sliced:
            env.set_population_slices(None)
