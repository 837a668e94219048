"""A population against its shards, for the GPU tests of the population path.  The reference of every such test is the single-policy
path: member m is NativePolicy row m on a shard handle of its own env slice (env_id_base = the slice's offset), its update NativePPO's.
shard_rollouts() makes the population rollout and the P shard rollouts and asserts them equal; age() then makes the acting policy an
older one in both.  Set-ups are computed once per shape per module (cached) and left unchanged by the tests."""
import pytest

from gpu_support import DEV

ROLLOUT_KEYS = ("obs", "act", "logp", "val", "rew", "done", "flags")


def cols(t, m, sizes):
    """Member m's env columns of a [K, N, ...] tensor (of an [N] one: its entries)."""
    o = sum(sizes[:m])
    return t[o:o + sizes[m]] if t.dim() == 1 else t[:, o:o + sizes[m]]


def close_all(env, shards):
    env.close()
    for sh in shards:
        sh.close()


_CACHE = {}


def cached(key, make):
    """make() once per key and module; close_cached closes what it returned."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def close_cached():
    yield
    for env, pop, b, shards, refs, sbs in _CACHE.values():
        close_all(env, shards)
    _CACHE.clear()


def shard_rollouts(torch, make_env, make_members, sizes, K, seed):
    """(env, pop, batch, shard envs, reference policies, shard batches): one population rollout over sum(sizes) envs and the P
    rollouts of make_env(sizes[m], sum(sizes[:m])) under make_members(D)[m] — built alike twice, once for the population, once as the
    references.  Asserted equal here: every ROLLOUT_KEYS column slice with its dtype, the bootstrap value, the final observations, and
    ssg_pop_dist's rows against ssg_ppo_dist's, which both reproduce the rollout's logp.  Both kinds of batch leave with logp_all."""
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    from ship_sim_gym_amd.ppo import NativePPO
    sizes = list(sizes)
    env = make_env(sum(sizes), 0)
    D = env.states_history
    pop, refs = NativePopulation(make_members(D)), make_members(D)
    A = pop.n_actions
    env.reset_tensor()
    b = dict(env.rollout_population(pop, K, seed=seed))
    ppo = PopulationPPO(pop, env)
    assert ppo.member_envs == sizes
    la = ppo.dist(b)
    assert torch.equal(la.gather(-1, b["act"].long().unsqueeze(-1)).squeeze(-1), b["logp"])
    assert bool((la[..., A:] == 0).all())
    shards, sbs = [], []
    for m, n in enumerate(sizes):
        sh = make_env(n, sum(sizes[:m]))
        sh.reset_tensor()
        sb = dict(sh.rollout_policy(refs[m], K, seed=seed))
        for k in ROLLOUT_KEYS:
            assert b[k].dtype == sb[k].dtype and torch.equal(cols(b[k], m, sizes), sb[k]), (m, k)
        assert torch.equal(cols(b["last_val"], m, sizes), sb["last_val"]), m
        assert torch.equal(env.obs[sum(sizes[:m]):sum(sizes[:m + 1])], sh.obs), m
        sla = NativePPO(refs[m], sh).dist(sb)
        assert torch.equal(cols(la, m, sizes), sla), m
        assert torch.equal(sla.gather(-1, sb["act"].long().unsqueeze(-1)).squeeze(-1), sb["logp"]), m
        shards.append(sh)
        sbs.append(sb)
    if len(sizes) > 1:                                                      # the members really differ
        w = min(sizes[:2])
        assert not torch.equal(b["val"][0, :w], b["val"][0, sizes[0]:sizes[0] + w])
    return env, pop, b, shards, refs, sbs


def age(torch, b, sbs, sizes, A, la, generator, forced_dones):
    """The acting policy made an OLDER one, alike in the population's batch and the shards': the log-distribution la perturbed
    (logp_all, and logp gathered from it), the value prediction perturbed, and with forced_dones terminations mid-rollout.  The draws,
    in this order: the noise on la, the noise on val, then the forced dones."""
    K, N = b["act"].shape
    noise = 0.3 * torch.randn((K, N, A), generator=generator, device=DEV)
    vnoise = (torch.rand((K, N), generator=generator, device=DEV) - 0.5) * 0.4
    old = torch.zeros_like(la)
    old[..., :A] = torch.log_softmax(la[..., :A] + noise, -1)
    b["logp_all"] = old
    b["logp"] = old.gather(-1, b["act"].long().unsqueeze(-1)).squeeze(-1).contiguous()
    b["val"] = (b["val"] + vnoise).contiguous()
    keys = ["logp_all", "logp", "val"]
    if forced_dones:
        forced = torch.rand((K, N), generator=generator, device=DEV) < 0.05
        assert int(forced.sum()) > 0
        b["done"] = (b["done"] | forced).to(torch.uint8).contiguous()
        keys.append("done")
    for m, sb in enumerate(sbs):
        for k in keys:
            sb[k] = cols(b[k], m, sizes).contiguous()


def member_hparams(P):
    """Per-member loss / Adam constants; member 1's beta1 takes lerp's other branch."""
    return {"lr": [1e-3 / (1 + m) for m in range(P)], "clip": [0.1 + 0.05 * (m % 5) for m in range(P)],
            "ent_coef": [0.005 * (m % 4) for m in range(P)], "beta1": [0.3 if m == 1 else 0.9 - 0.02 * (m % 3) for m in range(P)],
            "lam": [0.9 + 0.02 * (m % 5) for m in range(P)]}


def shard_reference(torch, m, hp, ext, refs, shards, sbs):
    """Member m's NativePPO on its shard with its own constants and extended terms, after gae on its shard batch."""
    from ship_sim_gym_amd.ppo import NativePPO
    ref = NativePPO(refs[m], shards[m], lr=hp["lr"][m], betas=(hp["beta1"][m], 0.999), clip=hp["clip"][m], ent_coef=hp["ent_coef"][m],
                    **{k: v[m] for k, v in ext.items()})
    ref.gae(sbs[m], 0.99, hp["lam"][m])
    return ref


def stacked_perms(torch, g, P, rows, samples):
    """[P, rows, samples]: every member's permutations of equally many samples."""
    return torch.stack([torch.stack([torch.randperm(samples, device=DEV, generator=g) for _ in range(rows)]) for _ in range(P)])


def perms_per_member(torch, g, rows, samples):
    """A list of P tensors [rows, samples[m]]: member m's own permutations."""
    return [torch.stack([torch.randperm(s, device=DEV, generator=g) for _ in range(rows)]) for s in samples]
