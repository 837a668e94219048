"""GPU checks of the return filter (ssg_ret_filter_apply; ship_sim_gym_amd/ret_filter.py).  The inputs are synthetic [K, N] tensors, not
env physics — rewards drawn from {-0.01, 1, -1} with one column of random f64, dones at about 5 %, env 0 never done and the last env
done at every step — and an env serves as the handle only.  The reference is ``ret_filter_reference`` (the numpy restatement of the
walk and of the device's reduction order): count, mean, M2 and the carry bit for bit; every denom_k within 2 ulp of the restatement's
(numpy's square root of the same M2_k: the observation filter's tolerance, for the same square root), the state's own denom within
2 ulp of the value formed from the device's own M2; out bit for bit clamp(rew / denom_k) formed from the device's own denom_k.

Shapes: n in {1, 2, 255, 256, 257, 769} (one env, below / at / above the 256-env tile, four tiles of which one a tail) x K in {1, 2, 5}
(below, half of and above the four-step staging); n = 2049 and 4097 at K = 3 (runs of 2 and 3 tiles, empty runs, a one-row tail tile);
K = 9 on a row pitch of n + 5 (two full stagings and one step, padded rows).  The inputs, the comparison rule and the handles fixture
live in tests/ret_filter_support.py; the rest of the domain — every pass count of the three launches up to K = 1024, runs of more than
eight tiles, the value edges, the member limit — is in tests/test_ret_filter_domain_gpu.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gpu_support import DEV, ROOT, torch_cuda, vec  # noqa: F401
from ppo_reference import actor_critic_policy
from ret_filter_support import D, _check, _dev, _filter, _inputs, handles  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(n, K, 0) for n in (1, 2, 255, 256, 257, 769) for K in (1, 2, 5)] + [(2049, 3, 0), (4097, 3, 0), (257, 9, 5)]


@pytest.mark.parametrize("n,K,pad", SHAPES, ids=["n%d-K%d%s" % (n, K, "-pad%d" % p if p else "") for n, K, p in SHAPES])
def test_apply_is_the_restatement_bit_for_bit(torch_cuda, handles, n, K, pad):
    torch = torch_cuda
    env = handles(n)
    rew, done = _inputs(K, n, seed=1000 * n + K)
    r, d = _dev(torch, rew, done, pad)
    results = []
    for fill in (0xFF, 0x00):                                          # the workspace's contents do not enter the result
        flt = _filter(env, gamma=0.99, clip=10.0, eps=1e-8)
        flt.to_native(K)
        flt.workspace.fill_(fill)
        out, den = flt.normalise(r, d)
        assert out.stride(0) == n + pad and den.shape == (K, 1)
        st, carry = _check(flt, np.zeros(4), np.zeros(n), rew, done, out, den)
        if n >= 2:
            assert carry[n - 1] == 0.0 and carry[0] != 0.0             # done at every step / never done
        # a second rollout on the running state, the carry in flight
        rew2, done2 = _inputs(K, n, seed=1000 * n + K + 500)
        r2, d2 = _dev(torch, rew2 * 3.0, done2, pad)
        out2, den2 = flt.normalise(r2, d2)
        _check(flt, st, carry, rew2 * 3.0, done2, out2, den2)
        results.append((flt.state.clone(), flt.carry.clone(), out.clone(), out2.clone(), den2.clone()))
        assert torch.equal(r[:, :n].cpu(), torch.from_numpy(rew))      # the raw rewards stay
    for a, b in zip(*results):
        assert torch.equal(a, b)
    if pad:                                                            # the padding columns were neither read into anything nor written
        base = torch.full((K, n + pad), -7.0, dtype=torch.float64, device=DEV)
        # (normalise allocates its own output: call the library on a buffer whose padding is known)
        import ctypes as C
        from ship_sim_gym_amd import _native as N
        flt = _filter(env)
        rec = flt.to_native(K)
        N.check(N.lib().ssg_ret_filter_apply(env._h, C.byref(rec), K, C.c_void_p(r.data_ptr()), C.c_void_p(d.data_ptr()), n + pad,
                                             C.c_void_p(base.data_ptr()), None, env._stream()), env._h, "ssg_ret_filter_apply")
        assert (base[:, n:] == -7.0).all() and torch.equal(base[:, :n], results[0][2])


@pytest.mark.parametrize("n,K1,K2", [(257, 3, 4), (769, 1, 6), (2049, 2, 1)])
def test_two_applies_continue_as_one(torch_cuda, handles, n, K1, K2):
    torch = torch_cuda
    env = handles(n)
    rew, done = _inputs(K1 + K2, n, seed=77 + n)
    r, d = _dev(torch, rew, done)
    one = _filter(env, gamma=0.95, clip=1.0)
    out, den = one.normalise(r, d)
    two = _filter(env, gamma=0.95, clip=1.0)
    oa, da = two.normalise(r[:K1], d[:K1])
    ob, db = two.normalise(r[K1:], d[K1:])
    assert torch.equal(one.state, two.state) and torch.equal(one.carry, two.carry)
    assert torch.equal(out, torch.cat([oa, ob])) and torch.equal(den, torch.cat([da, db]))
    assert (out.abs() == 1.0).any() and (out.abs() < 1.0).any()       # (the clip bites at the events: the denom is below 1)


@pytest.mark.parametrize("n", [257, 2049])
def test_frozen_leaves_state_and_carry(torch_cuda, handles, n):
    torch = torch_cuda
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    env = handles(n)
    K = 5
    rew, done = _inputs(K, n, seed=n)
    r, d = _dev(torch, rew, done)
    # the empty state: the rewards come back as they are (clip 0), or clamped
    flt = _filter(env, clip=0.0, update=False)
    out, den = flt.normalise(r, d)
    assert torch.equal(out, r) and (den == 1.0).all() and not flt.state.any() and not flt.carry.any()
    flt.clip = 0.5
    out, _ = flt.normalise(r, d)
    assert torch.equal(out, r.clamp(-0.5, 0.5)) and (out.abs() == 0.5).any()
    # a state with statistics
    flt = _filter(env, clip=0.0)
    flt.normalise(r, d)
    state, carry = flt.state.clone(), flt.carry.clone()
    assert carry.any() and flt.count.item() == K * n
    flt.train(False)
    flt.workspace.fill_(0xFF)
    for clip in (0.0, 1.0):                                            # the denom is below 1: a clip of 1 bites at the events
        flt.clip = clip
        rew2, done2 = _inputs(K, n, seed=n + 1)
        r2, d2 = _dev(torch, rew2, done2)
        out, den = flt.normalise(r2, d2)
        assert state.cpu().numpy().tobytes() == flt.state.cpu().numpy().tobytes()
        assert carry.cpu().numpy().tobytes() == flt.carry.cpu().numpy().tobytes()
        dd = state[0, 2].item()
        assert (den == dd).all() and 0.0 < dd < 1.0
        want = rew2 / dd
        if clip:
            want = np.clip(want, -clip, clip)
            assert (np.abs(want) == clip).any() and (np.abs(want) < clip).any()
        assert np.array_equal(out.cpu().numpy(), want)
        ref = ret_filter_reference(state[0].cpu().numpy(), carry.cpu().numpy(), rew2, done2, 0.99, clip, flt.eps, update=False)
        assert np.array_equal(ref[2], want)
    flt.train(True)                                                    # ... and updating again it moves on from where it was
    flt.clip = 10.0
    out, den = flt.normalise(r, d)
    _check(flt, state[0].cpu().numpy(), carry.cpu().numpy(), rew, done, out, den)


POPULATIONS = [("equal", 3, None, 771), ("sliced", 3, (2049, 300, 4700), 7049), ("many", 256, None, 768)]


@pytest.mark.parametrize("name,P,sizes,N_", POPULATIONS, ids=[p[0] for p in POPULATIONS])
def test_population_members_are_single_member_filters(torch_cuda, handles, name, P, sizes, N_):
    torch = torch_cuda
    K = 3
    env = vec(N_, D)
    if sizes is not None:
        env.set_population_slices(sizes)
    sz = list(sizes) if sizes is not None else [N_ // P] * P
    offs = [sum(sz[:m]) for m in range(P)]
    gammas = [0.9 + 0.1 * m / P for m in range(P)]                     # per-member discounts, all different
    rew, done = _inputs(K, N_, seed=P)
    rew2, done2 = _inputs(K, N_, seed=P + 1)
    r, d = _dev(torch, rew, done)
    r2, d2 = _dev(torch, rew2, done2)
    flt = _filter(env, n_members=P, gamma=gammas, clip=4.0)
    out, den = flt.normalise(r, d)
    out2, den2 = flt.normalise(r2, d2)
    assert flt.count.tolist() == [float(2 * K * s) for s in sz] and den.shape == (K, P)
    # every member is a single-member filter on a handle of n_m envs fed its columns (for the 256 members: eight of them)
    for m in (range(P) if P <= 8 else (0, 1, 100, 127, 128, 200, 254, 255)):
        o, n = offs[m], sz[m]
        sh = handles(n)
        one = _filter(sh, gamma=gammas[m], clip=4.0)
        so, sd = one.normalise(r[:, o:o + n].contiguous(), d[:, o:o + n].contiguous())
        so2, sd2 = one.normalise(r2[:, o:o + n].contiguous(), d2[:, o:o + n].contiguous())
        assert torch.equal(flt.state[m], one.state[0]) and torch.equal(flt.carry[o:o + n], one.carry), m
        assert torch.equal(out[:, o:o + n], so) and torch.equal(out2[:, o:o + n], so2), m
        assert torch.equal(den[:, m], sd[:, 0]) and torch.equal(den2[:, m], sd2[:, 0]), m
    # ... and the restatement, for the first and the last member
    for m in (0, P - 1):
        o, n = offs[m], sz[m]
        a = _filter(handles(n), gamma=gammas[m], clip=4.0)             # (only its settings are read)
        from ship_sim_gym_amd.ret_filter import ret_filter_reference
        st, carry, _, _ = ret_filter_reference(np.zeros(4), np.zeros(n), rew[:, o:o + n], done[:, o:o + n], gammas[m], 4.0, a.eps)
        _check(flt, st, carry, rew2[:, o:o + n], done2[:, o:o + n], out2, den2, member=m, cols=slice(o, o + n))
    env.close()


def _batch(torch, K, n, seed):
    rew, done = _inputs(K, n, seed)
    g = torch.Generator(device=DEV).manual_seed(seed)
    return dict(rew=torch.from_numpy(rew).to(DEV), done=torch.from_numpy(done).to(DEV),
                val=torch.randn((K, n), generator=g, device=DEV), last_val=torch.randn((n,), generator=g, device=DEV))


def test_gae_runs_on_the_normalised_rewards(torch_cuda, handles):
    torch = torch_cuda
    from ship_sim_gym_amd.ppo import NativePPO
    n, K = 769, 5
    env = handles(n)
    ppo = NativePPO(actor_critic_policy(torch, D, seed=3)[1], env)
    b = _batch(torch, K, n, seed=21)
    raw = b["rew"].clone()
    plain = [t.clone() for t in ppo.gae(dict(b), 0.97, 0.9)]           # a batch no filter ever touched
    flt = _filter(env, gamma=0.97)
    adv, ret = ppo.gae(b, 0.97, 0.9, return_filter=flt)
    assert torch.equal(b["rew"], raw) and b["rew_norm"].shape == (K, n) and b["rew_denom"].shape == (K, 1) and flt.count.item() == K * n
    twin = _filter(env, gamma=0.97)
    want = twin.normalise(raw, b["done"])[0]
    assert torch.equal(b["rew_norm"], want) and not torch.equal(want, raw)
    c = dict(b, rew=want.clone())
    for k in ("adv", "ret", "rew_norm", "rew_denom"):
        del c[k]
    adv2, ret2 = ppo.gae(c, 0.97, 0.9)
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2) and not torch.equal(adv, plain[0])
    # without the argument nothing changes, whatever the batch carries by now
    adv3, ret3 = ppo.gae(b, 0.97, 0.9)
    assert torch.equal(adv3, plain[0]) and torch.equal(ret3, plain[1]) and flt.count.item() == K * n


def test_population_gae_and_exploit(torch_cuda):
    torch = torch_cuda
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    P, n, K = 3, 257, 4
    env = vec(P * n, D)
    pop = NativePopulation([actor_critic_policy(torch, D, seed=50 + m)[1] for m in range(P)])
    gammas = [0.9, 0.95, 0.99]
    ppo = PopulationPPO(pop, env, gamma=gammas)
    b = _batch(torch, K, P * n, seed=8)
    raw = b["rew"].clone()
    plain = [t.clone() for t in ppo.gae(dict(b))]
    flt = _filter(env, n_members=P, gamma=gammas)
    adv, ret = ppo.gae(b, return_filter=flt)
    assert torch.equal(b["rew"], raw) and flt.count.tolist() == [float(K * n)] * P
    want = _filter(env, n_members=P, gamma=gammas).normalise(raw, b["done"])[0]
    assert torch.equal(b["rew_norm"], want)
    adv2, ret2 = ppo.gae(dict(rew=want.clone(), done=b["done"], val=b["val"], last_val=b["last_val"]))
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2) and not torch.equal(adv, plain[0])
    adv3, ret3 = ppo.gae(b)
    assert torch.equal(adv3, plain[0]) and torch.equal(ret3, plain[1])
    # exploit: exactly the source's rows of the registered filter, the carries stay; an unregistered filter is not touched
    other = _filter(env, n_members=P, gamma=gammas)
    other.state.copy_(flt.state)
    before, carry = flt.state.clone(), flt.carry.clone()
    assert carry.any() and not torch.equal(before[0], before[1]) and not torch.equal(before[1], before[2])
    with pytest.raises(ValueError):
        ppo.set_return_filter(_filter(env, n_members=1))
    ppo.set_return_filter(flt)
    ppo.exploit([1, 1, 2])
    assert torch.equal(flt.state[0], before[1]) and torch.equal(flt.state[1], before[1]) and torch.equal(flt.state[2], before[2])
    assert torch.equal(flt.carry, carry) and torch.equal(other.state, before)
    ppo.set_return_filter(None)
    ppo.exploit([2, 1, 2])
    assert torch.equal(flt.state[0], before[1])
    env.close()


def test_refusals_launch_nothing(torch_cuda, handles):
    torch = torch_cuda
    import ctypes as C
    from ship_sim_gym_amd import _native as N
    n, K = 300, 4
    env = handles(n)
    rew, done = _inputs(K, n, seed=2)
    r, d = _dev(torch, rew, done)
    flt = _filter(env)
    flt.normalise(r, d)
    state, carry = flt.state.clone(), flt.carry.clone()
    out = torch.full((K, n), -7.0, dtype=torch.float64, device=DEV)
    L, h = N.lib(), env._h

    def call(rec, K=K, rew=r.data_ptr(), stride=n, out=out.data_ptr()):
        return L.ssg_ret_filter_apply(h, C.byref(rec), K, C.c_void_p(rew), C.c_void_p(d.data_ptr()), stride, C.c_void_p(out), None,
                                      env._stream())

    for kw in (dict(struct_size=8), dict(flags=2), dict(n_members=0), dict(n_members=7), dict(clip=-1.0), dict(eps=float("nan")),
               dict(dev_gamma=None), dict(dev_state=None), dict(dev_carry=None), dict(dev_workspace=None), dict(workspace_nbytes=8)):
        rec = flt.to_native(K)
        for k, v in kw.items():
            setattr(rec, k, v)
        assert call(rec) == -1, kw
    rec = flt.to_native(K)
    assert call(rec, K=0) == -1 and call(rec, K=K + 1) == -1 and call(rec, stride=n - 1) == -1 and call(rec, out=r.data_ptr()) == -1
    assert call(rec, rew=None) == -1 and call(rec, out=None) == -1
    torch.cuda.synchronize()
    assert torch.equal(flt.state, state) and torch.equal(flt.carry, carry) and (out == -7.0).all()
    for bad in (r.float(), r[:, :-1], r.t()):
        with pytest.raises(ValueError):
            flt.normalise(bad, d)


def _run(args, timeout):
    return subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_ppo_script_runs_with_norm_reward(torch_cuda):
    out = _run([os.path.join(ROOT, "train", "ppo_torch.py"), "--mode", "native", "--update", "native", "--norm-reward", "--envs", "256",
                "--updates", "2", "--horizon", "8"], 300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = re.findall(r"policy loss (\S+)\s+value loss (\S+)\s+entropy (\S+)\s+\(return filter: (\d+) returns merged, std (\S+)\)", out.stdout)
    assert len(rows) == 2 and all(np.isfinite(float(v)) for row in rows for v in row), out.stdout
    assert [int(row[3]) for row in rows] == [256 * 8, 2 * 256 * 8] and all(float(row[4]) > 0.0 for row in rows)


def test_pbt_script_runs_with_norm_reward(torch_cuda):
    out = _run([os.path.join(ROOT, "train", "pbt_native.py"), "--members", "3", "--envs-per-member", "64", "--updates", "2", "--horizon", "8",
                "--perturb-every", "1", "--norm-reward"], 300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "update 2  episode_reward_mean" in out.stdout, out.stdout
    m = re.search(r"return filter: returns merged per member \[(\d+), (\d+), (\d+)\]  std \[(.*?)\]", out.stdout)
    assert m and [int(m.group(i)) for i in (1, 2, 3)] == [2 * 64 * 8] * 3, out.stdout
    stds = [float(s.strip("' ")) for s in m.group(4).split(",")]
    assert len(stds) == 3 and all(np.isfinite(s) and s > 0.0 for s in stds), out.stdout
