"""GPU checks of the episode log (ssg_episode_log_append; ship_sim_gym_amd/episode_log.py).  The inputs are synthetic [K, N] buffers — rew
drawn from {1, -1, -0.01}, done Bernoulli(p) or a pattern, flags with an ending at every done step and goal events between — and an env
serves as the handle only, but for the one real run at the end.  The reference is ``episode_log_reference``; every comparison is of
bytes: the ring, the head and both carries.

Shapes: N in {1, 63, 64, 65, 255, 256, 257, 513} (one env; below / at / above a wave; below / at / above the 256-env tile; two tiles and
a one-env tail) x K in {1, 2, 5}; per shape the done patterns p = 0, 0.3, 1, "only the last lane of each tile" and "only row K-1", each
at the capacities 1, count - 1, count, count + 1 and a prime below count, where count is what the two calls of a case end together.
Longer blocks — K at and above the walk's eight-row staging, K * tiles above the scan's 1 024-cell pass — have a test of their own."""
import ctypes as C

import numpy as np
import pytest

from gpu_support import DEV, env_config, torch_cuda  # noqa: F401
from ppo_reference import actor_critic_policy
from ret_filter_support import handles  # noqa: F401

pytestmark = pytest.mark.gpu

GOAL, ENDS = 0x2, np.array([0x1, 0x4, 0x8, 0x10, 0x1 | 0x4, 0x2 | 0x10], dtype=np.uint8)
PATTERNS = ("p0", "p0.3", "p1", "last_lane", "last_row")


def _inputs(K, n, pattern, seed):
    """(rew f64, done u8, flags u8) [K, n] in numpy."""
    rng = np.random.RandomState(seed)
    rew = rng.choice([1.0, -1.0, -0.01], size=(K, n))
    if pattern == "last_lane":  # env 255, 511, ... and the handle's last env
        done = np.zeros((K, n), dtype=np.uint8)
        done[:, 255::256] = 1
        done[:, n - 1] = 1
    elif pattern == "last_row":
        done = np.zeros((K, n), dtype=np.uint8)
        done[K - 1] = rng.random_sample(n) < 0.5
        done[K - 1, rng.randint(n)] = 1
    else:
        done = (rng.random_sample((K, n)) < float(pattern[1:])).astype(np.uint8)
    flags = np.where(done != 0, ENDS[rng.randint(0, len(ENDS), size=(K, n))], np.where(rng.random_sample((K, n)) < 0.2, GOAL, 0)).astype(np.uint8)
    return rew, done, flags


def _dev(torch, arrays, pad=0):
    """Device copies as [:, :n] views of buffers with a row pitch of n + pad (the padding holds NaN / 0xFF: a done byte there would count)."""
    out = []
    for a in arrays:
        K, n = a.shape
        t = torch.full((K, n + pad), float("nan") if a.dtype == np.float64 else 0xFF, dtype=torch.float64 if a.dtype == np.float64 else torch.uint8,
                       device=DEV)
        t[:, :n] = torch.from_numpy(a).to(DEV)
        out.append(t[:, :n])
    return out


def _log(env, cap, members=1, fill=0xAB):
    """A log whose ring holds a known pattern (a slot no rank owns keeps it) and whose workspace holds garbage."""
    from ship_sim_gym_amd.episode_log import EpisodeLog
    log = EpisodeLog(env, capacity=cap, n_members=members)
    log.ring.fill_(fill)
    return log


class _Ref(object):
    """The numpy side of a log: what episode_log_reference leaves, call after call."""

    def __init__(self, n, cap, fill=0xAB, env_base=0, members=None):
        from ship_sim_gym_amd.episode_log import RECORD_DTYPE
        self.ring = np.full(cap * 32, fill, dtype=np.uint8).view(RECORD_DTYPE).copy()
        self.head, self.cret, self.c = np.zeros(2, dtype=np.int64), np.zeros(n), np.zeros((n, 2), dtype=np.int32)
        self.steps, self.env_base, self.members = 0, env_base, members

    def append(self, rew, done, flags):
        from ship_sim_gym_amd.episode_log import episode_log_reference
        self.ring, self.head, self.cret, self.c = episode_log_reference(rew, done, flags, self.cret, self.c, self.head, self.ring, step0=self.steps,
                                                                        env_base=self.env_base, members=self.members)
        self.steps += rew.shape[0]
        return self


def _same(log, ref, what=""):
    """Ring, head and both carries, byte for byte."""
    got = log.ring.cpu().numpy().tobytes(), log.head.cpu().numpy(), log.carry_return.cpu().numpy(), log.carry.cpu().numpy()
    assert got[0] == ref.ring.tobytes(), ("ring", what)
    assert got[1].tolist() == ref.head.tolist(), ("head", what, got[1], ref.head)
    assert got[2].tobytes() == ref.cret.tobytes(), ("carry_return", what)
    assert got[3].tobytes() == ref.c.tobytes(), ("carry", what)
    assert log.steps == ref.steps


def _prime_below(x):
    for p in range(x - 1, 1, -1):
        if all(p % q for q in range(2, int(p ** 0.5) + 1)):
            return p
    return 1


SHAPES = [(n, K) for n in (1, 63, 64, 65, 255, 256, 257, 513) for K in (1, 2, 5)]


@pytest.mark.parametrize("n,K", SHAPES, ids=["n%d-K%d" % s for s in SHAPES])
def test_append_is_the_reference_byte_for_byte(torch_cuda, handles, n, K):
    torch = torch_cuda
    env = handles(n)
    for pi, pattern in enumerate(PATTERNS):
        a = _inputs(K, n, pattern, seed=1000 * n + 10 * K + pi)
        b = _inputs(K, n, pattern, seed=1000 * n + 10 * K + pi + 5)
        count = int(np.count_nonzero(a[1]) + np.count_nonzero(b[1]))
        da, db = _dev(torch, a), _dev(torch, b)
        caps = sorted({max(1, c) for c in (1, count - 1, count, count + 1, _prime_below(count))})
        for cap in caps:
            log, ref = _log(env, cap), _Ref(n, cap)
            log.to_native(K)
            log.workspace.fill_(0xFF)  # (the workspace's contents do not enter the result)
            log.append_rows(*da)
            _same(log, ref.append(*a), (pattern, cap, "first call"))
            log.append_rows(*db)       # the carries in flight, the head where the first call left it
            _same(log, ref.append(*b), (pattern, cap, "second call"))
            assert int(ref.head[0]) == count and int(ref.head[1]) == int(np.count_nonzero(b[1]))
        if pattern == "p0":
            assert count == 0 and ref.ring.view(np.uint8).min() == 0xAB and ref.c[:, 0].tolist() == [2 * K] * n
        if pattern == "p1":
            assert count == 2 * K * n and not ref.cret.any() and not ref.c.any()


# the walk stages 8 rows per barrier (two LDS buffers in turn) and the scan takes 1 024 cells per pass (two buffers in turn): K at, one
# above and two chunks above the staging, and 9 tiles x 230 rows = 2 070 cells = three passes of which the last is partial
LONG = [(257, 8, "p0.3"), (257, 9, "p0.3"), (65, 17, "p1"), (513, 25, "last_lane"), (2049, 230, "p0.02")]


@pytest.mark.parametrize("n,K,pattern", LONG, ids=["n%d-K%d-%s" % s for s in LONG])
def test_blocks_longer_than_one_chunk_of_rows_and_one_pass_of_cells(torch_cuda, handles, n, K, pattern):
    torch = torch_cuda
    env = handles(n)
    a = _inputs(K, n, pattern, seed=n + K)
    d = _dev(torch, a)
    count = int(np.count_nonzero(a[1]))
    assert count > 64
    for cap in (count + 3, _prime_below(count // 2)):
        log, ref = _log(env, cap), _Ref(n, cap)
        log.to_native(K)
        log.workspace.fill_(0xFF)
        log.append_rows(*d)
        _same(log, ref.append(*a), (cap, "first call"))
        log.append_rows(*d)
        _same(log, ref.append(*a), (cap, "second call"))


@pytest.mark.parametrize("n,K,pad", [(257, 5, 7), (65, 3, 1)])
def test_a_padded_row_pitch_and_an_env_id_base(torch_cuda, n, K, pad):
    torch = torch_cuda
    from gpu_support import vec
    env = vec(n, 7, base=1000)
    a = _inputs(K, n, "p0.3", seed=n + K)
    d = _dev(torch, a, pad)
    assert d[0].stride(0) == n + pad
    log, ref = _log(env, 4096), _Ref(n, 4096, env_base=1000)
    log.append_rows(*d)
    _same(log, ref.append(*a))
    rec, dropped = log.records()
    tt, ee = np.nonzero(a[1])
    assert dropped == 0 and rec["step"].tolist() == tt.tolist() and rec["env"].tolist() == (ee + 1000).tolist()  # np.nonzero's order
    env.close()


@pytest.mark.parametrize("n,K1,K2,cap", [(257, 2, 3, 4096), (257, 2, 3, 7), (513, 1, 4, 101), (64, 4, 1, 1), (255, 3, 3, 50)])
def test_two_calls_leave_what_one_call_leaves(torch_cuda, handles, n, K1, K2, cap):
    torch = torch_cuda
    env = handles(n)
    a = _inputs(K1 + K2, n, "p0.3", seed=3 * n + K1)
    d = _dev(torch, a)
    one, two = _log(env, cap), _log(env, cap)
    one.append_rows(*d)
    two.append_rows(*[t[:K1] for t in d])
    first = int(np.count_nonzero(a[1][:K1]))
    if cap < 4096:
        assert first > cap  # (the first call alone wraps the ring)
    two.append_rows(*[t[K1:] for t in d])
    assert torch.equal(one.ring, two.ring) and one.head[0].item() == two.head[0].item() == int(np.count_nonzero(a[1]))
    assert torch.equal(one.carry_return, two.carry_return) and torch.equal(one.carry, two.carry)
    assert two.head[1].item() == int(np.count_nonzero(a[1][K1:])) and one.steps == two.steps == K1 + K2
    _same(one, _Ref(n, cap).append(*a))


def test_three_calls_beyond_the_capacity_between_reads_drop_an_exact_count(torch_cuda, handles):
    torch = torch_cuda
    n, K, cap = 257, 3, 300
    env = handles(n)
    log, big = _log(env, cap), _Ref(n, 1 << 16)
    blocks = [_inputs(K, n, "p0.3", seed=40 + i) for i in range(4)]
    log.append_rows(*_dev(torch, blocks[0]))
    big.append(*blocks[0])
    rec, dropped = log.records()
    seen = int(big.head[0])
    assert dropped == 0 and seen <= cap and np.array_equal(rec, big.ring[:seen])
    for blk in blocks[1:]:
        log.append_rows(*_dev(torch, blk))
        big.append(*blk)
    total = int(big.head[0])
    assert total - seen > cap
    rec, dropped = log.records(since=seen)
    assert dropped == total - cap - seen and np.array_equal(rec, big.ring[total - cap:total]) and log.total() == total
    assert log.mean_last(100) == float(np.mean(big.ring["ret"][total - 100:total]))
    assert log.end_counts(rec)["episodes"] == cap


@pytest.mark.parametrize("sizes", [(128, 128, 128, 128), (64, 128, 64, 256)], ids=["equal", "unequal"])
def test_members_change_the_member_bits_and_nothing_else(torch_cuda, sizes):
    torch = torch_cuda
    from gpu_support import vec
    from ship_sim_gym_amd.episode_log import member_of_envs, record_member
    from ship_sim_gym_amd.population import NativePopulation, PopulationPPO
    n, K, P = 512, 5, 4
    env = vec(n, 7)
    blocks = [_inputs(K, n, "p0.3", seed=70 + i) for i in range(2)]
    devs = [_dev(torch, blk) for blk in blocks]
    plain = _log(env, 8192)  # one member, nothing bound
    for d in devs:
        plain.append_rows(*d)
    equal = len(set(sizes)) == 1
    if not equal:
        env.set_population_slices(sizes)
    members = member_of_envs(n, P, None if equal else sizes)
    log, ref = _log(env, 8192, members=P), _Ref(n, 8192, members=members)
    ppo = PopulationPPO(NativePopulation([actor_critic_policy(torch, 7, seed=100 + m)[1] for m in range(P)]), env)
    triple = torch.zeros((P, 3), dtype=torch.int64, device=DEV)
    for blk, d in zip(blocks, devs):
        log.append_rows(*d)
        ref.append(*blk)
        triple += ppo.episode_stats({"rew": d[0].contiguous(), "done": d[1].contiguous()})
    _same(log, ref)
    rec, _ = log.records()
    base, _ = plain.records()
    assert rec.shape == base.shape and rec.shape[0] == int(plain.head[0].item()) > 4 * 64
    got = record_member(rec)
    assert got.tolist() == members[rec["env"]].tolist() and set(got.tolist()) == set(range(P))
    for name in ("ret", "step", "env", "length", "goals"):
        assert rec[name].tobytes() == base[name].tobytes(), name
    assert (rec["end"] & 0xff).tobytes() == base["end"].tobytes() and not (base["end"] >> 8).any()
    assert torch.equal(log.carry_return, plain.carry_return) and torch.equal(log.carry, plain.carry) and torch.equal(log.head, plain.head)
    # per member: the sums over the log are ssg_pop_episode_stats' triple on the same batches, exactly
    want = triple.cpu().tolist()
    for m in range(P):
        mine = rec[got == m]
        assert [int(np.sum(np.rint(100.0 * mine["ret"]).astype(np.int64))), int(mine["length"].sum()), int(mine.shape[0])] == want[m], m
    if not equal:  # a member count that the bound layout is not for is refused, head and ring as they were
        bad = _log(env, 64, members=2)
        with pytest.raises(Exception, match="slices for 4 members"):
            bad.append_rows(*devs[0])
        assert not bad.head.any() and (bad.ring == 0xAB).all()
        env.set_population_slices(None)
    env.close()


def test_without_flags_goals_and_the_low_byte_of_end_are_zero(torch_cuda, handles):
    torch = torch_cuda
    n, K = 257, 5
    env = handles(n)
    a = _inputs(K, n, "p0.3", seed=9)
    d = _dev(torch, a)
    log, ref = _log(env, 4096), _Ref(n, 4096)
    log.append_rows(d[0], d[1], None)
    _same(log, ref.append(a[0], a[1], None))
    rec, _ = log.records()
    assert rec.shape[0] > 100 and not rec["goals"].any() and not rec["end"].any() and not log.carry[:, 1].any()
    with_flags = _log(env, 4096)
    with_flags.append_rows(*d)
    rf, _ = with_flags.records()
    assert rf["goals"].any() and rf["end"].all() and rf["ret"].tobytes() == rec["ret"].tobytes() and rf["length"].tobytes() == rec["length"].tobytes()


def test_every_refusal_is_bad_arg_and_leaves_head_and_ring(torch_cuda, handles):
    torch = torch_cuda
    from ship_sim_gym_amd import _native as N
    n, K = 257, 3
    env = handles(n)
    a = _inputs(K, n, "p1", seed=5)
    rew, done, flags = _dev(torch, a)
    log = _log(env, 64)
    good = log.to_native(K)
    L, h = N.lib(), env._h
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(rec=good, K=K, rew=vp(rew), done=vp(done), flags=vp(flags), stride=n, handle=h):
        return L.ssg_episode_log_append(handle, C.byref(rec) if rec is not None else None, K, 0, rew, done, flags, stride, env._stream())

    def changed(**kw):
        rec = N.EpisodeLogRecord.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(rec, k, v)
        return rec

    cases = {"a NULL handle": dict(handle=None), "a NULL record": dict(rec=None), "struct_size": dict(rec=changed(struct_size=8)),
             "capacity 0": dict(rec=changed(capacity=0)), "capacity < 0": dict(rec=changed(capacity=-5)),
             "n_members 0": dict(rec=changed(n_members=0)), "n_members 257": dict(rec=changed(n_members=N.POP_MAX_MEMBERS + 1)),
             "n_members that does not divide": dict(rec=changed(n_members=2)),
             "K 0": dict(K=0), "K < 0": dict(K=-1), "stride < n_envs": dict(stride=n - 1), "NULL reward": dict(rew=None), "NULL done": dict(done=None),
             "K * tiles above the bound": dict(K=N.EPISODE_LOG_MAX_CELLS // 2 + 1),
             "workspace too small": dict(rec=changed(workspace_nbytes=good.workspace_nbytes - 1)),
             "records not 16-byte aligned": dict(rec=changed(dev_records=good.dev_records + 8)),
             "carry not 8-byte aligned": dict(rec=changed(dev_carry=good.dev_carry + 4))}
    for field in ("dev_records", "dev_head", "dev_carry_return", "dev_carry", "dev_workspace"):
        cases["NULL " + field] = dict(rec=changed(**{field: None}))
    assert good.workspace_nbytes == 16 + 4 * K * 2
    for what, kw in cases.items():
        assert call(**kw) == -1, what
        if kw.get("handle", h) is not None:
            assert b"ssg_episode_log_append" in L.ssg_last_error(h), what
    torch.cuda.synchronize()
    assert not log.head.any() and (log.ring == 0xAB).all() and not log.carry.any() and not log.carry_return.any()
    assert call() == 0  # (the record the refusals were cut from is a good one)
    torch.cuda.synchronize()
    assert log.head.tolist() == [K * n, K * n]
    # the workspace call's own refusals are the CPU module's; here: an unbound handle is NOT_BOUND, after the arguments
    cfg = N.default_config()
    cfg.n_envs = n
    h2 = C.c_void_p()
    N.check(L.ssg_create(C.byref(cfg), C.byref(h2)))
    assert call(handle=h2) == -3 and call(handle=h2, K=0) == -1
    L.ssg_destroy(h2)


def test_a_real_run_is_the_numpy_walk_over_its_batches(torch_cuda):
    """256 envs with a step limit of 9, two rollouts of 16 steps through rollout_policy: every env times out at least three times."""
    torch = torch_cuda
    from ship_sim_gym_amd.vec_env import ShipVecEnv
    env = ShipVecEnv(256, n_maps=8, n_beams=1, env_config=env_config(1, max_steps=9))
    assert env.cfg.max_steps == 9 and env.states_history == 7
    env.reset_tensor()
    _, pol = actor_critic_policy(torch, 7, seed=1)
    log, ref = _log(env, 4096), _Ref(256, 4096)
    for i in range(2):
        b = env.rollout_policy(pol, 16, seed=5, step0=16 * i)
        log.append(b)
        ref.append(*[b[k].cpu().numpy() for k in ("rew", "done", "flags")])
    _same(log, ref)
    rec, dropped = log.records()
    assert dropped == 0 and rec.shape[0] == int(ref.head[0]) >= 3 * 256 and rec["length"].max() <= 9 and rec["length"].min() >= 1
    assert log.mean_last(100) == float(np.mean(ref.ring["ret"][:rec.shape[0]][-100:]))
    counts = log.end_counts(rec)
    assert counts["max_steps"] > 0 and counts["episodes"] == rec.shape[0] == env.stats()["episodes"]
    assert abs(float(np.sum(rec["ret"])) - env.stats()["sum_return"]) < 1e-6 * rec.shape[0]
    assert log.timesteps(rec).tolist() == ((rec["step"] + 1) * 256).tolist() and rec["step"].max() <= 31
    env.close()
