"""What the return filter's test modules share (tests/test_ret_filter_gpu.py, tests/test_ret_filter_domain_gpu.py and the CPU checks of
tests/test_ret_filter.py): the synthetic [K, n] inputs, the device copies on a padded row pitch, the comparison rule against
``ret_filter_reference``, the handles fixture (imported by name into each GPU module, which pytest then collects as that module's own),
and, for the checks that do not lean on the restatement, the samples of the documented recurrence and a batch's M2 with its tiles
merged in one sequential run.  Nothing here needs a device at import."""
import numpy as np
import pytest

from gpu_support import DEV, vec

D = 7
TILE, RUNS = 256, 8


def _inputs(K, n, seed):
    """(rew f64 [K, n], done u8 [K, n]) in numpy."""
    rng = np.random.RandomState(seed)
    rew = rng.choice([-0.01, 1.0, -1.0], size=(K, n), p=[0.9, 0.05, 0.05])
    rew[:, rng.randint(n)] = rng.uniform(-2.0, 2.0, K)
    done = (rng.random_sample((K, n)) < 0.05).astype(np.uint8)
    if n >= 2:
        done[:, 0], done[:, n - 1] = 0, 1
    return rew, done


def _ramp_inputs(K, n, seed):
    """_inputs with the last step's rewards a noisy ramp over the env index, 0.37 e + U(0, 1): the tiles' means of that batch then lie
    far apart against the spread inside a tile, so the delta * delta * (n * (n_b / n')) term carries M2 at every merge of tiles and of
    runs, and the association of those merges shows in M2's last bits."""
    rew, done = _inputs(K, n, seed)
    rew[K - 1] = 0.37 * np.arange(n) + np.random.RandomState(seed + 1).random_sample(n)
    return rew, done


def _ill_inputs(K, n, seed):
    """Ill-conditioned returns (at gamma = 0 the samples are the rewards): the exact values j 2^-10 + 2^20, j a uniform integer in
    -1024..1024, with _inputs' dones."""
    rng = np.random.RandomState(seed)
    return rng.randint(-1024, 1025, (K, n)) * 2.0 ** -10 + 2.0 ** 20, _inputs(K, n, seed)[1]


def _samples(carry, rew, done, gamma):
    """The header's walk, elementwise in f64 (c = c * gamma + rew[k]: the product, then the sum; the sample; c = 0 where done[k] != 0):
    the samples s [K, n] and the carry after the last row.  Every implementation of the recurrence gives these bits."""
    c = np.array(carry, dtype=np.float64)
    g = np.float64(gamma)
    s = np.empty(np.shape(rew))
    for k in range(len(rew)):
        prod = c * g
        c = prod + rew[k]
        s[k] = c
        c = np.where(np.asarray(done[k]) != 0, 0.0, c)
    return s, c


def _geometry(n):
    """(T tiles, L tiles per run) of a member of n rows."""
    T = -(-n // TILE)
    return T, -(-T // RUNS)


def _sequential_m2(x):
    """The M2 of one batch x [n] with the device's tile partials (two halving trees per 256-row tile) but ALL tiles merged in one
    sequential run in tile order: no eight runs and no tree over them.  Scalar Python floats, the header's merge."""
    cnt = mean = m2 = 0.0

    def tree(v):
        v = list(v) + [0.0] * (TILE - len(v))
        h = TILE // 2
        while h:
            v = [v[i] + v[i + h] for i in range(h)]
            h //= 2
        return v[0]

    for t in range(0, len(x), TILE):
        rows = [float(v) for v in x[t:t + TILE]]
        nt = float(len(rows))
        mu = tree(rows) / nt
        q = tree([(v - mu) * (v - mu) for v in rows])
        if cnt == 0.0:
            cnt, mean, m2 = nt, mu, q
        else:
            n2 = cnt + nt
            w = nt / n2
            d = mu - mean
            mean, m2, cnt = mean + d * w, (m2 + q) + (d * d) * (cnt * w), n2
    return m2


def _dev(torch, rew, done, pad=0):
    """The device copies, as [:, :n] views of buffers with a row pitch of n + pad (the padding holds NaN / 0xFF)."""
    K, n = rew.shape
    r = torch.full((K, n + pad), float("nan"), dtype=torch.float64, device=DEV)
    d = torch.full((K, n + pad), 0xFF, dtype=torch.uint8, device=DEV)
    r[:, :n] = torch.from_numpy(rew).to(DEV)
    d[:, :n] = torch.from_numpy(done).to(DEV)
    return r[:, :n], d[:, :n]


def _filter(env, **kw):
    from ship_sim_gym_amd.ret_filter import ReturnFilter
    return ReturnFilter(env, **kw)


def _ulp_close(got, want, ulps=2):
    return np.all(np.abs(got - want) <= ulps * np.spacing(np.abs(want)))


def _same_bits(got, want):
    """Equal as bit patterns: -0.0 is not 0.0, and a NaN equals itself."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def _check(flt, state0, carry0, rew, done, out, denom, member=0, cols=None, gamma=None):
    """One member's results of an updating apply against ret_filter_reference.  state0 [4] / carry0 [n_m]: what the member had before;
    rew / done: numpy [K, n_m], the member's columns; out / denom: the device's.  Returns (state, carry) of the device (numpy)."""
    from ship_sim_gym_amd.ret_filter import ret_filter_reference
    cols = slice(0, rew.shape[1]) if cols is None else cols
    gamma = flt.gamma[member] if gamma is None else gamma
    want_state, want_carry, _, want_den = ret_filter_reference(state0, carry0, rew, done, gamma, flt.clip, flt.eps)
    st, carry = flt.state[member].cpu().numpy(), flt.carry[cols].cpu().numpy()
    den = denom[:, member].cpu().numpy()
    got = out[:, cols].cpu().numpy()
    assert st[3] == want_state[3] == state0[3] + rew.size, (st[3], want_state[3])
    assert _same_bits(st[:2], want_state[:2]), (st, want_state)
    assert _same_bits(carry, want_carry)
    assert _ulp_close(den, want_den), np.abs(den - want_den).max()
    own = np.sqrt(st[1] / (st[3] - 1.0)) + flt.eps if st[3] >= 2 else 1.0
    assert _ulp_close(st[2], own) and st[2] == den[-1], (st[2], own, den[-1])
    want = rew / den[:, None]
    if flt.clip > 0.0:
        want = np.clip(want, -flt.clip, flt.clip)
    assert _same_bits(got, want), np.abs(got - want).max()
    return st, carry


@pytest.fixture(scope="module")
def handles(torch_cuda):
    """One handle per env count of the module (an env is the handle only: nothing here steps it)."""
    made = {}

    def get(n):
        if n not in made:
            made[n] = vec(n, D)
        return made[n]
    yield get
    for env in made.values():
        env.close()
