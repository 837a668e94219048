"""What the two GPU modules of data-parallel PPO share (tests/test_dp_gpu.py, tests/test_dp_domain_gpu.py): where the apply's words lie
in the workspace, bit-pattern comparisons, and numpy restatements of the sums the kernels make that ship_sim_gym_amd/dp.py's
references do not return (the workgroups' partial sums of squares, the re-added GAE partials).  No fixtures, no device code."""
import numpy as np

KLACC = 256 + 16  # the apply's running KL sum in the workspace: float 4 of the extended layout's first part
HEAD = 512        # the bytes DataParallelPPO keeps when the workspace grows: the statistics row and the KL part


def f32(t):
    return t.detach().cpu().numpy()


def layout(P):
    """Byte offsets of the clip sequence's gradient vector and partials in the workspace (csrc/shipsim_internal.h: ppo_ext_layout)."""
    gvec = 256 + 256
    return gvec, gvec + (4 * P + 255) // 256 * 256


def bits(a):
    """The bit patterns of an f32 / f64 array (uint32 / uint64): -0.0 differs from +0.0 and every NaN payload counts."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what, nan_ok=False):
    """got and want hold the same bits; nan_ok: the same entries are NaN (any payload) and every other entry holds the same bits."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bg, bw = bits(got), bits(want)
    if nan_ok:
        ng, nw = np.isnan(got), np.isnan(want)
        assert np.array_equal(ng, nw), (what, "NaN at", np.flatnonzero(ng != nw)[:8])
        bg, bw = bg[~ng], bw[~nw]
    if not np.array_equal(bg, bw):
        bad = np.flatnonzero(bg.reshape(-1) != bw.reshape(-1))
        keep = (~np.isnan(got)).reshape(-1) if nan_ok else np.ones(got.size, bool)
        at = np.flatnonzero(keep)[bad[:8]]
        raise AssertionError((what, "%d entries differ, first at" % bad.size, at.tolist(), got.reshape(-1)[at], want.reshape(-1)[at]))


def trees256(x):
    """The kernels' 256-entry halving tree (w = 128 .. 1: entry t += entry t + w) on every row of x (f64 [n, 256]) at once: f64 [n]."""
    x = np.array(x, dtype=np.float64).reshape(-1, 256).T.copy()
    w = 128
    while w:
        x[:w] += x[w: 2 * w]
        w >>= 1
    return x[0].copy()


def square_partials(g, stride):
    """dp_apply_kernel's f64 partials of the clip: workgroup b's tree over the squares of the combined gradient's entries 256 b ..
    256 b + 255 (zeros from P on), one per workgroup of the grid ceil(stride / 256), stride = P + 8."""
    g = np.asarray(g, dtype=np.float32)
    nb = -(-int(stride) // 256)
    sq = np.zeros(nb * 256)
    sq[:g.size] = g.astype(np.float64) ** 2
    return trees256(sq)


def norm_of_partials(part):
    """ppo_clip_kernel's norm: the partials added in index order (f64), the root rounded to f32."""
    total = 0.0
    for v in np.asarray(part, dtype=np.float64):
        total += float(v)
    with np.errstate(over="ignore"):  # (a norm past the largest f32 is +inf on the device too)
        return np.float32(np.sqrt(total))


def readd_partials(part, lanes=256):
    """dp_adv_moments_kernel / gae_stats_body on GAE's partials (f64 [nblocks, 2]): lane t adds partials t, t + 256, ... in that order
    from 0, then the halving tree over the 256 lanes.  Returns (S, Q, trips), trips the strided loop's longest trip count.
    lanes < 256: the same sums in ANOTHER order — only the first `lanes` lanes add, with that stride — for tests to assert that their
    data tells the orders apart."""
    part = np.asarray(part, dtype=np.float64).reshape(-1, 2)
    trips = -(-part.shape[0] // lanes)
    padded = np.zeros((trips * lanes, 2))
    padded[:part.shape[0]] = part
    acc = np.zeros((256, 2))
    for r in range(trips):
        acc[:lanes] += padded[r * lanes: r * lanes + lanes]
    return trees256(acc[:, 0])[0], trees256(acc[:, 1])[0], trips


def gae_inputs(K, n, seed, boot=False):
    """What GAE reads, as numpy (the same numbers wherever the test runs): rew f64, done u8, val f32 [K, n], last_val f32 [n], and with
    boot f32 [K, n]."""
    rng = np.random.RandomState(seed)
    b = dict(rew=rng.randn(K, n), done=(rng.rand(K, n) < 0.05).astype(np.uint8), val=rng.randn(K, n).astype(np.float32),
             last_val=rng.randn(n).astype(np.float32))
    if boot:
        b["boot"] = rng.randn(K, n).astype(np.float32)
    return b


def order_partials(nblocks, seed):
    """f64 [nblocks, 2] partials whose sums show the ORDER they are added in (the kernel adds what the workspace holds: no partial
    has to be a sum of squares): full 53-bit mantissas with exponents spread over 2^-8 .. 2^8 and, past one trip of the strided loop,
    a planted triple — partial 0 = +-2^60, partial 256 = -+2^60, partial 128 = 1.  Lane 0 adds partials 0 and 256 to exactly 0 and
    lane 128 keeps its 1; an order that brings partial 128 between them (a stride of 128, one lane adding everything) loses the 1 in
    2^60, so the sums differ by 1, far above their last bit.  (GAE's own partials seldom tell two orders apart: a sum of equal-scale
    f32 values is often exact in f64, and a last-bit difference in one lane is mostly absorbed by a total 256 times its size.)"""
    rng = np.random.RandomState(seed)
    part = rng.randn(nblocks, 2) * np.exp2(rng.randint(-8, 9, (nblocks, 2)).astype(np.float64))
    if nblocks > 256:
        part[0], part[256], part[128] = (2.0 ** 60, -2.0 ** 60), (-2.0 ** 60, 2.0 ** 60), (1.0, 1.0)
    return part
