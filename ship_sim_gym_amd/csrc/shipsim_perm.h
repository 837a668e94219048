// shipsim_perm.h — the minibatch shuffle as a counter-based permutation of [0, n) (ssg_host_perm, ssg_ppo_perm, ssg_pop_perm;
// include/shipsim.h).  Integer-only, __host__ __device__: ssg_host_perm (shipsim_api.cpp) and the kernel (shipsim_perm.hip) compile THIS
// text, and ppo.perm_reference restates it in numpy.
//
// The reference shuffles inside its update: PPO2's learn runs np.random.shuffle(inds) per epoch behind model.learn
// (train/stable_baselines/ppo.py:90), RLlib's SGD shuffles its minibatches (train/rllib/pbt.py:50-62).  Here element i of a row is a pure
// function of (seed, update, member, epoch, n, i): no sort, no scratch, no word passed between lanes, and the same bits from every
// launch geometry and entry point.  The stream is this library's own; it is not seed-compatible with numpy or torch.
//
// Construction.  b = max(kPermMinBits, ceil(log2 n)) bits, so 2^b >= n; x in [0, 2^b) is split into L (the high wl = b / 2 bits) and R
// (the low wr = b - wl bits).  One round of the alternating unbalanced Feistel network:
//     (L, R) <- (R, L ^ (F(R ^ key_r) & mask(width of L)))      and the two widths trade places,
// kPermRounds = 8 of them (an even count: the widths end where they began), F = the 32-bit multiply-xorshift finaliser perm_mix32.
// Key schedule, in uint64 arithmetic mod 2^64, mix64 = the splitmix64 finaliser (a bijection of uint64):
//     k = mix64(seed ^ kPermTag);  k = mix64(k + update);  k = mix64(k + (member << 32 | epoch));  k = mix64(k + n);
//     key_r = high 32 bits of mix64(k + (r + 1) * 0x9E3779B97F4A7C15),  r = 0 .. 7.
// Cycle walking: x = i; repeat x = network(x) until x < n.
//
// Why it is a permutation, and why the walk ends.
//  * Every round is a bijection of the 2^b domain: from (L', R') = (R, L ^ (F(R ^ key) & mask)) one recovers R = L' and
//    L = R' ^ (F(L' ^ key) & mask), whatever F is; the mask keeps L' ^ ... inside the width of L.  So the network N is a permutation of
//    [0, 2^b), and its cycles are closed.
//  * Start at i < n and follow i's cycle of N.  The cycle returns to i itself, which is below n, so the walk meets a point below n
//    after at most (cycle length) applications; every point it passes before that is >= n and all are distinct, and there are only
//    2^b - n such points: at most 2^b - n + 1 applications.
//  * The map i -> first point below n after i on i's cycle is a bijection of [0, n): it is the cycle of N with the points >= n struck
//    out, which is again a cycle.  So every row is an exact permutation.
//  * Above the floor 2^(b-1) < n, so the domain is below 2n: fewer than half of its points lie outside [0, n), and the expected number
//    of applications is below 2.
//
// The cap.  The loop stops after kPermWalkCap = 256 applications and returns -1, which the gradient kernels treat as a zero,
// gradient-free sample: whatever the rounds compute, a lane leaves after 256 of them — a wrong round cannot hang a device.  At the
// floor width the cap IS the bound above (2^8 - n + 1 <= 256 for n >= 1), so a bijection cannot reach it there.  Above the floor the
// bound 2^b - n + 1 is far larger than any useful cap; there the walk passes only points >= n, which are fewer than half of the
// domain, and for a network that mixes (which the uniformity tests of tests/test_perm.py are about) 256 such points in a row have a
// chance below 2^-256 per element.  That is an argument from the round function's quality, not from bijectivity alone; the tests assert
// that no -1 appears at every size they draw, and the longest walks seen are recorded in profiles/perm/README.md.
#ifndef SHIPSIM_PERM_H
#define SHIPSIM_PERM_H

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define SSG_PERM_HD __host__ __device__ __forceinline__
#else
#define SSG_PERM_HD inline
#endif

namespace ssg {

constexpr int kPermRounds = 8, kPermMinBits = 8, kPermWalkCap = 256;
constexpr uint64_t kPermMaxN = 1ull << 32;              // 1 <= n <= 2^32
constexpr uint64_t kPermTag = 0x5353475045524D31ull;    // "SSGPERM1"
constexpr uint64_t kPermGolden = 0x9E3779B97F4A7C15ull;

struct PermKey {
    uint32_t k[kPermRounds];
    uint64_t n;
    int wl, wr; // widths of L (high) and R (low); wl + wr = b
};

SSG_PERM_HD uint64_t perm_mix64(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

SSG_PERM_HD uint32_t perm_mix32(uint32_t v)
{
    v ^= v >> 16;
    v *= 0x85EBCA6Bu;
    v ^= v >> 13;
    v *= 0xC2B2AE35u;
    v ^= v >> 16;
    return v;
}

// the smallest b >= kPermMinBits with 2^b >= n (n in 1 .. 2^32: b in 8 .. 32)
SSG_PERM_HD int perm_bits(uint64_t n)
{
    int b = kPermMinBits;
    while (b < 32 && (1ull << b) < n) ++b;
    return b;
}

SSG_PERM_HD PermKey perm_key(uint64_t seed, uint64_t update, uint32_t member, uint32_t epoch, uint64_t n)
{
    PermKey key;
    uint64_t k = perm_mix64(seed ^ kPermTag);
    k = perm_mix64(k + update);
    k = perm_mix64(k + (((uint64_t)member << 32) | (uint64_t)epoch));
    k = perm_mix64(k + n);
    for (int r = 0; r < kPermRounds; ++r) key.k[r] = (uint32_t)(perm_mix64(k + (uint64_t)(r + 1) * kPermGolden) >> 32);
    key.n = n;
    const int b = perm_bits(n);
    key.wl = b / 2;
    key.wr = b - key.wl;
    return key;
}

// one application of the network to x in [0, 2^b)
SSG_PERM_HD uint32_t perm_network(const PermKey &key, uint32_t x)
{
    uint32_t ml = (1u << key.wl) - 1u, mr = (1u << key.wr) - 1u; // (wl, wr <= 16)
    uint32_t L = x >> key.wr, R = x & mr;
#pragma unroll
    for (int r = 0; r < kPermRounds; ++r) {
        const uint32_t t = L ^ (perm_mix32(R ^ key.k[r]) & ml);
        L = R;
        R = t;
        const uint32_t m = ml;
        ml = mr;
        mr = m;
    }
    return (L << key.wr) | R; // (an even number of rounds: the widths are back where they began)
}

// element i (< n) of the row: the cycle walk; -1 when the cap is reached (see the top)
SSG_PERM_HD int64_t perm_at(const PermKey &key, uint32_t i)
{
    uint32_t x = i;
    for (int it = 0; it < kPermWalkCap; ++it) {
        x = perm_network(key, x);
        if ((uint64_t)x < key.n) return (int64_t)x;
    }
    return -1;
}

// What one launch fills (shipsim_perm.hip): rows r = m * epochs + e, m < members, e < epochs, keyed (seed, update, member0 + m, e).
// slices NULL: every row has n entries and starts r * n entries into out.  Else the device table of ssg_pop_set_slices: member m's rows
// have K * n_m entries and start epochs * K * o_m + e * K * n_m entries in (o_m: its first env = the envs of the members before it);
// n is then the widest row, K * max n_m, and sizes the grid alone.
struct PermLaunch {
    uint64_t seed, update;
    int member0, members, epochs;
    long long n, K;
    const int32_t *slices;
    int64_t *out;
};
// (plain types, so that a host-only program can include this header: the hipError_t as an int, the hipStream_t as a pointer)
int launch_perm(const PermLaunch &l, void *stream);

} // namespace ssg

#endif /* SHIPSIM_PERM_H */
