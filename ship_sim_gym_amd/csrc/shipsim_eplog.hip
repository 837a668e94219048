// shipsim_eplog.hip — the episode log: ssg_episode_log_append (include/shipsim.h), in an object of its own so that every other
// object's device code stays what it is.
//
// What Monitor does on the host for one env (train/stable_baselines/ppo.py:7-8,38-40: one (r, l, t) row per finished episode), for the
// [K][N] reward / done / flags rows of a rollout on the device: every episode that ends in the block becomes one 32-byte record in the
// caller's ring, at the slot its RANK decides — rank = position in np.nonzero(done), (t ascending, env ascending).  The rank comes
// from a count per (row, 256-env tile), an exclusive scan of those counts by one workgroup, and a ballot prefix inside the tile: all
// integers, so there is nothing to round, no atomics, and the result does not depend on the launch geometry.
//
// Workspace: int64 [2] = (the head before the call, the call's count), then int32 [K * tiles] = the counts, scanned in place.
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kLogTile = 256, kLogWaves = kLogTile / 64;
static_assert(sizeof(ssg_episode_record) == 32, "a record is two 16-byte stores");

// (a) grid (K * tiles): workgroup b counts the done bytes of row t = b / tiles, tile = b % tiles.
__global__ void __launch_bounds__(kLogTile) eplog_count_kernel(int N, int tiles, size_t stride, const uint8_t *__restrict__ done,
                                                               int32_t *__restrict__ counts)
{
    __shared__ int wcnt[kLogWaves];
    const int t = blockIdx.x / tiles, tile = blockIdx.x - t * tiles;
    const int e = tile * kLogTile + (int)threadIdx.x;
    const bool d = e < N && done[(size_t)t * stride + e] != 0;
    const unsigned long long m = __ballot(d);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// (b) one workgroup: counts[0 .. cells) -> its exclusive prefix sums, in place, in passes of 4 * 256 cells: lane i of a pass owns cells
// [4 i, 4 i + 4) of it (consecutive lanes read consecutive 16 bytes), the lanes' sums are scanned inside each wave by shuffles and across
// the four waves through LDS, and the passes chain through a running total.  The next pass's loads are issued before this pass's
// barrier.  Integers: any order gives the same bits, this one is simply fixed.  Then the header and the head.
constexpr int kScanPer = 4, kScanPass = kScanPer * kLogTile;

__device__ __forceinline__ void scan_load(const int32_t *__restrict__ counts, int cells, int first, int (&v)[kScanPer])
{
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) v[j] = first + j < cells ? counts[first + j] : 0;
}

__global__ void __launch_bounds__(kLogTile) eplog_scan_kernel(int cells, int32_t *__restrict__ counts, long long *__restrict__ hdr,
                                                              long long *__restrict__ head)
{
    __shared__ int wsum[2][kLogWaves];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int total = 0, v[kScanPer], nxt[kScanPer];
    scan_load(counts, cells, (int)threadIdx.x * kScanPer, v);
    for (int p0 = 0, pass = 0; p0 < cells; p0 += kScanPass, ++pass) {
        const int first = p0 + (int)threadIdx.x * kScanPer;
        scan_load(counts, cells, first + kScanPass, nxt); // (all zeros past the last pass)
        const int mine = v[0] + v[1] + v[2] + v[3];
        int incl = mine; // inclusive scan of `mine` over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[pass & 1][w] = incl;
        __syncthreads(); // (one per pass: pass + 2 writes this buffer after the barrier of pass + 1, which follows every read of it here)
        int acc = total + incl - mine;
        for (int u = 0; u < w; ++u) acc += wsum[pass & 1][u];
        total += wsum[pass & 1][0] + wsum[pass & 1][1] + wsum[pass & 1][2] + wsum[pass & 1][3];
#pragma unroll
        for (int j = 0; j < kScanPer; ++j) {
            if (first + j < cells) counts[first + j] = acc;
            acc += v[j];
            v[j] = nxt[j];
        }
    }
    if (threadIdx.x == 0) {
        const long long old = head[0];
        hdr[0] = old;
        hdr[1] = total;
        head[0] = old + total;
        head[1] = total;
    }
}

struct LogWalk {
    int K, N, tiles;
    size_t stride;
    long long step0, env_base, capacity;
    int members, n;           // the member layout: equal slices of n envs, or ...
    const int32_t *slices;    // ... the bound table (nullable)
    const double *rew;
    const uint8_t *done, *flags; // flags nullable
    double *carry_ret;
    int2 *carry;
    const long long *hdr;
    const int32_t *base;      // the scanned counts
    uint4 *records;
};

// (c) grid (tiles): one lane per env, kLogRows rows at a time.  A lane first loads its done, reward and flags entries of the chunk's rows
// (independent loads, in flight together: a row at a time the walk is K dependent memory round trips), every wave leaves its done
// count of each row in cnt[chunk & 1][row][wave], and after ONE barrier per chunk the rows are walked in order: a lane's rank within the
// tile is the counts of the waves before its own plus the done lanes below it in its wave.  Every lane of the workgroup runs every chunk
// (lanes past N carry done = false), because of the barrier; the loads themselves are unconditional — a lane past N reads the handle's
// last env and a row past K the block's last row, both valid memory whose values are dropped — so that nothing waits between them.
// FLAGS: whether the caller gave a flags buffer.  Two buffers: a wave writes chunk c + 2's counts only after the barrier of
// chunk c + 1, which every wave reaches after reading chunk c's.
constexpr int kLogRows = 8;

template <bool FLAGS>
__global__ void __launch_bounds__(kLogTile) eplog_walk_kernel(const LogWalk a)
{
    __shared__ int cnt[2][kLogRows][kLogWaves];
    const int tile = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = tile * kLogTile + (int)threadIdx.x;
    const bool live = e < a.N;
    const size_t col = (size_t)(live ? e : a.N - 1); // the column this lane loads
    int member = 0;
    if (live && a.members > 1) {
        if (a.slices) { // the last row whose first env is <= e
            int lo = 0, hi = a.members - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (a.slices[(size_t)mid * SSG_POP_SLICE_ROW] <= e) lo = mid;
                else hi = mid - 1;
            }
            member = lo;
        } else
            member = e / a.n;
    }
    const long long head = a.hdr[0], count = a.hdr[1];
    const long long skip = count > a.capacity ? count - a.capacity : 0;
    double cum = a.carry_ret[col];
    int2 c = a.carry[col];
    for (int t0 = 0, chunk = 0; t0 < a.K; t0 += kLogRows, ++chunk) {
        const int rows = min(kLogRows, a.K - t0); // (uniform)
        double rw[kLogRows];
        unsigned fl[kLogRows];
        uint8_t db[kLogRows];
        bool dn[kLogRows];
#pragma unroll
        for (int j = 0; j < kLogRows; ++j) {
            const size_t i = (size_t)min(t0 + j, a.K - 1) * a.stride + col;
            rw[j] = a.rew[i];
            db[j] = a.done[i];
            fl[j] = FLAGS ? a.flags[i] : 0u;
        }
        unsigned long long m[kLogRows];
#pragma unroll
        for (int j = 0; j < kLogRows; ++j) {
            dn[j] = live && j < rows && db[j] != 0;
            m[j] = __ballot(dn[j]);
            if (lane == 0) cnt[chunk & 1][j][w] = __popcll(m[j]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLogRows; ++j) {
            if (live && j < rows) {
                cum += rw[j];
                c.x += 1;
                c.y += (fl[j] & SSG_EV_GOAL_REACHED) ? 1 : 0;
            }
            if (dn[j]) { // (false for j >= rows and for lanes past N)
                const int t = t0 + j;
                int r = a.base[(size_t)t * a.tiles + tile] + __popcll(m[j] & ((1ull << lane) - 1ull));
                for (int v = 0; v < w; ++v) r += cnt[chunk & 1][j][v];
                if ((long long)r >= skip) {
                    const long long slot = (head + (long long)r) % a.capacity;
                    const long long step = a.step0 + t;
                    uint4 q0, q1;
                    q0.x = (unsigned)__double2loint(cum);
                    q0.y = (unsigned)__double2hiint(cum);
                    q0.z = (unsigned)((unsigned long long)step & 0xffffffffull);
                    q0.w = (unsigned)((unsigned long long)step >> 32);
                    q1.x = (unsigned)(int)(a.env_base + e);
                    q1.y = (unsigned)c.x;
                    q1.z = (unsigned)c.y;
                    q1.w = (fl[j] & 0xffu) | ((unsigned)member << 8);
                    a.records[2 * slot] = q0;
                    a.records[2 * slot + 1] = q1;
                }
                cum = 0.0;
                c = make_int2(0, 0);
            }
        }
    }
    if (live) {
        a.carry_ret[e] = cum;
        a.carry[e] = c;
    }
}

} // namespace

size_t episode_log_workspace_bytes(int n_envs, int K) { return 16 + 4 * (size_t)K * (size_t)filter_tiles(n_envs); }

hipError_t launch_episode_log(const EpisodeLogLaunch &l, hipStream_t stream)
{
    const int tiles = filter_tiles(l.N), cells = l.K * tiles;
    long long *hdr = static_cast<long long *>(l.workspace);
    int32_t *counts = reinterpret_cast<int32_t *>(hdr + 2);
    hipLaunchKernelGGL(eplog_count_kernel, dim3(cells), dim3(kLogTile), 0, stream, l.N, tiles, l.stride, l.done, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eplog_scan_kernel, dim3(1), dim3(kLogTile), 0, stream, cells, counts, hdr, reinterpret_cast<long long *>(l.head));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    LogWalk a;
    a.K = l.K;
    a.N = l.N;
    a.tiles = tiles;
    a.stride = l.stride;
    a.step0 = l.step0;
    a.env_base = l.env_base;
    a.capacity = l.capacity;
    a.members = l.lay.members;
    a.n = l.lay.n;
    a.slices = l.lay.slices;
    a.rew = l.rew;
    a.done = l.done;
    a.flags = l.flags;
    a.carry_ret = l.carry_ret;
    a.carry = reinterpret_cast<int2 *>(l.carry);
    a.hdr = hdr;
    a.base = counts;
    a.records = reinterpret_cast<uint4 *>(l.records);
    if (l.flags) hipLaunchKernelGGL(eplog_walk_kernel<true>, dim3(tiles), dim3(kLogTile), 0, stream, a);
    else hipLaunchKernelGGL(eplog_walk_kernel<false>, dim3(tiles), dim3(kLogTile), 0, stream, a);
    return hipGetLastError();
}

} // namespace ssg
