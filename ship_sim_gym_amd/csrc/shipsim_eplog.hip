// shipsim_eplog.hip — the episode log: ssg_episode_log_append and the job-wide log's ssg_job_episode_log_shard / ssg_job_episode_log_merge_blocks
// (include/shipsim.h), in an object of its own so that every other object's device code stays what it is.
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
        // (unsigned: the shard call's staging head holds whatever bytes the caller's block did, and the sum may wrap)
        head[0] = (long long)((unsigned long long)old + (unsigned long long)total);
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

// ---- the job-wide log (include/shipsim.h, "Job-wide episode log") ----------------------------------------------------------------------
// A shard block, as the kernels see it: the header, lb and the record slots.
struct LogBlock {
    int rows, stage;
    size_t lb_bytes, bytes; // of lb with its padding; of the whole block
};
__device__ __forceinline__ const int32_t *block_lb(const char *b) { return reinterpret_cast<const int32_t *>(b + sizeof(ssg_episode_log_block_header)); }

// (d) the shard call's pack, between scan and walk, grid (ceil(lb entries / 256)): the scan left lb_r[t] at counts[t * tiles] and the
// call's count in hdr[1], and used the block's header as the staging ring's head (scratch: it held whatever the caller left there).
// Lane j writes lb[j] — counts[j * tiles] below K, the count at K, zero past it, padding included —, and lane 0 the header and
// hdr[0] = 0: the head the walk reads, so that local rank q meets slot q % stage.  Plain vector stores.
__global__ void __launch_bounds__(kLogTile) eplog_pack_kernel(int K, int tiles, long long step0, int stage, int lb_n, const int32_t *__restrict__ counts,
                                                              long long *__restrict__ hdr, char *__restrict__ block)
{
    const int j = blockIdx.x * kLogTile + (int)threadIdx.x;
    const long long count = hdr[1];
    if (j < lb_n) {
        int32_t *lb = reinterpret_cast<int32_t *>(block + sizeof(ssg_episode_log_block_header));
        lb[j] = j < K ? counts[(size_t)j * tiles] : (j == K ? (int32_t)count : 0);
    }
    if (j == 0) {
        long long *bh = reinterpret_cast<long long *>(block);
        bh[0] = count;
        bh[1] = step0;
        bh[2] = (long long)(unsigned)K | ((long long)stage << 32); // int32 K, int32 stage
        bh[3] = 0;
        hdr[0] = 0;
    }
}

struct LogMerge {
    int K, n_blocks;
    long long step0, capacity;
    LogBlock g;
    const char *blocks;
    const long long *head;
    uint4 *records;
};

// the call's total, from every block's lb[K] (K <= rows: inside lb); never below 0
__device__ __forceinline__ long long merge_total(const LogMerge &a)
{
    long long total = 0;
    for (int r = 0; r < a.n_blocks; ++r) total += block_lb(a.blocks + (size_t)r * a.g.bytes)[a.K];
    return total > 0 ? total : 0;
}

// (e) grid (ceil(stage / 256), n_blocks): one lane per (block r, slot i).  Everything a lane indexes is bounded by the call's own
// arguments, never by what a block says: i < stage, t in [0, K) before lb[t + 1] is read (K <= rows), R in [0, total) before the
// store, the slot taken modulo the capacity from non-negative terms.
__global__ void __launch_bounds__(kLogTile) eplog_merge_kernel(const LogMerge a)
{
    const int r = blockIdx.y, i = blockIdx.x * kLogTile + (int)threadIdx.x;
    if (i >= a.g.stage) return;
    const char *b = a.blocks + (size_t)r * a.g.bytes;
    long long cnt = reinterpret_cast<const long long *>(b)[0];
    if (cnt < 0) cnt = 0;
    const long long S = a.g.stage;
    if ((long long)i >= (cnt < S ? cnt : S)) return;
    long long q = i;
    if (cnt > S) { // the one q in [cnt - S, cnt) congruent to i
        const long long base = cnt - S;
        q = base + ((long long)i - base % S + S) % S;
    }
    const uint4 *slot = reinterpret_cast<const uint4 *>(b + sizeof(ssg_episode_log_block_header) + a.g.lb_bytes) + 2 * (size_t)i;
    const uint4 q0 = slot[0], q1 = slot[1];
    const long long step = (long long)(((unsigned long long)q0.w << 32) | (unsigned long long)q0.z);
    const long long t = step - a.step0;
    if (t < 0 || t >= (long long)a.K) return;
    long long R = q - (long long)block_lb(b)[t];
    for (int v = 0; v < a.n_blocks; ++v) R += (long long)block_lb(a.blocks + (size_t)v * a.g.bytes)[v < r ? t + 1 : t];
    const long long total = merge_total(a);
    if (R < 0 || R >= total || R < total - a.capacity) return;
    long long h0 = a.head[0] % a.capacity;
    if (h0 < 0) h0 += a.capacity;
    const long long dst = (h0 + R % a.capacity) % a.capacity;
    a.records[2 * dst] = q0;
    a.records[2 * dst + 1] = q1;
}

// (f) one lane, after (e) on the stream: the head moves once every record has read it.
__global__ void eplog_merge_head_kernel(const LogMerge a, long long *__restrict__ head)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const long long total = merge_total(a);
        head[0] += total;
        head[1] = total;
    }
}

LogWalk walk_args(const EpisodeLogLaunch &l, int tiles, const long long *hdr, const int32_t *counts)
{
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
    return a;
}

hipError_t launch_walk(const LogWalk &a, hipStream_t stream)
{
    if (a.flags) hipLaunchKernelGGL(eplog_walk_kernel<true>, dim3(a.tiles), dim3(kLogTile), 0, stream, a);
    else hipLaunchKernelGGL(eplog_walk_kernel<false>, dim3(a.tiles), dim3(kLogTile), 0, stream, a);
    return hipGetLastError();
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
    return launch_walk(walk_args(l, tiles, hdr, counts), stream);
}

hipError_t launch_episode_log_shard(const EpisodeLogLaunch &l, int rows, int stage, void *block, hipStream_t stream)
{
    const int tiles = filter_tiles(l.N), cells = l.K * tiles;
    long long *hdr = static_cast<long long *>(l.workspace);
    int32_t *counts = reinterpret_cast<int32_t *>(hdr + 2);
    char *b = static_cast<char *>(block);
    const size_t lb_bytes = episode_log_block_lb_bytes(rows);
    const int lb_n = (int)(lb_bytes / 4);
    hipLaunchKernelGGL(eplog_count_kernel, dim3(cells), dim3(kLogTile), 0, stream, l.N, tiles, l.stride, l.done, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // (the staging head is the block's header, scratch until the pack: the scan adds the count to whatever bytes it holds, in unsigned
    // arithmetic, and the pack overwrites both words; a zeroed pair would cost a launch of its own, the workspace has no word to spare)
    hipLaunchKernelGGL(eplog_scan_kernel, dim3(1), dim3(kLogTile), 0, stream, cells, counts, hdr, reinterpret_cast<long long *>(b));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eplog_pack_kernel, dim3((lb_n + kLogTile - 1) / kLogTile), dim3(kLogTile), 0, stream, l.K, tiles, l.step0, stage, lb_n,
                       counts, hdr, b);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    LogWalk a = walk_args(l, tiles, hdr, counts);
    a.capacity = stage;
    a.records = reinterpret_cast<uint4 *>(b + sizeof(ssg_episode_log_block_header) + lb_bytes);
    return launch_walk(a, stream);
}

hipError_t launch_episode_log_merge(int K, long long step0, int rows, int stage, const void *blocks, int n_blocks,
                                    ssg_episode_record *records, long long capacity, int64_t *head, hipStream_t stream)
{
    LogMerge a;
    a.K = K;
    a.n_blocks = n_blocks;
    a.step0 = step0;
    a.capacity = capacity;
    a.g.rows = rows;
    a.g.stage = stage;
    a.g.lb_bytes = episode_log_block_lb_bytes(rows);
    a.g.bytes = episode_log_block_bytes(rows, stage);
    a.blocks = static_cast<const char *>(blocks);
    a.head = reinterpret_cast<const long long *>(head);
    a.records = reinterpret_cast<uint4 *>(records);
    hipLaunchKernelGGL(eplog_merge_kernel, dim3((stage + kLogTile - 1) / kLogTile, n_blocks), dim3(kLogTile), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eplog_merge_head_kernel, dim3(1), dim3(64), 0, stream, a, reinterpret_cast<long long *>(head));
    return hipGetLastError();
}

} // namespace ssg
