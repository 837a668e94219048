// shipsim_retfilter.hip — return normalisation on the device: ssg_ret_filter_apply (include/shipsim.h, "Return filter").
//
// What Stable-Baselines' VecNormalize does to the rewards on the host around every env.step: keep a discounted return per env, fold
// the step's N returns into a running (count, mean, M2), and divide the step's rewards by the running standard deviation.  Here a whole
// rollout's [K][N] reward buffer is served by three launches, the kernel boundaries between them are the hand-offs:
//
//   1. walk, grid (256-env tiles, members): one lane per env walks k = 0 .. K-1 (c = c * gamma + r; sample; c = 0 where done).  The
//      tile's samples of four consecutive k are staged in LDS and each of the four waves reduces one k to the tile's (mean, M2) with the
//      observation filter's one-wave halving trees.  One partial per (k, tile) goes to the workspace; the carry is written back.
//   2. chain, one workgroup per member: work item (k, run) merges its run's tiles in tile order, the eight runs of a k meet in a halving
//      tree across adjacent lanes, then one thread chains the K batch merges into the state; every k's denom is formed from the chain.
//   3. normalise, grid (256-env tiles, members, groups of kRetRows steps): out = clamp(rew / denom_k, +-clip).
//
// A frozen call is launch 3 alone, with the state's own denom for every k.
//
// A job-wide filter (include/shipsim.h, "Job-wide return filter") splits launch 2 at its __syncthreads, with the ranks' gather between
// the halves: ssg_ret_filter_batches is launch 1 and ret_batch_kernel (launch 2's batches, stored as rows), ssg_ret_filter_apply_rows is
// ret_job_chain_kernel (each step's gathered rows merged in rank order, then launch 2's chain and denoms) and launch 3.
//
// Order.  Everything is f64, products and sums separately rounded (-ffp-contract=off).  Batch k of a member is reduced exactly as
// ssg_obs_filter_update reduces one column of n_m rows (shipsim_filter_common.h), so the result depends on a row's index within the
// member's slice, on n_m, K and the inputs only.  No atomics, no hand-off between workgroups inside a launch.  The same order in
// numpy: ship_sim_gym_amd/ret_filter.py, ret_filter_reference.
#include <cstdint>

#include "shipsim_filter_common.h"
#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kRetStage = 4; // steps staged in LDS per pass of launch 1: one per wave
constexpr int kRetRows = 8;  // steps per thread of launch 3

static_assert(kRetStage == kFltTile / 64, "launch 1 reduces one staged step per wave");
static_assert((kFltTile / kFltRuns) * kFltRuns == kFltTile && kFltRuns <= 64, "launch 2 keeps a step's runs in adjacent lanes of one wave");

// Launch 1.  part: f64 [members][K][gridDim.x][2] = the (mean, M2) of tile t's samples at step k.  rew / done: [K][stride].
__global__ void __launch_bounds__(kFltTile) ret_walk_kernel(const double *__restrict__ rew, const uint8_t *__restrict__ done, int K, size_t stride,
                                                            int n, const int32_t *__restrict__ slices, const double *__restrict__ gamma,
                                                            double *__restrict__ carry, double *__restrict__ part)
{
    __shared__ double stage[2][kRetStage][kFltTile]; // (two halves: a pass writes one while the slowest wave may still read the other)
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.y, n, &row0, &n_m);
    const int r0 = blockIdx.x * kFltTile;
    if (r0 >= n_m) return; // (a surplus workgroup of a shorter slice; uniform over the workgroup)
    const int rows = n_m - r0 < kFltTile ? n_m - r0 : kFltTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool live = tid < rows;
    const size_t e = row0 + (size_t)r0 + (size_t)(live ? tid : 0); // (idle lanes of a tail tile read row 0 of the tile and store nothing)
    const double g = gamma[blockIdx.y], cnt = (double)rows;
    double *out = part + ((size_t)blockIdx.y * K * gridDim.x + blockIdx.x) * 2;
    double c = carry[e];
    // the loads do not depend on the carry: the next pass's rows are requested before this pass's chain runs
    double r[kRetStage], rn[kRetStage];
    uint8_t d[kRetStage], dn[kRetStage];
#pragma unroll
    for (int j = 0; j < kRetStage; ++j) {
        const size_t at = (size_t)(j < K ? j : K - 1) * stride + e;
        r[j] = rew[at];
        d[j] = done[at];
    }
    for (int k0 = 0, half = 0; k0 < K; k0 += kRetStage, half ^= 1) {
#pragma unroll
        for (int j = 0; j < kRetStage; ++j) {
            const int k = k0 + kRetStage + j;
            const size_t at = (size_t)(k < K ? k : K - 1) * stride + e;
            rn[j] = rew[at];
            dn[j] = done[at];
        }
#pragma unroll
        for (int j = 0; j < kRetStage; ++j) {
            if (k0 + j < K) {
                c = c * g + r[j];
                stage[half][j][tid] = live ? c : 0.0; // (tail rows: + 0.0 is exact)
                if (d[j]) c = 0.0;
            }
        }
        __syncthreads();
        if (k0 + wave < K) { // a step per wave: lane l holds entries l, l + 64, l + 128, l + 192
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = stage[half][wave][lane + 64 * q];
            const double mean = wave_tree_sum(v[0], v[1], v[2], v[3]) / cnt;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double dv = v[q] - mean;
                v[q] = lane + 64 * q < rows ? dv * dv : 0.0;
            }
            const double m2 = wave_tree_sum(v[0], v[1], v[2], v[3]);
            if (lane == 0) {
                double *o = out + (size_t)(k0 + wave) * gridDim.x * 2;
                o[0] = mean;
                o[1] = m2;
            }
        }
#pragma unroll
        for (int j = 0; j < kRetStage; ++j) {
            r[j] = rn[j];
            d[j] = dn[j];
        }
    }
    if (live) carry[e] = c;
}

// Run g of a member of n_m rows in launch 2's reduction: its tiles [t0, t1) and the rows they hold.
struct RunTiles { int t0, t1; double n; };
__device__ __forceinline__ RunTiles run_tiles(int n_m, int g)
{
    const int T = (n_m + kFltTile - 1) / kFltTile, L = (T + kFltRuns - 1) / kFltRuns;
    const long long b0 = (long long)g * L * kFltTile, b1 = b0 + (long long)L * kFltTile; // the run's rows: [b0, b1) within n_m
    return {g * L, (g + 1) * L < T ? (g + 1) * L : T, (double)((b1 < n_m ? b1 : n_m) - (b0 < n_m ? b0 : n_m))};
}

// Batch k of a member from launch 1's partials (mine: the member's [K][tiles_stride][2]), for work item (k, run): the run's tiles merged
// in tile order; the eight runs of a step sit in adjacent lanes and meet in the halving tree (g += g + 4, g + 2, g + 1); lane g == 0
// returns batch k.  Whole waves call it (the shuffles), with k >= K in the lanes past the last step.  The one statement of this
// reduction: ret_chain_kernel and ret_batch_kernel both call it, so a job's rows hold the bits the plain call chains.
__device__ __forceinline__ Stat step_batch(const double *__restrict__ mine, int tiles_stride, int K, int n_m, const RunTiles &run, int k)
{
    const int t0 = run.t0, t1 = run.t1;
    Stat a = {0.0, 0.0, 0.0};
    if (k < K) {
        const double *row = mine + (size_t)k * tiles_stride * 2;
        for (int t = t0; t < t1; t += 8) { // (eight tiles' partials are loaded ahead of their merges, which stay in tile order)
            double pm[8], pq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int tt = t + j < t1 ? t + j : t1 - 1;
                pm[j] = row[2 * tt];
                pq[j] = row[2 * tt + 1];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (t + j >= t1) break;
                const int left = n_m - (t + j) * kFltTile;
                const Stat b = {(double)(left < kFltTile ? left : kFltTile), pm[j], pq[j]};
                merge(a, b);
            }
        }
    }
    a.n = run.n; // (what the merges summed, or 0 for an empty run)
#pragma unroll
    for (int h = kFltRuns / 2; h > 0; h >>= 1) {
        const Stat b = {__shfl_down(a.n, h, 64), __shfl_down(a.mean, h, 64), __shfl_down(a.m2, h, 64)};
        merge(a, b); // (lanes with g >= h merge what nothing below reads)
    }
    return a;
}

// Launch 2.  tiles_stride: launch 1's gridDim.x.  Work item i = 8 k + g: run g of step k (step_batch); lane g == 0 holds batch k.  Then
// thread 0 chains the K batches into the state, and every thread forms the denoms of its steps from the chain's (count, M2).
// denom: f64 [K][members].
__global__ void __launch_bounds__(kFltTile) ret_chain_kernel(const double *__restrict__ part, int tiles_stride, int K, int n,
                                                             const int32_t *__restrict__ slices, double eps, double *__restrict__ state,
                                                             double *__restrict__ denom)
{
    __shared__ double bat_mean[SSG_RET_FILTER_MAX_STEPS], bat_m2[SSG_RET_FILTER_MAX_STEPS]; // batch k; then the chain's count and M2 after k
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.x, n, &row0, &n_m);
    const int tid = threadIdx.x, g = tid & (kFltRuns - 1);
    const RunTiles run = run_tiles(n_m, g);
    const double *mine = part + (size_t)blockIdx.x * K * tiles_stride * 2;
    double *st = state + (size_t)blockIdx.x * SSG_FILTER_ROWS;
    for (int k0 = 0; k0 < K; k0 += kFltTile / kFltRuns) { // (uniform trip count: the shuffles are executed by whole waves)
        const int k = k0 + tid / kFltRuns;
        const Stat a = step_batch(mine, tiles_stride, K, n_m, run, k);
        if (g == 0 && k < K) {
            bat_mean[k] = a.mean;
            bat_m2[k] = a.m2;
        }
    }
    __syncthreads();
    if (tid == 0) {
        Stat s = {st[3], st[0], st[1]};
        for (int k = 0; k < K; ++k) {
            const Stat b = {(double)n_m, bat_mean[k], bat_m2[k]};
            merge(s, b);
            bat_mean[k] = s.n;
            bat_m2[k] = s.m2;
        }
        st[0] = s.mean;
        st[1] = s.m2;
        st[2] = s.n >= 2.0 ? sqrt(s.m2 / (s.n - 1.0)) + eps : 1.0;
        st[3] = s.n;
    }
    __syncthreads();
    for (int k = tid; k < K; k += kFltTile) {
        const double cnt = bat_mean[k];
        denom[(size_t)k * gridDim.x + blockIdx.x] = cnt >= 2.0 ? sqrt(bat_m2[k] / (cnt - 1.0)) + eps : 1.0;
    }
}

// A job-wide filter's launch 2a (ssg_ret_filter_batches), one member of n_m rows: ret_chain_kernel's batches without the chain, so a grid
// of ceil(K / 32) workgroups; lane g == 0 stores row k = {mean, M2, 0.0, n_m}, the state's row order.  rows: f64 [K][SSG_FILTER_ROWS].
typedef double Row4 __attribute__((ext_vector_type(4), aligned(8))); // (a row is one 32-byte access; the caller's rows are 8-byte aligned)
static_assert(SSG_FILTER_ROWS == 4, "a row of the job-wide return filter is the state's four entries");

__global__ void __launch_bounds__(kFltTile) ret_batch_kernel(const double *__restrict__ part, int tiles_stride, int K, int n_m,
                                                             double *__restrict__ rows)
{
    const int tid = threadIdx.x, g = tid & (kFltRuns - 1);
    const int k = blockIdx.x * (kFltTile / kFltRuns) + tid / kFltRuns;
    const Stat a = step_batch(part, tiles_stride, K, n_m, run_tiles(n_m, g), k);
    if (g == 0 && k < K) {
        const Row4 r = {a.mean, a.m2, 0.0, (double)n_m};
        reinterpret_cast<Row4 *>(rows)[k] = r;
    }
}

// A job-wide filter's launch 2b (ssg_ret_filter_apply_rows), one workgroup: rows f64 [W][K][SSG_FILTER_ROWS], the ranks' rows in rank order.
// Thread j merges a step's W rows in rank order, from rows[0] on (eight rows are loaded ahead of their merges); thread 0 chains the steps
// into the state; every thread forms the denoms of its steps.  The two LDS arrays of ret_chain_kernel serve kJobChunk steps at a time:
// a step's count, which there is the member's n for every step, takes the upper half of the first.  denom: f64 [K].
constexpr int kJobChunk = SSG_RET_FILTER_MAX_STEPS / 2;

__global__ void __launch_bounds__(kFltTile) ret_job_chain_kernel(const double *__restrict__ rows, int W, int K, double eps,
                                                                 double *__restrict__ state, double *__restrict__ denom)
{
    __shared__ double bat_mean[SSG_RET_FILTER_MAX_STEPS], bat_m2[SSG_RET_FILTER_MAX_STEPS]; // step j of the chunk, its count at kJobChunk + j; then the chain's count and M2 after it
    const int tid = threadIdx.x;
    const Row4 *all = reinterpret_cast<const Row4 *>(rows);
    Stat s = {0.0, 0.0, 0.0};
    if (tid == 0) s = {state[3], state[0], state[1]};
    for (int c0 = 0; c0 < K; c0 += kJobChunk) {
        const int kc = K - c0 < kJobChunk ? K - c0 : kJobChunk;
        for (int j = tid; j < kc; j += kFltTile) {
            const Row4 *src = all + (c0 + j);
            Stat a = {0.0, 0.0, 0.0};
            for (int w0 = 0; w0 < W; w0 += 8) {
                Row4 r[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) r[i] = src[(size_t)(w0 + i < W ? w0 + i : W - 1) * K];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (w0 + i >= W) break;
                    const Stat b = {r[i].w, r[i].x, r[i].y};
                    if (w0 + i == 0) a = b; // (the step starts from rank 0's row, not from an empty stat)
                    else merge(a, b);
                }
            }
            bat_mean[j] = a.mean;
            bat_m2[j] = a.m2;
            bat_mean[kJobChunk + j] = a.n;
        }
        __syncthreads();
        if (tid == 0) {
            for (int j = 0; j < kc; ++j) {
                const Stat b = {bat_mean[kJobChunk + j], bat_mean[j], bat_m2[j]};
                merge(s, b);
                bat_mean[j] = s.n;
                bat_m2[j] = s.m2;
            }
        }
        __syncthreads();
        for (int j = tid; j < kc; j += kFltTile) {
            const double cnt = bat_mean[j];
            denom[c0 + j] = cnt >= 2.0 ? sqrt(bat_m2[j] / (cnt - 1.0)) + eps : 1.0;
        }
        __syncthreads(); // (the next chunk's steps overwrite what the denoms were formed from)
    }
    if (tid == 0) {
        state[0] = s.mean;
        state[1] = s.m2;
        state[2] = s.n >= 2.0 ? sqrt(s.m2 / (s.n - 1.0)) + eps : 1.0;
        state[3] = s.n;
    }
}

// Launch 3.  den: the denom of (step k, member m) at den[k * den_k + m * den_m] — launch 2's [K][members], or the state's own denom for
// every k when frozen; a denom of 0.0 divides by 1.  den_out (nullable): f64 [K][members], the divisor each row was divided by.
__global__ void __launch_bounds__(kFltTile) ret_normalise_kernel(const double *__restrict__ rew, int K, size_t stride, int n,
                                                                 const int32_t *__restrict__ slices, const double *__restrict__ den,
                                                                 size_t den_k, size_t den_m, double clip, double *__restrict__ out,
                                                                 double *__restrict__ den_out)
{
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.y, n, &row0, &n_m);
    const int r = blockIdx.x * kFltTile + threadIdx.x;
    if (r >= n_m) return;
    const size_t e = row0 + (size_t)r;
    const int k0 = blockIdx.z * kRetRows;
    double v[kRetRows], dv[kRetRows];
#pragma unroll
    for (int j = 0; j < kRetRows; ++j) {
        const int k = k0 + j < K ? k0 + j : K - 1;
        v[j] = rew[(size_t)k * stride + e];
        dv[j] = den[(size_t)k * den_k + (size_t)blockIdx.y * den_m];
    }
#pragma unroll
    for (int j = 0; j < kRetRows; ++j) {
        const int k = k0 + j;
        if (k >= K) break;
        const double dd = dv[j] == 0.0 ? 1.0 : dv[j];
        double x = v[j] / dd;
        if (clip > 0.0) x = x < -clip ? -clip : (x > clip ? clip : x); // (a NaN reward stays NaN)
        out[(size_t)k * stride + e] = x;
        if (den_out && r == 0) den_out[(size_t)k * gridDim.y + blockIdx.y] = dd;
    }
}

} // namespace

// the tile partials of launch 1, f64 [members][K][tiles][2], then launch 2's denoms, f64 [K][members]
size_t ret_filter_workspace_bytes(int n_envs, int K, int members)
{
    return ((size_t)members * (size_t)K * (size_t)filter_tiles(n_envs) * 2 + (size_t)K * (size_t)members) * sizeof(double);
}

hipError_t launch_ret_filter(const RetFilterLaunch &l, hipStream_t stream)
{
    const MemberLayout &lay = l.lay;
    const int tiles = filter_tiles(lay.n);
    double *part = static_cast<double *>(l.workspace);
    double *denom = part + (size_t)lay.members * (size_t)l.K * (size_t)tiles * 2;
    const dim3 block(kFltTile);
    if (l.update) {
        hipLaunchKernelGGL(ret_walk_kernel, dim3((unsigned)tiles, (unsigned)lay.members), block, 0, stream, l.rew, l.done, l.K, l.stride, lay.n,
                           lay.slices, l.gamma, l.carry, part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(ret_chain_kernel, dim3((unsigned)lay.members), block, 0, stream, (const double *)part, tiles, l.K, lay.n, lay.slices, l.eps,
                           l.state, denom);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const double *den = l.update ? denom : l.state + 2;
    const size_t den_k = l.update ? (size_t)lay.members : 0, den_m = l.update ? 1 : SSG_FILTER_ROWS;
    hipLaunchKernelGGL(ret_normalise_kernel, dim3((unsigned)tiles, (unsigned)lay.members, (unsigned)((l.K + kRetRows - 1) / kRetRows)), block, 0,
                       stream, l.rew, l.K, l.stride, lay.n, lay.slices, den, den_k, den_m, l.clip, l.out, l.denom_out);
    return hipGetLastError();
}

// ssg_ret_filter_batches: the walk, then the shard's row per step; the state is not touched (one member: the whole handle)
hipError_t launch_ret_filter_batches(const RetFilterLaunch &l, double *rows, hipStream_t stream)
{
    const int tiles = filter_tiles(l.lay.n);
    double *part = static_cast<double *>(l.workspace);
    const dim3 block(kFltTile);
    hipLaunchKernelGGL(ret_walk_kernel, dim3((unsigned)tiles, 1u), block, 0, stream, l.rew, l.done, l.K, l.stride, l.lay.n, l.lay.slices, l.gamma,
                       l.carry, part);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    constexpr int per = kFltTile / kFltRuns;
    hipLaunchKernelGGL(ret_batch_kernel, dim3((unsigned)((l.K + per - 1) / per)), block, 0, stream, (const double *)part, tiles, l.K, l.lay.n, rows);
    return hipGetLastError();
}

// ssg_ret_filter_apply_rows: the chain over the gathered rows, then the division by its denoms (which live where launch_ret_filter's do)
hipError_t launch_ret_filter_rows(const RetFilterLaunch &l, const double *rows, int n_rows, hipStream_t stream)
{
    const int tiles = filter_tiles(l.lay.n);
    double *denom = static_cast<double *>(l.workspace) + (size_t)l.K * (size_t)tiles * 2;
    const dim3 block(kFltTile);
    hipLaunchKernelGGL(ret_job_chain_kernel, dim3(1u), block, 0, stream, rows, n_rows, l.K, l.eps, l.state, denom);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ret_normalise_kernel, dim3((unsigned)tiles, 1u, (unsigned)((l.K + kRetRows - 1) / kRetRows)), block, 0, stream, l.rew, l.K,
                       l.stride, l.lay.n, l.lay.slices, (const double *)denom, (size_t)1, (size_t)1, l.clip, l.out, l.denom_out);
    return hipGetLastError();
}

} // namespace ssg
