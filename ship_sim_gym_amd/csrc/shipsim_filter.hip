// shipsim_filter.hip — the running mean / std observation filter on the device: ssg_obs_filter_update (include/shipsim.h).
//
// What RLlib's MeanStdFilter and Stable-Baselines' VecNormalize do on the host around every env.step: fold the step's N observation
// rows into a running (count, mean, M2) per column.  Two launches, the kernel boundary between them is the hand-off:
//
//   1. partials, grid (256-row tiles, members): a workgroup stages its tile of the member's contiguous rows x D block in LDS (linear,
//      coalesced reads) and reduces every column to the tile's (mean, M2) with two halving trees — the sum, divided by the tile's row
//      count, then the sum of squared deviations from that mean.  One partial per tile and column goes to the workspace.
//   2. finalise, one workgroup per member: merges the member's partials (Chan et al.) in a fixed tree — eight runs of consecutive tiles,
//      each merged in tile order, then a halving tree over the eight — merges the result into the running state and writes mean, M2,
//      denom and count.
//
// Order.  Everything is f64, products and sums separately rounded (-ffp-contract=off).  The tile a row falls in, its place in the
// trees and the run its tile falls in depend on the row's index within the member's slice and on the slice's row count only: not on
// the grid, on which CU ran what, or on the other members.  No atomics, no hand-off between workgroups inside a launch.  The same order
// operation for operation in numpy: ship_sim_gym_amd/obs_filter.py, merge_reference.
//
// A job-wide filter (include/shipsim.h, "Job-wide observation filter") adds two kernels: the finalise launch that merges the batch into
// the state and into the rank's buffer (filter_finalise_dual_kernel, in place of launch 2 while a buffer is bound), and the merge of
// the ranks' gathered buffers into the base (filter_merge_rows_kernel; in numpy: merge_rows_reference).
#include <cstdint>

#include "shipsim_filter_common.h"
#include "shipsim_internal.h"

namespace ssg {
namespace {

// Launch 1.  part: f64 [members][gridDim.x][2][D] = the tile's mean and M2 per column.  The tile is staged kFltChunk columns at a time
// (all D at once when they fit: then the reads are one linear run over the tile's block); LDS rows have an odd stride in doubles, so
// that the 32 lanes of a ds_read_b64 group, one row each, fall on 32 different bank pairs.
__global__ void __launch_bounds__(kFltTile) filter_partials_kernel(const double *__restrict__ obs, int D, int n, const int32_t *__restrict__ slices,
                                                                   double *__restrict__ part)
{
    __shared__ double tile[kFltTile * kFltChunk];
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.y, n, &row0, &n_m);
    const int r0 = blockIdx.x * kFltTile;
    if (r0 >= n_m) return; // (a surplus workgroup of a shorter slice; uniform over the workgroup)
    const int rows = n_m - r0 < kFltTile ? n_m - r0 : kFltTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double *src = obs + (row0 + (size_t)r0) * (size_t)D;
    double *out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * (size_t)D;
    const double cnt = (double)rows;
    for (int c0 = 0; c0 < D; c0 += kFltChunk) {
        const int Dc = D - c0 < kFltChunk ? D - c0 : kFltChunk, S = Dc | 1;
        if (c0) __syncthreads(); // (the previous chunk's readers are done)
        // element i of the chunk is (row i / Dc, column i % Dc), tracked incrementally (256 = q * Dc + rem); eight loads are issued
        // before the first of them is stored, so that a thread has eight in flight
        {
            const int total = rows * Dc, q = kFltTile / Dc, rem = kFltTile % Dc;
            int c = tid % Dc, r = tid / Dc;
            for (int i = tid; i < total; i += 8 * kFltTile) {
                double v[8];
                int at[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    at[j] = r * S + c;
                    v[j] = i + j * kFltTile < total ? src[(size_t)r * D + c0 + c] : 0.0;
                    c += rem;
                    r += q;
                    if (c >= Dc) { c -= Dc; ++r; }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (i + j * kFltTile < total) tile[at[j]] = v[j];
            }
        }
        __syncthreads();
        for (int c = wave; c < Dc; c += kFltTile / 64) { // a column per wave at a time
            double v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = lane + 64 * k;
                v[k] = r < rows ? tile[r * S + c] : 0.0; // (tail rows: + 0.0 is exact)
            }
            const double mean = wave_tree_sum(v[0], v[1], v[2], v[3]) / cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double dv = v[k] - mean;
                v[k] = lane + 64 * k < rows ? dv * dv : 0.0;
            }
            const double m2 = wave_tree_sum(v[0], v[1], v[2], v[3]);
            if (lane == 0) {
                out[c0 + c] = mean;
                out[D + c0 + c] = m2;
            }
        }
    }
}

// Launch 2.  tiles_stride: launch 1's gridDim.x.  The member's T = ceil(n_m / 256) tiles form kFltRuns runs of L = ceil(T / kFltRuns)
// consecutive tiles (the last ones may be shorter or empty); work item (run g, column d) merges its run in tile order, then column d's
// eight results meet in a halving tree (g += g + 4, g + 2, g + 1), and the total is merged into the state.
__global__ void __launch_bounds__(kFltTile) filter_finalise_kernel(const double *__restrict__ part, int tiles_stride, int D, int n,
                                                                   const int32_t *__restrict__ slices, double eps, double *__restrict__ state)
{
    __shared__ double run_mean[kFltRuns * kFltMaxDim], run_m2[kFltRuns * kFltMaxDim];
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.x, n, &row0, &n_m);
    const int T = (n_m + kFltTile - 1) / kFltTile, L = (T + kFltRuns - 1) / kFltRuns;
    const double *mine = part + (size_t)blockIdx.x * tiles_stride * 2 * (size_t)D;
    double *st = state + (size_t)blockIdx.x * SSG_FILTER_ROWS * (size_t)D;
    const int tid = threadIdx.x;
    const double count = st[3 * D]; // (read by every lane before the barrier below, written after it)
    for (int item = tid; item < kFltRuns * D; item += kFltTile) {
        const int g = item / D, d = item - g * D;
        const int t1 = (g + 1) * L < T ? (g + 1) * L : T;
        Stat a = {0.0, 0.0, 0.0};
        for (int t = g * L; t < t1; t += 8) { // (eight tiles' partials are loaded ahead of their merges, which stay in tile order)
            double pm[8], pq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t tt = (size_t)(t + j < t1 ? t + j : t1 - 1);
                pm[j] = mine[tt * 2 * D + d];
                pq[j] = mine[tt * 2 * D + D + d];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (t + j >= t1) break;
                const int left = n_m - (t + j) * kFltTile;
                const Stat b = {(double)(left < kFltTile ? left : kFltTile), pm[j], pq[j]};
                merge(a, b);
            }
        }
        run_mean[item] = a.mean;
        run_m2[item] = a.m2;
    }
    __syncthreads();
    for (int d = tid; d < D; d += kFltTile) {
        Stat r[kFltRuns];
#pragma unroll
        for (int g = 0; g < kFltRuns; ++g) {
            const long long b0 = (long long)g * L * kFltTile, b1 = b0 + (long long)L * kFltTile; // the run's rows: [b0, b1) within n_m
            const long long lo = b0 < n_m ? b0 : n_m, hi = b1 < n_m ? b1 : n_m;
            r[g] = {(double)(hi - lo), run_mean[g * D + d], run_m2[g * D + d]};
        }
#pragma unroll
        for (int h = kFltRuns / 2; h > 0; h >>= 1)
#pragma unroll
            for (int g = 0; g < h; ++g) merge(r[g], r[g + h]);
        Stat s = {count, st[d], st[D + d]};
        merge(s, r[0]);
        st[d] = s.mean;
        st[D + d] = s.m2;
        st[2 * D + d] = s.n >= 2.0 ? sqrt(s.m2 / (s.n - 1.0)) + eps : 1.0;
        if (d == 0) st[3 * D] = s.n;
    }
}

// Launch 2 while a job-wide filter's buffer is bound (include/shipsim.h, "Job-wide observation filter"): the member's batch total r[0]
// is formed exactly as above and merged into two states, the bound one and the buffer — the statistics of this rank's own rows since the
// last synchronisation — each with its own count, read before the barrier.  The buffer's four rows are written like the state's, so it
// is a state block: bit for bit what an empty filter holds after the same batches.  A kernel of its own, its first part the text of
// the one above: with one body shared by both (a template, an inlined helper) the kernel above does not keep its machine code
// (profiles/obs_filter_job/README.md).
__global__ void __launch_bounds__(kFltTile) filter_finalise_dual_kernel(const double *__restrict__ part, int tiles_stride, int D, int n,
                                                                        const int32_t *__restrict__ slices, double eps, double *__restrict__ state,
                                                                        double *__restrict__ buffer)
{
    __shared__ double run_mean[kFltRuns * kFltMaxDim], run_m2[kFltRuns * kFltMaxDim];
    size_t row0;
    int n_m;
    member_rows(slices, blockIdx.x, n, &row0, &n_m);
    const int T = (n_m + kFltTile - 1) / kFltTile, L = (T + kFltRuns - 1) / kFltRuns;
    const double *mine = part + (size_t)blockIdx.x * tiles_stride * 2 * (size_t)D;
    double *st = state + (size_t)blockIdx.x * SSG_FILTER_ROWS * (size_t)D;
    const int tid = threadIdx.x;
    const double count = st[3 * D]; // (read by every lane before the barrier below, written after it)
    double *bf = buffer + (size_t)blockIdx.x * SSG_FILTER_ROWS * (size_t)D;
    const double bcount = bf[3 * D]; // (likewise)
    for (int item = tid; item < kFltRuns * D; item += kFltTile) {
        const int g = item / D, d = item - g * D;
        const int t1 = (g + 1) * L < T ? (g + 1) * L : T;
        Stat a = {0.0, 0.0, 0.0};
        for (int t = g * L; t < t1; t += 8) { // (eight tiles' partials are loaded ahead of their merges, which stay in tile order)
            double pm[8], pq[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t tt = (size_t)(t + j < t1 ? t + j : t1 - 1);
                pm[j] = mine[tt * 2 * D + d];
                pq[j] = mine[tt * 2 * D + D + d];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (t + j >= t1) break;
                const int left = n_m - (t + j) * kFltTile;
                const Stat b = {(double)(left < kFltTile ? left : kFltTile), pm[j], pq[j]};
                merge(a, b);
            }
        }
        run_mean[item] = a.mean;
        run_m2[item] = a.m2;
    }
    __syncthreads();
    for (int d = tid; d < D; d += kFltTile) {
        Stat r[kFltRuns];
#pragma unroll
        for (int g = 0; g < kFltRuns; ++g) {
            const long long b0 = (long long)g * L * kFltTile, b1 = b0 + (long long)L * kFltTile; // the run's rows: [b0, b1) within n_m
            const long long lo = b0 < n_m ? b0 : n_m, hi = b1 < n_m ? b1 : n_m;
            r[g] = {(double)(hi - lo), run_mean[g * D + d], run_m2[g * D + d]};
        }
#pragma unroll
        for (int h = kFltRuns / 2; h > 0; h >>= 1)
#pragma unroll
            for (int g = 0; g < h; ++g) merge(r[g], r[g + h]);
        Stat s = {count, st[d], st[D + d]};
        merge(s, r[0]);
        st[d] = s.mean;
        st[D + d] = s.m2;
        st[2 * D + d] = s.n >= 2.0 ? sqrt(s.m2 / (s.n - 1.0)) + eps : 1.0;
        if (d == 0) st[3 * D] = s.n;
        Stat b = {bcount, bf[d], bf[D + d]}; // the same total into the buffer
        merge(b, r[0]);
        bf[d] = b.mean;
        bf[D + d] = b.m2;
        bf[2 * D + d] = b.n >= 2.0 ? sqrt(b.m2 / (b.n - 1.0)) + eps : 1.0;
        if (d == 0) bf[3 * D] = b.n;
    }
}

// The rows merge of a job-wide filter (ssg_obs_filter_merge_rows): one workgroup per member, a thread per column.  state[m] = base[m]
// merged with rows[0][m], rows[1][m], ..., rows[n_rows - 1][m] in index order, a row of count 0 skipped (merge's empty side); every
// block is f64 [members][SSG_FILTER_ROWS][D], rows [n_rows] of them.  No atomics, no LDS; state must not alias base or rows.
__global__ void __launch_bounds__(kFltTile) filter_merge_rows_kernel(const double *__restrict__ base, const double *__restrict__ rows, int n_rows,
                                                                     int D, double eps, double *__restrict__ state)
{
    const size_t block = (size_t)SSG_FILTER_ROWS * (size_t)D, mine = (size_t)blockIdx.x * block, stride = (size_t)gridDim.x * block;
    const double *b0 = base + mine;
    double *st = state + mine;
    for (int d = threadIdx.x; d < D; d += kFltTile) {
        Stat s = {b0[3 * D], b0[d], b0[D + d]};
        for (int r = 0; r < n_rows; ++r) {
            const double *row = rows + (size_t)r * stride + mine;
            const Stat b = {row[3 * D], row[d], row[D + d]};
            merge(s, b);
        }
        st[d] = s.mean;
        st[D + d] = s.m2;
        st[2 * D + d] = s.n >= 2.0 ? sqrt(s.m2 / (s.n - 1.0)) + eps : 1.0;
        st[3 * D + d] = d == 0 ? s.n : 0.0;
    }
}

} // namespace

size_t filter_workspace_bytes(int n_envs, int obs_dim, int members)
{
    return (size_t)members * (size_t)filter_tiles(n_envs) * 2 * (size_t)obs_dim * sizeof(double);
}

hipError_t launch_filter_update(const double *obs, int D, const MemberLayout &lay, double eps, double *state, double *buffer, void *ws,
                                hipStream_t stream)
{
    const int tiles = filter_tiles(lay.n);
    double *part = static_cast<double *>(ws);
    hipLaunchKernelGGL(filter_partials_kernel, dim3((unsigned)tiles, (unsigned)lay.members), dim3(kFltTile), 0, stream, obs, D, lay.n, lay.slices, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (buffer)
        hipLaunchKernelGGL(filter_finalise_dual_kernel, dim3((unsigned)lay.members), dim3(kFltTile), 0, stream, (const double *)part, tiles, D, lay.n,
                           lay.slices, eps, state, buffer);
    else
        hipLaunchKernelGGL(filter_finalise_kernel, dim3((unsigned)lay.members), dim3(kFltTile), 0, stream, (const double *)part, tiles, D, lay.n,
                           lay.slices, eps, state);
    return hipGetLastError();
}

hipError_t launch_filter_merge_rows(const double *base, const double *rows, int n_rows, int D, int members, double eps, double *state,
                                    hipStream_t stream)
{
    hipLaunchKernelGGL(filter_merge_rows_kernel, dim3((unsigned)members), dim3(kFltTile), 0, stream, base, rows, n_rows, D, eps, state);
    return hipGetLastError();
}

} // namespace ssg
