// shipsim_report.hip — the update report (ssg_ppo_report / ssg_pop_report; include/shipsim.h).
//
// The reference's trainers print, per update, how the update went: PPO2's explained_variance, approxkl, clipfrac, policy_entropy,
// policy_loss, value_loss (train/stable_baselines/ppo.py:88-90, verbose=1 / tensorboard_log) and RLlib's vf_explained_var, kl, entropy,
// policy_loss, vf_loss (train/rllib/ppo.py:26-41, train/rllib/pbt.py:47-74).  The two launches here reduce a rollout's [K][N] buffers
// (and, optionally, the update's per-minibatch stats rows) to one f64 record of SSG_REPORT_COLS per member.  Nothing of any other
// object is part of this one; their device code is what it was.
//
// The order of operations is a function of (K, n_m, rows) alone:
//   walk    grid (blocks of the widest slice, members) x 256: lane e of member m's block b owns env o_m + b*256 + e and walks
//           t = 0 .. K-1 in ascending order over its column (loads may run ahead, the additions may not), f64, every product and sum
//           separately rounded; then the 256-entry LDS tree w = 128 .. 1 (gae_body's) per sum; one row of kReportSums per (m, b).
//   finish  one workgroup per member: thread j adds the partials of blocks j, j + 256, ... in that order, the same tree, then lane 0
//           forms the record (gae_stats_body's order).  Threads 0 .. 7 have each summed one column of the stats rows in row order.
// No floating-point atomics; plain stores; constant launch arguments.
//
// A data-parallel job's record (ssg_ppo_report_sums / ssg_ppo_report_rows; train/rllib/ppo.py:34-35: the experience of all workers) is
// formed from the ranks' sum rows, which are mergeable where records are not:
//   sums    the walk as above, then one workgroup that runs the finish's first two phases and stores the totals, n and the post flag
//           as one f64 row of SSG_REPORT_ROW_COLS: bit for bit what the finish forms internally;
//   rows    one 64-thread workgroup per output record: column c of the gathered rows accumulated in row order from row 0's value on,
//           the stats columns as in the finish, then form_record — the one function that turns {totals, n, post, stats sums} into the
//           record, shared with the finish, so one row gives ssg_ppo_report's record bit for bit.
#include <cmath>
#include <cstdint>
#include <limits>

#include "shipsim_internal.h"

namespace ssg {
namespace {

struct ReportArgs {
    int K, N;              // rows, and the distance between two rows
    int n;                 // envs per member on equal slices (N for one policy)
    int nb;                // partial rows per member
    const int32_t *slices; // nullable: unequal slices
    const float *val, *ret, *adv;
    const int32_t *act;    // the post-update group: all three or none
    const float *logp, *lpa;
    const float *bounds;   // nullable: f32 [members][2] = lo, hi per member; else lo / hi below
    float lo, hi;
    const float *stats;    // nullable: f32 [members][rows_max][n_cols]
    const int32_t *rows;   // nullable: int32 [members]
    int rows_max, n_cols;
    double *part;          // f64 [members][nb][kReportSums]
    double *out;           // f64 [members][SSG_REPORT_COLS]
};

// member m's first env and env count
__device__ __forceinline__ void member_slice(const ReportArgs &a, size_t m, size_t &e0, int &n)
{
    if (a.slices) {
        e0 = (size_t)a.slices[m * SSG_POP_SLICE_ROW];
        n = a.slices[m * SSG_POP_SLICE_ROW + 1];
    } else {
        e0 = m * (size_t)a.n;
        n = a.n;
    }
}

// the 256-entry tree of gae_body over kReportSums columns; afterwards entry 0 of each column holds the sum
__device__ __forceinline__ void tree_sums(double (*r)[256])
{
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < kReportSums; ++c) r[c][threadIdx.x] += r[c][threadIdx.x + w];
        __syncthreads();
    }
}

template <bool POST>
__device__ __forceinline__ void walk_body(const ReportArgs &a, double (*r)[256])
{
    const size_t m = blockIdx.y;
    size_t e0;
    int n;
    member_slice(a, m, e0, n);
    if ((int)(blockIdx.x * 256) >= n) return; // (uniform over the workgroup, ahead of every barrier)
    const int e = blockIdx.x * 256 + threadIdx.x;
    double s[kReportSums];
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) s[c] = 0.0;
    if (e < n) {
        float lo = a.lo, hi = a.hi;
        if (POST && a.bounds) {
            lo = a.bounds[m * 2];
            hi = a.bounds[m * 2 + 1];
        }
        const float *__restrict__ val = a.val, *__restrict__ ret = a.ret, *__restrict__ adv = a.adv;
        size_t i = e0 + (size_t)e;
#pragma unroll 4
        for (int t = 0; t < a.K; ++t, i += (size_t)a.N) {
            const double rr = (double)ret[i], v = (double)val[i], ad = (double)adv[i];
            const double err = rr - v;
            s[0] += rr;
            s[1] += rr * rr;
            s[2] += err;
            s[3] += err * err;
            s[4] += v;
            s[5] += ad;
            if constexpr (POST) {
                const float d = a.lpa[i * 4 + (size_t)(a.act[i] & 3)] - a.logp[i]; // ONE f32 subtraction
                const double dd = (double)d;
                s[6] += dd;
                s[7] += dd * dd;
                s[8] += (d > hi || d < lo) ? 1.0 : 0.0;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) r[c][threadIdx.x] = s[c];
    tree_sums(r);
    if (threadIdx.x < kReportSums) a.part[(m * (size_t)a.nb + blockIdx.x) * kReportSums + threadIdx.x] = r[threadIdx.x][0];
}

__global__ void __launch_bounds__(256) report_walk_kernel(const ReportArgs a)
{
    __shared__ double r[kReportSums][256];
    walk_body<false>(a, r);
}

__global__ void __launch_bounds__(256) report_walk_post_kernel(const ReportArgs a)
{
    __shared__ double r[kReportSums][256];
    walk_body<true>(a, r);
}

// thread j adds the partials of member m's blocks j, j + 256, ... in that order, then the tree: entry 0 of each column of r holds the
// member's total afterwards (the first two phases of the finish, which the sums kernel runs alone)
__device__ __forceinline__ void block_totals(const ReportArgs &a, size_t m, int B, double (*r)[256])
{
    double s[kReportSums];
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) s[c] = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const double *p = a.part + (m * (size_t)a.nb + b) * kReportSums;
#pragma unroll
        for (int c = 0; c < kReportSums; ++c) s[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) r[c][threadIdx.x] = s[c];
    tree_sums(r);
}

// threads 0 .. 7: column c of the stats rows summed in f64 in row order, one thread per column (0.0 for a column the rows lack)
__device__ __forceinline__ void stats_colsums(const float *stats, int rows, int n_cols, double *colsum)
{
    if (threadIdx.x < 8) {
        double c = 0.0;
        if ((int)threadIdx.x < n_cols) {
            const float *st = stats + threadIdx.x;
            for (int j = 0; j < rows; ++j) c += (double)st[(size_t)j * n_cols];
        }
        colsum[threadIdx.x] = c;
    }
}

// The record from {the nine totals, the count, the post-update group's state, the stats columns' sums}: the ONE place where the
// SSG_REPORT_COLS columns are formed, for report_finish_kernel and report_rows_kernel alike.  post: 1 on, 0 off, anything else (rows
// of a job that disagree) NaN in [8..11].
__device__ __forceinline__ void form_record(double *o, const double *tot, double cnt, int post, const double *colsum, int n_cols, int rows)
{
    const double mr = tot[0] / cnt;
    double vr = (tot[1] - tot[0] * mr) / cnt;
    if (vr < 0.0) vr = 0.0;
    const double me = tot[2] / cnt;
    double ve = (tot[3] - tot[2] * me) / cnt;
    if (ve < 0.0) ve = 0.0;
    o[0] = cnt;
    o[1] = mr;
    o[2] = vr;
    o[3] = me;
    o[4] = ve;
    o[5] = vr == 0.0 ? std::numeric_limits<double>::quiet_NaN() : 1.0 - ve / vr;
    o[6] = tot[4] / cnt;
    o[7] = tot[5] / cnt;
    if (post == 1) {
        o[8] = 1.0;
        o[9] = -(tot[6] / cnt);
        o[10] = 0.5 * (tot[7] / cnt);
        o[11] = tot[8] / cnt;
    } else {
        const double x = post == 0 ? 0.0 : std::numeric_limits<double>::quiet_NaN();
        o[8] = x;
        o[9] = x;
        o[10] = x;
        o[11] = x;
    }
    for (int c = 0; c < 8; ++c) o[12 + c] = rows > 0 && c < n_cols ? colsum[c] / (double)rows : 0.0;
    o[20] = (double)rows;
    o[21] = 0.0;
    o[22] = 0.0;
    o[23] = 0.0;
}

__global__ void __launch_bounds__(256) report_finish_kernel(const ReportArgs a)
{
    __shared__ double r[kReportSums][256];
    __shared__ double colsum[8];
    const size_t m = blockIdx.x;
    size_t e0;
    int n;
    member_slice(a, m, e0, n);
    const int B = (n + 255) / 256; // (ppo_gae_blocks)
    int rows = 0;
    if (a.stats) {
        rows = a.rows ? a.rows[m] : a.rows_max;
        if (rows > a.rows_max) rows = a.rows_max; // (rows past rows_max do not exist)
        if (rows < 0) rows = 0;
    }
    stats_colsums(a.stats + (m * (size_t)a.rows_max) * a.n_cols, rows, a.n_cols, colsum);
    block_totals(a, m, B, r);
    if (threadIdx.x != 0) return;
    double tot[kReportSums];
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) tot[c] = r[c][0];
    form_record(a.out + m * SSG_REPORT_COLS, tot, (double)a.K * (double)n, a.lpa ? 1 : 0, colsum, a.n_cols, rows);
}

// ssg_ppo_report_sums' second launch: one workgroup, the finish's first two phases over the one policy's partials, then the sum row
// [SSG_REPORT_ROW_COLS] = the nine totals, n, the post flag, 0 — plain stores by twelve threads.
__global__ void __launch_bounds__(256) report_sums_kernel(const ReportArgs a, double *__restrict__ row)
{
    __shared__ double r[kReportSums][256];
    block_totals(a, 0, (a.n + 255) / 256, r);
    const int c = threadIdx.x;
    if (c >= SSG_REPORT_ROW_COLS) return;
    double x = 0.0;
    if (c < 6 || (c < kReportSums && a.lpa)) x = r[c][0];
    else if (c == kReportSums) x = (double)a.K * (double)a.n;
    else if (c == kReportSums + 1) x = a.lpa ? 1.0 : 0.0;
    row[c] = x;
}

struct ReportRowsArgs {
    int W;                 // sum rows, 1..SSG_DP_MAX_SHARDS
    const double *rows;    // f64 [W][SSG_REPORT_ROW_COLS], shard order
    const float *stats;    // nullable: f32 [n_stat_rows][n_cols]
    int n_stat_rows, n_cols;
    double *out;           // f64 [gridDim.x][SSG_REPORT_COLS]: the job's record, then (per_shard) one per row
};

// ssg_ppo_report_rows: workgroup 0 forms the job's record — thread 8 + c accumulates column c (the nine sums and n) of the rows in row
// order, from row 0's value on; thread 18 compares the post flags —, workgroup 1 + r shard r's own from row r alone.  Threads 0 .. 7
// sum the stats columns as the finish does; lane 0 forms the record.
__global__ void __launch_bounds__(64) report_rows_kernel(const ReportRowsArgs a)
{
    __shared__ double tot[kReportSums + 1];
    __shared__ double colsum[8];
    __shared__ int post;
    const int first = blockIdx.x == 0 ? 0 : (int)blockIdx.x - 1;
    const int last = blockIdx.x == 0 ? a.W : first + 1; // (one past)
    const int t = threadIdx.x;
    const int rows = a.stats ? a.n_stat_rows : 0;
    if (a.stats) stats_colsums(a.stats, rows, a.n_cols, colsum);
    else if (t < 8) colsum[t] = 0.0;
    if (t >= 8 && t < 8 + kReportSums + 1) {
        const int c = t - 8;
        double x = a.rows[(size_t)first * SSG_REPORT_ROW_COLS + c];
        for (int r = first + 1; r < last; ++r) x += a.rows[(size_t)r * SSG_REPORT_ROW_COLS + c];
        tot[c] = x;
    }
    if (t == 8 + kReportSums + 1) {
        int on = 0, off = 0;
        for (int r = first; r < last; ++r) {
            const double f = a.rows[(size_t)r * SSG_REPORT_ROW_COLS + kReportSums + 1];
            on += f == 1.0;
            off += f == 0.0;
        }
        post = on == last - first ? 1 : off == last - first ? 0 : -1;
    }
    __syncthreads();
    if (t != 0) return;
    double s[kReportSums];
#pragma unroll
    for (int c = 0; c < kReportSums; ++c) s[c] = tot[c];
    form_record(a.out + (size_t)blockIdx.x * SSG_REPORT_COLS, s, tot[kReportSums], post, colsum, a.stats ? a.n_cols : 0, rows);
}

} // namespace

size_t report_scratch_bytes(int n_widest, int members)
{
    return ((size_t)members * (size_t)ppo_gae_blocks(n_widest) * kReportSums * sizeof(double) + 255) & ~(size_t)255;
}

void report_clip_bounds(double clip, float out_lo_hi[2])
{
    out_lo_hi[0] = clip >= 1.0 ? -std::numeric_limits<float>::infinity() : (float)std::log1p(-clip);
    out_lo_hi[1] = (float)std::log1p(clip);
}

hipError_t launch_report(const ReportLaunch &l, hipStream_t stream)
{
    if (!l.val || !l.ret || !l.adv || !l.part || (!l.out && !l.row) || l.lay.members < 1 || l.lay.n < 1 || l.K < 1) return hipErrorInvalidValue;
    if ((l.lpa != nullptr) != (l.act != nullptr) || (l.lpa != nullptr) != (l.logp != nullptr)) return hipErrorInvalidValue;
    ReportArgs a;
    a.K = l.K;
    a.N = l.N;
    a.n = l.lay.n;
    a.nb = ppo_gae_blocks(l.lay.n);
    a.slices = l.lay.slices;
    a.val = l.val;
    a.ret = l.ret;
    a.adv = l.adv;
    a.act = l.act;
    a.logp = l.logp;
    a.lpa = l.lpa;
    a.bounds = l.bounds;
    a.lo = l.lo;
    a.hi = l.hi;
    a.stats = l.stats;
    a.rows = l.rows;
    a.rows_max = l.stats ? l.rows_max : 0;
    a.n_cols = l.stats ? l.n_cols : 0;
    a.part = l.part;
    a.out = l.out;
    if (l.row && (l.lay.members != 1 || l.lay.slices)) return hipErrorInvalidValue; // (the sum row is one policy's)
    const dim3 grid((unsigned)a.nb, (unsigned)l.lay.members);
    if (l.lpa) hipLaunchKernelGGL(report_walk_post_kernel, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(report_walk_kernel, grid, dim3(256), 0, stream, a);
    if (l.row) hipLaunchKernelGGL(report_sums_kernel, dim3(1), dim3(256), 0, stream, a, l.row); // (one policy: ssg_ppo_report_sums)
    else hipLaunchKernelGGL(report_finish_kernel, dim3((unsigned)l.lay.members), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_report_rows(int n_rows, const double *rows, const float *stats, int n_stat_rows, int n_cols, bool per_shard, double *out,
                              hipStream_t stream)
{
    if (!rows || !out || n_rows < 1 || n_rows > SSG_DP_MAX_SHARDS) return hipErrorInvalidValue;
    ReportRowsArgs a;
    a.W = n_rows;
    a.rows = rows;
    a.stats = stats;
    a.n_stat_rows = stats ? n_stat_rows : 0;
    a.n_cols = stats ? n_cols : 0;
    a.out = out;
    hipLaunchKernelGGL(report_rows_kernel, dim3(1u + (per_shard ? (unsigned)n_rows : 0u)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace ssg
