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
    if (threadIdx.x < 8) {
        double c = 0.0;
        if ((int)threadIdx.x < a.n_cols) {
            const float *st = a.stats + (m * (size_t)a.rows_max) * a.n_cols + threadIdx.x;
            for (int j = 0; j < rows; ++j) c += (double)st[(size_t)j * a.n_cols];
        }
        colsum[threadIdx.x] = c;
    }
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
    if (threadIdx.x != 0) return;
    double *o = a.out + m * SSG_REPORT_COLS;
    const double cnt = (double)a.K * (double)n;
    const double mr = r[0][0] / cnt;
    double vr = (r[1][0] - r[0][0] * mr) / cnt;
    if (vr < 0.0) vr = 0.0;
    const double me = r[2][0] / cnt;
    double ve = (r[3][0] - r[2][0] * me) / cnt;
    if (ve < 0.0) ve = 0.0;
    o[0] = cnt;
    o[1] = mr;
    o[2] = vr;
    o[3] = me;
    o[4] = ve;
    o[5] = vr == 0.0 ? std::numeric_limits<double>::quiet_NaN() : 1.0 - ve / vr;
    o[6] = r[4][0] / cnt;
    o[7] = r[5][0] / cnt;
    if (a.lpa) {
        o[8] = 1.0;
        o[9] = -(r[6][0] / cnt);
        o[10] = 0.5 * (r[7][0] / cnt);
        o[11] = r[8][0] / cnt;
    } else {
        o[8] = 0.0;
        o[9] = 0.0;
        o[10] = 0.0;
        o[11] = 0.0;
    }
    for (int c = 0; c < 8; ++c) o[12 + c] = rows > 0 && c < a.n_cols ? colsum[c] / (double)rows : 0.0;
    o[20] = (double)rows;
    o[21] = 0.0;
    o[22] = 0.0;
    o[23] = 0.0;
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
    if (!l.val || !l.ret || !l.adv || !l.part || !l.out || l.lay.members < 1 || l.lay.n < 1 || l.K < 1) return hipErrorInvalidValue;
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
    const dim3 grid((unsigned)a.nb, (unsigned)l.lay.members);
    if (l.lpa) hipLaunchKernelGGL(report_walk_post_kernel, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(report_walk_kernel, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(report_finish_kernel, dim3((unsigned)l.lay.members), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace ssg
