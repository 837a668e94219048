// shipsim_advnorm.hip — PPO2's per-minibatch advantage normalisation (ssg_ppo_set_adv_norm, SSG_ADV_NORM_MINIBATCH; include/shipsim.h).
//
// The reference's PPO2 re-normalises the advantages inside every minibatch (train/stable_baselines/ppo.py:90: model.learn's _train_step,
// advs = (advs - advs.mean()) / (advs.std() + 1e-8) over the minibatch's own samples).  The gradient kernels (shipsim_ppo.hip) read
// {mean, std + adv_eps} through a pointer; the two launches here, ahead of a minibatch's gradient launch on its stream, fill a row of
// the caller's scratch with the statistics of THAT minibatch, and launch_ppo_minibatch points the gradient kernel at it.  Nothing of the
// gradient, reduction, clip or Adam kernels is part of this object; their device code is what it was (profiles/adv_norm/README.md).
//
// The estimator is gae_stats_body's: f64 sums s, q, c of adv, adv^2 and 1 over the minibatch's indices inside [0, n_samples);
// mean = s / c, var = max(0, (q - s*mean) / (c - 1)) (c == 1: var = 0), std+ = (float)sqrt(var) + adv_eps, row = {mean, std+, 1/std+, 0};
// c == 0: {0, 1, 1, 0}.  The order is a function of the minibatch's length M alone:
//   partials  grid (64, members) x 256: member m uses B = min(64, ceil(M / 1024)) workgroups; thread t of workgroup b takes the
//             positions i = b*256 + t, then steps by B*256 while i < M, in that order; then the 256-entry LDS tree w = 128 .. 1
//             (gae_body's); one (s, q, c) per workgroup.
//   finalise  one workgroup per member: thread b holds partial b (b < B, zeros beyond), the same tree, lane 0 writes the row.
// No floating-point atomics; plain stores.
//
// The job-wide form (ssg_ppo_minibatch_adv_sums / ssg_ppo_set_minibatch_adv_rows; the end of this file) takes the same sums for EVERY
// minibatch of an update in two launches — minibatch (e, j) of the permutation rows on grid row e*C + j — and leaves them as f64 rows
// {s, q, c, 0}; the rows of W shards, gathered, are then added in rank order and put through the same formula into a table of stats
// rows.  The accumulate loop, the trees and the formula are the device functions below, shared with the two kernels above them.
//
// Which row of the [K][N] buffers position i of member m's minibatch names is RESTATED from ppo_grad_body (its top and its step 1),
// for its four shapes: one policy; a population on equal slices; on per-member schedules; on unequal slices.
#include <cmath>
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

struct AdvNormArgs {
    const float *adv;
    const int64_t *idx;
    long long M, n_samples;
    int pop;              // a population: idx rows, slices and adv_eps per member
    long long n, N;       // envs per member, envs of the batch
    long long idx_stride; // int64 entries between two members' index rows
    const float *table;   // [members][kPopTableRow]; adv_eps at column adv_eps_col
    int adv_eps_col;
    float adv_eps;        // one policy's
    const int32_t *sched; // nullable: this launch's schedule records
    const int32_t *slices, *sched_hdr; // nullable: unequal slices
    long long K, perm_epochs;
    double *part; // f64 [members][kAdvNormBlocks][3]
    float *stats; // f32 [members][4]
};

// Member m's minibatch of this launch: its length (false: it has none, a schedule record with G == 0), where its indices start, and the
// member's envs / first env / sample count — ppo_grad_body's top.
struct MemberBatch {
    const int64_t *idx;
    long long M, n_samples, mem_n, mem_base;
};

__device__ __forceinline__ bool member_batch(const AdvNormArgs &a, size_t m, MemberBatch &b)
{
    b.idx = a.idx;
    b.M = a.M;
    b.n_samples = a.n_samples;
    b.mem_n = a.n;
    b.mem_base = a.pop ? (long long)m * a.n : 0;
    if (a.pop && !a.slices) b.idx += m * (size_t)a.idx_stride;
    if (a.slices) {
        const int32_t *row = a.slices + m * SSG_POP_SLICE_ROW;
        b.mem_base = row[0];
        b.mem_n = row[1];
        b.n_samples = a.K * b.mem_n;
        b.idx += a.perm_epochs * *reinterpret_cast<const long long *>(a.sched_hdr + m * kPopSchedRow + SH_PREFIX);
    }
    if (a.sched) {
        const int32_t *rec = a.sched + m * kPopSchedRow;
        if (rec[SR_G] == 0) return false;
        b.M = rec[SR_M];
        b.idx += *reinterpret_cast<const long long *>(rec + SR_OFF);
    }
    return true;
}

__device__ __forceinline__ int adv_norm_blocks(long long M)
{
    const long long b = (M + 1023) / 1024;
    return (int)(b < kAdvNormBlocks ? b : kAdvNormBlocks);
}

// the 256-entry tree of gae_body over three columns; afterwards entry 0 of each holds the sum
__device__ __forceinline__ void tree3(double *rs, double *rq, double *rc)
{
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rs[threadIdx.x] += rs[threadIdx.x + w];
            rq[threadIdx.x] += rq[threadIdx.x + w];
            rc[threadIdx.x] += rc[threadIdx.x + w];
        }
        __syncthreads();
    }
}

// thread t of workgroup bx of B: the positions bx*256 + t, then steps of B*256 while below M, added in that order.  pop: the index is
// member-local, sample t*mem_n + e being row t*N + mem_base + e of the batch.
__device__ __forceinline__ void adv_accumulate(const float *adv, const int64_t *idx, long long M, long long n_samples, int B, int bx, int pop,
                                               long long mem_n, long long N, long long mem_base, double &s, double &q, double &c)
{
    for (long long i = (long long)bx * 256 + threadIdx.x; i < M; i += (long long)B * 256) {
        long long j = idx[i];
        if (j >= n_samples) j = -1;
        if (j < 0) continue; // a zero, gradient-free sample of the gradient kernel: it counts for nothing
        if (pop) {
            const long long t = j / mem_n;
            j = t * N + mem_base + (j - t * mem_n);
        }
        const double v = (double)adv[j];
        s += v;
        q += v * v;
        c += 1.0;
    }
}

// the workgroup's tree over its threads' sums; lane 0 stores the (s, q, c) partial
__device__ __forceinline__ void adv_store_partial(double *rs, double *rq, double *rc, double s, double q, double c, double *p)
{
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    rc[threadIdx.x] = c;
    tree3(rs, rq, rc);
    if (threadIdx.x == 0) {
        p[0] = rs[0];
        p[1] = rq[0];
        p[2] = rc[0];
    }
}

// the finalising workgroup: thread b holds partial b (b < B, zeros beyond), the same tree; entry 0 of each column holds the sum
__device__ __forceinline__ void adv_sum_partials(double *rs, double *rq, double *rc, const double *part, int B)
{
    double s = 0.0, q = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const double *p = part + b * 3;
        s += p[0];
        q += p[1];
        c += p[2];
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    rc[threadIdx.x] = c;
    tree3(rs, rq, rc);
}

// the stats row {mean, std+, 1/std+, 0} of the sums S, Q and the count cnt
__device__ __forceinline__ void adv_stats_row(double S, double Q, double cnt, float adv_eps, float *st)
{
    if (cnt == 0.0) {
        st[0] = 0.0f;
        st[1] = 1.0f;
        st[2] = 1.0f;
        st[3] = 0.0f;
        return;
    }
    const double mean = S / cnt;
    double var = cnt > 1.0 ? (Q - S * mean) / (cnt - 1.0) : 0.0; // (one sample: PPO2's numpy std is 0; torch.std would be NaN)
    if (var < 0.0) var = 0.0;
    const float stdp = (float)sqrt(var) + adv_eps;
    st[0] = (float)mean;
    st[1] = stdp;
    st[2] = 1.0f / stdp;
    st[3] = 0.0f;
}

__global__ void __launch_bounds__(256) adv_norm_partial_kernel(const AdvNormArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t m = blockIdx.y;
    MemberBatch mb;
    if (!member_batch(a, m, mb)) return; // (uniform over the workgroup, ahead of every barrier; the member's row is left alone)
    const int B = adv_norm_blocks(mb.M);
    if ((int)blockIdx.x >= B) return;
    double s = 0.0, q = 0.0, c = 0.0;
    adv_accumulate(a.adv, mb.idx, mb.M, mb.n_samples, B, (int)blockIdx.x, a.pop, mb.mem_n, a.N, mb.mem_base, s, q, c);
    adv_store_partial(rs, rq, rc, s, q, c, a.part + (m * kAdvNormBlocks + blockIdx.x) * 3);
}

__global__ void __launch_bounds__(256) adv_norm_final_kernel(const AdvNormArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t m = blockIdx.x;
    MemberBatch mb;
    if (!member_batch(a, m, mb)) return;
    adv_sum_partials(rs, rq, rc, a.part + m * kAdvNormBlocks * 3, adv_norm_blocks(mb.M));
    if (threadIdx.x == 0)
        adv_stats_row(rs[0], rq[0], rc[0], a.pop ? a.table[m * kPopTableRow + a.adv_eps_col] : a.adv_eps, a.stats + m * 4);
}

// ---- the job-wide form: every minibatch of an update at once --------------------------------------------------------------------------
// minibatch y = e*C + j of the permutation rows: perm[e][j*chunk : min(n, (j+1)*chunk)]
struct MbSumsArgs {
    const float *adv;
    const int64_t *perm; // int64 [epochs][n]
    long long n_samples, n, chunk, C;
    double *part; // f64 [epochs*C][kAdvNormBlocks][3]
    double *out;  // f64 [epochs*C][4]
};

__device__ __forceinline__ long long mb_sums_batch(const MbSumsArgs &a, size_t y, const int64_t *&idx)
{
    const long long e = (long long)y / a.C, b0 = ((long long)y - e * a.C) * a.chunk;
    idx = a.perm + (size_t)e * (size_t)a.n + (size_t)b0;
    return a.chunk < a.n - b0 ? a.chunk : a.n - b0;
}

__global__ void __launch_bounds__(256) mb_sums_partial_kernel(const MbSumsArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t y = blockIdx.y;
    const int64_t *idx;
    const long long M = mb_sums_batch(a, y, idx);
    const int B = adv_norm_blocks(M);
    if ((int)blockIdx.x >= B) return; // (uniform over the workgroup, ahead of every barrier)
    double s = 0.0, q = 0.0, c = 0.0;
    adv_accumulate(a.adv, idx, M, a.n_samples, B, (int)blockIdx.x, 0, 1, 0, 0, s, q, c);
    adv_store_partial(rs, rq, rc, s, q, c, a.part + (y * kAdvNormBlocks + blockIdx.x) * 3);
}

__global__ void __launch_bounds__(256) mb_sums_final_kernel(const MbSumsArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t y = blockIdx.x;
    const int64_t *idx;
    const long long M = mb_sums_batch(a, y, idx);
    adv_sum_partials(rs, rq, rc, a.part + y * kAdvNormBlocks * 3, adv_norm_blocks(M));
    if (threadIdx.x == 0) {
        double *o = a.out + y * 4;
        o[0] = rs[0];
        o[1] = rq[0];
        o[2] = rc[0];
        o[3] = 0.0;
    }
}

// one lane per minibatch: the W shards' rows added in rank order, then the row
__global__ void __launch_bounds__(256) mb_rows_kernel(int W, int n_batches, const double *__restrict__ rows, float adv_eps, float *__restrict__ table)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n_batches) return;
    const double *r0 = rows + (size_t)b * 4;
    double S = r0[0], Q = r0[1], cnt = r0[2];
    for (int r = 1; r < W; ++r) {
        const double *p = r0 + (size_t)r * (size_t)n_batches * 4;
        S += p[0];
        Q += p[1];
        cnt += p[2];
    }
    adv_stats_row(S, Q, cnt, adv_eps, table + (size_t)b * 4);
}

} // namespace

hipError_t launch_adv_norm(const AdvNormLaunch &l, hipStream_t stream)
{
    if (!l.stats || !l.part || l.lay.members < 1) return hipErrorInvalidValue;
    AdvNormArgs a;
    a.adv = l.adv;
    a.idx = l.idx;
    a.M = l.M;
    a.n_samples = l.n_samples;
    a.pop = l.table != nullptr;
    a.n = l.lay.n;
    a.N = l.N;
    a.idx_stride = l.idx_stride;
    a.table = l.table;
    a.adv_eps_col = l.adv_eps_col;
    a.adv_eps = l.adv_eps;
    a.sched = l.sched;
    a.slices = l.lay.slices;
    a.sched_hdr = l.sched_hdr;
    a.K = l.K;
    a.perm_epochs = l.perm_epochs;
    a.part = l.part;
    a.stats = l.stats;
    hipLaunchKernelGGL(adv_norm_partial_kernel, dim3(kAdvNormBlocks, (unsigned)l.lay.members), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(adv_norm_final_kernel, dim3((unsigned)l.lay.members), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_minibatch_adv_sums(const MinibatchAdvSums &l, hipStream_t stream)
{
    MbSumsArgs a;
    a.adv = l.adv;
    a.perm = l.perm;
    a.n_samples = l.n_samples;
    a.n = l.n;
    a.chunk = l.chunk;
    a.C = (l.n + l.chunk - 1) / l.chunk;
    a.part = l.part;
    a.out = l.out;
    const unsigned rows = (unsigned)(l.epochs * a.C);
    // (the widest minibatch is a full chunk: B is monotone in M, so no workgroup a shorter one needs is missing)
    const long long bmax = (l.chunk + 1023) / 1024;
    hipLaunchKernelGGL(mb_sums_partial_kernel, dim3((unsigned)(bmax < kAdvNormBlocks ? bmax : kAdvNormBlocks), rows), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mb_sums_final_kernel, dim3(rows), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_minibatch_adv_rows(int n_shards, int n_batches, const double *rows, float adv_eps, float *table, hipStream_t stream)
{
    hipLaunchKernelGGL(mb_rows_kernel, dim3((unsigned)((n_batches + 255) / 256)), dim3(256), 0, stream, n_shards, n_batches, rows, adv_eps, table);
    return hipGetLastError();
}

} // namespace ssg
