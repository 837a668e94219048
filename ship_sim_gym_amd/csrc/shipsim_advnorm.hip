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

__global__ void __launch_bounds__(256) adv_norm_partial_kernel(const AdvNormArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t m = blockIdx.y;
    MemberBatch mb;
    if (!member_batch(a, m, mb)) return; // (uniform over the workgroup, ahead of every barrier; the member's row is left alone)
    const int B = adv_norm_blocks(mb.M);
    if ((int)blockIdx.x >= B) return;
    double s = 0.0, q = 0.0, c = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < mb.M; i += (long long)B * 256) {
        long long j = mb.idx[i];
        if (j >= mb.n_samples) j = -1;
        if (j < 0) continue; // a zero, gradient-free sample of the gradient kernel: it counts for nothing
        if (a.pop) {
            const long long t = j / mb.mem_n;
            j = t * a.N + mb.mem_base + (j - t * mb.mem_n);
        }
        const double v = (double)a.adv[j];
        s += v;
        q += v * v;
        c += 1.0;
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    rc[threadIdx.x] = c;
    tree3(rs, rq, rc);
    if (threadIdx.x == 0) {
        double *p = a.part + (m * kAdvNormBlocks + blockIdx.x) * 3;
        p[0] = rs[0];
        p[1] = rq[0];
        p[2] = rc[0];
    }
}

__global__ void __launch_bounds__(256) adv_norm_final_kernel(const AdvNormArgs a)
{
    __shared__ double rs[256], rq[256], rc[256];
    const size_t m = blockIdx.x;
    MemberBatch mb;
    if (!member_batch(a, m, mb)) return;
    const int B = adv_norm_blocks(mb.M);
    double s = 0.0, q = 0.0, c = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) {
        const double *p = a.part + (m * kAdvNormBlocks + b) * 3;
        s += p[0];
        q += p[1];
        c += p[2];
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    rc[threadIdx.x] = c;
    tree3(rs, rq, rc);
    if (threadIdx.x == 0) {
        float *st = a.stats + m * 4;
        const double cnt = rc[0];
        if (cnt == 0.0) {
            st[0] = 0.0f;
            st[1] = 1.0f;
            st[2] = 1.0f;
            st[3] = 0.0f;
            return;
        }
        const float adv_eps = a.pop ? a.table[m * kPopTableRow + a.adv_eps_col] : a.adv_eps;
        const double mean = rs[0] / cnt;
        double var = cnt > 1.0 ? (rq[0] - rs[0] * mean) / (cnt - 1.0) : 0.0; // (one sample: PPO2's numpy std is 0; torch.std would be NaN)
        if (var < 0.0) var = 0.0;
        const float stdp = (float)sqrt(var) + adv_eps;
        st[0] = (float)mean;
        st[1] = stdp;
        st[2] = 1.0f / stdp;
        st[3] = 0.0f;
    }
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

} // namespace ssg
