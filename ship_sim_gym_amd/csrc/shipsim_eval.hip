// shipsim_eval.hip — episode accounting of an evaluation run: ssg_evaluate / ssg_pop_evaluate / ssg_eval_reduce (include/shipsim.h), and
// the evaluation recorder's two row launches (ssg_set_eval_recorder; its frames are drawn in shipsim_render.hip).
//
// What the reference's train/rllib/rollout.py:8-26 does on the host for one env — add up the reward until done, print it — for every env
// of a handle on the device, one small launch after every step: an env counts its FIRST E episodes and then stops counting, so every
// env weighs the same whatever the length of its episodes, and each counted episode's ending is tallied from the step's event bits.
// All sums are integers (the return as llrint(100 * return), as pop_episode_stats_kernel counts it): order-free and exact.
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kEvalBlock = 256;

// One lane per env, after one step: rew / done / flags are that step's rows.  carry_ret f64 [N] and carry int32 [N][4] = (length, goal
// events of the running episode, episodes counted, 0) are the caller's, zero after a reset; stats int64 [N][kEvalCols], caller-zeroed.
// An env that has counted E episodes touches nothing.
__global__ void __launch_bounds__(kEvalBlock) eval_account_kernel(int N, int E, const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                                  const uint8_t *__restrict__ flags, double *__restrict__ carry_ret,
                                                                  int4 *__restrict__ carry, long long *__restrict__ stats)
{
    const int e = blockIdx.x * kEvalBlock + threadIdx.x;
    if (e >= N) return;
    int4 c = carry[e];
    if (c.z >= E) return;
    const unsigned f = flags[e];
    double ret = carry_ret[e] + rew[e];
    c.x += 1;
    c.y += (f & SSG_EV_GOAL_REACHED) ? 1 : 0;
    if (done[e]) {
        long long *row = stats + (size_t)e * kEvalCols;
        row[0] += 1;
        row[1] += (long long)llrint(ret * 100.0);
        row[2] += c.x;
        row[3] += (f & SSG_EV_COLLIDING) ? 1 : 0;
        row[4] += (f & SSG_EV_OUT_OF_BOUNDS) ? 1 : 0;
        row[5] += (f & SSG_EV_MAX_STEPS) ? 1 : 0;
        row[6] += (f & SSG_EV_NO_GOALS_LEFT) ? 1 : 0;
        row[7] += c.y;
        ret = 0.0;
        c.x = 0;
        c.y = 0;
        c.z += 1;
    }
    carry_ret[e] = ret;
    carry[e] = c;
}

// grid (members): workgroup m writes (does not accumulate) the column sums of rows [m*n, (m+1)*n) of stats into out[m]: a strided loop
// per lane, then an integer tree over the workgroup.
// (the body of both kernels: the member's n rows start at `rows`)
__device__ __forceinline__ void eval_reduce_body(int n, const long long *__restrict__ rows, long long *__restrict__ out,
                                                 long long (*red)[kEvalBlock])
{
    long long s[kEvalCols];
#pragma unroll
    for (int c = 0; c < kEvalCols; ++c) s[c] = 0;
    for (int i = threadIdx.x; i < n; i += kEvalBlock) {
#pragma unroll
        for (int c = 0; c < kEvalCols; ++c) s[c] += rows[(size_t)i * kEvalCols + c];
    }
#pragma unroll
    for (int c = 0; c < kEvalCols; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = kEvalBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int c = 0; c < kEvalCols; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < kEvalCols) out[(size_t)blockIdx.x * kEvalCols + threadIdx.x] = red[threadIdx.x][0];
}

__global__ void __launch_bounds__(kEvalBlock) eval_reduce_kernel(int n, const long long *__restrict__ stats, long long *__restrict__ out)
{
    __shared__ long long red[kEvalCols][kEvalBlock];
    eval_reduce_body(n, stats + (size_t)blockIdx.x * (size_t)n * kEvalCols, out, red);
}

// on unequal slices (ssg_pop_set_slices): workgroup m sums rows [o_m, o_m + n_m), its row of the slices table
__global__ void __launch_bounds__(kEvalBlock) eval_reduce_sliced_kernel(const int32_t *__restrict__ slices, const long long *__restrict__ stats,
                                                                        long long *__restrict__ out)
{
    __shared__ long long red[kEvalCols][kEvalBlock];
    const int32_t *row = slices + (size_t)blockIdx.x * SSG_POP_SLICE_ROW;
    eval_reduce_body(row[1], stats + (size_t)row[0] * kEvalCols, out, red);
}

// The evaluation recorder (ssg_set_eval_recorder; what train/rllib/rollout.py:20-21 appends per step): one lane per slot, R <= 64 lanes,
// one workgroup.  Both kernels read the carries the previous iteration's accounting launch left and the cursors the previous
// iteration's record_step left, so they agree on which slots are active (eval_rec_step); neither touches anything of the handle's.
constexpr int kRecBlock = SSG_EVAL_REC_MAX_ENVS;

// ahead of the policy launch: the raw observation row the policy is about to read
__global__ void __launch_bounds__(kRecBlock) eval_record_obs_kernel(const EvalRecLaunch r, const EvalRecIds ids, const double *__restrict__ dev_obs)
{
    const int s = threadIdx.x;
    if (s >= r.R) return;
    const int e = ids.e[s];
    const int t = eval_rec_step(r, e, s);
    if (t < 0) return;
    const double *src = dev_obs + (size_t)e * r.D;
    double *dst = r.obs + ((size_t)s * r.C + t) * r.D;
    for (int d = 0; d < r.D; ++d) dst[d] = src[d];
}

// between the step and the accounting launch: the policy's outputs, the step's rows, next_obs, then the cursor; a full slot of an env
// that still counts adds 1 to its overflow count instead
__global__ void __launch_bounds__(kRecBlock) eval_record_step_kernel(const EvalRecLaunch r, const EvalRecIds ids, const double *__restrict__ dev_obs,
                                                                    const int32_t *__restrict__ act, const float *__restrict__ logp,
                                                                    const float *__restrict__ value, const double *__restrict__ rew,
                                                                    const uint8_t *__restrict__ done, const uint8_t *__restrict__ flags)
{
    const int s = threadIdx.x;
    if (s >= r.R) return;
    const int e = ids.e[s];
    if (r.carry[4 * (size_t)e + 2] >= r.E) return;
    const int t = r.cursor[s];
    if (t >= r.C) {
        r.overflow[s] += 1;
        return;
    }
    const size_t i = (size_t)s * r.C + t;
    const uint8_t dn = done[e];
    r.act[i] = act[e];
    r.logp[i] = logp[e];
    r.value[i] = value[e];
    r.reward[i] = rew[e];
    r.done[i] = dn;
    r.flags[i] = flags[e];
    const double *src = (dn ? r.term_obs : dev_obs) + (size_t)e * r.D;
    double *dst = r.next_obs + i * r.D;
    for (int d = 0; d < r.D; ++d) dst[d] = src[d];
    r.cursor[s] = t + 1;
}

} // namespace

hipError_t launch_eval_record_obs(const EvalRecLaunch &r, const EvalRecIds &ids, const double *dev_obs, hipStream_t stream)
{
    hipLaunchKernelGGL(eval_record_obs_kernel, dim3(1), dim3(kRecBlock), 0, stream, r, ids, dev_obs);
    return hipGetLastError();
}

hipError_t launch_eval_record_step(const EvalRecLaunch &r, const EvalRecIds &ids, const double *dev_obs, const int32_t *act, const float *logp,
                                   const float *value, const double *rew, const uint8_t *done, const uint8_t *flags, hipStream_t stream)
{
    hipLaunchKernelGGL(eval_record_step_kernel, dim3(1), dim3(kRecBlock), 0, stream, r, ids, dev_obs, act, logp, value, rew, done, flags);
    return hipGetLastError();
}

hipError_t launch_eval_account(int N, int E, const double *rew, const uint8_t *done, const uint8_t *flags, double *carry_ret, int32_t *carry,
                               int64_t *stats, hipStream_t stream)
{
    hipLaunchKernelGGL(eval_account_kernel, dim3((N + kEvalBlock - 1) / kEvalBlock), dim3(kEvalBlock), 0, stream, N, E, rew, done, flags, carry_ret,
                       reinterpret_cast<int4 *>(carry), reinterpret_cast<long long *>(stats));
    return hipGetLastError();
}

hipError_t launch_eval_reduce(const MemberLayout &lay, const int64_t *stats, int64_t *out, hipStream_t stream)
{
    if (lay.slices)
        hipLaunchKernelGGL(eval_reduce_sliced_kernel, dim3(lay.members), dim3(kEvalBlock), 0, stream, lay.slices,
                           reinterpret_cast<const long long *>(stats), reinterpret_cast<long long *>(out));
    else
        hipLaunchKernelGGL(eval_reduce_kernel, dim3(lay.members), dim3(kEvalBlock), 0, stream, lay.n, reinterpret_cast<const long long *>(stats),
                           reinterpret_cast<long long *>(out));
    return hipGetLastError();
}

} // namespace ssg
