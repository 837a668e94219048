// shipsim_policy.hip — the policy half of a rollout step on the device: ssg_policy_act / ssg_rollout_policy (include/shipsim.h).
//
// What the reference's runner does around every env.step (train/stable_baselines/ppo.py:84-100: one policy forward per step) and what
// train/ppo_torch.py's Shard.step() does in a dozen PyTorch kernels: normalise the f64 observation, an MLP actor-critic in f32, inverse-CDF
// sampling of the action, the rollout-buffer values.  One launch per step, one lane per env.
//
// Shape.  One wave (64 lanes = 64 envs) per workgroup.  The activations of one layer live in LDS as rows of 65 floats (one column per
// lane, +1 of padding), which each lane reads back as its own column.  The weights are the same for every lane: 16 output rows at a
// time are staged into an LDS tile and read with broadcast ds_read_b128 (all lanes, one address: 4 weights per read).  A dense layer
// keeps 16 accumulators; per 4 inputs it issues 4 activation reads and 16 weight reads, then 64 fmaf.  (Reading the weights with
// scalar loads instead serialised on the scalar cache's latency: 120 us per launch at 65 536 envs.)  The MFMA alternative
// (v_mfma_f32_16x16x4_f32, exact f32 like the VALU) needs envs x outputs tiles through LDS; not built here.
//
// Numerics (the determinism contract).  x = (float)(obs / scale) with an f64 division, exactly torch's (obs / scale).float().  Every
// dense output is one fmaf chain that starts at the bias and adds W[j][k] * in[k] in increasing k; tanhf / expf / logf are the device
// library's.  An env's outputs depend on its own observation row, the parameters and its own uniform only: not on n_envs, the
// workgroup geometry, env_id_base (except through the Philox counter, which is the GLOBAL env id) or on whether the launch comes from
// ssg_policy_act or ssg_rollout_policy.
//
// Separate value network (SSG_POLICY_SEPARATE_VALUE, the SPLIT instantiations).  The pi tower runs dense, dense, then the logits head;
// the vf tower then runs the same device functions from the same row x, and ends in the value head: every output is the same kind of
// chain as above.  With two layers the shared plan overwrites x with the second layer's output; a launch that runs both towers keeps a
// third activation buffer for it instead, so that x survives for the vf tower (re-forming x would read the f64 observation rows twice).
// The value-only launch skips the pi tower, the dist kernel the vf tower: both keep the shared plan's two buffers.
//
// Time-out values (ssg_timeout_values / ssg_pop_timeout_values, -DSSG_POLICY_BOOT_TU): the value-only forward over the terminal
// observations of a rollout's K rows in one launch, for the waves whose flags hold a time-out (timeout_value_kernel, at the end of the
// kernels).
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kPolWave = 64;   // envs per workgroup (one wave)
constexpr int kPolStride = 65; // LDS floats per activation row: one per lane, +1 so that the obs pass's stores spread over the banks

__device__ __forceinline__ float activate(float v, int kind) { return kind == SSG_POLICY_RELU ? fmaxf(v, 0.0f) : tanhf(v); }

// Stage `rows` rows of a row-major [rows][K] weight block into the workgroup's weight tile (row stride K4 = K rounded up to 4, the
// padding zeroed), read linearly from global memory (coalesced).  The caller brackets it with barriers.
__device__ __forceinline__ void stage_rows(const float *__restrict__ W, int rows, int K, int K4, float *wt, int lane)
{
    for (int i = lane; i < rows * K; i += kPolWave) {
        const int r = i / K, c = i - r * K;
        wt[r * K4 + c] = W[i];
    }
    for (int i = lane; i < rows * (K4 - K); i += kPolWave) {
        const int r = i / (K4 - K), c = K + i - r * (K4 - K);
        wt[r * K4 + c] = 0.0f;
    }
}

// out[j] = activate(b[j] + sum_k W[j][k] * in[k]) for j < M (M a multiple of 16), W row-major [M][K]; in / out: LDS rows, this lane's
// column (in has K4 rows, those past K zero).  16 output rows at a time are staged in the weight tile; per 4 inputs a lane reads its
// 4 activations and, for each of the 16 outputs, the 4 weights as ONE broadcast ds_read_b128 (every lane reads the same address).
__device__ __forceinline__ void dense(const float *__restrict__ W, const float *__restrict__ b, int K, int M, int kind,
                                      const float *in, float *out, float *wt, int lane)
{
    const int K4 = (K + 3) & ~3;
    for (int j0 = 0; j0 < M; j0 += 16) {
        __syncthreads(); // (the previous tile's readers are done)
        stage_rows(W + (size_t)j0 * K, 16, K, K4, wt, lane);
        __syncthreads();
        float acc[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) acc[jj] = b[j0 + jj];
        for (int k = 0; k < K4; k += 4) {
            float v[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) v[t] = in[(k + t) * kPolStride + lane];
            // all 16 reads first, then the fmaf in t-major order: 16 independent chains between two dependent steps (each
            // accumulator still adds k, k+1, k+2, k+3 in order)
            float4 w[16];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) w[jj] = *reinterpret_cast<const float4 *>(wt + jj * K4 + k);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[jj] = fmaf(w[jj].x, v[0], acc[jj]);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[jj] = fmaf(w[jj].y, v[1], acc[jj]);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[jj] = fmaf(w[jj].z, v[2], acc[jj]);
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) acc[jj] = fmaf(w[jj].w, v[3], acc[jj]);
        }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) out[(j0 + jj) * kPolStride + lane] = activate(acc[jj], kind);
    }
}

// The heads over the last hidden layer h (this lane's column): P points at Wpi [A][H], bpi [A], Wv [1][H], bv [1].  Staged like a
// dense tile (rows 0..A-1 = Wpi, row 4 = Wv; H is a multiple of 16, so no padding); lg[j] for j >= A stays 0.
__device__ __forceinline__ void heads(const float *__restrict__ P, int H, int A, const float *h, float *wt, int lane, float (&lg)[4], float *v_out)
{
    const float *Wpi = P, *bpi = P + A * H, *Wv = bpi + A, *bv = Wv + H;
    __syncthreads();
    stage_rows(Wpi, A, H, H, wt, lane);
    stage_rows(Wv, 1, H, H, wt + 4 * H, lane);
    __syncthreads();
    float v = bv[0];
#pragma unroll
    for (int j = 0; j < 4; ++j) lg[j] = j < A ? bpi[j] : 0.0f;
    for (int k = 0; k < H; k += 4) {
        float hv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) hv[t] = h[(k + t) * kPolStride + lane];
        float4 w[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) w[j] = *reinterpret_cast<const float4 *>(wt + j * H + k); // (rows A..3 unused: never summed)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float hx = hv[t];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < A) lg[j] = fmaf(t == 0 ? w[j].x : t == 1 ? w[j].y : t == 2 ? w[j].z : w[j].w, hx, lg[j]);
            v = fmaf(t == 0 ? w[4].x : t == 1 ? w[4].y : t == 2 ? w[4].z : w[4].w, hx, v);
        }
    }
    *v_out = v;
}

// The two heads on their own (SPLIT): the chains of heads(), each over its own tower's last layer.  P points at Wpi [A][H], bpi [A].
__device__ __forceinline__ void head_pi(const float *__restrict__ P, int H, int A, const float *h, float *wt, int lane, float (&lg)[4])
{
    const float *Wpi = P, *bpi = P + A * H;
    __syncthreads();
    stage_rows(Wpi, A, H, H, wt, lane);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) lg[j] = j < A ? bpi[j] : 0.0f;
    for (int k = 0; k < H; k += 4) {
        float hv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) hv[t] = h[(k + t) * kPolStride + lane];
        float4 w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = *reinterpret_cast<const float4 *>(wt + j * H + k); // (rows A..3 unused: never summed)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float hx = hv[t];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < A) lg[j] = fmaf(t == 0 ? w[j].x : t == 1 ? w[j].y : t == 2 ? w[j].z : w[j].w, hx, lg[j]);
        }
    }
}

// P points at Wv [1][H], bv [1].
__device__ __forceinline__ float head_v(const float *__restrict__ P, int H, const float *h, float *wt, int lane)
{
    __syncthreads();
    stage_rows(P, 1, H, H, wt, lane);
    __syncthreads();
    float v = P[H];
    for (int k = 0; k < H; k += 4) {
        const float4 w = *reinterpret_cast<const float4 *>(wt + k);
        v = fmaf(w.x, h[(k + 0) * kPolStride + lane], v);
        v = fmaf(w.y, h[(k + 1) * kPolStride + lane], v);
        v = fmaf(w.z, h[(k + 2) * kPolStride + lane], v);
        v = fmaf(w.w, h[(k + 3) * kPolStride + lane], v);
    }
    return v;
}

// One tower's body from the x rows in bufA: Linear(D, H) + act [+ Linear(H, H) + act, into h2].  Returns the last layer's rows.
__device__ __forceinline__ const float *tower(const float *__restrict__ P, int D, int H, int L, int kind, const float *bufA, float *bufB,
                                              float *h2, float *wt, int lane)
{
    dense(P, P + H * D, D, H, kind, bufA, bufB, wt, lane);
    if (L != 2) return bufB;
    P += H * D + H;
    dense(P, P + H * H, H, H, kind, bufB, h2, wt, lane);
    return h2;
}

// log(sum_j exp(lg[j])) over j < A, the formula order of ppo_torch's log_softmax
__device__ __forceinline__ float log_sum_exp(const float (&lg)[4], int A)
{
    float m = lg[0];
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (j < A) m = fmaxf(m, lg[j]);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < A) s += expf(lg[j] - m);
    return m + logf(s);
}

// Step 1's element: x = (float)(obs / scale[d]); FILTER: (float)clamp((obs - mean[d]) / denom[d], -clip, +clip) from the rows staged in LDS
template <bool FILTER>
__device__ __forceinline__ float step1_x(double o, const double *__restrict__ scale, const double *fs, int d, int D, double clip)
{
    if constexpr (FILTER) {
        double v = (o - fs[d]) / fs[D + d];
        if (clip > 0.0) {
            v = v < -clip ? -clip : v;
            v = v > clip ? clip : v;
        }
        return (float)v;
    } else {
        return (float)(o / scale[d]);
    }
}

// (waves_per_eu(1, 2): lets the scheduler keep all 16 weight reads of a step in flight — 113 VGPRs — instead of two at a time)
//
// POP = false: ssg_policy_act's launch, n envs under one parameter buffer (plen unused).  POP = true: a population in one launch, grid
// (workgroups of n envs, members): member m = blockIdx.y owns the n envs [m*n, (m+1)*n) of every buffer and the parameter row
// params + m*plen, with a tail workgroup of its own, so an env's outputs are bit for bit those of the POP = false launch on that slice
// with that row (the same code below).  The Philox counter stays the global env id: env_base + m*n + e.
// SPLIT: the separate-value layout (p.activation carries SSG_POLICY_SEPARATE_VALUE); a launch with act_out runs both towers and has the
// third activation buffer behind bufB, the value-only launch runs the vf tower alone in the shared plan's two buffers.
// GREEDY (ssg_policy_act_greedy / ssg_pop_act_greedy, the evaluation loop): the same forward, then step 4 is the arg-max instead of a
// draw — no Philox round, `uniform` never read; value and x are the sampling launch's bit for bit.  A template parameter, so the four
// sampling instantiations keep their code.
// SLICED (with POP; ssg_pop_set_slices): the members' slices are unequal.  Member m = blockIdx.y owns the n_m envs from o_m on, row m
// = {o_m, n_m, ...} of the slices table; the grid is as wide as the largest slice needs, and a workgroup whose first env is past n_m
// leaves as a whole ahead of every barrier.  Nothing below relies on a member's base being a multiple of the wave: every global access
// is a scalar element of its row.  A kernel of its own takes the table, so the other instantiations keep their argument layout.
// FILTER (ssg_set_obs_filter): step 1 forms x from a running mean / std filter instead of the fixed scale.  `scale` then points at the
// filter's state rows, f64 [members][SSG_FILTER_ROWS][D] (mean, M2, denom, count), member m = blockIdx.y reads its own, and
// x = (float)clamp((obs - mean) / denom, -clip, +clip): subtraction, division and clamp in f64, one rounding to f32; clip == 0: no
// clamp; a denom entry of 0.0 (the rows of a state nothing was merged into yet) divides by 1.  Kernels of their own again (they take
// clip), built in an object of their own (-DSSG_POLICY_FILTER_TU), and everything FILTER adds sits under `if constexpr (FILTER)` or in
// step1_x: a declaration outside them, even an unused one, renumbers registers in the other instantiations.  Their device code is
// compared with the previous build's whenever this body changes (profiles/obs_filter/README.md).
template <bool POP, bool SPLIT, bool GREEDY, bool SLICED, bool FILTER = false>
__device__ __forceinline__ void policy_act_body(const ssg_policy &p, const float *__restrict__ params, const double *__restrict__ scale,
                                                int n, long long env_base, const double *__restrict__ obs,
                                                const float *__restrict__ uniform, uint64_t seed, int64_t step,
                                                int32_t *__restrict__ act_out, float *__restrict__ logp_out,
                                                float *__restrict__ value_out, float *__restrict__ x_out, int plen,
                                                const int32_t *__restrict__ slices, double clip = 0.0)
{
    static_assert(POP || !SLICED, "slices are a population's");
    extern __shared__ float4 lds4[];
    if (POP) { // the member's slice of every buffer
        size_t m0 = (size_t)blockIdx.y * (size_t)n;
        if (SLICED) {
            const int32_t *row = slices + (size_t)blockIdx.y * SSG_POP_SLICE_ROW;
            m0 = (size_t)row[0];
            n = row[1];
            if ((int)(blockIdx.x * kPolWave) >= n) return; // (uniform over the workgroup)
        }
        const size_t D = (size_t)p.obs_dim;
        params += (size_t)blockIdx.y * (size_t)plen;
        if constexpr (FILTER) scale += (size_t)blockIdx.y * SSG_FILTER_ROWS * D;
        env_base += (long long)m0;
        obs += m0 * D;
        if (!GREEDY && uniform) uniform += m0;
        if (act_out) act_out += m0;
        if (logp_out) logp_out += m0;
        if (value_out) value_out += m0;
        if (x_out) x_out += m0 * D;
    }
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * kPolWave;
    const int ne = (n - e0 < kPolWave) ? n - e0 : kPolWave; // tail workgroup: lanes >= ne store nothing
    const int D = p.obs_dim, H = p.hidden, A = p.n_actions;
    const int R4 = ((D > H ? D : H) + 3) & ~3;                // rows of bufA, and the weight tile's widest row
    float *wt = reinterpret_cast<float *>(lds4);              // weight tile: 16 rows x R4 (16-byte aligned rows of 4k floats)
    float *bufA = wt + 16 * R4;                               // x (rows D..R4 zero), then the second hidden layer
    float *bufB = bufA + R4 * kPolStride;                     // the first hidden layer

    // 1. x = (float)(obs / scale).  The workgroup's ne observation rows are ONE contiguous block of ne*D doubles: read it linearly
    // (coalesced), and write the x rows (same linear index, f32) the same way; element i is (env i / D, feature i % D), tracked
    // incrementally (64 = qd * D + rd).
    {
        const double *src = obs + (size_t)e0 * D;
        float *xdst = x_out ? x_out + (size_t)e0 * D : nullptr;
        const int total = ne * D, qd = kPolWave / D, rd = kPolWave % D;
        int d = lane % D, el = lane / D;
        if constexpr (FILTER) { // mean [D], then denom [D] (0 -> 1), staged in the weight tile, which is free until the first dense
            double *fs = reinterpret_cast<double *>(wt); // tile (its barrier follows this loop's last read)
            for (int i = lane; i < D; i += kPolWave) {
                const double den = scale[2 * D + i];
                fs[i] = scale[i];
                fs[D + i] = den == 0.0 ? 1.0 : den;
            }
            __syncthreads();
        }
        for (int i = lane; i < total; i += kPolWave) {
            const float xv = step1_x<FILTER>(src[i], scale, reinterpret_cast<const double *>(wt), d, D, clip);
            bufA[d * kPolStride + el] = xv;
            if (xdst) xdst[i] = xv;
            d += rd;
            el += qd;
            if (d >= D) { d -= D; ++el; }
        }
        for (int r = D; r < R4; ++r) bufA[r * kPolStride + lane] = 0.0f; // (padding rows: 0 * weight 0, never a NaN)
    }
    // (the first dense tile's barrier orders these stores before any lane reads another lane's column: after it every lane reads and
    // writes its own activation column only)

    float lg[4], v;
    if (SPLIT) {
        // 2s + 3s. each tower's body and its head; x stays in bufA while the vf tower still needs it
        const int L = p.n_hidden_layers, kind = p.activation & 0xff;
        const int T = H * D + H + (L - 1) * (H * H + H); // floats of one tower
        if (act_out) {
            const float *h = tower(params, D, H, L, kind, bufA, bufB, bufB + H * kPolStride, wt, lane);
            head_pi(params + T, H, A, h, wt, lane, lg);
        }
        const float *Pv = params + T + A * H + A;
        const float *h = tower(Pv, D, H, L, kind, bufA, bufB, bufA, wt, lane);
        v = head_v(Pv + T, H, h, wt, lane);
    } else {
        // 2. the body: Linear(D, H) + act [+ Linear(H, H) + act]
        const float *P = params;
        dense(P, P + H * D, D, H, p.activation, bufA, bufB, wt, lane);
        P += H * D + H;
        const float *h = bufB;
        if (p.n_hidden_layers == 2) {
            dense(P, P + H * H, H, H, p.activation, bufB, bufA, wt, lane);
            P += H * H + H;
            h = bufA;
        }

        // 3. the heads
        heads(P, H, A, h, wt, lane, lg, &v);
    }
    if (lane >= ne) return;
    const int e = e0 + lane;
    if (value_out) value_out[e] = v;
    if (!act_out) return; // (the bootstrap forward of ssg_rollout_policy: value only)

    if (GREEDY) {
        // 4g. a = the smallest j < A whose logit is the maximum (a later equal logit does not replace it), logp = lg[a] - lse: the
        // entry policy_dist_kernel writes for that action, bit for bit
        const float lse = log_sum_exp(lg, A);
        int a = 0;
        float best = lg[0];
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (j < A && lg[j] > best) { best = lg[j]; a = j; }
        act_out[e] = a;
        logp_out[e] = best - lse;
        return;
    }

    // 4. inverse-CDF sampling, the formula order of ppo_torch's Shard.step(): log_softmax, cumsum(exp), count(u > cdf[j]) over j < A-1
    const float lse = log_sum_exp(lg, A);
    float u;
    if (uniform) {
        u = uniform[e];
    } else { // Philox4x32-10, counter (global env, step), key = seed: fill_actions_kernel's stream, output word 1
        const uint64_t env = (uint64_t)(env_base + e), st = (uint64_t)step;
        uint32_t ctr[4] = {(uint32_t)env, (uint32_t)(env >> 32), (uint32_t)st, (uint32_t)(st >> 32)};
        uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            if (r) { key[0] += 0x9E3779B9u; key[1] += 0xBB67AE85u; }
            philox_round(ctr, key);
        }
        u = (float)(ctr[1] >> 8) * 0x1p-24f;
    }
    float cdf = 0.0f, lp = lg[0] - lse;
    int a = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j + 1 < A) {
            cdf += expf(lg[j] - lse);
            a += u > cdf ? 1 : 0;
        }
    }
    // A masked action (logit -inf, probability 0) is never drawn.  The f32 sum of the other actions' probabilities can round to
    // 1 - 2^-23 or less, and a u at the top of Philox's grid then counts past the last of them: step back to the action in front.
    // (A -inf logit ahead of the last adds 0 to cdf and is passed by both of its thresholds or by neither; action 0 stays the
    // answer to u = 0 whatever its logit.)
#pragma unroll
    for (int j = 3; j >= 1; --j)
        if (a == j && lg[j] == -INFINITY) a = j - 1;
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (a == j) lp = lg[j] - lse;
    act_out[e] = a;
    logp_out[e] = lp;
}

template <bool POP, bool SPLIT, bool GREEDY = false>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_act_kernel(const ssg_policy p, const float *__restrict__ params, const double *__restrict__ scale,
                                                              int n, long long env_base, const double *__restrict__ obs,
                                                              const float *__restrict__ uniform, uint64_t seed, int64_t step,
                                                              int32_t *__restrict__ act_out, float *__restrict__ logp_out,
                                                              float *__restrict__ value_out, float *__restrict__ x_out, int plen)
{
    policy_act_body<POP, SPLIT, GREEDY, false>(p, params, scale, n, env_base, obs, uniform, seed, step, act_out, logp_out, value_out, x_out, plen,
                                               nullptr);
}

// a population on unequal slices (no n: every member's is in the table)
template <bool SPLIT, bool GREEDY>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_act_sliced_kernel(const ssg_policy p, const float *__restrict__ params, const double *__restrict__ scale,
                                                              const int32_t *__restrict__ slices, long long env_base, const double *__restrict__ obs,
                                                              const float *__restrict__ uniform, uint64_t seed, int64_t step,
                                                              int32_t *__restrict__ act_out, float *__restrict__ logp_out,
                                                              float *__restrict__ value_out, float *__restrict__ x_out, int plen)
{
    policy_act_body<true, SPLIT, GREEDY, true>(p, params, scale, 0, env_base, obs, uniform, seed, step, act_out, logp_out, value_out, x_out, plen,
                                               slices);
}

// The acting policy's whole log-distribution over STORED x rows (ssg_ppo_dist / ssg_pop_dist): policy_act_kernel's forward from its
// step 2 on — the same dense, heads and log_sum_exp — so that logp_all[i][act[i]] is the rollout's logp[i] bit for bit.  Grid
// (workgroups of n rows, members, K): the workgroup's rows start at row blockIdx.z*N + blockIdx.y*n and run under parameter row
// blockIdx.y (one policy: members = 1, K = 1, n = the number of rows).  logp_all[i][j] = logit_j - lse for j < A, 0 for j >= A.
// SPLIT: the pi tower and the pi head open the packed row as the shared body and Wpi / bpi do, so the body code is the same and only
// the head differs; the vf tower is never read.
// SLICED: member blockIdx.y's rows of step blockIdx.z start at blockIdx.z*N + o_m and there are n_m of them (its row of the slices
// table); a workgroup past n_m leaves ahead of every barrier.  An x row at o_m*D floats is not 16-byte aligned: the rows are read
// element by element.  A logp_all row is 16 bytes per env whatever o_m is.
template <bool SPLIT, bool SLICED>
__device__ __forceinline__ void policy_dist_body(const ssg_policy &p, const float *__restrict__ params, int n, long long N,
                                                 const float *__restrict__ x, float *__restrict__ logp_all, int plen,
                                                 const int32_t *__restrict__ slices)
{
    extern __shared__ float4 lds4[];
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * kPolWave;
    size_t base = (size_t)blockIdx.y * (size_t)n;
    if (SLICED) {
        const int32_t *row = slices + (size_t)blockIdx.y * SSG_POP_SLICE_ROW;
        base = (size_t)row[0];
        n = row[1];
        if (e0 >= n) return; // (uniform over the workgroup)
    }
    const int ne = (n - e0 < kPolWave) ? n - e0 : kPolWave;
    const int D = p.obs_dim, H = p.hidden, A = p.n_actions;
    const size_t row0 = (size_t)blockIdx.z * (size_t)N + base + (size_t)e0;
    params += (size_t)blockIdx.y * (size_t)plen;
    const int R4 = ((D > H ? D : H) + 3) & ~3;
    float *wt = reinterpret_cast<float *>(lds4);
    float *bufA = wt + 16 * R4;
    float *bufB = bufA + R4 * kPolStride;
    {
        const float *src = x + row0 * D;
        const int total = ne * D, qd = kPolWave / D, rd = kPolWave % D;
        int d = lane % D, el = lane / D;
        for (int i = lane; i < total; i += kPolWave) {
            bufA[d * kPolStride + el] = src[i];
            d += rd;
            el += qd;
            if (d >= D) { d -= D; ++el; }
        }
        // (a tail workgroup's lanes >= ne compute on zeros and store nothing)
        if (lane >= ne)
            for (int r = 0; r < D; ++r) bufA[r * kPolStride + lane] = 0.0f;
        for (int r = D; r < R4; ++r) bufA[r * kPolStride + lane] = 0.0f;
    }
    const int kind = SPLIT ? (p.activation & 0xff) : p.activation;
    const float *P = params;
    dense(P, P + H * D, D, H, kind, bufA, bufB, wt, lane);
    P += H * D + H;
    const float *h = bufB;
    if (p.n_hidden_layers == 2) {
        dense(P, P + H * H, H, H, kind, bufB, bufA, wt, lane);
        P += H * H + H;
        h = bufA;
    }
    float lg[4], v;
    if (SPLIT) head_pi(P, H, A, h, wt, lane, lg);
    else heads(P, H, A, h, wt, lane, lg, &v);
    if (lane >= ne) return;
    const float lse = log_sum_exp(lg, A);
    float4 out;
    out.x = lg[0] - lse;
    out.y = 1 < A ? lg[1] - lse : 0.0f;
    out.z = 2 < A ? lg[2] - lse : 0.0f;
    out.w = 3 < A ? lg[3] - lse : 0.0f;
    float *dst = logp_all + (row0 + (size_t)lane) * 4;
    dst[0] = out.x;
    dst[1] = out.y;
    dst[2] = out.z;
    dst[3] = out.w;
}

template <bool SPLIT>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_dist_kernel(const ssg_policy p, const float *__restrict__ params, int n, long long N,
                                                               const float *__restrict__ x, float *__restrict__ logp_all, int plen)
{
    policy_dist_body<SPLIT, false>(p, params, n, N, x, logp_all, plen, nullptr);
}

template <bool SPLIT>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_dist_sliced_kernel(const ssg_policy p, const float *__restrict__ params,
                                                               const int32_t *__restrict__ slices, long long N,
                                                               const float *__restrict__ x, float *__restrict__ logp_all, int plen)
{
    policy_dist_body<SPLIT, true>(p, params, 0, N, x, logp_all, plen, slices);
}

#ifdef SSG_POLICY_FILTER_TU
template <bool POP, bool SPLIT, bool GREEDY>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_act_filter_kernel(const ssg_policy p, const float *__restrict__ params, const double *__restrict__ fstate,
                                                              int n, long long env_base, const double *__restrict__ obs,
                                                              const float *__restrict__ uniform, uint64_t seed, int64_t step,
                                                              int32_t *__restrict__ act_out, float *__restrict__ logp_out,
                                                              float *__restrict__ value_out, float *__restrict__ x_out, int plen, double clip)
{
    policy_act_body<POP, SPLIT, GREEDY, false, true>(p, params, fstate, n, env_base, obs, uniform, seed, step, act_out, logp_out, value_out, x_out,
                                                     plen, nullptr, clip);
}

template <bool SPLIT, bool GREEDY>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) policy_act_sliced_filter_kernel(const ssg_policy p, const float *__restrict__ params, const double *__restrict__ fstate,
                                                              const int32_t *__restrict__ slices, long long env_base, const double *__restrict__ obs,
                                                              const float *__restrict__ uniform, uint64_t seed, int64_t step,
                                                              int32_t *__restrict__ act_out, float *__restrict__ logp_out,
                                                              float *__restrict__ value_out, float *__restrict__ x_out, int plen, double clip)
{
    policy_act_body<true, SPLIT, GREEDY, true, true>(p, params, fstate, 0, env_base, obs, uniform, seed, step, act_out, logp_out, value_out, x_out,
                                                     plen, slices, clip);
}
#endif

#ifdef SSG_POLICY_BOOT_TU
// The time-out values of a rollout (ssg_timeout_values / ssg_pop_timeout_values): boot[k][e] = V(terminal observation of env e at step
// k) where the flags byte says the clock alone ended the episode, +0.0f elsewhere.  Grid (workgroups of n envs, members, K), policy_dist's
// geometry: workgroup (x, m, k) owns the envs [m0 + 64 x, ...) of member m (m0 = m*n, or its row of the slices table; one policy: members
// = 1, n = the envs) in row k: flags and boot k*stride entries in, the observation rows k*n_envs*D doubles into term_obs.  It reads its
// 64 flag bytes; with no time-out lane it writes +0.0f for its live lanes and leaves ahead of every barrier (uniform: one wave).
// Otherwise the value-only forward of policy_act_body on its rows — the same step1_x, dense, tower, heads / head_v, in its order, so a
// time-out's value is ssg_policy_act's dev_value for that row bit for bit — and per lane a SELECT: the rows of lanes the step did not
// reset hold stale or never-written memory (a NaN there must not reach boot through a product).  A filter's state rows are read, never
// updated.  A kernel of its own in an object of its own (-DSSG_POLICY_BOOT_TU): the other objects' device code stays what it is.
template <bool SPLIT, bool FILTER>
__global__ void __launch_bounds__(kPolWave) __attribute__((amdgpu_waves_per_eu(1, 2))) timeout_value_kernel(const ssg_policy p, const float *__restrict__ params, const double *__restrict__ scale,
                                                              int n, int n_envs, size_t stride, const int32_t *__restrict__ slices,
                                                              const uint8_t *__restrict__ flags, const double *__restrict__ term_obs,
                                                              float *__restrict__ boot, int plen, double clip)
{
    extern __shared__ float4 lds4[];
    size_t m0 = (size_t)blockIdx.y * (size_t)n;
    if (slices) {
        const int32_t *row = slices + (size_t)blockIdx.y * SSG_POP_SLICE_ROW;
        m0 = (size_t)row[0];
        n = row[1];
        if ((int)(blockIdx.x * kPolWave) >= n) return; // (uniform over the workgroup)
    }
    const int lane = threadIdx.x;
    const int e0 = blockIdx.x * kPolWave;
    const int ne = (n - e0 < kPolWave) ? n - e0 : kPolWave; // tail workgroup: lanes >= ne read no flag and store nothing
    const size_t k = blockIdx.z, o = k * stride + m0 + (size_t)e0 + (size_t)lane;
    bool timeout = false;
    if (lane < ne) {
        const unsigned f = flags[o];
        timeout = (f & SSG_EV_MAX_STEPS) != 0 && (f & (SSG_EV_COLLIDING | SSG_EV_OUT_OF_BOUNDS | SSG_EV_NO_GOALS_LEFT)) == 0;
    }
    if (!__any(timeout)) {
        if (lane < ne) boot[o] = 0.0f;
        return;
    }
    const int D = p.obs_dim, H = p.hidden, A = p.n_actions;
    params += (size_t)blockIdx.y * (size_t)plen;
    if constexpr (FILTER) scale += (size_t)blockIdx.y * SSG_FILTER_ROWS * (size_t)D;
    const int R4 = ((D > H ? D : H) + 3) & ~3;
    float *wt = reinterpret_cast<float *>(lds4);
    float *bufA = wt + 16 * R4;
    float *bufB = bufA + R4 * kPolStride;
    { // policy_act_body's step 1 on the workgroup's ne terminal-observation rows (no x rows are kept)
        const double *src = term_obs + ((k * (size_t)n_envs + m0) + (size_t)e0) * (size_t)D;
        const int total = ne * D, qd = kPolWave / D, rd = kPolWave % D;
        int d = lane % D, el = lane / D;
        if constexpr (FILTER) {
            double *fs = reinterpret_cast<double *>(wt);
            for (int i = lane; i < D; i += kPolWave) {
                const double den = scale[2 * D + i];
                fs[i] = scale[i];
                fs[D + i] = den == 0.0 ? 1.0 : den;
            }
            __syncthreads();
        }
        for (int i = lane; i < total; i += kPolWave) {
            bufA[d * kPolStride + el] = step1_x<FILTER>(src[i], scale, reinterpret_cast<const double *>(wt), d, D, clip);
            d += rd;
            el += qd;
            if (d >= D) { d -= D; ++el; }
        }
        for (int r = D; r < R4; ++r) bufA[r * kPolStride + lane] = 0.0f;
    }
    float v;
    if (SPLIT) { // the vf tower alone, in the shared plan's two buffers
        const int L = p.n_hidden_layers, kind = p.activation & 0xff;
        const int T = H * D + H + (L - 1) * (H * H + H);
        const float *Pv = params + T + A * H + A;
        const float *h = tower(Pv, D, H, L, kind, bufA, bufB, bufA, wt, lane);
        v = head_v(Pv + T, H, h, wt, lane);
    } else {
        const float *P = params;
        dense(P, P + H * D, D, H, p.activation, bufA, bufB, wt, lane);
        P += H * D + H;
        const float *h = bufB;
        if (p.n_hidden_layers == 2) {
            dense(P, P + H * H, H, H, p.activation, bufB, bufA, wt, lane);
            P += H * H + H;
            h = bufA;
        }
        float lg[4];
        heads(P, H, A, h, wt, lane, lg, &v);
    }
    if (lane < ne) boot[o] = timeout ? v : 0.0f;
}
#endif

} // namespace

static bool is_split(const ssg_policy &p) { return (p.activation & SSG_POLICY_SEPARATE_VALUE) != 0; }

// the dynamic-LDS limit of `count` kernels of a table
template <class Kernel>
static hipError_t raise_lds_limit(const Kernel *k, int count)
{
    for (int i = 0; i < count; ++i) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k[i]), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// One acting launch with an object's kernel for equal slices (or one policy) and its kernel for a slices table.  third: the kernels'
// third argument (the scale row, or the filter's state rows); extra: what they take after plen (the filter's clip).  A greedy launch
// writes act, logp and value (the callers refuse a NULL one) and reads no uniform, seed, step or env id.
template <class Kernel, class SlicedKernel, class... Extra>
static hipError_t launch_act(Kernel kernel, SlicedKernel sliced, const PolicyLaunch &l, const double *third, hipStream_t stream, Extra... extra)
{
    const ssg_policy &p = *l.policy;
    const dim3 grid((unsigned)((l.lay.n + kPolWave - 1) / kPolWave), (unsigned)l.lay.members);
    const size_t lds = policy_lds_bytes(p, l.greedy || l.act != nullptr);
    const int plen = l.pop ? ppo_packed_len(p) : 0;
    const float *uniform = l.greedy ? nullptr : l.uniform;
    const uint64_t seed = l.greedy ? 0 : l.seed;
    const int64_t step = l.greedy ? 0 : l.step;
    const long long env_base = l.greedy ? 0 : l.env_base;
    if (l.lay.slices)
        hipLaunchKernelGGL(sliced, grid, dim3(kPolWave), lds, stream, p, p.dev_params, third, l.lay.slices, env_base, l.obs, uniform, seed, step,
                           l.act, l.logp, l.value, l.x, plen, extra...);
    else
        hipLaunchKernelGGL(kernel, grid, dim3(kPolWave), lds, stream, p, p.dev_params, third, l.lay.n, env_base, l.obs, uniform, seed, step, l.act,
                           l.logp, l.value, l.x, plen, extra...);
    return hipGetLastError();
}

#ifdef SSG_POLICY_FILTER_TU
// the FILTER instantiations, indexed [population][split][greedy] and [split][greedy]
typedef decltype(&policy_act_filter_kernel<false, false, false>) FilterKernel;
typedef decltype(&policy_act_sliced_filter_kernel<false, false>) FilterSlicedKernel;
static const FilterKernel kFilter[2][2][2] = {
    {{policy_act_filter_kernel<false, false, false>, policy_act_filter_kernel<false, false, true>},
     {policy_act_filter_kernel<false, true, false>, policy_act_filter_kernel<false, true, true>}},
    {{policy_act_filter_kernel<true, false, false>, policy_act_filter_kernel<true, false, true>},
     {policy_act_filter_kernel<true, true, false>, policy_act_filter_kernel<true, true, true>}}};
static const FilterSlicedKernel kFilterSliced[2][2] = {{policy_act_sliced_filter_kernel<false, false>, policy_act_sliced_filter_kernel<false, true>},
                                                       {policy_act_sliced_filter_kernel<true, false>, policy_act_sliced_filter_kernel<true, true>}};

hipError_t prepare_policy_filter()
{
    const hipError_t e = raise_lds_limit(&kFilter[0][0][0], 8);
    return e != hipSuccess ? e : raise_lds_limit(&kFilterSliced[0][0], 4);
}

hipError_t launch_policy_filter(const PolicyLaunch &l, hipStream_t stream)
{
    const bool split = is_split(*l.policy);
    return launch_act(kFilter[l.pop][split][l.greedy], kFilterSliced[split][l.greedy], l, l.filter->state, stream, l.filter->clip);
}
#elif defined(SSG_POLICY_BOOT_TU)
// the time-out value instantiations, indexed [split][filter]
typedef decltype(&timeout_value_kernel<false, false>) TimeoutKernel;
static const TimeoutKernel kTimeout[2][2] = {{timeout_value_kernel<false, false>, timeout_value_kernel<false, true>},
                                             {timeout_value_kernel<true, false>, timeout_value_kernel<true, true>}};

hipError_t prepare_policy_boot() { return raise_lds_limit(&kTimeout[0][0], 4); }

hipError_t launch_timeout_values(const PolicyLaunch &l, const TimeoutLaunch &t, hipStream_t stream)
{
    const ssg_policy &p = *l.policy;
    const dim3 grid((unsigned)((l.lay.n + kPolWave - 1) / kPolWave), (unsigned)l.lay.members, (unsigned)t.K);
    hipLaunchKernelGGL(kTimeout[is_split(p)][l.filter != nullptr], grid, dim3(kPolWave), policy_lds_bytes(p, false), stream, p, p.dev_params,
                       l.filter ? l.filter->state : p.dev_obs_scale, l.lay.n, t.n_envs, t.stride, l.lay.slices, t.flags, t.term_obs, t.boot,
                       l.pop ? ppo_packed_len(p) : 0, l.filter ? l.filter->clip : 0.0);
    return hipGetLastError();
}
#else

// both_towers: a separate-value launch that samples actions too (two layers: the third activation buffer, H rows)
size_t policy_lds_bytes(const ssg_policy &p, bool both_towers)
{
    const size_t R4 = (size_t)(((p.obs_dim > p.hidden ? p.obs_dim : p.hidden) + 3) & ~3);
    const size_t third = is_split(p) && both_towers && p.n_hidden_layers == 2 ? (size_t)p.hidden : 0;
    return (16 * R4 + (R4 + (size_t)p.hidden + third) * kPolStride) * sizeof(float);
}

// The instantiations without a filter.  A kernel's place in the object file follows its first mention here, so the tables are in the
// order, and indexed in the order, that keeps the object's device code what it has been: on a slices table [greedy][split], on equal
// slices or for one policy [split][population], sampling ahead of policy_dist's pair and greedy behind it.
typedef decltype(&policy_act_kernel<false, false, false>) ActKernel;
typedef decltype(&policy_act_sliced_kernel<false, false>) ActSlicedKernel;
typedef decltype(&policy_dist_kernel<false>) DistKernel;
typedef decltype(&policy_dist_sliced_kernel<false>) DistSlicedKernel;
static const ActSlicedKernel kActSliced[2][2] = {{policy_act_sliced_kernel<false, false>, policy_act_sliced_kernel<true, false>},
                                                 {policy_act_sliced_kernel<false, true>, policy_act_sliced_kernel<true, true>}};
static const DistSlicedKernel kDistSliced[2] = {policy_dist_sliced_kernel<false>, policy_dist_sliced_kernel<true>};
static const ActKernel kAct[2][2] = {{policy_act_kernel<false, false, false>, policy_act_kernel<true, false, false>},
                                     {policy_act_kernel<false, true, false>, policy_act_kernel<true, true, false>}};
static const DistKernel kDist[2] = {policy_dist_kernel<false>, policy_dist_kernel<true>};
static const ActKernel kActGreedy[2][2] = {{policy_act_kernel<false, false, true>, policy_act_kernel<true, false, true>},
                                           {policy_act_kernel<false, true, true>, policy_act_kernel<true, true, true>}};

hipError_t prepare_policy()
{
    hipError_t e = raise_lds_limit(&kActSliced[0][0], 4);
    if (e == hipSuccess) e = raise_lds_limit(kDistSliced, 2);
    if (e == hipSuccess) e = raise_lds_limit(&kAct[0][0], 4);
    if (e == hipSuccess) e = raise_lds_limit(kDist, 2);
    if (e == hipSuccess) e = raise_lds_limit(&kActGreedy[0][0], 4);
    return e;
}

hipError_t launch_policy(const PolicyLaunch &l, hipStream_t stream)
{
    if (l.filter) return launch_policy_filter(l, stream);
    const bool split = is_split(*l.policy);
    return launch_act((l.greedy ? kActGreedy : kAct)[split][l.pop], kActSliced[l.greedy][split], l, l.policy->dev_obs_scale, stream);
}

hipError_t launch_policy_dist(const ssg_policy &p, const MemberLayout &lay, long long N, int K, const float *x, float *logp_all, hipStream_t stream)
{
    const dim3 grid((unsigned)((lay.n + kPolWave - 1) / kPolWave), (unsigned)lay.members, (unsigned)K);
    const size_t lds = policy_lds_bytes(p, false);
    if (lay.slices)
        hipLaunchKernelGGL(kDistSliced[is_split(p)], grid, dim3(kPolWave), lds, stream, p, p.dev_params, lay.slices, N, x, logp_all, ppo_packed_len(p));
    else
        hipLaunchKernelGGL(kDist[is_split(p)], grid, dim3(kPolWave), lds, stream, p, p.dev_params, lay.n, N, x, logp_all, ppo_packed_len(p));
    return hipGetLastError();
}

#endif // SSG_POLICY_FILTER_TU

} // namespace ssg
