// shipsim_ppo.hip — GAE and the PPO update on the device: ssg_ppo_gae / ssg_ppo_grad / ssg_ppo_adam / ssg_ppo_update (include/shipsim.h).
//
// What the reference's PPO2 does after every rollout inside model.learn (train/stable_baselines/ppo.py:90) and what train/ppo_torch.py
// does in eager PyTorch: GAE, advantage normalisation, then per minibatch the MLP forward, the clipped PPO loss, its backward and Adam.
//
// GAE.  One lane per env walks t = K-1 .. 0 over coalesced [K][N] rows with the trainer's f32 operations in its order (bitwise equal),
// and sums adv / adv^2 in f64 per workgroup; a one-workgroup kernel adds those partials in a fixed order into mean, std + adv_eps and
// its inverse, which the gradient kernel reads from the workspace.
//
// Gradient.  A workgroup (4 waves) takes tiles of 64 samples: the gathered inputs, every layer's activations and the backward deltas
// of a tile live in LDS as [sample][feature] rows (stride +1 float against bank conflicts).  The three matrix products per layer —
// forward Z = In·Wᵀ, backward dIn = dZ·W and the weight gradient dW = dZᵀ·In (a contraction over the tile's samples) — run on
// v_mfma_f32_16x16x4_f32 (exact f32: a k-ordered fmaf chain), one 16x16 output tile per wave at a time; the forward and dIn products
// read their B operand (the weights) from global memory (L2-resident) and keep 4 row-tile accumulators per weight fragment.  The heads
// (A <= 4 logits and the value) and the per-sample loss run on the VALU, one lane per sample.  A workgroup accumulates its tiles'
// weight gradients in its own slot of the caller's workspace (read-modify-write by the lane that owns the entry, so in tile order),
// its bias / head gradients and loss sums in registers; a second kernel adds the slots (a fixed tree) and, for an update, applies
// Adam to the packed parameters in place.  Deterministic for a given M (the grid depends on M only); no floating-point atomics.
// (A population on per-member schedules, the SCHED instantiations, keeps that: member m's tiles are dealt to ppo_grid(M_m) workgroups
// of a wider launch, and its reduction adds those ppo_grid(M_m) slots.)
//
// Separate value network (SSG_POLICY_SEPARATE_VALUE, the SPLIT instantiations).  The logits' deltas depend on the pi tower alone and the
// value's on the vf tower alone, so a tile runs the body below once per tower over the same LDS: the sample scalars and the X rows are
// loaded once, then the pi pass (forward over W0 / W1, logits, the policy, entropy and KL terms, backward into the pi tower's and pi
// head's slot entries) and the vf pass (forward over V0 / V1, the value and its loss, backward into the vf tower's and vf head's).
// No LDS beyond the shared plan's.
//
// Data parallel (ssg_ppo_adv_moments / ssg_ppo_set_adv_moments / ssg_ppo_apply_shards): three small kernels at the end of the file
// make the advantage statistics job-wide and apply the gathered gradient rows of W shards, the same arithmetic on every rank.
#include <cmath>
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kTile = 64;     // samples per tile
constexpr int kPpoBlock = 256; // threads of the gradient kernel (4 waves)

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float activate(float v, int kind) { return kind == SSG_POLICY_RELU ? fmaxf(v, 0.0f) : tanhf(v); }
// autograd's derivative from the stored output: tanh' = 1 - y*y; ReLU' = (y > 0)
__device__ __forceinline__ float dactivate(float y, int kind) { return kind == SSG_POLICY_RELU ? (y > 0.0f ? 1.0f : 0.0f) : 1.0f - y * y; }

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// x[0] + ... + x[N-1] as a pairwise tree (N a power of 2; x is overwritten).  Long f32 sums of the gradient run as trees, as torch's
// reductions do: a 64- or 512-term chain loses several times torch's accuracy on cancelling or repeated terms.
template <int N> __device__ __forceinline__ float tree_sum(float *x)
{
#pragma unroll
    for (int w = N / 2; w > 0; w >>= 1)
#pragma unroll
        for (int i = 0; i < w; ++i) x[i] = x[i] + x[i + w];
    return x[0];
}

// sum over the tile's 64 samples of v[s * stride]: 8 interleaved partial sums, then a tree
__device__ __forceinline__ float tile_sum(const float *v, int stride)
{
    float t[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int s = 0; s < kTile; s += 8)
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r] += v[(s + r) * stride];
    return tree_sum<8>(t);
}

// ------------------------------------------------------------------------------------------------------------------------------
// GAE
// ------------------------------------------------------------------------------------------------------------------------------
// The walk of workgroup blockIdx.x's 256 envs out of n, over [K] rows that are N apart (the body of both GAE kernels; every pointer
// is the first env's of the batch the workgroup belongs to, rs / rq its 2 x 256 doubles of LDS).
// BOOT (ssg_ppo_gae_boot / ssg_pop_gae_boot): a done sample's one-step target is boot[i] (the value of a timed-out episode's terminal
// observation, +0 for a true terminal) instead of 0 — a select; the lambda chain is cut at every done as before.  Kernels of their own
// below the three walks; everything BOOT adds sits under `if constexpr (BOOT)`, so the three kernels without it keep their code
// (how to check: profiles/timeout_boot/README.md).
template <bool BOOT = false>
__device__ __forceinline__ void gae_body(int K, int N, int n, const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                         const float *__restrict__ val, const float *__restrict__ last_val, float *__restrict__ adv_out,
                                         float *__restrict__ ret_out, float gf, float glf, double2 *__restrict__ part, double *rs, double *rq,
                                         const float *__restrict__ boot = nullptr)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0, q = 0.0;
    if (e < n) {
        float nxt = last_val[e], adv = 0.0f;
        for (int t = K - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + e;
            const float nonterm = 1.0f - (float)done[i], v = val[i];
            float delta;
            if constexpr (BOOT) {
                const float bt = boot[i]; // (read for every sample, with the row's other loads: not a load that waits for done[i])
                const float tgt = done[i] ? bt : nxt;
                delta = ((float)rew[i] + gf * tgt) - v;
            } else {
                delta = ((float)rew[i] + (gf * nxt) * nonterm) - v;
            }
            adv = delta + (glf * nonterm) * adv;
            adv_out[i] = adv;
            ret_out[i] = adv + v;
            nxt = v;
            s += (double)adv;
            q += (double)adv * (double)adv;
        }
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rs[threadIdx.x] += rs[threadIdx.x + w];
            rq[threadIdx.x] += rq[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = make_double2(rs[0], rq[0]);
}

__global__ void __launch_bounds__(256) ppo_gae_kernel(int K, int N, const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                      const float *__restrict__ val, const float *__restrict__ last_val,
                                                      float *__restrict__ adv_out, float *__restrict__ ret_out, float gf, float glf,
                                                      double2 *__restrict__ part)
{
    __shared__ double rs[256], rq[256];
    gae_body(K, N, N, rew, done, val, last_val, adv_out, ret_out, gf, glf, part, rs, rq);
}

// The per-member constants of a population (ssg_pop_pack_hparams derives them on the host with loss_row and adam_args, the functions
// one policy's launches take theirs from): kPopTableRow floats per member — lo, hi, clip, vf, ent, adv_eps, gamma, gamma*lam — then
// per Adam step kPopTableRow floats per member: AdamArgs' seven fields (adam_to_row).
enum { PT_LO = 0, PT_HI, PT_CLIP, PT_VF, PT_ENT, PT_ADV_EPS, PT_GF, PT_GLF };

// GAE of a population: member m = blockIdx.y owns columns [m*n, (m+1)*n) of the [K][N] buffers, walks them with its own gamma /
// lambda, and lays its partial sums out as a run over n envs does (256-env blocks from the member's first env: part[m*nb + block]).
__global__ void __launch_bounds__(256) pop_gae_kernel(int K, int N, int n, int nb, const double *__restrict__ rew,
                                                      const uint8_t *__restrict__ done, const float *__restrict__ val,
                                                      const float *__restrict__ last_val, float *__restrict__ adv_out,
                                                      float *__restrict__ ret_out, const float *__restrict__ table, double2 *__restrict__ part)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.y, e0 = m * (size_t)n;
    gae_body(K, N, n, rew + e0, done + e0, val + e0, last_val + e0, adv_out + e0, ret_out + e0, table[m * kPopTableRow + PT_GF],
             table[m * kPopTableRow + PT_GLF], part + m * (size_t)nb, rs, rq);
}

// GAE of a population on unequal slices (ssg_pop_set_slices), grid (blocks of the largest slice, members): member m walks its n_m
// columns from o_m on (its row of the slices table) and lays its partial sums out as a run over n_m envs does, in its row of the
// [members][nb] partials (nb: the blocks of the largest slice).  A workgroup past n_m leaves ahead of every barrier.
__global__ void __launch_bounds__(256) pop_gae_sliced_kernel(int K, int N, const int32_t *__restrict__ slices, int nb,
                                                             const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                             const float *__restrict__ val, const float *__restrict__ last_val,
                                                             float *__restrict__ adv_out, float *__restrict__ ret_out,
                                                             const float *__restrict__ table, double2 *__restrict__ part)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.y, e0 = (size_t)slices[m * SSG_POP_SLICE_ROW];
    const int n = slices[m * SSG_POP_SLICE_ROW + 1];
    if ((int)(blockIdx.x * 256) >= n) return; // (uniform over the workgroup)
    gae_body(K, N, n, rew + e0, done + e0, val + e0, last_val + e0, adv_out + e0, ret_out + e0, table[m * kPopTableRow + PT_GF],
             table[m * kPopTableRow + PT_GLF], part + m * (size_t)nb, rs, rq);
}

// The three walks above with BOOT: the same geometry, partials and argument order, plus the boot rows (N apart, like every buffer).
__global__ void __launch_bounds__(256) ppo_gae_boot_kernel(int K, int N, const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                           const float *__restrict__ val, const float *__restrict__ last_val,
                                                           float *__restrict__ adv_out, float *__restrict__ ret_out, float gf, float glf,
                                                           double2 *__restrict__ part, const float *__restrict__ boot)
{
    __shared__ double rs[256], rq[256];
    gae_body<true>(K, N, N, rew, done, val, last_val, adv_out, ret_out, gf, glf, part, rs, rq, boot);
}

__global__ void __launch_bounds__(256) pop_gae_boot_kernel(int K, int N, int n, int nb, const double *__restrict__ rew,
                                                           const uint8_t *__restrict__ done, const float *__restrict__ val,
                                                           const float *__restrict__ last_val, float *__restrict__ adv_out,
                                                           float *__restrict__ ret_out, const float *__restrict__ table,
                                                           double2 *__restrict__ part, const float *__restrict__ boot)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.y, e0 = m * (size_t)n;
    gae_body<true>(K, N, n, rew + e0, done + e0, val + e0, last_val + e0, adv_out + e0, ret_out + e0, table[m * kPopTableRow + PT_GF],
                   table[m * kPopTableRow + PT_GLF], part + m * (size_t)nb, rs, rq, boot + e0);
}

__global__ void __launch_bounds__(256) pop_gae_boot_sliced_kernel(int K, int N, const int32_t *__restrict__ slices, int nb,
                                                                  const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                                  const float *__restrict__ val, const float *__restrict__ last_val,
                                                                  float *__restrict__ adv_out, float *__restrict__ ret_out,
                                                                  const float *__restrict__ table, double2 *__restrict__ part,
                                                                  const float *__restrict__ boot)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.y, e0 = (size_t)slices[m * SSG_POP_SLICE_ROW];
    const int n = slices[m * SSG_POP_SLICE_ROW + 1];
    if ((int)(blockIdx.x * 256) >= n) return; // (uniform over the workgroup)
    gae_body<true>(K, N, n, rew + e0, done + e0, val + e0, last_val + e0, adv_out + e0, ret_out + e0, table[m * kPopTableRow + PT_GF],
                   table[m * kPopTableRow + PT_GLF], part + m * (size_t)nb, rs, rq, boot + e0);
}

// stats[0] = mean, stats[1] = std + adv_eps (unbiased std, as torch's .std()), stats[2] = 1 / stats[1]
__device__ __forceinline__ void gae_stats_body(const double2 *__restrict__ part, int nblocks, double n, float adv_eps,
                                               float *__restrict__ stats, double *rs, double *rq)
{
    double s = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        s += part[b].x;
        q += part[b].y;
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rs[threadIdx.x] += rs[threadIdx.x + w];
            rq[threadIdx.x] += rq[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = rs[0] / n;
        double var = (rq[0] - rs[0] * mean) / (n - 1.0);
        if (var < 0.0) var = 0.0;
        const float stdp = (float)sqrt(var) + adv_eps;
        stats[0] = (float)mean;
        stats[1] = stdp;
        stats[2] = 1.0f / stdp;
        stats[3] = 0.0f;
    }
}

__global__ void __launch_bounds__(256) ppo_gae_stats_kernel(const double2 *__restrict__ part, int nblocks, double n, float adv_eps,
                                                            float *__restrict__ stats)
{
    __shared__ double rs[256], rq[256];
    gae_stats_body(part, nblocks, n, adv_eps, stats, rs, rq);
}

// one workgroup per member: the member's nblocks partials in the single run's order, into stats[m][4]
__global__ void __launch_bounds__(256) pop_gae_stats_kernel(const double2 *__restrict__ part, int nblocks, double n,
                                                            const float *__restrict__ table, float *__restrict__ stats)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.x;
    gae_stats_body(part + m * (size_t)nblocks, nblocks, n, table[m * kPopTableRow + PT_ADV_EPS], stats + m * 4, rs, rq);
}

// on unequal slices: the member's block count and its divisor K * n_m come from its row of the slices table; nb: the partials' row length
__global__ void __launch_bounds__(256) pop_gae_stats_sliced_kernel(const double2 *__restrict__ part, int nb, int K,
                                                                   const int32_t *__restrict__ slices, const float *__restrict__ table,
                                                                   float *__restrict__ stats)
{
    __shared__ double rs[256], rq[256];
    const size_t m = blockIdx.x;
    const int32_t *row = slices + m * SSG_POP_SLICE_ROW;
    gae_stats_body(part + m * (size_t)nb, row[2], (double)K * (double)row[1], table[m * kPopTableRow + PT_ADV_EPS], stats + m * 4, rs, rq);
}

// ------------------------------------------------------------------------------------------------------------------------------
// the minibatch gradient
// ------------------------------------------------------------------------------------------------------------------------------
struct GradArgs {
    int D, H, L, A, kind; // (kind: the activation's low byte)
    const float *params;
    const float *x;
    const int32_t *act;
    const float *logp, *adv, *ret;
    const int64_t *idx;
    long long M, n_samples;
    const float *stats; // mean, std + adv_eps (ssg_ppo_gae)
    float *slots;       // [grid][P + 4]
    int P;
    float lo, hi, clip, vf, ent, invM;
};

// out[s][col] = act(bias[col] + sum_k in[s][k] * W[col][k]) for the tile's 64 rows; W global row-major [NT*16][K]; K4 = K rounded up
// to 4 (in's columns K..K4 are zero).  Wave `wave` takes output column tiles wave, wave+4, ...; per k-step one weight fragment
// feeds the 4 row tiles.
__device__ __forceinline__ void mm_forward(const float *__restrict__ W, const float *__restrict__ bias, int K, int K4, int NT,
                                           const float *in, int sin, float *out, int sout, int kind, int wave, int lane)
{
    const int r16 = lane & 15, kq = lane >> 4;
    for (int ct = wave; ct < NT; ct += 4) {
        const int col = ct * 16 + r16;
        const float *wrow = W + (size_t)col * K;
        f4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int k0 = 0; k0 < K4; k0 += 4) {
            const int k = k0 + kq;
            const float b = k < K ? wrow[k] : 0.0f;
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(in[(rt * 16 + r16) * sin + k], b, acc[rt]);
        }
        const float bb = bias[col];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(rt * 16 + kq * 4 + r) * sout + col] = activate(acc[rt][r] + bb, kind);
    }
}

// out[s][col] = (sum_j dz[s][j] * W[j][col]) * act'(y[s][col]): the delta of the layer below, W global row-major [H][H].
__device__ __forceinline__ void mm_backward(const float *__restrict__ W, int H, const float *dz, const float *y, float *out, int sh,
                                            int kind, int wave, int lane)
{
    const int r16 = lane & 15, kq = lane >> 4, NT = H / 16;
    for (int ct = wave; ct < NT; ct += 4) {
        const int col = ct * 16 + r16;
        f4 acc[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) acc[rt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int j0 = 0; j0 < H; j0 += 4) {
            const float b = W[(size_t)(j0 + kq) * H + col];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = mfma4(dz[(rt * 16 + r16) * sh + j0 + kq], b, acc[rt]);
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rt * 16 + kq * 4 + r;
                out[row * sh + col] = acc[rt][r] * dactivate(y[row * sh + col], kind);
            }
    }
}

// g[j][k] (+)= sum_s dz[s][j] * in[s][k] over the tile's 64 samples, j < NTj*16, k < Kcols (g row-major, row stride Kcols; in's
// columns up to NTk*16 exist, those past Kcols are zero and not stored).  first: this workgroup's first tile (store, not add).
__device__ __forceinline__ void mm_wgrad(const float *dz, int sdz, const float *in, int sin, int NTj, int NTk, int Kcols, float *g,
                                         bool first, int wave, int lane)
{
    const int r16 = lane & 15, kq = lane >> 4;
    for (int t = wave; t < NTj * NTk; t += 4) {
        const int jt = t / NTk, kt = t - jt * NTk;
        const int col = kt * 16 + r16;
        f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int s0 = 0; s0 < kTile; s0 += 4) {
            const int s = s0 + kq;
            acc = mfma4(dz[s * sdz + jt * 16 + r16], in[s * sin + col], acc);
        }
        if (col < Kcols) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float *dst = g + (size_t)(jt * 16 + kq * 4 + r) * Kcols + col;
                *dst = first ? acc[r] : *dst + acc[r];
            }
        }
    }
}

// What a population's launch adds to GradArgs (whose params / idx / stats / slots are then member 0's and whose lo .. ent are unused).
struct PopGradArgs {
    long long n, N;       // envs per member, envs of the batch: member m's sample i = t*n + e is row t*N + m*n + e of the [K][N] buffers
    long long idx_stride; // int64 entries between two members' index rows
    const float *table;   // [members][kPopTableRow]
};

// What a population on unequal slices adds (the SLICED instantiations; ssg_pop_set_slices): member m's envs are [o_m, o_m + n_m), its
// row of `slices`; its samples are K * n_m, sample i = t*n_m + e is row t*N + o_m + e; its permutation block starts perm_epochs * (the
// int64 at SH_PREFIX of its header row of the schedule table) entries into idx.
struct SliceGradArgs {
    const int32_t *slices, *sched_hdr;
    long long K, perm_epochs;
};

// What the extended loss (ssg_ppo_grad_ext / ssg_ppo_update_ext / ssg_pop_update_ext) adds to GradArgs.  A term is off for a member
// whose constant is <= 0 (or whose pointer is NULL): its samples then take exactly the operations of the plain loss.
struct ExtGradArgs {
    const float *logp_all; // f32 [rows][4]: the acting policy's log-distribution (ssg_ppo_dist); read where the KL term is on
    const float *v_old;    // f32 [rows]: the rollout's value prediction; read where the value clip is on
    const float *kl_coef;  // device f32 [members] (one policy: [1]); NULL = no KL term
    const float *pop_ext;  // POP: f32 [members][kPopExtRow] = vf_clip, max_grad_norm, kl_target, 0
    float vf_clip;         // one policy: the value clip range (<= 0 = off)
};

// POP = false: ssg_ppo_grad's launch (pa unused).  POP = true: the minibatch gradient of every member in one launch, grid
// (ppo_grid(M), members): member m = blockIdx.y reads parameter row m, its own index row (member-local indices), its advantage
// statistics (stats + 4m) and loss constants (table row m), and owns the slots [m*grid, (m+1)*grid) — what the POP = false launch
// computes for that member alone, tile for tile (the same code below).
// EXT = false: the loss of ssg_ppo_grad (ea unused), slots of P + 4 floats.  EXT = true: plus the value clip and the KL penalty,
// slots of P + kExtStats floats (the loss sums pg, VL, entropy, clip fraction, KL, then zeros).
// SPLIT = false: the shared body (one pass per tile: pi and vf below are both true, constants).  SPLIT = true: two passes per tile.
// SCHED (with POP): the members are on schedules of their own (ssg_pop_update_sched).  The launch is as wide as the longest minibatch
// in the call needs, grid (ppo_grid(max C_m), members); member m's record of this launch gives ITS minibatch length M_m, its
// offset into its permutation rows and G_m = ppo_grid(M_m) (0 when it has no minibatch left).  Workgroups blockIdx.x >= G_m leave
// before the first barrier; the others deal the member's tiles among G_m — exactly the workgroups, tiles and slots of the POP = false
// launch for M_m alone.  A template flag, not a nullable pointer, and kernels of their own that take the records (sched: this
// launch's [members][kPopSchedRow], shipsim_internal.h) as one more argument: the other instantiations keep their argument layout and
// compile from the text they had.
// SLICED (with SCHED): unequal slices, see SliceGradArgs; kernels of their own again.  Everything behind the gather — tiles, slots,
// the reduction — depends on M_m and G_m alone, so it is the SCHED code unchanged.
template <bool POP, bool EXT, bool SPLIT, bool SCHED, bool SLICED = false>
__device__ __forceinline__ void ppo_grad_body(const GradArgs &a_, const PopGradArgs &pa, const ExtGradArgs &ea, const int32_t *sched,
                                              const SliceGradArgs &sa = SliceGradArgs{})
{
    static_assert(POP || !SCHED, "a schedule is a population's");
    static_assert(SCHED || !SLICED, "unequal slices run on schedules");
    extern __shared__ float4 lds4[];
    float *lds = reinterpret_cast<float *>(lds4);
    GradArgs a = a_;
    const int SS = a_.P + (EXT ? kExtStats : 4); // floats per slot
    float vf_clip = 0.0f, kl_coef = 0.0f;
    if (EXT) {
        vf_clip = POP ? ea.pop_ext[(size_t)blockIdx.y * kPopExtRow] : ea.vf_clip;
        kl_coef = ea.kl_coef ? ea.kl_coef[POP ? blockIdx.y : 0] : 0.0f;
    }
    const bool vclip_on = EXT && vf_clip > 0.0f, kl_on = EXT && kl_coef > 0.0f;
    if (POP) {
        const size_t m = blockIdx.y;
        a.params += m * (size_t)a.P;
        if (!SLICED) a.idx += m * (size_t)pa.idx_stride;
        a.stats += m * 4;
        a.slots += m * (size_t)gridDim.x * (size_t)SS;
        const float *row = pa.table + m * kPopTableRow;
        a.lo = row[PT_LO];
        a.hi = row[PT_HI];
        a.clip = row[PT_CLIP];
        a.vf = row[PT_VF];
        a.ent = row[PT_ENT];
    }
    long long mem_n = pa.n, mem_base = POP ? (long long)blockIdx.y * pa.n : 0; // the member's envs and its first env
    if (SLICED) {
        const int32_t *row = sa.slices + (size_t)blockIdx.y * SSG_POP_SLICE_ROW;
        mem_base = row[0];
        mem_n = row[1];
        a.n_samples = sa.K * mem_n;
        a.idx += sa.perm_epochs * *reinterpret_cast<const long long *>(sa.sched_hdr + (size_t)blockIdx.y * kPopSchedRow + SH_PREFIX);
    }
    unsigned gm = 0; // SCHED: the member's own grid, the workgroups that share its tiles
    if (SCHED) {
        const int32_t *rec = sched + (size_t)blockIdx.y * kPopSchedRow;
        gm = (unsigned)rec[SR_G];
        if (blockIdx.x >= gm) return; // (uniform over the workgroup, and ahead of every barrier)
        a.M = rec[SR_M];
        a.idx += *reinterpret_cast<const long long *>(rec + SR_OFF);
        a.invM = __int_as_float(rec[SR_INVM]);
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, H = a.H, A = a.A, kind = a.kind, NT = H / 16;
    const int DT = (D + 15) / 16, D4 = (D + 3) & ~3;
    const int SX = DT * 16 + 1, SH = H + 1;
    // LDS: X [64][SX] | HB0 [64][SH] | HB1 [64][SH] (2 layers) | DZ [64][SH] | WH [5][H] | DLOG [64][4] | DV [64] | sample scalars
    float *X = lds;
    float *HB0 = X + kTile * SX;
    float *HB1 = HB0 + kTile * SH;
    float *DZ = HB1 + (a.L == 2 ? kTile * SH : 0);
    float *WH = DZ + kTile * SH;
    float *DLOG = WH + 5 * H;
    float *DV = DLOG + kTile * 4;
    float *SLOGP = DV + kTile, *SADV = SLOGP + kTile, *SRET = SADV + kTile, *RED = SRET + kTile;
    int *SACT = reinterpret_cast<int *>(RED + kTile * 4);
    long long *SIDX = reinterpret_cast<long long *>(SACT + kTile); // (8-byte aligned: every region above is a multiple of 2 floats)
    // EXT: | v_old [64] | logp_old [64][4] | the fifth loss sum [64]
    float *SVOLD = reinterpret_cast<float *>(SIDX + kTile), *SLPO = SVOLD + kTile, *RED5 = SLPO + kTile * 4;

    // packed offsets (include/shipsim.h)
    const float *P = a.params;
    const int T = H * D + H + (a.L - 1) * (H * H + H); // floats of one tower (the shared body)
    const float *Wpi = P + T;
    const float *bpi = Wpi + A * H, *Wv = bpi + A + (SPLIT ? T : 0), *bv = Wv + H;
    float *g = a.slots + (size_t)blockIdx.x * SS;
    float *gWpi = g + (Wpi - P), *gbpi = g + (bpi - P), *gWv = g + (Wv - P), *gbv = g + (bv - P);

    for (int i = tid; i < kTile * SX; i += kPpoBlock) X[i] = 0.0f; // (the padding columns stay zero)
    for (int i = tid; i < 5 * H; i += kPpoBlock) {
        const int j = i / H, k = i - j * H;
        WH[i] = j < A ? Wpi[j * H + k] : (j == 4 ? Wv[k] : 0.0f);
    }
    const float mean = a.stats[0], stdp = a.stats[1];
    const float *HL = a.L == 2 ? HB1 : HB0; // the last hidden layer
    float accb0 = 0.0f, accb1 = 0.0f, accb0v = 0.0f, accb1v = 0.0f; // (...v: the vf tower's, SPLIT)
    float accW[4] = {0.0f, 0.0f, 0.0f, 0.0f}, accWv = 0.0f, accbh = 0.0f;
    float st_pg = 0.0f, st_vl = 0.0f, st_en = 0.0f, st_cf = 0.0f, st_kl = 0.0f;
    const long long ntiles = (a.M + kTile - 1) / kTile;
    bool first = true;
    for (long long tile = blockIdx.x; tile < ntiles; tile += SCHED ? gm : gridDim.x) {
        // 1. the tile's sample scalars, then its x rows (a row outside [0, n_samples) is a zero, gradient-free sample)
        if (tid < kTile) {
            const long long i = tile * kTile + tid;
            long long j = i < a.M ? a.idx[i] : -1;
            if (j >= a.n_samples) j = -1;
            if (POP && j >= 0) {
                const long long t = j / mem_n;
                j = t * pa.N + mem_base + (j - t * mem_n);
            }
            SIDX[tid] = j;
            if (j >= 0) {
                SACT[tid] = a.act[j];
                SLOGP[tid] = a.logp[j];
                SADV[tid] = (a.adv[j] - mean) / stdp;
                SRET[tid] = a.ret[j];
                if (vclip_on) SVOLD[tid] = ea.v_old[j];
                if (kl_on) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) SLPO[tid * 4 + c] = ea.logp_all[(size_t)j * 4 + c];
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < kTile * D; i += kPpoBlock) {
            const int s = i / D, d = i - s * D;
            const long long j = SIDX[s];
            X[s * SX + d] = j >= 0 ? a.x[(size_t)j * D + d] : 0.0f;
        }
        __syncthreads();
        for (int pass = 0; pass < (SPLIT ? 2 : 1); ++pass) {
        // which heads this pass serves, and its tower in the packed row and in the slot
        const bool pi = !SPLIT || pass == 0, vf = !SPLIT || pass == 1;
        const int to = pass * (T + A * H + A);
        const float *W0 = P + to, *b0 = W0 + H * D;
        const float *W1 = b0 + H, *b1 = W1 + H * H;
        float *gW0 = g + to, *gW1 = gW0 + H * D + H;
        // 2. forward body
        mm_forward(W0, b0, D, D4, NT, X, SX, HB0, SH, kind, wave, lane);
        __syncthreads();
        if (a.L == 2) {
            mm_forward(W1, b1, H, H, NT, HB0, SH, HB1, SH, kind, wave, lane);
            __syncthreads();
        }
        // 3. heads, loss and its gradient wrt the logits and the value: one lane per sample
        if (tid < kTile) {
            const int s = tid;
            float lg[4], v = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) lg[j] = 0.0f;
            const float *h = HL + s * SH;
            for (int k = 0; k < H; ++k) {
                const float hk = h[k];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pi && j < A) lg[j] = fmaf(WH[j * H + k], hk, lg[j]);
                if (vf) v = fmaf(WH[4 * H + k], hk, v);
            }
            float dl[4] = {0.0f, 0.0f, 0.0f, 0.0f}, dv = 0.0f;
            if (pi && SIDX[s] >= 0) {
                float m = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < A) {
                        lg[j] += bpi[j];
                        m = fmaxf(m, lg[j]);
                    }
                float se = 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < A) se += expf(lg[j] - m);
                const float lse = m + logf(se);
                float lp[4], p[4], ent = 0.0f, lpa = 0.0f;
                const int act = SACT[s];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lp[j] = j < A ? lg[j] - lse : 0.0f;
                    p[j] = j < A ? expf(lp[j]) : 0.0f;
                    ent -= p[j] * lp[j];
                    if (j == act) lpa = lp[j];
                }
                const float ratio = expf(lpa - SLOGP[s]), An = SADV[s];
                const float s1 = ratio * An, s2 = fminf(fmaxf(ratio, a.lo), a.hi) * An;
                const float gmin = -a.invM; // d loss / d min(s1, s2)
                const float g1 = s1 < s2 ? gmin : (s1 == s2 ? 0.5f * gmin : 0.0f);
                const float g2 = s2 < s1 ? gmin : (s1 == s2 ? 0.5f * gmin : 0.0f);
                const bool inside = ratio >= a.lo && ratio <= a.hi;
                const float gr = g1 * An + (inside ? g2 * An : 0.0f);
                const float glpa = gr * ratio, gent = -a.ent * a.invM;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < A) dl[j] = glpa * ((j == act ? 1.0f : 0.0f) - p[j]) + gent * (-p[j] * (lp[j] + ent));
                st_pg += -fminf(s1, s2);
                st_en += ent;
                st_cf += fabsf(ratio - 1.0f) > a.clip ? 1.0f : 0.0f;
                if (kl_on) { // KL(old || new) = sum_j p_old[j] * (logp_old[j] - logp[j]); d/d logit j = p[j]*sum(p_old) - p_old[j]
                    float po[4], spo = 0.0f, kl = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        po[j] = j < A ? expf(SLPO[s * 4 + j]) : 0.0f;
                        if (j < A) {
                            spo += po[j];
                            kl += po[j] * (SLPO[s * 4 + j] - lp[j]);
                        }
                    }
                    const float gk = kl_coef * a.invM;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j < A) dl[j] += gk * (p[j] * spo - po[j]);
                    st_kl += kl;
                }
            }
            if (vf && SIDX[s] >= 0) {
                v += bv[0];
                const float err = v - SRET[s];
                dv = a.vf * 2.0f * err * a.invM;
                float vl = err * err;
                if (vclip_on) { // VL = max((v - ret)^2, (v_old + clamp(v - v_old, -c, c) - ret)^2): max and clamp as autograd takes them
                    const float vo = SVOLD[s], d = v - vo;
                    const float errc = (vo + fminf(fmaxf(d, -vf_clip), vf_clip)) - SRET[s];
                    const float l1 = vl, l2 = errc * errc;
                    const float w1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f), w2 = l2 > l1 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
                    const bool vin = d >= -vf_clip && d <= vf_clip;
                    const float gv = w1 * (2.0f * err) + (vin ? w2 * (2.0f * errc) : 0.0f);
                    dv = a.vf * gv * a.invM;
                    vl = fmaxf(l1, l2);
                }
                st_vl += vl;
            }
            if (pi) {
#pragma unroll
                for (int j = 0; j < 4; ++j) DLOG[s * 4 + j] = dl[j];
            }
            if (vf) DV[s] = dv;
        }
        __syncthreads();
        // 4. the heads' backward: the last hidden layer's delta, and the heads' own gradients (registers, one column per lane)
        for (int i = tid; i < kTile * H; i += kPpoBlock) {
            const int s = i / H, k = i - s * H;
            float d = vf ? DV[s] * WH[4 * H + k] : 0.0f;
            if (pi)
                for (int j = 0; j < A; ++j) d = fmaf(DLOG[s * 4 + j], WH[j * H + k], d);
            DZ[s * SH + k] = d * dactivate(HL[s * SH + k], kind);
        }
        if (tid < H) {
            for (int s = 0; s < kTile; ++s) {
                const float hk = HL[s * SH + tid];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pi) accW[j] = fmaf(DLOG[s * 4 + j], hk, accW[j]);
                if (vf) accWv = fmaf(DV[s], hk, accWv);
            }
        } else if (tid >= 128 && tid <= 128 + A) {
            const int j = tid - 128;
            if (j < A ? pi : vf) accbh += j < A ? tile_sum(DLOG + j, 4) : tile_sum(DV, 1);
        }
        __syncthreads();
        // 5. the second hidden layer: dW1 = dZᵀ·HB0, db1, and the first layer's delta into HB1 (dead by now)
        const float *DZ0 = DZ;
        if (a.L == 2) {
            mm_wgrad(DZ, SH, HB0, SH, NT, NT, H, gW1, first, wave, lane);
            mm_backward(W1, H, DZ, HB0, HB1, SH, kind, wave, lane);
            if (tid >= 128 && tid < 128 + H) (pass == 0 ? accb1 : accb1v) += tile_sum(DZ + tid - 128, SH);
            __syncthreads();
            DZ0 = HB1;
        }
        // 6. the first layer: dW0 = dZ0ᵀ·X, db0
        mm_wgrad(DZ0, SH, X, SX, NT, DT, D, gW0, first, wave, lane);
        if (tid < H) (pass == 0 ? accb0 : accb0v) += tile_sum(DZ0 + tid, SH);
        __syncthreads();
        }
        first = false;
    }
    // the register-held sums into the slot
    float *gb0 = g + H * D, *gb1 = gb0 + H + H * H;
    if (tid < H) {
        gb0[tid] = accb0;
        for (int j = 0; j < A; ++j) gWpi[j * H + tid] = accW[j];
        gWv[tid] = accWv;
        if (SPLIT) gb0[T + A * H + A + tid] = accb0v;
    }
    if (a.L == 2 && tid >= 128 && tid < 128 + H) {
        gb1[tid - 128] = accb1;
        if (SPLIT) gb1[T + A * H + A + tid - 128] = accb1v;
    }
    if (tid >= 128 && tid <= 128 + A) (tid - 128 < A ? gbpi[tid - 128] : gbv[0]) = accbh;
    if (tid < kTile) {
        RED[tid * 4 + 0] = st_pg;
        RED[tid * 4 + 1] = st_vl;
        RED[tid * 4 + 2] = st_en;
        RED[tid * 4 + 3] = st_cf;
        if (EXT) RED5[tid] = st_kl;
    }
    __syncthreads();
    if (tid < 4) {
        float s = 0.0f;
        for (int i = 0; i < kTile; ++i) s += RED[i * 4 + tid];
        g[a.P + tid] = s;
    } else if (EXT && tid == 4) {
        float s = 0.0f;
        for (int i = 0; i < kTile; ++i) s += RED5[i];
        g[a.P + 4] = s;
    } else if (EXT && tid < kExtStats) {
        g[a.P + tid] = 0.0f;
    }
}

template <bool POP, bool SPLIT> __global__ void __launch_bounds__(kPpoBlock) ppo_grad_kernel(const GradArgs a, const PopGradArgs pa)
{
    ppo_grad_body<POP, false, SPLIT, false>(a, pa, ExtGradArgs{}, nullptr);
}

template <bool POP, bool SPLIT>
__global__ void __launch_bounds__(kPpoBlock) ppo_grad_ext_kernel(const GradArgs a, const PopGradArgs pa, const ExtGradArgs ea)
{
    ppo_grad_body<POP, true, SPLIT, false>(a, pa, ea, nullptr);
}

// a population on per-member schedules
template <bool SPLIT>
__global__ void __launch_bounds__(kPpoBlock) ppo_grad_sched_kernel(const GradArgs a, const PopGradArgs pa, const int32_t *__restrict__ sched)
{
    ppo_grad_body<true, false, SPLIT, true>(a, pa, ExtGradArgs{}, sched);
}

template <bool SPLIT>
__global__ void __launch_bounds__(kPpoBlock) ppo_grad_ext_sched_kernel(const GradArgs a, const PopGradArgs pa, const ExtGradArgs ea,
                                                                       const int32_t *__restrict__ sched)
{
    ppo_grad_body<true, true, SPLIT, true>(a, pa, ea, sched);
}

// ... on unequal slices
template <bool SPLIT>
__global__ void __launch_bounds__(kPpoBlock) ppo_grad_sliced_kernel(const GradArgs a, const PopGradArgs pa, const int32_t *__restrict__ sched,
                                                                    const SliceGradArgs sa)
{
    ppo_grad_body<true, false, SPLIT, true, true>(a, pa, ExtGradArgs{}, sched, sa);
}

template <bool SPLIT>
__global__ void __launch_bounds__(kPpoBlock) ppo_grad_ext_sliced_kernel(const GradArgs a, const PopGradArgs pa, const ExtGradArgs ea,
                                                                        const int32_t *__restrict__ sched, const SliceGradArgs sa)
{
    ppo_grad_body<true, true, SPLIT, true, true>(a, pa, ea, sched, sa);
}

// grad[p] = sum over the slots (a fixed order); entries P..P+3 (when nstats) are the loss sums -> stats = sum / M.  With params: Adam, torch's
// foreach formula: m = lerp(m, g, 1-b1); v = v*b2 + (1-b2)*g*g; p += step_size * m / (sqrt(v) / sqrt(bc2) + eps), step_size = -lr/bc1.
// torch's lerp (ATen/native/Lerp.h) has two branches: m + w*(g - m) for |w| < 0.5, g - (g - m)*(1 - w) otherwise (b1 <= 0.5), with
// 1 - w formed in f32; with b1 = 0 the second gives m = g exactly.
struct AdamArgs {
    float w1, one_minus_w1, beta2, w2, bc2_sqrt, eps, step_size;
};

// the sum of entry p over the G slots in order, 64 at a time as a tree of 4 trees of 16 (the missing ones are zeros)
__device__ __forceinline__ float slot_sum(const float *__restrict__ slots, int G, int stride, int p)
{
    float s = 0.0f;
#pragma unroll 1
    for (int b0 = 0; b0 < G; b0 += 64) {
        float u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float w[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int gi = b0 + i * 16 + j;
                w[j] = gi < G ? slots[(size_t)gi * stride + p] : 0.0f;
            }
            u[i] = tree_sum<16>(w);
        }
        s += tree_sum<4>(u);
    }
    return s;
}

// one Adam step of entry p with gradient s
__device__ __forceinline__ void adam_apply(const AdamArgs &ad, float s, int p, int P, float *__restrict__ params, float *__restrict__ mv)
{
    float m = mv[p], v = mv[P + p];
    m = fabsf(ad.w1) < 0.5f ? m + ad.w1 * (s - m) : s - (s - m) * ad.one_minus_w1;
    v = v * ad.beta2;
    v = v + ad.w2 * (s * s);
    mv[p] = m;
    mv[P + p] = v;
    const float den = sqrtf(v) / ad.bc2_sqrt + ad.eps;
    params[p] = params[p] + ad.step_size * (m / den);
}

// AdamArgs as kPopTableRow floats of the population's table (pop_pack writes a row per member and step, the kernels read theirs)
inline void adam_to_row(const AdamArgs &ad, float *row)
{
    row[0] = ad.w1;
    row[1] = ad.one_minus_w1;
    row[2] = ad.beta2;
    row[3] = ad.w2;
    row[4] = ad.bc2_sqrt;
    row[5] = ad.eps;
    row[6] = ad.step_size;
    row[7] = 0.0f;
}

__device__ __forceinline__ AdamArgs adam_from_row(const float *__restrict__ row)
{
    AdamArgs ad;
    ad.w1 = row[0];
    ad.one_minus_w1 = row[1];
    ad.beta2 = row[2];
    ad.w2 = row[3];
    ad.bc2_sqrt = row[4];
    ad.eps = row[5];
    ad.step_size = row[6];
    return ad;
}

// A population's launch, member m = blockIdx.y: its Adam constants of this step (row m of the step's table rows), its run of `run`
// floats of vec (the slots, or the clip sequence's gradient vector), its stats row, parameter row and moment rows.
__device__ __forceinline__ void member_rows(size_t m, int P, size_t run, long long stats_stride, const float *__restrict__ adam, AdamArgs &ad,
                                            const float *__restrict__ &vec, float *__restrict__ &stats_out, float *__restrict__ &params,
                                            float *__restrict__ &mv)
{
    ad = adam_from_row(adam + m * kPopTableRow);
    vec += m * run;
    if (stats_out) stats_out += m * (size_t)stats_stride;
    if (params) params += m * (size_t)P;
    if (mv) mv += m * 2 * (size_t)P;
}

// What the extended update adds to the reduction (stride = P + kExtStats).  The stats row is f32 [kExtStats]: the five loss means,
// [5] the global gradient norm before clipping (0 here; ppo_clip_kernel writes it), [6] the KL coefficient in use, [7] 0.  The
// member's mean(KL) of this minibatch is also added to klacc[m] (set, on an epoch's first chunk): a running f32 sum in chunk
// order, which the adaptation kernel turns into the epoch's mean after the last minibatch.
struct ExtReduceArgs {
    const float *kl_coef; // f32 [members], nullable
    float *klacc;         // f32 [members]
    int first_chunk;      // this minibatch is the first of its epoch
    float *gvec;          // non-NULL = the clip sequence: f32 [members][P] receives the gradient and part the sums of squares, no Adam
    double *part;         // f64 [members][gridDim.x]
};

// POP = false: one policy's launch (stats_stride, adam unused).  POP = true: reduce + Adam of every member in one launch, grid
// (ceil(stride / 256), members): member m = blockIdx.y sums its own G slots, writes its stats row (stats_out + m*stats_stride,
// nullable) and steps parameter row m / moments row m with ITS Adam constants of this step (adam row m: the host's doubles, rounded
// as adam_args rounds them).
// EXT = false: stats rows of 4 loss means (stride = P + 4, or P for ssg_ppo_adam's G = 1), ea and sq unused.  EXT = true: see
// ExtReduceArgs; sq is the workgroup's 256 doubles of LDS.
// SCHED (with POP; sched = this launch's schedule records, else unused): the member's run of slots is the launch's (G of them), of
// which it sums ITS first G_m = ppo_grid(M_m) and divides by its own (float)M_m; first_chunk is its record's.  A member without a
// minibatch in this launch does nothing at all: no Adam step, no stats row, no klacc, gvec or part write.
template <bool POP, bool EXT, bool SCHED>
__device__ __forceinline__ void ppo_reduce_body(const float *__restrict__ slots, int G, int P, int stride, float fM, float *__restrict__ grad_out,
                                                float *__restrict__ stats_out, float *__restrict__ params, float *__restrict__ mv,
                                                const AdamArgs &ad_, long long stats_stride, const float *__restrict__ adam,
                                                const ExtReduceArgs &ea, double *sq, const int32_t *__restrict__ sched)
{
    static_assert(POP || !SCHED, "a schedule is a population's");
    AdamArgs ad = ad_;
    const size_t m = POP ? blockIdx.y : 0;
    int Gm = G, first_chunk = EXT ? ea.first_chunk : 0;
    if (SCHED) {
        const int32_t *rec = sched + m * kPopSchedRow;
        if (!rec[SR_ACTIVE]) return; // (the whole workgroup: ahead of the barriers below)
        Gm = rec[SR_G] < G ? rec[SR_G] : G;
        fM = (float)rec[SR_M];
        first_chunk = rec[SR_FIRST];
    }
    if (POP) member_rows(m, P, (size_t)G * (size_t)stride, stats_stride, adam, ad, slots, stats_out, params, mv);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (!EXT && p >= stride) return; // (EXT: every lane stays for the barriers of the sum of squares)
    const float s = p < stride ? slot_sum(slots, Gm, stride, p) : 0.0f;
    if (p >= P && p < stride) {
        const int q = p - P;
        const float mean = s / fM;
        if (!EXT) {
            if (stats_out) stats_out[q] = mean;
        } else {
            const float klc = ea.kl_coef ? ea.kl_coef[m] : 0.0f;
            if (stats_out) stats_out[q] = q < 5 ? mean : (q == 6 ? (klc > 0.0f ? klc : 0.0f) : 0.0f);
            if (q == 4) ea.klacc[m] = first_chunk ? mean : ea.klacc[m] + mean;
        }
    }
    if (p < P) {
        if (grad_out) grad_out[p] = s;
        if (EXT && ea.gvec) ea.gvec[m * (size_t)P + p] = s;
        else if (params) adam_apply(ad, s, p, P, params, mv);
    }
    if (EXT && ea.gvec) { // the workgroup's sum of squares, f64, a fixed tree
        sq[threadIdx.x] = p < P ? (double)s * (double)s : 0.0;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sq[threadIdx.x] += sq[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) ea.part[m * (size_t)gridDim.x + blockIdx.x] = sq[0];
    }
}

template <bool POP>
__global__ void __launch_bounds__(256) ppo_reduce_kernel(const float *__restrict__ slots, int G, int P, int stride, float fM,
                                                         float *__restrict__ grad_out, float *__restrict__ stats_out,
                                                         float *__restrict__ params, float *__restrict__ mv, const AdamArgs ad,
                                                         long long stats_stride, const float *__restrict__ adam)
{
    ppo_reduce_body<POP, false, false>(slots, G, P, stride, fM, grad_out, stats_out, params, mv, ad, stats_stride, adam, ExtReduceArgs{},
                                       nullptr, nullptr);
}

template <bool POP>
__global__ void __launch_bounds__(256) ppo_reduce_ext_kernel(const float *__restrict__ slots, int G, int P, int stride, float fM,
                                                             float *__restrict__ grad_out, float *__restrict__ stats_out,
                                                             float *__restrict__ params, float *__restrict__ mv, const AdamArgs ad,
                                                             long long stats_stride, const float *__restrict__ adam,
                                                             const ExtReduceArgs ea)
{
    __shared__ double sq[256];
    ppo_reduce_body<POP, true, false>(slots, G, P, stride, fM, grad_out, stats_out, params, mv, ad, stats_stride, adam, ea, sq, nullptr);
}

// a population on per-member schedules (no fM: every member divides by its record's M)
__global__ void __launch_bounds__(256) ppo_reduce_sched_kernel(const float *__restrict__ slots, int G, int P, int stride,
                                                               float *__restrict__ stats_out, float *__restrict__ params,
                                                               float *__restrict__ mv, long long stats_stride,
                                                               const float *__restrict__ adam, const int32_t *__restrict__ sched)
{
    ppo_reduce_body<true, false, true>(slots, G, P, stride, 0.0f, nullptr, stats_out, params, mv, AdamArgs{}, stats_stride, adam,
                                       ExtReduceArgs{}, nullptr, sched);
}

__global__ void __launch_bounds__(256) ppo_reduce_ext_sched_kernel(const float *__restrict__ slots, int G, int P, int stride,
                                                                   float *__restrict__ stats_out, float *__restrict__ params,
                                                                   float *__restrict__ mv, long long stats_stride,
                                                                   const float *__restrict__ adam, const ExtReduceArgs ea,
                                                                   const int32_t *__restrict__ sched)
{
    __shared__ double sq[256];
    ppo_reduce_body<true, true, true>(slots, G, P, stride, 0.0f, nullptr, stats_out, params, mv, AdamArgs{}, stats_stride, adam, ea, sq, sched);
}

// The third launch of the clip sequence, grid (ceil(P / 256), members): every workgroup adds the member's nb partial sums of squares
// in index order (f64), then in f32 norm = (float)sqrt(sum), coef = min(1, max_grad_norm / (norm + 1e-6f)) — torch's
// clip_grad_norm_ — and Adam on g * coef.  A member with max_grad_norm <= 0 gets coef = 1.0f (exact) and a norm column of 0.
// params NULL (ssg_ppo_grad_ext): the norm column alone.  SCHED: a member without a minibatch in this launch (its record) is skipped.
template <bool POP, bool SCHED>
__device__ __forceinline__ void ppo_clip_body(const float *__restrict__ gvec, const double *__restrict__ part, int nb, int P,
                                              float max_grad_norm, const float *__restrict__ pop_ext, float *__restrict__ stats_out,
                                              long long stats_stride, float *__restrict__ params, float *__restrict__ mv,
                                              const AdamArgs &ad_, const float *__restrict__ adam, const int32_t *__restrict__ sched)
{
    static_assert(POP || !SCHED, "a schedule is a population's");
    AdamArgs ad = ad_;
    const size_t m = POP ? blockIdx.y : 0;
    if (SCHED && !sched[m * kPopSchedRow + SR_ACTIVE]) return;
    if (POP) {
        member_rows(m, P, (size_t)P, stats_stride, adam, ad, gvec, stats_out, params, mv);
        max_grad_norm = pop_ext[m * kPopExtRow + 1];
    }
    double sum = 0.0;
    for (int b = 0; b < nb; ++b) sum += part[m * (size_t)nb + b];
    const float norm = (float)sqrt(sum);
    const bool on = max_grad_norm > 0.0f;
    const float coef = on ? fminf(1.0f, max_grad_norm / (norm + 1e-6f)) : 1.0f;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && stats_out) stats_out[5] = on ? norm : 0.0f;
    if (p < P && params) adam_apply(ad, gvec[p] * coef, p, P, params, mv);
}

template <bool POP>
__global__ void __launch_bounds__(256) ppo_clip_kernel(const float *__restrict__ gvec, const double *__restrict__ part, int nb, int P,
                                                       float max_grad_norm, const float *__restrict__ pop_ext,
                                                       float *__restrict__ stats_out, long long stats_stride, float *__restrict__ params,
                                                       float *__restrict__ mv, const AdamArgs ad, const float *__restrict__ adam)
{
    ppo_clip_body<POP, false>(gvec, part, nb, P, max_grad_norm, pop_ext, stats_out, stats_stride, params, mv, ad, adam, nullptr);
}

__global__ void __launch_bounds__(256) ppo_clip_sched_kernel(const float *__restrict__ gvec, const double *__restrict__ part, int nb, int P,
                                                             const float *__restrict__ pop_ext, float *__restrict__ stats_out,
                                                             long long stats_stride, float *__restrict__ params, float *__restrict__ mv,
                                                             const float *__restrict__ adam, const int32_t *__restrict__ sched)
{
    ppo_clip_body<true, true>(gvec, part, nb, P, 0.0f, pop_ext, stats_out, stats_stride, params, mv, AdamArgs{}, adam, sched);
}

// The last launch of an extended update with a KL target, one workgroup, lane m = member m: RLlib's update_kl on the f32 mean of the
// last epoch's minibatch means of KL.  A member whose target is <= 0 keeps its coefficient.  sched_hdr (nullable): the schedule table's
// header rows — member m's last epoch had ITS chunks_m minibatches (and klacc[m] is that epoch's sum: an idle member never touches it).
__global__ void __launch_bounds__(256) ppo_kl_adapt_kernel(int members, float *__restrict__ kl_coef, const float *__restrict__ klacc,
                                                           float chunks, float kl_target, const float *__restrict__ pop_ext,
                                                           const int32_t *__restrict__ sched_hdr)
{
    const int m = threadIdx.x;
    if (m >= members) return;
    if (sched_hdr) chunks = (float)sched_hdr[(size_t)m * kPopSchedRow + SH_CHUNKS];
    const float target = pop_ext ? pop_ext[(size_t)m * kPopExtRow + 2] : kl_target;
    if (!(target > 0.0f)) return;
    const float mean = klacc[m] / chunks;
    if (mean > 2.0f * target) kl_coef[m] = kl_coef[m] * 1.5f;
    else if (mean < 0.5f * target) kl_coef[m] = kl_coef[m] * 0.5f;
}

// ------------------------------------------------------------------------------------------------------------------------------
// the PBT exploit copy and the per-member episode statistics
// ------------------------------------------------------------------------------------------------------------------------------
struct PopSrc {
    uint8_t src[SSG_POP_MAX_MEMBERS]; // by value in the kernel arguments: the caller's host array is free when the call returns
};

// grid (ceil(3L / 256), members): member m with src[m] != m takes the parameter row and both moment rows of src[m].  The host
// refused a source that is itself a destination, so no row is read and written in one launch.
__global__ void __launch_bounds__(256) pop_exploit_kernel(const PopSrc s, int L, float *__restrict__ params, float *__restrict__ mv)
{
    const int m = blockIdx.y, from = s.src[m];
    if (from == m) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < L) params[(size_t)m * L + i] = params[(size_t)from * L + i];
    else if (i < 3 * L) mv[(size_t)m * 2 * L + (i - L)] = mv[(size_t)from * 2 * L + (i - L)];
}

// grid (ceil(n / 256), members): one lane per env walks t = 0 .. K-1 with the env's carried return / length; an episode is counted at
// its done step as the step kernel counts it (llrint(100 * cum): cum is a sum of {1, -1, -0.01} terms).  Integer sums per workgroup,
// then three integer atomics per workgroup on the member's triple: order-free and exact.
// (the body of both kernels: the member's n envs start at env e0; red: the workgroup's 3 x 256 integers of LDS)
__device__ __forceinline__ void episode_stats_body(int K, int N, int n, size_t e0, const double *__restrict__ rew,
                                                   const uint8_t *__restrict__ done, double *__restrict__ carry_ret,
                                                   int32_t *__restrict__ carry_len, unsigned long long *__restrict__ out, long long (*red)[256])
{
    const int el = blockIdx.x * 256 + threadIdx.x;
    long long s_ret = 0, s_len = 0, s_eps = 0;
    if (el < n) {
        const size_t e = e0 + (size_t)el;
        double cum = carry_ret[e];
        int len = carry_len[e];
        for (int t = 0; t < K; ++t) {
            const size_t i = (size_t)t * N + e;
            cum += rew[i];
            len += 1;
            if (done[i]) {
                s_ret += (long long)llrint(cum * 100.0);
                s_len += len;
                s_eps += 1;
                cum = 0.0;
                len = 0;
            }
        }
        carry_ret[e] = cum;
        carry_len[e] = len;
    }
    red[0][threadIdx.x] = s_ret;
    red[1][threadIdx.x] = s_len;
    red[2][threadIdx.x] = s_eps;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < 3 && red[2][0] != 0) atomicAdd(out + (size_t)blockIdx.y * 3 + threadIdx.x, (unsigned long long)red[threadIdx.x][0]);
}

__global__ void __launch_bounds__(256) pop_episode_stats_kernel(int K, int N, int n, const double *__restrict__ rew,
                                                                const uint8_t *__restrict__ done, double *__restrict__ carry_ret,
                                                                int32_t *__restrict__ carry_len, unsigned long long *__restrict__ out)
{
    __shared__ long long red[3][256];
    episode_stats_body(K, N, n, (size_t)blockIdx.y * (size_t)n, rew, done, carry_ret, carry_len, out, red);
}

// on unequal slices: grid (blocks of the largest slice, members); member m's envs are its row of the slices table
__global__ void __launch_bounds__(256) pop_episode_stats_sliced_kernel(int K, int N, const int32_t *__restrict__ slices,
                                                                       const double *__restrict__ rew, const uint8_t *__restrict__ done,
                                                                       double *__restrict__ carry_ret, int32_t *__restrict__ carry_len,
                                                                       unsigned long long *__restrict__ out)
{
    __shared__ long long red[3][256];
    const int32_t *row = slices + (size_t)blockIdx.y * SSG_POP_SLICE_ROW;
    if ((int)(blockIdx.x * 256) >= row[1]) return; // (uniform over the workgroup, ahead of the barriers)
    episode_stats_body(K, N, row[1], (size_t)row[0], rew, done, carry_ret, carry_len, out, red);
}

// One policy's row of loss / GAE constants (PT_*), f32 from the caller's doubles: torch rounds a Python scalar to f32 when it meets
// an f32 tensor; 1 - clip, 1 + clip and gamma * lam are formed in double first.  The one place these roundings are written: a
// population's table rows (pop_pack) and one policy's kernel arguments (launch_ppo_minibatch) both come from here.
void loss_row(const ssg_ppo_hparams &hp, float *row)
{
    row[PT_LO] = (float)(1.0 - hp.clip);
    row[PT_HI] = (float)(1.0 + hp.clip);
    row[PT_CLIP] = (float)hp.clip;
    row[PT_VF] = (float)hp.vf_coef;
    row[PT_ENT] = (float)hp.ent_coef;
    row[PT_ADV_EPS] = (float)hp.adv_eps;
    row[PT_GF] = (float)hp.gamma;
    row[PT_GLF] = (float)(hp.gamma * hp.lam);
}

AdamArgs adam_args(const ssg_ppo_hparams &hp, int64_t step)
{
    const double bc1 = 1.0 - std::pow(hp.beta1, (double)step), bc2 = 1.0 - std::pow(hp.beta2, (double)step);
    AdamArgs ad;
    ad.w1 = (float)(1.0 - hp.beta1);
    ad.one_minus_w1 = 1.0f - ad.w1;
    ad.beta2 = (float)hp.beta2;
    ad.w2 = (float)(1.0 - hp.beta2);
    ad.bc2_sqrt = (float)std::sqrt(bc2);
    ad.eps = (float)hp.eps;
    ad.step_size = (float)(-(hp.lr / bc1));
    return ad;
}

} // namespace

int ppo_packed_len(const ssg_policy &p)
{
    const int D = p.obs_dim, H = p.hidden, A = p.n_actions;
    const int tower = H * D + H + (p.n_hidden_layers - 1) * (H * H + H);
    return ((p.activation & SSG_POLICY_SEPARATE_VALUE) ? 2 : 1) * tower + A * H + A + H + 1;
}

int ppo_grid(long long M)
{
    const long long t = (M + kTile - 1) / kTile;
    return (int)(t < kPpoMaxGrid ? t : kPpoMaxGrid);
}

size_t ppo_grad_lds_bytes(const ssg_policy &p)
{
    const size_t D = (size_t)p.obs_dim, H = (size_t)p.hidden;
    const size_t SX = (D + 15) / 16 * 16 + 1, SH = H + 1;
    const size_t floats = kTile * SX + kTile * SH * (size_t)(p.n_hidden_layers + 1) + 5 * H + kTile * 4 + kTile + 4 * kTile + kTile * 4;
    return floats * sizeof(float) + kTile * sizeof(int) + kTile * sizeof(long long) + 8;
}

// (the extended instantiations add v_old, four logp_old and the fifth loss sum per sample of the tile: 1.5 KB)
size_t ppo_grad_ext_lds_bytes(const ssg_policy &p) { return ppo_grad_lds_bytes(p) + 6 * kTile * sizeof(float); }

// The gradient kernel's instantiations: for a population or not (and then on per-member schedules, and on unequal slices, or not), the
// extended loss or not, separate towers or not.  prepare_ppo walks the tables, launch_ppo_minibatch indexes them.  Every table lists the
// instantiations with their flags ON first, so it is indexed [!split] (and then [!pop]): an instantiation's place in the object's .text
// follows its first mention, and these orders, of the tables and inside them, keep the object's device code byte for byte.
static decltype(&ppo_grad_kernel<false, false>) const kGrad[2][2] = {{ppo_grad_kernel<true, true>, ppo_grad_kernel<false, true>},
                                                                    {ppo_grad_kernel<true, false>, ppo_grad_kernel<false, false>}};
static decltype(&ppo_grad_ext_kernel<false, false>) const kGradExt[2][2] = {{ppo_grad_ext_kernel<true, true>, ppo_grad_ext_kernel<false, true>},
                                                                            {ppo_grad_ext_kernel<true, false>, ppo_grad_ext_kernel<false, false>}};
static decltype(&ppo_grad_sched_kernel<false>) const kGradSched[2] = {ppo_grad_sched_kernel<true>, ppo_grad_sched_kernel<false>};
static decltype(&ppo_grad_ext_sched_kernel<false>) const kGradExtSched[2] = {ppo_grad_ext_sched_kernel<true>, ppo_grad_ext_sched_kernel<false>};
static decltype(&ppo_grad_ext_sliced_kernel<false>) const kGradExtSliced[2] = {ppo_grad_ext_sliced_kernel<true>, ppo_grad_ext_sliced_kernel<false>};
static decltype(&ppo_grad_sliced_kernel<false>) const kGradSliced[2] = {ppo_grad_sliced_kernel<true>, ppo_grad_sliced_kernel<false>};

// (the dynamic-LDS limit of the gradient kernels: up to 151 KB at obs_dim 176, hidden 128, 2 layers)
template <typename Kernel> static hipError_t raise_lds_limit(const Kernel *k, int count)
{
    for (int i = 0; i < count; ++i) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k[i]), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t prepare_ppo()
{
    hipError_t e = raise_lds_limit(&kGrad[0][0], 4);
    if (e == hipSuccess) e = raise_lds_limit(&kGradExt[0][0], 4);
    if (e == hipSuccess) e = raise_lds_limit(kGradSched, 2);
    if (e == hipSuccess) e = raise_lds_limit(kGradExtSched, 2);
    if (e == hipSuccess) e = raise_lds_limit(kGradExtSliced, 2);
    if (e == hipSuccess) e = raise_lds_limit(kGradSliced, 2);
    return e;
}

hipError_t launch_ppo_gae(const ssg_ppo_hparams &hp, int K, int N, const double *rew, const uint8_t *done, const float *val,
                          const float *last_val, float *adv, float *ret, void *ws, hipStream_t stream, const float *boot)
{
    const int nb = ppo_gae_blocks(N);
    float *stats = reinterpret_cast<float *>(static_cast<char *>(ws) + kPpoStatsOff);
    double2 *part = reinterpret_cast<double2 *>(static_cast<char *>(ws) + kPpoSlotsOff);
    float row[kPopTableRow];
    loss_row(hp, row);
    if (boot)
        hipLaunchKernelGGL(ppo_gae_boot_kernel, dim3(nb), dim3(256), 0, stream, K, N, rew, done, val, last_val, adv, ret, row[PT_GF],
                           row[PT_GLF], part, boot);
    else
        hipLaunchKernelGGL(ppo_gae_kernel, dim3(nb), dim3(256), 0, stream, K, N, rew, done, val, last_val, adv, ret, row[PT_GF], row[PT_GLF],
                           part);
    hipLaunchKernelGGL(ppo_gae_stats_kernel, dim3(1), dim3(256), 0, stream, (const double2 *)part, nb, (double)K * (double)N,
                       row[PT_ADV_EPS], stats);
    return hipGetLastError();
}

hipError_t launch_ppo_minibatch(const PpoMinibatch &mb, hipStream_t stream)
{
    const ssg_policy &p = *mb.policy;
    const bool pop = mb.table != nullptr; // a population reads its constants from the table: the POP instantiations
    const bool sched = mb.sched != nullptr; // ... and its members' minibatches from the schedule records: the SCHED ones (G: the launch's)
    if (sched && !pop) return hipErrorInvalidValue;
    const bool sliced = mb.lay.slices != nullptr; // ... on unequal slices: the SLICED ones
    if (sliced && !(sched && mb.sched_hdr)) return hipErrorInvalidValue;
    const SliceGradArgs sa = {mb.lay.slices, mb.sched_hdr, mb.K, mb.perm_epochs};
    const bool split = (p.activation & SSG_POLICY_SEPARATE_VALUE) != 0;
    const PpoExtLaunch *ext = mb.ext;
    const int P = ppo_packed_len(p), G = ppo_grid(mb.M), stride = P + (ext ? kExtStats : 4);
    char *base = static_cast<char *>(mb.ws);
    const PpoExtLayout lay = ext ? ppo_ext_layout(mb.slots_off, mb.lay.members, G, P) : PpoExtLayout{};
    float row[kPopTableRow] = {}; // (a population's gradient kernel reads row m of the table instead)
    if (!pop) loss_row(*mb.hp, row);
    GradArgs a;
    a.D = p.obs_dim;
    a.H = p.hidden;
    a.L = p.n_hidden_layers;
    a.A = p.n_actions;
    a.kind = p.activation & 0xff;
    a.params = p.dev_params;
    a.x = mb.batch.x;
    a.act = mb.batch.act;
    a.logp = mb.batch.logp;
    a.adv = mb.batch.adv;
    a.ret = mb.batch.ret;
    a.idx = mb.idx;
    a.M = mb.M;
    a.n_samples = mb.n_samples;
    a.stats = reinterpret_cast<const float *>(base + kPpoStatsOff);
    if (mb.adv_stats && !mb.adv_part) a.stats = mb.adv_stats; // a finished row of the job's table (ssg_ppo_set_adv_table)
    if (mb.adv_part) { // per-minibatch normalisation: this minibatch's own statistics first (two launches), into the scratch's rows
        if (!mb.adv_stats) return hipErrorInvalidValue;
        AdvNormLaunch an = {};
        an.adv = mb.batch.adv;
        an.idx = mb.idx;
        an.M = mb.M;
        an.n_samples = mb.n_samples;
        an.lay = mb.lay;
        an.N = mb.N;
        an.idx_stride = mb.idx_stride;
        an.table = mb.table;
        an.adv_eps_col = PT_ADV_EPS;
        an.adv_eps = row[PT_ADV_EPS];
        an.sched = mb.sched;
        an.sched_hdr = mb.sched_hdr;
        an.K = mb.K;
        an.perm_epochs = mb.perm_epochs;
        an.stats = mb.adv_stats;
        an.part = mb.adv_part;
        const hipError_t e = launch_adv_norm(an, stream);
        if (e != hipSuccess) return e;
        a.stats = mb.adv_stats;
    }
    a.slots =reinterpret_cast<float *>(base + (ext ? lay.slots : mb.slots_off));
    a.P = P;
    a.lo = row[PT_LO];
    a.hi = row[PT_HI];
    a.clip = row[PT_CLIP];
    a.vf = row[PT_VF];
    a.ent = row[PT_ENT];
    a.invM = 1.0f / (float)mb.M;
    PopGradArgs pa;
    pa.n = mb.lay.n;
    pa.N = mb.N;
    pa.idx_stride = mb.idx_stride;
    pa.table = mb.table;
    float *params = mb.adam_mv ? const_cast<float *>(p.dev_params) : nullptr;
    const AdamArgs ad = mb.adam_mv && !pop ? adam_args(*mb.hp, mb.step) : AdamArgs{};
    const dim3 ggrid((unsigned)G, (unsigned)mb.lay.members), rgrid((unsigned)((stride + 255) / 256), (unsigned)mb.lay.members);
    if (!ext) {
        if (sliced) hipLaunchKernelGGL(kGradSliced[!split], ggrid, dim3(kPpoBlock), ppo_grad_lds_bytes(p), stream, a, pa, mb.sched, sa);
        else if (sched) hipLaunchKernelGGL(kGradSched[!split], ggrid, dim3(kPpoBlock), ppo_grad_lds_bytes(p), stream, a, pa, mb.sched);
        else hipLaunchKernelGGL(kGrad[!split][!pop], ggrid, dim3(kPpoBlock), ppo_grad_lds_bytes(p), stream, a, pa);
        if (sched)
            hipLaunchKernelGGL(ppo_reduce_sched_kernel, rgrid, dim3(256), 0, stream, (const float *)a.slots, G, P, stride, mb.stats_out, params,
                               mb.adam_mv, mb.stats_stride, mb.adam_row, mb.sched);
        else
            hipLaunchKernelGGL(pop ? ppo_reduce_kernel<true> : ppo_reduce_kernel<false>, rgrid, dim3(256), 0, stream, (const float *)a.slots, G,
                               P, stride, (float)mb.M, mb.grad_out, mb.stats_out, params, mb.adam_mv, ad, mb.stats_stride, mb.adam_row);
        return hipGetLastError();
    }
    ExtGradArgs ea;
    ea.logp_all = ext->logp_all;
    ea.v_old = ext->value_old;
    ea.kl_coef = ext->kl_coef;
    ea.pop_ext = ext->pop_ext;
    ea.vf_clip = ext->vf_clip;
    if (sliced) hipLaunchKernelGGL(kGradExtSliced[!split], ggrid, dim3(kPpoBlock), ppo_grad_ext_lds_bytes(p), stream, a, pa, ea, mb.sched, sa);
    else if (sched) hipLaunchKernelGGL(kGradExtSched[!split], ggrid, dim3(kPpoBlock), ppo_grad_ext_lds_bytes(p), stream, a, pa, ea, mb.sched);
    else hipLaunchKernelGGL(kGradExt[!split][!pop], ggrid, dim3(kPpoBlock), ppo_grad_ext_lds_bytes(p), stream, a, pa, ea);
    ExtReduceArgs er;
    er.kl_coef = ext->kl_coef;
    er.klacc = reinterpret_cast<float *>(base + lay.klacc);
    er.first_chunk = ext->first_chunk ? 1 : 0;
    er.gvec = ext->clip_seq ? reinterpret_cast<float *>(base + lay.gvec) : nullptr;
    er.part = reinterpret_cast<double *>(base + lay.part);
    const dim3 cgrid((unsigned)((P + 255) / 256), (unsigned)mb.lay.members);
    if (sched) {
        hipLaunchKernelGGL(ppo_reduce_ext_sched_kernel, rgrid, dim3(256), 0, stream, (const float *)a.slots, G, P, stride, mb.stats_out, params,
                           mb.adam_mv, mb.stats_stride, mb.adam_row, er, mb.sched);
        if (ext->clip_seq)
            hipLaunchKernelGGL(ppo_clip_sched_kernel, cgrid, dim3(256), 0, stream, (const float *)er.gvec, (const double *)er.part, lay.nb, P,
                               ext->pop_ext, mb.stats_out, mb.stats_stride, params, mb.adam_mv, mb.adam_row, mb.sched);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(pop ? ppo_reduce_ext_kernel<true> : ppo_reduce_ext_kernel<false>, rgrid, dim3(256), 0, stream, (const float *)a.slots,
                       G, P, stride, (float)mb.M, mb.grad_out, mb.stats_out, params, mb.adam_mv, ad, mb.stats_stride, mb.adam_row, er);
    if (ext->clip_seq)
        hipLaunchKernelGGL(pop ? ppo_clip_kernel<true> : ppo_clip_kernel<false>, cgrid,
                           dim3(256), 0, stream, (const float *)er.gvec, (const double *)er.part, lay.nb, P, ext->max_grad_norm, ext->pop_ext,
                           mb.stats_out, mb.stats_stride, params, mb.adam_mv, ad, mb.adam_row);
    return hipGetLastError();
}

hipError_t launch_kl_adapt(int members, const PpoExtLaunch &ext, float kl_target, int P, long long chunks, const int32_t *sched_hdr, void *ws,
                           size_t slots_off, hipStream_t stream)
{
    const PpoExtLayout lay = ppo_ext_layout(slots_off, members, 1, P);
    hipLaunchKernelGGL(ppo_kl_adapt_kernel, dim3(1), dim3(256), 0, stream, members, ext.kl_coef,
                       (const float *)(static_cast<char *>(ws) + lay.klacc), (float)chunks, kl_target, ext.pop_ext, sched_hdr);
    return hipGetLastError();
}

hipError_t launch_ppo_adam(const ssg_policy &p, const ssg_ppo_hparams &hp, const float *grad, float *adam_mv, int64_t step,
                           hipStream_t stream)
{
    const int P = ppo_packed_len(p);
    hipLaunchKernelGGL(ppo_reduce_kernel<false>, dim3((P + 255) / 256), dim3(256), 0, stream, grad, 1, P, P, 1.0f, (float *)nullptr,
                       (float *)nullptr, const_cast<float *>(p.dev_params), adam_mv, adam_args(hp, step), 0ll, (const float *)nullptr);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------------
// the population launchers
// ------------------------------------------------------------------------------------------------------------------------------
void pop_pack(int members, const ssg_ppo_hparams *hp, int64_t step0, int n_steps, float *out)
{
    for (int m = 0; m < members; ++m) loss_row(hp[m], out + (size_t)m * kPopTableRow);
    for (int j = 0; j < n_steps; ++j)
        for (int m = 0; m < members; ++m) adam_to_row(adam_args(hp[m], step0 + 1 + j), out + ((size_t)(1 + j) * members + m) * kPopTableRow);
}

// the same table for members that have taken different numbers of Adam steps: row (j, m) is Adam step step0[m] + 1 + j of member m
void pop_pack_steps(int members, const ssg_ppo_hparams *hp, const int64_t *step0, int n_steps, float *out)
{
    for (int m = 0; m < members; ++m) loss_row(hp[m], out + (size_t)m * kPopTableRow);
    for (int j = 0; j < n_steps; ++j)
        for (int m = 0; m < members; ++m) adam_to_row(adam_args(hp[m], step0[m] + 1 + j), out + ((size_t)(1 + j) * members + m) * kPopTableRow);
}

hipError_t launch_pop_gae(const MemberLayout &lay, int K, int N, const float *table, const double *rew, const uint8_t *done, const float *val,
                          const float *last_val, const float *boot, float *adv, float *ret, void *ws, hipStream_t stream)
{
    const int members = lay.members, n = lay.n, nb = ppo_gae_blocks(n);
    const int32_t *slices = lay.slices;
    float *stats = reinterpret_cast<float *>(static_cast<char *>(ws) + kPpoStatsOff);
    double2 *part = reinterpret_cast<double2 *>(static_cast<char *>(ws) + kPopSlotsOff);
    if (slices) {
        if (boot)
            hipLaunchKernelGGL(pop_gae_boot_sliced_kernel, dim3(nb, members), dim3(256), 0, stream, K, N, slices, nb, rew, done, val, last_val,
                               adv, ret, table, part, boot);
        else
            hipLaunchKernelGGL(pop_gae_sliced_kernel, dim3(nb, members), dim3(256), 0, stream, K, N, slices, nb, rew, done, val, last_val, adv,
                               ret, table, part);
        hipLaunchKernelGGL(pop_gae_stats_sliced_kernel, dim3(members), dim3(256), 0, stream, (const double2 *)part, nb, K, slices, table, stats);
        return hipGetLastError();
    }
    if (boot)
        hipLaunchKernelGGL(pop_gae_boot_kernel, dim3(nb, members), dim3(256), 0, stream, K, N, n, nb, rew, done, val, last_val, adv, ret, table,
                           part, boot);
    else
        hipLaunchKernelGGL(pop_gae_kernel, dim3(nb, members), dim3(256), 0, stream, K, N, n, nb, rew, done, val, last_val, adv, ret, table, part);
    hipLaunchKernelGGL(pop_gae_stats_kernel, dim3(members), dim3(256), 0, stream, (const double2 *)part, nb, (double)K * (double)n, table, stats);
    return hipGetLastError();
}

hipError_t launch_pop_exploit(const ssg_policy &p, int members, const int32_t *src, float *adam_mv, hipStream_t stream)
{
    PopSrc s;
    for (int m = 0; m < SSG_POP_MAX_MEMBERS; ++m) s.src[m] = (uint8_t)(m < members ? src[m] : m);
    const int L = ppo_packed_len(p);
    hipLaunchKernelGGL(pop_exploit_kernel, dim3((3 * L + 255) / 256, members), dim3(256), 0, stream, s, L, const_cast<float *>(p.dev_params),
                       adam_mv);
    return hipGetLastError();
}

hipError_t launch_pop_episode_stats(const MemberLayout &lay, int K, int N, const double *rew, const uint8_t *done, double *carry_ret,
                                    int32_t *carry_len, int64_t *out, hipStream_t stream)
{
    const dim3 grid((lay.n + 255) / 256, lay.members);
    if (lay.slices)
        hipLaunchKernelGGL(pop_episode_stats_sliced_kernel, grid, dim3(256), 0, stream, K, N, lay.slices, rew, done, carry_ret, carry_len,
                           reinterpret_cast<unsigned long long *>(out));
    else
        hipLaunchKernelGGL(pop_episode_stats_kernel, grid, dim3(256), 0, stream, K, N, lay.n, rew, done, carry_ret, carry_len,
                           reinterpret_cast<unsigned long long *>(out));
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------------------
// data parallel: one policy trained from W shards' gradients (ssg_ppo_adv_moments / ssg_ppo_set_adv_moments / ssg_ppo_apply_shards)
// ------------------------------------------------------------------------------------------------------------------------------
// Every rank runs these launches on the same gathered rows, so the ranks' parameters stay bit-identical without a broadcast.  The
// kernels sit at the end of the object, behind everything it held: those kernels keep their device code (profiles/dp/README.md).
namespace {

// GAE's f64 partials, added again in gae_stats_body's order, as the shard's moments {S, Q, n, 0} instead of its statistics.
__global__ void __launch_bounds__(256) dp_adv_moments_kernel(const double2 *__restrict__ part, int nblocks, double n, double *__restrict__ out4)
{
    __shared__ double rs[256], rq[256];
    double s = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) {
        s += part[b].x;
        q += part[b].y;
    }
    rs[threadIdx.x] = s;
    rq[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rs[threadIdx.x] += rs[threadIdx.x + w];
            rq[threadIdx.x] += rq[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out4[0] = rs[0];
        out4[1] = rq[0];
        out4[2] = n;
        out4[3] = 0.0;
    }
}

// One lane: the W rows' S, Q and n in row order (f64), then gae_stats_body's formula.  Fewer than 2 samples in all have no unbiased
// std: the row becomes NaN, which no later gradient can mistake for statistics (the device has no return code).
__global__ void __launch_bounds__(64) dp_set_adv_moments_kernel(int W, const double *__restrict__ rows, float adv_eps, float *__restrict__ stats)
{
    if (threadIdx.x != 0) return;
    double S = 0.0, Q = 0.0, n = 0.0;
    for (int r = 0; r < W; ++r) {
        S += rows[r * 4 + 0];
        Q += rows[r * 4 + 1];
        n += rows[r * 4 + 2];
    }
    if (!(n >= 2.0)) {
        const float bad = __int_as_float(0x7fc00000);
        stats[0] = bad;
        stats[1] = bad;
        stats[2] = bad;
        stats[3] = 0.0f;
        return;
    }
    const double mean = S / n;
    double var = (Q - S * mean) / (n - 1.0);
    if (var < 0.0) var = 0.0;
    const float stdp = (float)sqrt(var) + adv_eps;
    stats[0] = (float)mean;
    stats[1] = stdp;
    stats[2] = 1.0f / stdp;
    stats[3] = 0.0f;
}

struct DpWeights {
    float w[SSG_DP_MAX_SHARDS]; // by value in the kernel arguments: M_r / sum M, rounded on the host
};

// Grid ceil((P + kExtStats) / 256), entry p on lane p % 256 of workgroup p / 256 — ppo_reduce_ext_kernel's partition, so the sums of
// squares below are its partials.  g = w_0*row_0[p], then g = g + w_r*row_r[p] in row order, every product and sum rounded to f32
// on its own.  p < P: the gradient entry — into gvec with the clip sequence (ppo_clip_kernel follows), else one Adam step.  p >= P:
// the stats columns, as ppo_reduce_body's EXT branch writes them; ext == 0 (the plain loss): columns 0..3, the rest zero, no KL sum.
__global__ void __launch_bounds__(256) dp_apply_kernel(const float *__restrict__ rows, int W, const DpWeights wt, int P, int ext,
                                                       const float *__restrict__ kl_coef, float *__restrict__ klacc, int first_chunk,
                                                       float *__restrict__ gvec, double *__restrict__ part, float *__restrict__ stats_out,
                                                       float *__restrict__ params, float *__restrict__ mv, const AdamArgs ad)
{
    __shared__ double sq[256];
    const int stride = P + kExtStats;
    const int p = blockIdx.x * 256 + threadIdx.x;
    float s = 0.0f;
    if (p < stride) {
        s = __fmul_rn(wt.w[0], rows[p]);
        for (int r = 1; r < W; ++r) s = __fadd_rn(s, __fmul_rn(wt.w[r], rows[(size_t)r * stride + p]));
    }
    if (p >= P && p < stride) {
        const int q = p - P;
        const float klc = ext && kl_coef ? kl_coef[0] : 0.0f;
        if (stats_out) stats_out[q] = q < (ext ? 5 : 4) ? s : (q == 6 ? (klc > 0.0f ? klc : 0.0f) : 0.0f);
        if (ext && q == 4) klacc[0] = first_chunk ? s : klacc[0] + s;
    }
    if (p < P) {
        if (gvec) gvec[p] = s;
        else adam_apply(ad, s, p, P, params, mv);
    }
    if (gvec) { // the workgroup's sum of squares, f64, ppo_reduce_body's tree
        sq[threadIdx.x] = p < P ? (double)s * (double)s : 0.0;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sq[threadIdx.x] += sq[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) part[blockIdx.x] = sq[0];
    }
}

} // namespace

hipError_t launch_dp_adv_moments(int K, int N, void *ws, double *out4, hipStream_t stream)
{
    const double2 *part = reinterpret_cast<const double2 *>(static_cast<char *>(ws) + kPpoSlotsOff);
    hipLaunchKernelGGL(dp_adv_moments_kernel, dim3(1), dim3(256), 0, stream, part, ppo_gae_blocks(N), (double)K * (double)N, out4);
    return hipGetLastError();
}

hipError_t launch_dp_set_adv_moments(int n_shards, const double *rows, double adv_eps, void *ws, hipStream_t stream)
{
    float *stats = reinterpret_cast<float *>(static_cast<char *>(ws) + kPpoStatsOff);
    hipLaunchKernelGGL(dp_set_adv_moments_kernel, dim3(1), dim3(64), 0, stream, n_shards, rows, (float)adv_eps, stats);
    return hipGetLastError();
}

hipError_t launch_dp_apply(const DpApply &a, hipStream_t stream)
{
    const ssg_policy &p = *a.policy;
    const int P = ppo_packed_len(p), stride = P + kExtStats;
    const PpoExtLayout lay = ppo_ext_layout(kPpoSlotsOff, 1, 1, P);
    char *base = static_cast<char *>(a.ws);
    DpWeights wt = {};
    double total = 0.0;
    for (int r = 0; r < a.n_shards; ++r) total += (double)a.counts[r];
    for (int r = 0; r < a.n_shards; ++r) wt.w[r] = (float)((double)a.counts[r] / total);
    const bool clip = a.ext && a.max_grad_norm > 0.0f;
    float *klacc = a.ext ? reinterpret_cast<float *>(base + lay.klacc) + kDpKlaccFloat : nullptr;
    float *gvec = clip ? reinterpret_cast<float *>(base + lay.gvec) : nullptr;
    double *part = clip ? reinterpret_cast<double *>(base + lay.part) : nullptr;
    float *params = const_cast<float *>(p.dev_params);
    const AdamArgs ad = adam_args(*a.hp, a.step);
    hipLaunchKernelGGL(dp_apply_kernel, dim3((stride + 255) / 256), dim3(256), 0, stream, a.rows, a.n_shards, wt, P, a.ext ? 1 : 0,
                       (const float *)a.kl_coef, klacc, a.first_chunk ? 1 : 0, gvec, part, a.stats_out, params, a.adam_mv, ad);
    if (clip)
        hipLaunchKernelGGL(ppo_clip_kernel<false>, dim3((P + 255) / 256), dim3(256), 0, stream, (const float *)gvec, (const double *)part,
                           lay.nb, P, a.max_grad_norm, (const float *)nullptr, a.stats_out, 0ll, params, a.adam_mv, ad,
                           (const float *)nullptr);
    if (a.ext && a.last_chunk && a.kl_coef && a.kl_target > 0.0f)
        hipLaunchKernelGGL(ppo_kl_adapt_kernel, dim3(1), dim3(256), 0, stream, 1, a.kl_coef, (const float *)klacc, (float)a.n_chunks,
                           a.kl_target, (const float *)nullptr, (const int32_t *)nullptr);
    return hipGetLastError();
}

} // namespace ssg
