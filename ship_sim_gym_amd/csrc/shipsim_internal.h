// shipsim_internal.h — shared between the kernels (.hip) and the C-ABI host layer (.cpp).  Not installed.
#ifndef SHIPSIM_INTERNAL_H
#define SHIPSIM_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "shipsim.h"

namespace ssg {

// f64 column indices inside the state blob (each column = n_pad doubles, lane-contiguous)
enum { COL_X = 0, COL_Y, COL_VX, COL_VY, COL_A, COL_W, COL_CUM, COL_LIDAR /* + n_beams columns */ };
// i32 column indices
enum { ICOL_RUDDER = 0, ICOL_STEP, ICOL_MAP, ICOL_EPISODE /* episodes started so far (map_ring mode) */,
       ICOL_GEN /* worlds drawn so far for this env's ring */, ICOL_COUNT };

// config 4 (n_ships = 4) f64 columns of the dyn region
enum {
    DC_TRAFFIC = 0,                                   // 3 ships x (x, y, angle, vx, vy, w, v_bias.x, v_bias.y, w_bias)
    DC_GOAL_COLS = 8,
    DC_GOALS = DC_TRAFFIC + 9 * SSG_N_TRAFFIC,        // SSG_MAX_GOALS x (x, y, vx, vy, v_bias.x, v_bias.y, w, w_bias)
    DC_ARB = DC_GOALS + DC_GOAL_COLS * SSG_MAX_GOALS, // per pair: jnAcc[2], jtAcc[2]
    kDynPairs = 54,                                   // ship-bank 6, ship-ship 3, goal-bank 12, goal-ship 18, goal-goal 15
    kPolyPairs = 9,                                   // the first 9 pair ids are polygon pairs (two hashed contacts)
    DC_PREV_GOAL = DC_ARB + 4 * kDynPairs,            // (gx, gy) of the newest frame: the next observation's older frame
    DC_TROT = DC_PREV_GOAL + 2,                       // 3 ships x (cos a, sin a) of the angle column: the step kernel's collide_ship
                                                      // against traffic rebuilds the ship's world hull without a sincos
    DC_COUNT = DC_TROT + 2 * SSG_N_TRAFFIC
};
// u32 columns of the dyn region
enum { DU_META = 0 /* state | age << 3 | count << 5 */, DU_HASH = kDynPairs /* contact hashes, polygon pairs */,
       DU_COUNT = kDynPairs + kPolyPairs };

// The queue of the full dyn step is BUCKETED by (bank record, steps since the reset): after a reset the traffic ships and goal
// bodies of an env replay a transient that depends on its world and age only (the player pushes nothing), so envs of one
// bucket walk the same code path and a wave of bucket-mates does not pay for the union of 64 different ones.  Every bucket has
// its own array of n_pad slots (DevCfg::dyn_bucket) and its own counter; a producer appends with one returning atomic.  The
// full step walks the buckets MAP-MAJOR, every map's stretch rounded up to a wave (kDynGrp slots): the lanes of a wave all sit
// on one bank record, which it then keeps once per wave instead of once per lane — and finds its 48 entries from the 512
// counters alone (rounds 2-4 ran a counting-sort kernel between the producers and the full step: 5.4 us per step).
constexpr int kDynAgeBuckets = 8, kDynMapBuckets = 64, kDynBuckets = kDynAgeBuckets * kDynMapBuckets;
constexpr int kDynGrp = 48;       // envs per wave of the full step (shipsim_dynamics.hip: kGrp)
constexpr int kDynPad = kDynMapBuckets * kDynGrp; // slots beyond n_pad the full step's grid covers: every map's stretch rounded up to a wave
// Counters: one per 128-byte line.  (Atomics on neighbouring words of ONE line serialise in the L2.  Measured with the bucketed
// queue: a map's eight age counters in one line — two 16-byte loads per lane at the head of the full step instead of eight
// 4-byte ones over 512 lines — made the full step 1.1 us faster and the step kernel, whose returning atomics then meet on 64
// lines, 1.7 us slower.)
constexpr int kDynBucketStride = 32;
constexpr int kDynCountWords = kDynBuckets * kDynBucketStride; // one set; DevCfg::dyn_count holds two (see dyn_par)
__host__ __device__ __forceinline__ constexpr int dyn_counter_word(unsigned bucket) { return (int)bucket * kDynBucketStride; }
// sort bucket of an env that is `age` steps into its episode on bank record `map_id`
__host__ __device__ __forceinline__ unsigned dyn_bucket_of(int age, int map_id)
{
    const unsigned agek = (unsigned)(age < kDynAgeBuckets - 1 ? (age < 0 ? 0 : age) : kDynAgeBuckets - 1);
    return ((unsigned)map_id & (unsigned)(kDynMapBuckets - 1)) * (unsigned)kDynAgeBuckets + agek;
}
// The sorted queue scatters the envs of a wave over the whole batch: gathered from the struct-of-arrays columns, an env's 75
// body fields cost the wave 75 x 64 cache lines.  The full dyn step therefore keeps a ROW-MAJOR shadow of them, five 128-byte
// lines per env: [0, 48) goal g field f at 8g + f, [48, 75) traffic ship k field f at 48 + 9k + f.  Written by everything that
// writes the columns (dyn_init, the full step's write-back, ssg_dyn_invalidate after a caller's own writes); read by the full
// step only.  The columns stay the interface of everything else (classify pass, step kernel, ssg_state_field).
constexpr int kDynRow = 80, kDynRowTraffic = 48;
// ---- the memo of the full dyn step (round 5; bank mode with at most kDynMapBuckets records) -------------------------------
// cpSpaceStep of an env's non-player bodies is a pure function of those bodies' cpBody fields, the cached arbiters, the goal
// mask and the bank record (the player pushes nothing).  In bank mode thousands of envs share a record and replay the SAME
// states after every reset: the first env that computes the step of a state stores (state -> next state) in a table kept in the
// state blob, and every later env in that state copies the result instead of walking the ~100 k-cycle GJK / EPA / solver chain
// that every launch of the full step used to end with.  A hit is verified against the COMPLETE input state (not a hash), so a
// memoised step writes bit for bit what the computed one writes.  Entry = header + key + value, in 8-byte words:
//   [0] tag  = (hash & ~0xFF) | generation (1..255; 0 = never used): claimed with one atomicCAS
//   [1] ready = tag once key and value are complete;  [2] born = the launch number that wrote it (entries are used from the
//   NEXT launch on: nothing written by a running launch is ever read by it);  [3] pad
//   key  [4 .. 4 + kMemoKeyWords): header (bank record | participating goals | live-arbiter count), live mask, the three
//        ships' 9 fields, the participating goals' 8 fields (0 for goals that are removed or inert: zero velocities and no
//        broadphase candidate this step — their step is the identity and nobody sees them), up to 4 cached arbiters
//        (pair id | state/age/count | contact hashes, 4 accumulated impulses)
//   value: header (changed | arbiters written | arbiters aged), live mask out, ships 3 x (9 fields, cos, sin), goals 6 x 8,
//        up to 8 arbiter records, up to 4 aged arbiters' meta words
constexpr int kMemoEntries = 1 << 14;
enum { ME_TAG = 0, ME_READY, ME_BORN, ME_PAD, ME_KEY };
constexpr int kMemoArbIn = 4, kMemoArbOut = 8, kMemoAged = 4, kMemoArbWords = 6 /* pair id | meta | hashes, 4 impulses, pad */;
// (every section starts on an even word: 16-byte loads; sections a lane's state does not use — goals that take no part, arbiter
// slots beyond its count — are neither written nor read: the key's header says which ones are in use)
constexpr int kMemoKeyShips = 2, kMemoKeyGoals = kMemoKeyShips + 28 /* 3 x 9 fields + pad */, kMemoKeyArbs = kMemoKeyGoals + 8 * SSG_MAX_GOALS;
constexpr int kMemoKeyWords = kMemoKeyArbs + kMemoArbIn * kMemoArbWords; // 102
constexpr int ME_VAL = ME_KEY + kMemoKeyWords;
constexpr int kMemoValShipWords = 12 /* 9 fields, cos, sin, pad */;
constexpr int kMemoValShips = 2, kMemoValGoals = kMemoValShips + kMemoValShipWords * SSG_N_TRAFFIC, kMemoValArbs = kMemoValGoals + 8 * SSG_MAX_GOALS;
constexpr int kMemoValAged = kMemoValArbs + kMemoArbOut * kMemoArbWords;
constexpr int kMemoValWords = kMemoValAged + kMemoAged; // 138
constexpr int kMemoStride = ME_VAL + kMemoValWords;     // words per entry (244)
static_assert(kMemoKeyGoals % 2 == 0 && kMemoKeyArbs % 2 == 0 && kMemoValGoals % 2 == 0 && kMemoValArbs % 2 == 0 && kMemoValAged % 2 == 0, "even sections");
constexpr int kMemoProbes = 4;
// The narrowphase memo (same launches, same generation / born protocol, a table of its own): cpCollide of a traffic ship against
// a bank hull — GJK + EPA from a cold start + support-edge clipping, ~28 k cycles of a lone wave — is a pure function of the bank
// record, the side, the ship and its pose (position, rotation).  A ship that rests against its bank keeps its pose bit for bit
// while other bodies of its env still move, so envs whose STATE is new (the state memo misses) mostly meet a ship x bank pair
// that is not.  Entry: header as above, key = (record | side | ship | fingerprint | bank epoch), p.x, p.y, cos, sin;
// value = count | contact hashes, normal, p1[2], p2[2].
constexpr int kNpmEntries = 1 << 14, kNpmProbes = 2;
enum { NE_KEY = 4, NE_VAL = NE_KEY + 6, kNpmStride = NE_VAL + 12 };
constexpr int kMemoStatSlots = 256, kMemoStatWords = 16; // per workgroup slot: [0] hits [1] computed [2] results stored [3] / [4] ship x bank narrowphase memo: hits / computed; [5..15] unused
static_assert(ME_KEY % 2 == 0 && ME_VAL % 2 == 0 && kMemoStride % 2 == 0, "16-byte loads of key and value");
constexpr int kPadEnvs = 256;   // columns are padded to a multiple of this many envs
constexpr int kStatsSlots = 256;   // per-workgroup-slot i64 counters: [0] sum_return*100 [1] sum_length [2] episodes [3] goals hit
constexpr int kStatsDoubles = 4 * kStatsSlots;

// Kernel argument block (by value in kernarg memory; wave-uniform -> SGPRs).
struct DevCfg {
    int n_envs, n_pad;
    long long env_id_base;
    int n_beams, history /* frames the step kernel writes: min(full_history, 2) */, max_steps, n_goals;
    int full_history;     // EnvConfig.HISTORY_SIZE
    double *obs2;         // [n_envs][2F] staging rows of the step kernel when full_history > 2 (inside the state blob)
    double *obsH;         // [n_envs][H*F] the handle's own observation rows when full_history > 2 (frame-shift source)
    unsigned flags;
    int n_maps;
    int map_ring;         // 0, or R: env e owns bank records [e*R, e*R + R) as a ring of worlds (one per episode)
    int rudder_step, rudder_max;
    double spread_deg, lidar_dist, goal_r, width, height, dt, damp, spawn_x, spawn_y;
    double hull[2 * SSG_SHIP_VERTS], nrm[2 * SSG_SHIP_VERTS];
    double m_inv, i_inv, force_y, px0, py0;
    double beam_cos[SSG_MAX_BEAMS], beam_sin[SSG_MAX_BEAMS]; // cos/sin of the beam offsets phi_i from the heading
    double *f64cols;
    int32_t *i32cols;
    uint8_t *mask;
    double *stats;
    const double *bank;
    unsigned long long *dbg; // -DSSG_STAMPS builds: per-wave s_memtime stamps; product builds: the launch's clock stamps (ssg_debug_launch_clock)
    double *term_obs;        // nullable: [n_envs][history * (6 + n_beams)] rows that receive the TERMINAL observation of an env the
                             // step kernel auto-resets (ssg_set_terminal_obs)
    // config 4 (n_ships == 4): columns of the non-player bodies (shipsim_dynamics.hip); null otherwise
    int n_ships;
    double *dyn_f64;
    uint32_t *dyn_u32;
    unsigned long long *dyn_live; // bit p: pair p has a cached arbiter
    uint8_t *dyn_flag;            // (bit 0 unused: the step kernel runs collide_ship against the traffic ships itself)
                                  // bit 1: env was auto-reset by the step kernel (step -> dyn kernel)
                                  // bit 2: the env's non-player bodies are at rest (see dyn_classify_kernel)
                                  // bit 3: the env has an entry in the queue of the next full step (cleared by that step)
    unsigned long long *dyn_hash; // bank generation (DynCfg::bank_epoch) the rest bit was established for
    // The queue of the full dyn step.  Produced for step t+1 by the step kernel's body role at the end of step t (or, after a
    // host-side reset / bank change / ssg_dyn_invalidate, by dyn_classify_kernel): one array of n_pad env indices per sort bucket,
    // filled in arrival order (a returning atomic on the bucket's counter).  Two counter sets: the full step reads set dyn_par
    // and zeroes the other one, into which the step kernel that follows counts the next step's entries; the host flips dyn_par
    // after every step.
    int32_t *dyn_bucket;          // [kDynBuckets][n_pad]
    unsigned *dyn_count;          // [2][kDynCountWords]: bucket b's counter at dyn_counter_word(b) of its set
    int32_t *dyn_qmap;            // [n_pad] the bank record an env's queue entry was queued under (valid while flag bit 3 is set)
    int dyn_par;                  // the counter set that holds THIS step's queue
    double dyn_reach2[SSG_N_TRAFFIC]; // (traffic ship k's hull radius + margin)^2: the step kernel's reject in front of collide_ship's exact test
    double thull[SSG_N_TRAFFIC][2 * SSG_SHIP_VERTS], tnrm[SSG_N_TRAFFIC][2 * SSG_SHIP_VERTS]; // the traffic hulls (local), for that test
    double *dyn_row;              // [n_pad][kDynRow] row-major shadow of the DC_TRAFFIC / DC_GOALS columns (see kDynRow)
    // the memo of the full dyn step (see kMemoEntries); null = off (SSG_FLAG_DYN_MEMO_OFF, per-env worlds, banks of > 64 records)
    unsigned long long *dyn_memo;       // [kMemoEntries][kMemoStride]
    unsigned long long *dyn_memo_stats; // [kMemoStatSlots][kMemoStatWords]
    unsigned long long *dyn_npm;        // [kNpmEntries][kNpmStride] the narrowphase memo (null with dyn_memo)
    unsigned long long dyn_seq;         // number of this launch of the full step (entries born in it are not read by it)
    unsigned dyn_memo_gen;              // 1..255: entries of another generation count as empty (bank change = new generation)
};

// Constants of the traffic ships and of Chipmunk's solver, by value to the dyn kernels only.
struct DynCfg {
    double thull[SSG_N_TRAFFIC][2 * SSG_SHIP_VERTS], tnrm[SSG_N_TRAFFIC][2 * SSG_SHIP_VERTS];
    double tx[SSG_N_TRAFFIC], ty[SSG_N_TRAFFIC], t_i_inv[SSG_N_TRAFFIC], t_m_inv;
    double goal_m_inv, goal_i_inv;
    double ship_friction;  // 0.7 (models.py:98); banks and goals keep Chipmunk's default 0
    double bias_coef, slop; // 1 - pow(collisionBias, dt), collisionSlop
    unsigned bank_epoch;    // bumped whenever the map bank changes: part of the pose hash
    int stop_after;         // development aid (SSG_DYN_STOP): leave the dyn kernel after phase n; 0 = run it all
    unsigned memo_fp;       // fingerprint of every constant the full step reads (this struct, dt, damping, goal radius, ...): part of
                            // the memo key, so a table never answers for another configuration
};

// traj: env rows between the output slots of consecutive steps of the launch (0 = every step rewrites the same rows)
hipError_t launch_step(const DevCfg &c, int epw, bool lds, size_t lds_bytes, const int32_t *actions_kn, int K, double *obs,
                       double *reward, uint8_t *done, uint8_t *flags, long long traj, hipStream_t stream);
size_t step_lds_bytes(int n_beams, int block, bool lds_bank, int n_maps, bool dyn /* the config-4 instantiations */);
hipError_t prepare_step(const DevCfg &c, int block, bool lds, size_t lds_bytes);
hipError_t launch_reset(const DevCfg &c, const uint8_t *mask, const int32_t *map_ids, double *obs, hipStream_t stream);
// sort + full step of the queue; classify = true: rebuild the queue first from the per-env flags (the step kernel did not
// produce it: first step after a host-side reset, bank change or ssg_dyn_invalidate)
hipError_t launch_dyn_step(const DevCfg &c, const DynCfg &d, bool classify, hipStream_t stream);
hipError_t prepare_dyn(const DevCfg &c);
hipError_t launch_dyn_invalidate(const DevCfg &c, const uint8_t *mask, hipStream_t stream);
hipError_t launch_dyn_reset(const DevCfg &c, const DynCfg &d, const uint8_t *mask, const int32_t *map_ids, double *obs, bool append, hipStream_t stream); // player + other bodies, one launch
hipError_t launch_render(const DevCfg &c, const DynCfg &d, int e, int width, int height, uint8_t *rgb, unsigned flags,
                         hipStream_t stream);
hipError_t launch_calib_copy8(const double *src, double *dst, size_t n, hipStream_t stream);
hipError_t launch_clock_probe(unsigned long long *out, int n_blocks, int iters, hipStream_t stream);
hipError_t launch_remap_map_ids(const DevCfg &c, hipStream_t stream); // ICOL_MAP %= n_maps after the bank shrank
hipError_t launch_history_shift(const DevCfg &c, const uint8_t *done, double *obs, hipStream_t stream);
hipError_t launch_generate_bank(uint64_t seed, int n_maps, int n_goals, double width, double height, double width_frac,
                                double spawn_x, double spawn_y, double *bank, double *raw, hipStream_t stream);
// map_ring mode: scan the envs for missing worlds (queue of env << 32 | episode at `queue`, its length at `count`, which
// the caller zeroed on the stream), then generate them densely; raw: optional per-slot debug rows
hipError_t launch_refill_worlds(const DevCfg &c, uint64_t seed, double width_frac, unsigned long long *queue, unsigned *count,
                                double *bank, double *raw, hipStream_t stream);
hipError_t launch_fill_actions(uint64_t seed, uint64_t step0, int K, long long env_base, int n, int32_t *out,
                               hipStream_t stream);
// How a launch's envs are divided among members.  ONE convention, for every launcher below and for the entry points that resolve it
// (shipsim_api.cpp: member_layout, whole_layout) and hand it down unchanged:
//   members >= 1;
//   n is the launch's WIDTH: all envs for one policy, else the equal slice N / members — member m owns envs [m*n, (m+1)*n) — or the
//     widest slice of a bound table;
//   slices is NULL unless a table is bound and applies: the device table of ssg_pop_set_slices, SSG_POP_SLICE_ROW int32 per member =
//     {o_m, n_m, ppo_gae_blocks(n_m), 0}; member m then owns envs [o_m, o_m + n_m).
// Whether a launch runs a population's instantiations (a parameter row per member) is a separate fact, said beside the record.
struct MemberLayout {
    int members, n;
    const int32_t *slices;
};
// The policy kernel (shipsim_policy.hip).  One acting launch: one policy over its layout's envs, or a population (pop) — p is then the
// shared shape with dev_params = f32 [members][L], and member m acts on its envs.  act / logp NULL = value only (no sampling), x NULL = no
// x rows.  greedy: the arg-max action and its logp; act, logp and value are all written and uniform, seed, step and env_base are not
// read.  filter (nullable): the kernels of
// shipsim_policy_filter.o, x = (float)clamp((obs - mean) / denom, +-clip) from member m's state rows in place of obs / scale.
struct ObsFilterArgs { const double *state; double clip; };
struct PolicyLaunch {
    const double *obs;
    const float *uniform; // nullable: then Philox draws under (seed, step)
    uint64_t seed;
    int64_t step;
    int32_t *act;
    float *logp, *value, *x;
    bool greedy;
    const ssg_policy *policy;
    MemberLayout lay;
    bool pop;              // the POP instantiations: parameter row m for member m
    long long env_base;    // the global id of env 0 (the uniforms' counter)
    const ObsFilterArgs *filter;
};
size_t policy_lds_bytes(const ssg_policy &p, bool both_towers); // (both_towers: a separate-value launch that also samples)
hipError_t prepare_policy(); // (the dynamic-LDS limit of the kernels: up to 90 KB per workgroup at obs_dim 176, hidden 128; 124 KB when a separate-value launch keeps its third buffer)
hipError_t launch_policy(const PolicyLaunch &l, hipStream_t stream);
// the same with l.filter set, in an object of its own (-DSSG_POLICY_FILTER_TU) so that the unfiltered instantiations are compiled as before;
// launch_policy hands such a record on
hipError_t prepare_policy_filter();
hipError_t launch_policy_filter(const PolicyLaunch &l, hipStream_t stream);
// The time-out values of a rollout's K rows (ssg_timeout_values / ssg_pop_timeout_values), in a third object of shipsim_policy.hip
// (-DSSG_POLICY_BOOT_TU).  Of l it reads policy, lay, pop and filter; row k's flags and boot entries start k*stride in, its
// observation rows k*n_envs*obs_dim doubles into term_obs.
struct TimeoutLaunch {
    int K, n_envs;
    size_t stride;
    const uint8_t *flags;
    const double *term_obs;
    float *boot;
};
hipError_t prepare_policy_boot();
hipError_t launch_timeout_values(const PolicyLaunch &l, const TimeoutLaunch &t, hipStream_t stream);
// GAE and the PPO update (shipsim_ppo.hip).  Workspace: f32[4] advantage statistics at kPpoStatsOff (mean, std + adv_eps, its
// inverse), then from kPpoSlotsOff the gradient kernel's per-workgroup slots [grid][P + 4] — or, during ssg_ppo_gae, its f64 partials.
constexpr size_t kPpoStatsOff = 0, kPpoSlotsOff = 256;
constexpr int kPpoMaxGrid = 512; // gradient workgroups at most (the slots a minibatch's partial gradients are summed over)
inline int ppo_gae_blocks(long long N) { return (int)((N + 255) / 256); }
int ppo_packed_len(const ssg_policy &p);
int ppo_grid(long long M); // gradient workgroups for a minibatch of M samples
size_t ppo_grad_lds_bytes(const ssg_policy &p);
hipError_t prepare_ppo(); // (the dynamic-LDS limit of the gradient kernel: up to 151 KB at obs_dim 176, hidden 128, 2 layers)
hipError_t launch_ppo_gae(const ssg_ppo_hparams &hp, int K, int N, const double *rew, const uint8_t *done, const float *val,
                          const float *last_val, float *adv, float *ret, void *ws, hipStream_t stream, const float *boot = nullptr);
hipError_t launch_ppo_adam(const ssg_policy &p, const ssg_ppo_hparams &hp, const float *grad, float *adam_mv, int64_t step,
                           hipStream_t stream);
// A population of `members` policies on one handle (ssg_pop_*): p is the shared shape with dev_params = f32 [members][L]; member m owns
// the n = N / members envs [m*n, (m+1)*n).  Workspace: f32 [members][4] advantage statistics at kPpoStatsOff (room for
// SSG_POP_MAX_MEMBERS rows), then from kPopSlotsOff the gradient slots [members][grid][L + 4] — or, during ssg_pop_gae, the f64
// partials [members][ppo_gae_blocks(n)].  table: the device copy of what pop_pack wrote, kPopTableRow floats per member (loss / GAE
// constants), then per Adam step kPopTableRow floats per member.
constexpr size_t kPopSlotsOff = 4096;
constexpr int kPopTableRow = 8;
// The schedule table of ssg_pop_update_sched (ssg_pop_pack_schedule writes it, the caller uploads it): kPopSchedRow int32 per member —
// SH_* — then per launch kPopSchedRow int32 per member — SR_*: what differs between the members within launch j, where member m runs
// ITS minibatch j (chunk j % chunks_m of its permutation row j / chunks_m) or, past its steps_m, nothing.
constexpr int kPopSchedRow = SSG_POP_SCHED_ROW;
enum { SH_STEPS = 0, SH_CHUNKS, SH_C, SH_EPOCHS, SH_PREFIX /* int64: entries [4], [5]; ssg_pop_pack_schedule_samples only */ };
enum { SR_OFF = 0 /* int64: entries [0], [1] */, SR_M = 2, SR_G, SR_FIRST, SR_ACTIVE, SR_INVM /* f32 bits of 1 / (float)M */ };
static_assert(SSG_POP_MAX_MEMBERS * 16 <= kPopSlotsOff, "the members' advantage statistics fit in front of the slots");
void pop_pack(int members, const ssg_ppo_hparams *hp, int64_t step0, int n_steps, float *out); // host only
void pop_pack_steps(int members, const ssg_ppo_hparams *hp, const int64_t *step0, int n_steps, float *out); // (a starting step per member)
hipError_t launch_pop_gae(const MemberLayout &lay, int K, int N, const float *table, const double *rew, const uint8_t *done, const float *val,
                          const float *last_val, const float *boot /* nullable */, float *adv, float *ret, void *ws, hipStream_t stream);
hipError_t launch_pop_exploit(const ssg_policy &p, int members, const int32_t *src, float *adam_mv, hipStream_t stream);
// The extended update (ssg_ppo_grad_ext / ssg_ppo_update_ext / ssg_pop_update_ext): value clip, KL penalty, gradient-norm clip.
// From the plain path's slot offset the workspace holds the running sum of the epoch's mean(KL) (f32 [members]), the gradient vector of
// the clip sequence (f32 [members][P]), its per-workgroup sums of squares (f64 [members][nb]), then the slots [grid][P + kExtStats].
constexpr int kExtStats = 8;  // loss sums per slot and stats columns per minibatch
constexpr int kPopExtRow = 4; // ssg_pop_ext.dev_ext: vf_clip, max_grad_norm, kl_target, 0 per member
struct PpoExtLayout {
    size_t slots, gvec, part, klacc, end;
    int nb; // workgroups of the reduction: ceil((P + kExtStats) / 256)
};
inline PpoExtLayout ppo_ext_layout(size_t slots_off, int members, int G, int P)
{
    const size_t m = (size_t)members, a = 255;
    PpoExtLayout l;
    l.nb = (P + kExtStats + 255) / 256;
    // (the fixed-size parts first: their places do not move with the minibatch length; every part is `members` times one policy's,
    // each rounded up to 256 bytes, so a population's workspace stays P times a single policy's)
    l.klacc = slots_off;
    l.gvec = l.klacc + m * 256;
    l.part = l.gvec + m * (((size_t)P * sizeof(float) + a) & ~a);
    l.slots = l.part + m * (((size_t)l.nb * sizeof(double) + a) & ~a);
    l.end = l.slots + m * (size_t)G * (size_t)(P + kExtStats) * sizeof(float);
    return l;
}
struct PpoExtLaunch {
    const float *logp_all, *value_old; // device; NULL where the term that reads them is off for everyone
    float *kl_coef;                    // device f32 [members]; NULL = no KL term
    const float *pop_ext;              // a population's f32 [members][kPopExtRow]; NULL for one policy
    float vf_clip, max_grad_norm;      // one policy's constants (a population reads pop_ext)
    bool clip_seq;                     // three launches per minibatch: gradient, reduction + sums of squares, clip + Adam
    bool first_chunk;                  // the minibatch is the first of its epoch (restarts the running KL sum)
};
size_t ppo_grad_ext_lds_bytes(const ssg_policy &p);
// the five per-sample columns of a batch (device): rows t*N + e of the [K][N] rollout buffers, x with obs_dim floats per row
struct PpoBatch {
    const float *x;
    const int32_t *act;
    const float *logp, *adv, *ret;
};
// One minibatch of `members` policies: the gradients into the workspace's slots, then per member their sum — into grad_out (nullable)
// and, with adam_mv, one Adam step on its parameter row — and the minibatch's loss means into stats_out (nullable; member m's row at
// stats_out + m*stats_stride; 4 floats, kExtStats with ext).  The constants are ONE policy's (hp, and the Adam step number `step`;
// table NULL, lay.members 1, lay.n / N / idx_stride unused) or a population's (table: its loss rows, adam_row: this step's Adam rows).
struct PpoMinibatch {
    const ssg_policy *policy; // the shape; dev_params = f32 [members][P]
    MemberLayout lay;         // member m's sample i = t*n + e is row t*N + m*n + e, N the envs of the batch
    long long N;
    long long n_samples;      // samples per member (an index outside [0, n_samples) is a zero, gradient-free sample)
    PpoBatch batch;
    const int64_t *idx;       // M indices (member-local); member m's at idx + m*idx_stride
    long long idx_stride, M;
    void *ws;
    size_t slots_off;         // kPpoSlotsOff or kPopSlotsOff
    const ssg_ppo_hparams *hp;
    int64_t step;
    const float *table, *adam_row;
    const int32_t *sched;     // nullable; this launch's schedule records [members][kPopSchedRow]: M is then the LAUNCH's (max C_m, for
                              // the grid and the slot stride) and idx every member's first permutation row; the records say the rest
    const PpoExtLaunch *ext;  // nullable: the extended loss and reduction
    float *grad_out, *stats_out;
    long long stats_stride;
    float *adam_mv;
    // a population on unequal slices (lay.slices, with sched): the schedule table's header rows, whose entries SH_PREFIX hold
    // the int64 sum of the samples of the members before m — member m's permutation block starts perm_epochs times that far into idx
    // and its samples are K * n_m (lay.n, n_samples and idx_stride are then unused)
    const int32_t *sched_hdr;
    long long K, perm_epochs;
    // per-minibatch advantage normalisation (ssg_ppo_set_adv_norm; both NULL: the batch statistics in the workspace): the scratch's
    // stats rows and partials.  The two launches of shipsim_advnorm.hip then run ahead of the gradient launch, which reads these rows.
    // adv_stats alone (ssg_ppo_set_adv_table): a finished row of the job's table, read as it is, nothing launched ahead.
    float *adv_stats;
    double *adv_part;
};
hipError_t launch_ppo_minibatch(const PpoMinibatch &mb, hipStream_t stream);
// Per-minibatch advantage statistics (shipsim_advnorm.hip).  Scratch: f32 [members][4] rows, then f64 [members][kAdvNormBlocks][3]
// partials (s, q, c), each part rounded up to 256 bytes.
constexpr int kAdvNormBlocks = 64;
inline size_t adv_norm_stats_bytes(int members) { return ((size_t)members * 4 * sizeof(float) + 255) & ~(size_t)255; }
inline size_t adv_norm_bytes(int members)
{
    return adv_norm_stats_bytes(members) + (((size_t)members * kAdvNormBlocks * 3 * sizeof(double) + 255) & ~(size_t)255);
}
// The minibatch as PpoMinibatch names it (table NULL: one policy, adv_eps its own; else adv_eps is column adv_eps_col of table row m).
struct AdvNormLaunch {
    const float *adv;
    const int64_t *idx;
    long long M, n_samples;
    MemberLayout lay;
    long long N, idx_stride;
    const float *table;
    int adv_eps_col;
    float adv_eps;
    const int32_t *sched, *sched_hdr;
    long long K, perm_epochs;
    float *stats;
    double *part;
};
hipError_t launch_adv_norm(const AdvNormLaunch &l, hipStream_t stream);
// The job-wide form (ssg_ppo_minibatch_adv_sums / ssg_ppo_set_minibatch_adv_rows): the sums {s, q, c, 0} of every minibatch of an
// update — minibatch e*C + j is perm[e][j*chunk : min(n, (j+1)*chunk)], C = ceil(n / chunk) — in two launches, with the partials
// scratch f64 [epochs*C][kAdvNormBlocks][3]; then the table of stats rows from the W shards' gathered sums, one launch.
inline size_t minibatch_adv_bytes(int n_batches) { return ((size_t)n_batches * kAdvNormBlocks * 3 * sizeof(double) + 255) & ~(size_t)255; }
struct MinibatchAdvSums {
    const float *adv;
    const int64_t *perm;
    long long n_samples, epochs, n, chunk;
    double *part, *out;
};
hipError_t launch_minibatch_adv_sums(const MinibatchAdvSums &l, hipStream_t stream);
hipError_t launch_minibatch_adv_rows(int n_shards, int n_batches, const double *rows, float adv_eps, float *table, hipStream_t stream);
// RLlib's update_kl on every member's coefficient from the last epoch's `chunks` minibatches (sched_hdr, nullable: the schedule
// table, whose header row m holds member m's own chunk count)
hipError_t launch_kl_adapt(int members, const PpoExtLaunch &ext, float kl_target, int P, long long chunks, const int32_t *sched_hdr, void *ws,
                           size_t slots_off, hipStream_t stream);
// Data parallel (ssg_ppo_adv_moments / ssg_ppo_set_adv_moments / ssg_ppo_apply_shards; the end of shipsim_ppo.hip).  The apply keeps
// its running sum of mean(KL) at float kDpKlaccFloat of the extended layout's klacc part: float 0 is the gradient entry points' own,
// which every shard's local ssg_ppo_grad_ext overwrites between two applies.
constexpr int kDpKlaccFloat = 4;
hipError_t launch_dp_adv_moments(int K, int N, void *ws, double *out4, hipStream_t stream);
hipError_t launch_dp_set_adv_moments(int n_shards, const double *rows, double adv_eps, void *ws, hipStream_t stream);
// One apply: the rows f32 [n_shards][P + kExtStats] combined with the weights counts[r] / sum(counts), then the clip (ext and
// max_grad_norm > 0: two launches) and Adam step `step`; with last_chunk, a coefficient and kl_target > 0 the adaptation launch
// follows, dividing the running sum by n_chunks.
struct DpApply {
    const ssg_policy *policy;
    const ssg_ppo_hparams *hp;
    bool ext;                     // the extended loss's stats columns, KL sum and clip; false: the plain loss (no workspace use)
    float max_grad_norm, kl_target;
    float *kl_coef;               // device f32 [1], nullable
    int n_shards;
    const float *rows;
    const int64_t *counts;        // host
    bool first_chunk, last_chunk;
    int n_chunks;
    float *adam_mv;
    int64_t step;
    float *stats_out;             // nullable, f32 [kExtStats]
    void *ws;
};
hipError_t launch_dp_apply(const DpApply &a, hipStream_t stream);
// the acting policy's log-distribution over stored x rows (shipsim_policy.hip): member m's rows t*N + (its envs), t < K, under parameter row m
hipError_t launch_policy_dist(const ssg_policy &p, const MemberLayout &lay, long long N, int K, const float *x, float *logp_all, hipStream_t stream);
hipError_t launch_pop_episode_stats(const MemberLayout &lay, int K, int N, const double *rew, const uint8_t *done, double *carry_ret,
                                    int32_t *carry_len, int64_t *out, hipStream_t stream);
// episode accounting of an evaluation run (shipsim_eval.hip): one step's rows into the per-env carries and stats rows (an env counts its
// first E episodes), and the per-member column sums of the stats rows
constexpr int kEvalCols = SSG_EVAL_STATS;
hipError_t launch_eval_account(int N, int E, const double *rew, const uint8_t *done, const uint8_t *flags, double *carry_ret, int32_t *carry,
                               int64_t *stats, hipStream_t stream);
hipError_t launch_eval_reduce(const MemberLayout &lay, const int64_t *stats, int64_t *out, hipStream_t stream);
// the evaluation recorder (ssg_set_eval_recorder): what its launches need of the bound record and of the call.  The tracked env ids
// travel by value (kernarg memory): the library's copy of the caller's host array.
struct EvalRecIds {
    int32_t e[SSG_EVAL_REC_MAX_ENVS];
};
struct EvalRecLaunch {
    int R, C, D, E;          // slots, steps per slot, observation width, the call's episodes_per_env
    const int32_t *carry;    // the call's dev_carry: int32 [N][4], [2] = episodes counted
    int32_t *cursor, *overflow;
    double *obs, *next_obs;
    int32_t *act;
    float *logp, *value;
    double *reward;
    uint8_t *done, *flags;
    const double *term_obs;  // the record's rows, where the step kernel stored the terminal observations
    uint8_t *frames;         // nullable
    int fw, fh, fevery, fslots; // frame size, S, frames per slot = ceil(C / S)
    unsigned fflags;
};
// the step index t = cursor[slot] an ACTIVE slot writes in this iteration, or -1: its env has counted E episodes, or the slot is full.
// Nothing these launches write enters it, and the accounting launch comes after them: all of an iteration's launches agree.
__device__ __forceinline__ int eval_rec_step(const EvalRecLaunch &r, int e, int slot)
{
    if (r.carry[4 * (size_t)e + 2] >= r.E) return -1;
    const int t = r.cursor[slot];
    return t < r.C ? t : -1;
}
// (shipsim_eval.hip) ahead of the policy launch: the active slots' rows of dev_obs; between the step and the accounting launch: the
// policy's and the step's outputs for the active slots, next_obs, and the cursors
hipError_t launch_eval_record_obs(const EvalRecLaunch &r, const EvalRecIds &ids, const double *dev_obs, hipStream_t stream);
hipError_t launch_eval_record_step(const EvalRecLaunch &r, const EvalRecIds &ids, const double *dev_obs, const int32_t *act, const float *logp,
                                   const float *value, const double *rew, const uint8_t *done, const uint8_t *flags, hipStream_t stream);
// (shipsim_render.hip) `count` frames in one launch, frame i = env ids[i]; and the recorder's frames of the active slots, ahead of the step
hipError_t launch_render_envs(const DevCfg &c, const DynCfg &d, const int32_t *ids, int count, int width, int height, uint8_t *rgb,
                              unsigned flags, hipStream_t stream);
hipError_t launch_eval_record_frames(const DevCfg &c, const DynCfg &d, const EvalRecLaunch &r, const EvalRecIds &ids, hipStream_t stream);
// the observation filter (shipsim_filter.hip): 256-row tiles, staged at most kFltChunk columns at a time; the workspace holds launch 1's
// partials, f64 [members][filter_tiles(widest slice)][2][D]
constexpr int kFltTile = 256, kFltChunk = 31, kFltMaxDim = SSG_MAX_HISTORY * (6 + SSG_MAX_BEAMS);
inline int filter_tiles(long long n) { return (int)((n + kFltTile - 1) / kFltTile); }
size_t filter_workspace_bytes(int n_envs, int obs_dim, int members);
// the two launches: the rows of member m's envs of obs into its SSG_FILTER_ROWS state rows — and, with `buffer` (a job-wide filter's, else
// NULL), the same batch total into the buffer's rows too, through the dual finalise kernel: still two launches
hipError_t launch_filter_update(const double *obs, int D, const MemberLayout &lay, double eps, double *state, double *buffer, void *ws,
                                hipStream_t stream);
// state[m] = base[m] merged with rows[0][m] .. rows[n_rows - 1][m], every block f64 [members][SSG_FILTER_ROWS][D]: one launch
hipError_t launch_filter_merge_rows(const double *base, const double *rows, int n_rows, int D, int members, double eps, double *state,
                                    hipStream_t stream);
// the return filter (shipsim_retfilter.hip): the workspace holds the walk's tile partials, f64 [members][K][filter_tiles(n_envs)][2], then
// the chain's denoms, f64 [K][members]
size_t ret_filter_workspace_bytes(int n_envs, int K, int members);
// One call's launches: walk, chain and normalise when `update`, else normalise alone with the state's own denom.  Member m's envs are
// columns of the [K][stride] buffers.
struct RetFilterLaunch {
    const double *rew;
    const uint8_t *done;
    int K;
    size_t stride;
    MemberLayout lay;
    bool update;
    double clip, eps;
    const double *gamma; // f64 [members]
    double *state;       // f64 [members][SSG_FILTER_ROWS]
    double *carry;       // f64 [n_envs]
    void *workspace;
    double *out;         // [K][stride]
    double *denom_out;   // nullable: f64 [K][members]
};
hipError_t launch_ret_filter(const RetFilterLaunch &l, hipStream_t stream);
// The job-wide filter's two calls, one member (lay: the whole handle).  batches: the walk, then rows f64 [K][SSG_FILTER_ROWS], the shard's
// {mean, M2, 0, n} per step; state, out and denom_out are not read.  rows: the chain over rows f64 [n_rows][K][SSG_FILTER_ROWS] into the
// state, then the division; done, gamma and carry are not read.  The workspace is launch_ret_filter's.
hipError_t launch_ret_filter_batches(const RetFilterLaunch &l, double *rows, hipStream_t stream);
hipError_t launch_ret_filter_rows(const RetFilterLaunch &l, const double *rows, int n_rows, hipStream_t stream);
// the episode log (shipsim_eplog.hip): the workspace holds int64 [2] (the head before the call, the call's count), then the counts of
// every (row, 256-env tile), int32 [K][filter_tiles(n_envs)], scanned in place
size_t episode_log_workspace_bytes(int n_envs, int K);
// One call's three launches (count, scan, walk): the episodes that end in the [K][stride] rows go to records[(head + rank) % capacity],
// rank in (t, env) order.  lay decides the member bits of a record only.
struct EpisodeLogLaunch {
    int K, N;
    size_t stride;
    long long step0, env_base, capacity;
    MemberLayout lay;
    const double *rew;
    const uint8_t *done, *flags; // flags nullable
    double *carry_ret;           // f64 [N]
    int32_t *carry;              // int32 [N][2]
    int64_t *head;               // int64 [2]
    void *workspace;
    ssg_episode_record *records; // [capacity]
};
hipError_t launch_episode_log(const EpisodeLogLaunch &l, hipStream_t stream);
// the job-wide log's shard block: the header, int32 lb[rows + 1] padded to 16 bytes, then `stage` records
inline size_t episode_log_block_lb_bytes(int rows) { return (((size_t)rows + 1) * 4 + 15) & ~(size_t)15; }
inline size_t episode_log_block_bytes(int rows, int stage)
{
    return sizeof(ssg_episode_log_block_header) + episode_log_block_lb_bytes(rows) + sizeof(ssg_episode_record) * (size_t)stage;
}
// One shard call's four launches (count, scan, pack, walk): launch_episode_log's three on a staging ring of `stage` slots with head 0
// in the block's record region, and the pack of the header and lb.  l.records, l.head and l.capacity are not read.
hipError_t launch_episode_log_shard(const EpisodeLogLaunch &l, int rows, int stage, void *block, hipStream_t stream);
// One merge call's two launches: the records of the n_blocks stacked blocks into records[(head + R) % capacity], then the head.
hipError_t launch_episode_log_merge(int K, long long step0, int rows, int stage, const void *blocks, int n_blocks,
                                    ssg_episode_record *records, long long capacity, int64_t *head, hipStream_t stream);
// the update report (shipsim_report.hip): the scratch holds the walk's partials, f64 [members][ppo_gae_blocks(widest slice)][kReportSums]
// = sums of ret, ret^2, ret - val, (ret - val)^2, val, adv, d, d^2 and the clipped count
constexpr int kReportSums = 9;
size_t report_scratch_bytes(int n_widest, int members);
// lo = (float)log1p(-clip), -inf from clip 1 on; hi = (float)log1p(clip): formed in double (ssg_report_clip_bounds)
void report_clip_bounds(double clip, float out_lo_hi[2]);
// One call's two launches (walk, finish): member m's columns of the [K] rows (N apart) into its record out[m][SSG_REPORT_COLS].
struct ReportLaunch {
    int K, N;
    MemberLayout lay;
    const float *val, *ret, *adv;
    const int32_t *act;          // the post-update group: act, logp and lpa (f32 [K*N][4]) together, or all NULL
    const float *logp, *lpa;
    const float *bounds;         // nullable: f32 [members][2]; else lo, hi for every member
    float lo, hi;
    const float *stats;          // nullable: f32 [members][rows_max][n_cols]
    const int32_t *rows;         // nullable: int32 [members], member m's own row count (<= rows_max)
    int rows_max, n_cols;
    double *part, *out;
    double *row;                 // nullable: f64 [SSG_REPORT_ROW_COLS]; given, the second launch writes the sum row instead of the record
                                 // (one policy, no slices; out, stats and rows are then not read)
};
hipError_t launch_report(const ReportLaunch &l, hipStream_t stream);
// One launch, one small workgroup per record: the job's record from the W sum rows (f64 [W][SSG_REPORT_ROW_COLS], shard order) into
// out[0], and with per_shard shard r's own, from row r alone, into out[1 + r]; stats (nullable, f32 [n_stat_rows][n_cols]) as the finish.
hipError_t launch_report_rows(int n_rows, const double *rows, const float *stats, int n_stat_rows, int n_cols, bool per_shard, double *out,
                              hipStream_t stream);

#ifdef __HIPCC__
// One round of Philox4x32-10 (counter ctr, key key).  The counter-based streams of the library — fill_actions_kernel's actions
// (shipsim_kernels.hip) and the policy kernel's uniforms (shipsim_policy.hip) — both key it with the seed and count with
// (env_lo, env_hi, step_lo, step_hi) over the GLOBAL env id.
__device__ __forceinline__ void philox_round(uint32_t (&ctr)[4], const uint32_t (&key)[2])
{
    const uint64_t p0 = (uint64_t)0xD2511F53u * ctr[0];
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * ctr[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ ctr[1] ^ key[0];
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ ctr[3] ^ key[1];
    const uint32_t n3 = (uint32_t)p0;
    ctr[0] = n0; ctr[1] = n1; ctr[2] = n2; ctr[3] = n3;
}

// ShipEnv.reset / ShipGame.reset of ONE env (ship_env.py:171-184, game.py:260-277): the player's columns, the goal mask, the
// observation rows (deque([-1]*n), then the spawn frame).  Shared by reset_kernel and, for config 4, the kernel that also rebuilds
// the env's traffic ships and goal bodies in the same launch (shipsim_dynamics.hip).  Returns the bank record the env is reset onto.
__device__ __forceinline__ int reset_env(const DevCfg &c, const int e, const int32_t *__restrict__ map_ids, double *__restrict__ obs)
{
    const size_t np = (size_t)c.n_pad;
    int m;
    const int started = c.i32cols[ICOL_EPISODE * np + e]; // episodes this env has started so far
    if (map_ids) m = (int)((unsigned)map_ids[e] % (unsigned)c.n_maps); // a record index never points outside the bank
    else if (c.map_ring > 0) m = e * c.map_ring + started % c.map_ring;   // the env's next brand-new world
    else m = (int)((c.env_id_base + (long long)e) % (long long)c.n_maps);
    c.i32cols[ICOL_EPISODE * np + e] = started + 1;
    const double *rec = c.bank + (size_t)m * SSG_MAP_STRIDE;
    c.f64cols[COL_X * np + e] = c.spawn_x;
    c.f64cols[COL_Y * np + e] = c.spawn_y;
    c.f64cols[COL_VX * np + e] = 0.0;
    c.f64cols[COL_VY * np + e] = 0.0;
    c.f64cols[COL_A * np + e] = 0.0;
    c.f64cols[COL_W * np + e] = 0.0;
    c.f64cols[COL_CUM * np + e] = 0.0;
    for (int i = 0; i < c.n_beams; ++i) c.f64cols[(COL_LIDAR + i) * np + e] = -1.0;
    c.i32cols[ICOL_RUDDER * np + e] = 0;
    c.i32cols[ICOL_STEP * np + e] = 0;
    c.i32cols[ICOL_MAP * np + e] = m;
    c.mask[e] = (uint8_t)((1u << c.n_goals) - 1u);
    // deque([-1]*n), ship_env.py:180-181, then the spawn frame — into the caller's rows and, with HISTORY_SIZE > 2, into the
    // handle's own copy of the rows (the frame-shift kernel's source: the caller's buffer is output only)
    const int F = 6 + c.n_beams;
    double *dst[2] = {obs ? obs + (size_t)e * (size_t)(F * c.full_history) : nullptr,
                      c.obsH ? c.obsH + (size_t)e * (size_t)(F * c.full_history) : nullptr};
    for (int t = 0; t < 2; ++t) {
        double *orow = dst[t];
        if (!orow) continue;
        for (int i = 0; i < F * (c.full_history - 1); ++i) orow[i] = -1.0;
        orow += F * (c.full_history - 1);
        orow[0] = c.spawn_x; orow[1] = c.spawn_y; orow[2] = 0.0; orow[3] = 0.0;
        orow[4] = rec[SSG_MAP_OFF_SPAWN_GOAL]; orow[5] = rec[SSG_MAP_OFF_SPAWN_GOAL + 1];
        for (int i = 0; i < c.n_beams; ++i) orow[6 + i] = -1.0;
    }
    return m;
}

// sin / cos of a body angle (cpvforangle).  The library's sincos is ~190 instructions of full-range machinery; body
// angles stay within a few turns, so for |a| <= 2^18 this is a three-term Cody-Waite reduction by pi/2 with FMAs
// (error < 2^-100 |a|) followed by the fdlibm / musl kernels on [-pi/4, pi/4] with the reduction's tail.  The contract,
// for |a| <= 2^18: |error| <= max(1 ulp of the exact result, 2^-100 |a|) — within 1 ulp of sin / cos wherever the
// result is large enough for the reduction's error to resolve, and 2^-100 |a| absolute at the doubles nearest k pi/2,
// whose exact sin or cos is tiny (hundreds of ulps of a 1e-14 result there, 1e-27 absolute: the same class as the
// library's own result for a body's rotation); sin is odd and cos even bit for bit; (0) -> (0, 1) exactly.  Asserted
// against an exact (mpmath) fixture built around these edges by tests/test_sincos.py, on a host build of this very
// function (it is pure IEEE f64 with fma and rint: host and device bits agree), and on the step kernel's own bits in
// every layout by tests/test_sincos_gpu.py; the measured errors: profiles/sincos/README.md.  One definition for the
// step kernel and the dyn kernels, so the player's rotation has the same bits wherever it is recomputed.
__host__ __device__ __forceinline__ void sincos_body(double a, double *sn_out, double *cs_out)
{
    if (!(fabs(a) <= 262144.0)) { // (also NaN / inf)
        sincos(a, sn_out, cs_out);
        return;
    }
    const double k = rint(a * 6.36619772367581382433e-01);
    const double r1 = fma(-k, 1.57079632679489655800e+00, a);
    const double r = fma(-k, 6.12323399573676603587e-17, r1);
    double y = fma(-k, 6.12323399573676603587e-17, r1 - r); // the tail of the reduced argument
    y = fma(k, 1.4973849048591698e-33, y);                  // pi/2 = HI + MID - 1.497e-33
    const int n = (int)k;
    const double z = r * r, w = z * z;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double rs = fma(z, fma(z, S4, S3), S2) + z * w * fma(z, S6, S5);
    const double v = z * r;
    const double s0 = r - ((z * (0.5 * y - v * rs) - y) - v * S1);
    const double rc = z * fma(z, fma(z, C3, C2), C1) + w * w * fma(z, fma(z, C6, C5), C4);
    const double hz = 0.5 * z, ww = 1.0 - hz;
    const double c0 = ww + (((1.0 - ww) - hz) + (z * rc - r * y));
    double sn = (n & 1) ? c0 : s0, cs = (n & 1) ? s0 : c0;
    sn = (n & 2) ? -sn : sn;
    cs = ((n + 1) & 2) ? -cs : cs;
    *sn_out = sn;
    *cs_out = cs;
}
#endif

} // namespace ssg
#endif
