/*
 * shipsim.h — C ABI of libshipsim.so: the MI355X (gfx950) batched replacement for the pymunk-backed
 * ShipEnv.step()/reset() hot path of CapAI/ship-sim-gym.
 *
 * The reference reaches its physics through pymunk 5.4.0's cffi binding of libchipmunk.so
 * (notebooks/"Ship Sim Gym.ipynb":51, requirements.txt:78).  Each entry point below names the reference
 * call site(s) it replaces; all pointers are plain host or device addresses, sizes are explicit, no C++ or
 * torch types cross the boundary, nothing throws and nothing aborts.  Return value: 0 (SSG_OK) or a
 * negative ssg_status; ssg_last_error() gives the text.  A handle is used by one host thread at a time;
 * distinct handles (one per GPU / per env shard) are independent.  Device work is enqueued on the caller's
 * hipStream_t (passed as void*) and is asynchronous unless stated.
 *
 * Device memory is owned by the caller (PyTorch-ROCm tensors as containers): the state blob, the map bank
 * and every per-call buffer.  The library owns only the handle (host memory).
 */
#ifndef SHIPSIM_H
#define SHIPSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SSG_ABI_VERSION 9 /* 2: ssg_config.n_ships, SSG_F_TRAFFIC / SSG_F_GOAL_BODIES (config 4); 3: ssg_init_state;
                             4: map record without dtMin/dtMax (SSG_MAP_STRIDE 145, SSG_PLANE_DOUBLES 5);
                             5: ssg_config.map_ring, ssg_refill_worlds (a brand-new world per episode, generated on the device);
                             6: ssg_rollout_traj (every step of a fused rollout lands in its own slot of a trajectory buffer);
                             7: SSG_FLAG_DYN_MEMO_OFF, SSG_F_DYN_MEMO_STATS (config 4: the memo table of the full cpSpaceStep lives
                                in the state blob, which grows by ~30 MB);
                             8: ssg_set_terminal_obs (the RLlib flow without a reset launch), ssg_step_host / ssg_wait_host (a numpy-protocol step in one
                                call), ssg_debug_launch_clock, ssg_debug_clock_probe;
                             9: ssg_policy, ssg_policy_act, ssg_rollout_policy (the policy forward + action sampling of a rollout step on
                                the device: rollouts with the policy in the loop, driven from C); extended, additively and without a
                                version change: ssg_ppo_hparams, ssg_ppo_workspace_nbytes, ssg_ppo_gae, ssg_ppo_grad, ssg_ppo_adam,
                                ssg_ppo_update (GAE and the PPO update of that policy on the device); ssg_population and the ssg_pop_*
                                entry points (a population of such policies sharing every launch: batched PPO for PBT) */

typedef enum ssg_status {
    SSG_OK = 0,
    SSG_ERR_BAD_ARG = -1,
    SSG_ERR_HIP = -2,
    SSG_ERR_NOT_BOUND = -3,
    SSG_ERR_UNSUPPORTED = -4,
    SSG_ERR_NO_DEVICE = -5
} ssg_status;

/* ---- limits ---- */
#define SSG_MAX_BEAMS 16
#define SSG_MAX_GOALS 6       /* bits 0..5 of the goal mask; bit 7 = "rudder has been moved"; reference N_GOALS = 5 */
#define SSG_MAX_HULL 12       /* game_map.gen_river_poly: 10 jittered points + 2 corners, game_map.py:22-73 */
#define SSG_SHIP_VERTS 5      /* SHIP_TEMPLATE, models.py:6 */
#define SSG_MAX_HISTORY 8
#define SSG_N_TRAFFIC 3       /* ShipGame.add_default_traffic, game.py:279-286 */

/* ---- flags ---- */
#define SSG_FLAG_AUTO_RESET        0x1u /* VecEnv semantics: a done env is reset inside ssg_step and the returned
                                           observation is the reset observation (SubprocVecEnv worker behaviour,
                                           train/stable_baselines/ppo.py:123) */
#define SSG_FLAG_FIX_COLLISION_REWARD 0x2u /* off by default: the reference's determine_reward overwrites the
                                           collision reward (ship_env.py:66-77); set to make in-bounds collisions -1 */
#define SSG_FLAG_BANK_IN_GLOBAL    0x4u /* never stage the map bank in LDS (per-lane gathers from L2/HBM); forced
                                           when the bank does not fit LDS or when every env has its own slot */

#define SSG_FLAG_DYN_MEMO_OFF      0x10u /* config 4, development / measurement aid: never look a cpSpaceStep up in the memo table
                                           (see SSG_F_DYN_MEMO_STATS): every queued env walks the full narrowphase / solver chain.
                                           Results are bit for bit the same either way. */
#define SSG_FLAG_EXACT_LIDAR       0x8u /* lidar: intersect every hull plane with every beam in cpPolyShapeSegmentQuery's
                                           order of operations (one division per plane and beam, plain IEEE products and
                                           sums, no fused multiply-add) instead of the default one-division-per-beam
                                           evaluation of the same predicate.  Not bitwise the reference: the beam end comes
                                           from the angle-sum identity (~1e-13 from cos / sin of the beam's angle).  The two
                                           paths differ only for rays within rounding of a decision boundary of the query
                                           (a hull vertex, an edge's end, an origin on a plane).  Validation aid. */

/*
 * Map bank record: SSG_MAP_STRIDE doubles per map, built on the host by ssg_host_build_map().
 *   [0] nL  [1] nR                      hull plane counts (as doubles)
 *   [2..5]  left  hull AABB l,b,r,t     [6..9] right hull AABB
 *   [10..22)  goal centres x0,y0,x1,y1,...  (SSG_MAX_GOALS pairs)
 *   [22] [23] the goal nearest to the spawn point (the reset observation's goal, ship_env.py:102-108)
 *   [24 + 5*j ..)  left  plane j: v0x v0y nx ny (v0.n)       j < 12
 *   [84 + 5*j ..)  right plane j
 * v0/n are Chipmunk's splitting planes of the hulled polygon (pm.Poly, models.py:180) and v0.n the plane offset
 * cpPolyShapeSegmentQuery uses; its per-plane edge extents dtMin = cross(n, v[j-1]) and dtMax = cross(n, v[j]) are
 * recomputed where needed from the neighbouring plane's v0 (the same two products and one difference).
 *   [144] spare
 * 145 doubles: an ODD stride in 8-byte units, so the same field of different maps falls on different LDS banks
 * (lanes of a wave sit on different maps; an even stride made such reads 8-way bank conflicts).  A 64-map bank is
 * 74 240 bytes and fits the CU's 160 KiB of LDS beside the pose exchange and the lidar waves' buffers, for up to 12
 * beams at 256 envs per workgroup.
 */
#define SSG_MAP_STRIDE 145
#define SSG_MAP_OFF_COUNTS 0
#define SSG_MAP_OFF_AABB 2
#define SSG_MAP_OFF_GOALS 10
#define SSG_MAP_OFF_SPAWN_GOAL 22
#define SSG_MAP_OFF_PLANES 24
#define SSG_PLANE_DOUBLES 5

typedef struct ssg_config {
    uint32_t struct_size;  /* sizeof(ssg_config), checked by ssg_create */
    uint32_t flags;        /* SSG_FLAG_* */
    int32_t device_id;     /* HIP device ordinal */
    int32_t n_envs;        /* envs owned by this handle (this rank's shard) */
    int64_t env_id_base;   /* global id of local env 0: keys the action stream and default map assignment */
    /* EnvConfig / LiDAR (config.py:14-17, models.py:29) */
    int32_t n_beams;       /* 1..SSG_MAX_BEAMS; reference LiDAR default 10 */
    int32_t history;       /* EnvConfig.HISTORY_SIZE, 1..SSG_MAX_HISTORY (reference default 2); above 2 every step is its own
                              launch followed by a frame-shift kernel (the fused rollout path needs history <= 2) */
    int32_t max_steps;     /* EnvConfig.MAX_STEPS */
    int32_t n_goals;       /* N_GOALS = 5, game.py:17; <= SSG_MAX_GOALS */
    double lidar_spread_deg; /* 90 */
    double lidar_dist;       /* 100 */
    double goal_radius;      /* 5, game.py:82 */
    /* GameConfig (config.py:20-24) */
    double width, height;  /* BOUNDS */
    double dt;             /* SPEED * base_dt (game.py:27,194), computed by the host in double */
    double damping_pow_dt; /* pow(space.damping = 0.4, dt) (game.py:270; cpSpaceStep) */
    /* player ship (models.py:87-111, game.py:274-275) */
    double spawn_x, spawn_y;
    double ship_hull[2 * SSG_SHIP_VERTS];    /* CCW hull of SHIP_TEMPLATE*(w,h) in cpConvexHull order */
    double ship_normals[2 * SSG_SHIP_VERTS]; /* local splitting-plane normals of that hull */
    double ship_m_inv, ship_i_inv;           /* 1/mass, 1/cpMomentForPoly */
    double force_y;                          /* force_vector = (0,100) */
    double thrust_px0, thrust_py0;           /* point_of_thrust before the first rotate(), models.py:109 */
    int32_t rudder_step, rudder_max;         /* 5, 10 */
    /* config 4 (BASELINE configs[3]) */
    int32_t n_ships;       /* 1 (default), or 4 = the player + ShipGame.add_default_traffic() after every reset
                              (game.py:279-286): goal bodies become dynamic and Chipmunk's contact solver runs for the
                              traffic ships and goals; every step is then two launches — cpSpaceStep of the queued envs, the step
                              kernel — (no fused rollout) */
    int32_t map_ring;      /* 0 (default): envs walk through a shared bank of worlds.  R in 2..128: EVERY EPISODE GETS A BRAND-NEW
                              WORLD (R up to 128; n_envs * R * SSG_MAP_STRIDE < 2^31), as ShipGame.reset does (game.py:260-277: gen_level + gen_goal_path at every reset): the bank
                              holds n_envs * R records, env e owns records [e*R, e*R + R) as a ring, episode p of env e lives
                              in record e*R + p mod R and is drawn on the device by ssg_refill_worlds from a Philox stream keyed
                              by (seed, global env id, p).  An (auto-)reset moves the env to its next record; the library
                              refills the rings between launches (at most R-1 steps are fused into one launch, so an env can
                              never outrun its ring).  The bank is read from L2/HBM in this mode (it does not fit LDS). */
} ssg_config;

typedef struct ssg_handle ssg_handle;

/* State blob fields (struct-of-arrays, one column of n_envs_padded elements per field, lane-contiguous). */
typedef enum ssg_field {
    SSG_F_X = 0, SSG_F_Y, SSG_F_VX, SSG_F_VY, SSG_F_ANGLE, SSG_F_W, /* f64: body p, v, a, w            */
    SSG_F_CUM_REWARD,                                              /* f64: ShipEnv.cumulative_reward    */
    SSG_F_LIDAR,                                                   /* f64 x n_beams: LiDAR.vals (sticky) */
    SSG_F_RUDDER,                                                  /* i32: Ship.rudder_angle            */
    SSG_F_STEP_COUNT,                                              /* i32: ShipEnv.step_count           */
    SSG_F_MAP_ID,                                                  /* i32: bank record of this env      */
    SSG_F_GOAL_MASK,                                               /* u8 : bit g = goal g still listed  */
    SSG_F_STATS,                                                   /* i64 [256 slots][4] per handle, to be summed
                                                                      over slots: 100*sum_return, sum_length,
                                                                      n_episodes, n_goals_hit */
    SSG_F_TRAFFIC,      /* f64 x 27, n_ships == 4 only: ship k = columns 9k..9k+8: x, y, angle, vx, vy, w, v_bias.x,
                           v_bias.y, w_bias (cpBody fields of add_default_traffic's ships) */
    SSG_F_GOAL_BODIES,  /* f64 x 8*SSG_MAX_GOALS, n_ships == 4 only: goal g = columns 8g..8g+7: x, y, vx, vy, v_bias.x,
                           v_bias.y, w, w_bias (add_goal's dynamic circle bodies, game.py:77-95) */
    SSG_F_DYN_FLAGS,    /* u8, n_ships == 4 only: bit 0 unused (rounds 2-3: the player touches a traffic ship; the step kernel
                           now runs that test itself), bit 1 = bodies to be rebuilt after an in-kernel auto-reset, bit 2 = the traffic ships and
                           goal bodies are at rest (their cpSpaceStep is skipped as the identity; inspection only), bit 3 = the env
                           has an entry in the queue of the next full cpSpaceStep */
    SSG_F_EPISODES,     /* i32: episodes this env has started so far (every reset counts; in map_ring mode episode p lives in
                           bank record e*R + p mod R) */
    SSG_F_DYN_MEMO_STATS, /* i64 [256 slots][16], n_ships == 4 only, to be summed over slots: [0] cpSpaceSteps answered by the memo
                           table, [1] computed, [2] results stored, [3] / [4] cpCollide(traffic ship, bank hull) answered by the narrowphase memo / computed
                           ([5..15] unused) — inspection only.  No reference counterpart: Chipmunk steps
                           every space every time (game.py:194).  In bank mode (shared worlds, <= 64 records) the traffic ships
                           and goal bodies of thousands of envs pass through the SAME states after every reset — cpSpaceStep of
                           those bodies is a pure function of their cpBody fields, the cached arbiters and the bank record (the
                           player pushes nothing) — so the first env to step a state stores (state -> next state) in a table
                           inside the state blob and later envs in that state copy the result after comparing the COMPLETE
                           state word for word: a memoised step writes exactly the bits a computed one writes. */
    /* The cached arbiters of the config-4 space (cpSpace.cachedArbiters), n_ships == 4 only, inspection only.  One row per
       PAIR ID p, the shape pair in the canonical collide order of the dyn kernel (k, j: traffic ships 0..2, s: bank hull 0/1,
       g, h: goals 0..5):  p = 2k + s (ship k, bank s) [0, 6) | 6 + j + k - 1 (ships j < k) [6, 9) | 9 + 2g + s (goal g, bank s)
       [9, 21) | 21 + 3g + k (goal g, ship k) [21, 39) | 39 + g(g - 1)/2 + h (goals h < g) [39, 54).  The solver's list holds
       every pair that has contacts in a step, in that collide order (at most 54).  A row is meaningful only while bit p of
       the live mask is set.  The arbiters of a goal the player reached leave with it at the env's next full step. */
    SSG_F_DYN_LIVE,     /* u64: bit p = pair p has a cached arbiter */
    SSG_F_DYN_ARB_META, /* u32 x 54: pair p = column p: state (1 first contact, 2 normal, 4 cached) | age << 3 (steps since it was
                           last touched, < 3) | contact count << 5 */
    SSG_F_DYN_ARB_HASH, /* u32 x 9 (the polygon pairs p < 9): contact hash 0 | contact hash 1 << 16 (0 when one contact) */
    SSG_F_DYN_ARB_IMPULSE, /* f64 x 4*54: pair p = columns 4p..4p+3: jnAcc of contact 0, 1, jtAcc of contact 0, 1 */
    SSG_F_COUNT
} ssg_field;

/* ---------------------------------------------------------------------------------------------------
 * Lifecycle
 * ------------------------------------------------------------------------------------------------- */
int ssg_abi_version(void);
const char *ssg_strerror(int status);
const char *ssg_last_error(const ssg_handle *h);

/* Replaces: ShipEnv.__init__ + ShipGame.__init__ (ship_env.py:23-48, game.py:32-58) and the pm.Space()/Body/
 * Poly construction inside them (game.py:269-270, models.py:87-111,153-196).  Host only: no GPU work. */
int ssg_create(const ssg_config *cfg, ssg_handle **out);
/* Replaces: the garbage collection of a ShipEnv and its pm.Space (the reference never closes one explicitly:
 * ship_env.py:23-48 creates, nothing destroys).  Frees the handle only — the state blob and the bank are the caller's. */
int ssg_destroy(ssg_handle *h);

/* Fill *cfg with the reference defaults (config.py:8-24, models.py:6,29,87-110, game.py:17,82,274-275). */
int ssg_default_config(ssg_config *cfg);
/* Recompute ship_hull / ship_normals / ship_m_inv / ship_i_inv for SHIP_TEMPLATE*(width_scale,height_scale):
 * Ship.__init__ (models.py:87-100): pm.moment_for_poly on the template order, pm.Poly hull order. */
int ssg_config_set_ship(ssg_config *cfg, double width_scale, double height_scale, double mass);

/* ---------------------------------------------------------------------------------------------------
 * Memory binding (caller-owned device memory)
 * What the reference keeps inside pymunk objects — cpBody position / velocity / angle per ship (models.py:87-111), the
 * goal list and its bodies (game.py:77-95), LiDAR.vals (models.py:36), ShipEnv.step_count / cumulative_reward / states
 * (ship_env.py:171-184) — lives here as struct-of-arrays columns in ONE blob the caller allocates; these three calls have
 * no reference counterpart beyond that.
 * ------------------------------------------------------------------------------------------------- */
int ssg_state_nbytes(const ssg_handle *h, size_t *nbytes);
/* offset (bytes) of a field's first column in the blob, element size, columns per env-field. */
int ssg_state_field(const ssg_handle *h, int field, size_t *offset, int *elem_size, int *n_columns,
                    size_t *column_stride_bytes);
/* dev_state: ssg_state_nbytes() bytes of device memory, 256-byte aligned.  The blob must start out ZEROED (episode
 * counters, the config-4 queue counter and rest/arbiter columns are only ever updated, never initialised, by the step
 * kernels): either hand over zeroed memory, or call ssg_init_state, or let the first full reset after binding do it —
 * ssg_reset with dev_mask == NULL on a freshly bound blob zeroes it first. */
int ssg_bind_state(ssg_handle *h, void *dev_state);
/* Zero the whole bound state blob asynchronously on `stream` (hipMemsetAsync): episode statistics, config-4 columns and
 * all body state; follow with ssg_reset.  Replaces nothing in the reference (a fresh ShipEnv object starts empty). */
int ssg_init_state(ssg_handle *h, void *stream);
/* Replaces: gen_level + PolyEnv (game.py:60-71, models.py:153-196) and the goal list (game.py:77-95).
 * dev_bank: n_maps records of SSG_MAP_STRIDE doubles in device memory.  Installing a bank with FEWER maps than the
 * previous one re-maps every env's record index modulo the new n_maps before the next reset / step (an env keeps
 * stepping on a record that exists; callers normally reset after a bank change anyway).  Map ids handed to ssg_reset
 * are likewise taken modulo n_maps: a record index can never point outside the bank. */
int ssg_set_map_bank(ssg_handle *h, const double *dev_bank, int n_maps);

/* ---------------------------------------------------------------------------------------------------
 * The hot path
 * ------------------------------------------------------------------------------------------------- */
/* Replaces: ShipEnv.reset -> ShipGame.reset (ship_env.py:171-184, game.py:260-277).
 * dev_mask: u8[n_envs], non-zero = reset this env; NULL = all.  dev_map_ids: i32[n_envs] record to install for
 * each reset env; NULL = (env_id_base + e) mod n_maps (map_ring mode: must be NULL — the env moves to the next record of
 * its own ring; SSG_ERR_BAD_ARG otherwise).  dev_obs: f64[n_envs][history*(6+n_beams)], rows of reset
 * envs are overwritten with the reset observation. */
int ssg_reset(ssg_handle *h, const uint8_t *dev_mask, const int32_t *dev_map_ids, double *dev_obs, void *stream);

/* Replaces: ShipEnv.step (ship_env.py:136-156) = handle_discrete_action (game.py:140-153) + update: LiDAR.query
 * (models.py:39-76) + space.step = cpSpaceStep (game.py:194) with the collide_ship / collide_goal callbacks
 * (game.py:232-257) + determine_reward / __add_states / is_done (ship_env.py:62-134).
 * dev_actions i32[n_envs] in {0,1,2,3}; dev_obs f64[n_envs][D]; dev_reward f64[n_envs]; dev_done u8[n_envs] (0/1);
 * dev_flags u8[n_envs] event bits SSG_EV_* or NULL. */
int ssg_step(ssg_handle *h, const int32_t *dev_actions, double *dev_obs, double *dev_reward, uint8_t *dev_done,
             uint8_t *dev_flags /* nullable */, void *stream);

/* Replaces: one `env.step(actions)` of the reference's trainers on HOST arrays (train/stable_baselines/ppo.py:122-123: SubprocVecEnv's
 * pipe round trip per step; train/rllib/ppo.py:21-44) — the whole step of the numpy protocols in ONE call, all asynchronous on `stream`:
 * host_actions (i32[n_envs], pinned host memory) -> dev_actions, ssg_step into dev_obs / dev_reward / dev_done / dev_flags, then ONE copy
 * of the caller's packed output block [dev_block, dev_block + block_bytes) — which those four buffers are sections of — into host_block
 * (pinned host memory), and a completion event of the handle's `slot` (0..7: callers rotate host blocks so that the arrays of one step
 * stay valid while the next steps run).  ssg_wait_host(h, slot) blocks the calling thread until that step's host block is complete.
 * What ShipVecEnv.step_async / step_wait are made of: one foreign call each instead of a dozen interpreter-level stream / copy / event
 * operations (which cost more than the 14-us step at small batches). */
int ssg_step_host(ssg_handle *h, const int32_t *host_actions, int32_t *dev_actions, double *dev_obs, double *dev_reward, uint8_t *dev_done,
                  uint8_t *dev_flags /* nullable */, const void *dev_block, void *host_block, size_t block_bytes, int slot, void *stream);
/* Replaces: the blocking half of that step — SubprocVecEnv.step_wait's `remote.recv()` (train/stable_baselines/ppo.py:122-123) — for
 * the step issued into `slot`: returns when its host block is complete. */
int ssg_wait_host(ssg_handle *h, int slot);

/* Replaces: what RLlib's VectorEnv flow sees of an episode's end (train/rllib/ppo.py:21-44 over ShipEnv.step / ShipEnv.reset,
 * ship_env.py:136-156,171-184): vector_step reports the TERMINAL observation of a done env, reset_at then resets it and returns the
 * reset observation.  With SSG_FLAG_AUTO_RESET a done env is reset inside ssg_step and its row of dev_obs is the reset observation;
 * with dev_term_obs != NULL (f64[n_envs][history*(6+n_beams)], caller-owned) the step kernel ALSO stores the terminal observation
 * of every env it resets into that env's row of dev_term_obs (rows of other envs are left untouched): one step, no reset launch,
 * both observations.  ssg_step / ssg_rollout only (a trajectory rollout keeps every step in its own slot and is not served);
 * history <= 2 (SSG_ERR_UNSUPPORTED otherwise: reset the done envs with a masked ssg_reset there).  NULL switches it off. */
int ssg_set_terminal_obs(ssg_handle *h, double *dev_term_obs);

/* Per-env event bits written to dev_flags (the reference's ShipGame.colliding / goal_reached attributes that
 * tests reach through env.game.*, game.py:190-191,240,254, plus which is_done branch fired). */
#define SSG_EV_COLLIDING 0x1u
#define SSG_EV_GOAL_REACHED 0x2u
#define SSG_EV_OUT_OF_BOUNDS 0x4u
#define SSG_EV_MAX_STEPS 0x8u
#define SSG_EV_NO_GOALS_LEFT 0x10u

/* K consecutive steps, step k reading dev_actions + k*n_envs (the random-action rollout loop of
 * train/random.py:14-27, batched), enqueued on `stream` as ceil(K / SSG_ROLLOUT_STEPS_PER_LAUNCH) launches of the step
 * kernel: inside a launch the map bank stays in LDS and the body state in registers from step to step.
 * obs/reward/done/flags are overwritten by every step and the state blob is updated every step; the final contents of
 * every buffer are bit for bit those of K separate ssg_step calls.  With history > 2 or n_ships = 4 every step is its own
 * launch sequence (frame shift / the two dyn kernels before the step kernel): same results, no fusion.
 * HIP graphs: a 1-ship handle on a shared bank with history <= 2 launches with constant arguments, so ssg_step / ssg_rollout on a
 * capturing stream can be captured and replayed (on this ROCm a replay costs more than the plain launch it replaces).  Handles
 * with n_ships > 1, map_ring or history > 2 take per-call host state in their kernel arguments: ssg_step / ssg_rollout / ssg_reset
 * return SSG_ERR_UNSUPPORTED on a capturing stream instead of recording a step that every replay would repeat. */
#define SSG_ROLLOUT_STEPS_PER_LAUNCH 100 /* steps fused into one launch of the step kernel by ssg_rollout */
int ssg_rollout(ssg_handle *h, const int32_t *dev_actions_KN, int K, double *dev_obs, double *dev_reward,
                uint8_t *dev_done, uint8_t *dev_flags /* nullable */, void *stream);

/* The same K steps, with EVERY step's outputs kept: step k writes its observation rows at dev_obs + k * step_stride_envs * D
 * doubles (D = history*(6+n_beams)) and its reward / done / flags at element k * step_stride_envs of their buffers — the
 * (obs, reward, done) of every step that the reference's rollout loop consumes (train/random.py:14-27: `obs, reward, done, _ =
 * env.step(action)` inside the loop), as trajectory tensors [K][step_stride_envs][...].  step_stride_envs = n_envs gives
 * contiguous [K][n_envs] tensors; a larger stride interleaves this handle's shard into a wider [K][total_envs] layout;
 * 0 = ssg_rollout (every step rewrites the same rows).  Must be 0 or >= n_envs.  Same launches, same fusion, same results
 * per step as K ssg_step calls — a fused step's outputs just no longer overwrite the previous step's, so all of them reach
 * HBM (233 B per env-step at 8 beams, history 2) and every fused step can be checked against the oracle. */
int ssg_rollout_traj(ssg_handle *h, const int32_t *dev_actions_KN, int K, double *dev_obs, double *dev_reward,
                     uint8_t *dev_done, uint8_t *dev_flags /* nullable */, int64_t step_stride_envs, void *stream);

/* Random-action rollout driver (train/random.py:14-27 batched): fills i32[K][n_envs] with a counter-based
 * Philox4x32-10 stream keyed by (seed, step0+k, env_id_base+e), uniform on Discrete(3) (ship_env.py:19). */
int ssg_fill_actions(ssg_handle *h, uint64_t seed, uint64_t step0, int K, int32_t *dev_actions, void *stream);

/* Reset-time world generation on the device: fills dev_bank with n_maps fresh records — river
 * banks as game_map.gen_river_poly draws them (game_map.py:22-73), hulls/planes as pm.Poly derives them, goals as
 * gen_goal_path places them (game.py:300-330) — from a Philox4x32-10 stream keyed by (seed, map index).  NOT
 * seed-compatible with the reference's Mersenne-Twister draws: a separate mode for refreshing the bank without the
 * host.  dev_raw (nullable): per map 48 + 3*n_goals doubles = the raw 2x12 polygon vertices, then per goal (y, the
 * uniform draw u, the fallback x), so a test can rebuild every record on the host and compare bit for bit.
 * Call ssg_set_map_bank afterwards (or pass the already-installed bank pointer to refresh it in place).
 * width_frac in (0, 1].  THE LAW of the draws is the reference's for width_frac * width >= 6.85: a bank vertex's x is
 * the half-normal x_max - |gauss(0, 50)| cut at the strip's inner edge, which is what gen_river_poly's redrawn two-sided
 * gauss(x_max, 50) comes to as long as its 1000-try cap is out of reach (at that bound a vertex reaches the cap with
 * probability (1 - q)^999 = 1e-12, q = Phi(width_frac * width / 100) - 1/2).  BELOW that bound the device's law is NOT
 * the reference's: a device try passes with 2q, so it reaches the cap with (1 - 2q)^999 only, and a vertex kept at the
 * cap is folded (never above x_max) where the reference's is not.  Nothing is refused there. */
int ssg_generate_bank(ssg_handle *h, uint64_t seed, double width_frac, double *dev_bank, int n_maps, double *dev_raw,
                      void *stream);

/* map_ring mode (ssg_config.map_ring = R >= 2): generate every world the rings are missing — for each env the episodes
 * from the first one not yet drawn up to (current episode + R - 1) — into the bank installed with ssg_set_map_bank
 * (n_maps = n_envs * R), on the device: river banks as game_map.gen_river_poly draws them (game_map.py:22-73), hulls /
 * planes as pm.Poly derives them, goals as gen_goal_path places them (game.py:300-330), Philox4x32-10 keyed by (seed,
 * env_id_base + e, episode).  Must be called once after ssg_set_map_bank and before the first ssg_reset (it fills the
 * rings and fixes seed / width_frac for the automatic refills ssg_reset / ssg_step / ssg_rollout issue afterwards).
 * dev_raw (nullable): [n_envs * R][48 + 3*n_goals] doubles, row e*R + slot receives the raw polygons and goal draws of the
 * world generated into that slot by THIS call (rows of slots not regenerated are left untouched), so a test can rebuild
 * the records on the host and compare bit for bit.  NOT seed-compatible with the reference's Mersenne-Twister draws.
 * width_frac in (0, 1]; as for ssg_generate_bank, below width_frac * width = 6.85 (where a vertex reaches the reference's
 * 1000-try cap with probability above 1e-12) the device's law of the bank vertices is NOT the reference's. */
int ssg_refill_worlds(ssg_handle *h, uint64_t seed, double width_frac, double *dev_raw, void *stream);

/* Config 4 only; no reference counterpart (writing `ship.body.position` on a pymunk body, game.py:117-131, needs no
 * announcement there).  The traffic ships and goal bodies of an env whose space has reached a fixed point of cpSpaceStep are
 * not stepped again until something changes (SSG_F_DYN_FLAGS bit 2), and WHICH envs the next step's dyn kernels visit is
 * decided at the end of each step from the player state the step kernel holds in registers.  The library sees resets, goal
 * removals and bank changes itself; a caller that WRITES ANY state column of a config-4 handle between two steps — the
 * SSG_F_TRAFFIC / SSG_F_GOAL_BODIES columns, but also the player's own SSG_F_X .. SSG_F_W, SSG_F_GOAL_MASK, SSG_F_STEP_COUNT
 * or SSG_F_MAP_ID (scenario set-up, curriculum placement, tests) — tells it with this call: the queue of the next step is then
 * rebuilt from the columns, and the ships' rotation columns (what collide_ship's player x traffic test in the step kernel turns
 * their hulls with) are recomputed from the angles.
 * dev_mask: u8[n_envs], non-zero = also clear the env's rest bit and refresh its row-major shadow; NULL = all envs.  (The rotation
 * columns are recomputed for every env whatever the mask says.)
 * The caller-owned state blob also holds the queue of the next full cpSpaceStep, whose live counter set is named by the HANDLE:
 * a blob that is copied, restored in place or bound to another handle between two steps must be followed by ssg_bind_state or
 * ssg_dyn_invalidate(h, NULL, ...) — both make the next step rebuild the queue from the per-env flags AND start the memo tables
 * inside the blob empty (a memo key names the bank RECORD, not the bank's contents: entries another handle stored over another bank
 * must never answer for this one). */
int ssg_dyn_invalidate(ssg_handle *h, const uint8_t *dev_mask, void *stream);

/* Replaces: ShipGame.render + ShipGame.get_screen (game.py:133-138,197-229) for ONE env: an RGB frame of `width` x
 * `height` pixels covering the env's bounds, laid out like pygame.surfarray.array3d ([x][y][3], screen y down).
 * flags bit 0 = GameConfig.DEBUG drawing (shapes in their colours + one circle per lidar beam end); the yellow
 * player marker is always drawn.  A beam whose origin lies inside a bank hull (or on its boundary) is drawn as a hit at
 * the beam's far end, as cpShapeSegmentQuery reports it.  Arguments are checked before the handle's bindings: a NULL
 * handle or buffer, an env_index outside 0 .. n_envs-1 or a width / height outside 1 .. 8192 is SSG_ERR_BAD_ARG on any
 * handle, then an unbound handle is SSG_ERR_NOT_BOUND.  Debugging / video aid (`metadata['render.modes']` lists 'rgb_array',
 * ship_env.py:18); not a hot path. */
int ssg_render(ssg_handle *h, int env_index, int width, int height, uint8_t *dev_rgb, uint32_t flags, void *stream);

/* Replaces: the env.render() of every step of the evaluation loop (train/rllib/rollout.py:18-19) over ShipGame.render + get_screen
 * (game.py:133-138,197-229), for `count` envs in ONE launch: a grid over (128-pixel column blocks, rows, frame).  dev_env_ids is a
 * DEVICE array int32 [count]; frame i (dev_rgb + i * width * height * 3, laid out [width][height][3]) is bit for bit what
 * ssg_render(h, dev_env_ids[i], width, height, ..., flags) writes: both kernels call the same per-block beam set-up and the same
 * per-pixel function.  The ids live on the device and the host cannot see them: a frame whose id is outside 0 .. n_envs-1 is skipped
 * by the kernel and left UNWRITTEN (the other frames are drawn).  Ids may repeat.  The checks of ssg_render in its order — NULL
 * handle, NULL buffers or a width / height outside 1 .. 8192 — plus count outside 1 .. SSG_RENDER_MAX_ENVS and
 * count * width * height * 3 above 2^31: SSG_ERR_BAD_ARG on any handle; then an unbound handle is SSG_ERR_NOT_BOUND. */
#define SSG_RENDER_MAX_ENVS 4096
int ssg_render_envs(ssg_handle *h, const int32_t *dev_env_ids, int count, int width, int height, uint8_t *dev_rgb, uint32_t flags,
                    void *stream);

/* Measurement aid (config 4; no reference counterpart): with enable != 0, every following ssg_step / ssg_rollout* call brackets the
 * two launches of each step — the full cpSpaceStep of the queued envs, the step kernel — with HIP events on the caller's stream and
 * waits for its own work at the end of the call.  Returns the averages (microseconds per step) and the number of steps accumulated
 * since the previous call, then starts over.  How bench.py splits a config-4 step into its two kernels. */
int ssg_debug_kernel_times(ssg_handle *h, int enable, double *dyn_step_us, double *step_kernel_us, uint64_t *steps);

/* Inspection aid (config 4; no reference counterpart): launches of the full cpSpaceStep so far, and how many of them had to
 * rebuild their queue from the per-env flags first (a pass over every env: after a full ssg_reset, a bank change,
 * ssg_dyn_invalidate, a second masked ssg_reset between two steps; NOT after one masked ssg_reset between two steps, whose envs
 * join the queue the step kernel left). */
int ssg_debug_dyn_counters(const ssg_handle *h, uint64_t *full_steps, uint64_t *queue_rebuilds);

/* Inspection aid (no reference counterpart): how ssg_set_map_bank laid the step kernel out for this handle — envs per workgroup (256, 128 or 64),
 * whether the bank is staged in LDS (0 = gathered from L2 / HBM) and the dynamic LDS bytes per workgroup.  The bank is staged when it
 * fits the CU's 160 KiB of LDS beside the exchange and lidar buffers at the workgroup size preferred for the env count; otherwise it is
 * staged beside a smaller workgroup only if gathering would not allow a larger one. */
int ssg_debug_launch_geometry(const ssg_handle *h, int *envs_per_workgroup, int *bank_in_lds, size_t *lds_bytes);

/* Measurement aid (no reference counterpart): coalesced 8-byte-per-lane device copy of n_doubles doubles, the
 * step kernel's access width, for calibrating rocprofv3's FETCH_SIZE / WRITE_SIZE on a known byte count. */
int ssg_debug_copy8(const double *dev_src, double *dev_dst, size_t n_doubles, void *stream);

/* Measurement aid (no reference counterpart): the shader clock DURING the step kernel's launches.  With dev_buf != NULL (two u64 of
 * device memory), the first wave of workgroup 0 of every following step-kernel launch stores, when it ends, dev_buf[0] = shader-clock
 * cycles (s_memtime) and dev_buf[1] = ticks of the constant 100 MHz reference counter (s_memrealtime) that passed since it started:
 * clock = 100 MHz x cycles / ticks, measured inside the timed launch itself with nothing launched around it.  NULL switches it off
 * (the default; the kernel then executes two scalar counter reads per wave and one untaken branch).  How bench.py reports
 * `repeats_shader_clock_ghz`. */
int ssg_debug_launch_clock(ssg_handle *h, uint64_t *dev_buf);

/* Measurement aid (no reference counterpart): the shader clock under an FP64 VALU load.  n_blocks workgroups of 256 lanes run
 * `iters` rounds of eight independent double mul + add chains; dev_out[2*b] = shader-clock cycles (s_memtime) and dev_out[2*b+1] =
 * ticks of the constant 100 MHz reference counter (s_memrealtime) that workgroup b saw pass meanwhile: clock = 100 MHz x cycles /
 * ticks.  (A probe wide enough to load every CU pulls the chip into its power-limited clocks and slows whatever is timed right
 * after it: bench.py uses ssg_debug_launch_clock for the timed repeats instead.) */
int ssg_debug_clock_probe(uint64_t *dev_out, int n_blocks, int iters, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The policy in the loop (ABI 9)
 * An MLP actor-critic evaluated on the device for every env of a handle, with the action sampled there too: what the reference's
 * runner does around each env.step (train/stable_baselines/ppo.py:84-100) and what train/ppo_torch.py does with a dozen PyTorch
 * kernels per rollout step.  f32 parameters, f64 observations in.
 *
 * Packed parameter layout (dev_params, f32, 4-byte aligned, no padding), with D = obs_dim, H = hidden, A = n_actions; W is nn.Linear's
 * own [out][in] row-major order, so the buffer is torch.cat([p.flatten() for p in net.parameters()]) of
 * Sequential(Linear(D, H), act[, Linear(H, H), act]) followed by the heads Linear(H, A) and Linear(H, 1):
 *   [0 .. H*D)                  W0  [H][D]
 *   [H*D .. H*D + H)            b0  [H]
 *   then, with n_hidden_layers = 2:
 *   [o1 .. o1 + H*H)            W1  [H][H]          o1 = H*D + H
 *   [o1 + H*H .. o1 + H*H + H)  b1  [H]
 *   then, at oh = H*D + H (+ H*H + H with 2 layers):
 *   [oh .. oh + A*H)            Wpi [A][H]
 *   [oh + A*H .. + A)           bpi [A]
 *   [oh + A*H + A .. + H)       Wv  [1][H]
 *   [oh + A*H + A + H]          bv  [1]
 *   total: H*D + H + (n_hidden_layers - 1)*(H*H + H) + A*H + A + H + 1 floats.
 *
 * Separate value network (activation | SSG_POLICY_SEPARATE_VALUE): Stable-Baselines' MlpPolicy (net_arch [dict(vf=[64, 64], pi=[64, 64])],
 * train/stable_baselines/ppo.py) and RLlib's default vf_share_layers = False (train/rllib/pbt.py).  Two towers of the same hidden and
 * n_hidden_layers, one ending in the logits and one in the value; the buffer is torch.cat([p.flatten() ...]) of a module that declares
 * pi_body, pi, vf_body, v in that order.  With T = H*D + H + (n_hidden_layers - 1)*(H*H + H) floats per tower:
 *   [0 .. T)                    pi tower: W0 [H][D], b0 [H] [, W1 [H][H], b1 [H]]
 *   [T .. T + A*H + A)          pi head:  Wpi [A][H], bpi [A]
 *   [ov .. ov + T)              vf tower: V0 [H][D], c0 [H] [, V1 [H][H], c1 [H]]      ov = T + A*H + A
 *   [ov + T .. ov + T + H + 1)  vf head:  Wv [1][H], bv [1]
 *   total: 2*T + A*H + A + H + 1 floats.
 * Both towers start from the same normalised row x; the logits depend on the pi tower and pi head alone, the value on the vf tower and
 * vf head alone, each output still one k-ordered fmaf chain from its bias (a separate policy whose vf tower holds its pi tower's numbers
 * gives bit for bit the outputs of the shared policy over that one body).  A launch runs only the tower it needs: the value-only
 * forward (dev_last_value of ssg_rollout_policy / ssg_pop_rollout) skips the pi tower, ssg_ppo_dist / ssg_pop_dist skip the vf tower.
 * In the gradient, vf_coef scales the vf tower's and vf head's entries only and the policy, entropy and KL terms reach the pi tower's and
 * pi head's entries only.  Out of scope: hidden above SSG_POLICY_MAX_HIDDEN (RLlib's 256), towers of different width or depth,
 * partially shared layers.
 * Forward, per env e: x[d] = (float)(obs[e][d] / obs_scale[d]) (f64 division, then one rounding to f32); every dense output is an
 * fmaf chain from its bias over k = 0, 1, ... in order, followed by tanh / ReLU on the hidden layers; logits = the pi head, value = the
 * v head.  Sampling (f32): m = max(logits), lse = m + log(sum exp(l - m)), logp_all = l - lse, cdf = cumsum(exp(logp_all)),
 * act = #{j < A-1 : u > cdf[j]}, logp = logp_all[act]; while that action is j >= 1 with a logit of -inf (a masked action: the f32
 * cdf in front of it may stop short of 1 - 2^-24) act = j - 1.  So u = 0 gives action 0 whatever its probability, a NaN or +inf
 * logit gives action 0 with logp NaN, and a -inf logit at j >= 1 is never drawn.  An env's outputs depend on its own observation
 * row, the parameters and its own u only (bitwise: not on n_envs, sharding or the launch that computed them).
 * ------------------------------------------------------------------------------------------------- */
#define SSG_POLICY_MAX_HIDDEN 128
#define SSG_POLICY_TANH 0
#define SSG_POLICY_RELU 1
#define SSG_POLICY_SEPARATE_VALUE 0x100 /* or-ed into `activation`: separate pi / vf towers (layout above) */
typedef struct ssg_policy {
    uint32_t struct_size;        /* sizeof(ssg_policy) */
    int32_t obs_dim;             /* == history*(6+n_beams) of the handle */
    int32_t hidden;              /* 16..SSG_POLICY_MAX_HIDDEN, multiple of 16 */
    int32_t n_hidden_layers;     /* 1 or 2 */
    int32_t n_actions;           /* 2..4 (ssg_step accepts actions 0..3; the reference's action space is Discrete(3), ship_env.py:19) */
    int32_t activation;          /* low byte: SSG_POLICY_TANH or SSG_POLICY_RELU; bit SSG_POLICY_SEPARATE_VALUE; any other bit is refused */
    const float *dev_params;     /* packed f32, layout above */
    const double *dev_obs_scale; /* f64[obs_dim]: x = (float)(obs / scale) */
} ssg_policy;

/* Replaces: the policy half of one rollout step of the reference's runner inside model.learn (train/stable_baselines/ppo.py:84-100:
 * one policy forward + action sampling per env.step over the SubprocVecEnv of :122-123).  For every env e of the handle, on the
 * observation rows dev_obs (f64[n_envs][D]): dev_actions[e] (i32, ready for ssg_step), dev_logp[e], dev_value[e] (f32) and, with
 * dev_x != NULL, the normalised row dev_x[e][0..D) (f32).  u = dev_uniform[e] (f32[n_envs]) when given; otherwise Philox4x32-10 with
 * counter (env_lo, env_hi, step_lo, step_hi) over the GLOBAL env id env_id_base + e and key = seed (ssg_fill_actions' stream), output
 * word 1: u = (w1 >> 8) * 2^-24.  One launch on `stream`.  SSG_ERR_BAD_ARG (nothing launched) for a bad policy record or a NULL
 * required pointer. */
int ssg_policy_act(ssg_handle *h, const ssg_policy *pol, const double *dev_obs, const float *dev_uniform /* nullable */, uint64_t seed,
                   int64_t step, int32_t *dev_actions, float *dev_logp, float *dev_value, float *dev_x /* nullable */, void *stream);

/* Replaces: the whole rollout loop of that runner (train/stable_baselines/ppo.py:84-100, one policy forward + env.step per step over
 * the SubprocVecEnv of :122-123), K steps enqueued from C on `stream`: step k = ssg_policy_act for step step0 + k (uniforms row k of
 * dev_uniform_KN, or Philox as above) writing its row of act / logp / value / x, then ssg_step with that row of actions, which rewrites
 * dev_obs in place and writes its row of reward / done / flags.  Row k of every [K][...] buffer starts step_stride_envs envs after row
 * k-1 (>= n_envs, as in ssg_rollout_traj).  dev_last_value (nullable): the value of the observation after step K-1 (the bootstrap
 * value of PPO's GAE), one more value-only forward.  Every handle ssg_step serves is served (history 1..8, n_ships = 4, map_ring), with
 * the same launches ssg_step issues.  SSG_ERR_BAD_ARG (nothing launched) for a bad policy record, NULL required pointers, K < 1 or a
 * stride < n_envs.  With a time-out record bound (ssg_set_timeout_boot, below) the loop also keeps every step's terminal observations
 * and ends with one more launch, ssg_timeout_values; it then needs dev_flags_KN and refuses a capturing stream. */
int ssg_rollout_policy(ssg_handle *h, const ssg_policy *pol, int K, const float *dev_uniform_KN /* nullable */, uint64_t seed,
                       int64_t step0, double *dev_obs, int32_t *dev_act_KN, float *dev_logp_KN, float *dev_value_KN,
                       float *dev_x_KND /* nullable */, double *dev_reward_KN, uint8_t *dev_done_KN, uint8_t *dev_flags_KN /* nullable */,
                       float *dev_last_value /* nullable */, int64_t step_stride_envs, void *stream);

/* Replaces: the deterministic action of a trained policy — Stable-Baselines' model.predict(obs, deterministic=True), and the
 * agent.compute_action of the reference's evaluation script (train/rllib/rollout.py:15) run without exploration.  ssg_policy_act's
 * forward, then instead of a draw: dev_actions[e] = the smallest j < n_actions whose logit is the maximum, dev_logp[e] = that logit
 * - lse (the entry ssg_ppo_dist writes for it, bit for bit).  No uniform is read and no Philox round is run, so there is no seed or
 * step; dev_value and dev_x are bit for bit what ssg_policy_act writes for the same observations.  One launch.  Validates and refuses
 * as ssg_policy_act does. */
int ssg_policy_act_greedy(ssg_handle *h, const ssg_policy *pol, const double *dev_obs, int32_t *dev_actions, float *dev_logp,
                          float *dev_value, float *dev_x /* nullable */, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The PPO update on the device (additions to ABI 9)
 * What the reference's PPO2 does after every rollout inside model.learn (train/stable_baselines/ppo.py:90), and what
 * train/ppo_torch.py does in eager PyTorch: GAE over the rollout buffers of ssg_rollout_policy, the advantage mean / unbiased std,
 * then epochs x minibatches of {forward, clipped PPO loss, backward, Adam} on the packed parameters of an ssg_policy.
 *
 * Samples.  A rollout of K steps x N envs is K*N samples in [K][N] order: sample i = t*N + e.  The gradient entry points read
 * x f32 [K*N][obs_dim] (the normalised observations ssg_rollout_policy writes), act i32, logp f32 (of the acting policy), and
 * adv / ret f32 from ssg_ppo_gae, each [K*N], through a minibatch of int64 sample indices.
 *
 * Loss, per minibatch of M samples (p = softmax(logits), r = exp(log p[act] - logp_old), A = (adv - mean) / (std + adv_eps) with the
 * mean / unbiased std that ssg_ppo_gae left in the workspace):
 *   loss = -mean(min(r*A, clamp(r, 1-clip, 1+clip)*A)) + vf_coef*mean((v - ret)^2) - ent_coef*mean(entropy(p))
 * Its gradient follows autograd's conventions: min passes half the gradient to each side on a tie, clamp passes it inside
 * [1-clip, 1+clip] inclusive, tanh' = 1 - y*y, ReLU'(0) = 0.  Sums over samples run in a fixed order (per workgroup tile, then the
 * workgroups' partials; the bias sums and the partials as pairwise trees): a gradient is bitwise reproducible for a given M.  No
 * floating-point atomics.
 *
 * Adam: torch.optim.Adam's default (foreach) formula, step t = 1, 2, ...:  m = lerp(m, g, 1-beta1);  v = beta2*v + (1-beta2)*g*g;
 *   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  lerp is torch's, with both of its branches (w = 1-beta1
 *   in f32):  m + w*(g - m) when |w| < 0.5;  g - (g - m)*(1 - w) otherwise (beta1 <= 0.5; 1 - w formed in f32), so beta1 = 0 gives m = g.  dev_adam_mv: f32 [2*P] (m, then v; zero before step 1),
 * P = the packed length.  The Adam entry points write pol->dev_params in place: the next ssg_rollout_policy sees the new weights.
 *
 * Workspace: caller-owned device memory of ssg_ppo_workspace_nbytes bytes (256-byte aligned), shared by the calls of one update:
 * ssg_ppo_gae leaves the advantage statistics in it, which the gradient entry points read on the device (no host round trip).
 * ------------------------------------------------------------------------------------------------- */
typedef struct ssg_ppo_hparams {
    uint32_t struct_size; /* sizeof(ssg_ppo_hparams) */
    double gamma;         /* GAE discount (rounded to f32 where the reference trainer multiplies a tensor by it) */
    double lam;           /* GAE lambda (gamma*lam formed in double, then rounded to f32) */
    double clip;          /* PPO clip range, > 0 */
    double vf_coef;       /* value-loss coefficient (train/ppo_torch.py: 0.5) */
    double ent_coef;      /* entropy coefficient (0.01) */
    double lr;            /* Adam learning rate (3e-4) */
    double beta1, beta2;  /* Adam betas (0.9, 0.999) */
    double eps;           /* Adam eps (1e-8) */
    double adv_eps;       /* advantage normalisation: (adv - mean) / (std + adv_eps) (1e-8) */
} ssg_ppo_hparams;

/* Replaces nothing (memory binding): the workspace size for a policy shaped like *pol, rollouts of up to n_samples = K*N samples
 * and minibatches of up to max_minibatch samples.  SSG_ERR_BAD_ARG for a bad record or sizes < 1. */
int ssg_ppo_workspace_nbytes(const ssg_policy *pol, int64_t n_samples, int64_t max_minibatch, size_t *nbytes);

/* Replaces: the advantage / return computation of PPO2's runner before the update behind model.learn
 * (train/stable_baselines/ppo.py:90; train/ppo_torch.py's GAE loop).  One lane per env walks t = K-1 .. 0 with exactly the
 * reference trainer's f32 operations: nonterm = 1 - done; delta = (rew + (gamma*nxt)*nonterm) - val;
 * adv = delta + (gamma*lam)*nonterm*adv; ret = adv + val; nxt = val (nxt starts at dev_last_value).  Rows of every [K][N] buffer are
 * N apart.  Also leaves mean(adv) and std(adv) (unbiased) in the workspace.  Two launches on `stream`.  SSG_ERR_BAD_ARG (nothing
 * launched) for NULL pointers, K < 1, N < 1, K*N < 2 or a workspace too small. */
int ssg_ppo_gae(ssg_handle *h, const ssg_ppo_hparams *hp, int K, int N, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                const float *dev_value_KN, const float *dev_last_value, float *dev_adv_KN, float *dev_ret_KN, void *dev_workspace,
                size_t workspace_nbytes, void *stream);

/* Replaces: one minibatch of PPO2's update behind model.learn (train/stable_baselines/ppo.py:90) without the optimiser step: the
 * gradient of the loss above over the samples dev_idx[0 .. M) (int64, each in [0, n_samples)) of a rollout of n_samples, written to
 * dev_grad (f32 [P], the packed layout of ssg_policy).  dev_stats (nullable): f32[4] = the minibatch means of the pg loss, (v - ret)^2,
 * the entropy and the clip fraction (|r - 1| > clip).  Needs ssg_ppo_gae's statistics in the workspace.  Two launches on `stream`.
 * SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers, M < 1 or a workspace too small. */
int ssg_ppo_grad(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, int64_t n_samples, const float *dev_x,
                 const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_idx,
                 int64_t M, float *dev_grad, float *dev_stats /* nullable */, void *dev_workspace, size_t workspace_nbytes, void *stream);

/* Replaces: the optimiser step of that update (PPO2's Adam, train/stable_baselines/ppo.py:90; torch.optim.Adam.step in
 * train/ppo_torch.py): Adam step `step` (>= 1) with the gradient dev_grad (f32 [P]) on pol->dev_params, moments in dev_adam_mv.
 * One launch on `stream`.  SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers or step < 1. */
int ssg_ppo_adam(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const float *dev_grad, float *dev_adam_mv,
                 int64_t step, void *stream);

/* Replaces: the whole update behind model.learn (train/stable_baselines/ppo.py:90: noptepochs x nminibatches of gradient + Adam),
 * enqueued from C on `stream`: for epoch e and minibatch b, the samples dev_perm[e*n_samples + b*C .. + C) (C = ceil(n_samples /
 * minibatches), the last chunk shorter: torch.chunk's split, so as many chunks as it makes), then {gradient, Adam step step0 + 1 + j}
 * for the j-th minibatch, two launches each.  dev_stats (nullable): f32 [epochs*chunks][4], ssg_ppo_grad's stats per minibatch.
 * Needs ssg_ppo_gae's statistics in the workspace.  SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers,
 * epochs < 1, minibatches < 1, step0 < 0 or a workspace too small. */
int ssg_ppo_update(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, int64_t n_samples, const float *dev_x,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_perm,
                   int epochs, int minibatches, float *dev_adam_mv, int64_t step0, float *dev_stats /* nullable */,
                   void *dev_workspace, size_t workspace_nbytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The extended PPO update (additions to ABI 9): value clipping, a KL penalty, gradient-norm clipping
 * What the reference trainers' own PPO adds to the loss above.  train/stable_baselines/ppo.py builds PPO2 with its defaults: the value
 * loss clipped around the rollout's value prediction (cliprange) and the gradients through clip_by_global_norm(0.5);
 * train/rllib/pbt.py:55-62 sets kl_coeff = 1.0: RLlib's PPO adds kl_coeff * KL(old || new), adapts the coefficient after every update
 * against kl_target and clips the value loss (vf_clip_param).  Every term is opt-in; with all of them off the _ext entry points compute
 * bit for bit what the plain ones compute.
 *
 * Loss, per minibatch of M samples, with the symbols above (v_old = the rollout's value, logp_old = the acting policy's whole
 * log-distribution from ssg_ppo_dist, p_old = exp(logp_old)):
 *   loss = pg + vf_coef*mean(VL) - ent_coef*mean(entropy(p)) + kl_coef*mean(KL)
 *   KL = sum_{j<A} p_old[j] * (logp_old[j] - logp[j])
 *   VL = (v - ret)^2                                                              when vf_clip <= 0
 *      = max((v - ret)^2, (v_old + clamp(v - v_old, -vf_clip, vf_clip) - ret)^2)   otherwise
 * (PPO2's factor 0.5 on the value loss is the caller's vf_coef.)  The gradient follows autograd: max passes the gradient to the larger
 * side and half to each on a tie, clamp passes it inside [-vf_clip, vf_clip] inclusive, and the KL term's gradient with respect to
 * logit j is p[j]*sum(p_old) - p_old[j].  A KL coefficient of 0 is "no KL term" (mean(KL) is then reported as 0).
 *
 * Gradient-norm clipping (max_grad_norm > 0): a minibatch takes three launches instead of two — the gradient kernel; the slot
 * reduction into a gradient vector in the workspace plus per-workgroup sums of squares (f64, a fixed tree); a launch in which every
 * workgroup adds those partials in index order and forms in f32 norm = (float)sqrt(sum), coef = min(1, max_grad_norm / (norm + 1e-6f))
 * (torch.nn.utils.clip_grad_norm_), then Adam on g * coef.
 *
 * The coefficient's adaptation (kl_target > 0; RLlib's update_kl): the last launch of an _ext update takes the f32 mean of mean(KL)
 * over the last epoch's minibatches (a running f32 sum in chunk order, kept in the workspace, divided by the number of chunks) and
 * multiplies *dev_kl_coef by 1.5 when that mean is above 2*kl_target, by 0.5 when it is below 0.5*kl_target.  Both inequalities
 * are strict, in f32: a mean of exactly 2*kl_target or 0.5*kl_target leaves the coefficient alone.  The divisor is the number of
 * chunks MADE (ceil(n / ceil(n / minibatches)), which can be fewer than minibatches), and the sum restarts on every epoch's first
 * chunk, so neither an earlier epoch nor an earlier call enters.  On per-member schedules (ssg_pop_update_sched) member m's mean is
 * over ITS last epoch's chunks_m minibatches, however many launches ago that epoch ended.  A kl_target <= 0 keeps the coefficient,
 * whatever the sum holds; the sum is kept whether or not dev_stats is given.
 *
 * Stats rows of the _ext entry points are f32[8]: [0..3] as above with [1] = mean(VL), [4] mean(KL), [5] the global gradient norm
 * before clipping (0 when max_grad_norm is off), [6] the KL coefficient the minibatch used, [7] 0.  No floating-point atomics; a
 * gradient stays bitwise reproducible for a given M.  The workspace is ssg_ppo_workspace_nbytes' / ssg_pop_workspace_nbytes', which
 * cover the _ext calls.
 * ------------------------------------------------------------------------------------------------- */
typedef struct ssg_ppo_ext {
    uint32_t struct_size;       /* sizeof(ssg_ppo_ext) */
    double vf_clip;             /* value clip range; <= 0 = off */
    double max_grad_norm;       /* global gradient-norm clip; <= 0 = off */
    double kl_target;           /* <= 0 = the coefficient is never adapted */
    float *dev_kl_coef;         /* f32[1] on the device; NULL = no KL term */
    const float *dev_logp_all;  /* f32 [n_samples][4] (ssg_ppo_dist); required when dev_kl_coef is given */
    const float *dev_value_old; /* f32 [n_samples] (the rollout's dev_value_KN); required when vf_clip > 0 */
} ssg_ppo_ext;

/* Replaces: the old policy's action distribution that RLlib's PPO keeps in its sample batch for the KL term (train/rllib/pbt.py:55-62,
 * kl_coeff) — the rollout stores only logp[act].  The policy forward of ssg_policy_act over the stored normalised rows dev_x (f32
 * [n_samples][obs_dim], what ssg_rollout_policy wrote): dev_logp_all[i][j] = logit_j - lse for j < n_actions, 0 for the columns up to 4.
 * The same device code as the acting forward: called with the pre-update parameters, dev_logp_all[i][act[i]] is the rollout's logp[i]
 * bit for bit.  One launch.  SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers or n_samples outside 1..2^31-1. */
int ssg_ppo_dist(ssg_handle *h, const ssg_policy *pol, int64_t n_samples, const float *dev_x, float *dev_logp_all, void *stream);

/* Replaces: one minibatch of the reference trainers' update without the optimiser step, with their loss terms
 * (train/stable_baselines/ppo.py:90; train/rllib/pbt.py:47-74).  ssg_ppo_grad with the extended loss; dev_grad is the UNCLIPPED
 * gradient, dev_stats (nullable) f32[8] with the norm in [5] when max_grad_norm > 0 (three launches then, two otherwise).  The
 * coefficient is not adapted.  Refusals as ssg_ppo_grad, plus a bad ssg_ppo_ext record or a missing pointer that a switched-on term
 * needs: SSG_ERR_BAD_ARG, nothing launched. */
int ssg_ppo_grad_ext(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples,
                     const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                     const int64_t *dev_idx, int64_t M, float *dev_grad, float *dev_stats /* nullable */, void *dev_workspace,
                     size_t workspace_nbytes, void *stream);

/* Replaces: the whole update of those trainers (PPO2's noptepochs x nminibatches with clipped value loss and clip_by_global_norm,
 * train/stable_baselines/ppo.py:90; RLlib's SGD phase with the KL penalty and update_kl, train/rllib/pbt.py:47-74).  ssg_ppo_update
 * with the extended loss: per minibatch two launches, three with max_grad_norm > 0, and with kl_target > 0 and a coefficient one
 * more launch at the end (the adaptation).  dev_stats (nullable): f32 [epochs*chunks][8].  Refusals as ssg_ppo_update and
 * ssg_ppo_grad_ext. */
int ssg_ppo_update_ext(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples,
                       const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                       const int64_t *dev_perm, int epochs, int minibatches, float *dev_adam_mv, int64_t step0,
                       float *dev_stats /* nullable */, void *dev_workspace, size_t workspace_nbytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * A population of policies on one handle (additions to ABI 9)
 * Both reference trainers train populations: train/rllib/pbt.py:29-74 runs 120 PPO trials under PopulationBasedTraining,
 * train/stable_baselines/ppo.py:118-137 three PPO2 models, one per learning rate.  Here P members share every launch of the rollout,
 * of GAE and of the update, and each member's results are bit for bit what the single-policy entry points above compute for that
 * member alone (the same device code behind a member dimension of the grid).
 *
 * Members.  All members share one architecture and one observation scale; dev_params is f32 [P][L] (L = the packed length of
 * ssg_policy), and row m is a valid packed buffer of its own: an ssg_policy with dev_params = row m is member m.  The handle's envs
 * are split into P equal contiguous slices by local env index: member m owns envs [m*n, (m+1)*n), n = n_envs / P (n_envs % P != 0 is
 * SSG_ERR_BAD_ARG; n itself is unconstrained: every member has its own tail workgroup).  Env e runs under member e / n; its Philox
 * counter stays the global env id env_id_base + e.
 *
 * Samples.  The rollout buffers are the [K][N] buffers of ssg_rollout_policy, N = n_envs.  Member m's sample i = t*n + e (e < n) is
 * row t*N + m*n + e of them; dev_perm is int64 [P][epochs][K*n] of such member-local indices.
 *
 * Hyper-parameters are per member (a host array of P ssg_ppo_hparams); epochs and minibatches are common to the population in
 * ssg_pop_update / ssg_pop_update_ext and per member in ssg_pop_update_sched (below).  The f32
 * constants the kernels use (1 -+ clip, the coefficients, gamma, gamma*lam, adv_eps, and per Adam step 1-beta1, beta2, 1-beta2,
 * sqrt(1-beta2^t), eps, -lr/(1-beta1^t)) are derived on the host, in double, exactly as the single-policy entry points derive them, by
 * ssg_pop_pack_hparams into a caller buffer of SSG_POP_TABLE_FLOATS floats; the caller uploads it and passes the device copy
 * (dev_table) to ssg_pop_gae / ssg_pop_update.  (The library owns no device memory; the host arrays are free once a call returns.)
 *
 * Workspace: ssg_pop_workspace_nbytes bytes, 256-byte aligned; ssg_pop_gae leaves f32 [P][4] advantage statistics (mean, std + adv_eps,
 * its inverse, 0) at its start, per member over that member's K*n samples, which ssg_pop_update reads.  dev_adam_mv: f32 [P][2L].
 * The extended loss terms are per member too (ssg_pop_update_ext below), and so may the epochs and the minibatch count be
 * (ssg_pop_update_sched), and the batch size (train_batch_size) as a member's share of the handle's envs: unequal slices,
 * ssg_pop_set_slices below.  PPO2's per-minibatch advantage normalisation is a mode of the handle (ssg_ppo_set_adv_norm
 * below), common to the members.  Out of scope: unequal rollout lengths, populations spanning handles or GPUs, per-member architectures.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_POP_MAX_MEMBERS 256
#define SSG_POP_TABLE_FLOATS(n_members, n_steps) ((size_t)(n_members) * 8u * (size_t)(1 + (n_steps)))
typedef struct ssg_population {
    uint32_t struct_size;        /* sizeof(ssg_population) */
    int32_t n_members;           /* P: 1..SSG_POP_MAX_MEMBERS, a divisor of the handle's n_envs (or the P of ssg_pop_set_slices) */
    int32_t obs_dim;             /* the shape, as in ssg_policy */
    int32_t hidden;
    int32_t n_hidden_layers;
    int32_t n_actions;
    int32_t activation;          /* ssg_policy's encoding, SSG_POLICY_SEPARATE_VALUE included */
    int32_t reserved;            /* 0 */
    float *dev_params;           /* f32 [P][L]: row m = member m's packed parameters */
    const double *dev_obs_scale; /* f64[obs_dim], common to the population */
} ssg_population;

/* Replaces: the policy half of one rollout step of EVERY trial of the reference's population (train/rllib/pbt.py:47-74: 120 PPO trials,
 * each with its own sampler; train/stable_baselines/ppo.py:84-100 per model).  ssg_policy_act with env e evaluated under the parameters
 * of member e / n: same buffers, same uniforms / Philox keying, ONE launch for the whole population.  SSG_ERR_BAD_ARG (nothing
 * launched) for a bad record, n_members out of range or not a divisor of n_envs, or a NULL required pointer. */
int ssg_pop_act(ssg_handle *h, const ssg_population *pop, const double *dev_obs, const float *dev_uniform /* nullable */, uint64_t seed,
                int64_t step, int32_t *dev_actions, float *dev_logp, float *dev_value, float *dev_x /* nullable */, void *stream);

/* Replaces: the rollout loops of that population (train/rllib/pbt.py:47-74; train/stable_baselines/ppo.py:118-137: three models on the
 * same vector env, :84-100 per step).  ssg_rollout_policy with env e under member e / n: the same buffers, strides, uniforms, Philox
 * keying, dev_last_value and per-step launch sequence (one policy launch per step for the whole population, then ssg_step); every
 * handle ssg_rollout_policy serves is served.  Refusals as ssg_rollout_policy, plus those of ssg_pop_act. */
int ssg_pop_rollout(ssg_handle *h, const ssg_population *pop, int K, const float *dev_uniform_KN /* nullable */, uint64_t seed,
                    int64_t step0, double *dev_obs, int32_t *dev_act_KN, float *dev_logp_KN, float *dev_value_KN,
                    float *dev_x_KND /* nullable */, double *dev_reward_KN, uint8_t *dev_done_KN, uint8_t *dev_flags_KN /* nullable */,
                    float *dev_last_value /* nullable */, int64_t step_stride_envs, void *stream);

/* Replaces: train/rllib/rollout.py:15's compute_action for every trial of the PBT experiment at once (train/rllib/pbt.py:29-43).
 * ssg_policy_act_greedy with env e under member e / n's parameter row, one launch for the whole population; each member's slice is
 * bit for bit ssg_policy_act_greedy on that slice with that row.  Validates and refuses as ssg_pop_act does. */
int ssg_pop_act_greedy(ssg_handle *h, const ssg_population *pop, const double *dev_obs, int32_t *dev_actions, float *dev_logp,
                       float *dev_value, float *dev_x /* nullable */, void *stream);

/* Replaces nothing (host only; no reference counterpart: ray hands every trial its own config dict, train/rllib/pbt.py:56-70).  Fills
 * out[0 .. SSG_POP_TABLE_FLOATS(n_members, n_steps)) with the members' f32 constants: 8 per member for GAE and the loss, then for Adam
 * steps step0 + 1 .. step0 + n_steps 8 per member and step (n_steps = 0: no Adam rows, enough for ssg_pop_gae).  SSG_ERR_BAD_ARG for
 * NULL pointers, n_members out of range, n_steps < 0, step0 < 0, out_floats too small or a bad ssg_ppo_hparams record. */
int ssg_pop_pack_hparams(int n_members, const ssg_ppo_hparams *hparams, int64_t step0, int n_steps, float *out, size_t out_floats);

/* Replaces nothing (memory binding; no reference counterpart): the workspace size for a population shaped like *pop, rollouts of up to
 * samples_per_member = K*n samples per member and minibatches of up to max_minibatch samples per member.  SSG_ERR_BAD_ARG for a bad
 * record, n_members out of range or sizes < 1. */
int ssg_pop_workspace_nbytes(const ssg_population *pop, int64_t samples_per_member, int64_t max_minibatch, size_t *nbytes);

/* Replaces: the advantage computation of every trial (train/rllib/pbt.py:47-74, with `lambda` among the mutated hyper-parameters,
 * :36; train/stable_baselines/ppo.py:90 per model).  ssg_ppo_gae per member with that member's gamma / lam (dev_table) over its
 * columns of the [K][N] buffers (N = the handle's n_envs); the advantage mean / unbiased std are per member, with partial sums laid
 * out per member exactly as a single run over n envs lays them out (256-env blocks counted from the member's first env, the same
 * final reduction).  Two launches.  SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers, K < 1, K*n < 2 or a workspace
 * too small. */
int ssg_pop_gae(ssg_handle *h, const ssg_population *pop, const float *dev_table, int K, const double *dev_reward_KN,
                const uint8_t *dev_done_KN, const float *dev_value_KN, const float *dev_last_value, float *dev_adv_KN, float *dev_ret_KN,
                void *dev_workspace, size_t workspace_nbytes, void *stream);

/* Replaces: the SGD phase of every trial (train/rllib/pbt.py:47-74: num_sgd_iter x minibatches per trial, with lr and clip_param
 * mutated per trial, :36-38; train/stable_baselines/ppo.py:118-137: one model.learn per learning rate).  ssg_ppo_update for all members
 * at once: epochs x chunks steps (C = ceil(K*n / minibatches), torch.chunk's split) of {gradient of every member, reduce + Adam of every
 * member}, two launches per step with grid = (the single-policy grid for the chunk length, P).  dev_table: the device copy of
 * ssg_pop_pack_hparams' output for table_steps >= epochs*chunks Adam steps (its step0 is the population's Adam step count before this
 * call).  dev_stats (nullable): f32 [P][epochs*chunks][4].  Needs ssg_pop_gae's statistics in the workspace.  No floating-point
 * atomics; member m's parameters, moments and stats are bitwise those of ssg_ppo_update on its slice.  SSG_ERR_BAD_ARG (nothing
 * launched) for a bad record, NULL pointers, K < 1, epochs < 1, minibatches < 1, table_steps too small or a workspace too small — and,
 * like ssg_pop_update_ext, while slices are bound to the handle (ssg_pop_set_slices: the update then runs through ssg_pop_update_sched). */
int ssg_pop_update(ssg_handle *h, const ssg_population *pop, const float *dev_table, int table_steps, int K, const float *dev_x,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_perm,
                   int epochs, int minibatches, float *dev_adam_mv, float *dev_stats /* nullable */, void *dev_workspace,
                   size_t workspace_nbytes, void *stream);

/* The extended update for a population.  The per-member constants are read on the device, like dev_table: dev_ext is f32
 * [P][4] = per member vf_clip, max_grad_norm, kl_target, 0 (the caller rounds them from double); an entry <= 0 switches that term off
 * for that member.  What changes the launch sequence or needs a buffer the host must know, so flags says it: */
#define SSG_POP_EXT_GRAD_CLIP 0x1u /* some member has max_grad_norm > 0: the three-launch sequence runs for the population */
#define SSG_POP_EXT_VF_CLIP 0x2u   /* some member has vf_clip > 0: dev_value_old is required */
typedef struct ssg_pop_ext {
    uint32_t struct_size;       /* sizeof(ssg_pop_ext) */
    uint32_t flags;             /* SSG_POP_EXT_* */
    const float *dev_ext;       /* f32 [P][4] */
    float *dev_kl_coef;         /* f32 [P]; NULL = no KL term for anyone (a member's 0 = none for that member) */
    const float *dev_logp_all;  /* f32 [K][N][4] (ssg_pop_dist); required when dev_kl_coef is given */
    const float *dev_value_old; /* f32 [K][N]; required with SSG_POP_EXT_VF_CLIP */
} ssg_pop_ext;

/* Replaces: the old action distributions every RLlib trial keeps for its KL term (train/rllib/pbt.py:47-74).  ssg_ppo_dist for a
 * population over the [K][N] rows of dev_x: row t*N + m*n + e runs under parameter row m.  One launch for all members.
 * SSG_ERR_BAD_ARG (nothing launched) for a bad record, NULL pointers or K outside 1..65535. */
int ssg_pop_dist(ssg_handle *h, const ssg_population *pop, int K, const float *dev_x, float *dev_logp_all, void *stream);

/* Replaces: the SGD phase of every trial with RLlib's loss (train/rllib/pbt.py:47-74, kl_coeff = 1.0 at :55-62) or PPO2's
 * (train/stable_baselines/ppo.py:118-137).  ssg_pop_update with the extended loss per member.  With SSG_POP_EXT_GRAD_CLIP every
 * minibatch takes three launches; members with max_grad_norm <= 0 then get coef = 1.0f, which is exact.  The last launch adapts the
 * coefficients of the members whose kl_target is > 0 (when dev_kl_coef is given).  dev_stats (nullable): f32 [P][epochs*chunks][8].
 * Member m's parameters, moments, stats rows and coefficient are bitwise those of ssg_ppo_update_ext on its slice alone with its
 * constants (of ssg_ppo_update when all its terms are off).  Refusals as ssg_pop_update, plus a bad ssg_pop_ext record or a missing
 * pointer that a switched-on term needs. */
int ssg_pop_update_ext(ssg_handle *h, const ssg_population *pop, const ssg_pop_ext *ext, const float *dev_table, int table_steps, int K,
                       const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                       const int64_t *dev_perm, int epochs, int minibatches, float *dev_adam_mv, float *dev_stats /* nullable */,
                       void *dev_workspace, size_t workspace_nbytes, void *stream);

/* Per-member schedules: member m runs epochs[m] epochs of its own chunking of its K*n samples (minibatches[m] asked for; torch.chunk's
 * split: chunks of C_m = ceil(K*n / minibatches[m]), the last one shorter, chunks_m = ceil(K*n / C_m) of them), steps_m = epochs[m] *
 * chunks_m Adam steps in all.  Launch j of the update serves minibatch j of every member that still has one, n_launches = max steps_m
 * launch groups, each as wide as max C_m needs.  What differs between the members within a launch travels in a device table of int32,
 * SSG_POP_SCHED_ROW per member (steps_m, chunks_m, C_m, epochs[m], 0...) followed, per launch j and member m, by a record of
 * SSG_POP_SCHED_ROW: [0..1] the int64 offset of the minibatch in the member's permutation rows (ep * K*n + b0), [2] its length M,
 * [3] the member's own gradient grid G (min(ceil(M / 64), 512): the single-policy grid for M, so the member's sums run in the
 * single-policy order), [4] 1 on the first chunk of an epoch, [5] 1 while j < steps_m (else the record is all zeros and the member
 * sits the launch out), [6] the f32 bits of 1 / (float)M, [7] 0. */
#define SSG_POP_SCHED_ROW 8
#define SSG_POP_SCHED_INTS(n_members, n_launches) ((size_t)(n_members) * 8u * (size_t)(1 + (n_launches)))

/* Replaces nothing (host only; ray hands every trial its own num_sgd_iter / sgd_minibatch_size in its config dict, train/rllib/pbt.py:40-41
 * the mutated ones, :65-68 the initial draws).  Packs the schedule table for samples_per_member = K*n samples.  steps_out (nullable)
 * receives steps_m, *n_launches_out max steps_m.  out == NULL is the size query: only those are written and the table needs
 * SSG_POP_SCHED_INTS(n_members, *n_launches_out) int32.  SSG_ERR_BAD_ARG for NULL epochs / minibatches / n_launches_out, n_members out
 * of range, samples_per_member < 1, an entry < 1, a step count beyond 2^31-1 or out_ints too small. */
int ssg_pop_pack_schedule(int n_members, int64_t samples_per_member, const int32_t *epochs, const int32_t *minibatches,
                          int32_t *out /* nullable */, size_t out_ints, int32_t *steps_out /* nullable */, int32_t *n_launches_out);

/* Replaces nothing (host only; the per-trial optimiser state ray restores with a checkpoint, train/rllib/pbt.py:29-43).
 * ssg_pop_pack_hparams for members that have taken different numbers of Adam steps (they do once their schedules differ, pbt.py:40-41):
 * the Adam rows of member m are steps step0[m] + 1 .. step0[m] + n_steps — bitwise what ssg_pop_pack_hparams writes for that member
 * when called with step0 = step0[m].  Refusals as ssg_pop_pack_hparams (NULL step0, an entry < 0). */
int ssg_pop_pack_hparams_steps(int n_members, const ssg_ppo_hparams *hparams, const int64_t *step0, int n_steps, float *out,
                               size_t out_floats);

/* Replaces: the SGD phase of every trial with the trial's OWN num_sgd_iter and sgd_minibatch_size (train/rllib/pbt.py:40-41 mutated,
 * :65-68 drawn from {10, 20, 30} and {128, 512, 2048}).  ssg_pop_update (ext == NULL) or ssg_pop_update_ext on per-member schedules:
 * epochs / minibatches are host arrays of P entries, dev_sched the device copy of ssg_pop_pack_schedule's table for them, dev_table
 * ssg_pop_pack_hparams(_steps)' for table_steps >= n_launches Adam steps, dev_perm int64 [P][perm_epochs][K*n] with perm_epochs >=
 * max epochs (member m reads its first epochs[m] rows).  The workspace is ssg_pop_workspace_nbytes' for max_minibatch = max C_m.
 * dev_stats (nullable): f32 [P][n_launches][4, or 8 with ext]; member m's rows past steps_m are not written.  Two launches per launch
 * group (three with SSG_POP_EXT_GRAD_CLIP), plus the KL adaptation, in which member m divides by its own chunks_m.  Member m's
 * parameters, moments, stats rows and coefficient are bitwise those of ssg_ppo_update(_ext) on its slice with epochs[m] and
 * minibatches[m]; with equal entries the call computes what ssg_pop_update(_ext) computes.  SSG_ERR_BAD_ARG (nothing launched) as
 * ssg_pop_update / ssg_pop_update_ext, and for NULL epochs / minibatches / dev_sched, an entry < 1, perm_epochs < max epochs or
 * table_steps < n_launches.  With unequal slices bound (ssg_pop_set_slices): see there for dev_sched, dev_perm and the workspace. */
int ssg_pop_update_sched(ssg_handle *h, const ssg_population *pop, const ssg_pop_ext *ext /* nullable: the plain loss */,
                         const float *dev_table, int table_steps, const int32_t *dev_sched, const int32_t *epochs,
                         const int32_t *minibatches, int perm_epochs, int K, const float *dev_x, const int32_t *dev_act,
                         const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_perm, float *dev_adam_mv,
                         float *dev_stats /* nullable */, void *dev_workspace, size_t workspace_nbytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Per-member batch sizes: unequal env slices (ABI 9 addition)
 * The reference's sixth mutated hyper-parameter is train_batch_size (train/rllib/pbt.py:42, drawn from {10000, 20000, 40000} at :69-70).
 * A population may be laid out over the handle's envs in contiguous slices of unequal size: member m owns envs [o_m, o_m + n_m), o_0 = 0,
 * o_{m+1} = o_m + n_m, every n_m >= 1, sum n_m == n_envs.  All members still roll out the same K steps and update at the same moment; a
 * member's batch is K * n_m samples (its SHARE of the handle's K * n_envs, not an absolute count).  Envs are fungible: the layout may
 * be re-bound between updates without touching env state.
 *
 * The layout is bound to the handle (ssg_pop_set_slices), as the terminal-observation buffer and the map bank are.  While it is bound:
 *  - a population whose n_members equals the bound P follows the slices and the divisor check does not apply; any other P is
 *    SSG_ERR_BAD_ARG and nothing is launched — for every ssg_pop_* entry point that takes the handle, and for ssg_eval_reduce with
 *    n_members > 1;
 *  - ssg_pop_act, ssg_pop_act_greedy, ssg_pop_rollout, ssg_pop_dist, ssg_pop_evaluate: env e runs under the member whose slice holds
 *    it, the Philox counter stays the global env id, still one policy launch (grid: workgroups of the largest slice x P; a workgroup
 *    past its member's n_m leaves at once);
 *  - ssg_pop_gae: member m walks its own columns, its partial sums are laid out as a single run over n_m envs lays them out (256-env
 *    blocks from o_m) and its statistics divide by K * n_m; SSG_ERR_BAD_ARG when some K * n_m < 2;
 *  - the update runs through ssg_pop_update_sched only (it already gives every member its own M, G and step count): ssg_pop_update
 *    and ssg_pop_update_ext return SSG_ERR_BAD_ARG.  dev_sched must come from ssg_pop_pack_schedule_samples with samples[m] = K * n_m;
 *    member m's sample i = t*n_m + e is row t*N + o_m + e; dev_perm is a FLAT int64 buffer: member m's block is perm_epochs rows of
 *    K * n_m member-local indices, the blocks in member order, nothing padded to the widest member.  The workspace is
 *    ssg_pop_workspace_nbytes' for samples_per_member = max K * n_m and max_minibatch = max C_m;
 *  - ssg_pop_episode_stats and ssg_eval_reduce sum each member's own rows; ssg_pop_exploit does not depend on the slices.
 * Contract: member m's rollout rows, advantages, statistics, parameters, moments, stats rows and KL coefficient are bit for bit what
 * ssg_policy_act, ssg_rollout_policy, ssg_ppo_gae and ssg_ppo_update(_ext) compute on a handle of n_m envs with env_id_base + o_m.  With
 * equal slices bound every result is bit for bit what it is with nothing bound; with nothing bound nothing changes.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_POP_SLICE_ROW 4

/* Replaces nothing (host only; ray hands every trial its own train_batch_size, train/rllib/pbt.py:69-70).  Packs the slices table:
 * SSG_POP_SLICE_ROW int32 per member, row m = {o_m, n_m, the 256-env blocks of n_m, 0}.  SSG_ERR_BAD_ARG for NULL pointers, n_members
 * outside 1..SSG_POP_MAX_MEMBERS, an entry < 1, a sum beyond 2^31-1 or out_ints < SSG_POP_SLICE_ROW * n_members. */
int ssg_pop_pack_slices(int n_members, const int32_t *n_envs_per_member, int32_t *out, size_t out_ints);

/* Replaces nothing (memory binding).  Binds the layout to the handle: the handle keeps a host copy of the P sizes and the caller's
 * device pointer to the packed table (ssg_pop_pack_slices' output for the same sizes; the caller owns that memory and keeps it alive
 * while the layout is bound).  n_members == 0 or a NULL pointer unbinds.  SSG_ERR_BAD_ARG (the binding stays as it was): a sum
 * different from the handle's n_envs, an entry < 1, n_members outside 1..SSG_POP_MAX_MEMBERS. */
int ssg_pop_set_slices(ssg_handle *h, int n_members, const int32_t *n_envs_per_member /* host [P] */,
                       const int32_t *dev_slices /* device copy of the packed table */);

/* Replaces nothing (introspection).  *n_members = the bound P (0: nothing bound); out (nullable) receives the P sizes. */
int ssg_pop_get_slices(const ssg_handle *h, int *n_members, int32_t *out /* nullable: int32 [P] */);

/* Replaces nothing (host only).  ssg_pop_pack_schedule with a sample count per member (samples[m] = K * n_m): C_m, chunks_m, M and G
 * derive from the member's own count.  Header row m also carries, in entries [4..5], the int64 sum of samples[0..m): member m's block
 * of the flat permutation buffer starts perm_epochs times that many entries in.  With all counts equal the records, and entries
 * [0..3] of the header rows, are those of ssg_pop_pack_schedule.  Refusals as ssg_pop_pack_schedule (NULL samples, an entry < 1). */
int ssg_pop_pack_schedule_samples(int n_members, const int64_t *samples /* [P]: K*n_m */, const int32_t *epochs, const int32_t *minibatches,
                                  int32_t *out /* nullable */, size_t out_ints, int32_t *steps_out /* nullable */, int32_t *n_launches_out);

/* Replaces: PopulationBasedTraining's exploit step (train/rllib/pbt.py:29-43: a bottom-quantile trial restores a top-quantile trial's
 * checkpoint), on the device: member m takes the parameter row AND the Adam moments of member src[m] (host array int32 [P];
 * src[m] == m keeps).  Validated on the host: every index in range and no source itself a destination (src[src[m]] == src[m]), so the
 * copy does not depend on its order; otherwise SSG_ERR_BAD_ARG and nothing is launched.  One launch; src is free when the call returns. */
int ssg_pop_exploit(ssg_handle *h, const ssg_population *pop, const int32_t *src, float *dev_adam_mv, void *stream);

/* Replaces: the per-trial episode_reward_mean PopulationBasedTraining ranks trials by (train/rllib/pbt.py:31, reward_attr) —
 * SSG_F_STATS is per handle and cannot be split by member.  One lane per env walks t = 0 .. K-1 over dev_reward_KN / dev_done_KN
 * ([K][N] rows of a rollout) with caller-owned carry columns (dev_carry_return f64 [N], dev_carry_length i32 [N]; zero after a reset),
 * so an episode that spans rollouts is counted once, at its end; at a done step it adds llrint(100 * return), the length and 1 to the
 * member's row of dev_out (int64 [P][3], accumulated: the caller zeroes it).  Integer sums: order-free and exact.  One launch. */
int ssg_pop_episode_stats(ssg_handle *h, int n_members, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                          double *dev_carry_return, int32_t *dev_carry_length, int64_t *dev_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Evaluation (ABI 9 addition): run a policy, or a population, for whole episodes and report how it did
 * The reference's evaluation script (train/rllib/rollout.py:8-26): act, step until done, print the episode's reward.  Here for every env
 * of a handle at once, with no host synchronisation inside a call.  Every env contributes exactly its first E episodes (an env that
 * crashes early does not weigh more than one that sails on), and each counted episode's ending is tallied from the SSG_EV_* bits of its
 * done step.
 *
 * Per-env carry, caller-owned, zeroed by the caller after a reset: dev_carry_return f64 [N] (the running episode's return) and dev_carry
 * int32 [N][4] = (length, goal events of the running episode, episodes counted so far, 0), 16-byte aligned.  While an env's episodes
 * counted is below E, every step adds the reward to its return, 1 to its length and 1 to its goal events when the step's flags have
 * SSG_EV_GOAL_REACHED; at a done step it adds to its row of dev_env_stats (int64 [N][SSG_EVAL_STATS], caller-zeroed):
 *   [0] 1 (an episode)                 [1] llrint(100 * return), as ssg_pop_episode_stats counts it      [2] length
 *   [3] 1 if the done step's flags have SSG_EV_COLLIDING       [4] ... SSG_EV_OUT_OF_BOUNDS      [5] ... SSG_EV_MAX_STEPS
 *   [6] ... SSG_EV_NO_GOALS_LEFT       [7] the episode's goal events
 * ([3]..[6] are not exclusive of each other), then zeroes return, length and goal events and bumps its episode count.  Once an env has
 * counted E episodes its row and carry no longer change, though the env keeps stepping.  An episode still running when a call ends
 * stays in the carry: a later call continues it.  The carry's fourth word is neither read nor computed: it keeps the caller's value.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_EVAL_STATS 8
#define SSG_EVAL_GREEDY 0x1u /* ssg_eval.flags: the arg-max action (ssg_policy_act_greedy) instead of a draw */
typedef struct ssg_eval {
    uint32_t struct_size;        /* sizeof(ssg_eval) */
    uint32_t flags;              /* SSG_EVAL_GREEDY or 0; any other bit is refused */
    int32_t episodes_per_env;    /* E >= 1 */
    int32_t n_steps;             /* T >= 1: the iterations this call enqueues */
    uint64_t seed;               /* Philox key of the sampled mode without uniforms, as ssg_rollout_policy keys it */
    int64_t step0;               /* iteration k is step step0 + k of that stream */
    const float *dev_uniform_TN; /* nullable: f32 [T][N], row k drives iteration k; refused together with SSG_EVAL_GREEDY */
    double *dev_obs;             /* f64 [N][D]: the handle's current observations, rewritten by every step */
    int32_t *dev_act;            /* one-row scratch buffers [N], rewritten by every iteration: all required */
    float *dev_logp;
    float *dev_value;
    double *dev_reward;
    uint8_t *dev_done;
    uint8_t *dev_flags;
    double *dev_carry_return;    /* f64 [N] */
    int32_t *dev_carry;          /* int32 [N][4], 16-byte aligned */
    int64_t *dev_env_stats;      /* int64 [N][SSG_EVAL_STATS] */
} ssg_eval;

/* Replaces: the loop of train/rllib/rollout.py:8-26 (compute_action, env.step until done, the episode's reward summed), T iterations
 * enqueued from C on `stream` with no host synchronisation.  Iteration k: (1) the policy launch at step step0 + k — greedy, or sampling
 * with row k of dev_uniform_TN, or Philox exactly as ssg_rollout_policy keys it; (2) ssg_rollout_traj(h, dev_act, 1, ...), the call
 * ssg_rollout_policy makes: every handle kind it serves is served, with identical launches; (3) the accounting launch above.
 * Everything refusable is refused before the first launch: what ssg_rollout_policy refuses (a capturing stream and an unfilled map ring
 * among it), a bad ssg_eval record, a NULL required pointer, and a handle without SSG_FLAG_AUTO_RESET (a done env would never start its
 * next episode). */
int ssg_evaluate(ssg_handle *h, const ssg_policy *pol, const ssg_eval *ev, void *stream);

/* Replaces: the `reward_total += reward` ... print of train/rllib/rollout.py:13-26 for a caller that steps the handle itself (ssg_step
 * with its own actions): the accounting launch of ssg_evaluate alone, on one step's dev_reward / dev_done / dev_flags rows ([N] each),
 * with episodes_per_env = E >= 1 and the carries and stats rows described above.  One launch.  SSG_ERR_BAD_ARG (nothing launched) for
 * E < 1, a NULL pointer or a dev_carry that is not 16-byte aligned. */
int ssg_eval_account(ssg_handle *h, int episodes_per_env, const double *dev_reward, const uint8_t *dev_done, const uint8_t *dev_flags,
                     double *dev_carry_return, int32_t *dev_carry, int64_t *dev_env_stats, void *stream);

/* Replaces: train/rllib/rollout.py:8-26 for every trial of the PBT experiment at once (train/rllib/pbt.py:29-43 ranks trials by training
 * episodes; this is the held-out run).  ssg_evaluate with the population's one policy launch per step (ssg_pop_act / ssg_pop_act_greedy);
 * member m's envs are rows [m*n, (m+1)*n) of every buffer, n = N / n_members.  Refuses what ssg_pop_rollout and ssg_evaluate refuse. */
int ssg_pop_evaluate(ssg_handle *h, const ssg_population *pop, const ssg_eval *ev, void *stream);

/* Replaces: the mean over rollouts a user of train/rllib/rollout.py:8-26 forms by hand.  dev_member_stats (int64 [n_members][SSG_EVAL_STATS])
 * is WRITTEN, not accumulated, with the column sums of each member's n = N / n_members rows of dev_env_stats: one workgroup per member,
 * a strided loop and an integer tree, no atomics.  n_members = 1 serves a single policy.  One launch. */
int ssg_eval_reduce(ssg_handle *h, int n_members, const int64_t *dev_env_stats, int64_t *dev_member_stats, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Evaluation recorder (addition to ABI 9): the trajectories, and optionally the frames, of a few envs of an evaluation run
 * The reference's evaluation loop renders every step (train/rllib/rollout.py:18-19) and with --out keeps
 * [state, action, next_state, reward, done] of every step (train/rllib/rollout.py:20-28).  While a record is bound to a handle,
 * ssg_evaluate / ssg_pop_evaluate keep exactly that for R tracked envs, on the device, with no host synchronisation and no atomics.
 *
 * Slot r tracks env e = env_ids[r].  All buffers are the caller's, on the device, env-major (a slot's C steps are contiguous):
 * obs / next_obs f64 [R][C][D] (D = history * (6 + n_beams)), act i32 / logp f32 / value f32 / reward f64 / done u8 / flags u8 [R][C],
 * cursor i32 [R] (steps kept so far) and overflow i32 [R] (counted steps that found the slot full); the caller zeroes cursor and
 * overflow to start a recording, and nothing else needs initialising.
 *
 * Iteration k of the loop, for every slot r:
 *   - the slot is ACTIVE iff env e has counted fewer than E = ssg_eval.episodes_per_env episodes (dev_carry[e][2] < E, read BEFORE
 *     this iteration's accounting launch) and cursor[r] < C.  An active slot writes, at t = cursor[r]:
 *       obs[r][t]      env e's row of dev_obs as the policy launch read it: the raw f64 row, before any observation filter
 *       act, logp, value [r][t]   the policy launch's outputs for e
 *       reward, done, flags [r][t]   the step's
 *       next_obs[r][t] the TERMINAL observation of the step (env e's row of dev_term_obs) when done, else e's row of dev_obs after it
 *       frames[r][t / S] when frames are on and t % S == 0: bit for bit the frame ssg_render(h, e, W, H, ..., frame_flags) draws at
 *                      the moment obs[r][t] was current — BEFORE the step: what the agent saw when it chose act[r][t]
 *     and then cursor[r] += 1;
 *   - a slot whose env still counts but whose cursor[r] == C writes nothing and adds 1 to overflow[r];
 *   - a slot whose env has counted E episodes touches nothing, ever.
 * The kept steps of a slot are therefore exactly the steps the accounting counted, until the capacity runs out; episodes are cut
 * where done is set, and a later call continues at the cursors as it continues the carries.  The post-crash state of a done step is
 * never drawn: the env is reset inside the step, so the frame after a done step shows the next episode's first state.
 *
 * Launches.  Per iteration: one R-lane launch ahead of the policy launch (obs), one R-lane launch between the step and the accounting
 * launch (everything else, the cursors), and with frames one launch of R x W x H pixels ahead of the step.  For the duration of the
 * call the step kernel's terminal-observation rows (ssg_set_terminal_obs) point at dev_term_obs; the caller's own binding is back in
 * place on every way out.  The handle's state blob, observations, reward / done / flags rows, carries and stats rows are bit for bit
 * what they are with nothing bound, and with nothing bound the loop enqueues exactly the launches it enqueued before this addition.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_EVAL_REC_MAX_ENVS 64
typedef struct ssg_eval_recorder {
    uint32_t struct_size;     /* sizeof(ssg_eval_recorder) */
    int32_t n_tracked;        /* R in 1..SSG_EVAL_REC_MAX_ENVS */
    const int32_t *env_ids;   /* HOST int32 [R]: distinct, each in [0, n_envs), any order; copied by ssg_set_eval_recorder */
    int32_t capacity;         /* C >= 1: the steps kept per tracked env, across all of its episodes */
    int32_t frame_width;      /* W, H in 1..8192 and S >= 1: read only with dev_frames != NULL */
    int32_t frame_height;
    int32_t frame_every;      /* S: a frame for every S-th kept step of a slot (t % S == 0) */
    uint32_t frame_flags;     /* bit 0 = debug drawing, as ssg_render's flags */
    uint32_t reserved;        /* 0 */
    double *dev_obs;          /* f64 [R][C][D] */
    double *dev_next_obs;     /* f64 [R][C][D] */
    int32_t *dev_act;         /* [R][C] each */
    float *dev_logp;
    float *dev_value;
    double *dev_reward;
    uint8_t *dev_done;
    uint8_t *dev_flags;
    int32_t *dev_cursor;      /* i32 [R] */
    int32_t *dev_overflow;    /* i32 [R] */
    double *dev_term_obs;     /* f64 [n_envs][D]: scratch for the step kernel's terminal-observation rows; need not be initialised */
    uint8_t *dev_frames;      /* nullable (no frames): u8 [R][ceil(C / S)][W][H][3], each frame laid out as ssg_render's */
} ssg_eval_recorder;

/* Replaces: `rollout.append([state, action, next_state, reward, done])` and env.render() of train/rllib/rollout.py:18-21, as a record
 * bound to the handle (host only, nothing launched, nothing allocated); NULL unbinds.  The library checks env_ids and keeps its own
 * copy, which every recorder launch receives by value: the caller's array is free when the call returns.  Every refusal is made
 * before anything changes and leaves the previous binding in place: SSG_ERR_UNSUPPORTED for history > 2 (no terminal observations:
 * ssg_set_terminal_obs); SSG_ERR_BAD_ARG for a handle without SSG_FLAG_AUTO_RESET, a struct_size mismatch, reserved != 0, n_tracked
 * outside 1..SSG_EVAL_REC_MAX_ENVS, capacity < 1, a NULL env_ids or required buffer, an env id that repeats or lies outside
 * [0, n_envs), and with dev_frames: frame_width or frame_height outside 1..8192, frame_every < 1, or more than 2^31 bytes of frames
 * per slot (ceil(C / S) * W * H * 3). */
int ssg_set_eval_recorder(ssg_handle *h, const ssg_eval_recorder *rec /* NULL unbinds */);

/* Replaces nothing (introspection).  *out = the bound record; out->struct_size == 0 (all of *out zero): nothing bound.  out->env_ids
 * points at the library's own copy, valid until the next ssg_set_eval_recorder or ssg_destroy on the handle. */
int ssg_get_eval_recorder(const ssg_handle *h, ssg_eval_recorder *out /* struct_size 0: nothing bound */);

/* ---------------------------------------------------------------------------------------------------
 * Episode log (addition to ABI 9): every finished TRAINING episode on record, in a ring on the device
 * The reference's Stable-Baselines script wraps its envs in Monitor and reads the per-episode (r, l, t) rows back with load_results /
 * ts2xy (train/stable_baselines/ppo.py:7-8,38-40): its callback plots return against timesteps and keeps the best model by
 * np.mean(y[-100:]), the mean of the last 100 episodes (train/stable_baselines/ppo.py:25-52).  ssg_pop_episode_stats and the handle's
 * counters give one sum per update; this keeps the episodes themselves.  Nothing is bound to the handle: the record below and all of
 * its buffers are the caller's, as with ssg_eval_recorder, and a call reads the [K][N] reward / done / flags rows a rollout left.
 *
 * Per-env carry, caller-owned, zero after a reset: dev_carry_return f64 [N] (the running episode's return) and dev_carry int32 [N][2] =
 * (length, goal events of the running episode).  Every step adds the reward to the return (in step order, in f64, as
 * ssg_pop_episode_stats adds it), 1 to the length and 1 to the goal events when the step's flags have SSG_EV_GOAL_REACHED; a done step
 * appends one ssg_episode_record and zeroes the three.  An episode still running when a call ends stays in the carry.
 *
 * The order contract.  The episodes that end in one call are ranked by (t ascending, then env ascending): the order of
 * np.nonzero(done) on the [K, N] array.  With head = dev_head[0] before the call and count = the episodes the call ends, the episode of
 * rank r goes to slot (head + r) % capacity.  When count > capacity, the records of rank below count - capacity are not written at all
 * (later ranks of the same call own their slots), so two ranks never race for a slot.  Then dev_head[0] = head + count and
 * dev_head[1] = count.  The ring and the head depend on the inputs alone — not on the launch geometry, not on the member layout (only
 * the member bits of `end` do), not on how a sequence of steps is cut into calls: two calls over K1 and then K2 rows leave, bit for bit,
 * the ring, dev_head[0] and the carries that one call over the K1 + K2 rows leaves (dev_head[1] is the last call's own count).
 *
 * Launches: three on `stream`, always — no atomics, no host synchronisation.  (a) count: one workgroup per (row, 256-env tile) counts the
 * tile's done bytes of that row (wave ballots and popcounts) into the workspace's counts[t * tiles + tile]; (b) scan: ONE workgroup
 * turns counts into its exclusive prefix sums in index order (integers: exact), copies dev_head[0] and the total into the workspace and
 * advances dev_head; (c) walk: one lane per env walks t = 0 .. K-1 with its carries, eight rows loaded at a time; at a done step its
 * rank is the scanned entry of (t, tile) plus its rank among the tile's done lanes of that row (a ballot prefix per wave; the four
 * waves' counts meet in LDS, one barrier per eight rows), and it writes its record with two 16-byte vector stores.  The walk reads the
 * old head from the workspace, never from dev_head.
 * The member of env e is e / (N / n_members) on equal slices and a binary search of the slices table otherwise, once per lane.
 * One call at a time per workspace.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_EPISODE_LOG_MAX_CELLS (1 << 22) /* K * ceil(n_envs / 256) of one call at most: what the one scanning workgroup takes on */
typedef struct ssg_episode_record {
    double ret;      /* the episode's return: carry + rew[t0] + ... + rew[t], added in step order in f64 */
    int64_t step;    /* step0 + t of its done step */
    int32_t env;     /* global env id: the handle's env_id_base + e */
    int32_t length;  /* steps, carried across calls */
    int32_t goals;   /* steps of the episode whose flags had SSG_EV_GOAL_REACHED (0 when dev_flags_KN is NULL) */
    uint32_t end;    /* low byte: the done step's flags byte (0 when NULL); bits 8..15: the member that owns the env */
} ssg_episode_record;

typedef struct ssg_episode_log {
    uint32_t struct_size;            /* sizeof(ssg_episode_log) */
    int32_t n_members;               /* 1 for a single policy, P for a population (equal split or the ssg_pop_set_slices layout) */
    int64_t capacity;                /* slots of the ring, >= 1 */
    ssg_episode_record *dev_records; /* [capacity], 16-byte aligned; need not be initialised */
    int64_t *dev_head;               /* int64 [2], caller-zeroed: [0] episodes ever appended, [1] episodes appended by the last call */
    double *dev_carry_return;        /* f64 [n_envs] */
    int32_t *dev_carry;              /* int32 [n_envs][2]: length, goal events; 8-byte aligned */
    void *dev_workspace;             /* >= ssg_episode_log_workspace_nbytes(n_envs, K) bytes, 16-byte aligned */
    size_t workspace_nbytes;
} ssg_episode_log;

/* Replaces nothing (host only; Monitor appends to a file as it goes).  The workspace of ssg_episode_log_append for a handle of n_envs
 * envs and calls of up to K rows: int64 [2] (the head before the call, the call's count), then int32 [K * ceil(n_envs / 256)] (the
 * counts, scanned in place) — 16 + 4 * K * ceil(n_envs / 256) bytes.  SSG_ERR_BAD_ARG for NULL nbytes, an argument < 1 or
 * K * ceil(n_envs / 256) above SSG_EPISODE_LOG_MAX_CELLS. */
int ssg_episode_log_workspace_nbytes(int n_envs, int K, size_t *nbytes);

/* Replaces: Monitor's per-episode (r, l, t) rows, read by load_results / ts2xy in train/stable_baselines/ppo.py:7-8,38-40 — for the K
 * rows of a rollout at once, as described above: three launches on `stream`.  dev_reward_KN / dev_done_KN / dev_flags_KN: the rollout's
 * f64 / u8 / u8 [K][step_stride_envs] buffers in the handle's row layout (what ssg_rollout_policy / ssg_pop_rollout wrote); with
 * dev_flags_KN NULL every record has goals = 0 and a zero low byte of `end`.  Row t is step step0 + t.  The arguments are judged first,
 * then the handle (SSG_ERR_NOT_BOUND without a state blob, like every call that launches).  Refuses (SSG_ERR_BAD_ARG, nothing launched,
 * head and ring untouched): a NULL handle or record; struct_size mismatch; capacity < 1; n_members outside 1..SSG_POP_MAX_MEMBERS,
 * different from a bound slices layout, or one the handle's envs do not split into; NULL dev_records, dev_head, dev_carry_return,
 * dev_carry or dev_workspace; a dev_records or dev_workspace that is not 16-byte aligned, a dev_carry that is not 8-byte aligned;
 * K < 1; K * ceil(n_envs / 256) above SSG_EPISODE_LOG_MAX_CELLS; step_stride_envs < n_envs; NULL dev_reward_KN or dev_done_KN;
 * workspace_nbytes below ssg_episode_log_workspace_nbytes(n_envs, K). */
int ssg_episode_log_append(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, const double *dev_reward_KN,
                           const uint8_t *dev_done_KN, const uint8_t *dev_flags_KN /* nullable */, int64_t step_stride_envs, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Job-wide episode log (addition to ABI 9): the log of a data-parallel job, one gather per rollout
 * The reference's SubprocVecEnv + Monitor + load_results give the per-episode rows over ALL workers' episodes
 * (train/stable_baselines/ppo.py:7-8,25-52,122-123).  Rank r of W owns N_r envs, a contiguous range of global env ids in rank order;
 * the ranks roll out in lockstep, so a call covers the same K rows from the same step0 on every rank.  The job's log is the log ONE
 * ssg_episode_log_append would keep over the concatenated envs: records ranked by (row t ascending, global env ascending).
 *
 * The protocol.  lb_r[t] (t = 0..K) = the episodes that end on shard r in rows before t (lb_r[K] = count_r).  An episode of local rank
 * q on shard r (its position in np.nonzero(done_r)) that ends in row t has the job rank
 *     R = (q - lb_r[t]) + sum_{r' < r} lb_r'[t + 1] + sum_{r' >= r} lb_r'[t]
 * and total = sum_r lb_r[K].  With head = dev_head[0] before the call the record goes to slot (head + R) % capacity unless
 * R < total - capacity; then dev_head[0] = head + total and dev_head[1] = total.  Integers only, no scan across ranks.
 *
 * The shard block: one contiguous, 16-byte aligned buffer per rank and call —
 *     ssg_episode_log_block_header (32 bytes) | int32 lb[rows + 1], zero past K, padded with zeros to 16 bytes | ssg_episode_record [stage]
 * `rows` is the largest K of one call, `stage` (S) the record slots; both are the same on every rank and in every call of a log.  The
 * episode of local rank q lives in slot q % S, and a rank ships its last S records of the call at most (q >= count_r - S).  With
 * S = min(capacity, rows * ceil(total_envs / W)) nothing that the single log would keep is lost: a shard ends rows * N_r episodes per
 * call at most, and a record below its shard's last `capacity` cannot survive in the job's ring.  Slots that no episode of the call
 * owns are unspecified and never read.
 *
 * Launches.  ssg_job_episode_log_shard: four on `stream` — ssg_episode_log_append's count, scan and walk kernels as they are, on a staging
 * ring of capacity S in the block's record region whose head is zero (the order contract already puts rank q at q % S and skips the
 * ranks below count_r - S; the scanned workspace holds lb_r[t] at counts[t * tiles]), and between scan and walk one small kernel that
 * packs the header and lb and zeroes the head the walk reads.  ssg_job_episode_log_merge_blocks: two — one lane per (block r, slot i) with
 * i < min(count_r, S) recovers q (i itself, or the one q in [count_r - S, count_r) congruent to i), takes t = record.step - step0,
 * forms R from the 2 W lb entries and stores the record with the walk's two 16-byte stores, reading dev_head as it stood; then one
 * small launch advances dev_head.  No atomics, no host synchronisation.
 * Memory safety does not rest on the blocks being well-formed: a record with t outside [0, K) or R outside [0, total) is skipped,
 * lb is never indexed past `rows`, a negative count_r or total counts as 0.  Ranks that disagree on K or step0 are a caller error
 * with in-bounds behaviour.
 *
 * Names.  The three calls are ssg_job_episode_log_*, not ssg_episode_log_*: that prefix belongs to the calls of ONE handle's log,
 * ssg_episode_log_workspace_nbytes and ssg_episode_log_append, and tests/test_episode_log.py pins the header to exactly those two
 * under it.  The calls below work on another object — a shard's block, the job's ring — and take the handle's record only for its
 * carries, workspace, ring and head.  `rows` is at most SSG_EPISODE_LOG_MAX_CELLS in all three (a call's K * tiles is, and K <= rows
 * needs no more).
 * ------------------------------------------------------------------------------------------------- */
typedef struct ssg_episode_log_block_header {
    int64_t count;    /* count_r: the episodes that end on the shard in the call */
    int64_t step0;    /* the call's */
    int32_t K;        /* the call's rows */
    int32_t stage;    /* S */
    int64_t reserved; /* 0 */
} ssg_episode_log_block_header;

/* Replaces nothing (host only).  The size of a shard block for calls of up to `rows` rows with `stage` record slots:
 * 32 + 16 * ceil((rows + 1) / 4) + 32 * stage bytes.  SSG_ERR_BAD_ARG for NULL nbytes, rows outside 1..SSG_EPISODE_LOG_MAX_CELLS or
 * stage < 1. */
int ssg_job_episode_log_block_nbytes(int rows, int stage, size_t *nbytes);

/* Replaces: Monitor's per-episode rows of ONE SubprocVecEnv worker's envs, before load_results merges the workers' files
 * (train/stable_baselines/ppo.py:7-8,122-123).  Takes what ssg_episode_log_append takes, advances the shard's carries exactly as it
 * does, and fills dev_block as described above; log->dev_records and log->dev_head (the job's ring) are not touched, the workspace is
 * ssg_episode_log_append's.  Four launches on `stream`.  Refuses (SSG_ERR_BAD_ARG, nothing launched) everything
 * ssg_episode_log_append refuses, and: n_members != 1; rows above SSG_EPISODE_LOG_MAX_CELLS; K > rows; stage < 1; a NULL dev_block or one that is not 16-byte aligned;
 * block_nbytes below ssg_job_episode_log_block_nbytes(rows, stage); a block that overlaps the ring. */
int ssg_job_episode_log_shard(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, const double *dev_reward_KN,
                              const uint8_t *dev_done_KN, const uint8_t *dev_flags_KN /* nullable */, int64_t step_stride_envs, int rows,
                              int stage, void *dev_block, size_t block_nbytes, void *stream);

/* Replaces: load_results' merge of the workers' monitor files into one table (train/stable_baselines/ppo.py:7-8,38-40) — for the
 * n_blocks shard blocks of one call, stacked in rank order (ssg_job_episode_log_block_nbytes(rows, stage) bytes apart), as described
 * above: two launches on `stream`.  Of the record it uses dev_records, capacity and dev_head alone.  Every rank that merges the same
 * blocks into the same ring and head holds the same bits.  Refuses (SSG_ERR_BAD_ARG, nothing launched, head and ring untouched): a
 * NULL handle or record; struct_size mismatch; capacity < 1; n_members != 1; NULL dev_records, dev_head or dev_blocks; a dev_records
 * or dev_blocks that is not 16-byte aligned, a dev_head that is not 8-byte aligned; n_blocks outside 1..SSG_DP_MAX_SHARDS; K < 1 or
 * K > rows; rows above SSG_EPISODE_LOG_MAX_CELLS; stage < 1; blocks that overlap the ring or the head. */
int ssg_job_episode_log_merge_blocks(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, int rows, int stage,
                                     const void *dev_blocks, int n_blocks, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Observation filter (ABI 9 addition): a running mean / std per observation column, kept and applied on the device
 * The reference's RLlib trainers run "PPO" with its defaults (train/rllib/pbt.py:50, train/rllib/ppo.py:28), which in the RLlib
 * generation those scripts are written for include observation_filter = "MeanStdFilter"; Stable-Baselines users wrap the SubprocVecEnv
 * of train/stable_baselines/ppo.py:123 in VecNormalize for the same purpose.  This is that filter's arithmetic, defined below on its
 * own terms: no bit parity with either library is claimed.  With nothing bound, nothing changes: x = (float)(obs / obs_scale).
 *
 * State, per member (one for a single policy) and observation column d, all f64: count, mean[d], M2[d] (the sum of squared
 * deviations from the mean) and denom[d].  dev_state is f64 [n_members][SSG_FILTER_ROWS][obs_dim], row 0 = mean, row 1 = M2,
 * row 2 = denom, row 3 = {count, 0, ...}; all zeros is the empty state.
 *
 * Merging a batch of n_b rows with batch mean mu_b and batch M2_b (Chan et al.), in exactly this association, every product and sum
 * separately rounded (no fused multiply-add):
 *     n'     = n + n_b
 *     delta  = mu_b - mean
 *     mean'  = mean + delta * (n_b / n')
 *     M2'    = (M2 + M2_b) + (delta * delta) * (n * (n_b / n'))
 *     denom' = sqrt(M2' / (n' - 1)) + eps     if n' >= 2, else 1.0
 * Merging into an empty side (n == 0) takes the other side's values as they are.  A constant column c therefore keeps mean == c bit
 * for bit and M2 == 0.0 through every merge, provided the batch's own mean is exact (below: whenever 256 * c is exact in f64).
 *
 * The reduction order of ssg_obs_filter_update over a member's n rows (row r = the r-th row of the member's slice).  It depends on r and
 * n only — not on the launch geometry, on the other members, or on which compute unit ran what — so the result is bitwise reproducible:
 *   1. Tiles.  Rows [256 t, min(256 t + 256, n)) form tile t, n_t rows.  Per column, with x[i] = the tile's i-th row for i < n_t and
 *      0.0 for n_t <= i < 256: S = the halving tree over x (for h = 128, 64, ..., 1: x[i] = x[i] + x[i + h] for i < h; S = x[0]);
 *      mu_t = S / n_t; then q[i] = (x[i] - mu_t) * (x[i] - mu_t) for i < n_t and 0.0 above, and M2_t = the same halving tree over q.
 *   2. Runs.  With T = ceil(n / 256) tiles and L = ceil(T / 8), run g (0..7) holds tiles [g L, min(g L + L, T)) and is formed by
 *      merging them, with the formula above, in increasing t into an empty state (a run may be empty).
 *   3. The eight runs meet in a halving tree (for h = 4, 2, 1: run g = merge(run g, run g + h) for g < h), and run 0 is merged into the
 *      running state as the batch.
 *
 * Normalising: x[d] = (float) clamp((obs[d] - mean[d]) / denom[d], -clip, +clip) — subtraction, division and clamp in f64, then one
 * rounding to f32; clip == 0: no clamp.  A denom entry of 0.0 (the empty state; eps == 0 on a constant column) divides by 1, so the
 * empty state behaves as mean = 0, denom = 1.  ssg_policy.dev_obs_scale is not read while a filter is bound.
 *
 * While a filter is bound to a handle (ssg_set_obs_filter), every policy launch on it forms x this way: ssg_policy_act,
 * ssg_policy_act_greedy, ssg_rollout_policy and ssg_evaluate need n_members == 1, the ssg_pop_* counterparts n_members == P (member m
 * uses its own state rows); anything else is SSG_ERR_BAD_ARG with nothing launched.  ssg_rollout_policy and ssg_pop_rollout enqueue
 * ssg_obs_filter_update ahead of each step's policy launch when SSG_FILTER_UPDATE is set — first merge the N current rows, then
 * normalise those same rows with the merged state, as both libraries do — and never for the value-only forward after the last step:
 * those rows are step 0 of the next rollout.  ssg_policy_act*, ssg_pop_act*, ssg_evaluate and ssg_pop_evaluate never update
 * (evaluation is frozen, like VecNormalize.training = False).  The PPO update reads the stored x rows and does not change.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_FILTER_ROWS 4          /* state rows per member: mean, M2, denom, {count, 0, ...} */
#define SSG_FILTER_UPDATE 0x1u     /* rollout loops merge each step's observations ahead of its policy launch */
typedef struct ssg_obs_filter {
    uint32_t struct_size, flags;   /* sizeof(ssg_obs_filter); SSG_FILTER_UPDATE or 0 (frozen); any other bit refused */
    int32_t n_members, obs_dim;    /* 1 for a single policy, P for a population; history * (6 + n_beams) */
    double clip, eps;              /* clip >= 0 (0: none), eps >= 0; NaN refused */
    double *dev_state;             /* f64 [n_members][SSG_FILTER_ROWS][obs_dim], caller-owned; zero = empty */
    void *dev_workspace;           /* caller-owned, >= ssg_obs_filter_workspace_nbytes(n_envs, obs_dim, n_members) bytes */
    size_t workspace_nbytes;
} ssg_obs_filter;

/* Replaces nothing (host only; the libraries' filters allocate on the host as they go).  The workspace of ssg_obs_filter_update for a
 * handle of n_envs envs: the tile partials, f64 [n_members][ceil(n_envs / 256)][2][obs_dim].  SSG_ERR_BAD_ARG for an argument < 1, NULL
 * nbytes, obs_dim beyond SSG_MAX_HISTORY * (6 + SSG_MAX_BEAMS) or n_members beyond SSG_POP_MAX_MEMBERS. */
int ssg_obs_filter_workspace_nbytes(int n_envs, int obs_dim, int n_members, size_t *nbytes);

/* Replaces: the filter's update on a batch of observations — MeanStdFilter.__call__(x, update=True) behind the "PPO" default of
 * train/rllib/pbt.py:50, VecNormalize's obs_rms.update around the env of train/stable_baselines/ppo.py:123 — as two launches on `stream`
 * (tile partials, then one workgroup per member), whatever f->flags says.  dev_obs: f64 [n_envs][obs_dim] in the handle's row layout;
 * member m's rows are [m n, (m + 1) n), n = n_envs / n_members, or its slice of ssg_pop_set_slices.  f need not be the bound record.
 * Refuses (SSG_ERR_BAD_ARG, nothing launched) what ssg_set_obs_filter refuses, a NULL dev_obs, and an n_members the handle's envs do
 * not split into. */
int ssg_obs_filter_update(ssg_handle *h, const ssg_obs_filter *f, const double *dev_obs, void *stream);

/* Replaces nothing (memory binding; the reference's counterpart is the "observation_filter" entry of the trainer config behind
 * train/rllib/pbt.py:50).  Binds a copy of the record to the handle; the caller owns dev_state and dev_workspace and keeps them alive
 * while it is bound.  NULL unbinds.  SSG_ERR_BAD_ARG, the binding left as it was: struct_size mismatch; obs_dim different from the
 * handle's history * (6 + n_beams); n_members outside 1..SSG_POP_MAX_MEMBERS, or different from a bound slices layout; NULL dev_state
 * or dev_workspace; workspace_nbytes below ssg_obs_filter_workspace_nbytes; an unknown flag; a negative or NaN clip or eps. */
int ssg_set_obs_filter(ssg_handle *h, const ssg_obs_filter *f /* NULL unbinds */);

/* Replaces nothing (introspection).  *out = the bound record; out->struct_size == 0 (all of *out zero): nothing bound. */
int ssg_get_obs_filter(const ssg_handle *h, ssg_obs_filter *out /* struct_size 0: nothing bound */);

/* ---------------------------------------------------------------------------------------------------
 * Job-wide observation filter (ABI 9 addition): the filter above for W ranks that train one policy (ssg_ppo_apply_shards)
 * RLlib's trainers normalise on every worker with the worker's own running filter while it samples, and after each training iteration
 * the driver merges the workers' new statistics and sends the merged filter back (FilterManager.synchronize behind the "PPO" default
 * of train/rllib/ppo.py:28 and train/rllib/pbt.py:50).  Restated on this library's terms; ssg_obs_filter and ssg_obs_filter_update do
 * not change, and with nothing below bound every launch is what it was.
 *
 * A rank keeps three blocks of the state's layout, f64 [n_members][SSG_FILTER_ROWS][obs_dim]:
 *   state   what the policy launches apply and the rollout loops update, exactly as above (the record's dev_state);
 *   buffer  the statistics of this rank's own rows since the last synchronisation: merged from the same per-step batch totals, starting
 *           from all zeros.  It is a state block: mean, M2, denom and count, bit for bit what an empty filter holds after those batches;
 *   base    the state every rank held right after the last synchronisation, identical on all ranks.
 * During a rollout a rank applies its state = base plus its own progress, as an RLlib worker does: the x rows a rollout stores are
 * normalised with rank-local statistics.  After the rollout, before GAE, the ranks all-gather their buffers in rank order —
 * rows f64 [W][n_members][SSG_FILTER_ROWS][obs_dim] — and every rank computes, per member and column,
 *     state = (...((base (+) rows[0]) (+) rows[1]) ...) (+) rows[W - 1]
 * with (+) the merge formula above in its stated association, an empty side (count 0) leaving the other as it is, and denom by the
 * rule above (sqrt(M2 / (n - 1)) + eps for n >= 2, else 1.0); then base = state and buffer = 0 (the caller's copies).  Every rank runs
 * the same arithmetic on the same gathered rows, so the states are bit-identical on all ranks without a broadcast, as
 * ssg_ppo_apply_shards keeps the parameters.
 *
 * No parity with the plain filter is claimed: with one rank, base (+) buffer is not bit for bit the running state of a filter that
 * merged the same batches one by one, because the association differs ((base (+) (b_1 (+) b_2 ...)) against ((base (+) b_1) (+) b_2 ...)).
 * The return filter across ranks is exact and needs no base: "Job-wide return filter" below.  Out of scope: statistics merged per step.
 * ------------------------------------------------------------------------------------------------- */

/* Replaces nothing (memory binding; the reference's counterpart is the per-worker filter buffer RLlib keeps beside the
 * "observation_filter" of train/rllib/ppo.py:28).  Binds dev_buffer, f64 [n_members][SSG_FILTER_ROWS][obs_dim] of the BOUND record,
 * caller-owned, to the handle; NULL unbinds.  While it is bound and the record has SSG_FILTER_UPDATE, the per-step update inside
 * ssg_rollout_policy and ssg_pop_rollout merges each batch total into dev_state and into dev_buffer (the dual finalise kernel: still
 * two launches per step); with nothing bound the launches are what they were.  Every ssg_set_obs_filter call that succeeds, bind or
 * unbind, drops this binding.  SSG_ERR_BAD_ARG, the binding left as it was: a NULL handle; no filter bound; a dev_buffer that is not
 * 8-byte aligned or overlaps the bound record's dev_state. */
int ssg_set_obs_filter_buffer(ssg_handle *h, double *dev_buffer /* NULL unbinds */);

/* Replaces nothing (introspection).  *out = the bound buffer, NULL: none. */
int ssg_get_obs_filter_buffer(const ssg_handle *h, double **out);

/* Replaces: a worker's filter update on a batch of observations, which RLlib applies to the filter and to its buffer alike —
 * MeanStdFilter.__call__(x, update=True) behind the "PPO" default of train/rllib/ppo.py:28.  ssg_obs_filter_update through the dual
 * finalise kernel, by the launcher the rollout loops use: the batch total, formed exactly as there, is merged into f->dev_state and
 * into dev_buffer, each with its own count.  For callers that feed explicit rows; neither f nor dev_buffer need be bound.  Refuses
 * (SSG_ERR_BAD_ARG, nothing launched) what ssg_obs_filter_update refuses, and a dev_buffer that is NULL, not 8-byte aligned or
 * overlaps f->dev_state. */
int ssg_obs_filter_update_buffered(ssg_handle *h, const ssg_obs_filter *f, double *dev_buffer, const double *dev_obs, void *stream);

/* Replaces: the driver's merge of the workers' filter buffers and its copy back to them — FilterManager.synchronize after every
 * training iteration of train/rllib/ppo.py:28 / train/rllib/pbt.py:50 — as one launch on `stream` (one workgroup per member, a thread
 * per column): f->dev_state = dev_base merged with dev_rows[0 .. n_rows - 1] in index order (section comment above); dev_base is f64
 * [n_members][SSG_FILTER_ROWS][obs_dim], dev_rows [n_rows] such blocks.  f->flags and the workspace's contents are not read.  Refuses
 * (SSG_ERR_BAD_ARG, nothing launched) what ssg_set_obs_filter refuses; a NULL or not 8-byte aligned dev_base or dev_rows; n_rows
 * outside 1..SSG_DP_MAX_SHARDS; a dev_base or dev_rows that overlaps f->dev_state. */
int ssg_obs_filter_merge_rows(ssg_handle *h, const ssg_obs_filter *f, const double *dev_base, const double *dev_rows, int n_rows, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Return filter (ABI 9 addition): the rewards of a rollout divided by a running standard deviation of the discounted return
 * The other half of the wrapper above: Stable-Baselines users of train/stable_baselines/ppo.py:123 get VecNormalize(norm_reward=True)
 * by default, which keeps a discounted return per env, updates a running variance with every step's returns and divides the step's
 * rewards by the running standard deviation.  This is that on the device, for a whole rollout's [K][N] reward buffer in one call
 * between the rollout and GAE, defined below on its own terms: no bit parity with Stable-Baselines is claimed (it uses the population
 * variance and sqrt(var + eps)).  Nothing is bound to the handle, the rollout loops do not change, and the raw reward buffer is left as
 * it is (episode statistics and evaluation read it): the call writes a second buffer, which ssg_ppo_gae / ssg_pop_gae take in place
 * of the raw one.
 *
 * State, per member (one for a single policy), all f64: dev_state is [n_members][SSG_FILTER_ROWS], the observation filter's rows at
 * obs_dim = 1: {mean, M2, denom, count}; all zeros is the empty state.  dev_carry, f64 [n_envs], is the discounted return in flight of
 * every env: zero at the start, owned by the caller, zeroed by the caller when the envs are reset by hand.  dev_gamma, f64 [n_members],
 * is the members' discounts, on the device.
 *
 * The walk, in f64, every product and sum separately rounded (no fused multiply-add).  For env e of member m and k = 0 .. K-1:
 *     c       = c * gamma[m] + rew[k][e]        (the product, then the sum)
 *     s[k][e] = c                               (the sample that enters the statistics)
 *     c       = 0.0 where done[k][e] != 0       (after the sample is taken: VecNormalize's ret[news] = 0)
 * and after row K-1 c is written back to dev_carry[e].
 *
 * Batch k of member m is its n_m samples s[k][.] in the order of its rows, reduced exactly as ssg_obs_filter_update reduces one column
 * of n_m rows (above: 256-row tiles with the two halving trees, eight runs of consecutive tiles merged in tile order, the halving tree
 * over the runs), and state_k = merge(state_{k-1}, batch_k) with the merge above in its stated association;
 * denom_k = sqrt(M2_k / (n_k - 1)) + eps for n_k >= 2, else 1.0.  After the call the state is state_{K-1}.
 *
 * Output: out[k][e] = clamp(rew[k][e] / denom_k[m], -clip, +clip), in f64; clip == 0: no clamp; a denom of 0.0 (eps == 0 on constant
 * returns) divides by 1.  Step k is divided by statistics that already include step k, as the library does.  The mean is kept but not
 * subtracted.
 *
 * Frozen (SSG_RET_FILTER_UPDATE clear): dev_state and dev_carry are neither read-modified nor written, and every row is divided by the
 * state's own denom (1 for the empty state).
 *
 * The result depends on a row's index within its member's slice, on n_m, K and the inputs only — not on the launch geometry or on the
 * other members — so it is bitwise reproducible, and two calls over K1 and then K2 rows leave what one call over the K1 + K2 rows does.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_RET_FILTER_UPDATE 0x1u       /* walk the returns and merge them into the state; clear: frozen */
#define SSG_RET_FILTER_MAX_STEPS 1024    /* the largest K of one ssg_ret_filter_apply call (split a longer rollout into several calls) */
typedef struct ssg_ret_filter {
    uint32_t struct_size, flags;   /* sizeof(ssg_ret_filter); SSG_RET_FILTER_UPDATE or 0 (frozen); any other bit refused */
    int32_t n_members, reserved;   /* 1 for a single policy, P for a population (equal split or the ssg_pop_set_slices layout); 0 */
    double clip, eps;              /* clip >= 0 (0: none), eps >= 0; NaN refused */
    const double *dev_gamma;       /* f64 [n_members], each in [0, 1] (the caller's to check: the host does not read device memory) */
    double *dev_state;             /* f64 [n_members][SSG_FILTER_ROWS], caller-owned; zero = empty */
    double *dev_carry;             /* f64 [n_envs], caller-owned; zero at the start */
    void *dev_workspace;           /* caller-owned, >= ssg_ret_filter_workspace_nbytes(n_envs, K, n_members) bytes */
    size_t workspace_nbytes;
} ssg_ret_filter;

/* Replaces nothing (host only; VecNormalize allocates on the host as it goes).  The workspace of ssg_ret_filter_apply for a handle of
 * n_envs envs and calls of up to K steps: the tile partials, f64 [n_members][K][ceil(n_envs / 256)][2], then the denoms, f64
 * [K][n_members] — 8 * n_members * K * (2 * ceil(n_envs / 256) + 1) bytes.  SSG_ERR_BAD_ARG for an argument < 1, NULL nbytes, K beyond
 * SSG_RET_FILTER_MAX_STEPS or n_members beyond SSG_POP_MAX_MEMBERS. */
int ssg_ret_filter_workspace_nbytes(int n_envs, int K, int n_members, size_t *nbytes);

/* Replaces: the reward branch of VecNormalize.step_wait (ret = ret * gamma + rews; ret_rms.update(ret); rews = clip(rews /
 * sqrt(ret_rms.var + eps)); ret[news] = 0) as wrapped around the env of train/stable_baselines/ppo.py:123, for the K steps of a rollout
 * at once: three launches on `stream` (the walk with its tile partials; one workgroup per member; the division), one when frozen.
 * dev_reward_KN / dev_done_KN: the rollout's f64 / u8 [K][step_stride_envs] buffers in the handle's row layout (what
 * ssg_rollout_policy / ssg_pop_rollout wrote); member m's envs are columns [m n, (m + 1) n), n = n_envs / n_members, or its slice of
 * ssg_pop_set_slices.  dev_reward_out_KN: f64, the same stride, WRITTEN for every k < K and e < n_envs (padding columns are not
 * touched); it must not be the input buffer.  dev_denom_KP (nullable): f64 [K][n_members], the divisor of every row (1.0 where the
 * denom was 0.0).  The arguments are judged first, then the handle (SSG_ERR_NOT_BOUND without a state blob, like every call that
 * launches).  Refuses (SSG_ERR_BAD_ARG, nothing launched): a NULL handle or record; struct_size mismatch;
 * an unknown flag; n_members outside 1..SSG_POP_MAX_MEMBERS, different from a bound slices layout, or one the handle's envs do not
 * split into; a negative or NaN clip or eps; NULL dev_gamma, dev_state, dev_carry or dev_workspace; K < 1 or K >
 * SSG_RET_FILTER_MAX_STEPS; step_stride_envs < n_envs; NULL dev_reward_KN, dev_done_KN or dev_reward_out_KN; dev_reward_out_KN ==
 * dev_reward_KN; workspace_nbytes below ssg_ret_filter_workspace_nbytes(n_envs, K, n_members). */
int ssg_ret_filter_apply(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                         int64_t step_stride_envs, double *dev_reward_out_KN, double *dev_denom_KP, void *stream);

/* Job-wide return filter (ABI 9 addition): the filter above for W ranks that train one policy (ssg_ppo_apply_shards)
 * A Stable-Baselines user gets VecNormalize around the WHOLE SubprocVecEnv of train/stable_baselines/ppo.py:122-123: one running
 * variance over the returns of all envs.  For W ranks, rank r owning n_r of the envs, that is computed exactly, because the walk above
 * does not read the running state: a rank reduces its shard to one row per step, the ranks exchange the rows once per rollout, and
 * every rank chains the same rows in the same order.  Job filters have one member (n_members == 1) and update (SSG_RET_FILTER_UPDATE
 * set; a frozen filter needs no rows and stays ssg_ret_filter_apply).
 *
 * For rank r and k = 0 .. K-1, batch_{r,k} is the shard's n_r samples s[k][.] of the walk above, reduced exactly as above (256-row
 * tiles, eight runs merged in tile order, the halving tree over the runs).  The rank's row k is {mean, M2, 0.0, n_r}: the state's row
 * order with the denom slot zero.  With rows f64 [W][K][SSG_FILTER_ROWS], the ranks' rows in rank order, every rank computes
 *     step_k    = rows[0][k] merged with rows[1][k], ..., rows[W-1][k]   (rank order, the merge above in its stated association,
 *                                                                        starting from rows[0][k]; a row of count 0 is skipped)
 *     state_k   = merge(state_{k-1}, step_k)
 *     denom_k   = sqrt(M2_k / (n_k - 1)) + eps for n_k >= 2, else 1.0
 *     out[k][e] = clamp(rew[k][e] / denom_k, -clip, +clip)               (the division above, on the rank's own envs)
 * The carry stays with its env on its rank.  Every rank runs the same arithmetic on the same rows, so the states are bit-identical on
 * all ranks without a broadcast, and what they hold is what one filter over all sum(n_r) envs would hold had it reduced each step's
 * samples shard by shard.  With W = 1, step_k is the rank's own batch k: the state, carry, denoms and output are ssg_ret_filter_apply's
 * bit for bit.  Out of scope: populations across ranks, a frozen job call, statistics merged per step over the wire. */

/* Replaces: the return walk and the per-step variance update of VecNormalize.step_wait on this rank's envs (ret = ret * gamma + rews;
 * the batch moments ret_rms.update forms; ret[news] = 0) as wrapped around the env of train/stable_baselines/ppo.py:123, for K steps: two launches on `stream`, the walk of ssg_ret_filter_apply and a
 * grid of ceil(K / 32) workgroups that reduces the walk's tile partials to dev_rows_K4, f64 [K][SSG_FILTER_ROWS] = {mean, M2, 0.0,
 * n_envs} per step — the bits ssg_ret_filter_apply chains.  dev_carry is updated; dev_state is neither read nor written.  The
 * workspace is ssg_ret_filter_workspace_nbytes(n_envs, K, 1); the rows are the caller's.  Refuses (SSG_ERR_BAD_ARG, nothing launched)
 * what ssg_ret_filter_apply refuses of the record, K, the stride, the reward and done buffers and the workspace; n_members != 1; a
 * record without SSG_RET_FILTER_UPDATE; NULL or not 8-byte aligned rows; rows that overlap f->dev_state. */
int ssg_ret_filter_batches(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                           int64_t step_stride_envs, double *dev_rows_K4, void *stream);

/* Replaces: the rest of that reward branch for a job (ret_rms.update's merge into the running moments with every rank's batch, and rews
 * = clip(rews / sqrt(ret_rms.var + eps)), around the SubprocVecEnv of train/stable_baselines/ppo.py:122-123): two launches on `stream`, one workgroup that merges each step's n_rows rows in rank order
 * and chains the K steps into f->dev_state, then the division of ssg_ret_filter_apply.  dev_rows_WK4: f64 [n_rows][K][SSG_FILTER_ROWS],
 * the ranks' ssg_ret_filter_batches rows of these K steps in rank order.  dev_reward_KN, dev_reward_out_KN and step_stride_envs as in
 * ssg_ret_filter_apply; dev_denom_K (nullable): f64 [K], the divisor of every row.  dev_carry and dev_gamma are not read; the denoms
 * live in the workspace, as there.  Refuses (SSG_ERR_BAD_ARG, nothing launched) what ssg_ret_filter_apply refuses of the record, K,
 * the stride, the reward and output buffers and the workspace; n_members != 1; a record without SSG_RET_FILTER_UPDATE; NULL or not
 * 8-byte aligned rows; n_rows outside 1..SSG_DP_MAX_SHARDS; rows that overlap f->dev_state. */
int ssg_ret_filter_apply_rows(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_rows_WK4, int n_rows, const double *dev_reward_KN,
                              int64_t step_stride_envs, double *dev_reward_out_KN, double *dev_denom_K, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Per-minibatch advantage normalisation (ABI 9 addition): PPO2's rule in the device update
 * train/stable_baselines/ppo.py:90 trains with PPO2, whose _train_step re-normalises the advantages inside every minibatch:
 * advs = (advs - advs.mean()) / (advs.std() + 1e-8) over the minibatch's own samples.  The loss section above normalises once per
 * rollout, with the statistics ssg_ppo_gae / ssg_pop_gae leave in the workspace (train/ppo_torch.py's rule, and RLlib's).  The mode is
 * bound to the handle together with a caller-owned scratch, as ssg_set_terminal_obs and ssg_set_obs_filter bind theirs.
 *
 * SSG_ADV_NORM_BATCH (the default): A = (adv - mean) / (std + adv_eps) with the workspace's batch statistics, as above.
 * SSG_ADV_NORM_MINIBATCH: for every minibatch of every member, with s, q and c the f64 sums of adv, adv^2 and 1 over the minibatch's
 * indices that lie in [0, n_samples) (an index outside stays the zero, gradient-free sample it is and counts for nothing):
 *   mean = s / c;   var = max(0, (q - s*mean) / (c - 1));   std+ = (float)sqrt(var) + adv_eps;   A = (adv - (float)mean) / std+
 * the estimator of ssg_ppo_gae (the unbiased std) over the minibatch.  c == 1: var = 0, so the one sample's A is 0 — what PPO2's numpy
 * std gives; torch.std would give NaN.  c == 0: mean 0, std+ 1.  adv_eps is the policy's (ssg_ppo_hparams) or the member's (its table
 * row).  The row f32[4] = {mean, std+, 1/std+, 0} of member m is written to the scratch's stats rows, where the gradient kernel reads
 * it; the batch statistics in the workspace are not touched, so switching back to SSG_ADV_NORM_BATCH needs no new GAE.  No bit parity
 * with Stable-Baselines is claimed: PPO2 uses the population std, a relative difference of about 1 / (2M).
 *
 * Order of the sums (a function of the minibatch's length M alone; no floating-point atomics).  Two launches per minibatch ahead of the
 * gradient launch, on its stream.  Partials, grid (64, members) x 256 threads: a member with M indices uses B = min(64, ceil(M / 1024))
 * workgroups; thread t of workgroup b takes positions i = b*256 + t, then steps by B*256 while i < M, adding in that order; the 256
 * threads' sums are added as a halving tree (w = 128 .. 1: entry t += entry t + w); one (s, q, c) per workgroup.  Finalise, one
 * workgroup per member: entry b = partial b for b < B and 0 beyond, the same tree, then the row.  A member of a schedule without a
 * minibatch in a launch keeps its row.
 *
 * Scratch: f32 [n_members][4] stats rows, then f64 [n_members][64][3] partials (member m's workgroup b: s, q, c; a minibatch writes
 * its first B), each part rounded up to 256 bytes.  Two updates in flight on one handle would share it: one update at a time per
 * handle, as with the workspace.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_ADV_NORM_BATCH 0
#define SSG_ADV_NORM_MINIBATCH 1

/* Replaces nothing (memory binding; PPO2 behind train/stable_baselines/ppo.py:90 normalises on the host as it goes): the scratch size
 * for n_members members (1 for one policy).  SSG_ERR_BAD_ARG for NULL nbytes or n_members outside 1..SSG_POP_MAX_MEMBERS. */
int ssg_ppo_adv_norm_nbytes(int n_members, size_t *nbytes);

/* Replaces: the choice PPO2 makes in _train_step behind model.learn (train/stable_baselines/ppo.py:90) to normalise the advantages per
 * minibatch.  Binds the mode and the caller-owned, 256-byte aligned device scratch to the handle (host only, nothing launched); while
 * SSG_ADV_NORM_MINIBATCH is bound, ssg_ppo_grad, ssg_ppo_grad_ext, ssg_ppo_update, ssg_ppo_update_ext, ssg_pop_update,
 * ssg_pop_update_ext and ssg_pop_update_sched normalise per minibatch, and one of them called with more members than n_members is
 * refused (SSG_ERR_BAD_ARG, nothing launched).  SSG_ADV_NORM_BATCH unbinds (the other arguments are then not read).  SSG_ERR_BAD_ARG,
 * the binding left as it was: a NULL handle; an unknown mode; with SSG_ADV_NORM_MINIBATCH an n_members outside
 * 1..SSG_POP_MAX_MEMBERS, a NULL or misaligned dev_scratch, or scratch_nbytes below ssg_ppo_adv_norm_nbytes(n_members). */
int ssg_ppo_set_adv_norm(ssg_handle *h, int mode, int n_members, void *dev_scratch, size_t scratch_nbytes);

/* Replaces nothing (introspection; train/stable_baselines/ppo.py:90 has no such switch).  *mode = the bound mode, *n_members = the
 * member count its scratch serves (0 with SSG_ADV_NORM_BATCH). */
int ssg_ppo_get_adv_norm(const ssg_handle *h, int *mode, int *n_members);

/* ---------------------------------------------------------------------------------------------------
 * Job-wide per-minibatch advantage normalisation (ABI 9 addition): PPO2's rule for W ranks that train one policy
 * The Stable-Baselines script trains PPO2 over a SubprocVecEnv (train/stable_baselines/ppo.py:88-90,122-123): the minibatch PPO2
 * re-normalises over holds all workers' samples.  In a data-parallel job (ssg_ppo_apply_shards, below) minibatch (e, j) of the job is
 * the union of the ranks' minibatches (e, j), so its statistics are sums over the ranks.  The advantages are fixed once GAE has run and
 * a rank's permutations are known before its first gradient, so the sums of EVERY minibatch of an update are formed in one pass:
 *   1. ssg_ppo_minibatch_adv_sums: this shard's f64 rows {s, q, c, 0}, one per minibatch, two launches per update;
 *   2. the caller gathers the shards' row blocks (one all-gather per update, or a stack);
 *   3. ssg_ppo_set_minibatch_adv_rows: every rank adds the blocks in rank order and writes the same table of stats rows, one launch;
 *   4. ssg_ppo_set_adv_table binds the table; ahead of every local gradient call ssg_ppo_select_adv_row names the minibatch's row.
 * The per-minibatch loop exchanges nothing beyond the gradient rows it already gathers.
 *
 * Minibatch (e, j) of a shard is perm[e][j*chunk : min(n, (j+1)*chunk)], C = ceil(n / chunk) of them per epoch — the slice
 * ssg_ppo_update cuts — and its row is e*C + j.  s, q and c are the f64 sums of adv, adv^2 and 1 over the minibatch's indices inside
 * [0, n_samples), in the order ssg_ppo_set_adv_norm's two launches add them for a minibatch of that length M: B = min(64, ceil(M /
 * 1024)) workgroups, positions b*256 + t stepping by B*256, the 256-entry halving tree, then the tree over the B partials.  The grid of
 * the first launch is (B of the longest minibatch, epochs*C) x 256 threads, of the second epochs*C workgroups.  No floating-point
 * atomics, no host synchronisation.  The ranks' M may differ (unequal shards): each sums its own.
 *
 * The table's row b, with S, Q and C the sums over r = 0 .. W-1 of rows[r][b][0..2], added in f64 in rank order starting from rank 0's:
 *   C == 0: {0, 1, 1, 0};  else mean = S/C;  var = C > 1 ? max(0, (Q - S*mean) / (C - 1)) : 0;  std+ = (float)sqrt(var) + adv_eps;
 *   {(float)mean, std+, 1/std+, 0}
 * — SSG_ADV_NORM_MINIBATCH's formula, so with W = 1 the row is bit for bit what that mode writes for the minibatch.  The estimator
 * stays the unbiased one (PPO2's is the population std, as said above).
 *
 * A handle has ONE source of per-minibatch statistics: binding a table puts the mode back to SSG_ADV_NORM_BATCH, and a successful
 * ssg_ppo_set_adv_norm drops a bound table; neither refuses because of the other.  While a table is bound, ssg_ppo_grad and
 * ssg_ppo_grad_ext launch no statistics kernel and read {mean, std+, 1/std+} from dev_table + 4*row; ssg_ppo_apply_shards runs as ever
 * (it reads no advantage); ssg_ppo_update, ssg_ppo_update_ext and the ssg_pop_update* entry points are refused (SSG_ERR_BAD_ARG, after
 * everything else the host judges about the call): a table row is one minibatch's, and those calls run many.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_ADV_TABLE_MAX_ROWS 65535 /* minibatches of one ssg_ppo_minibatch_adv_sums call, rows of one table: a grid's second dimension */

/* Replaces nothing (memory binding; PPO2 behind train/stable_baselines/ppo.py:90 keeps its sums on the host): the size of
 * ssg_ppo_minibatch_adv_sums' partials scratch for n_batches minibatches, f64 [n_batches][64][3] rounded up to 256 bytes.
 * SSG_ERR_BAD_ARG for NULL nbytes or n_batches outside 1..SSG_ADV_TABLE_MAX_ROWS. */
int ssg_ppo_minibatch_adv_nbytes(int n_batches, size_t *nbytes);

/* Replaces: a worker's share of advs.mean() and advs.std() of every minibatch of one PPO2 update over a SubprocVecEnv
 * (train/stable_baselines/ppo.py:88-90,122-123), step 1 above.  dev_adv f32 [n_samples] (GAE's output, rows t*N + e), dev_perm int64
 * [epochs][n], dev_out f64 [epochs*C][4], dev_scratch 256-byte aligned, of ssg_ppo_minibatch_adv_nbytes(epochs*C) bytes.  An index
 * outside [0, n_samples) counts for nothing.  Two launches on `stream`.  SSG_ERR_BAD_ARG (nothing launched): NULL pointers; n_samples,
 * epochs, n or chunk < 1; chunk > n; epochs*C > SSG_ADV_TABLE_MAX_ROWS; a misaligned scratch or one too small.  SSG_ERR_NOT_BOUND
 * without a state blob. */
int ssg_ppo_minibatch_adv_sums(ssg_handle *h, int64_t n_samples, const float *dev_adv, const int64_t *dev_perm, int epochs, int64_t n,
                               int64_t chunk, double *dev_out, void *dev_scratch, size_t scratch_nbytes, void *stream);

/* Replaces: advs.mean() and advs.std() + 1e-8 of every minibatch of that update over all workers' samples
 * (train/stable_baselines/ppo.py:88-90,122-123), step 3 above.  dev_rows f64 [n_shards][n_batches][4] (the gathered blocks, rank
 * order), dev_table f32 [n_batches][4].  One lane per minibatch on ceil(n_batches / 256) workgroups of 256; one launch on `stream`.
 * SSG_ERR_BAD_ARG (nothing launched): NULL pointers, n_shards outside 1..SSG_DP_MAX_SHARDS (64), n_batches outside
 * 1..SSG_ADV_TABLE_MAX_ROWS, an adv_eps that is not finite.  SSG_ERR_NOT_BOUND without a state blob. */
int ssg_ppo_set_minibatch_adv_rows(ssg_handle *h, int n_shards, int n_batches, const double *dev_rows, double adv_eps, float *dev_table,
                                   void *stream);

/* Replaces nothing (memory binding; the minibatch PPO2 normalises behind train/stable_baselines/ppo.py:90 is its own).  Binds the
 * caller-owned, 16-byte aligned table f32 [n_rows][4] to the handle and selects row 0; a NULL dev_table unbinds (n_rows is not read).
 * Host only, nothing launched.  SSG_ERR_BAD_ARG, the binding left as it was: a NULL handle, a misaligned table, n_rows < 1. */
int ssg_ppo_set_adv_table(ssg_handle *h, float *dev_table /* NULL unbinds */, int n_rows);

/* Replaces nothing (the loop index of PPO2's minibatch loop behind train/stable_baselines/ppo.py:90): the row of the bound table the
 * next ssg_ppo_grad / ssg_ppo_grad_ext reads.  Host only.  SSG_ERR_BAD_ARG, the selection left as it was: a NULL handle, no table
 * bound, a row outside [0, n_rows). */
int ssg_ppo_select_adv_row(ssg_handle *h, int row);

/* Replaces nothing (introspection; train/stable_baselines/ppo.py:90 has no such binding).  The bound table (NULL: none), its rows and
 * the selected row (0 and 0 without a table). */
int ssg_ppo_get_adv_table(const ssg_handle *h, float **dev_table, int *n_rows, int *row);

/* ---------------------------------------------------------------------------------------------------
 * The minibatch permutations (ABI 9 addition): the shuffle of the update, drawn by the library
 * Both reference trainers shuffle inside their update: PPO2's learn runs np.random.shuffle(inds) once per epoch behind model.learn
 * (train/stable_baselines/ppo.py:90), and RLlib's SGD shuffles its minibatches the same way (train/rllib/pbt.py:50-62).  The update
 * entry points above read a dev_perm the caller made; these fill one, so that a C caller needs no sort and no generator of its own.
 *
 * Element i of a row is a pure function of (seed, update, member, epoch, n, i), n the row's length: a keyed 8-round Feistel network
 * over the smallest bit width b >= 8 with 2^b >= n, re-applied while the value is >= n (cycle walking); the round keys come from
 * (seed, update, member, epoch, n) through a 64-bit integer mixer.  csrc/shipsim_perm.h is the definition (and the argument why every
 * row is an exact permutation of [0, n)); the host entry and the kernel compile that one text, and ppo.perm_reference restates it in
 * numpy.  The rows are bitwise reproducible: they do not depend on the launch geometry, the stream, the device or the entry point.
 * `update` is the caller's count of updates (any value >= 0; the Python classes count their calls of update()), `member` the
 * population member (0 for one policy), `epoch` the row within the call.  The stream of values is this library's own: it is NOT
 * seed-compatible with numpy's or torch's generators, and no statistical claim beyond tests/test_perm.py's is made — it is a shuffle
 * for minibatches, not a cryptographic permutation.  1 <= n <= 2^32.
 *
 * The walk is capped at 256 applications; a lane that reached the cap would write -1, which the gradient kernels treat as a zero,
 * gradient-free sample.  csrc/shipsim_perm.h says why a row never holds one.
 * ------------------------------------------------------------------------------------------------- */
/* Replaces: np.random.shuffle(inds) of PPO2's learn (behind model.learn, train/stable_baselines/ppo.py:90), restated for the host; no
 * device is needed.  Writes elements [first, first + count) of the row keyed (seed, update, member, epoch) over [0, n) to out (int64
 * [count]).  SSG_ERR_BAD_ARG: NULL out; update, member or epoch < 0; n outside 1..2^32; first < 0, count < 1 or first + count > n. */
int ssg_host_perm(uint64_t seed, int64_t update, int member, int epoch, int64_t n, int64_t first, int64_t count, int64_t *out);

/* Replaces: the `noptepochs` shuffles of one PPO2 update (np.random.shuffle(inds) per epoch, train/stable_baselines/ppo.py:90).  Writes
 * dev_perm int64 [epochs][n_samples], the layout ssg_ppo_update / ssg_ppo_update_ext read: row e is the row keyed (seed, update, member,
 * e) over [0, n_samples), bit for bit ssg_host_perm's.  One launch on `stream`; no scratch, no atomics.  The arguments are judged first,
 * then the handle (SSG_ERR_NOT_BOUND without a state blob, like every call that launches).  SSG_ERR_BAD_ARG, nothing launched: a NULL
 * handle or dev_perm; update or member < 0; epochs < 1; n_samples outside 1..2^32. */
int ssg_ppo_perm(ssg_handle *h, uint64_t seed, int64_t update, int member, int epochs, int64_t n_samples, int64_t *dev_perm, void *stream);

/* Replaces: the same shuffles for every member of a population in ONE launch (each trial of train/rllib/pbt.py:50-62 shuffles its own
 * minibatches, and each of the three PPO2 models of train/stable_baselines/ppo.py:90 shuffles inside its learn).  Member m's rows are bit for bit ssg_ppo_perm(..., member = m, n_samples = K * n_m): a member is the single policy on
 * its shard here too.  Without slices bound to the handle: dev_perm int64 [members][perm_epochs][K * n], what ssg_pop_update /
 * ssg_pop_update_ext (perm_epochs = epochs) and ssg_pop_update_sched read on equal slices.  With slices bound (ssg_pop_set_slices):
 * the flat, unpadded layout ssg_pop_update_sched reads there — member m's block starts perm_epochs * (the samples K * n_j of the
 * members j < m) entries in and holds perm_epochs rows of K * n_m; `n` is not read.  perm_epochs * K * n_envs entries are written in
 * all.  SSG_ERR_BAD_ARG, nothing launched: a NULL handle or dev_perm; update < 0; K < 1; perm_epochs < 1; members outside
 * 1..SSG_POP_MAX_MEMBERS or different from the bound slices' member count; without slices n < 1; a row longer than 2^32. */
int ssg_pop_perm(ssg_handle *h, uint64_t seed, int64_t update, int members, int K, int n, int perm_epochs, int64_t *dev_perm, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Time-out bootstrap (ABI 9 addition): GAE that bootstraps a timed-out episode from the value of its terminal observation
 * The env ends an episode for five reasons (the SSG_EV_* bits); four are ends of the task, the fifth is the clock
 * (ship_env.py:131: step_count >= MAX_STEPS).  ssg_ppo_gae scores all five alike: delta = rew + gamma * 0 - val.  The observation
 * carries no clock, so the value network cannot tell a state at step 999 from the same state at step 3, yet gets targets several
 * units apart (the step reward is -0.01): the time-limit bias of Pardo et al. 2018, which Stable-Baselines3 and RLlib correct by
 * adding gamma * V(terminal observation) at a truncation.  This is that correction; it is opt-in, and with nothing bound and the
 * plain GAE entry points nothing changes.
 *
 * Sample (k, e) is a TIME-OUT when its flags byte f has (f & SSG_EV_MAX_STEPS) != 0 and (f & (SSG_EV_COLLIDING |
 * SSG_EV_OUT_OF_BOUNDS | SSG_EV_NO_GOALS_LEFT)) == 0; SSG_EV_GOAL_REACHED does not matter (a goal reached on the last allowed step,
 * with goals left, is still a time-out).  The bits are independent: a collision on the step that exhausts the clock carries both and
 * is a true terminal.  boot[k][e] = V(terminal observation of env e at step k) for a time-out, +0.0f for every other sample.
 *
 * The values cost ONE launch per rollout, not one per step.  While a record is bound (ssg_set_timeout_boot), ssg_rollout_policy /
 * ssg_pop_rollout point the step kernel's terminal-observation rows (ssg_set_terminal_obs) at row k of dev_term_obs_KND for step k,
 * put back whatever the caller had bound there once the loop is done, and after the last-value forward enqueue ssg_timeout_values /
 * ssg_pop_timeout_values over the K rows.  Every other output of the rollout, and the env state, is bit for bit what it is with
 * nothing bound.  Such a rollout needs dev_flags_KN and K <= rows (SSG_ERR_BAD_ARG otherwise), and refuses a capturing stream
 * (SSG_ERR_UNSUPPORTED: the handle's terminal-observation binding changes from step to step), each with nothing launched.
 *
 * Memory.  dev_term_obs_KND holds rows * n_envs * D * 8 bytes — 537 MB at 65 536 envs x 32 rows x D = 32, 67 MB at 4 096 x 64.  It is
 * written sparsely (the rows of the envs a step resets), read where a wave holds a time-out, allocated by the caller only when the
 * feature is on, and reused across rollouts.  Rows of envs that were not reset hold stale or never-written memory; the launch selects,
 * it never multiplies.
 * ------------------------------------------------------------------------------------------------- */
typedef struct ssg_timeout_boot {
    uint32_t struct_size;       /* sizeof(ssg_timeout_boot) */
    int32_t rows;               /* >= 1: the longest rollout (K) the buffers serve */
    double *dev_term_obs_KND;   /* f64 [rows][n_envs][D], D = history * (6 + n_beams), caller-owned; need not be initialised */
    float *dev_boot_KN;         /* f32, row k at k * step_stride_envs of the rollout (>= rows * step_stride_envs floats), caller-owned */
} ssg_timeout_boot;

/* Replaces: the `done` of ShipEnv.step at the clock (ship_env.py:131) as the trainers read it — nothing in the reference tells a
 * time-out from a terminal state (memory binding; the libraries' counterpart is the TimeLimit.truncated / terminal_observation entry
 * of the info dict).  Binds a copy of the record to the handle (host only, nothing launched); NULL unbinds.  The binding left as it
 * was: history > 2 is SSG_ERR_UNSUPPORTED and a handle without SSG_FLAG_AUTO_RESET SSG_ERR_BAD_ARG, as ssg_set_terminal_obs refuses
 * them; SSG_ERR_BAD_ARG for a struct_size mismatch, rows < 1 or a NULL buffer. */
int ssg_set_timeout_boot(ssg_handle *h, const ssg_timeout_boot *rec /* NULL unbinds */);

/* Replaces nothing (introspection).  *out = the bound record; out->struct_size == 0 (all of *out zero): nothing bound. */
int ssg_get_timeout_boot(const ssg_handle *h, ssg_timeout_boot *out /* struct_size 0: nothing bound */);

/* Replaces: the value of the terminal observation that Stable-Baselines3 / RLlib add at a truncation, for the episodes ShipEnv.step
 * ends at the clock (ship_env.py:131), over the K rows of a rollout in ONE launch on `stream`: grid (workgroups of 64 envs, 1, K).
 * A workgroup (one wave) reads its 64 flag bytes of row k (dev_flags_KN + k * step_stride_envs); with no time-out among them it
 * writes +0.0f for its envs and leaves; otherwise it runs ssg_policy_act's value-only forward (the vf tower alone with
 * SSG_POLICY_SEPARATE_VALUE, else the body and the v head; the fixed scale or the bound observation filter) on its rows of
 * dev_term_obs_KND + k * n_envs * D and writes, per env, the value for a time-out and +0.0f otherwise (a select).  Every entry
 * dev_boot_KN[k * step_stride_envs + e], k < K, e < n_envs, is written by every call: the buffer needs no clearing.  A time-out's
 * value is bit for bit what ssg_policy_act writes as dev_value for that observation row under the same parameters and filter
 * state.  A bound observation filter's state is read as the rollout left it (the state dev_last_value was computed under) and never
 * updated by this launch.  No record need be bound.  SSG_ERR_BAD_ARG (nothing launched): a bad policy record, a NULL buffer, K outside
 * 1..65535, step_stride_envs < n_envs, a bound filter of another member count. */
int ssg_timeout_values(ssg_handle *h, const ssg_policy *pol, int K, const uint8_t *dev_flags_KN, const double *dev_term_obs_KND,
                       float *dev_boot_KN, int64_t step_stride_envs, void *stream);

/* Replaces: the same for the trials of train/rllib/pbt.py:50-62, every member's in ONE launch: grid (workgroups of the widest slice,
 * members, K), member m on its columns [m n, (m + 1) n), n = n_envs / P, or its slice of ssg_pop_set_slices, under its parameter row
 * and its filter state rows.  Member m's entries are bit for bit ssg_timeout_values' on its shard.  Refuses as ssg_timeout_values
 * and as ssg_pop_act do. */
int ssg_pop_timeout_values(ssg_handle *h, const ssg_population *pop, int K, const uint8_t *dev_flags_KN, const double *dev_term_obs_KND,
                           float *dev_boot_KN, int64_t step_stride_envs, void *stream);

/* Replaces: the advantage / return computation behind model.learn (train/stable_baselines/ppo.py:90) with the truncation handled as
 * Stable-Baselines3's collect_rollouts does (ship_env.py:131 is where the clock ends an episode).  ssg_ppo_gae's arguments plus
 * dev_boot_KN (f32, rows N apart: ssg_timeout_values' output).  The walk, in f32, t = K-1 .. 0:
 *     nonterm = 1 - done;  v = val[i]
 *     tgt     = done ? boot[i] : nxt                        (a select)
 *     delta   = (rew[i] + gamma*tgt) - v
 *     adv     = delta + ((gamma*lam)*nonterm)*adv;  ret = adv + v;  nxt = v
 * The lambda chain is still cut at every done (the next row belongs to a new episode); only the one-step target changes.  The
 * advantage statistics and the partials' layout are ssg_ppo_gae's; with an all-zero boot, adv, ret and the statistics are bit for bit
 * ssg_ppo_gae's (finite inputs; rewards other than -0.0, which the env never pays).  Two launches.  Refuses as ssg_ppo_gae, and a NULL
 * dev_boot_KN. */
int ssg_ppo_gae_boot(ssg_handle *h, const ssg_ppo_hparams *hp, int K, int N, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                     const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN, float *dev_adv_KN,
                     float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream);

/* Replaces: the same for every trial of train/rllib/pbt.py:50-62 in two launches: ssg_pop_gae's arguments plus dev_boot_KN (rows
 * n_envs apart), on equal slices or the ssg_pop_set_slices layout; member m is bit for bit ssg_ppo_gae_boot on its shard with its own
 * gamma / lambda.  Refuses as ssg_pop_gae, and a NULL dev_boot_KN. */
int ssg_pop_gae_boot(ssg_handle *h, const ssg_population *pop, const float *dev_table, int K, const double *dev_reward_KN,
                     const uint8_t *dev_done_KN, const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN,
                     float *dev_adv_KN, float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Data parallel (additions to ABI 9): one policy trained from the experience of W env shards
 * The RLlib reference scripts collect experience on cpu_count() - 1 workers and train ONE policy from all of it
 * (train/rllib/ppo.py:34-35, train/rllib/pbt.py:57-58); the Stable-Baselines script does the same over a SubprocVecEnv
 * (train/stable_baselines/ppo.py:122-123).  Here every shard (a handle: a rank of ship_sim_gym_amd/sharding.py, or one of several handles
 * of one process) runs ssg_ppo_gae and, per minibatch, ssg_ppo_grad / ssg_ppo_grad_ext on its own samples; the caller gathers the
 * shards' rows (an all-gather, or a stack), and EVERY shard then runs the same two calls below on the same gathered rows in the same
 * order.  Same arithmetic on same inputs: the parameters, moments and KL coefficient stay bit-identical on all shards with no
 * parameter broadcast.  The library moves no data between devices; the gather is the caller's.
 *
 * Advantage statistics over the job.  ssg_ppo_gae leaves per-workgroup f64 partials of sum(adv) and sum(adv^2) at the start of the
 * workspace's slots; ssg_ppo_adv_moments re-adds them in the order the statistics launch used and returns the shard's moments
 * {S, Q, n, 0}.  The slots overwrite those partials once a gradient entry point runs: take the moments between GAE and the first
 * gradient.  ssg_ppo_set_adv_moments sums the gathered rows in row order (f64) and writes
 *   mean = S/n;  var = max(0, (Q - S*mean) / (n - 1));  std+ = (float)sqrt(var) + adv_eps;  {(float)mean, std+, 1/std+, 0}
 * where ssg_ppo_gae wrote its own: with one row, its own shard's, the head of the workspace is bit for bit what ssg_ppo_gae left.
 *
 * Apply.  Row r of dev_rows (f32 [W][P + 8]) holds shard r's gradient of its LOCAL minibatch of M_r samples (the mean-loss gradient
 * ssg_ppo_grad / ssg_ppo_grad_ext write; with the extended loss taken with max_grad_norm = 0, so unclipped and without a norm
 * launch), then that shard's stats row (the plain loss's four columns zero-padded to 8).  With w_r = (float)((double)M_r / (double)sum M),
 * formed on the host:
 *   g[p] = w_0*row_0[p];   g[p] = g[p] + w_r*row_r[p]  for r = 1 .. W-1
 * every product and every sum rounded to f32 on its own (no fused multiply-add): the mean-loss gradient of the job's minibatch.  Stats
 * columns 0..4 are combined the same way; column 6 is the KL coefficient in use, columns 5 and 7 as ssg_ppo_update_ext writes them.
 * With ext NULL only columns 0..3 are combined: columns 4..7 are written as zeros whatever the rows hold there.
 * One launch of ceil((P + 8) / 256) workgroups of 256, entry p on lane p % 256 of workgroup p / 256; without gradient-norm clipping it
 * ends with Adam step `step` (ssg_ppo_adam's constants and formula).  With ext->max_grad_norm > 0 each workgroup also forms the f64
 * sum of squares of its entries p < P (a halving tree), and the clip launch of ssg_ppo_update_ext follows: partials in index order,
 * norm = (float)sqrt(sum), coef = min(1, max_grad_norm / (norm + 1e-6f)), Adam on g*coef.  With ext the running f32 sum of mean(KL)
 * (a workspace word of this call's own: the shards' local gradient calls do not disturb it) is set on first_chunk and added to
 * otherwise; with last_chunk, a coefficient and kl_target > 0 the adaptation launch follows, dividing that sum by n_chunks — the
 * number of applies since first_chunk, this one included, which the caller states in the record.  With W = 1 all of this is bit
 * for bit what one minibatch of ssg_ppo_update / ssg_ppo_update_ext does to the parameters, moments, stats row and coefficient.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_DP_MAX_SHARDS 64
typedef struct ssg_ppo_shards {
    uint32_t struct_size;   /* sizeof(ssg_ppo_shards) */
    int32_t n_shards;       /* W in 1..SSG_DP_MAX_SHARDS */
    const float *dev_rows;  /* f32 [W][P + 8] on the device */
    const int64_t *counts;  /* HOST int64 [W]: M_r >= 1, the samples of shard r's minibatch */
    int32_t first_chunk;    /* the minibatch is the first of its epoch: the running KL sum restarts */
    int32_t last_chunk;     /* ... the last of the update: with kl_target > 0 and a coefficient the adaptation follows */
    int32_t n_chunks;       /* read with last_chunk when the adaptation runs: its divisor, >= 1 */
    int32_t reserved;       /* 0 */
} ssg_ppo_shards;

/* Replaces: the first half of the advantage standardisation RLlib applies to the experience its workers collected
 * (train/rllib/ppo.py:34-35: num_workers) — a shard's share of it.  Valid between ssg_ppo_gae / ssg_ppo_gae_boot over K x N and the
 * next gradient entry point on the same workspace.  Writes dev_out4 (f64 [4] on the device) = {S = sum adv, Q = sum adv^2,
 * (double)K*N, 0}.  One launch on `stream`.  SSG_ERR_BAD_ARG (nothing launched): NULL pointers, K < 1, N < 1 or a workspace too
 * small for ssg_ppo_gae over N envs. */
int ssg_ppo_adv_moments(ssg_handle *h, int K, int N, void *dev_workspace, size_t workspace_nbytes, double *dev_out4, void *stream);

/* Replaces: the second half — the statistics of the whole job's advantages (train/rllib/pbt.py:57-58 trains one policy from all
 * workers' samples), from the gathered moments dev_rows (f64 [n_shards][4], rows in shard order), into the workspace where the
 * gradient entry points read them.  One launch, one lane.  A job of fewer than 2 samples has no unbiased std: the device refuses it
 * by writing NaN statistics (a launch has no return code), which every later gradient shows.  SSG_ERR_BAD_ARG (nothing launched):
 * NULL pointers, n_shards outside 1..SSG_DP_MAX_SHARDS, an adv_eps that is not finite, a workspace of fewer than 256 bytes. */
int ssg_ppo_set_adv_moments(ssg_handle *h, int n_shards, const double *dev_rows /* [W][4] */, double adv_eps, void *dev_workspace,
                            size_t workspace_nbytes, void *stream);

/* Replaces: the SGD step RLlib's trainer takes on the batch gathered from its workers (train/rllib/ppo.py:34-35,
 * train/rllib/pbt.py:57-58) and PPO2's over its SubprocVecEnv (train/stable_baselines/ppo.py:122-123): the apply described above.
 * ext NULL: the plain loss (one launch, no workspace use beyond the check).  ext: its max_grad_norm, kl_target and dev_kl_coef are
 * read (the batch pointers are not); one launch, two with max_grad_norm > 0, one more for the adaptation.  dev_stats (nullable):
 * f32[8].  SSG_ERR_BAD_ARG (nothing launched): a bad policy, hparams, ext or shards record (struct_size, n_shards out of range,
 * reserved != 0, n_chunks < 1 where it is read), NULL dev_rows, counts or dev_adam_mv, a count < 1, step < 1, a workspace too small
 * (ssg_ppo_workspace_nbytes covers it), or SSG_ADV_NORM_MINIBATCH bound to the handle: that mode's statistics are one shard's.  The
 * job's per-minibatch statistics come from a table (ssg_ppo_set_adv_table, above), with which this call runs as ever. */
int ssg_ppo_apply_shards(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext /* nullable */,
                         const ssg_ppo_shards *sh, float *dev_adam_mv, int64_t step, float *dev_stats /* nullable */,
                         void *dev_workspace, size_t workspace_nbytes, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The update report (additions to ABI 9): how an update went, reduced on the device
 * The Stable-Baselines script's PPO2(..., verbose=1, tensorboard_log=tb_dir).learn(..., log_interval=10000)
 * (train/stable_baselines/ppo.py:88-90) prints and logs, per update, explained_variance, approxkl, clipfrac, policy_entropy,
 * policy_loss and value_loss; RLlib's PPO (train/rllib/ppo.py:26-41, train/rllib/pbt.py:47-74) reports vf_explained_var, kl, entropy,
 * policy_loss, vf_loss, cur_kl_coeff and cur_lr per iteration.  ssg_ppo_report / ssg_pop_report reduce a rollout's buffers to one f64
 * record of SSG_REPORT_COLS per policy, in two launches.
 *
 * The walk.  One lane per env, 256-env workgroups counted from the member's first env (ssg_ppo_gae's layout).  Lane e walks
 * t = 0 .. K-1 in ascending order over its column i = t*N + o_m + e, in f64, every product and sum rounded on its own (no fused
 * multiply-add), with r = (double)ret[i], v = (double)val[i], a = (double)adv[i], err = r - v:
 *     S_r += r;  Q_r += r*r;  S_e += err;  Q_e += err*err;  S_v += v;  S_a += a
 * and, with the post-update group (dev_logp_all_new given), d = logp_all_new[i][act[i] & 3] - logp[i] as ONE f32 subtraction:
 *     S_d += (double)d;  Q_d += (double)d * (double)d;  C += (d > hi || d < lo) ? 1 : 0
 * The clip decision is taken in the log domain, so the kernel runs no expf and has an exact restatement: lo = (float)log1p(-clip),
 * -inf from clip 1 on, hi = (float)log1p(clip), both formed on the host in double (ssg_report_clip_bounds).  This is PPO2's clipfrac
 * up to the rounding of the gradient kernel's fabsf(expf(d) - 1) > clip at the boundary.  Each workgroup reduces every sum with the
 * 256-entry halving tree (w = 128 .. 1) and writes one partial row per (member, block) into the scratch.
 *
 * The finish.  One workgroup per member: thread j adds the partials of blocks j, j + 256, ... in that order, then one more tree
 * (the order of ssg_ppo_gae's statistics launch).  The record, all in f64, with n = (double)K * n_m:
 *     [0]      n
 *     [1],[2]  mean(ret) = S_r/n;  var(ret) = max(0, (Q_r - S_r*mean) / n): the population variance (np.var)
 *     [3],[4]  mean(ret - val);  var(ret - val), the same formula
 *     [5]      explained variance = 1 - [4]/[2]; NaN when [2] == 0 (as Stable-Baselines' explained_variance)
 *     [6],[7]  mean(val);  mean(adv) (raw, before any normalisation)
 *     [8]      1.0 when the post-update group was computed, else 0.0 (then [9..11] are 0.0)
 *     [9]      approximate KL = -(S_d/n)
 *     [10]     PPO2's approxkl = 0.5 * (Q_d/n)
 *     [11]     C/n: the clip fraction over the whole batch under the post-update policy
 *     [12..19] the means of columns 0..7 of the member's stats rows (the f32 rows ssg_ppo_update(_ext) / ssg_pop_update* wrote: pg
 *              loss, value loss, entropy, clip fraction; with the extended loss KL, gradient norm, KL coefficient, unused): column c
 *              summed in f64 over its rows in row order by one thread, divided by the row count; 0.0 for columns the rows do not
 *              have, and for all eight when no rows are given (or the member's count is 0)
 *     [20]     the number of stats rows used
 *     [21..23] 0.0
 * No floating-point atomics, no host synchronisation, constant launch arguments (a capturing stream is fine).
 *
 * Contract.  The record depends on the inputs alone, bitwise: not on the stream or on earlier calls.  Member m's record of
 * ssg_pop_report is bit for bit ssg_ppo_report's on its shard (its columns as a [K][n_m] batch) with its bounds and its rows.  Equal
 * slices bound with ssg_pop_set_slices give bit for bit what an unbound handle gives.  The calls read their inputs only, and write
 * only the scratch and dev_out.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_REPORT_COLS 24
#define SSG_REPORT_EXPLAINED_VARIANCE 5
#define SSG_REPORT_POST 8
#define SSG_REPORT_STATS 12
#define SSG_REPORT_ROWS 20

/* Replaces nothing (host helper; the thresholds behind PPO2's clipfrac, train/stable_baselines/ppo.py:88-90, in the log domain).
 * out_lo_hi = {clip >= 1 ? -inf : (float)log1p(-clip), (float)log1p(clip)}, so that C and Python form the same bits.  Host only.
 * SSG_ERR_BAD_ARG for clip <= 0 (or NaN) or a NULL pointer. */
int ssg_report_clip_bounds(double clip, float out_lo_hi[2]);

/* Replaces nothing (sizing helper).  *nbytes = a scratch size that serves ssg_ppo_report over n_envs envs and ssg_pop_report for
 * n_members members on any slice layout of n_envs envs: n_members * ceil(n_envs / 256) partial rows of 9 doubles, rounded up to 256
 * bytes.  Host only.  SSG_ERR_BAD_ARG for an argument < 1, n_members > SSG_POP_MAX_MEMBERS or a NULL pointer. */
int ssg_ppo_report_workspace_nbytes(int n_envs, int n_members, size_t *nbytes);

/* Replaces: the per-update log of PPO2 (train/stable_baselines/ppo.py:88-90: explained_variance, approxkl, clipfrac, policy_entropy,
 * policy_loss, value_loss) and of RLlib's PPO (train/rllib/ppo.py:26-41: vf_explained_var, kl, entropy, policy_loss, vf_loss) for
 * one policy: the record above over the K x N batch (rows N apart; N is the batch's, not the handle's), into dev_out24 (f64
 * [SSG_REPORT_COLS] on the device).  dev_act, dev_logp and dev_logp_all_new (f32 [K*N][4]: an ssg_ppo_dist call made AFTER the
 * update) are nullable together; dev_stats (nullable) is f32 [n_rows][n_cols], n_cols 4 or 8.  The scratch needs
 * ceil(N / 256) * 9 doubles.  Two launches on `stream`.  SSG_ERR_BAD_ARG (nothing launched): a NULL handle, value, ret, adv, scratch
 * or out pointer; K < 1 or N < 1; one of dev_act / dev_logp / dev_logp_all_new given without the others; clip <= 0 with the
 * post-update group; n_cols not 4 or 8, or n_rows < 1, with dev_stats given; a scratch that is too small or not 256-byte aligned. */
int ssg_ppo_report(ssg_handle *h, int K, int N, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                   const int32_t *dev_act /* nullable */, const float *dev_logp /* nullable */,
                   const float *dev_logp_all_new /* nullable */, double clip, const float *dev_stats /* nullable */, int n_rows,
                   int n_cols, void *dev_scratch, size_t scratch_nbytes, double *dev_out24, void *stream);

/* Replaces: the same for every trial of train/rllib/pbt.py:47-74 in the same two launches: grid (blocks of the widest slice,
 * members).  The buffers are the [K][n_envs] ones of ssg_pop_gae; member m owns columns [m n, (m + 1) n), n = n_envs / P, or its
 * slice of ssg_pop_set_slices: unbound, n_envs % P != 0 is refused; slices bound for another P are refused.  dev_bounds (f32 [P][2]:
 * each member's lo, hi of ssg_report_clip_bounds) is required with the post-update group (dev_logp_all_new: ssg_pop_dist AFTER the
 * update).  dev_stats (nullable): f32 [P][rows_max][n_cols]; dev_rows (nullable): int32 [P], member m's own row count in
 * 0..rows_max, NULL meaning rows_max for all.  Rows past a member's count are never read (ssg_pop_update_sched leaves them
 * unwritten).  dev_out: f64 [P][SSG_REPORT_COLS].  The scratch needs P * ceil(widest slice / 256) * 9 doubles.  Refuses as
 * ssg_ppo_report, and n_members outside 1..SSG_POP_MAX_MEMBERS, a NULL dev_bounds with the post-update group. */
int ssg_pop_report(ssg_handle *h, int n_members, int K, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                   const int32_t *dev_act /* nullable */, const float *dev_logp /* nullable */,
                   const float *dev_logp_all_new /* nullable */, const float *dev_bounds /* [P][2] */,
                   const float *dev_stats /* nullable */, int rows_max, int n_cols, const int32_t *dev_rows /* nullable */,
                   void *dev_scratch, size_t scratch_nbytes, double *dev_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * The update report of a data-parallel job (additions to ABI 9): one record over the experience of all ranks
 * RLlib's vf_explained_var and kl are taken over the batch gathered from all workers (train/rllib/ppo.py:34-35), PPO2's over the whole
 * SubprocVecEnv (train/stable_baselines/ppo.py:88-90,122-123).  The walk above reduces a batch to nine raw f64 sums, and the record is
 * formed from those sums and the count alone; so every rank reduces its shard to one SUM ROW, the rows are all-gathered once per
 * update, and every rank forms the same record from the same rows in rank order (the pattern of ssg_ppo_adv_moments /
 * ssg_ppo_set_adv_moments).  A sum row is f64 [SSG_REPORT_ROW_COLS]:
 *     [0..8]  the walk's sums S_r, Q_r, S_e, Q_e, S_v, S_a, S_d, Q_d, C: bit for bit the totals the finish forms internally
 *     [9]     n = (double)K * (double)N
 *     [10]    1.0 when the post-update group was walked, else 0.0 (then [6..8] are 0.0)
 *     [11]    0.0
 * ssg_ppo_report_rows accumulates column c of the rows in f64 in row order, starting from row 0's value and adding rows 1 .. W-1; the
 * count n = sum n_r likewise; the record [0..11] then has the formulas above, and the stats columns [12..20] are formed as the finish
 * forms them (one thread per column, the stats rows in row order).  The post group is on when every row's [10] is 1.0 and off when
 * every row's is 0.0; rows that disagree are a caller's error that a launch cannot return, so [8..11] of the job's record are NaN.
 * One __device__ function turns {totals, n, post, stats sums} into the record for the finish and for ssg_ppo_report_rows alike.
 *
 * Contract.  With ONE row, that of ssg_ppo_report_sums on the same inputs, the record is bit for bit ssg_ppo_report's: with and without
 * the post group, with and without stats, NaN explained variance for constant returns included.  The record depends on the rows and
 * the stats alone.  No floating-point atomics, no host synchronisation, constant launch arguments.  ssg_ppo_report / ssg_pop_report
 * give what they gave.
 * ------------------------------------------------------------------------------------------------- */
#define SSG_REPORT_ROW_COLS 12

/* Replaces: a worker's share of the per-update log RLlib takes over the experience of all its workers (train/rllib/ppo.py:34-35) and
 * PPO2 over its SubprocVecEnv (train/stable_baselines/ppo.py:88-90,122-123): this shard's sum row into dev_row12 (f64
 * [SSG_REPORT_ROW_COLS] on the device).  The walk of ssg_ppo_report (the same kernels, grid and partials in the same scratch,
 * ssg_ppo_report_workspace_nbytes), then one workgroup: thread j adds the partials of blocks j, j + 256, ... in that order, the
 * 256-entry tree, plain stores.  Two launches on `stream`.  Refuses what ssg_ppo_report refuses (SSG_ERR_BAD_ARG, nothing launched);
 * dev_row12 stands for its dev_out24. */
int ssg_ppo_report_sums(ssg_handle *h, int K, int N, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                        const int32_t *dev_act /* nullable */, const float *dev_logp /* nullable */,
                        const float *dev_logp_all_new /* nullable */, double clip, void *dev_scratch, size_t scratch_nbytes,
                        double *dev_row12, void *stream);

/* Replaces: the per-update log over the batch gathered from all workers (train/rllib/ppo.py:34-35;
 * train/stable_baselines/ppo.py:88-90,122-123): the job's record from the gathered sum rows dev_rows (f64 [n_rows][SSG_REPORT_ROW_COLS],
 * shard order) into dev_out[0]; with per_shard != 0 also shard r's own view, formed from row r alone with the same stats columns,
 * into dev_out[1 + r].  dev_out: f64 [1 + (per_shard ? n_rows : 0)][SSG_REPORT_COLS].  dev_stats (nullable): f32
 * [n_stat_rows][n_cols], n_cols 4 or 8 — in a job the rows ssg_ppo_apply_shards wrote, identical on every rank.  One launch, one
 * 64-thread workgroup per record.  SSG_ERR_BAD_ARG (nothing launched, dev_out untouched): a NULL handle, rows or out pointer; n_rows
 * outside 1..SSG_DP_MAX_SHARDS; n_cols not 4 or 8, or n_stat_rows < 1, with dev_stats given. */
int ssg_ppo_report_rows(ssg_handle *h, int n_rows, const double *dev_rows, const float *dev_stats /* nullable */, int n_stat_rows,
                        int n_cols, int per_shard, double *dev_out, void *stream);

/* ---------------------------------------------------------------------------------------------------
 * Host-side geometry (what pymunk's cffi exposed at reset time); no GPU needed.
 * ------------------------------------------------------------------------------------------------- */
/* Replaces cpConvexHull as reached by pm.Poly(...) (models.py:96,180).  out_xy holds >= count pairs. */
int ssg_host_convex_hull(int count, const double *verts_xy, double *out_xy, int *out_count);
/* Replaces pm.moment_for_poly (models.py:89). */
int ssg_host_moment_for_poly(double mass, int count, const double *verts_xy, double *out);
/* Replaces Space.segment_query((W/2,y),(edge,y),10,filter)[0] over the two bank shapes (game.py:322-323):
 * hulls are the records' planes.  hit=0 -> the reference's IndexError fallback applies. */
int ssg_host_goal_x_range(const double *map_record, double width, double y, double *lo, double *hi, int *hit);
/* Builds one bank record from the two raw 12-gons of gen_river_poly (game_map.py:22-73) and the goal centres of
 * gen_goal_path (game.py:300-330): what PolyEnv.__init__ (models.py:153-196: pm.Poly hulls the points, one static shape per
 * bank) and add_goal (game.py:77-95) leave in the pm.Space at reset. */
int ssg_host_build_map(const double *left_xy, int n_left, const double *right_xy, int n_right,
                       const double *goals_xy, int n_goals, double spawn_x, double spawn_y, double *record_out);
/* Generic fat/thin segment query against one hull of a record (side 0 = left, 1 = right): cpShapeSegmentQuery as reached by
 * Shape.segment_query (the lidar beams, models.py:67, radius 0) and Space.segment_query (the goal path's fat rays,
 * game.py:322-323, radius 10). */
int ssg_host_segment_query(const double *map_record, int side, double ax, double ay, double bx, double by,
                           double radius, int *hit, double *px, double *py, double *alpha);

#ifdef __cplusplus
}
#endif
#endif /* SHIPSIM_H */
