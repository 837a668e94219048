// shipsim_api.cpp — the extern "C" boundary of libshipsim.so (include/shipsim.h) and the host-side geometry
// that pymunk's cffi layer provided to the reference at reset time (hulling, splitting planes, moments, the
// fat segment queries of gen_goal_path).  No torch types, no exceptions across the boundary.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "shipsim.h"
#include "shipsim_internal.h"
#include "shipsim_perm.h"

namespace {

// map_ring mode: the ring's source (fixed by ssg_refill_worlds), the refill's work queue in the blob, and how many more episodes an env
// may start before the rings must be refilled (an env consumes at most one world per step or reset).
struct MapRing {
    bool ready = false;
    int credit = 0;
    uint64_t seed = 0;
    double width_frac = 0.5;
    unsigned long long *queue = nullptr;
    unsigned *count = nullptr; // the queue's length
};

// The state blob's layout: every section's offset and size.  A section the config has no use for has size 0: no bytes, a null pointer.
struct Span { size_t off = 0, size = 0; };
struct BlobLayout {
    int n_pad = 0;
    size_t nbytes = 0;
    Span stats, f64, i32, mask;
    Span obs2, obsH;             // history > 2: the step kernel's two-frame staging rows, then the handle's own [n][H*F] observation rows
    Span ring_queue, ring_count; // map_ring: work queue of the ring refill, (env, episode) pairs + its length
    // config 4: columns of the traffic ships, goal bodies and cached arbiters (shipsim_internal.h DC_* / DU_*), the queue of the full step
    // (one array of n_pad slots per sort bucket, two sets of counters), the memo tables (the narrowphase memo follows the state memo)
    Span dyn_f64, dyn_live, dyn_u32, dyn_flag, dyn_hash, dyn_count, dyn_row, dyn_bucket, dyn_memo_stats, dyn_memo, dyn_npm, dyn_qmap;
};

// The one walk over the sections, from the (normalised) config: it builds the record and points the kernel arguments and the ring's queue
// into `blob` (null while none is bound; the pointer of a section that does not exist is never written and stays null).
BlobLayout blob_layout(const ssg_config &c, void *blob, ssg::DevCfg &d, MapRing &ring)
{
    BlobLayout L;
    L.n_pad = (c.n_envs + ssg::kPadEnvs - 1) / ssg::kPadEnvs * ssg::kPadEnvs;
    const size_t np = (size_t)L.n_pad, F = (size_t)(6 + c.n_beams);
    auto put = [&L, blob](auto *&p, Span &s, size_t bytes, size_t align = 1) {
        s = {(L.nbytes + align - 1) & ~(align - 1), bytes};
        L.nbytes = s.off + bytes;
        p = blob ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(static_cast<char *>(blob) + s.off) : nullptr;
    };
    put(d.stats, L.stats, ssg::kStatsDoubles * sizeof(double));
    put(d.f64cols, L.f64, (size_t)(ssg::COL_LIDAR + c.n_beams) * np * sizeof(double));
    put(d.i32cols, L.i32, (size_t)ssg::ICOL_COUNT * np * sizeof(int32_t));
    put(d.mask, L.mask, np);
    if (c.history > 2) {
        put(d.obs2, L.obs2, np * 2 * F * sizeof(double), 256);
        put(d.obsH, L.obsH, np * (size_t)c.history * F * sizeof(double));
    }
    if (c.map_ring > 0) {
        put(ring.queue, L.ring_queue, np * (size_t)c.map_ring * sizeof(unsigned long long), 256);
        put(ring.count, L.ring_count, 256);
    }
    if (c.n_ships > 1) {
        put(d.dyn_f64, L.dyn_f64, (size_t)ssg::DC_COUNT * np * sizeof(double), 256);
        put(d.dyn_live, L.dyn_live, np * sizeof(unsigned long long));
        put(d.dyn_u32, L.dyn_u32, (size_t)ssg::DU_COUNT * np * sizeof(uint32_t));
        put(d.dyn_flag, L.dyn_flag, np);
        put(d.dyn_hash, L.dyn_hash, np * sizeof(unsigned long long));
        put(d.dyn_count, L.dyn_count, (2 * (size_t)ssg::kDynCountWords * sizeof(unsigned) + 255) & ~(size_t)255);
        put(d.dyn_row, L.dyn_row, np * (size_t)ssg::kDynRow * sizeof(double));
        put(d.dyn_bucket, L.dyn_bucket, (size_t)ssg::kDynBuckets * np * sizeof(int32_t));
        put(d.dyn_memo_stats, L.dyn_memo_stats, (size_t)ssg::kMemoStatSlots * ssg::kMemoStatWords * sizeof(unsigned long long), 256);
        put(d.dyn_memo, L.dyn_memo, (size_t)ssg::kMemoEntries * ssg::kMemoStride * sizeof(unsigned long long));
        put(d.dyn_npm, L.dyn_npm, (size_t)ssg::kNpmEntries * ssg::kNpmStride * sizeof(unsigned long long));
        put(d.dyn_qmap, L.dyn_qmap, np * sizeof(int32_t));
    }
    return L;
}

// ssg_state_field's table.  Column j of a field starts (first_column + j) * n_pad elements into its section; a `packed` field is its
// section as one array, elements side by side.  columns 0: one per beam.  config4: n_ships == 4 only.
const struct FieldRow { int field, n_fields; Span BlobLayout::*section; int first_column, elem_size, columns; bool packed, config4; } kFields[] = {
    {SSG_F_X, 7, &BlobLayout::f64, ssg::COL_X, 8, 1, false, false}, // x, y, vx, vy, angle, w, cumulative reward: a column each, in this order
    {SSG_F_LIDAR, 1, &BlobLayout::f64, ssg::COL_LIDAR, 8, 0, false, false},
    {SSG_F_RUDDER, 3, &BlobLayout::i32, ssg::ICOL_RUDDER, 4, 1, false, false}, // rudder, step count, map id
    {SSG_F_GOAL_MASK, 1, &BlobLayout::mask, 0, 1, 1, false, false},
    // kStatsSlots rows of 4 int64 counters; sum over rows: [0] sum_return*100 [1] sum_length [2] episodes [3] goals
    {SSG_F_STATS, 1, &BlobLayout::stats, 0, 8, 4 * ssg::kStatsSlots, true, false},
    {SSG_F_TRAFFIC, 1, &BlobLayout::dyn_f64, ssg::DC_TRAFFIC, 8, 9 * SSG_N_TRAFFIC, false, true},
    {SSG_F_GOAL_BODIES, 1, &BlobLayout::dyn_f64, ssg::DC_GOALS, 8, ssg::DC_GOAL_COLS * SSG_MAX_GOALS, false, true},
    {SSG_F_DYN_FLAGS, 1, &BlobLayout::dyn_flag, 0, 1, 1, false, true},
    {SSG_F_EPISODES, 1, &BlobLayout::i32, ssg::ICOL_EPISODE, 4, 1, false, false},
    {SSG_F_DYN_MEMO_STATS, 1, &BlobLayout::dyn_memo_stats, 0, 8, ssg::kMemoStatSlots * ssg::kMemoStatWords, true, true},
    {SSG_F_DYN_LIVE, 1, &BlobLayout::dyn_live, 0, 8, 1, false, true},
    {SSG_F_DYN_ARB_META, 1, &BlobLayout::dyn_u32, ssg::DU_META, 4, ssg::kDynPairs, false, true},
    {SSG_F_DYN_ARB_HASH, 1, &BlobLayout::dyn_u32, ssg::DU_HASH, 4, ssg::kPolyPairs, false, true},
    {SSG_F_DYN_ARB_IMPULSE, 1, &BlobLayout::dyn_f64, ssg::DC_ARB, 8, 4 * ssg::kDynPairs, false, true},
};
static_assert(SSG_F_CUM_REWARD - SSG_F_X == ssg::COL_CUM - ssg::COL_X && SSG_F_MAP_ID - SSG_F_RUDDER == ssg::ICOL_MAP - ssg::ICOL_RUDDER, "the two runs of fields are runs of columns");

// The host's half of the config-4 step.  The step kernel's body role leaves, in one of two counter sets, the queue of envs whose bodies the
// NEXT full cpSpaceStep must visit; the full step consumes it or, when it cannot be trusted, rebuilds it from the per-env flags (a memset
// of the counters + the classify pass over every env: 12-19 us).  INVARIANT: the queue is trusted only while nothing on the host has
// touched the envs, the blob, the bank or the kernel arguments since the step kernel left it, except ONE masked reset that joined it.
// The memo of the full step (shipsim_internal.h, kMemoEntries) lives by GENERATIONS: a new one makes every stored entry count as empty.
constexpr int kMemoGenSteps = 1 << 15;
class DynStep {
    ssg::DevCfg &d; ssg::DynCfg &dyn; // the handle's kernel arguments: dyn_par, dyn_seq, dyn_memo_gen and bank_epoch are written here alone
    bool queue_valid = false;          // the step kernel's last launch left the next step's queue, and the invariant holds
    int masked_resets_since_step = 0;  // masked ssg_reset calls that joined the live queue since the last step (at most one may)
    unsigned memo_gen = 1;             // generation of the memo's entries (1..255; no memset: the generation is part of the tag)
    int memo_steps = 0;                // launches since it began
    bool memo_clear_pending = false;   // the tables must be zeroed before the next launch that could read them
    // A new generation is started whenever the bank changes (entries of the old bank could never match again and would only fill the table) and every
    // kMemoGenSteps launches (states a caller poked in once, or a long tail of rare ones, do not silt the table up).
    void new_generation() {
        if (++memo_gen > 255) { memo_gen = 1; memo_clear_pending = true; } // a wrapped generation could meet its own old tags
        memo_steps = 0;
        d.dyn_memo_gen = memo_gen;
    }

public:
    DynStep(ssg::DevCfg &dev, ssg::DynCfg &dyn_cfg) : d(dev), dyn(dyn_cfg) {}
    // (ssg_debug_dyn_counters) launches of the full step so far, and those that rebuilt the queue from the per-env flags first
    unsigned long long launches = 0, classifies = 0;
    void args_refreshed() { d.dyn_par = 0; d.dyn_memo_gen = memo_gen; d.dyn_seq = launches; queue_valid = false; }
    // A blob was bound, or the bound one may have been copied or restored: its memo tables may hold another bank's or handle's results under
    // this handle's generation (the key names the record, not the bank's contents): zeroed before the next launch that could read them.
    void blob_rebound() { new_generation(); memo_clear_pending = true; queue_valid = false; }
    // The blob was zeroed, some envs were edited, or a launch failed (a queue never consumed, or never written): the next step starts over.
    void queue_lost() { queue_valid = false; }
    // A new bank, or the bound one regenerated in place: resting traffic must be re-collided against the new banks.
    void bank_changed() { dyn.bank_epoch++; new_generation(); queue_valid = false; }
    // A reset arrives; true: it JOINS the queue the step kernel left (the RLlib flow resets its done envs with a masked reset after every
    // step).  One such reset per step: every env then has at most one entry per sort bucket, which is what a bucket's n_pad slots hold; a
    // second one, a full reset, or a queue that is not there rebuild it.  And only where the full step runs its one-record-per-wave kernel
    // (shared banks of at most kDynMapBuckets records): that kernel drops an entry queued under another record than the env now sits on,
    // and a record IS its map bucket there.  The per-lane-planes kernel (larger banks, map_ring) cannot tell a stale entry from the new
    // one — both would be stepped, by different waves: an env's bodies could advance twice in one step — so it rebuilds after any reset.
    bool reset_arrives(bool masked, bool one_record_per_wave) {
        const bool join = masked && queue_valid && masked_resets_since_step == 0 && one_record_per_wave;
        if (join) masked_resets_since_step = 1;
        else queue_valid = false;
        return join;
    }
    // A full step begins: *rebuild says whether its classify pass rebuilds the queue (this step's bucket counters then start from zero);
    // the memo's generation moves on, and the memsets the launch needs are issued (memo_bytes: both tables, one behind the other).
    hipError_t step_begins(size_t memo_bytes, hipStream_t st, bool *rebuild) {
        hipError_t e = hipSuccess;
        *rebuild = !queue_valid;
        if (*rebuild) {
            d.dyn_par = 0;
            classifies++;
            e = hipMemsetAsync(d.dyn_count, 0, ssg::kDynCountWords * sizeof(unsigned), st);
        }
        if (d.dyn_memo) {
            if (++memo_steps > kMemoGenSteps) new_generation();
            if (memo_clear_pending && e == hipSuccess) {
                e = hipMemsetAsync(d.dyn_memo, 0, memo_bytes, st);
                memo_clear_pending = false;
            }
        }
        d.dyn_seq = ++launches;
        return e;
    }
    // Both launches of a step went out: the step kernel's body role queues the envs whose bodies must be stepped next, in the other set.
    void step_issued() { queue_valid = true; masked_resets_since_step = 0; d.dyn_par ^= 1; }
};

} // namespace

struct ssg_handle {
    // configuration and the kernel arguments derived from it (refresh_dev)
    ssg_config cfg;
    ssg::DevCfg dev{};
    ssg::DynCfg dyn{};
    // the bound blob and its layout; the bank
    BlobLayout layout;
    void *state = nullptr;
    bool zeroed = false;        // the bound blob is known to have been zeroed by us (ssg_init_state / first full reset)
    const double *bank = nullptr;
    int n_maps = 0;
    bool remap_pending = false; // the bank shrank: ICOL_MAP must be taken modulo n_maps before the next kernel reads it
    // launch geometry (ssg_set_map_bank), and which kernels have their dynamic-LDS limit set: the step kernels, the policy kernel
    // (ssg_policy_act / ssg_rollout_policy), the gradient kernel (ssg_ppo_grad / ssg_ppo_update), the FILTER and the time-out kernels
    int block = 256;
    bool lds = false;
    size_t lds_bytes = 0;
    bool prepared = false, policy_prepared = false, ppo_prepared = false, policy_filter_prepared = false, policy_boot_prepared = false;
    // config 4: the host's half of the step; ssg_debug_kernel_times (HIP events around the two launches of every config-4 step)
    DynStep dyn_step{dev, dyn};
    bool time_kernels = false;
    double t_dyn_ms = 0.0, t_step_ms = 0.0;
    unsigned long long t_steps = 0;
    MapRing ring;
    // ssg_step_host / ssg_wait_host: one completion event per host block slot, created on first use
    static constexpr int kHostSlots = 8;
    hipEvent_t host_ev[kHostSlots] = {};
    bool host_ev_made[kHostSlots] = {};
    // bound records.  ssg_pop_set_slices: the members' env counts (empty: nothing bound), the caller's device table, the largest and smallest slice
    std::vector<int32_t> pop_sizes;
    const int32_t *dev_slices = nullptr;
    int slice_max = 0, slice_min = 0;
    ssg_obs_filter flt{};     // ssg_set_obs_filter (these three: a copy; struct_size 0: nothing bound)
    double *flt_buffer = nullptr; // ssg_set_obs_filter_buffer: the bound filter's job buffer (NULL: none; every ssg_set_obs_filter drops it)
    ssg_timeout_boot tob{};   // ssg_set_timeout_boot
    ssg_eval_recorder rec{};  // ssg_set_eval_recorder, its env_ids pointing at the copy beside it
    ssg::EvalRecIds rec_ids{};
    // ssg_ppo_set_adv_norm: the mode (SSG_ADV_NORM_BATCH: nothing bound), the member count the scratch serves and the caller's scratch
    int adv_norm_mode = SSG_ADV_NORM_BATCH, adv_norm_members = 0;
    void *adv_norm_scratch = nullptr;
    // ssg_ppo_set_adv_table: the job's table of per-minibatch stats rows f32 [adv_table_rows][4] (NULL: none) and the selected row;
    // bound only while the mode above is SSG_ADV_NORM_BATCH — a handle has one source of per-minibatch statistics at a time
    float *adv_table = nullptr;
    int adv_table_rows = 0, adv_table_row = 0;
    std::string err;
};

namespace {

thread_local std::string g_err; // errors raised before a handle exists

int fail(ssg_handle *h, int code, const std::string &msg)
{
    if (h) h->err = msg;
    else g_err = msg;
    return code;
}

// ---------------------------------------------------------------------------------------------------------
// host geometry
// ---------------------------------------------------------------------------------------------------------
struct P2 { double x, y; };
inline double cross3(const P2 &o, const P2 &a, const P2 &b) { return (a.x - o.x) * (b.y - o.y) - (a.y - o.y) * (b.x - o.x); }

// Strict convex hull, counter-clockwise, first vertex = lexicographic (x, then y) minimum: the vertex order
// cpConvexHull (QuickHull, tol 0) hands to cpPolyShape.  Implemented as Andrew's monotone chain.
std::vector<P2> convex_hull(std::vector<P2> pts)
{
    std::sort(pts.begin(), pts.end(), [](const P2 &a, const P2 &b) { return a.x < b.x || (a.x == b.x && a.y < b.y); });
    pts.erase(std::unique(pts.begin(), pts.end(), [](const P2 &a, const P2 &b) { return a.x == b.x && a.y == b.y; }),
              pts.end());
    const int n = (int)pts.size();
    if (n <= 2) return pts;
    std::vector<P2> h(2 * n);
    int k = 0;
    for (int i = 0; i < n; ++i) { // lower chain
        while (k >= 2 && cross3(h[k - 2], h[k - 1], pts[i]) <= 0.0) --k;
        h[k++] = pts[i];
    }
    for (int i = n - 2, t = k + 1; i >= 0; --i) { // upper chain
        while (k >= t && cross3(h[k - 2], h[k - 1], pts[i]) <= 0.0) --k;
        h[k++] = pts[i];
    }
    h.resize(k - 1);
    return h;
}

struct Plane { double v0x, v0y, nx, ny, v0n, dtmin, dtmax; };

// cpPolyShape SetVerts: plane i = { v0 = v[i], n = normalize(rperp(v[i] - v[i-1])) }, rperp(x,y) = (y,-x),
// normalize(v) = v * (1/(|v| + DBL_MIN)); plus the constants cpPolyShapeSegmentQuery derives per plane.
std::vector<Plane> planes_of(const std::vector<P2> &v)
{
    const int n = (int)v.size();
    std::vector<Plane> pl(n);
    for (int i = 0; i < n; ++i) {
        const P2 &a = v[(i - 1 + n) % n], &b = v[i];
        const double ex = b.x - a.x, ey = b.y - a.y;
        const double rx = ey, ry = -ex;
        const double inv = 1.0 / (std::sqrt(rx * rx + ry * ry) + DBL_MIN);
        Plane p;
        p.v0x = b.x; p.v0y = b.y;
        p.nx = rx * inv; p.ny = ry * inv;
        pl[i] = p;
    }
    for (int i = 0; i < n; ++i) {
        Plane &p = pl[i];
        const P2 &prev = v[(i - 1 + n) % n];
        p.v0n = p.v0x * p.nx + p.v0y * p.ny;          // cpvdot(v0, n)
        p.dtmin = p.nx * prev.y - p.ny * prev.x;      // cpvcross(n, v[i-1])
        p.dtmax = p.nx * p.v0y - p.ny * p.v0x;        // cpvcross(n, v[i])
    }
    return pl;
}

struct HullView {
    int n;
    const double *pl; // n planes of SSG_PLANE_DOUBLES doubles
    double v0x(int i) const { return pl[SSG_PLANE_DOUBLES * i + 0]; }
    double v0y(int i) const { return pl[SSG_PLANE_DOUBLES * i + 1]; }
    double nx(int i) const { return pl[SSG_PLANE_DOUBLES * i + 2]; }
    double ny(int i) const { return pl[SSG_PLANE_DOUBLES * i + 3]; }
    double v0n(int i) const { return pl[SSG_PLANE_DOUBLES * i + 4]; }
    // cpPolyShapeSegmentQuery's edge extents: cpvcross(n, v[i-1]) and cpvcross(n, v[i])
    double dtmin(int i) const { const int p = (i - 1 + n) % n; return nx(i) * v0y(p) - ny(i) * v0x(p); }
    double dtmax(int i) const { return nx(i) * v0y(i) - ny(i) * v0x(i); }
};

inline double clamp01(double f) { return std::max(0.0, std::min(f, 1.0)); }

// cpPolyShapePointQuery (radius 0): signed distance of p to the hull and the closest boundary point.
double point_query(const HullView &h, double px, double py, double *cx, double *cy)
{
    double v0x = h.v0x(h.n - 1), v0y = h.v0y(h.n - 1);
    double best = INFINITY, bx = 0, by = 0;
    bool outside = false;
    for (int i = 0; i < h.n; ++i) {
        const double v1x = h.v0x(i), v1y = h.v0y(i);
        outside = outside || ((h.nx(i) * (px - v1x) + h.ny(i) * (py - v1y)) > 0.0);
        const double dx = v0x - v1x, dy = v0y - v1y;
        const double t = clamp01((dx * (px - v1x) + dy * (py - v1y)) / (dx * dx + dy * dy));
        const double qx = v1x + dx * t, qy = v1y + dy * t;
        const double ex = px - qx, ey = py - qy;
        const double d = std::sqrt(ex * ex + ey * ey);
        if (d < best) { best = d; bx = qx; by = qy; }
        v0x = v1x; v0y = v1y;
    }
    if (cx) *cx = bx;
    if (cy) *cy = by;
    return outside ? best : -best;
}

struct SegHit { bool hit; double px, py, alpha; };

// cpShapeSegmentQuery -> cpPolyShapeSegmentQuery + CircleSegmentQuery for the bevelled corners (poly radius 0,
// query radius r2), as Space.segment_query / Shape.segment_query reach it.
SegHit segment_query(const HullView &h, double ax, double ay, double bx, double by, double r2)
{
    SegHit out{false, bx, by, 1.0};
    if (point_query(h, ax, ay, nullptr, nullptr) <= r2) {
        out.hit = true;
        out.alpha = 0.0;
        return out; // reported point stays the far end b
    }
    for (int i = 0; i < h.n; ++i) {
        const double nx = h.nx(i), ny = h.ny(i);
        const double an = ax * nx + ay * ny;
        const double d = an - h.v0n(i) - r2;
        if (d < 0.0) continue;
        const double bn = bx * nx + by * ny;
        const double t = d / std::max(an - bn, DBL_MIN);
        if (t < 0.0 || 1.0 < t) continue;
        const double omt = 1.0 - t;
        const double ptx = ax * omt + bx * t, pty = ay * omt + by * t;
        const double dtv = nx * pty - ny * ptx;
        if (h.dtmin(i) <= dtv && dtv <= h.dtmax(i)) {
            out.hit = true;
            out.px = ptx - nx * r2;
            out.py = pty - ny * r2;
            out.alpha = t;
        }
    }
    if (r2 > 0.0) {
        for (int i = 0; i < h.n; ++i) {
            const double cx = h.v0x(i), cy = h.v0y(i);
            const double dax = ax - cx, day = ay - cy, dbx = bx - cx, dby = by - cy;
            const double daa = dax * dax + day * day, dab = dax * dbx + day * dby, dbb = dbx * dbx + dby * dby;
            const double qa = daa - 2.0 * dab + dbb;
            const double qb = dab - daa;
            const double det = qb * qb - qa * (daa - r2 * r2);
            if (det >= 0.0) {
                const double t = (-qb - std::sqrt(det)) / qa;
                if (0.0 <= t && t <= 1.0 && t < out.alpha) {
                    const double omt = 1.0 - t;
                    double nx = dax * omt + dbx * t, ny = day * omt + dby * t;
                    const double inv = 1.0 / (std::sqrt(nx * nx + ny * ny) + DBL_MIN);
                    nx *= inv; ny *= inv;
                    out.hit = true;
                    out.px = (ax * omt + bx * t) - nx * r2;
                    out.py = (ay * omt + by * t) - ny * r2;
                    out.alpha = t;
                }
            }
        }
    }
    return out;
}

HullView hull_of_record(const double *rec, int side)
{
    return HullView{(int)rec[SSG_MAP_OFF_COUNTS + side],
                    rec + SSG_MAP_OFF_PLANES + side * (SSG_MAX_HULL * SSG_PLANE_DOUBLES)};
}

const double kShipTemplate[SSG_SHIP_VERTS][2] = {{0, 0}, {0, 10}, {5, 15}, {10, 10}, {10, 0}}; // models.py:6

double moment_for_poly(double m, int n, const double *v)
{
    // cpMomentForPoly, offset (0,0): about the local origin
    double sum1 = 0.0, sum2 = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x1 = v[2 * i], y1 = v[2 * i + 1];
        const int j = (i + 1) % n;
        const double x2 = v[2 * j], y2 = v[2 * j + 1];
        const double a = x2 * y1 - y2 * x1;
        const double b = (x1 * x1 + y1 * y1) + (x1 * x2 + y1 * y2) + (x2 * x2 + y2 * y2);
        sum1 += a * b;
        sum2 += a;
    }
    return (m * sum1) / (6.0 * sum2);
}

int set_ship(ssg_config *cfg, double ws, double hs, double mass)
{
    double pts[2 * SSG_SHIP_VERTS];
    std::vector<P2> v(SSG_SHIP_VERTS);
    for (int i = 0; i < SSG_SHIP_VERTS; ++i) {
        pts[2 * i] = kShipTemplate[i][0] * ws;
        pts[2 * i + 1] = kShipTemplate[i][1] * hs;
        v[i] = P2{pts[2 * i], pts[2 * i + 1]};
    }
    const double moment = moment_for_poly(mass, SSG_SHIP_VERTS, pts); // on the template order, as models.py:88-89
    std::vector<P2> hull = convex_hull(v);
    if ((int)hull.size() != SSG_SHIP_VERTS) return SSG_ERR_BAD_ARG;
    std::vector<Plane> pl = planes_of(hull);
    for (int i = 0; i < SSG_SHIP_VERTS; ++i) {
        cfg->ship_hull[2 * i] = hull[i].x;
        cfg->ship_hull[2 * i + 1] = hull[i].y;
        cfg->ship_normals[2 * i] = pl[i].nx;
        cfg->ship_normals[2 * i + 1] = pl[i].ny;
    }
    cfg->ship_m_inv = 1.0 / mass;
    cfg->ship_i_inv = 1.0 / moment;
    return SSG_OK;
}

// ShipGame.add_default_traffic (game.py:279-286): add_ship(x, y, width, height) -> Ship.__init__ (models.py:87-111),
// mass = the Ship default, moment about the local origin, hull in cpConvexHull order; plus Chipmunk's space defaults.
int set_traffic(ssg_handle *h)
{
    static const double kTraffic[SSG_N_TRAFFIC][4] = {{100, 200, 1, 1}, {300, 200, 1.5, 2}, {400, 350, 1, 3}};
    ssg::DynCfg &d = h->dyn;
    const double mass = 1.0 / h->cfg.ship_m_inv;
    for (int k = 0; k < SSG_N_TRAFFIC; ++k) {
        ssg_config tmp = h->cfg;
        const int rc = set_ship(&tmp, kTraffic[k][2], kTraffic[k][3], mass);
        if (rc != SSG_OK) return rc;
        std::memcpy(d.thull[k], tmp.ship_hull, sizeof(d.thull[k]));
        std::memcpy(d.tnrm[k], tmp.ship_normals, sizeof(d.tnrm[k]));
        d.t_i_inv[k] = tmp.ship_i_inv;
        d.tx[k] = kTraffic[k][0];
        d.ty[k] = kTraffic[k][1];
    }
    d.t_m_inv = h->cfg.ship_m_inv;
    // add_goal (game.py:77-95): mass 1, pm.moment_for_circle(1, 0, radius) = m * 0.5 * (r1^2 + r2^2)
    d.goal_m_inv = 1.0 / 1.0;
    d.goal_i_inv = 1.0 / (1.0 * 0.5 * (0.0 * 0.0 + h->cfg.goal_radius * h->cfg.goal_radius));
    d.ship_friction = 0.7;                                      // models.py:98
    d.slop = 0.1;                                               // cpSpace collisionSlop
    d.bias_coef = 1.0 - std::pow(std::pow(1.0 - 0.1, 60.0), h->cfg.dt); // 1 - collisionBias^dt (cpSpaceStep)
    return SSG_OK;
}

void refresh_dev(ssg_handle *h)
{
    const ssg_config &c = h->cfg;
    ssg::DevCfg &d = h->dev;
    d.n_envs = c.n_envs;
    d.env_id_base = c.env_id_base;
    d.n_beams = c.n_beams;
    d.history = c.history < 2 ? c.history : 2;
    d.full_history = c.history;
    d.max_steps = c.max_steps;
    d.n_goals = c.n_goals;
    d.flags = c.flags;
    d.n_maps = h->n_maps;
    d.map_ring = c.map_ring;
    d.rudder_step = c.rudder_step;
    d.rudder_max = c.rudder_max;
    d.spread_deg = c.lidar_spread_deg;
    d.lidar_dist = c.lidar_dist;
    d.goal_r = c.goal_radius;
    d.width = c.width;
    d.height = c.height;
    d.dt = c.dt;
    d.damp = c.damping_pow_dt;
    d.spawn_x = c.spawn_x;
    d.spawn_y = c.spawn_y;
    std::memcpy(d.hull, c.ship_hull, sizeof(d.hull));
    std::memcpy(d.nrm, c.ship_normals, sizeof(d.nrm));
    d.m_inv = c.ship_m_inv;
    d.i_inv = c.ship_i_inv;
    d.force_y = c.force_y;
    d.px0 = c.thrust_px0;
    d.py0 = c.thrust_py0;
    {
        // LiDAR.query (models.py:48-49,62): rotation_i = angle + rad(90 - spread/2) + rad(spread/n_beams) * i
        const double deg2rad = 0.017453292519943295; // CPython math.radians: pi/180
        const double delta = (c.lidar_spread_deg / (double)c.n_beams) * deg2rad;
        const double phi0 = (90.0 - c.lidar_spread_deg / 2) * deg2rad;
        for (int i = 0; i < SSG_MAX_BEAMS; ++i) {
            const double phi = phi0 + delta * (double)i;
            d.beam_cos[i] = std::cos(phi);
            d.beam_sin[i] = std::sin(phi);
        }
    }
    h->layout = blob_layout(c, h->state, d, h->ring);
    d.n_pad = h->layout.n_pad;
    d.bank = h->bank;
    d.n_ships = c.n_ships;
    // the memo: shared bank records are what makes states repeat (not per-env worlds; the key holds 16 bits of record index)
    if ((c.flags & SSG_FLAG_DYN_MEMO_OFF) || c.map_ring != 0 || h->n_maps <= 0 || h->n_maps > 65536) d.dyn_memo = d.dyn_npm = nullptr;
    {   // every constant the full step reads, folded into 16 bits of the memo key
        unsigned long long fp = 0xcbf29ce484222325ull;
        auto eat = [&](const void *p, size_t n) { const unsigned char *b = static_cast<const unsigned char *>(p); for (size_t i = 0; i < n; ++i) fp = (fp ^ b[i]) * 0x100000001b3ull; };
        eat(h->dyn.thull, sizeof h->dyn.thull); eat(h->dyn.tnrm, sizeof h->dyn.tnrm); eat(h->dyn.tx, sizeof h->dyn.tx); eat(h->dyn.ty, sizeof h->dyn.ty);
        eat(h->dyn.t_i_inv, sizeof h->dyn.t_i_inv); eat(&h->dyn.t_m_inv, 8); eat(&h->dyn.goal_m_inv, 8); eat(&h->dyn.goal_i_inv, 8);
        eat(&h->dyn.ship_friction, 8); eat(&h->dyn.bias_coef, 8); eat(&h->dyn.slop, 8);
        eat(&c.dt, 8); eat(&c.damping_pow_dt, 8); eat(&c.goal_radius, 8); eat(&c.n_goals, 4);
        h->dyn.memo_fp = (unsigned)((fp ^ (fp >> 16) ^ (fp >> 32) ^ (fp >> 48)) & 0xFFFFu);
    }
    {   // the step kernel's reject in front of collide_ship's exact player x traffic test: no vertex of ship k's hull is further than
        // its hull radius from its body position
        auto radius = [](const double *hull) {
            double r2 = 0.0;
            for (int i = 0; i < SSG_SHIP_VERTS; ++i) r2 = std::max(r2, hull[2 * i] * hull[2 * i] + hull[2 * i + 1] * hull[2 * i + 1]);
            return std::sqrt(r2);
        };
        for (int k = 0; k < SSG_N_TRAFFIC; ++k) {
            const double r = radius(h->dyn.thull[k]) * 1.001 + 1.0;
            d.dyn_reach2[k] = r * r;
        }
        std::memcpy(d.thull, h->dyn.thull, sizeof(d.thull));
        std::memcpy(d.tnrm, h->dyn.tnrm, sizeof(d.tnrm));
    }
    h->dyn_step.args_refreshed();
}

int pick_block(int n_envs)
{
    if (const char *s = std::getenv("SSG_BLOCK")) {
        const int b = std::atoi(s);
        if (b == 64 || b == 128 || b == 256) return b;
    }
    // Envs per workgroup (the workgroup has twice as many threads: role-split waves).  MI355X has 256 CUs and a
    // workgroup that stages the bank owns its CU's LDS: aim for >= 256 workgroups before growing them.
    if (n_envs <= 64 * 256) return 64;
    if (n_envs <= 128 * 256) return 128;
    return 256;
}

// Config 4 and map_ring launches carry per-call HOST state in their kernel arguments (which counter set holds the live queue, the
// launch number the memo's entries are stamped with, the ring's credit): captured into a HIP graph they would be replayed with
// the arguments of the captured call — silently wrong steps.  Refuse a capturing stream for those handles.  (1-ship handles on a
// shared bank launch with constant arguments and can be captured.)
int refuse_capture(ssg_handle *h, void *stream, const char *what)
{
    if (h->cfg.n_ships <= 1 && h->cfg.map_ring <= 0 && h->cfg.history <= 2) return SSG_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(static_cast<hipStream_t>(stream), &cs) != hipSuccess) { (void)hipGetLastError(); return SSG_OK; }
    if (cs == hipStreamCaptureStatusNone) return SSG_OK;
    return fail(h, SSG_ERR_UNSUPPORTED, std::string(what) + ": the stream is capturing a HIP graph, and this handle's launches (n_ships > 1, map_ring or "
                                        "history > 2) take per-call host state in their arguments — a replay would repeat the captured step's");
}

int check_ready(ssg_handle *h, bool need_bank)
{
    if (!h) return SSG_ERR_BAD_ARG;
    if (!h->state) return fail(h, SSG_ERR_NOT_BOUND, "no state blob bound: call ssg_bind_state first");
    if (need_bank && (!h->bank || h->n_maps <= 0))
        return fail(h, SSG_ERR_NOT_BOUND, "no map bank set: call ssg_set_map_bank first");
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(h, SSG_ERR_NO_DEVICE, std::string("hipGetDevice: ") + hipGetErrorString(e));
    if (dev != h->cfg.device_id) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "current HIP device %d differs from the handle's device %d", dev,
                      h->cfg.device_id);
        return fail(h, SSG_ERR_BAD_ARG, buf);
    }
    return SSG_OK;
}

} // namespace

extern "C" {

int ssg_abi_version(void) { return SSG_ABI_VERSION; }

const char *ssg_strerror(int status)
{
    switch (status) {
    case SSG_OK: return "ok";
    case SSG_ERR_BAD_ARG: return "bad argument";
    case SSG_ERR_HIP: return "HIP runtime error";
    case SSG_ERR_NOT_BOUND: return "state or map bank not bound";
    case SSG_ERR_UNSUPPORTED: return "unsupported configuration";
    case SSG_ERR_NO_DEVICE: return "no usable HIP device";
    default: return "unknown status";
    }
}

const char *ssg_last_error(const ssg_handle *h) { return h ? h->err.c_str() : g_err.c_str(); }

int ssg_default_config(ssg_config *cfg)
{
    if (!cfg) return fail(nullptr, SSG_ERR_BAD_ARG, "cfg is NULL");
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(ssg_config);
    cfg->flags = SSG_FLAG_AUTO_RESET;
    cfg->device_id = 0;
    cfg->n_envs = 1;
    cfg->env_id_base = 0;
    cfg->n_beams = 10;          // models.py:29
    cfg->history = 2;           // config.py:15
    cfg->max_steps = 1000;      // config.py:16
    cfg->n_goals = 5;           // game.py:17
    cfg->lidar_spread_deg = 90; // models.py:29
    cfg->lidar_dist = 100;
    cfg->goal_radius = 5;       // game.py:82
    cfg->width = 600;           // config.py:24
    cfg->height = 600;
    cfg->dt = 10 * 0.1;         // SPEED * base_dt, config.py:23, game.py:27
    cfg->damping_pow_dt = std::pow(0.4, cfg->dt); // game.py:270
    cfg->spawn_x = 600 / 2.0;   // game.py:274
    cfg->spawn_y = 25;
    cfg->force_y = 100;         // models.py:107
    cfg->thrust_px0 = 0.0;      // models.py:109: shape.bb.center() of a shape not yet in a space
    cfg->thrust_py0 = 0.0;
    cfg->rudder_step = 5;       // game.py:149-151
    cfg->rudder_max = 10;       // models.py:110
    cfg->n_ships = 1;           // ShipGame.reset adds the player only (game.py:274-275)
    return set_ship(cfg, 2.0, 3.0, 5.0); // game.py:275, models.py:87
}

int ssg_config_set_ship(ssg_config *cfg, double width_scale, double height_scale, double mass)
{
    if (!cfg || !(mass > 0.0) || !(width_scale > 0.0) || !(height_scale > 0.0))
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_config_set_ship: bad argument");
    return set_ship(cfg, width_scale, height_scale, mass);
}

int ssg_create(const ssg_config *cfg, ssg_handle **out)
{
    if (!cfg || !out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: NULL argument");
    if (cfg->struct_size != sizeof(ssg_config)) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: struct_size mismatch");
    if (cfg->n_envs < 1) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: n_envs must be >= 1");
    if (cfg->n_beams < 1 || cfg->n_beams > SSG_MAX_BEAMS)
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: n_beams must be in 1..16");
    // ship_env.py:46-47 raises ValueError("history_size must be greater than zero")
    if (cfg->history < 1) return fail(nullptr, SSG_ERR_BAD_ARG, "history_size must be greater than zero");
    if (cfg->history > SSG_MAX_HISTORY) return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: history must be <= 8");
    if (cfg->n_goals < 1 || cfg->n_goals > SSG_MAX_GOALS) return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: n_goals must be in 1..6");
    if (!(cfg->dt > 0.0)) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: dt must be > 0");
    if (cfg->max_steps < 1) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: max_steps must be >= 1");
    if (cfg->n_ships != 0 && cfg->n_ships != 1 && cfg->n_ships != 1 + SSG_N_TRAFFIC)
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: n_ships must be 1 or 4 (player + add_default_traffic)");
    if (cfg->map_ring != 0 && (cfg->map_ring < 2 || cfg->map_ring > 128))
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: map_ring must be 0 or in 2..128");
    // (record offsets are 32-bit: record index x SSG_MAP_STRIDE doubles must stay below 2^31)
    if (cfg->map_ring != 0 && (long long)cfg->n_envs * cfg->map_ring * SSG_MAP_STRIDE > 2147483647LL)
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: n_envs * map_ring * SSG_MAP_STRIDE must be < 2^31 (use a smaller ring, or shard the envs over more handles)");
    if (cfg->map_ring != 0 && cfg->history > 2)
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: map_ring needs history <= 2");
    if (cfg->n_ships > 1 && (cfg->flags & SSG_FLAG_EXACT_LIDAR))
        return fail(nullptr, SSG_ERR_UNSUPPORTED, "ssg_create: SSG_FLAG_EXACT_LIDAR is not built for n_ships = 4");
    ssg_handle *h = new (std::nothrow) ssg_handle();
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_create: out of host memory");
    h->cfg = *cfg;
    if (h->cfg.n_ships == 0) h->cfg.n_ships = 1;
    if (h->cfg.map_ring > 0) h->cfg.flags |= SSG_FLAG_BANK_IN_GLOBAL; // n_envs * R records never fit LDS
    if (h->cfg.n_ships > 1) {
        const int rc = set_traffic(h);
        if (rc != SSG_OK) { delete h; return fail(nullptr, rc, "ssg_create: traffic ship geometry"); }
    }
    h->block = pick_block(cfg->n_envs);
    if (h->cfg.n_ships > 1 && h->block == 128) h->block = 64; // the config-4 step kernel is built for 64 and 256
    refresh_dev(h);
    *out = h;
    return SSG_OK;
}

int ssg_destroy(ssg_handle *h)
{
    if (h)
        for (int i = 0; i < ssg_handle::kHostSlots; ++i)
            if (h->host_ev_made[i]) (void)hipEventDestroy(h->host_ev[i]);
    delete h;
    return SSG_OK;
}

int ssg_state_nbytes(const ssg_handle *h, size_t *nbytes)
{
    if (!h || !nbytes) return SSG_ERR_BAD_ARG;
    *nbytes = h->layout.nbytes;
    return SSG_OK;
}

int ssg_state_field(const ssg_handle *h, int field, size_t *offset, int *elem_size, int *n_columns,
                    size_t *column_stride_bytes)
{
    if (!h || !offset || !elem_size || !n_columns || !column_stride_bytes) return SSG_ERR_BAD_ARG;
    const FieldRow *r = std::find_if(std::begin(kFields), std::end(kFields), [field](const FieldRow &f) { return field >= f.field && field < f.field + f.n_fields; });
    if (r == std::end(kFields) || (r->config4 && h->cfg.n_ships <= 1)) return SSG_ERR_BAD_ARG;
    const size_t column = r->packed ? (size_t)r->elem_size : (size_t)h->layout.n_pad * (size_t)r->elem_size;
    *offset = (h->layout.*r->section).off + (size_t)(r->first_column + field - r->field) * column;
    *elem_size = r->elem_size;
    *n_columns = r->columns ? r->columns : h->cfg.n_beams;
    *column_stride_bytes = column;
    return SSG_OK;
}

int ssg_bind_state(ssg_handle *h, void *dev_state)
{
    if (!h || !dev_state) return fail(h, SSG_ERR_BAD_ARG, "ssg_bind_state: NULL argument");
    if (reinterpret_cast<uintptr_t>(dev_state) % 256 != 0)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_bind_state: state blob must be 256-byte aligned");
    h->state = dev_state;
    h->zeroed = false;
    h->dyn_step.blob_rebound();
    refresh_dev(h);
    return SSG_OK;
}

// map_ring mode: draw the worlds the rings are missing and restore the credit of R-1 episode starts per env
static int ring_refill(ssg_handle *h, double *dev_raw, void *stream)
{
    MapRing &r = h->ring;
    hipError_t e = ssg::launch_refill_worlds(h->dev, r.seed, r.width_frac, r.queue, r.count, const_cast<double *>(h->bank), dev_raw,
                                             static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ring refill launch: ") + hipGetErrorString(e));
    r.credit = h->cfg.map_ring - 1;
    // (A refill draws the worlds of FUTURE episodes, into the R-1 slots an env's current episode does not occupy, so no env's current world changes:
    // the rest bits and the queue of the next full cpSpaceStep stay valid and DynStep hears nothing of it; dropping the queue cost ~13 us a step.)
    return SSG_OK;
}

int ssg_init_state(ssg_handle *h, void *stream)
{
    int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = hipMemsetAsync(h->state, 0, h->layout.nbytes, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ssg_init_state: ") + hipGetErrorString(e));
    h->zeroed = true;
    h->dyn_step.queue_lost();
    // map_ring mode: the episode counters and the rings' "worlds drawn" counters were just zeroed together, so the rings
    // must hold episodes 0 .. R-1 again: redraw them (the bookkeeping and the bank never disagree)
    if (h->cfg.map_ring > 0 && h->ring.ready) return ring_refill(h, nullptr, stream);
    return SSG_OK;
}

int ssg_set_map_bank(ssg_handle *h, const double *dev_bank, int n_maps)
{
    if (!h || !dev_bank || n_maps < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_set_map_bank: bad argument");
    if ((long long)n_maps * SSG_MAP_STRIDE > 2147483647LL) return fail(h, SSG_ERR_UNSUPPORTED, "ssg_set_map_bank: n_maps * SSG_MAP_STRIDE must be < 2^31");
    if (reinterpret_cast<uintptr_t>(dev_bank) % 16 != 0)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_set_map_bank: bank must be 16-byte aligned");
    if (h->cfg.map_ring > 0 && (long long)n_maps != (long long)h->cfg.n_envs * h->cfg.map_ring)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_set_map_bank: map_ring mode needs n_maps == n_envs * map_ring");
    if (h->cfg.map_ring > 0) h->ring.ready = false; // a new bank: its rings are empty until ssg_refill_worlds
    // Envs per workgroup, and whether the bank is staged in the CU's LDS or gathered from L2 / HBM.  Staged: the largest size, from
    // the one preferred for this env count down, at which the bank fits the LDS beside the lidar buffers.  Gathered: the largest
    // size at which the record heads fit.  A staged bank wins at EQUAL workgroup size (65 536 envs, 10 beams, 64 records: 6.45
    // against 7.2 us per step), but a workgroup smaller than the preferred one means more workgroups than the chip holds at once
    // — they own their CU's LDS — i.e. launches of several rounds: 65 536 envs x 8 beams on 120 records took 16.1 us per step
    // staged on 64-env workgroups (four rounds) against 6.4 gathered on 256-env ones; 100 records, 128-env workgroups: 8.6
    // against 6.5.
    const bool dyn_cfg = h->cfg.n_ships > 1;
    auto fix_dyn = [&](int b) { return (dyn_cfg && b == 128) ? 64 : b; }; // the config-4 step kernel is built for 64 and 256
    const int preferred = fix_dyn(pick_block(h->cfg.n_envs));
    int staged_block = preferred, gathered_block = preferred;
    while (staged_block > 64 && ssg::step_lds_bytes(h->cfg.n_beams, staged_block, true, n_maps, dyn_cfg) > 160u * 1024u) staged_block = fix_dyn(staged_block / 2);
    while (gathered_block > 64 && ssg::step_lds_bytes(h->cfg.n_beams, gathered_block, false, n_maps, dyn_cfg) > 160u * 1024u) gathered_block = fix_dyn(gathered_block / 2);
    const bool can_stage = !(h->cfg.flags & SSG_FLAG_BANK_IN_GLOBAL) &&
                           ssg::step_lds_bytes(h->cfg.n_beams, staged_block, true, n_maps, dyn_cfg) <= 160u * 1024u;
    if (h->bank && n_maps < h->n_maps) h->remap_pending = true; // stale record indices >= n_maps must not survive
    h->bank = dev_bank;
    h->n_maps = n_maps;
    h->dyn_step.bank_changed();
    h->lds = can_stage && (staged_block == preferred || gathered_block <= staged_block);
    h->block = h->lds ? staged_block : gathered_block;
    h->lds_bytes = ssg::step_lds_bytes(h->cfg.n_beams, h->block, h->lds, n_maps, h->cfg.n_ships > 1);
    h->prepared = false;
    refresh_dev(h);
    return SSG_OK;
}

// map_ring mode: the ring was filled by ssg_refill_worlds, or the call is refused (before_reset: ssg_reset's wording)
static int ring_ready_or_refuse(ssg_handle *h, bool before_reset = false)
{
    if (h->cfg.map_ring <= 0 || h->ring.ready) return SSG_OK;
    return fail(h, SSG_ERR_NOT_BOUND, before_reset ? "map_ring mode: call ssg_refill_worlds before the first ssg_reset"
                                                   : "map_ring mode: call ssg_refill_worlds first");
}

// map_ring mode: take up to n episode starts per env (a reset is one, every step may be one) out of the ring's credit, refilling
// first if none is left, so that every ring still holds an unused world for each of them.  *taken (where asked): 1 .. n.
static int ring_take(ssg_handle *h, int n, void *stream, int *taken = nullptr)
{
    MapRing &r = h->ring;
    const int rc = r.credit < 1 ? ring_refill(h, nullptr, stream) : SSG_OK;
    if (rc != SSG_OK) return rc;
    if (n > r.credit) n = r.credit;
    r.credit -= n;
    if (taken) *taken = n;
    return SSG_OK;
}

static int flush_remap(ssg_handle *h, void *stream)
{
    if (!h->remap_pending) return SSG_OK;
    hipError_t e = ssg::launch_remap_map_ids(h->dev, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("map id remap launch: ") + hipGetErrorString(e));
    h->remap_pending = false;
    return SSG_OK;
}

int ssg_reset(ssg_handle *h, const uint8_t *dev_mask, const int32_t *dev_map_ids, double *dev_obs, void *stream)
{
    int rc = check_ready(h, true);
    if (rc == SSG_OK) rc = refuse_capture(h, stream, "ssg_reset");
    if (rc == SSG_OK && !dev_mask && !h->zeroed) rc = ssg_init_state(h, stream); // first full reset on a freshly bound blob: zeroed counters / columns
    if (rc == SSG_OK) rc = flush_remap(h, stream);
    if (rc != SSG_OK) return rc;
    if (h->cfg.map_ring > 0) {
        if (dev_map_ids) // episode p of env e lives in record e*R + p mod R: there is no other record to put it on
            return fail(h, SSG_ERR_BAD_ARG, "ssg_reset: dev_map_ids must be NULL in map_ring mode (an env's records are its own ring)");
        rc = ring_ready_or_refuse(h, true);
        if (rc == SSG_OK) rc = ring_take(h, 1, stream);
        if (rc != SSG_OK) return rc;
    }
    const bool one_record_per_wave = h->cfg.map_ring == 0 && h->n_maps <= ssg::kDynMapBuckets;
    const bool join = h->dyn_step.reset_arrives(dev_mask != nullptr, one_record_per_wave);
    const hipStream_t st = static_cast<hipStream_t>(stream); // config 4: the player, then add_default_traffic + fresh goal bodies, in one launch
    hipError_t e = h->cfg.n_ships > 1 ? ssg::launch_dyn_reset(h->dev, h->dyn, dev_mask, dev_map_ids, dev_obs, join, st)
                                      : ssg::launch_reset(h->dev, dev_mask, dev_map_ids, dev_obs, st);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("reset launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

static int prepare(ssg_handle *h)
{
    if (h->prepared) return SSG_OK;
    hipError_t e = ssg::prepare_step(h->dev, h->block, h->lds, h->lds_bytes);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_step: ") + hipGetErrorString(e));
    if (h->cfg.n_ships > 1) {
        e = ssg::prepare_dyn(h->dev);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_dyn: ") + hipGetErrorString(e));
    }
    h->prepared = true;
    return SSG_OK;
}

int ssg_step(ssg_handle *h, const int32_t *dev_actions, double *dev_obs, double *dev_reward, uint8_t *dev_done, uint8_t *dev_flags, void *stream)
{
    return ssg_rollout_traj(h, dev_actions, 1, dev_obs, dev_reward, dev_done, dev_flags, 0, stream);
}

int ssg_step_host(ssg_handle *h, const int32_t *host_actions, int32_t *dev_actions, double *dev_obs, double *dev_reward, uint8_t *dev_done,
                  uint8_t *dev_flags, const void *dev_block, void *host_block, size_t block_bytes, int slot, void *stream)
{
    if (!h || !host_actions || !dev_actions || !dev_block || !host_block || block_bytes == 0 || slot < 0 || slot >= ssg_handle::kHostSlots)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_step_host: NULL buffer, empty block or slot out of range");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!h->host_ev_made[slot]) {
        if (hipEventCreateWithFlags(&h->host_ev[slot], hipEventDisableTiming) != hipSuccess) return fail(h, SSG_ERR_HIP, "ssg_step_host: hipEventCreate failed");
        h->host_ev_made[slot] = true;
    }
    hipError_t e = hipMemcpyAsync(dev_actions, host_actions, (size_t)h->cfg.n_envs * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ssg_step_host: actions host -> device: ") + hipGetErrorString(e));
    int rc = ssg_step(h, dev_actions, dev_obs, dev_reward, dev_done, dev_flags, stream);
    if (rc != SSG_OK) return rc;
    e = hipMemcpyAsync(host_block, dev_block, block_bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(h->host_ev[slot], st);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ssg_step_host: outputs device -> host: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_wait_host(ssg_handle *h, int slot)
{
    if (!h || slot < 0 || slot >= ssg_handle::kHostSlots || !h->host_ev_made[slot]) return fail(h, SSG_ERR_BAD_ARG, "ssg_wait_host: no ssg_step_host was issued into this slot");
    hipError_t e = hipEventSynchronize(h->host_ev[slot]);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ssg_wait_host: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_rollout(ssg_handle *h, const int32_t *dev_actions, int K, double *dev_obs, double *dev_reward, uint8_t *dev_done, uint8_t *dev_flags, void *stream)
{
    return ssg_rollout_traj(h, dev_actions, K, dev_obs, dev_reward, dev_done, dev_flags, 0, stream);
}

namespace {
// One call's K steps: every step's actions, where the outputs go, how many steps one launch may fuse, the stream.
struct StepCall {
    const int32_t *actions; // [K][n_envs]
    int K;
    double *obs, *reward;
    uint8_t *done, *flags; // flags may be NULL
    long long stride; // envs between two steps' output slots; 0: every step writes the same rows
    int fuse;
    hipStream_t stream;
    // the call from step k on: its actions and output slots
    StepCall from(int k, const ssg_config &cfg) const {
        const size_t r = (size_t)k * (size_t)stride, D = (size_t)cfg.history * (size_t)(6 + cfg.n_beams);
        return {actions + (size_t)k * cfg.n_envs, K - k, obs + r * D, reward + r, done + r, flags ? flags + r : nullptr, stride, fuse, stream};
    }
};

// ssg_debug_kernel_times, a measurement aid: three events per step (before the full cpSpaceStep, between, after the step kernel); destroyed
// on every way out of the call, and no timing at all if one of them cannot be created
struct EventSet {
    std::vector<hipEvent_t> v;
    void mark(size_t i, hipStream_t st) const { if (!v.empty()) (void)hipEventRecord(v[i], st); }
    void create(size_t n) {
        v.reserve(n);
        for (size_t i = 0; i < n; ++i) { hipEvent_t ev; if (hipEventCreate(&ev) != hipSuccess) { clear(); return; } v.push_back(ev); }
    }
    void clear() { for (auto ev : v) (void)hipEventDestroy(ev); v.clear(); }
    ~EventSet() { clear(); }
};
} // namespace

// history > 2 and config 4: one launch of the step kernel per step.  Non-default history: into the staging rows, then the frame shift (see
// the kernel).  Config 4: every step is the dyn kernel (traffic ships, goal bodies, contact solver) followed by the step kernel, which
// reads this step's goal positions and the traffic-contact bit it left in the dyn columns.
static int steps_one_launch_each(ssg_handle *h, const StepCall &c)
{
    const bool dyn = h->cfg.n_ships > 1, shift = h->cfg.history > 2;
    EventSet evs;
    if (dyn && h->time_kernels) evs.create(3 * (size_t)c.K);
    auto failed = [h](const char *what, hipError_t e) { h->dyn_step.queue_lost(); return fail(h, SSG_ERR_HIP, std::string(what) + hipGetErrorString(e)); };
    for (int k = 0; k < c.K; ++k) {
        const StepCall s = c.from(k, h->cfg);
        evs.mark(3 * k, c.stream);
        const int rc = h->cfg.map_ring > 0 ? ring_take(h, 1, c.stream) : SSG_OK;
        if (rc != SSG_OK) return rc;
        if (dyn) {
            bool rebuild;
            hipError_t e = h->dyn_step.step_begins(h->layout.dyn_memo.size + h->layout.dyn_npm.size, c.stream, &rebuild);
            if (e == hipSuccess) e = ssg::launch_dyn_step(h->dev, h->dyn, rebuild, c.stream);
            if (e != hipSuccess) return failed("dyn step launch: ", e);
        }
        evs.mark(3 * k + 1, c.stream);
        hipError_t e = ssg::launch_step(h->dev, h->block, h->lds, h->lds_bytes, s.actions, 1, shift ? h->dev.obs2 : s.obs, s.reward, s.done,
                                        s.flags, 0, c.stream);
        evs.mark(3 * k + 2, c.stream);
        if (e == hipSuccess && shift) e = ssg::launch_history_shift(h->dev, s.done, s.obs, c.stream);
        if (e != hipSuccess) return failed("step launch: ", e);
        if (dyn) h->dyn_step.step_issued();
    }
    if (!evs.v.empty()) { // (this call then waits for its own work: a measurement run, not the product path)
        (void)hipStreamSynchronize(c.stream);
        for (int k = 0; k < c.K; ++k) {
            float a = 0.f, b = 0.f;
            (void)hipEventElapsedTime(&a, evs.v[3 * k], evs.v[3 * k + 1]);
            (void)hipEventElapsedTime(&b, evs.v[3 * k + 1], evs.v[3 * k + 2]);
            h->t_dyn_ms += a; h->t_step_ms += b; h->t_steps++;
        }
    }
    return SSG_OK;
}

// Steps fused into launches (state in registers, bank staged once), at most c.fuse per launch.  map_ring, a brand-new world per episode: an env
// starts at most one episode per step, so a launch also fuses at most as many steps as the ring has credit — its whole credit, up to 127 steps, in
// ONE launch (100 + 27 was a launch more per refill cycle) unless SSG_FUSE asks for fewer — then the rings are refilled (two small launches).
static int steps_fused(ssg_handle *h, const StepCall &c)
{
    const bool ring = h->cfg.map_ring > 0;
    for (int k = 0, n; k < c.K; k += n) {
        n = c.K - k;
        if (n > c.fuse && !(ring && c.fuse >= SSG_ROLLOUT_STEPS_PER_LAUNCH)) n = c.fuse;
        const int rc = ring ? ring_take(h, n, c.stream, &n) : SSG_OK;
        if (rc != SSG_OK) return rc;
        const StepCall s = c.from(k, h->cfg);
        hipError_t e = ssg::launch_step(h->dev, h->block, h->lds, h->lds_bytes, s.actions, n, s.obs, s.reward, s.done, s.flags, c.stride, c.stream);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("step launch: ") + hipGetErrorString(e));
    }
    return SSG_OK;
}

int ssg_rollout_traj(ssg_handle *h, const int32_t *dev_actions, int K, double *dev_obs, double *dev_reward,
                     uint8_t *dev_done, uint8_t *dev_flags, int64_t step_stride_envs, void *stream)
{
    int rc = check_ready(h, true);
    if (rc != SSG_OK) return rc;
    if (!dev_actions || !dev_obs || !dev_reward || !dev_done || K < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_step/ssg_rollout: NULL buffer or K < 1");
    if (step_stride_envs != 0 && step_stride_envs < (int64_t)h->cfg.n_envs)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_rollout_traj: step_stride_envs must be 0 or >= n_envs (steps would overlap)");
    rc = refuse_capture(h, stream, "ssg_step/ssg_rollout");
    if (rc == SSG_OK) rc = prepare(h);
    if (rc == SSG_OK) rc = flush_remap(h, stream);
    if (rc == SSG_OK) rc = ring_ready_or_refuse(h);
    if (rc != SSG_OK) return rc;
    // One launch runs up to kFuse consecutive steps (state in registers, bank staged once): 100 by default, which keeps a launch near a
    // millisecond and amortises the fixed launch cost to < 1 %.  SSG_FUSE=1 in the environment forces one launch per step.
    static const int kFuse = [] {
        const char *s = std::getenv("SSG_FUSE");
        return std::max(1, s ? std::atoi(s) : SSG_ROLLOUT_STEPS_PER_LAUNCH);
    }();
    const StepCall c = {dev_actions, K, dev_obs, dev_reward, dev_done, dev_flags, (long long)step_stride_envs, kFuse, static_cast<hipStream_t>(stream)};
    return h->cfg.history > 2 || h->cfg.n_ships > 1 ? steps_one_launch_each(h, c) : steps_fused(h, c);
}

// the activation kind in the low byte, SSG_POLICY_SEPARATE_VALUE or not, and no other bit
static bool activation_ok(int32_t activation)
{
    const int32_t kind = activation & ~SSG_POLICY_SEPARATE_VALUE;
    return kind == SSG_POLICY_TANH || kind == SSG_POLICY_RELU;
}

// ABI 9: the policy in the loop.  Everything a call could refuse is refused here, before anything is enqueued.
static int check_policy(ssg_handle *h, const ssg_policy *pol, const char *what)
{
    const std::string w(what);
    if (!pol) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL policy");
    if (pol->struct_size != sizeof(ssg_policy)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_policy.struct_size != sizeof(ssg_policy)");
    const int D = h->cfg.history * (6 + h->cfg.n_beams);
    if (pol->obs_dim != D) {
        char buf[160];
        std::snprintf(buf, sizeof buf, ": obs_dim %d differs from the handle's history*(6+n_beams) = %d", pol->obs_dim, D);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    if (pol->hidden < 16 || pol->hidden > SSG_POLICY_MAX_HIDDEN || pol->hidden % 16 != 0)
        return fail(h, SSG_ERR_BAD_ARG, w + ": hidden must be a multiple of 16 in 16..SSG_POLICY_MAX_HIDDEN");
    if (pol->n_hidden_layers < 1 || pol->n_hidden_layers > 2) return fail(h, SSG_ERR_BAD_ARG, w + ": n_hidden_layers must be 1 or 2");
    if (pol->n_actions < 2 || pol->n_actions > 4) return fail(h, SSG_ERR_BAD_ARG, w + ": n_actions must be in 2..4 (ssg_step accepts actions 0..3)");
    if (!activation_ok(pol->activation))
        return fail(h, SSG_ERR_BAD_ARG, w + ": activation must be SSG_POLICY_TANH or SSG_POLICY_RELU, optionally with SSG_POLICY_SEPARATE_VALUE");
    if (!pol->dev_params || !pol->dev_obs_scale) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_params or dev_obs_scale");
    return SSG_OK;
}

static int prepare_policy(ssg_handle *h)
{
    if (h->policy_prepared) return SSG_OK;
    hipError_t e = ssg::prepare_policy();
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_policy: ") + hipGetErrorString(e));
    h->policy_prepared = true;
    return SSG_OK;
}

// The resolver of ssg::MemberLayout (shipsim_internal.h), in two parts; every entry point takes its layout from one of them and hands it
// down as it is.  P members (1..SSG_POP_MAX_MEMBERS: the caller's range check) against the handle: the table bound to it
// (ssg_pop_set_slices), which must be for P members, else the equal split — which the envs must allow where the call launches on it
// (equal_split; ssg_set_obs_filter binds and ssg_pop_perm draws without asking).
static int member_layout(ssg_handle *h, int P, const char *what, bool equal_split, ssg::MemberLayout &lay)
{
    char buf[200];
    const int bound = (int)h->pop_sizes.size(), N = h->cfg.n_envs;
    if (bound && bound != P)
        std::snprintf(buf, sizeof buf, ": %d members, but slices for %d members are bound to the handle (ssg_pop_set_slices)", P, bound);
    else if (!bound && equal_split && N % P != 0)
        std::snprintf(buf, sizeof buf, ": the handle's %d envs do not split into %d equal member slices", N, P);
    else {
        lay = bound ? ssg::MemberLayout{P, h->slice_max, h->dev_slices} : ssg::MemberLayout{P, N / P, nullptr};
        return SSG_OK;
    }
    return fail(h, SSG_ERR_BAD_ARG, std::string(what) + buf);
}

// ... and one policy on the whole handle, whatever is bound
static ssg::MemberLayout whole_layout(const ssg_handle *h) { return {1, h->cfg.n_envs, nullptr}; }

// ABI 9 addition: the observation filter.  The record against the handle: everything ssg_set_obs_filter refuses.
static int check_filter(ssg_handle *h, const ssg_obs_filter *f, const char *what)
{
    const std::string w(what);
    char buf[200];
    if (f->struct_size != sizeof(ssg_obs_filter)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_obs_filter.struct_size != sizeof(ssg_obs_filter)");
    if (f->flags & ~SSG_FILTER_UPDATE) return fail(h, SSG_ERR_BAD_ARG, w + ": unknown bit in ssg_obs_filter.flags");
    const int D = h->cfg.history * (6 + h->cfg.n_beams);
    if (f->obs_dim != D) {
        std::snprintf(buf, sizeof buf, ": obs_dim %d differs from the handle's history*(6+n_beams) = %d", f->obs_dim, D);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    if (f->n_members < 1 || f->n_members > SSG_POP_MAX_MEMBERS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_members must be in 1..SSG_POP_MAX_MEMBERS");
    ssg::MemberLayout lay; // (a table bound for another member count; whether the envs split equally is the launching call's question)
    const int rc = member_layout(h, f->n_members, what, false, lay);
    if (rc != SSG_OK) return rc;
    if (!(f->clip >= 0.0) || !(f->eps >= 0.0)) return fail(h, SSG_ERR_BAD_ARG, w + ": clip and eps must be >= 0 (and not NaN)");
    if (!f->dev_state || !f->dev_workspace) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_state or dev_workspace");
    const size_t need = ssg::filter_workspace_bytes(h->cfg.n_envs, D, f->n_members);
    if (f->workspace_nbytes < need) {
        std::snprintf(buf, sizeof buf, ": workspace_nbytes %zu < %zu (ssg_obs_filter_workspace_nbytes)", f->workspace_nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    return SSG_OK;
}

// a job-wide filter's buffer (non-NULL) against the record f it is updated beside: f64 [n_members][SSG_FILTER_ROWS][obs_dim] like
// f->dev_state, and apart from it (the dual finalise kernel writes both)
static int check_filter_buffer(ssg_handle *h, const ssg_obs_filter *f, const double *dev_buffer, const char *what)
{
    const std::string w(what);
    if (reinterpret_cast<uintptr_t>(dev_buffer) % 8 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_buffer must be 8-byte aligned");
    const uintptr_t block = (uintptr_t)f->n_members * SSG_FILTER_ROWS * (uintptr_t)f->obs_dim * sizeof(double);
    const uintptr_t st = reinterpret_cast<uintptr_t>(f->dev_state), bf = reinterpret_cast<uintptr_t>(dev_buffer);
    if (bf < st + block && st < bf + block) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_buffer overlaps the filter's dev_state");
    return SSG_OK;
}

static int prepare_policy_filter(ssg_handle *h)
{
    if (!h->flt.struct_size || h->policy_filter_prepared) return SSG_OK;
    hipError_t e = ssg::prepare_policy_filter();
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_policy_filter: ") + hipGetErrorString(e));
    h->policy_filter_prepared = true;
    return SSG_OK;
}

static int prepare_policy_boot(ssg_handle *h)
{
    if (h->policy_boot_prepared) return SSG_OK;
    hipError_t e = ssg::prepare_policy_boot();
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_policy_boot: ") + hipGetErrorString(e));
    h->policy_boot_prepared = true;
    return SSG_OK;
}

// ABI 9 additions: GAE and the PPO update.  As above, everything a call could refuse is refused before anything is enqueued.
static int check_policy_shape(const ssg_policy *pol)
{
    return pol && pol->struct_size == sizeof(ssg_policy) && pol->obs_dim >= 1 && pol->obs_dim <= SSG_MAX_HISTORY * (6 + SSG_MAX_BEAMS) &&
           pol->hidden >= 16 && pol->hidden <= SSG_POLICY_MAX_HIDDEN && pol->hidden % 16 == 0 && pol->n_hidden_layers >= 1 &&
           pol->n_hidden_layers <= 2 && pol->n_actions >= 2 && pol->n_actions <= 4 &&
           activation_ok(pol->activation);
}

static int check_hparams(ssg_handle *h, const ssg_ppo_hparams *hp, const char *what)
{
    const std::string w(what);
    if (!hp) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL hparams");
    if (hp->struct_size != sizeof(ssg_ppo_hparams)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ppo_hparams.struct_size != sizeof(ssg_ppo_hparams)");
    const double v[] = {hp->gamma, hp->lam, hp->clip, hp->vf_coef, hp->ent_coef, hp->lr, hp->beta1, hp->beta2, hp->eps, hp->adv_eps};
    for (double x : v)
        if (!std::isfinite(x)) return fail(h, SSG_ERR_BAD_ARG, w + ": a hyper-parameter is not finite");
    if (!(hp->clip > 0.0)) return fail(h, SSG_ERR_BAD_ARG, w + ": clip must be > 0");
    if (!(hp->beta1 >= 0.0 && hp->beta1 < 1.0 && hp->beta2 >= 0.0 && hp->beta2 < 1.0)) return fail(h, SSG_ERR_BAD_ARG, w + ": betas must be in [0, 1)");
    return SSG_OK;
}

static size_t ppo_need_gae(long long N) { return ssg::kPpoSlotsOff + (size_t)ssg::ppo_gae_blocks(N) * 16; }
// the workspace of one gradient minibatch of M samples for `members` policies, slots from slots_off (kPpoSlotsOff / kPopSlotsOff); ext:
// slots of P + kExtStats floats behind the clip sequence's vector, partials and the KL sum
static size_t need_grad(size_t slots_off, int members, const ssg_policy &p, long long M, bool ext)
{
    const int G = ssg::ppo_grid(M), P = ssg::ppo_packed_len(p);
    if (ext) return ssg::ppo_ext_layout(slots_off, members, G, P).end;
    return slots_off + (size_t)members * (size_t)G * (size_t)(P + 4) * sizeof(float);
}

static int check_workspace(ssg_handle *h, const void *ws, size_t nbytes, size_t need, const char *what)
{
    const std::string w(what);
    if (!ws) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL workspace");
    if (reinterpret_cast<uintptr_t>(ws) % 256 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": the workspace must be 256-byte aligned");
    if (nbytes < need) {
        char buf[200];
        std::snprintf(buf, sizeof buf, ": workspace of %zu bytes, this call needs %zu (ssg_ppo_workspace_nbytes)", nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    return SSG_OK;
}

static int prepare_ppo(ssg_handle *h)
{
    if (h->ppo_prepared) return SSG_OK;
    hipError_t e = ssg::prepare_ppo();
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("prepare_ppo: ") + hipGetErrorString(e));
    h->ppo_prepared = true;
    return SSG_OK;
}

int ssg_ppo_workspace_nbytes(const ssg_policy *pol, int64_t n_samples, int64_t max_minibatch, size_t *nbytes)
{
    if (!nbytes || !check_policy_shape(pol) || n_samples < 1 || max_minibatch < 1)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_workspace_nbytes: bad policy record, NULL nbytes or a size < 1");
    *nbytes = std::max(ppo_need_gae(n_samples), std::max(need_grad(ssg::kPpoSlotsOff, 1, *pol, max_minibatch, false),
                                                         need_grad(ssg::kPpoSlotsOff, 1, *pol, max_minibatch, true)));
    return SSG_OK;
}

// The body of ssg_ppo_gae and ssg_ppo_gae_boot (with_boot: dev_boot_KN is required and the BOOT walk runs).
static int ppo_gae(ssg_handle *h, const ssg_ppo_hparams *hp, int K, int N, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                   const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN, bool with_boot, float *dev_adv_KN,
                   float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream, const char *what)
{
    const std::string w(what);
    int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    rc = check_hparams(h, hp, what);
    if (rc != SSG_OK) return rc;
    if (!dev_reward_KN || !dev_done_KN || !dev_value_KN || !dev_last_value || !dev_adv_KN || !dev_ret_KN)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL reward, done, value, last value, adv or ret buffer");
    if (with_boot && !dev_boot_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_boot_KN");
    if (K < 1 || N < 1 || (long long)K * N < 2) return fail(h, SSG_ERR_BAD_ARG, w + ": K and N must be >= 1 and K*N >= 2");
    rc = check_workspace(h, dev_workspace, workspace_nbytes, ppo_need_gae(N), what);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_ppo_gae(*hp, K, N, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value, dev_adv_KN, dev_ret_KN,
                                       dev_workspace, static_cast<hipStream_t>(stream), with_boot ? dev_boot_KN : nullptr);
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("gae launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_gae(ssg_handle *h, const ssg_ppo_hparams *hp, int K, int N, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                const float *dev_value_KN, const float *dev_last_value, float *dev_adv_KN, float *dev_ret_KN, void *dev_workspace,
                size_t workspace_nbytes, void *stream)
{
    return ppo_gae(h, hp, K, N, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value, nullptr, false, dev_adv_KN, dev_ret_KN, dev_workspace,
                   workspace_nbytes, stream, "ssg_ppo_gae");
}

int ssg_ppo_gae_boot(ssg_handle *h, const ssg_ppo_hparams *hp, int K, int N, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                     const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN, float *dev_adv_KN,
                     float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    return ppo_gae(h, hp, K, N, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value, dev_boot_KN, true, dev_adv_KN, dev_ret_KN,
                   dev_workspace, workspace_nbytes, stream, "ssg_ppo_gae_boot");
}

static int check_batch(ssg_handle *h, int64_t n_samples, const ssg::PpoBatch &b, const void *idx, const char *what)
{
    if (!b.x || !b.act || !b.logp || !b.adv || !b.ret || !idx)
        return fail(h, SSG_ERR_BAD_ARG, std::string(what) + ": NULL x, act, logp, adv, ret or index buffer");
    if (n_samples < 1) return fail(h, SSG_ERR_BAD_ARG, std::string(what) + ": n_samples < 1");
    return SSG_OK;
}

// Per-minibatch advantage normalisation (ssg_ppo_set_adv_norm): while it is bound, every minibatch of the gradient / update entry points
// takes its statistics from the handle's scratch (its stats rows, then its partials) instead of the workspace's batch statistics.
// With a table bound (ssg_ppo_set_adv_table) the gradient call reads the selected row, and nothing is launched ahead of it.
static void adv_norm_bind(const ssg_handle *h, ssg::PpoMinibatch &mb)
{
    if (h->adv_table) mb.adv_stats = h->adv_table + 4 * (size_t)h->adv_table_row;
    if (h->adv_norm_mode != SSG_ADV_NORM_MINIBATCH) return;
    char *base = static_cast<char *>(h->adv_norm_scratch);
    mb.adv_stats = reinterpret_cast<float *>(base);
    mb.adv_part = reinterpret_cast<double *>(base + ssg::adv_norm_stats_bytes(h->adv_norm_members));
}

// the call's member count must fit the bound scratch
static int check_adv_norm_members(ssg_handle *h, int members, const char *what)
{
    if (h->adv_norm_mode != SSG_ADV_NORM_MINIBATCH || members <= h->adv_norm_members) return SSG_OK;
    char buf[200];
    std::snprintf(buf, sizeof buf, ": %d members, but the bound advantage-normalisation scratch serves n_members = %d (ssg_ppo_set_adv_norm)", members,
                  h->adv_norm_members);
    return fail(h, SSG_ERR_BAD_ARG, std::string(what) + buf);
}

// torch.chunk of n samples into `minibatches`: chunks of C = ceil(n / minibatches), the last one shorter — so ceil(n / C) of them
struct Chunking {
    long long C, chunks;
};
static Chunking chunking(long long n, int minibatches)
{
    const long long C = (n + minibatches - 1) / minibatches;
    return {C, (n + C - 1) / C};
}

int ssg_ppo_adam(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const float *dev_grad, float *dev_adam_mv,
                 int64_t step, void *stream)
{
    int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    rc = check_policy(h, pol, "ssg_ppo_adam");
    if (rc == SSG_OK) rc = check_hparams(h, hp, "ssg_ppo_adam");
    if (rc != SSG_OK) return rc;
    if (!dev_grad || !dev_adam_mv) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_adam: NULL dev_grad or dev_adam_mv");
    if (step < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_adam: step must be >= 1");
    hipError_t e = ssg::launch_ppo_adam(*pol, *hp, dev_grad, dev_adam_mv, step, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("adam launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 additions: a population of policies on one handle.  Order of the refusals: no handle (BAD_ARG), no state blob (NOT_BOUND), then
// everything the host can judge about the arguments (BAD_ARG), and only then the device (check_ready) — nothing is enqueued before all
// of it passed.
static int pop_bound(ssg_handle *h)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop: NULL handle");
    if (!h->state) return fail(h, SSG_ERR_NOT_BOUND, "no state blob bound: call ssg_bind_state first");
    return SSG_OK;
}

static ssg_policy pop_policy(const ssg_population &pop)
{
    ssg_policy p;
    p.struct_size = sizeof(ssg_policy);
    p.obs_dim = pop.obs_dim;
    p.hidden = pop.hidden;
    p.n_hidden_layers = pop.n_hidden_layers;
    p.n_actions = pop.n_actions;
    p.activation = pop.activation;
    p.dev_params = pop.dev_params;
    p.dev_obs_scale = pop.dev_obs_scale;
    return p;
}

static bool pop_shape_ok(const ssg_population *pop)
{
    if (!pop || pop->struct_size != sizeof(ssg_population)) return false;
    if (pop->n_members < 1 || pop->n_members > SSG_POP_MAX_MEMBERS) return false;
    const ssg_policy p = pop_policy(*pop);
    return check_policy_shape(&p) != 0;
}

// the record against the handle: shape, member count (lay: its layout), pointers
static int check_population(ssg_handle *h, const ssg_population *pop, const char *what, ssg::MemberLayout &lay)
{
    const std::string w(what);
    if (!pop) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL population");
    if (pop->struct_size != sizeof(ssg_population)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_population.struct_size != sizeof(ssg_population)");
    if (pop->n_members < 1 || pop->n_members > SSG_POP_MAX_MEMBERS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_members must be in 1..SSG_POP_MAX_MEMBERS");
    const int rc = member_layout(h, pop->n_members, what, true, lay);
    if (rc != SSG_OK) return rc;
    const ssg_policy p = pop_policy(*pop);
    return check_policy(h, &p, what);
}

int ssg_ppo_dist(ssg_handle *h, const ssg_policy *pol, int64_t n_samples, const float *dev_x, float *dev_logp_all, void *stream)
{
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_policy(h, pol, "ssg_ppo_dist");
    if (rc != SSG_OK) return rc;
    if (!dev_x || !dev_logp_all) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_dist: NULL dev_x or dev_logp_all");
    if (n_samples < 1 || n_samples > 0x7fffffffll) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_dist: n_samples must be in 1..2^31-1");
    rc = check_ready(h, false);
    if (rc == SSG_OK) rc = prepare_policy(h);
    if (rc != SSG_OK) return rc;
    // (one policy over n_samples stored rows, which need not be the handle's envs)
    hipError_t e = ssg::launch_policy_dist(*pol, {1, (int)n_samples, nullptr}, n_samples, 1, dev_x, dev_logp_all, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("policy dist launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// Who acts in a policy call: one policy on all the handle's envs, or a population on its slices.  The two functions that fill the record
// are the only places that know the difference; what: the entry point's name, for its messages.
struct PolicyCall {
    ssg_policy pol; // (a population's: the shared shape over its parameter rows)
    ssg::MemberLayout lay;
    bool pop;
    const char *what;
};

static int one_policy_call(ssg_handle *h, const ssg_policy *pol, const char *what, PolicyCall &c)
{
    const int rc = check_policy(h, pol, what);
    if (rc == SSG_OK) c = {*pol, whole_layout(h), false, what};
    return rc;
}

static int population_call(ssg_handle *h, const ssg_population *pop, const char *what, PolicyCall &c)
{
    ssg::MemberLayout lay;
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_population(h, pop, what, lay);
    if (rc == SSG_OK) c = {pop_policy(*pop), lay, true, what};
    return rc;
}

// the call's member count must be the bound observation filter's, if one is bound
static int check_filter_members(ssg_handle *h, const PolicyCall &c)
{
    if (!h->flt.struct_size || h->flt.n_members == c.lay.members) return SSG_OK;
    char buf[200];
    std::snprintf(buf, sizeof buf, ": the bound observation filter has %d members, this call %d (ssg_set_obs_filter)", h->flt.n_members, c.lay.members);
    return fail(h, SSG_ERR_BAD_ARG, std::string(c.what) + buf);
}

// One policy launch of the call, with the FILTER kernels while a filter is bound.  l: the launch's own, leading part of the record (obs,
// uniform, seed, step, act, logp, value, x, greedy).
static hipError_t policy_launch(ssg_handle *h, const PolicyCall &c, ssg::PolicyLaunch l, hipStream_t st)
{
    const ssg::ObsFilterArgs f = {h->flt.dev_state, h->flt.clip};
    l.policy = &c.pol;
    l.lay = c.lay;
    l.pop = c.pop;
    l.env_base = h->cfg.env_id_base;
    l.filter = h->flt.struct_size ? &f : nullptr;
    return ssg::launch_policy(l, st);
}

static int policy_launch_failed(ssg_handle *h, const PolicyCall &c, hipError_t e)
{
    return fail(h, SSG_ERR_HIP, std::string(c.pop ? "population policy launch: " : "policy launch: ") + hipGetErrorString(e));
}

// the rollout loop's merge of the current observation rows ahead of a step's policy launch: only with SSG_FILTER_UPDATE bound
static hipError_t filter_step_update(ssg_handle *h, const PolicyCall &c, const double *obs, hipStream_t st)
{
    const ssg_obs_filter &f = h->flt;
    if (!f.struct_size || !(f.flags & SSG_FILTER_UPDATE)) return hipSuccess;
    return ssg::launch_filter_update(obs, f.obs_dim, c.lay, f.eps, f.dev_state, h->flt_buffer, f.dev_workspace, st); // (check_filter_members: the filter's members are the call's)
}

// What a loop of policy launches and steps asks last, once the host has judged the entry point's own arguments: the filter's member
// count, the bank and the device, what the per-step ssg_step would refuse (before the first policy launch), the kernels' attributes.
static int prepare_steps(ssg_handle *h, const PolicyCall &c, void *stream)
{
    int rc = check_filter_members(h, c);
    if (rc == SSG_OK) rc = check_ready(h, true);
    if (rc == SSG_OK) rc = ring_ready_or_refuse(h);
    if (rc == SSG_OK) rc = refuse_capture(h, stream, c.what);
    if (rc == SSG_OK) rc = prepare(h);
    if (rc == SSG_OK) rc = prepare_policy(h);
    if (rc == SSG_OK) rc = prepare_policy_filter(h);
    return rc;
}

// The body of the four act entry points; l as for policy_launch.  (The single-policy entries have asked check_ready already, ahead of
// their record: the order of their refusals.)
static int policy_act(ssg_handle *h, const PolicyCall &c, const ssg::PolicyLaunch &l, void *stream)
{
    if (!l.obs || !l.act || !l.logp || !l.value)
        return fail(h, SSG_ERR_BAD_ARG, std::string(c.what) + ": NULL dev_obs, dev_actions, dev_logp or dev_value");
    int rc = check_filter_members(h, c);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc == SSG_OK) rc = prepare_policy(h);
    if (rc == SSG_OK) rc = prepare_policy_filter(h);
    if (rc != SSG_OK) return rc;
    const hipError_t e = policy_launch(h, c, l, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? SSG_OK : policy_launch_failed(h, c, e);
}

int ssg_policy_act(ssg_handle *h, const ssg_policy *pol, const double *dev_obs, const float *dev_uniform, uint64_t seed, int64_t step,
                   int32_t *dev_actions, float *dev_logp, float *dev_value, float *dev_x, void *stream)
{
    PolicyCall c;
    int rc = check_ready(h, false);
    if (rc == SSG_OK) rc = one_policy_call(h, pol, "ssg_policy_act", c);
    return rc != SSG_OK ? rc : policy_act(h, c, {dev_obs, dev_uniform, seed, step, dev_actions, dev_logp, dev_value, dev_x, false}, stream);
}

int ssg_policy_act_greedy(ssg_handle *h, const ssg_policy *pol, const double *dev_obs, int32_t *dev_actions, float *dev_logp,
                          float *dev_value, float *dev_x, void *stream)
{
    PolicyCall c;
    int rc = check_ready(h, false);
    if (rc == SSG_OK) rc = one_policy_call(h, pol, "ssg_policy_act_greedy", c);
    return rc != SSG_OK ? rc : policy_act(h, c, {dev_obs, nullptr, 0, 0, dev_actions, dev_logp, dev_value, dev_x, true}, stream);
}

int ssg_pop_act(ssg_handle *h, const ssg_population *pop, const double *dev_obs, const float *dev_uniform, uint64_t seed, int64_t step,
                int32_t *dev_actions, float *dev_logp, float *dev_value, float *dev_x, void *stream)
{
    PolicyCall c;
    const int rc = population_call(h, pop, "ssg_pop_act", c);
    return rc != SSG_OK ? rc : policy_act(h, c, {dev_obs, dev_uniform, seed, step, dev_actions, dev_logp, dev_value, dev_x, false}, stream);
}

int ssg_pop_act_greedy(ssg_handle *h, const ssg_population *pop, const double *dev_obs, int32_t *dev_actions, float *dev_logp,
                       float *dev_value, float *dev_x, void *stream)
{
    PolicyCall c;
    const int rc = population_call(h, pop, "ssg_pop_act_greedy", c);
    return rc != SSG_OK ? rc : policy_act(h, c, {dev_obs, nullptr, 0, 0, dev_actions, dev_logp, dev_value, dev_x, true}, stream);
}

// One launch of the time-out values over K rows (ssg_timeout_values, ssg_pop_timeout_values, the end of a rollout with a record bound)
static hipError_t timeout_launch(ssg_handle *h, const PolicyCall &c, int K, const uint8_t *flags, const double *term_obs, float *boot,
                                 int64_t stride, hipStream_t st)
{
    const ssg::ObsFilterArgs f = {h->flt.dev_state, h->flt.clip};
    ssg::PolicyLaunch l = {};
    l.policy = &c.pol;
    l.lay = c.lay;
    l.pop = c.pop;
    l.filter = h->flt.struct_size ? &f : nullptr;
    return ssg::launch_timeout_values(l, {K, h->cfg.n_envs, (size_t)stride, flags, term_obs, boot}, st);
}

// The body of ssg_timeout_values / ssg_pop_timeout_values, once their record passed.
static int timeout_values(ssg_handle *h, const PolicyCall &c, int K, const uint8_t *dev_flags_KN, const double *dev_term_obs_KND,
                          float *dev_boot_KN, int64_t step_stride_envs, void *stream)
{
    const std::string w(c.what);
    if (!dev_flags_KN || !dev_term_obs_KND || !dev_boot_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_flags_KN, dev_term_obs_KND or dev_boot_KN");
    if (K < 1 || K > 65535) return fail(h, SSG_ERR_BAD_ARG, w + ": K must be in 1..65535");
    if (step_stride_envs < (int64_t)h->cfg.n_envs) return fail(h, SSG_ERR_BAD_ARG, w + ": step_stride_envs < n_envs (rows would overlap)");
    int rc = check_filter_members(h, c);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc == SSG_OK) rc = prepare_policy_boot(h);
    if (rc != SSG_OK) return rc;
    const hipError_t e = timeout_launch(h, c, K, dev_flags_KN, dev_term_obs_KND, dev_boot_KN, step_stride_envs, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? SSG_OK : fail(h, SSG_ERR_HIP, std::string("time-out values launch: ") + hipGetErrorString(e));
}

int ssg_timeout_values(ssg_handle *h, const ssg_policy *pol, int K, const uint8_t *dev_flags_KN, const double *dev_term_obs_KND,
                       float *dev_boot_KN, int64_t step_stride_envs, void *stream)
{
    PolicyCall c;
    int rc = check_ready(h, false);
    if (rc == SSG_OK) rc = one_policy_call(h, pol, "ssg_timeout_values", c);
    return rc != SSG_OK ? rc : timeout_values(h, c, K, dev_flags_KN, dev_term_obs_KND, dev_boot_KN, step_stride_envs, stream);
}

int ssg_pop_timeout_values(ssg_handle *h, const ssg_population *pop, int K, const uint8_t *dev_flags_KN, const double *dev_term_obs_KND,
                           float *dev_boot_KN, int64_t step_stride_envs, void *stream)
{
    PolicyCall c;
    const int rc = population_call(h, pop, "ssg_pop_timeout_values", c);
    return rc != SSG_OK ? rc : timeout_values(h, c, K, dev_flags_KN, dev_term_obs_KND, dev_boot_KN, step_stride_envs, stream);
}

// Restores the caller's terminal-observation binding (ssg_set_terminal_obs) on every way out of a loop that points h->dev.term_obs at
// rows of its own for the duration of a call: policy_rollout with a time-out record bound, run_evaluate with a recorder bound.
struct TermObsGuard {
    ssg_handle *h;
    double *saved;
    ~TermObsGuard() { h->dev.term_obs = saved; }
};

// The body of both rollout entry points: K times the filter's merge (if it updates), ONE policy launch for everyone and the step, then
// the bootstrap value.  (ssg_rollout_policy has asked check_ready already, ahead of its record: the order of its refusals.)
// With a time-out record bound (ssg_set_timeout_boot): step k's terminal observations go to row k of the record's rows — h->dev.term_obs
// is a host-side field handed to every launch — the caller's own ssg_set_terminal_obs binding is back in place on every way out of the
// loop, and one launch after the bootstrap forward turns the K rows of flags into the record's boot rows.
static int policy_rollout(ssg_handle *h, const PolicyCall &c, int K, const float *dev_uniform_KN, uint64_t seed, int64_t step0, double *dev_obs,
                          int32_t *dev_act_KN, float *dev_logp_KN, float *dev_value_KN, float *dev_x_KND, double *dev_reward_KN,
                          uint8_t *dev_done_KN, uint8_t *dev_flags_KN, float *dev_last_value, int64_t step_stride_envs, void *stream)
{
    const std::string w(c.what);
    if (!dev_obs || !dev_act_KN || !dev_logp_KN || !dev_value_KN || !dev_reward_KN || !dev_done_KN)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_obs, act, logp, value, reward or done buffer");
    if (K < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": K < 1");
    if (step_stride_envs < (int64_t)h->cfg.n_envs) return fail(h, SSG_ERR_BAD_ARG, w + ": step_stride_envs < n_envs (steps would overlap)");
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const bool boot = h->tob.struct_size != 0;
    if (boot) {
        if (K > h->tob.rows || K > 65535)
            return fail(h, SSG_ERR_BAD_ARG, w + ": K exceeds the rows of the bound time-out record (ssg_set_timeout_boot), or 65535");
        if (!dev_flags_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": a time-out record is bound (ssg_set_timeout_boot): dev_flags_KN is required");
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();
        else if (cs != hipStreamCaptureStatusNone)
            return fail(h, SSG_ERR_UNSUPPORTED, w + ": the stream is capturing a HIP graph, and with a time-out record bound (ssg_set_timeout_boot) "
                                                    "the handle's terminal-observation rows change from step to step");
    }
    int rc = prepare_steps(h, c, stream);
    if (rc == SSG_OK && boot) rc = prepare_policy_boot(h);
    if (rc != SSG_OK) return rc;
    const size_t S = (size_t)step_stride_envs, D = (size_t)c.pol.obs_dim;
    TermObsGuard guard = {h, h->dev.term_obs};
    for (int k = 0; k < K; ++k) {
        const size_t r = (size_t)k * S;
        if (boot) h->dev.term_obs = h->tob.dev_term_obs_KND + (size_t)k * (size_t)h->cfg.n_envs * D;
        hipError_t e = filter_step_update(h, c, dev_obs, st); // (first merge the step's rows, a member's into its own state rows, then normalise them)
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("observation filter launch: ") + hipGetErrorString(e));
        e = policy_launch(h, c, {dev_obs, dev_uniform_KN ? dev_uniform_KN + r : nullptr, seed, step0 + k, dev_act_KN + r, dev_logp_KN + r,
                                 dev_value_KN + r, dev_x_KND ? dev_x_KND + r * D : nullptr, false}, st);
        if (e != hipSuccess) return policy_launch_failed(h, c, e);
        // (ssg_step as it stands: the same launches, frame shifts, dyn kernels and ring refills as a caller's own step)
        rc = ssg_rollout_traj(h, dev_act_KN + r, 1, dev_obs, dev_reward_KN + r, dev_done_KN + r, dev_flags_KN ? dev_flags_KN + r : nullptr, 0,
                              stream);
        if (rc != SSG_OK) return rc;
    }
    if (dev_last_value) { // the value of the observation after the last step (PPO's bootstrap): a value-only forward (no filter merge)
        const hipError_t e = policy_launch(h, c, {dev_obs, nullptr, seed, step0 + K, nullptr, nullptr, dev_last_value, nullptr, false}, st);
        if (e != hipSuccess) return policy_launch_failed(h, c, e);
    }
    if (boot) {
        const hipError_t e = timeout_launch(h, c, K, dev_flags_KN, h->tob.dev_term_obs_KND, h->tob.dev_boot_KN, step_stride_envs, st);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("time-out values launch: ") + hipGetErrorString(e));
    }
    return SSG_OK;
}

int ssg_rollout_policy(ssg_handle *h, const ssg_policy *pol, int K, const float *dev_uniform_KN, uint64_t seed, int64_t step0,
                       double *dev_obs, int32_t *dev_act_KN, float *dev_logp_KN, float *dev_value_KN, float *dev_x_KND,
                       double *dev_reward_KN, uint8_t *dev_done_KN, uint8_t *dev_flags_KN, float *dev_last_value,
                       int64_t step_stride_envs, void *stream)
{
    PolicyCall c;
    int rc = check_ready(h, true);
    if (rc == SSG_OK) rc = one_policy_call(h, pol, "ssg_rollout_policy", c);
    if (rc != SSG_OK) return rc;
    return policy_rollout(h, c, K, dev_uniform_KN, seed, step0, dev_obs, dev_act_KN, dev_logp_KN, dev_value_KN, dev_x_KND, dev_reward_KN,
                          dev_done_KN, dev_flags_KN, dev_last_value, step_stride_envs, stream);
}

int ssg_pop_rollout(ssg_handle *h, const ssg_population *pop, int K, const float *dev_uniform_KN, uint64_t seed, int64_t step0,
                    double *dev_obs, int32_t *dev_act_KN, float *dev_logp_KN, float *dev_value_KN, float *dev_x_KND,
                    double *dev_reward_KN, uint8_t *dev_done_KN, uint8_t *dev_flags_KN, float *dev_last_value, int64_t step_stride_envs,
                    void *stream)
{
    PolicyCall c;
    const int rc = population_call(h, pop, "ssg_pop_rollout", c);
    if (rc != SSG_OK) return rc;
    return policy_rollout(h, c, K, dev_uniform_KN, seed, step0, dev_obs, dev_act_KN, dev_logp_KN, dev_value_KN, dev_x_KND, dev_reward_KN,
                          dev_done_KN, dev_flags_KN, dev_last_value, step_stride_envs, stream);
}

static size_t pop_need_gae(int P, long long n) { return ssg::kPopSlotsOff + (size_t)P * (size_t)ssg::ppo_gae_blocks(n) * 16; }
int ssg_pop_workspace_nbytes(const ssg_population *pop, int64_t samples_per_member, int64_t max_minibatch, size_t *nbytes)
{
    if (!nbytes || !pop_shape_ok(pop) || samples_per_member < 1 || max_minibatch < 1)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_workspace_nbytes: bad population record, n_members out of range, NULL nbytes or a size < 1");
    const ssg_policy pol = pop_policy(*pop);
    *nbytes = std::max(pop_need_gae(pop->n_members, samples_per_member),
                       std::max(need_grad(ssg::kPopSlotsOff, pop->n_members, pol, max_minibatch, false),
                                need_grad(ssg::kPopSlotsOff, pop->n_members, pol, max_minibatch, true)));
    return SSG_OK;
}

// The body of ssg_pop_gae and ssg_pop_gae_boot (with_boot: dev_boot_KN is required and the BOOT walk runs).
static int pop_gae(ssg_handle *h, const ssg_population *pop, const float *dev_table, int K, const double *dev_reward_KN,
                   const uint8_t *dev_done_KN, const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN, bool with_boot,
                   float *dev_adv_KN, float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream, const char *what)
{
    const std::string w(what);
    ssg::MemberLayout lay;
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_population(h, pop, what, lay);
    if (rc != SSG_OK) return rc;
    if (!dev_table || !dev_reward_KN || !dev_done_KN || !dev_value_KN || !dev_last_value || !dev_adv_KN || !dev_ret_KN)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL table, reward, done, value, last value, adv or ret buffer");
    if (with_boot && !dev_boot_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_boot_KN");
    if (K < 1 || (long long)K * (lay.slices ? h->slice_min : lay.n) < 2)
        return fail(h, SSG_ERR_BAD_ARG, w + ": K must be >= 1 and K * (a member's envs) >= 2 for every member");
    rc = check_workspace(h, dev_workspace, workspace_nbytes, pop_need_gae(lay.members, lay.n), what);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_pop_gae(lay, K, h->cfg.n_envs, dev_table, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value,
                                       with_boot ? dev_boot_KN : nullptr, dev_adv_KN, dev_ret_KN, dev_workspace, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("population gae launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_pop_gae(ssg_handle *h, const ssg_population *pop, const float *dev_table, int K, const double *dev_reward_KN,
                const uint8_t *dev_done_KN, const float *dev_value_KN, const float *dev_last_value, float *dev_adv_KN, float *dev_ret_KN,
                void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    return pop_gae(h, pop, dev_table, K, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value, nullptr, false, dev_adv_KN, dev_ret_KN,
                   dev_workspace, workspace_nbytes, stream, "ssg_pop_gae");
}

int ssg_pop_gae_boot(ssg_handle *h, const ssg_population *pop, const float *dev_table, int K, const double *dev_reward_KN,
                     const uint8_t *dev_done_KN, const float *dev_value_KN, const float *dev_last_value, const float *dev_boot_KN,
                     float *dev_adv_KN, float *dev_ret_KN, void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    return pop_gae(h, pop, dev_table, K, dev_reward_KN, dev_done_KN, dev_value_KN, dev_last_value, dev_boot_KN, true, dev_adv_KN, dev_ret_KN,
                   dev_workspace, workspace_nbytes, stream, "ssg_pop_gae_boot");
}

int ssg_pop_dist(ssg_handle *h, const ssg_population *pop, int K, const float *dev_x, float *dev_logp_all, void *stream)
{
    ssg::MemberLayout lay;
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_population(h, pop, "ssg_pop_dist", lay);
    if (rc != SSG_OK) return rc;
    if (!dev_x || !dev_logp_all) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_dist: NULL dev_x or dev_logp_all");
    if (K < 1 || K > 65535) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_dist: K must be in 1..65535");
    rc = check_ready(h, false);
    if (rc == SSG_OK) rc = prepare_policy(h);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_policy_dist(pop_policy(*pop), lay, h->cfg.n_envs, K, dev_x, dev_logp_all, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("population dist launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// The schedule of `members` members over n samples each: steps / launches / the longest chunk, and (out != NULL) the table.  false: an
// entry < 1 or a step count that does not fit an int32.
// samples (nullable): a sample count per member in place of n (ssg_pop_pack_schedule_samples; every entry >= 1) — the header rows then
// carry the prefix sums at SH_PREFIX.
static bool pop_schedule(int members, long long n_all, const int32_t *epochs, const int32_t *minibatches, int32_t *out, int32_t *steps_out,
                         long long *n_launches, long long *Cmax, const int64_t *samples = nullptr)
{
    long long launches = 0, cmax = 0;
    for (int m = 0; m < members; ++m) {
        if (epochs[m] < 1 || minibatches[m] < 1) return false;
        const long long n = samples ? (long long)samples[m] : n_all;
        const Chunking ck = chunking(n, minibatches[m]);
        const long long steps = (long long)epochs[m] * ck.chunks;
        if (steps > 0x7fffffffll || ck.C > 0x7fffffffll) return false;
        if (steps_out) steps_out[m] = (int32_t)steps;
        launches = std::max(launches, steps);
        cmax = std::max(cmax, ck.C);
    }
    *n_launches = launches;
    *Cmax = cmax;
    if (!out) return true;
    const size_t R = ssg::kPopSchedRow;
    std::memset(out, 0, SSG_POP_SCHED_INTS(members, launches) * sizeof(int32_t));
    long long prefix = 0;
    for (int m = 0; m < members; ++m) {
        const long long n = samples ? (long long)samples[m] : n_all;
        const Chunking ck = chunking(n, minibatches[m]);
        const long long steps = (long long)epochs[m] * ck.chunks;
        int32_t *hdr = out + (size_t)m * R;
        hdr[ssg::SH_STEPS] = (int32_t)steps;
        hdr[ssg::SH_CHUNKS] = (int32_t)ck.chunks;
        hdr[ssg::SH_C] = (int32_t)ck.C;
        hdr[ssg::SH_EPOCHS] = epochs[m];
        if (samples) std::memcpy(hdr + ssg::SH_PREFIX, &prefix, sizeof prefix);
        prefix += n;
        for (long long j = 0; j < steps; ++j) {
            const long long ep = j / ck.chunks, b0 = (j - ep * ck.chunks) * ck.C, M = std::min(ck.C, n - b0), off = ep * n + b0;
            int32_t *rec = out + ((size_t)(1 + j) * (size_t)members + (size_t)m) * R;
            const float invM = 1.0f / (float)M; // (as launch_ppo_minibatch forms it for one policy's kernel arguments)
            std::memcpy(rec + ssg::SR_OFF, &off, sizeof off);
            rec[ssg::SR_M] = (int32_t)M;
            rec[ssg::SR_G] = ssg::ppo_grid(M);
            rec[ssg::SR_FIRST] = b0 == 0;
            rec[ssg::SR_ACTIVE] = 1;
            std::memcpy(rec + ssg::SR_INVM, &invM, sizeof invM);
        }
    }
    return true;
}

// The body of ssg_pop_pack_schedule and ssg_pop_pack_schedule_samples (per_member: `samples` lists a count per member in place of n_all).
static int pack_schedule(int n_members, int64_t n_all, const int64_t *samples, bool per_member, const int32_t *epochs, const int32_t *minibatches,
                         int32_t *out, size_t out_ints, int32_t *steps_out, int32_t *n_launches_out, const char *what)
{
    const std::string w(what);
    const bool bad = !epochs || !minibatches || !n_launches_out || n_members < 1 || n_members > SSG_POP_MAX_MEMBERS;
    if (per_member) {
        if (bad || !samples) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL samples, epochs, minibatches or n_launches_out, or n_members out of range");
        for (int m = 0; m < n_members; ++m)
            if (samples[m] < 1) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": a member's sample count is < 1");
    } else if (bad || n_all < 1)
        return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL epochs, minibatches or n_launches_out, n_members out of range or samples_per_member < 1");
    long long launches = 0, cmax = 0;
    if (!pop_schedule(n_members, n_all, epochs, minibatches, nullptr, steps_out, &launches, &cmax, samples))
        return fail(nullptr, SSG_ERR_BAD_ARG, w + ": a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)");
    *n_launches_out = (int32_t)launches;
    if (!out) return SSG_OK; // the size query
    if (out_ints < SSG_POP_SCHED_INTS(n_members, launches))
        return fail(nullptr, SSG_ERR_BAD_ARG, w + ": out_ints < SSG_POP_SCHED_INTS(n_members, n_launches)");
    pop_schedule(n_members, n_all, epochs, minibatches, out, steps_out, &launches, &cmax, samples);
    return SSG_OK;
}

int ssg_pop_pack_schedule(int n_members, int64_t samples_per_member, const int32_t *epochs, const int32_t *minibatches, int32_t *out,
                          size_t out_ints, int32_t *steps_out, int32_t *n_launches_out)
{
    return pack_schedule(n_members, samples_per_member, nullptr, false, epochs, minibatches, out, out_ints, steps_out, n_launches_out,
                         "ssg_pop_pack_schedule");
}

int ssg_pop_pack_schedule_samples(int n_members, const int64_t *samples, const int32_t *epochs, const int32_t *minibatches, int32_t *out,
                                  size_t out_ints, int32_t *steps_out, int32_t *n_launches_out)
{
    return pack_schedule(n_members, 0, samples, true, epochs, minibatches, out, out_ints, steps_out, n_launches_out,
                         "ssg_pop_pack_schedule_samples");
}

// the slices table of `P` sizes (out nullable: the checks alone); false: an entry < 1 or a sum beyond 2^31-1
static bool pack_slices(int P, const int32_t *sizes, int32_t *out, long long *sum)
{
    long long o = 0;
    for (int m = 0; m < P; ++m) {
        if (sizes[m] < 1) return false;
        if (out) {
            int32_t *row = out + (size_t)m * SSG_POP_SLICE_ROW;
            row[0] = (int32_t)o;
            row[1] = sizes[m];
            row[2] = ssg::ppo_gae_blocks(sizes[m]);
            row[3] = 0;
        }
        o += sizes[m];
        if (o > 0x7fffffffll) return false;
    }
    *sum = o;
    return true;
}

int ssg_pop_pack_slices(int n_members, const int32_t *n_envs_per_member, int32_t *out, size_t out_ints)
{
    if (!n_envs_per_member || !out || n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_pack_slices: NULL pointer or n_members out of range");
    if (out_ints < (size_t)n_members * SSG_POP_SLICE_ROW)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_pack_slices: out_ints < SSG_POP_SLICE_ROW * n_members");
    long long sum = 0;
    if (!pack_slices(n_members, n_envs_per_member, nullptr, &sum))
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_pack_slices: a member's env count is < 1 or the sum exceeds 2^31-1");
    pack_slices(n_members, n_envs_per_member, out, &sum);
    return SSG_OK;
}

int ssg_pop_set_slices(ssg_handle *h, int n_members, const int32_t *n_envs_per_member, const int32_t *dev_slices)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_set_slices: NULL handle");
    if (n_members == 0 || !n_envs_per_member || !dev_slices) { // unbind
        h->pop_sizes.clear();
        h->dev_slices = nullptr;
        h->slice_max = h->slice_min = 0;
        return SSG_OK;
    }
    if (n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_set_slices: n_members must be in 1..SSG_POP_MAX_MEMBERS");
    long long sum = 0;
    if (!pack_slices(n_members, n_envs_per_member, nullptr, &sum))
        return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_set_slices: a member's env count is < 1 or the sum exceeds 2^31-1");
    if (sum != (long long)h->cfg.n_envs) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "ssg_pop_set_slices: the slices sum to %lld envs, the handle has %d", sum, h->cfg.n_envs);
        return fail(h, SSG_ERR_BAD_ARG, buf);
    }
    h->pop_sizes.assign(n_envs_per_member, n_envs_per_member + n_members);
    h->dev_slices = dev_slices;
    h->slice_max = *std::max_element(h->pop_sizes.begin(), h->pop_sizes.end());
    h->slice_min = *std::min_element(h->pop_sizes.begin(), h->pop_sizes.end());
    return SSG_OK;
}

int ssg_pop_get_slices(const ssg_handle *h, int *n_members, int32_t *out)
{
    if (!h || !n_members) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_get_slices: NULL handle or n_members");
    *n_members = (int)h->pop_sizes.size();
    if (out) std::copy(h->pop_sizes.begin(), h->pop_sizes.end(), out);
    return SSG_OK;
}

// The body of ssg_pop_pack_hparams and ssg_pop_pack_hparams_steps (per_member: `steps` lists a starting step per member in place of step0).
static int pack_hparams(int n_members, const ssg_ppo_hparams *hparams, int64_t step0, const int64_t *steps, bool per_member, int n_steps,
                        float *out, size_t out_floats, const char *what)
{
    const std::string w(what);
    const bool bad = !hparams || !out || n_members < 1 || n_members > SSG_POP_MAX_MEMBERS || n_steps < 0;
    if (per_member) {
        if (bad || !steps) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL pointer, n_members out of range or n_steps < 0");
        for (int m = 0; m < n_members; ++m)
            if (steps[m] < 0) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": a member's step0 is < 0");
    } else if (bad || step0 < 0)
        return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL pointer, n_members out of range, n_steps < 0 or step0 < 0");
    if (out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps))
        return fail(nullptr, SSG_ERR_BAD_ARG, w + ": out_floats < SSG_POP_TABLE_FLOATS(n_members, n_steps)");
    for (int m = 0; m < n_members; ++m) {
        const int rc = check_hparams(nullptr, hparams + m, what);
        if (rc != SSG_OK) return rc;
    }
    if (per_member) ssg::pop_pack_steps(n_members, hparams, steps, n_steps, out);
    else ssg::pop_pack(n_members, hparams, step0, n_steps, out);
    return SSG_OK;
}

int ssg_pop_pack_hparams(int n_members, const ssg_ppo_hparams *hparams, int64_t step0, int n_steps, float *out, size_t out_floats)
{
    return pack_hparams(n_members, hparams, step0, nullptr, false, n_steps, out, out_floats, "ssg_pop_pack_hparams");
}

int ssg_pop_pack_hparams_steps(int n_members, const ssg_ppo_hparams *hparams, const int64_t *step0, int n_steps, float *out, size_t out_floats)
{
    return pack_hparams(n_members, hparams, 0, step0, true, n_steps, out, out_floats, "ssg_pop_pack_hparams_steps");
}

// ABI 9 additions: the gradient and the update of one policy and of a population — ssg_ppo_grad / _grad_ext / _update / _update_ext,
// ssg_pop_update / _update_ext / _update_sched.  The entry point writes its own arguments into an UpdateCall; one of two fillers refuses
// what the host can judge and completes the record — they are the only places that know one policy from a population — and update_call
// is the tail all seven share: the workspace, the device, the kernels' attributes, then the one launch or the loop.  As everywhere,
// nothing is enqueued before every refusal has passed.

// A population on per-member schedules (ssg_pop_update_sched): what run_update takes from the schedule instead of from epochs x chunks.
struct PopSchedule {
    const int32_t *dev_sched; // the device table: header rows, then the records of launch 0, 1, ...
    long long n_launches;     // max steps_m
    long long Cmax;           // max C_m: every launch is as wide as the longest minibatch of the call needs
    int perm_epochs;          // permutation rows per member
};

struct UpdateCall {
    const char *what, *launch; // the entry point's name in its messages, and what a launch failure's message begins with
    // From the entry point: batch, ws, stats_out, and idx + M + grad_out (a gradient call: M indices) or idx + adam_mv (an update: the
    // [epochs][n] permutation rows; a population: [members][epochs][n]) with, for one policy, step = the Adam steps taken so far.  The
    // rest from the filler, but for what changes per minibatch.
    ssg::PpoMinibatch mb;
    size_t ws_nbytes;
    bool loop;                // false: a gradient call — ONE launch, no Adam step
    int epochs, minibatches;  // the loop on a common schedule, or
    bool sched;               // ... on per-member ones:
    PopSchedule sc;
    bool ext;                 // the extended loss:
    ssg::PpoExtLaunch el;
    bool kl_adapt;            // ... and whether the loop ends with the adaptation of the KL coefficient(s)
    float kl_target;          // (one policy's; a population's are rows of dev_ext)
    ssg_policy pol;           // what mb.policy points to, so a filled record is not copied (a population's: the shape over its rows)
    bool device_checked;      // the filler has consulted the device already (see one_policy_update)
};

static int check_ext(ssg_handle *h, const ssg_ppo_ext *ext, const char *what)
{
    const std::string w(what);
    if (!ext) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_ppo_ext");
    if (ext->struct_size != sizeof(ssg_ppo_ext)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ppo_ext.struct_size != sizeof(ssg_ppo_ext)");
    if (!std::isfinite(ext->vf_clip) || !std::isfinite(ext->max_grad_norm) || !std::isfinite(ext->kl_target))
        return fail(h, SSG_ERR_BAD_ARG, w + ": vf_clip, max_grad_norm or kl_target is not finite");
    if (ext->dev_kl_coef && !ext->dev_logp_all) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_kl_coef without dev_logp_all (ssg_ppo_dist)");
    if (ext->vf_clip > 0.0 && !ext->dev_value_old) return fail(h, SSG_ERR_BAD_ARG, w + ": vf_clip > 0 without dev_value_old");
    return SSG_OK;
}

static ssg::PpoExtLaunch ext_launch(const ssg_ppo_ext &ext)
{
    ssg::PpoExtLaunch e;
    e.kl_coef = ext.dev_kl_coef;
    e.logp_all = ext.dev_kl_coef ? ext.dev_logp_all : nullptr;
    e.vf_clip = ext.vf_clip > 0.0 ? (float)ext.vf_clip : 0.0f;
    e.value_old = ext.vf_clip > 0.0 ? ext.dev_value_old : nullptr;
    e.max_grad_norm = ext.max_grad_norm > 0.0 ? (float)ext.max_grad_norm : 0.0f;
    e.clip_seq = ext.max_grad_norm > 0.0;
    e.pop_ext = nullptr;
    e.first_chunk = true;
    return e;
}

// ONE policy on all the handle's samples.  c.ext: `ext` is required (the _ext entry points).
// The two orders of refusal.  The _ext pair refuses as every later entry point does (the comment above pop_bound): no handle, no state
// blob, everything the host can judge, and only then the device, in the tail.  ssg_ppo_grad and ssg_ppo_update are older than that rule
// and keep the order they shipped with, which callers can see: the device first (check_ready; a NULL handle is a bare SSG_ERR_BAD_ARG
// without a message), then the arguments.  The tail then leaves the device alone.
static int one_policy_update(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples,
                             UpdateCall &c)
{
    const std::string w(c.what);
    c.device_checked = !c.ext;
    int rc = c.device_checked ? check_ready(h, false) : pop_bound(h);
    if (rc == SSG_OK) rc = check_policy(h, pol, c.what);
    if (rc == SSG_OK) rc = check_hparams(h, hp, c.what);
    if (rc == SSG_OK && c.ext) rc = check_ext(h, ext, c.what);
    if (rc == SSG_OK) rc = check_batch(h, n_samples, c.mb.batch, c.mb.idx, c.what);
    if (rc != SSG_OK) return rc;
    if (c.loop) {
        if (!c.mb.adam_mv) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_adam_mv");
        if (c.epochs < 1 || c.minibatches < 1 || c.mb.step < 0) return fail(h, SSG_ERR_BAD_ARG, w + ": epochs < 1, minibatches < 1 or step0 < 0");
    } else {
        if (!c.mb.grad_out) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_grad");
        if (c.mb.M < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": M < 1");
    }
    c.pol = *pol;
    c.mb.policy = &c.pol;
    c.mb.lay = whole_layout(h);
    c.mb.n_samples = n_samples;
    c.mb.slots_off = ssg::kPpoSlotsOff;
    c.mb.hp = hp;
    if (c.ext) {
        c.el = ext_launch(*ext);
        c.kl_adapt = ext->kl_target > 0.0 && ext->dev_kl_coef;
        c.kl_target = (float)ext->kl_target;
    }
    return SSG_OK;
}

// the ssg_pop_ext record, for ssg_pop_update_ext and ssg_pop_update_sched
static int check_pop_ext(ssg_handle *h, const ssg_pop_ext *ext, const char *what)
{
    const std::string w(what);
    if (!ext) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_pop_ext");
    if (ext->struct_size != sizeof(ssg_pop_ext)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_pop_ext.struct_size != sizeof(ssg_pop_ext)");
    if (ext->flags & ~(SSG_POP_EXT_GRAD_CLIP | SSG_POP_EXT_VF_CLIP)) return fail(h, SSG_ERR_BAD_ARG, w + ": unknown ssg_pop_ext.flags bits");
    if (!ext->dev_ext) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_ext");
    if (ext->dev_kl_coef && !ext->dev_logp_all) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_kl_coef without dev_logp_all (ssg_pop_dist)");
    if ((ext->flags & SSG_POP_EXT_VF_CLIP) && !ext->dev_value_old) return fail(h, SSG_ERR_BAD_ARG, w + ": SSG_POP_EXT_VF_CLIP without dev_value_old");
    return SSG_OK;
}

// a population's: the members' constants are rows of dev_ext, the flags say which terms some member has on
static ssg::PpoExtLaunch ext_launch(const ssg_pop_ext &ext)
{
    ssg::PpoExtLaunch e;
    e.kl_coef = ext.dev_kl_coef;
    e.logp_all = ext.dev_kl_coef ? ext.dev_logp_all : nullptr;
    e.value_old = (ext.flags & SSG_POP_EXT_VF_CLIP) ? ext.dev_value_old : nullptr;
    e.pop_ext = ext.dev_ext;
    e.vf_clip = e.max_grad_norm = 0.0f; // (per member: dev_ext)
    e.clip_seq = (ext.flags & SSG_POP_EXT_GRAD_CLIP) != 0;
    e.first_chunk = true;
    return e;
}

// A population on the handle's slices, every member on its K * (its envs) samples.  c.ext: `ext` is required.  c.sched: the per-member
// epochs / minibatches (host arrays, from which the launches, their width and the workspace are re-derived: what the device table was
// packed from decides them) with the device table and the permutation rows per member, in place of c.epochs / c.minibatches; unequal
// slices run only so.
static int population_update(ssg_handle *h, const ssg_population *pop, const ssg_pop_ext *ext, const float *dev_table, int table_steps, int K,
                             const int32_t *dev_sched, const int32_t *epochs, const int32_t *minibatches, int perm_epochs, UpdateCall &c)
{
    const std::string w(c.what);
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_population(h, pop, c.what, c.mb.lay);
    if (rc == SSG_OK && c.ext) rc = check_pop_ext(h, ext, c.what);
    if (rc != SSG_OK) return rc;
    if (K < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": K < 1");
    const int P = pop->n_members, N = h->cfg.n_envs;
    const int32_t *slices = c.mb.lay.slices;
    if (slices && !c.sched)
        return fail(h, SSG_ERR_BAD_ARG, w + ": slices are bound to the handle (ssg_pop_set_slices): the update runs through ssg_pop_update_sched");
    long long n = (long long)K * (N / P); // samples per member (unequal slices: the widest member's, below)
    rc = check_batch(h, n, c.mb.batch, c.mb.idx, c.what);
    if (rc == SSG_OK) rc = check_adv_norm_members(h, P, c.what);
    if (rc != SSG_OK) return rc;
    if (!dev_table || !c.mb.adam_mv) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_table or dev_adam_mv");
    if (!c.sched) {
        if (c.epochs < 1 || c.minibatches < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": epochs < 1 or minibatches < 1");
        if ((long long)table_steps < (long long)c.epochs * chunking(n, c.minibatches).chunks)
            return fail(h, SSG_ERR_BAD_ARG, w + ": the table holds fewer Adam steps than epochs * chunks");
    } else {
        if (!epochs || !minibatches) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL epochs or minibatches");
        if (!dev_sched) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_sched");
        c.sc.dev_sched = dev_sched;
        c.sc.perm_epochs = perm_epochs;
        // unequal slices: every member's own sample count, and what the SLICED kernels read instead of n, n_samples and idx_stride
        std::vector<int64_t> samples;
        if (slices) {
            for (int32_t n_m : h->pop_sizes) samples.push_back((int64_t)K * n_m);
            c.mb.sched_hdr = dev_sched;
            c.mb.K = K;
            c.mb.perm_epochs = perm_epochs;
            n = *std::max_element(samples.begin(), samples.end());
        }
        if (!pop_schedule(P, n, epochs, minibatches, nullptr, nullptr, &c.sc.n_launches, &c.sc.Cmax, samples.empty() ? nullptr : samples.data()))
            return fail(h, SSG_ERR_BAD_ARG, w + ": a member's epochs or minibatches is < 1 (or its steps exceed 2^31-1)");
        if (perm_epochs < *std::max_element(epochs, epochs + P)) return fail(h, SSG_ERR_BAD_ARG, w + ": perm_epochs < the largest epochs of a member");
        if ((long long)table_steps < c.sc.n_launches)
            return fail(h, SSG_ERR_BAD_ARG, w + ": the table holds fewer Adam steps than the schedule's launches (max epochs * chunks)");
    }
    c.pol = pop_policy(*pop);
    c.mb.policy = &c.pol;
    c.mb.N = N;
    c.mb.n_samples = n;
    c.mb.slots_off = ssg::kPopSlotsOff;
    c.mb.table = dev_table;
    if (c.ext) {
        c.el = ext_launch(*ext);
        c.kl_adapt = ext->dev_kl_coef != nullptr;
    }
    return SSG_OK;
}

// The loop of the five update entry points.  c.mb: idx = the permutation rows, stats_out = the caller's stats rows or NULL, step = the
// Adam steps taken so far, table = a population's table.  Minibatch j of the call reads chunk j % chunks of permutation row j / chunks,
// takes Adam step step + 1 + j (a population: the table's Adam rows 1 + j) and writes stats row j.  With c.sched launch j serves
// minibatch j of every member that has one: M, the chunk's place and first_chunk are per member, in the table's records of launch j; the
// launch itself is sized for Cmax.  c.kl_adapt: end with the adaptation of the coefficient(s) from the last epoch's chunks.
static int run_update(ssg_handle *h, UpdateCall &c, hipStream_t st)
{
    ssg::PpoMinibatch mb = c.mb;
    ssg::PpoExtLaunch *ext = c.ext ? &c.el : nullptr;
    const PopSchedule *sched = c.sched ? &c.sc : nullptr;
    const long long n = mb.n_samples;
    const Chunking ck = sched ? Chunking{sched->Cmax, 0} : chunking(n, c.minibatches);
    const long long launches = sched ? sched->n_launches : (long long)c.epochs * ck.chunks;
    const int cols = ext ? ssg::kExtStats : 4;
    const int64_t *perm = mb.idx;
    float *stats = mb.stats_out;
    mb.ext = ext;
    mb.idx_stride = (long long)(sched ? sched->perm_epochs : c.epochs) * n;
    mb.stats_stride = cols * launches;
    for (long long j = 0; j < launches; ++j) {
        if (sched) {
            mb.M = sched->Cmax;
            mb.sched = sched->dev_sched + (size_t)(1 + j) * (size_t)mb.lay.members * ssg::kPopSchedRow;
        } else {
            const long long ep = j / ck.chunks, b0 = (j - ep * ck.chunks) * ck.C;
            mb.M = std::min(ck.C, n - b0);
            mb.idx = perm + (size_t)ep * (size_t)n + (size_t)b0;
            if (ext) ext->first_chunk = b0 == 0;
        }
        mb.stats_out = stats ? stats + cols * j : nullptr;
        ++mb.step;
        if (mb.table) mb.adam_row = mb.table + (size_t)(1 + j) * (size_t)mb.lay.members * ssg::kPopTableRow;
        hipError_t e = ssg::launch_ppo_minibatch(mb, st);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.launch) + " launch: " + hipGetErrorString(e));
    }
    if (c.kl_adapt) {
        hipError_t e = ssg::launch_kl_adapt(mb.lay.members, *ext, c.kl_target, ssg::ppo_packed_len(c.pol), ck.chunks,
                                            sched ? sched->dev_sched : nullptr, mb.ws, mb.slots_off, st);
        if (e != hipSuccess)
            return fail(h, SSG_ERR_HIP, std::string(mb.table ? "population kl adapt launch: " : "kl adapt launch: ") + hipGetErrorString(e));
    }
    return SSG_OK;
}

// The tail of all seven: the workspace against the widest minibatch of the call, the device, the kernels' attributes, the bound
// per-minibatch normalisation, and then the gradient call's one launch or the loop.
static int update_call(ssg_handle *h, UpdateCall &c, void *stream)
{
    const long long M = !c.loop ? c.mb.M : c.sched ? c.sc.Cmax : chunking(c.mb.n_samples, c.minibatches).C;
    int rc = check_workspace(h, c.mb.ws, c.ws_nbytes, need_grad(c.mb.slots_off, c.mb.lay.members, c.pol, M, c.ext), c.what);
    if (rc == SSG_OK && h->adv_table && (c.loop || c.mb.table)) // (the last thing the host judges: no refusal of a handle without a table moves)
        rc = fail(h, SSG_ERR_BAD_ARG, std::string(c.what) + ": an advantage table is bound to the handle (ssg_ppo_set_adv_table): a table row is one "
                                                           "minibatch's and this call runs many, or many members'; only ssg_ppo_grad and ssg_ppo_grad_ext read it");
    if (rc == SSG_OK && !c.device_checked) rc = check_ready(h, false);
    if (rc == SSG_OK) rc = prepare_ppo(h);
    if (rc != SSG_OK) return rc;
    adv_norm_bind(h, c.mb);
    if (c.loop) return run_update(h, c, static_cast<hipStream_t>(stream));
    c.mb.ext = c.ext ? &c.el : nullptr;
    hipError_t e = ssg::launch_ppo_minibatch(c.mb, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.launch) + " launch: " + hipGetErrorString(e));
    return SSG_OK;
}

// what every one of the seven writes into its record first
static UpdateCall update_args(const char *what, const char *launch, bool ext, const float *dev_x, const int32_t *dev_act, const float *dev_logp,
                              const float *dev_adv, const float *dev_ret, const int64_t *dev_idx, float *dev_stats, void *dev_workspace,
                              size_t workspace_nbytes)
{
    UpdateCall c = {};
    c.what = what;
    c.launch = launch;
    c.ext = ext;
    c.mb.batch = {dev_x, dev_act, dev_logp, dev_adv, dev_ret};
    c.mb.idx = dev_idx;
    c.mb.stats_out = dev_stats;
    c.mb.ws = dev_workspace;
    c.ws_nbytes = workspace_nbytes;
    return c;
}

// ... and an update after it: the loop, its moments and, where they are common, its epochs and minibatches
static void update_loop(UpdateCall &c, float *dev_adam_mv, int epochs, int minibatches)
{
    c.loop = true;
    c.mb.adam_mv = dev_adam_mv;
    c.epochs = epochs;
    c.minibatches = minibatches;
}

static int ppo_grad(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples, int64_t M,
                    float *dev_grad, UpdateCall c, void *stream)
{
    c.mb.M = M;
    c.mb.grad_out = dev_grad;
    const int rc = one_policy_update(h, pol, hp, ext, n_samples, c);
    return rc == SSG_OK ? update_call(h, c, stream) : rc;
}

int ssg_ppo_grad(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, int64_t n_samples, const float *dev_x,
                 const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_idx,
                 int64_t M, float *dev_grad, float *dev_stats, void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    return ppo_grad(h, pol, hp, nullptr, n_samples, M, dev_grad,
                    update_args("ssg_ppo_grad", "ppo grad", false, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_idx, dev_stats, dev_workspace,
                                workspace_nbytes), stream);
}

int ssg_ppo_grad_ext(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples,
                     const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                     const int64_t *dev_idx, int64_t M, float *dev_grad, float *dev_stats, void *dev_workspace, size_t workspace_nbytes,
                     void *stream)
{
    return ppo_grad(h, pol, hp, ext, n_samples, M, dev_grad,
                    update_args("ssg_ppo_grad_ext", "ppo grad_ext", true, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_idx, dev_stats,
                                dev_workspace, workspace_nbytes), stream);
}

static int ppo_update(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples, int epochs,
                      int minibatches, float *dev_adam_mv, int64_t step0, UpdateCall c, void *stream)
{
    update_loop(c, dev_adam_mv, epochs, minibatches);
    c.mb.step = step0;
    const int rc = one_policy_update(h, pol, hp, ext, n_samples, c);
    return rc == SSG_OK ? update_call(h, c, stream) : rc;
}

int ssg_ppo_update(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, int64_t n_samples, const float *dev_x,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_perm,
                   int epochs, int minibatches, float *dev_adam_mv, int64_t step0, float *dev_stats, void *dev_workspace,
                   size_t workspace_nbytes, void *stream)
{
    return ppo_update(h, pol, hp, nullptr, n_samples, epochs, minibatches, dev_adam_mv, step0,
                      update_args("ssg_ppo_update", "ppo update", false, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_perm, dev_stats,
                                  dev_workspace, workspace_nbytes), stream);
}

int ssg_ppo_update_ext(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, int64_t n_samples,
                       const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                       const int64_t *dev_perm, int epochs, int minibatches, float *dev_adam_mv, int64_t step0, float *dev_stats,
                       void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    return ppo_update(h, pol, hp, ext, n_samples, epochs, minibatches, dev_adam_mv, step0,
                      update_args("ssg_ppo_update_ext", "ppo update_ext", true, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_perm, dev_stats,
                                  dev_workspace, workspace_nbytes), stream);
}

// ABI 9 additions: data parallel — the job-wide advantage statistics and the apply of W shards' gradient rows.  Refusals in the order
// of every later entry point (the comment above pop_bound): the handle, the state blob, what the host can judge, then the device.
int ssg_ppo_adv_moments(ssg_handle *h, int K, int N, void *dev_workspace, size_t workspace_nbytes, double *dev_out4, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!dev_out4) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_adv_moments: NULL dev_out4");
    if (K < 1 || N < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_adv_moments: K and N must be >= 1");
    rc = check_workspace(h, dev_workspace, workspace_nbytes, ppo_need_gae(N), "ssg_ppo_adv_moments");
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_dp_adv_moments(K, N, dev_workspace, dev_out4, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("adv moments launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_set_adv_moments(ssg_handle *h, int n_shards, const double *dev_rows, double adv_eps, void *dev_workspace, size_t workspace_nbytes,
                            void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!dev_rows) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_moments: NULL dev_rows");
    if (n_shards < 1 || n_shards > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_moments: n_shards must be in 1..SSG_DP_MAX_SHARDS");
    if (!std::isfinite(adv_eps)) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_moments: adv_eps is not finite");
    rc = check_workspace(h, dev_workspace, workspace_nbytes, ssg::kPpoSlotsOff, "ssg_ppo_set_adv_moments");
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_dp_set_adv_moments(n_shards, dev_rows, adv_eps, dev_workspace, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("set adv moments launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_apply_shards(ssg_handle *h, const ssg_policy *pol, const ssg_ppo_hparams *hp, const ssg_ppo_ext *ext, const ssg_ppo_shards *sh,
                         float *dev_adam_mv, int64_t step, float *dev_stats, void *dev_workspace, size_t workspace_nbytes, void *stream)
{
    const char *what = "ssg_ppo_apply_shards";
    const std::string w(what);
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_policy(h, pol, what);
    if (rc == SSG_OK) rc = check_hparams(h, hp, what);
    if (rc != SSG_OK) return rc;
    if (ext) { // (the batch pointers of the record are not read here: check_ext's rules about them are the gradient call's)
        if (ext->struct_size != sizeof(ssg_ppo_ext)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ppo_ext.struct_size != sizeof(ssg_ppo_ext)");
        if (!std::isfinite(ext->vf_clip) || !std::isfinite(ext->max_grad_norm) || !std::isfinite(ext->kl_target))
            return fail(h, SSG_ERR_BAD_ARG, w + ": vf_clip, max_grad_norm or kl_target is not finite");
    }
    if (!sh) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_ppo_shards");
    if (sh->struct_size != sizeof(ssg_ppo_shards)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ppo_shards.struct_size != sizeof(ssg_ppo_shards)");
    if (sh->n_shards < 1 || sh->n_shards > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_shards must be in 1..SSG_DP_MAX_SHARDS");
    if (sh->reserved != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ppo_shards.reserved must be 0");
    if (!sh->dev_rows || !sh->counts || !dev_adam_mv) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_rows, counts or dev_adam_mv");
    for (int r = 0; r < sh->n_shards; ++r)
        if (sh->counts[r] < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": a shard's count is < 1");
    if (step < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": step must be >= 1");
    const bool adapt = ext && sh->last_chunk && ext->dev_kl_coef && ext->kl_target > 0.0;
    if (adapt && sh->n_chunks < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": n_chunks must be >= 1 where the adaptation runs");
    if (h->adv_norm_mode == SSG_ADV_NORM_MINIBATCH)
        return fail(h, SSG_ERR_BAD_ARG, w + ": SSG_ADV_NORM_MINIBATCH is bound to the handle (ssg_ppo_set_adv_norm): per-minibatch statistics "
                                            "across shards are out of scope");
    const size_t need = ext ? ssg::ppo_ext_layout(ssg::kPpoSlotsOff, 1, 1, ssg::ppo_packed_len(*pol)).slots : ssg::kPpoSlotsOff;
    rc = check_workspace(h, dev_workspace, workspace_nbytes, need, what);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    ssg::DpApply a = {};
    a.policy = pol;
    a.hp = hp;
    a.ext = ext != nullptr;
    a.max_grad_norm = ext && ext->max_grad_norm > 0.0 ? (float)ext->max_grad_norm : 0.0f;
    a.kl_target = ext ? (float)ext->kl_target : 0.0f;
    a.kl_coef = ext ? ext->dev_kl_coef : nullptr;
    a.n_shards = sh->n_shards;
    a.rows = sh->dev_rows;
    a.counts = sh->counts;
    a.first_chunk = sh->first_chunk != 0;
    a.last_chunk = sh->last_chunk != 0;
    a.n_chunks = sh->n_chunks;
    a.adam_mv = dev_adam_mv;
    a.step = step;
    a.stats_out = dev_stats;
    a.ws = dev_workspace;
    hipError_t e = ssg::launch_dp_apply(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("apply shards launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_pop_update(ssg_handle *h, const ssg_population *pop, const float *dev_table, int table_steps, int K, const float *dev_x,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret, const int64_t *dev_perm,
                   int epochs, int minibatches, float *dev_adam_mv, float *dev_stats, void *dev_workspace, size_t workspace_nbytes,
                   void *stream)
{
    UpdateCall c = update_args("ssg_pop_update", "population update", false, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_perm, dev_stats,
                               dev_workspace, workspace_nbytes);
    update_loop(c, dev_adam_mv, epochs, minibatches);
    const int rc = population_update(h, pop, nullptr, dev_table, table_steps, K, nullptr, nullptr, nullptr, 0, c);
    return rc == SSG_OK ? update_call(h, c, stream) : rc;
}

int ssg_pop_update_ext(ssg_handle *h, const ssg_population *pop, const ssg_pop_ext *ext, const float *dev_table, int table_steps, int K,
                       const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                       const int64_t *dev_perm, int epochs, int minibatches, float *dev_adam_mv, float *dev_stats, void *dev_workspace,
                       size_t workspace_nbytes, void *stream)
{
    UpdateCall c = update_args("ssg_pop_update_ext", "population update_ext", true, dev_x, dev_act, dev_logp, dev_adv, dev_ret, dev_perm,
                               dev_stats, dev_workspace, workspace_nbytes);
    update_loop(c, dev_adam_mv, epochs, minibatches);
    const int rc = population_update(h, pop, ext, dev_table, table_steps, K, nullptr, nullptr, nullptr, 0, c);
    return rc == SSG_OK ? update_call(h, c, stream) : rc;
}

int ssg_pop_update_sched(ssg_handle *h, const ssg_population *pop, const ssg_pop_ext *ext, const float *dev_table, int table_steps,
                         const int32_t *dev_sched, const int32_t *epochs, const int32_t *minibatches, int perm_epochs, int K,
                         const float *dev_x, const int32_t *dev_act, const float *dev_logp, const float *dev_adv, const float *dev_ret,
                         const int64_t *dev_perm, float *dev_adam_mv, float *dev_stats, void *dev_workspace, size_t workspace_nbytes,
                         void *stream)
{
    UpdateCall c = update_args("ssg_pop_update_sched", ext ? "population update_sched (ext)" : "population update_sched", ext != nullptr, dev_x,
                               dev_act, dev_logp, dev_adv, dev_ret, dev_perm, dev_stats, dev_workspace, workspace_nbytes);
    update_loop(c, dev_adam_mv, 0, 0);
    c.sched = true;
    const int rc = population_update(h, pop, ext, dev_table, table_steps, K, dev_sched, epochs, minibatches, perm_epochs, c);
    return rc == SSG_OK ? update_call(h, c, stream) : rc;
}

int ssg_pop_exploit(ssg_handle *h, const ssg_population *pop, const int32_t *src, float *dev_adam_mv, void *stream)
{
    ssg::MemberLayout lay;
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_population(h, pop, "ssg_pop_exploit", lay);
    if (rc != SSG_OK) return rc;
    if (!src || !dev_adam_mv) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_exploit: NULL src or dev_adam_mv");
    const int P = pop->n_members;
    for (int m = 0; m < P; ++m)
        if (src[m] < 0 || src[m] >= P) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_exploit: a source index is out of range");
    for (int m = 0; m < P; ++m)
        if (src[src[m]] != src[m]) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_exploit: a source is itself a destination (chained copy)");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_pop_exploit(pop_policy(*pop), P, src, dev_adam_mv, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("population exploit launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_pop_episode_stats(ssg_handle *h, int n_members, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                          double *dev_carry_return, int32_t *dev_carry_length, int64_t *dev_out, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_episode_stats: n_members must be in 1..SSG_POP_MAX_MEMBERS and divide the handle's n_envs");
    ssg::MemberLayout lay;
    rc = member_layout(h, n_members, "ssg_pop_episode_stats", true, lay);
    if (rc != SSG_OK) return rc;
    if (K < 1 || !dev_reward_KN || !dev_done_KN || !dev_carry_return || !dev_carry_length || !dev_out)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_episode_stats: K < 1 or a NULL buffer");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_pop_episode_stats(lay, K, h->cfg.n_envs, dev_reward_KN, dev_done_KN, dev_carry_return, dev_carry_length, dev_out,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("population episode stats launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 additions: evaluation.  Order of the refusals as for a population: no handle (BAD_ARG), no state blob (NOT_BOUND), everything
// the host can judge about the records (BAD_ARG), and only then the bank and the device — nothing is enqueued before all of it passed.
static int check_eval(ssg_handle *h, const ssg_eval *ev, const char *what)
{
    const std::string w(what);
    if (!ev) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_eval");
    if (ev->struct_size != sizeof(ssg_eval)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_eval.struct_size != sizeof(ssg_eval)");
    if (ev->flags & ~SSG_EVAL_GREEDY) return fail(h, SSG_ERR_BAD_ARG, w + ": unknown bit in ssg_eval.flags");
    if (ev->episodes_per_env < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": episodes_per_env < 1");
    if (ev->n_steps < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": n_steps < 1");
    if ((ev->flags & SSG_EVAL_GREEDY) && ev->dev_uniform_TN)
        return fail(h, SSG_ERR_BAD_ARG, w + ": dev_uniform_TN given together with SSG_EVAL_GREEDY (a greedy action reads no uniform)");
    if (!(h->cfg.flags & SSG_FLAG_AUTO_RESET))
        return fail(h, SSG_ERR_BAD_ARG, w + ": the handle lacks SSG_FLAG_AUTO_RESET (a done env would never start its next episode)");
    if (!ev->dev_obs || !ev->dev_act || !ev->dev_logp || !ev->dev_value || !ev->dev_reward || !ev->dev_done || !ev->dev_flags)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_obs, dev_act, dev_logp, dev_value, dev_reward, dev_done or dev_flags");
    if (!ev->dev_carry_return || !ev->dev_carry || !ev->dev_env_stats)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_carry_return, dev_carry or dev_env_stats");
    if (reinterpret_cast<uintptr_t>(ev->dev_carry) % 16 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_carry must be 16-byte aligned");
    return SSG_OK;
}

// both entry points behind their record
static int run_evaluate(ssg_handle *h, const PolicyCall &c, const ssg_eval *evp, void *stream)
{
    int rc = check_eval(h, evp, c.what);
    if (rc == SSG_OK) rc = prepare_steps(h, c, stream);
    if (rc != SSG_OK) return rc;
    const ssg_eval &ev = *evp;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const bool greedy = (ev.flags & SSG_EVAL_GREEDY) != 0;
    const int N = h->cfg.n_envs;
    // With a recorder bound (ssg_set_eval_recorder): the step kernel's terminal-observation rows are the record's for this call, and
    // each iteration gains the recorder's launches — obs (and the frames) ahead of the step, the rest ahead of the accounting.
    const bool rec = h->rec.struct_size != 0;
    TermObsGuard guard = {h, h->dev.term_obs};
    ssg::EvalRecLaunch rl = {};
    if (rec) {
        const ssg_eval_recorder &r = h->rec;
        h->dev.term_obs = r.dev_term_obs;
        rl = {r.n_tracked, r.capacity, h->cfg.history * (6 + h->cfg.n_beams), ev.episodes_per_env, ev.dev_carry, r.dev_cursor, r.dev_overflow,
              r.dev_obs, r.dev_next_obs, r.dev_act, r.dev_logp, r.dev_value, r.dev_reward, r.dev_done, r.dev_flags, r.dev_term_obs, r.dev_frames,
              r.frame_width, r.frame_height, r.frame_every, r.dev_frames ? (r.capacity + r.frame_every - 1) / r.frame_every : 0, r.frame_flags};
    }
    for (int k = 0; k < ev.n_steps; ++k) {
        const float *u = ev.dev_uniform_TN ? ev.dev_uniform_TN + (size_t)k * (size_t)N : nullptr;
        if (rec) {
            hipError_t e = ssg::launch_eval_record_obs(rl, h->rec_ids, ev.dev_obs, st);
            if (e == hipSuccess && rl.frames) e = ssg::launch_eval_record_frames(h->dev, h->dyn, rl, h->rec_ids, st);
            if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.what) + ": recorder launch: " + hipGetErrorString(e));
        }
        // (a bound observation filter is applied and never updated: evaluation is frozen)
        hipError_t e = policy_launch(h, c, {ev.dev_obs, u, ev.seed, ev.step0 + k, ev.dev_act, ev.dev_logp, ev.dev_value, nullptr, greedy}, st);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.what) + ": policy launch: " + hipGetErrorString(e));
        // (ssg_step as it stands, the call the rollouts make)
        rc = ssg_rollout_traj(h, ev.dev_act, 1, ev.dev_obs, ev.dev_reward, ev.dev_done, ev.dev_flags, 0, stream);
        if (rc != SSG_OK) return rc;
        if (rec) {
            e = ssg::launch_eval_record_step(rl, h->rec_ids, ev.dev_obs, ev.dev_act, ev.dev_logp, ev.dev_value, ev.dev_reward, ev.dev_done,
                                             ev.dev_flags, st);
            if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.what) + ": recorder launch: " + hipGetErrorString(e));
        }
        e = ssg::launch_eval_account(N, ev.episodes_per_env, ev.dev_reward, ev.dev_done, ev.dev_flags, ev.dev_carry_return, ev.dev_carry,
                                     ev.dev_env_stats, st);
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(c.what) + ": accounting launch: " + hipGetErrorString(e));
    }
    return SSG_OK;
}

int ssg_evaluate(ssg_handle *h, const ssg_policy *pol, const ssg_eval *ev, void *stream)
{
    PolicyCall c;
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = one_policy_call(h, pol, "ssg_evaluate", c);
    return rc == SSG_OK ? run_evaluate(h, c, ev, stream) : rc;
}

int ssg_pop_evaluate(ssg_handle *h, const ssg_population *pop, const ssg_eval *ev, void *stream)
{
    PolicyCall c;
    const int rc = population_call(h, pop, "ssg_pop_evaluate", c);
    return rc == SSG_OK ? run_evaluate(h, c, ev, stream) : rc;
}

int ssg_set_eval_recorder(ssg_handle *h, const ssg_eval_recorder *rec)
{
    const char *w = "ssg_set_eval_recorder: ";
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, std::string(w) + "NULL handle");
    if (!rec) { // unbind
        h->rec = ssg_eval_recorder{};
        return SSG_OK;
    }
    if (h->cfg.history > 2)
        return fail(h, SSG_ERR_UNSUPPORTED, std::string(w) + "history > 2 builds its rows in the frame-shift kernel: no terminal observations (ssg_set_terminal_obs)");
    if (!(h->cfg.flags & SSG_FLAG_AUTO_RESET))
        return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "only a handle that resets its done envs in-kernel (SSG_FLAG_AUTO_RESET) is evaluated and stores terminal observations");
    if (rec->struct_size != sizeof(ssg_eval_recorder)) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "ssg_eval_recorder.struct_size != sizeof(ssg_eval_recorder)");
    if (rec->reserved != 0) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "ssg_eval_recorder.reserved must be 0");
    if (rec->n_tracked < 1 || rec->n_tracked > SSG_EVAL_REC_MAX_ENVS) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "n_tracked must be in 1..SSG_EVAL_REC_MAX_ENVS");
    if (rec->capacity < 1) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "capacity < 1");
    if (!rec->env_ids || !rec->dev_obs || !rec->dev_next_obs || !rec->dev_act || !rec->dev_logp || !rec->dev_value || !rec->dev_reward ||
        !rec->dev_done || !rec->dev_flags || !rec->dev_cursor || !rec->dev_overflow || !rec->dev_term_obs)
        return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "NULL env_ids or a NULL required buffer (all but dev_frames are required)");
    for (int r = 0; r < rec->n_tracked; ++r) {
        if (rec->env_ids[r] < 0 || rec->env_ids[r] >= h->cfg.n_envs) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "an env id is outside [0, n_envs)");
        for (int q = 0; q < r; ++q)
            if (rec->env_ids[q] == rec->env_ids[r]) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "an env id repeats (two slots would record one env)");
    }
    if (rec->dev_frames) {
        if (rec->frame_width < 1 || rec->frame_height < 1 || rec->frame_width > 8192 || rec->frame_height > 8192)
            return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "frame_width and frame_height must be in 1..8192");
        if (rec->frame_every < 1) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "frame_every < 1");
        const long long slots = ((long long)rec->capacity + rec->frame_every - 1) / rec->frame_every;
        if (slots * rec->frame_width * rec->frame_height * 3 > (1ll << 31))
            return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "more than 2^31 bytes of frames per slot (ceil(capacity / frame_every) * width * height * 3)");
    }
    h->rec = *rec;
    std::copy(rec->env_ids, rec->env_ids + rec->n_tracked, h->rec_ids.e);
    std::fill(h->rec_ids.e + rec->n_tracked, h->rec_ids.e + SSG_EVAL_REC_MAX_ENVS, 0);
    h->rec.env_ids = h->rec_ids.e;
    return SSG_OK;
}

int ssg_get_eval_recorder(const ssg_handle *h, ssg_eval_recorder *out)
{
    if (!h || !out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_get_eval_recorder: NULL handle or out");
    *out = h->rec;
    return SSG_OK;
}

int ssg_obs_filter_workspace_nbytes(int n_envs, int obs_dim, int n_members, size_t *nbytes)
{
    if (!nbytes || n_envs < 1 || obs_dim < 1 || n_members < 1 || obs_dim > ssg::kFltMaxDim || n_members > SSG_POP_MAX_MEMBERS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_obs_filter_workspace_nbytes: NULL nbytes, an argument < 1, obs_dim or n_members out of range");
    *nbytes = ssg::filter_workspace_bytes(n_envs, obs_dim, n_members);
    return SSG_OK;
}

int ssg_set_obs_filter(ssg_handle *h, const ssg_obs_filter *f)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_set_obs_filter: NULL handle");
    if (!f) { // unbind
        h->flt = ssg_obs_filter{};
        h->flt_buffer = nullptr;
        return SSG_OK;
    }
    const int rc = check_filter(h, f, "ssg_set_obs_filter");
    if (rc != SSG_OK) return rc; // (the binding stays as it was, the buffer's too)
    h->flt = *f;
    h->flt_buffer = nullptr; // (a buffer belongs to the record it was bound beside)
    return SSG_OK;
}

int ssg_set_obs_filter_buffer(ssg_handle *h, double *dev_buffer)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_set_obs_filter_buffer: NULL handle");
    if (!h->flt.struct_size) return fail(h, SSG_ERR_BAD_ARG, "ssg_set_obs_filter_buffer: no observation filter is bound (ssg_set_obs_filter)");
    if (dev_buffer) {
        const int rc = check_filter_buffer(h, &h->flt, dev_buffer, "ssg_set_obs_filter_buffer");
        if (rc != SSG_OK) return rc; // (the binding stays as it was)
    }
    h->flt_buffer = dev_buffer; // (NULL unbinds)
    return SSG_OK;
}

int ssg_get_obs_filter_buffer(const ssg_handle *h, double **out)
{
    if (!h || !out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_get_obs_filter_buffer: NULL handle or out");
    *out = h->flt_buffer;
    return SSG_OK;
}

int ssg_get_obs_filter(const ssg_handle *h, ssg_obs_filter *out)
{
    if (!h || !out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_get_obs_filter: NULL handle or out");
    *out = h->flt;
    return SSG_OK;
}

// ABI 9 addition: per-minibatch advantage normalisation.  Host only: nothing here touches the device.
int ssg_ppo_adv_norm_nbytes(int n_members, size_t *nbytes)
{
    if (!nbytes || n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_adv_norm_nbytes: NULL nbytes or n_members outside 1..SSG_POP_MAX_MEMBERS");
    *nbytes = ssg::adv_norm_bytes(n_members);
    return SSG_OK;
}

int ssg_ppo_set_adv_norm(ssg_handle *h, int mode, int n_members, void *dev_scratch, size_t scratch_nbytes)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_norm: NULL handle");
    if (mode != SSG_ADV_NORM_BATCH && mode != SSG_ADV_NORM_MINIBATCH) {
        char buf[120];
        std::snprintf(buf, sizeof buf, "ssg_ppo_set_adv_norm: unknown mode %d (SSG_ADV_NORM_BATCH or SSG_ADV_NORM_MINIBATCH)", mode);
        return fail(h, SSG_ERR_BAD_ARG, buf); // (the binding stays as it was, here and below)
    }
    if (mode == SSG_ADV_NORM_BATCH) { // unbind
        h->adv_norm_mode = SSG_ADV_NORM_BATCH;
        h->adv_norm_members = 0;
        h->adv_norm_scratch = nullptr;
        h->adv_table = nullptr; // (a successful call drops a bound table: the mode named here is the handle's one source)
        h->adv_table_rows = h->adv_table_row = 0;
        return SSG_OK;
    }
    if (n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_norm: n_members must be in 1..SSG_POP_MAX_MEMBERS");
    if (!dev_scratch) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_norm: NULL dev_scratch with SSG_ADV_NORM_MINIBATCH");
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256 != 0)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_norm: dev_scratch must be 256-byte aligned");
    const size_t need = ssg::adv_norm_bytes(n_members);
    if (scratch_nbytes < need) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "ssg_ppo_set_adv_norm: scratch_nbytes of %zu bytes, n_members = %d needs %zu (ssg_ppo_adv_norm_nbytes)",
                      scratch_nbytes, n_members, need);
        return fail(h, SSG_ERR_BAD_ARG, buf);
    }
    h->adv_norm_mode = mode;
    h->adv_norm_members = n_members;
    h->adv_norm_scratch = dev_scratch;
    h->adv_table = nullptr;
    h->adv_table_rows = h->adv_table_row = 0;
    return SSG_OK;
}

int ssg_ppo_get_adv_norm(const ssg_handle *h, int *mode, int *n_members)
{
    if (!h || !mode || !n_members) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_get_adv_norm: NULL handle, mode or n_members");
    *mode = h->adv_norm_mode;
    *n_members = h->adv_norm_members;
    return SSG_OK;
}

// ABI 9 additions: the job-wide per-minibatch advantage normalisation.  The table binding is host only; the two launching calls refuse
// in the order of the data-parallel entry points: the handle, the state blob, what the host can judge, then the device.
int ssg_ppo_set_adv_table(ssg_handle *h, float *dev_table, int n_rows)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_table: NULL handle");
    if (!dev_table) { // unbind (n_rows is not read; the mode stays as it is)
        h->adv_table = nullptr;
        h->adv_table_rows = h->adv_table_row = 0;
        return SSG_OK;
    }
    if (reinterpret_cast<uintptr_t>(dev_table) % 16 != 0)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_table: dev_table must be 16-byte aligned"); // (the binding stays as it was, here and below)
    if (n_rows < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_set_adv_table: n_rows < 1");
    h->adv_table = dev_table;
    h->adv_table_rows = n_rows;
    h->adv_table_row = 0;
    h->adv_norm_mode = SSG_ADV_NORM_BATCH; // (the table is now the handle's one source of per-minibatch statistics)
    h->adv_norm_members = 0;
    h->adv_norm_scratch = nullptr;
    return SSG_OK;
}

int ssg_ppo_select_adv_row(ssg_handle *h, int row)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_select_adv_row: NULL handle");
    if (!h->adv_table) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_select_adv_row: no advantage table is bound (ssg_ppo_set_adv_table)");
    if (row < 0 || row >= h->adv_table_rows) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "ssg_ppo_select_adv_row: row %d is outside [0, %d), the bound table's rows", row, h->adv_table_rows);
        return fail(h, SSG_ERR_BAD_ARG, buf);
    }
    h->adv_table_row = row;
    return SSG_OK;
}

int ssg_ppo_get_adv_table(const ssg_handle *h, float **dev_table, int *n_rows, int *row)
{
    if (!h || !dev_table || !n_rows || !row) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_get_adv_table: NULL handle, dev_table, n_rows or row");
    *dev_table = h->adv_table;
    *n_rows = h->adv_table_rows;
    *row = h->adv_table_row;
    return SSG_OK;
}

int ssg_ppo_minibatch_adv_nbytes(int n_batches, size_t *nbytes)
{
    if (!nbytes || n_batches < 1 || n_batches > SSG_ADV_TABLE_MAX_ROWS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_minibatch_adv_nbytes: NULL nbytes or n_batches outside 1..SSG_ADV_TABLE_MAX_ROWS");
    *nbytes = ssg::minibatch_adv_bytes(n_batches);
    return SSG_OK;
}

int ssg_ppo_minibatch_adv_sums(ssg_handle *h, int64_t n_samples, const float *dev_adv, const int64_t *dev_perm, int epochs, int64_t n,
                               int64_t chunk, double *dev_out, void *dev_scratch, size_t scratch_nbytes, void *stream)
{
    const char *w = "ssg_ppo_minibatch_adv_sums: ";
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!dev_adv || !dev_perm || !dev_out || !dev_scratch) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "NULL dev_adv, dev_perm, dev_out or dev_scratch");
    if (n_samples < 1 || epochs < 1 || n < 1 || chunk < 1) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "n_samples, epochs, n or chunk < 1");
    if (chunk > n) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "chunk > n");
    const int64_t chunks = (n + chunk - 1) / chunk;
    if (chunks > SSG_ADV_TABLE_MAX_ROWS / epochs) { // (epochs * chunks > SSG_ADV_TABLE_MAX_ROWS, without the product)
        char buf[200];
        std::snprintf(buf, sizeof buf, "%d epochs x %lld chunks: more than SSG_ADV_TABLE_MAX_ROWS minibatches in one call (the grid's rows)", epochs,
                      (long long)chunks);
        return fail(h, SSG_ERR_BAD_ARG, std::string(w) + buf);
    }
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256 != 0) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "dev_scratch must be 256-byte aligned");
    const size_t need = ssg::minibatch_adv_bytes((int)(epochs * chunks));
    if (scratch_nbytes < need) {
        char buf[200];
        std::snprintf(buf, sizeof buf, "scratch_nbytes of %zu bytes, %lld minibatches need %zu (ssg_ppo_minibatch_adv_nbytes)", scratch_nbytes,
                      (long long)(epochs * chunks), need);
        return fail(h, SSG_ERR_BAD_ARG, std::string(w) + buf);
    }
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    const ssg::MinibatchAdvSums l = {dev_adv, dev_perm, n_samples, epochs, n, chunk, static_cast<double *>(dev_scratch), dev_out};
    hipError_t e = ssg::launch_minibatch_adv_sums(l, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("minibatch adv sums launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_set_minibatch_adv_rows(ssg_handle *h, int n_shards, int n_batches, const double *dev_rows, double adv_eps, float *dev_table,
                                   void *stream)
{
    const char *w = "ssg_ppo_set_minibatch_adv_rows: ";
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!dev_rows || !dev_table) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "NULL dev_rows or dev_table");
    if (n_shards < 1 || n_shards > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "n_shards must be in 1..SSG_DP_MAX_SHARDS");
    if (n_batches < 1 || n_batches > SSG_ADV_TABLE_MAX_ROWS) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "n_batches must be in 1..SSG_ADV_TABLE_MAX_ROWS");
    if (!std::isfinite(adv_eps)) return fail(h, SSG_ERR_BAD_ARG, std::string(w) + "adv_eps is not finite");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_minibatch_adv_rows(n_shards, n_batches, dev_rows, (float)adv_eps, dev_table, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("minibatch adv rows launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 addition: the minibatch permutations (shipsim_perm.h).  The arguments are judged first (BAD_ARG), then the handle's state blob
// (NOT_BOUND) and the device; nothing is enqueued before all of it passed.
int ssg_host_perm(uint64_t seed, int64_t update, int member, int epoch, int64_t n, int64_t first, int64_t count, int64_t *out)
{
    if (!out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_host_perm: NULL out");
    if (update < 0 || member < 0 || epoch < 0) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_host_perm: update, member or epoch < 0");
    if (n < 1 || (uint64_t)n > ssg::kPermMaxN) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_host_perm: n must be in 1..2^32");
    if (first < 0 || count < 1 || first >= n || count > n - first)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_host_perm: [first, first + count) must be a non-empty window of [0, n)");
    const ssg::PermKey key = ssg::perm_key(seed, (uint64_t)update, (uint32_t)member, (uint32_t)epoch, (uint64_t)n);
    for (int64_t i = 0; i < count; ++i) out[i] = ssg::perm_at(key, (uint32_t)(first + i));
    return SSG_OK;
}

static int run_perm(ssg_handle *h, const ssg::PermLaunch &l, void *stream, const char *what)
{
    int rc = pop_bound(h);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    const hipError_t e = static_cast<hipError_t>(ssg::launch_perm(l, stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_perm(ssg_handle *h, uint64_t seed, int64_t update, int member, int epochs, int64_t n_samples, int64_t *dev_perm, void *stream)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_perm: NULL handle");
    if (!dev_perm) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_perm: NULL dev_perm");
    if (update < 0 || member < 0 || epochs < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_perm: update or member < 0, or epochs < 1");
    if (n_samples < 1 || (uint64_t)n_samples > ssg::kPermMaxN) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_perm: n_samples must be in 1..2^32");
    ssg::PermLaunch l{};
    l.seed = seed;
    l.update = (uint64_t)update;
    l.member0 = member;
    l.members = 1;
    l.epochs = epochs;
    l.n = n_samples;
    l.out = dev_perm;
    return run_perm(h, l, stream, "ssg_ppo_perm");
}

int ssg_pop_perm(ssg_handle *h, uint64_t seed, int64_t update, int members, int K, int n, int perm_epochs, int64_t *dev_perm, void *stream)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_pop_perm: NULL handle");
    if (!dev_perm) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_perm: NULL dev_perm");
    if (update < 0 || K < 1 || perm_epochs < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_perm: update < 0, K < 1 or perm_epochs < 1");
    if (members < 1 || members > SSG_POP_MAX_MEMBERS) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_perm: members must be in 1..SSG_POP_MAX_MEMBERS");
    ssg::PermLaunch l{};
    l.seed = seed;
    l.update = (uint64_t)update;
    l.members = members;
    l.epochs = perm_epochs;
    l.K = K;
    l.out = dev_perm;
    ssg::MemberLayout lay; // (no table bound: the caller's n, which need not be an equal split of the handle's envs)
    const int rc = member_layout(h, members, "ssg_pop_perm", false, lay);
    if (rc != SSG_OK) return rc;
    if (lay.slices) {
        l.slices = lay.slices;
        l.n = (long long)K * lay.n; // (the widest row; n is not read)
    } else {
        if (n < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_perm: n < 1");
        l.n = (long long)K * n;
    }
    if ((uint64_t)l.n > ssg::kPermMaxN) return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_perm: a row of K * n entries exceeds 2^32");
    return run_perm(h, l, stream, "ssg_pop_perm");
}

// ssg_obs_filter_update (buffered false: dev_buffer is not read) and ssg_obs_filter_update_buffered, through the rollout loop's launcher
static int filter_update(ssg_handle *h, const ssg_obs_filter *f, bool buffered, double *dev_buffer, const double *dev_obs, void *stream,
                         const char *what)
{
    const std::string w(what);
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!f) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_obs_filter");
    rc = check_filter(h, f, what);
    if (rc != SSG_OK) return rc;
    if (buffered) {
        if (!dev_buffer) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_buffer");
        rc = check_filter_buffer(h, f, dev_buffer, what);
        if (rc != SSG_OK) return rc;
    }
    if (!dev_obs) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_obs");
    ssg::MemberLayout lay = whole_layout(h); // (one member: the whole handle, and the envs' split is not asked)
    if (f->n_members > 1) rc = member_layout(h, f->n_members, what, true, lay);
    if (rc == SSG_OK) rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_filter_update(dev_obs, f->obs_dim, lay, f->eps, f->dev_state, buffered ? dev_buffer : nullptr, f->dev_workspace,
                                             static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("observation filter launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_obs_filter_update(ssg_handle *h, const ssg_obs_filter *f, const double *dev_obs, void *stream)
{
    return filter_update(h, f, false, nullptr, dev_obs, stream, "ssg_obs_filter_update");
}

int ssg_obs_filter_update_buffered(ssg_handle *h, const ssg_obs_filter *f, double *dev_buffer, const double *dev_obs, void *stream)
{
    return filter_update(h, f, true, dev_buffer, dev_obs, stream, "ssg_obs_filter_update_buffered");
}

int ssg_obs_filter_merge_rows(ssg_handle *h, const ssg_obs_filter *f, const double *dev_base, const double *dev_rows, int n_rows, void *stream)
{
    const char *what = "ssg_obs_filter_merge_rows";
    const std::string w(what);
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!f) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_obs_filter");
    rc = check_filter(h, f, what);
    if (rc != SSG_OK) return rc;
    if (!dev_base || !dev_rows) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_base or dev_rows");
    if (reinterpret_cast<uintptr_t>(dev_base) % 8 != 0 || reinterpret_cast<uintptr_t>(dev_rows) % 8 != 0)
        return fail(h, SSG_ERR_BAD_ARG, w + ": dev_base and dev_rows must be 8-byte aligned");
    if (n_rows < 1 || n_rows > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_rows must be in 1..SSG_DP_MAX_SHARDS");
    // (the kernel reads base and rows while it writes the state: a block of either that overlaps the state's would be read half merged)
    const uintptr_t block = (uintptr_t)f->n_members * SSG_FILTER_ROWS * (uintptr_t)f->obs_dim * sizeof(double);
    const uintptr_t st = reinterpret_cast<uintptr_t>(f->dev_state), b0 = reinterpret_cast<uintptr_t>(dev_base), r0 = reinterpret_cast<uintptr_t>(dev_rows);
    if (b0 < st + block && st < b0 + block) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_base overlaps the filter's dev_state");
    if (r0 < st + block && st < r0 + block * (uintptr_t)n_rows) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_rows overlaps the filter's dev_state");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_filter_merge_rows(dev_base, dev_rows, n_rows, f->obs_dim, f->n_members, f->eps, f->dev_state,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("observation filter rows merge launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 addition: the return filter.  Everything the host can judge comes first (BAD_ARG), then the handle's state blob and the device.
int ssg_ret_filter_workspace_nbytes(int n_envs, int K, int n_members, size_t *nbytes)
{
    if (!nbytes || n_envs < 1 || K < 1 || n_members < 1 || K > SSG_RET_FILTER_MAX_STEPS || n_members > SSG_POP_MAX_MEMBERS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ret_filter_workspace_nbytes: NULL nbytes, an argument < 1, K or n_members out of range");
    *nbytes = ssg::ret_filter_workspace_bytes(n_envs, K, n_members);
    return SSG_OK;
}

// What the three launching calls ask of their record, in ssg_ret_filter_apply's order, up to the buffers (which differ): the record, K and
// the stride.  job: ssg_ret_filter_batches / ssg_ret_filter_apply_rows, which serve one updating member.  lay: the launch's layout.
static int check_ret_filter(ssg_handle *h, const ssg_ret_filter *f, int K, int64_t step_stride_envs, const std::string &w, bool job,
                            ssg::MemberLayout &lay)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL handle");
    if (!f) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_ret_filter");
    if (f->struct_size != sizeof(ssg_ret_filter)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_ret_filter.struct_size != sizeof(ssg_ret_filter)");
    if (f->flags & ~SSG_RET_FILTER_UPDATE) return fail(h, SSG_ERR_BAD_ARG, w + ": unknown bit in ssg_ret_filter.flags");
    const int P = f->n_members, N = h->cfg.n_envs;
    if (P < 1 || P > SSG_POP_MAX_MEMBERS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_members must be in 1..SSG_POP_MAX_MEMBERS");
    if (job && P != 1) return fail(h, SSG_ERR_BAD_ARG, w + ": a job-wide filter has one member (n_members != 1)");
    if (job && !(f->flags & SSG_RET_FILTER_UPDATE))
        return fail(h, SSG_ERR_BAD_ARG, w + ": the record is frozen (SSG_RET_FILTER_UPDATE clear): a frozen filter needs no rows, call ssg_ret_filter_apply");
    int rc = member_layout(h, P, w.c_str(), true, lay); // (asked for one member too, which then runs on the whole handle)
    if (rc != SSG_OK) return rc;
    if (P == 1) lay = whole_layout(h);
    if (!(f->clip >= 0.0) || !(f->eps >= 0.0)) return fail(h, SSG_ERR_BAD_ARG, w + ": clip and eps must be >= 0 (and not NaN)");
    if (!f->dev_gamma || !f->dev_state || !f->dev_carry || !f->dev_workspace)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_gamma, dev_state, dev_carry or dev_workspace");
    if (K < 1 || K > SSG_RET_FILTER_MAX_STEPS) return fail(h, SSG_ERR_BAD_ARG, w + ": K must be in 1..SSG_RET_FILTER_MAX_STEPS");
    if (step_stride_envs < N) return fail(h, SSG_ERR_BAD_ARG, w + ": step_stride_envs < n_envs");
    return SSG_OK;
}

// ... and after the buffers: the workspace, then the handle's state blob
static int check_ret_filter_workspace(ssg_handle *h, const ssg_ret_filter *f, int K, const std::string &w)
{
    char buf[200];
    const size_t need = ssg::ret_filter_workspace_bytes(h->cfg.n_envs, K, f->n_members);
    if (f->workspace_nbytes < need) {
        std::snprintf(buf, sizeof buf, ": workspace_nbytes %zu < %zu (ssg_ret_filter_workspace_nbytes)", f->workspace_nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    return check_ready(h, false);
}

static ssg::RetFilterLaunch ret_filter_launch(const ssg_ret_filter *f, int K, int64_t step_stride_envs, const ssg::MemberLayout &lay)
{
    ssg::RetFilterLaunch l{};
    l.K = K;
    l.stride = (size_t)step_stride_envs;
    l.lay = lay;
    l.update = (f->flags & SSG_RET_FILTER_UPDATE) != 0;
    l.clip = f->clip;
    l.eps = f->eps;
    l.gamma = f->dev_gamma;
    l.state = f->dev_state;
    l.carry = f->dev_carry;
    l.workspace = f->dev_workspace;
    return l;
}

int ssg_ret_filter_apply(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                         int64_t step_stride_envs, double *dev_reward_out_KN, double *dev_denom_KP, void *stream)
{
    const std::string w("ssg_ret_filter_apply");
    ssg::MemberLayout lay;
    int rc = check_ret_filter(h, f, K, step_stride_envs, w, false, lay);
    if (rc != SSG_OK) return rc;
    if (!dev_reward_KN || !dev_done_KN || !dev_reward_out_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL reward, done or output buffer");
    if (dev_reward_out_KN == dev_reward_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": the output buffer must not be the reward buffer");
    rc = check_ret_filter_workspace(h, f, K, w);
    if (rc != SSG_OK) return rc;
    ssg::RetFilterLaunch l = ret_filter_launch(f, K, step_stride_envs, lay);
    l.rew = dev_reward_KN;
    l.done = dev_done_KN;
    l.out = dev_reward_out_KN;
    l.denom_out = dev_denom_KP;
    hipError_t e = ssg::launch_ret_filter(l, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("return filter launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// the rows of a job-wide call, f64 [n_rows][K][SSG_FILTER_ROWS], against the record's state: the chain reads them while it writes the state
static int check_ret_filter_rows(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_rows, int n_rows, const std::string &w)
{
    if (!dev_rows) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL rows");
    if (reinterpret_cast<uintptr_t>(dev_rows) % 8 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": the rows must be 8-byte aligned");
    if (n_rows < 1 || n_rows > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_rows must be in 1..SSG_DP_MAX_SHARDS");
    const uintptr_t st = reinterpret_cast<uintptr_t>(f->dev_state), st_bytes = SSG_FILTER_ROWS * sizeof(double);
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(dev_rows), r_bytes = (uintptr_t)n_rows * (uintptr_t)K * SSG_FILTER_ROWS * sizeof(double);
    if (r0 < st + st_bytes && st < r0 + r_bytes) return fail(h, SSG_ERR_BAD_ARG, w + ": the rows overlap the filter's dev_state");
    return SSG_OK;
}

int ssg_ret_filter_batches(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_reward_KN, const uint8_t *dev_done_KN,
                           int64_t step_stride_envs, double *dev_rows_K4, void *stream)
{
    const std::string w("ssg_ret_filter_batches");
    ssg::MemberLayout lay;
    int rc = check_ret_filter(h, f, K, step_stride_envs, w, true, lay);
    if (rc != SSG_OK) return rc;
    if (!dev_reward_KN || !dev_done_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL reward or done buffer");
    rc = check_ret_filter_rows(h, f, K, dev_rows_K4, 1, w);
    if (rc == SSG_OK) rc = check_ret_filter_workspace(h, f, K, w);
    if (rc != SSG_OK) return rc;
    ssg::RetFilterLaunch l = ret_filter_launch(f, K, step_stride_envs, lay);
    l.rew = dev_reward_KN;
    l.done = dev_done_KN;
    hipError_t e = ssg::launch_ret_filter_batches(l, dev_rows_K4, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("return filter batches launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ret_filter_apply_rows(ssg_handle *h, const ssg_ret_filter *f, int K, const double *dev_rows_WK4, int n_rows, const double *dev_reward_KN,
                              int64_t step_stride_envs, double *dev_reward_out_KN, double *dev_denom_K, void *stream)
{
    const std::string w("ssg_ret_filter_apply_rows");
    ssg::MemberLayout lay;
    int rc = check_ret_filter(h, f, K, step_stride_envs, w, true, lay);
    if (rc != SSG_OK) return rc;
    if (!dev_reward_KN || !dev_reward_out_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL reward or output buffer");
    if (dev_reward_out_KN == dev_reward_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": the output buffer must not be the reward buffer");
    rc = check_ret_filter_rows(h, f, K, dev_rows_WK4, n_rows, w);
    if (rc == SSG_OK) rc = check_ret_filter_workspace(h, f, K, w);
    if (rc != SSG_OK) return rc;
    ssg::RetFilterLaunch l = ret_filter_launch(f, K, step_stride_envs, lay);
    l.rew = dev_reward_KN;
    l.out = dev_reward_out_KN;
    l.denom_out = dev_denom_K;
    hipError_t e = ssg::launch_ret_filter_rows(l, dev_rows_WK4, n_rows, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("return filter rows launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 addition: the episode log.  Everything the host can judge comes first (BAD_ARG), then the handle's state blob and the device.
int ssg_episode_log_workspace_nbytes(int n_envs, int K, size_t *nbytes)
{
    if (!nbytes || n_envs < 1 || K < 1 || (long long)K * ssg::filter_tiles(n_envs) > SSG_EPISODE_LOG_MAX_CELLS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_episode_log_workspace_nbytes: NULL nbytes, an argument < 1 or K * tiles above SSG_EPISODE_LOG_MAX_CELLS");
    *nbytes = ssg::episode_log_workspace_bytes(n_envs, K);
    return SSG_OK;
}

// What ssg_episode_log_append asks, in its order, and its launch record; ssg_job_episode_log_shard asks the same first.
static int check_episode_log(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, const double *dev_reward_KN,
                             const uint8_t *dev_done_KN, const uint8_t *dev_flags_KN, int64_t step_stride_envs, const std::string &w,
                             ssg::EpisodeLogLaunch &l)
{
    char buf[200];
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL handle");
    if (!log) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_episode_log");
    if (log->struct_size != sizeof(ssg_episode_log)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_episode_log.struct_size != sizeof(ssg_episode_log)");
    if (log->capacity < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": capacity < 1");
    const int P = log->n_members, N = h->cfg.n_envs;
    if (P < 1 || P > SSG_POP_MAX_MEMBERS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_members must be in 1..SSG_POP_MAX_MEMBERS");
    ssg::MemberLayout lay;
    int rc = member_layout(h, P, w.c_str(), true, lay); // (asked for one member too, which then owns the whole handle)
    if (rc != SSG_OK) return rc;
    if (P == 1) lay = whole_layout(h);
    if (!log->dev_records || !log->dev_head || !log->dev_carry_return || !log->dev_carry || !log->dev_workspace)
        return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_records, dev_head, dev_carry_return, dev_carry or dev_workspace");
    if (reinterpret_cast<uintptr_t>(log->dev_records) % 16 != 0 || reinterpret_cast<uintptr_t>(log->dev_workspace) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(log->dev_carry) % 8 != 0 || reinterpret_cast<uintptr_t>(log->dev_head) % 8 != 0)
        return fail(h, SSG_ERR_BAD_ARG, w + ": dev_records and dev_workspace must be 16-byte aligned, dev_carry and dev_head 8-byte aligned");
    if (K < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": K < 1");
    if ((long long)K * ssg::filter_tiles(N) > SSG_EPISODE_LOG_MAX_CELLS)
        return fail(h, SSG_ERR_BAD_ARG, w + ": K * ceil(n_envs / 256) above SSG_EPISODE_LOG_MAX_CELLS (split the rows into several calls)");
    if (step_stride_envs < N) return fail(h, SSG_ERR_BAD_ARG, w + ": step_stride_envs < n_envs");
    if (!dev_reward_KN || !dev_done_KN) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL reward or done buffer");
    const size_t need = ssg::episode_log_workspace_bytes(N, K);
    if (log->workspace_nbytes < need) {
        std::snprintf(buf, sizeof buf, ": workspace_nbytes %zu < %zu (ssg_episode_log_workspace_nbytes)", log->workspace_nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    l.K = K;
    l.N = N;
    l.stride = (size_t)step_stride_envs;
    l.step0 = step0;
    l.env_base = h->cfg.env_id_base;
    l.capacity = log->capacity;
    l.lay = lay;
    l.rew = dev_reward_KN;
    l.done = dev_done_KN;
    l.flags = dev_flags_KN;
    l.carry_ret = log->dev_carry_return;
    l.carry = log->dev_carry;
    l.head = log->dev_head;
    l.workspace = log->dev_workspace;
    l.records = log->dev_records;
    return SSG_OK;
}

int ssg_episode_log_append(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, const double *dev_reward_KN,
                           const uint8_t *dev_done_KN, const uint8_t *dev_flags_KN, int64_t step_stride_envs, void *stream)
{
    ssg::EpisodeLogLaunch l;
    int rc = check_episode_log(h, log, K, step0, dev_reward_KN, dev_done_KN, dev_flags_KN, step_stride_envs, "ssg_episode_log_append", l);
    if (rc != SSG_OK) return rc;
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_episode_log(l, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("episode log launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 addition: the job-wide episode log.  The same order: the arguments (BAD_ARG), then the handle's state blob and the device.
int ssg_job_episode_log_block_nbytes(int rows, int stage, size_t *nbytes)
{
    if (!nbytes || rows < 1 || rows > SSG_EPISODE_LOG_MAX_CELLS || stage < 1)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_job_episode_log_block_nbytes: NULL nbytes, rows outside 1..SSG_EPISODE_LOG_MAX_CELLS or stage < 1");
    *nbytes = ssg::episode_log_block_bytes(rows, stage);
    return SSG_OK;
}

// [p, p + n) against the ring and the head of `log`
static bool overlaps_ring(const ssg_episode_log *log, const void *p, size_t n)
{
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(p), b1 = b0 + n;
    const uintptr_t r0 = reinterpret_cast<uintptr_t>(log->dev_records), r1 = r0 + (uintptr_t)log->capacity * sizeof(ssg_episode_record);
    const uintptr_t h0 = reinterpret_cast<uintptr_t>(log->dev_head), h1 = h0 + 2 * sizeof(int64_t);
    return (b0 < r1 && r0 < b1) || (b0 < h1 && h0 < b1);
}

int ssg_job_episode_log_shard(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, const double *dev_reward_KN,
                              const uint8_t *dev_done_KN, const uint8_t *dev_flags_KN, int64_t step_stride_envs, int rows, int stage,
                              void *dev_block, size_t block_nbytes, void *stream)
{
    const std::string w("ssg_job_episode_log_shard");
    char buf[200];
    ssg::EpisodeLogLaunch l;
    int rc = check_episode_log(h, log, K, step0, dev_reward_KN, dev_done_KN, dev_flags_KN, step_stride_envs, w, l);
    if (rc != SSG_OK) return rc;
    if (log->n_members != 1) return fail(h, SSG_ERR_BAD_ARG, w + ": a job-wide log has one member (n_members != 1)");
    if (rows > SSG_EPISODE_LOG_MAX_CELLS) return fail(h, SSG_ERR_BAD_ARG, w + ": rows above SSG_EPISODE_LOG_MAX_CELLS");
    if (rows < 1 || K > rows) return fail(h, SSG_ERR_BAD_ARG, w + ": K must be in 1..rows");
    if (stage < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": stage < 1");
    if (!dev_block) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_block");
    if (reinterpret_cast<uintptr_t>(dev_block) % 16 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_block must be 16-byte aligned");
    const size_t need = ssg::episode_log_block_bytes(rows, stage);
    if (block_nbytes < need) {
        std::snprintf(buf, sizeof buf, ": block_nbytes %zu < %zu (ssg_job_episode_log_block_nbytes)", block_nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    if (overlaps_ring(log, dev_block, need)) return fail(h, SSG_ERR_BAD_ARG, w + ": the block overlaps the ring or the head");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_episode_log_shard(l, rows, stage, dev_block, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("episode log shard launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_job_episode_log_merge_blocks(ssg_handle *h, const ssg_episode_log *log, int K, int64_t step0, int rows, int stage, const void *dev_blocks,
                                     int n_blocks, void *stream)
{
    const std::string w("ssg_job_episode_log_merge_blocks");
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, w + ": NULL handle");
    if (!log) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL ssg_episode_log");
    if (log->struct_size != sizeof(ssg_episode_log)) return fail(h, SSG_ERR_BAD_ARG, w + ": ssg_episode_log.struct_size != sizeof(ssg_episode_log)");
    if (log->capacity < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": capacity < 1");
    if (log->n_members != 1) return fail(h, SSG_ERR_BAD_ARG, w + ": a job-wide log has one member (n_members != 1)");
    if (!log->dev_records || !log->dev_head || !dev_blocks) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_records, dev_head or dev_blocks");
    if (reinterpret_cast<uintptr_t>(log->dev_records) % 16 != 0 || reinterpret_cast<uintptr_t>(dev_blocks) % 16 != 0 ||
        reinterpret_cast<uintptr_t>(log->dev_head) % 8 != 0)
        return fail(h, SSG_ERR_BAD_ARG, w + ": dev_records and dev_blocks must be 16-byte aligned, dev_head 8-byte aligned");
    if (n_blocks < 1 || n_blocks > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, w + ": n_blocks must be in 1..SSG_DP_MAX_SHARDS");
    if (rows > SSG_EPISODE_LOG_MAX_CELLS) return fail(h, SSG_ERR_BAD_ARG, w + ": rows above SSG_EPISODE_LOG_MAX_CELLS");
    if (rows < 1 || K < 1 || K > rows) return fail(h, SSG_ERR_BAD_ARG, w + ": K must be in 1..rows");
    if (stage < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": stage < 1");
    if (overlaps_ring(log, dev_blocks, (size_t)n_blocks * ssg::episode_log_block_bytes(rows, stage)))
        return fail(h, SSG_ERR_BAD_ARG, w + ": the blocks overlap the ring or the head");
    const int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_episode_log_merge(K, step0, rows, stage, dev_blocks, n_blocks, log->dev_records, log->capacity, log->dev_head,
                                                 static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("episode log merge launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

// ABI 9 addition: the update report.  Everything the host can judge comes first (BAD_ARG), then the device; nothing is enqueued before.
int ssg_report_clip_bounds(double clip, float out_lo_hi[2])
{
    if (!out_lo_hi || !(clip > 0.0)) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_report_clip_bounds: NULL out_lo_hi or clip <= 0");
    ssg::report_clip_bounds(clip, out_lo_hi);
    return SSG_OK;
}

int ssg_ppo_report_workspace_nbytes(int n_envs, int n_members, size_t *nbytes)
{
    if (!nbytes || n_envs < 1 || n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_ppo_report_workspace_nbytes: NULL nbytes, an argument < 1 or n_members above SSG_POP_MAX_MEMBERS");
    *nbytes = ssg::report_scratch_bytes(n_envs, n_members);
    return SSG_OK;
}

// The body of ssg_ppo_report and ssg_pop_report: the launch record is complete but for the checks both calls share.
static int report(ssg_handle *h, ssg::ReportLaunch &l, bool need_bounds, void *dev_scratch, size_t scratch_nbytes, void *stream, const char *what)
{
    const std::string w(what);
    char buf[200];
    if (!l.val || !l.ret || !l.adv || (!l.out && !l.row)) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL value, ret, adv or out buffer");
    if (l.K < 1 || l.N < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": K and N must be >= 1");
    const int given = (l.act != nullptr) + (l.logp != nullptr) + (l.lpa != nullptr);
    if (given != 0 && given != 3) return fail(h, SSG_ERR_BAD_ARG, w + ": dev_act, dev_logp and dev_logp_all_new go together: all three or none");
    if (given && need_bounds && !l.bounds) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_bounds with the post-update group");
    if (l.stats && l.n_cols != 4 && l.n_cols != 8) return fail(h, SSG_ERR_BAD_ARG, w + ": n_cols must be 4 or 8");
    if (l.stats && l.rows_max < 1) return fail(h, SSG_ERR_BAD_ARG, w + ": fewer than 1 stats row");
    if (!dev_scratch) return fail(h, SSG_ERR_BAD_ARG, w + ": NULL dev_scratch");
    if (reinterpret_cast<uintptr_t>(dev_scratch) % 256 != 0) return fail(h, SSG_ERR_BAD_ARG, w + ": the scratch must be 256-byte aligned");
    const size_t need = (size_t)l.lay.members * (size_t)ssg::ppo_gae_blocks(l.lay.n) * ssg::kReportSums * sizeof(double);
    if (scratch_nbytes < need) {
        std::snprintf(buf, sizeof buf, ": scratch of %zu bytes, this call needs %zu (ssg_ppo_report_workspace_nbytes)", scratch_nbytes, need);
        return fail(h, SSG_ERR_BAD_ARG, w + buf);
    }
    const int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    l.part = static_cast<double *>(dev_scratch);
    hipError_t e = ssg::launch_report(l, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("report launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_ppo_report(ssg_handle *h, int K, int N, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_logp_all_new, double clip, const float *dev_stats,
                   int n_rows, int n_cols, void *dev_scratch, size_t scratch_nbytes, double *dev_out24, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    ssg::ReportLaunch l = {};
    l.K = K;
    l.N = N;
    l.lay = ssg::MemberLayout{1, N, nullptr};
    l.val = dev_value_KN;
    l.ret = dev_ret_KN;
    l.adv = dev_adv_KN;
    l.act = dev_act;
    l.logp = dev_logp;
    l.lpa = dev_logp_all_new;
    if (dev_logp_all_new) {
        if (!(clip > 0.0)) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report: clip must be > 0 with the post-update group");
        float b[2];
        ssg::report_clip_bounds(clip, b);
        l.lo = b[0];
        l.hi = b[1];
    }
    l.stats = dev_stats;
    l.rows_max = n_rows;
    l.n_cols = n_cols;
    l.out = dev_out24;
    return report(h, l, false, dev_scratch, scratch_nbytes, stream, "ssg_ppo_report");
}

// The sum row of one rank's shard: ssg_ppo_report's checks and walk, then the launch that stores the totals instead of the record.
int ssg_ppo_report_sums(ssg_handle *h, int K, int N, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                        const int32_t *dev_act, const float *dev_logp, const float *dev_logp_all_new, double clip, void *dev_scratch,
                        size_t scratch_nbytes, double *dev_row12, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    ssg::ReportLaunch l = {};
    l.K = K;
    l.N = N;
    l.lay = ssg::MemberLayout{1, N, nullptr};
    l.val = dev_value_KN;
    l.ret = dev_ret_KN;
    l.adv = dev_adv_KN;
    l.act = dev_act;
    l.logp = dev_logp;
    l.lpa = dev_logp_all_new;
    if (dev_logp_all_new) {
        if (!(clip > 0.0)) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report_sums: clip must be > 0 with the post-update group");
        float b[2];
        ssg::report_clip_bounds(clip, b);
        l.lo = b[0];
        l.hi = b[1];
    }
    l.row = dev_row12;
    return report(h, l, false, dev_scratch, scratch_nbytes, stream, "ssg_ppo_report_sums");
}

// The job's record from the gathered rows: host checks, then one launch.
int ssg_ppo_report_rows(ssg_handle *h, int n_rows, const double *dev_rows, const float *dev_stats, int n_stat_rows, int n_cols, int per_shard,
                        double *dev_out, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (!dev_rows || !dev_out) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report_rows: NULL dev_rows or dev_out");
    if (n_rows < 1 || n_rows > SSG_DP_MAX_SHARDS) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report_rows: n_rows must be in 1..SSG_DP_MAX_SHARDS");
    if (dev_stats && n_cols != 4 && n_cols != 8) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report_rows: n_cols must be 4 or 8");
    if (dev_stats && n_stat_rows < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_ppo_report_rows: fewer than 1 stats row");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_report_rows(n_rows, dev_rows, dev_stats, n_stat_rows, n_cols, per_shard != 0, dev_out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("report rows launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_pop_report(ssg_handle *h, int n_members, int K, const float *dev_value_KN, const float *dev_ret_KN, const float *dev_adv_KN,
                   const int32_t *dev_act, const float *dev_logp, const float *dev_logp_all_new, const float *dev_bounds,
                   const float *dev_stats, int rows_max, int n_cols, const int32_t *dev_rows, void *dev_scratch, size_t scratch_nbytes,
                   double *dev_out, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_pop_report: n_members must be in 1..SSG_POP_MAX_MEMBERS");
    ssg::ReportLaunch l = {};
    rc = member_layout(h, n_members, "ssg_pop_report", true, l.lay);
    if (rc != SSG_OK) return rc;
    l.K = K;
    l.N = h->cfg.n_envs;
    l.val = dev_value_KN;
    l.ret = dev_ret_KN;
    l.adv = dev_adv_KN;
    l.act = dev_act;
    l.logp = dev_logp;
    l.lpa = dev_logp_all_new;
    l.bounds = dev_bounds;
    l.stats = dev_stats;
    l.rows = dev_stats ? dev_rows : nullptr;
    l.rows_max = rows_max;
    l.n_cols = n_cols;
    l.out = dev_out;
    return report(h, l, true, dev_scratch, scratch_nbytes, stream, "ssg_pop_report");
}

int ssg_eval_account(ssg_handle *h, int episodes_per_env, const double *dev_reward, const uint8_t *dev_done, const uint8_t *dev_flags,
                     double *dev_carry_return, int32_t *dev_carry, int64_t *dev_env_stats, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (episodes_per_env < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_eval_account: episodes_per_env < 1");
    if (!dev_reward || !dev_done || !dev_flags || !dev_carry_return || !dev_carry || !dev_env_stats)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_eval_account: NULL dev_reward, dev_done, dev_flags, dev_carry_return, dev_carry or dev_env_stats");
    if (reinterpret_cast<uintptr_t>(dev_carry) % 16 != 0) return fail(h, SSG_ERR_BAD_ARG, "ssg_eval_account: dev_carry must be 16-byte aligned");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_eval_account(h->cfg.n_envs, episodes_per_env, dev_reward, dev_done, dev_flags, dev_carry_return, dev_carry,
                                            dev_env_stats, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("evaluation accounting launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_eval_reduce(ssg_handle *h, int n_members, const int64_t *dev_env_stats, int64_t *dev_member_stats, void *stream)
{
    int rc = pop_bound(h);
    if (rc != SSG_OK) return rc;
    if (n_members < 1 || n_members > SSG_POP_MAX_MEMBERS)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_eval_reduce: n_members must be in 1..SSG_POP_MAX_MEMBERS and divide the handle's n_envs");
    ssg::MemberLayout lay = whole_layout(h); // (one policy's reduce over the whole handle: the slices do not enter)
    if (n_members > 1) rc = member_layout(h, n_members, "ssg_eval_reduce", true, lay);
    if (rc != SSG_OK) return rc;
    if (!dev_env_stats || !dev_member_stats) return fail(h, SSG_ERR_BAD_ARG, "ssg_eval_reduce: NULL dev_env_stats or dev_member_stats");
    rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_eval_reduce(lay, dev_env_stats, dev_member_stats, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("evaluation reduce launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_fill_actions(ssg_handle *h, uint64_t seed, uint64_t step0, int K, int32_t *dev_actions, void *stream)
{
    if (!h || !dev_actions || K < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_fill_actions: bad argument");
    hipError_t e = ssg::launch_fill_actions(seed, step0, K, h->cfg.env_id_base, h->cfg.n_envs, dev_actions,
                                            static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("fill_actions launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_set_terminal_obs(ssg_handle *h, double *dev_term_obs)
{
    if (!h) return SSG_ERR_BAD_ARG;
    if (dev_term_obs && h->cfg.history > 2)
        return fail(h, SSG_ERR_UNSUPPORTED, "ssg_set_terminal_obs: history > 2 builds its rows in the frame-shift kernel (reset the done envs with a masked ssg_reset instead)");
    if (dev_term_obs && !(h->cfg.flags & SSG_FLAG_AUTO_RESET))
        return fail(h, SSG_ERR_BAD_ARG, "ssg_set_terminal_obs: only a handle that resets its done envs in-kernel (SSG_FLAG_AUTO_RESET) replaces terminal observations");
    h->dev.term_obs = dev_term_obs;
    return SSG_OK;
}

int ssg_set_timeout_boot(ssg_handle *h, const ssg_timeout_boot *rec)
{
    if (!h) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_set_timeout_boot: NULL handle");
    if (!rec) {
        h->tob = ssg_timeout_boot{};
        return SSG_OK;
    }
    if (h->cfg.history > 2)
        return fail(h, SSG_ERR_UNSUPPORTED, "ssg_set_timeout_boot: history > 2 builds its rows in the frame-shift kernel: no terminal observations (ssg_set_terminal_obs)");
    if (!(h->cfg.flags & SSG_FLAG_AUTO_RESET))
        return fail(h, SSG_ERR_BAD_ARG, "ssg_set_timeout_boot: only a handle that resets its done envs in-kernel (SSG_FLAG_AUTO_RESET) stores terminal observations");
    if (rec->struct_size != sizeof(ssg_timeout_boot)) return fail(h, SSG_ERR_BAD_ARG, "ssg_set_timeout_boot: ssg_timeout_boot.struct_size != sizeof(ssg_timeout_boot)");
    if (rec->rows < 1) return fail(h, SSG_ERR_BAD_ARG, "ssg_set_timeout_boot: rows < 1");
    if (!rec->dev_term_obs_KND || !rec->dev_boot_KN) return fail(h, SSG_ERR_BAD_ARG, "ssg_set_timeout_boot: NULL dev_term_obs_KND or dev_boot_KN");
    h->tob = *rec;
    return SSG_OK;
}

int ssg_get_timeout_boot(const ssg_handle *h, ssg_timeout_boot *out)
{
    if (!h || !out) return fail(nullptr, SSG_ERR_BAD_ARG, "ssg_get_timeout_boot: NULL handle or out");
    *out = h->tob;
    return SSG_OK;
}

#ifndef SSG_STAMPS
int ssg_debug_launch_clock(ssg_handle *h, uint64_t *dev_buf)
{
    if (!h) return SSG_ERR_BAD_ARG;
    h->dev.dbg = reinterpret_cast<unsigned long long *>(dev_buf);
    return SSG_OK;
}
#else
int ssg_debug_launch_clock(ssg_handle *h, uint64_t *) { return fail(h, SSG_ERR_UNSUPPORTED, "ssg_debug_launch_clock: a -DSSG_STAMPS build uses the buffer for its own stamps"); }
#endif

#ifdef SSG_STAMPS
// diagnostic builds only: where per-wave s_memtime stamps go (16 u64 per wave)
int ssg_debug_set_stamp_buffer(ssg_handle *h, void *dev_buf)
{
    if (!h) return SSG_ERR_BAD_ARG;
    h->dev.dbg = static_cast<unsigned long long *>(dev_buf);
    return SSG_OK;
}
#endif

int ssg_generate_bank(ssg_handle *h, uint64_t seed, double width_frac, double *dev_bank, int n_maps, double *dev_raw,
                      void *stream)
{
    if (!h || !dev_bank || n_maps < 1 || !(width_frac > 0.0) || !(width_frac <= 1.0))
        return fail(h, SSG_ERR_BAD_ARG, "ssg_generate_bank: bad argument");
    hipError_t e = ssg::launch_generate_bank(seed, n_maps, h->cfg.n_goals, h->cfg.width, h->cfg.height, width_frac,
                                             h->cfg.spawn_x, h->cfg.spawn_y, dev_bank, dev_raw, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("generate_bank launch: ") + hipGetErrorString(e));
    if (dev_bank == h->bank) h->dyn_step.bank_changed(); // regenerated in place
    return SSG_OK;
}

int ssg_refill_worlds(ssg_handle *h, uint64_t seed, double width_frac, double *dev_raw, void *stream)
{
    int rc = check_ready(h, true);
    if (rc != SSG_OK) return rc;
    if (h->cfg.map_ring <= 0) return fail(h, SSG_ERR_BAD_ARG, "ssg_refill_worlds: the handle was not created with map_ring");
    if (!(width_frac > 0.0) || !(width_frac <= 1.0)) return fail(h, SSG_ERR_BAD_ARG, "ssg_refill_worlds: bad width_frac");
    h->ring.seed = seed;
    h->ring.width_frac = width_frac;
    if (!h->zeroed) { // zero a freshly bound blob HERE, before the rings' counters are written (a later full ssg_reset must not wipe them)
        hipError_t e = hipMemsetAsync(h->state, 0, h->layout.nbytes, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("ssg_refill_worlds: ") + hipGetErrorString(e));
        h->zeroed = true;
    }
    rc = ring_refill(h, dev_raw, stream);
    if (rc == SSG_OK) h->ring.ready = true;
    return rc;
}

int ssg_dyn_invalidate(ssg_handle *h, const uint8_t *dev_mask, void *stream)
{
    int rc = check_ready(h, false);
    if (rc != SSG_OK) return rc;
    if (h->cfg.n_ships <= 1) return SSG_OK; // nothing to wake
    if (dev_mask) h->dyn_step.queue_lost();
    else h->dyn_step.blob_rebound(); // "the blob may have been copied or restored"
    hipError_t e = ssg::launch_dyn_invalidate(h->dev, dev_mask, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("dyn_invalidate launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_render(ssg_handle *h, int env_index, int width, int height, uint8_t *dev_rgb, uint32_t flags, void *stream)
{
    // the arguments first: a bad one is refused before anything asks for a device
    if (!h) return SSG_ERR_BAD_ARG;
    if (!dev_rgb || env_index < 0 || env_index >= h->cfg.n_envs || width < 1 || height < 1 || width > 8192 || height > 8192)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_render: bad argument");
    int rc = check_ready(h, true);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_render(h->dev, h->dyn, env_index, width, height, dev_rgb, flags, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("render launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_render_envs(ssg_handle *h, const int32_t *dev_env_ids, int count, int width, int height, uint8_t *dev_rgb, uint32_t flags, void *stream)
{
    // ssg_render's checks in its order (the ids are on the device: the kernel skips a frame whose id is out of range)
    if (!h) return SSG_ERR_BAD_ARG;
    if (!dev_rgb || !dev_env_ids || width < 1 || height < 1 || width > 8192 || height > 8192)
        return fail(h, SSG_ERR_BAD_ARG, "ssg_render_envs: bad argument");
    if (count < 1 || count > SSG_RENDER_MAX_ENVS) return fail(h, SSG_ERR_BAD_ARG, "ssg_render_envs: count must be in 1..SSG_RENDER_MAX_ENVS");
    if ((long long)count * width * height * 3 > (1ll << 31))
        return fail(h, SSG_ERR_BAD_ARG, "ssg_render_envs: count * width * height * 3 exceeds 2^31 bytes (render in blocks)");
    int rc = check_ready(h, true);
    if (rc != SSG_OK) return rc;
    hipError_t e = ssg::launch_render_envs(h->dev, h->dyn, dev_env_ids, count, width, height, dev_rgb, flags, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(h, SSG_ERR_HIP, std::string("render_envs launch: ") + hipGetErrorString(e));
    return SSG_OK;
}

int ssg_debug_kernel_times(ssg_handle *h, int enable, double *dyn_step_us, double *step_kernel_us, uint64_t *steps)
{
    if (!h) return SSG_ERR_BAD_ARG;
    if (dyn_step_us) *dyn_step_us = h->t_steps ? h->t_dyn_ms * 1e3 / (double)h->t_steps : 0.0;
    if (step_kernel_us) *step_kernel_us = h->t_steps ? h->t_step_ms * 1e3 / (double)h->t_steps : 0.0;
    if (steps) *steps = h->t_steps;
    h->time_kernels = enable != 0;
    h->t_dyn_ms = h->t_step_ms = 0.0;
    h->t_steps = 0;
    return SSG_OK;
}

int ssg_debug_dyn_counters(const ssg_handle *h, uint64_t *full_steps, uint64_t *queue_rebuilds)
{
    if (!h) return SSG_ERR_BAD_ARG;
    if (full_steps) *full_steps = h->dyn_step.launches;
    if (queue_rebuilds) *queue_rebuilds = h->dyn_step.classifies;
    return SSG_OK;
}

int ssg_debug_launch_geometry(const ssg_handle *h, int *envs_per_workgroup, int *bank_in_lds, size_t *lds_bytes)
{
    if (!h) return SSG_ERR_BAD_ARG;
    if (envs_per_workgroup) *envs_per_workgroup = h->block;
    if (bank_in_lds) *bank_in_lds = h->lds ? 1 : 0;
    if (lds_bytes) *lds_bytes = h->lds_bytes;
    return SSG_OK;
}

int ssg_debug_copy8(const double *dev_src, double *dev_dst, size_t n_doubles, void *stream)
{
    if (!dev_src || !dev_dst) return SSG_ERR_BAD_ARG;
    return ssg::launch_calib_copy8(dev_src, dev_dst, n_doubles, static_cast<hipStream_t>(stream)) == hipSuccess ? SSG_OK : SSG_ERR_HIP;
}

int ssg_debug_clock_probe(uint64_t *dev_out, int n_blocks, int iters, void *stream)
{
    if (!dev_out || n_blocks < 1 || iters < 1) return SSG_ERR_BAD_ARG;
    return ssg::launch_clock_probe(reinterpret_cast<unsigned long long *>(dev_out), n_blocks, iters, static_cast<hipStream_t>(stream)) == hipSuccess
               ? SSG_OK : SSG_ERR_HIP;
}

// ---- host geometry ----
int ssg_host_convex_hull(int count, const double *verts_xy, double *out_xy, int *out_count)
{
    if (count < 1 || !verts_xy || !out_xy || !out_count) return SSG_ERR_BAD_ARG;
    std::vector<P2> v(count);
    for (int i = 0; i < count; ++i) v[i] = P2{verts_xy[2 * i], verts_xy[2 * i + 1]};
    std::vector<P2> h = convex_hull(v);
    for (size_t i = 0; i < h.size(); ++i) { out_xy[2 * i] = h[i].x; out_xy[2 * i + 1] = h[i].y; }
    *out_count = (int)h.size();
    return SSG_OK;
}

int ssg_host_moment_for_poly(double mass, int count, const double *verts_xy, double *out)
{
    if (count < 3 || !verts_xy || !out) return SSG_ERR_BAD_ARG;
    *out = moment_for_poly(mass, count, verts_xy);
    return SSG_OK;
}

int ssg_host_build_map(const double *left_xy, int n_left, const double *right_xy, int n_right, const double *goals_xy,
                       int n_goals, double spawn_x, double spawn_y, double *rec)
{
    if (!left_xy || !right_xy || !rec || n_left < 3 || n_right < 3 || n_goals < 0 || n_goals > SSG_MAX_GOALS ||
        (n_goals > 0 && !goals_xy))
        return SSG_ERR_BAD_ARG;
    std::fill(rec, rec + SSG_MAP_STRIDE, 0.0);
    const double *src[2] = {left_xy, right_xy};
    const int cnt[2] = {n_left, n_right};
    for (int s = 0; s < 2; ++s) {
        std::vector<P2> v(cnt[s]);
        for (int i = 0; i < cnt[s]; ++i) v[i] = P2{src[s][2 * i], src[s][2 * i + 1]};
        std::vector<P2> hull = convex_hull(v); // pm.Poly hulls its vertex list, models.py:180
        if (hull.size() < 3 || hull.size() > SSG_MAX_HULL) return SSG_ERR_UNSUPPORTED;
        std::vector<Plane> pl = planes_of(hull);
        rec[SSG_MAP_OFF_COUNTS + s] = (double)hull.size();
        double l = INFINITY, r = -INFINITY, b = INFINITY, t = -INFINITY; // cpPolyShapeCacheData on a static body
        for (const P2 &p : hull) {
            l = std::min(l, p.x); r = std::max(r, p.x);
            b = std::min(b, p.y); t = std::max(t, p.y);
        }
        double *bbp = rec + SSG_MAP_OFF_AABB + 4 * s;
        bbp[0] = l; bbp[1] = b; bbp[2] = r; bbp[3] = t;
        double *pp = rec + SSG_MAP_OFF_PLANES + s * (SSG_MAX_HULL * SSG_PLANE_DOUBLES);
        for (size_t i = 0; i < pl.size(); ++i) {
            double *q = pp + SSG_PLANE_DOUBLES * i;
            q[0] = pl[i].v0x; q[1] = pl[i].v0y; q[2] = pl[i].nx; q[3] = pl[i].ny;
            q[4] = pl[i].v0n;
        }
    }
    for (int g = 0; g < n_goals; ++g) {
        rec[SSG_MAP_OFF_GOALS + 2 * g] = goals_xy[2 * g];
        rec[SSG_MAP_OFF_GOALS + 2 * g + 1] = goals_xy[2 * g + 1];
    }
    // the reset observation's nearest goal (closest_goal, game.py:333-349: strict '<', first listed wins)
    double gx = -1.0, gy = -1.0, best = 0.0;
    for (int g = 0; g < n_goals; ++g) {
        const double dx = goals_xy[2 * g] - spawn_x, dy = goals_xy[2 * g + 1] - spawn_y;
        const double d = std::sqrt(dx * dx + dy * dy);
        if (g == 0 || d < best) { best = d; gx = goals_xy[2 * g]; gy = goals_xy[2 * g + 1]; }
    }
    rec[SSG_MAP_OFF_SPAWN_GOAL] = gx;
    rec[SSG_MAP_OFF_SPAWN_GOAL + 1] = gy;
    return SSG_OK;
}

int ssg_host_segment_query(const double *rec, int side, double ax, double ay, double bx, double by, double radius,
                           int *hit, double *px, double *py, double *alpha)
{
    if (!rec || side < 0 || side > 1 || !hit) return SSG_ERR_BAD_ARG;
    SegHit r = segment_query(hull_of_record(rec, side), ax, ay, bx, by, radius);
    *hit = r.hit ? 1 : 0;
    if (px) *px = r.px;
    if (py) *py = r.py;
    if (alpha) *alpha = r.alpha;
    return SSG_OK;
}

int ssg_host_goal_x_range(const double *rec, double width, double y, double *lo, double *hi, int *hit)
{
    if (!rec || !lo || !hi || !hit) return SSG_ERR_BAD_ARG;
    // game.py:322-325: fat (radius 10) rays from the mid-line to x=0 and x=W; [0] of each hit list; tolerance 60.
    const double tolerance = 60.0;
    const double ax = width / 2, ay = y;
    SegHit l{false, 0, 0, 1}, r{false, 0, 0, 1};
    for (int s = 0; s < 2 && !l.hit; ++s) l = segment_query(hull_of_record(rec, s), ax, ay, 0.0, y, 10.0);
    for (int s = 0; s < 2 && !r.hit; ++s) r = segment_query(hull_of_record(rec, s), ax, ay, width, y, 10.0);
    *hit = (l.hit && r.hit) ? 1 : 0;
    if (*hit) {
        *lo = l.px + tolerance;
        *hi = r.px - tolerance;
    }
    return SSG_OK;
}

} // extern "C"
