// shipsim_render.hip — `rgb_array` frames: of one env (ssg_render), of many in one launch (ssg_render_envs), and of the evaluation
// recorder's tracked envs (ssg_set_eval_recorder); one rasteriser behind all three (debugging / videos).
//
// Replaces ShipGame.render + get_screen (game.py:133-138,197-229): the screen is cleared to (0, 0, 200); in debug mode
// pymunk's debug draw paints every shape of the space in insertion order with its colour — banks (139, 69, 19)
// models.py:181, goals green game.py:88, the player white game.py:275, traffic black game.py:284-286 — then one
// radius-10 circle per lidar beam at the beam's end point (red where it hit a bank, green where it did not,
// game.py:207-225; a beam whose origin lies inside a bank or on its boundary is a hit reported at the beam's far end, as
// cpShapeSegmentQuery reports it); finally a yellow radius-10 circle at the player's position (game.py:227-229).  The
// radii are 10 world units at every frame size.  The beams are queried at the current pose (the reference draws the
// previous step's results and rounds circle centres to integer pixels).  Screen y points down (`invert_p`,
// game.py:73-75); the buffer is laid out like pygame.surfarray.array3d: [x][y][rgb]; pixel (sx, sy) shows the world point
// ((sx + 0.5) W / width, H - (sy + 0.5) H / height).  A goal is drawn while its bit of the goal mask is set, from the
// bank record (n_ships == 1) or from its body's position (config 4).
// One thread per pixel: filled convex shapes are half-plane tests against the same splitting planes the physics uses.
// Not pixel-identical to pygame's scan conversion or pymunk's outline style (neither is available to compare).
#include <hip/hip_runtime.h>

#include <cmath>

#include "shipsim_internal.h"

namespace ssg {
namespace {

__device__ __forceinline__ bool in_hull(const double *pl, int n, int stride, double x, double y)
{
    bool in = n > 0;
    for (int j = 0; j < n; ++j) {
        const double *q = pl + stride * j;
        in &= (q[2] * (x - q[0]) + q[3] * (y - q[1])) <= 0.0;
    }
    return in;
}

// world vertices / normals of a 5-vertex ship hull at pose (px, py, angle), then the point test
__device__ bool in_ship(const double *hull, const double *nrm, double px, double py, double ang, double x, double y)
{
    double sa, ca;
    sincos(ang, &sa, &ca);
    bool in = true;
    for (int i = 0; i < SSG_SHIP_VERTS; ++i) {
        const double hx = hull[2 * i], hy = hull[2 * i + 1], nx = nrm[2 * i], ny = nrm[2 * i + 1];
        const double vx = ca * hx + (-sa) * hy + px, vy = sa * hx + ca * hy + py;
        const double wx = ca * nx + (-sa) * ny, wy = sa * nx + ca * ny;
        in &= (wx * (x - vx) + wy * (y - vy)) <= 0.0;
    }
    return in;
}

// cpShapeSegmentQuery (radius 0) of the segment a->b against one hull: smallest entering alpha, 2 = miss, or -1 = the point
// query at a is not positive (a inside the hull or on its boundary): a hit at alpha 0 whose reported point stays b, the far end
__device__ double seg_hull(const double *pl, int n, double ax, double ay, double bx, double by)
{
    double best = 2.0;
    bool inside = n > 0;
    for (int j = 0; j < n; ++j) {
        const double *q = pl + SSG_PLANE_DOUBLES * j;
        const double nx = q[2], ny = q[3];
        const double an = ax * nx + ay * ny, bn = bx * nx + by * ny;
        const double d = an - q[4];
        inside &= d <= 0.0;
        if (d < 0.0) continue;
        const double t = d / fmax(an - bn, 2.2250738585072014e-308);
        if (t < 0.0 || t > 1.0) continue;
        const double hx = ax + (bx - ax) * t, hy = ay + (by - ay) * t;
        const double dt = nx * hy - ny * hx;
        const double *qp = pl + SSG_PLANE_DOUBLES * ((j - 1 + n) % n);
        const double dtmin = nx * qp[1] - ny * qp[0], dtmax = nx * q[1] - ny * q[0];
        if (dtmin <= dt && dt <= dtmax && t < best) best = t;
    }
    return inside ? -1.0 : best;
}

// what both halves of a frame read of env e
struct RenderEnv {
    double px, py, ang;
    const double *rec;
    unsigned gmask;
};

__device__ __forceinline__ RenderEnv render_env(const DevCfg &c, int e)
{
    const size_t np = (size_t)c.n_pad;
    RenderEnv v;
    v.px = c.f64cols[(size_t)COL_X * np + e];
    v.py = c.f64cols[(size_t)COL_Y * np + e];
    v.ang = c.f64cols[(size_t)COL_A * np + e];
    v.rec = c.bank + (size_t)c.i32cols[(size_t)ICOL_MAP * np + e] * SSG_MAP_STRIDE;
    v.gmask = c.mask[e];
    return v;
}

// the beam ends of one frame, in the workgroup's LDS
struct RenderBeams {
    double x[SSG_MAX_BEAMS], y[SSG_MAX_BEAMS];
    int hit[SSG_MAX_BEAMS];
};

// Per workgroup, ahead of its pixels (the caller puts a __syncthreads() between the two): lane i < n_beams queries beam i.
__device__ __forceinline__ void render_beams(const DevCfg &c, const RenderEnv &v, unsigned flags, RenderBeams &bm)
{
    const double px = v.px, py = v.py, ang = v.ang;
    const double *rec = v.rec;
    if ((flags & 1u) && threadIdx.x < (unsigned)c.n_beams) {
        // LiDAR.query on the current pose (models.py:39-76): origin = position + half the world AABB extents
        double sa, ca;
        sincos(ang, &sa, &ca);
        double l = INFINITY, r = -INFINITY, b = INFINITY, t = -INFINITY;
        for (int i = 0; i < SSG_SHIP_VERTS; ++i) {
            const double vx = ca * c.hull[2 * i] + (-sa) * c.hull[2 * i + 1] + px, vy = sa * c.hull[2 * i] + ca * c.hull[2 * i + 1] + py;
            l = fmin(l, vx); r = fmax(r, vx); b = fmin(b, vy); t = fmax(t, vy);
        }
        const double ox = px + (r - l) / 2, oy = py + (t - b) / 2;
        const int i = threadIdx.x;
        const double dx = ca * c.beam_cos[i] - sa * c.beam_sin[i], dy = sa * c.beam_cos[i] + ca * c.beam_sin[i];
        const double ex = ox + c.lidar_dist * dx, ey = oy + c.lidar_dist * dy;
        double alpha = 2.0;
        for (int s = 0; s < 2 && alpha > 1.0; ++s) // first listed shape that reports a hit wins
            alpha = seg_hull(rec + SSG_MAP_OFF_PLANES + s * SSG_MAX_HULL * SSG_PLANE_DOUBLES, (int)rec[SSG_MAP_OFF_COUNTS + s], ox, oy, ex, ey);
        const double tt = (alpha >= 0.0 && alpha <= 1.0) ? alpha : 1.0; // a miss and an origin inside a hull both report the far end
        bm.x[i] = ox + (ex - ox) * tt; bm.y[i] = oy + (ey - oy) * tt; bm.hit[i] = alpha <= 1.0;
    }
}

// Pixel (sx, sy) of env e's frame into rgb ([width][height][3]); sx < width is the caller's check.
__device__ __forceinline__ void render_pixel(const DevCfg &c, const DynCfg &d, int e, const RenderEnv &v, int width, int height, int sx, int sy,
                                             uint8_t *__restrict__ rgb, unsigned flags, const RenderBeams &bm)
{
    const size_t np = (size_t)c.n_pad;
    const double px = v.px, py = v.py, ang = v.ang;
    const double *rec = v.rec;
    const unsigned gmask = v.gmask;
    const bool debug = flags & 1u;
    // pixel centre -> world point (screen y points down)
    const double x = (sx + 0.5) * (c.width / width), y = c.height - (sy + 0.5) * (c.height / height);
    uint8_t R = 0, G = 0, B = 200; // screen.fill((0, 0, 200))
    if (debug) {
        for (int s = 0; s < 2; ++s)
            if (in_hull(rec + SSG_MAP_OFF_PLANES + s * SSG_MAX_HULL * SSG_PLANE_DOUBLES, (int)rec[SSG_MAP_OFF_COUNTS + s],
                        SSG_PLANE_DOUBLES, x, y)) { R = 139; G = 69; B = 19; }
        for (int g = 0; g < c.n_goals; ++g) {
            if (!((gmask >> g) & 1u)) continue;
            double gx, gy;
            if (c.n_ships > 1) { gx = c.dyn_f64[(size_t)(DC_GOALS + DC_GOAL_COLS * g) * np + e]; gy = c.dyn_f64[(size_t)(DC_GOALS + DC_GOAL_COLS * g + 1) * np + e]; }
            else { gx = rec[SSG_MAP_OFF_GOALS + 2 * g]; gy = rec[SSG_MAP_OFF_GOALS + 2 * g + 1]; }
            if ((x - gx) * (x - gx) + (y - gy) * (y - gy) <= c.goal_r * c.goal_r) { R = 0; G = 255; B = 0; }
        }
        if (in_ship(c.hull, c.nrm, px, py, ang, x, y)) { R = 255; G = 255; B = 255; }
        if (c.n_ships > 1)
            for (int k = 0; k < SSG_N_TRAFFIC; ++k) {
                const double *t = c.dyn_f64 + (size_t)(DC_TRAFFIC + 9 * k) * np + e;
                if (in_ship(d.thull[k], d.tnrm[k], t[0], t[np], t[2 * np], x, y)) { R = 0; G = 0; B = 0; }
            }
        for (int i = 0; i < c.n_beams; ++i) {
            const double ddx = x - bm.x[i], ddy = y - bm.y[i];
            if (ddx * ddx + ddy * ddy <= 100.0) { R = bm.hit[i] ? 255 : 0; G = bm.hit[i] ? 0 : 255; B = 0; }
        }
    }
    if ((x - px) * (x - px) + (y - py) * (y - py) <= 100.0) { R = 255; G = 255; B = 0; }
    uint8_t *o = rgb + ((size_t)sx * height + sy) * 3;
    o[0] = R; o[1] = G; o[2] = B;
}

// One frame's share of a workgroup: grid x = 128-pixel column blocks, grid y = rows; every lane takes part in the beam set-up.
__device__ __forceinline__ void render_frame(const DevCfg &c, const DynCfg &d, int e, int width, int height, uint8_t *__restrict__ rgb,
                                             unsigned flags, RenderBeams &bm)
{
    const RenderEnv v = render_env(c, e);
    render_beams(c, v, flags, bm);
    __syncthreads();
    const int sx = blockIdx.x * blockDim.x + threadIdx.x, sy = blockIdx.y;
    if (sx >= width) return;
    render_pixel(c, d, e, v, width, height, sx, sy, rgb, flags, bm);
}

constexpr int kRenderBlock = 128;

} // namespace

__global__ void render_kernel(const DevCfg c, const DynCfg d, int e, int width, int height, uint8_t *__restrict__ rgb,
                              unsigned flags)
{
    __shared__ RenderBeams bm;
    render_frame(c, d, e, width, height, rgb, flags, bm);
}

// grid z = frame: frame i shows env ids[i]; an id outside 0 .. n_envs-1 leaves its frame unwritten (uniform over the workgroup)
__global__ void render_envs_kernel(const DevCfg c, const DynCfg d, const int32_t *__restrict__ ids, int width, int height,
                                   uint8_t *__restrict__ rgb, unsigned flags)
{
    __shared__ RenderBeams bm;
    const int e = ids[blockIdx.z];
    if (e < 0 || e >= c.n_envs) return;
    render_frame(c, d, e, width, height, rgb + (size_t)blockIdx.z * width * height * 3, flags, bm);
}

// the evaluation recorder's frames (ssg_set_eval_recorder), ahead of the step: grid z = slot; an active slot whose step index t is a
// multiple of S draws its env into frame t / S of the slot (uniform over the workgroup)
__global__ void eval_record_frames_kernel(const DevCfg c, const DynCfg d, const EvalRecLaunch r, const EvalRecIds ids)
{
    __shared__ RenderBeams bm;
    const int s = blockIdx.z, e = ids.e[s];
    const int t = eval_rec_step(r, e, s);
    if (t < 0 || t % r.fevery != 0) return;
    render_frame(c, d, e, r.fw, r.fh, r.frames + ((size_t)s * r.fslots + t / r.fevery) * ((size_t)r.fw * r.fh * 3), r.fflags, bm);
}

static dim3 render_grid(int width, int height, int frames)
{
    return dim3((unsigned)((width + kRenderBlock - 1) / kRenderBlock), (unsigned)height, (unsigned)frames);
}

hipError_t launch_render(const DevCfg &c, const DynCfg &d, int e, int width, int height, uint8_t *rgb, unsigned flags,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(render_kernel, render_grid(width, height, 1), dim3(kRenderBlock), 0, stream, c, d, e, width, height, rgb, flags);
    return hipGetLastError();
}

hipError_t launch_render_envs(const DevCfg &c, const DynCfg &d, const int32_t *ids, int count, int width, int height, uint8_t *rgb,
                              unsigned flags, hipStream_t stream)
{
    hipLaunchKernelGGL(render_envs_kernel, render_grid(width, height, count), dim3(kRenderBlock), 0, stream, c, d, ids, width, height, rgb,
                       flags);
    return hipGetLastError();
}

hipError_t launch_eval_record_frames(const DevCfg &c, const DynCfg &d, const EvalRecLaunch &r, const EvalRecIds &ids, hipStream_t stream)
{
    hipLaunchKernelGGL(eval_record_frames_kernel, render_grid(r.fw, r.fh, r.R), dim3(kRenderBlock), 0, stream, c, d, r, ids);
    return hipGetLastError();
}

} // namespace ssg
