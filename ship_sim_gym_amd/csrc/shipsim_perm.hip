// shipsim_perm.hip — the minibatch permutations of the PPO update, drawn on the device (ssg_ppo_perm, ssg_pop_perm; include/shipsim.h).
//
// The reference shuffles inside its update (np.random.shuffle(inds) per epoch behind model.learn, train/stable_baselines/ppo.py:90);
// the update entry points here read a dev_perm the caller made.  This object fills one: every row is the counter-based permutation of
// shipsim_perm.h, element i a pure function of (seed, update, member, epoch, n, i), so the rows do not depend on the grid, and
// ssg_host_perm — the same header compiled for the host — gives the same bits.  Nothing of the other objects is part of this one.
//
// One launch per call: grid (index blocks, rows) x 256 threads, a row per blockIdx.y (rows beyond the grid's 65 535 are taken in further
// rounds of it).  A lane computes kPermPerLane = 2 consecutive elements and writes them as int64 with one 16-byte vector store where the
// address allows it (a wave then writes 1 KiB contiguously), else with two 8-byte stores.  No LDS, no atomics.  The row's round keys
// depend on blockIdx.y and the kernel arguments alone, so they are wave-uniform.  The cycle walk is a lane-dependent loop: a wave runs
// as long as its slowest lane, below 2 applications expected per element and kPermWalkCap at the very most (shipsim_perm.h).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "shipsim.h"
#include "shipsim_perm.h"

namespace ssg {
namespace {

constexpr int kPermPerLane = 2, kPermBlock = 256, kPermMaxGridY = 65535;

__global__ void __launch_bounds__(kPermBlock) perm_kernel(const PermLaunch a)
{
    const long long rows = (long long)a.members * a.epochs;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const int m = (int)(r / a.epochs), e = (int)(r - (long long)m * a.epochs);
        long long n = a.n, off = r * a.n;
        if (a.slices) {
            const int32_t *row = a.slices + (size_t)m * SSG_POP_SLICE_ROW;
            n = a.K * row[1];
            off = (long long)a.epochs * a.K * row[0] + (long long)e * n;
        }
        const long long i0 = ((long long)blockIdx.x * kPermBlock + threadIdx.x) * kPermPerLane;
        if (i0 >= n) continue;
        const PermKey key = perm_key(a.seed, a.update, (uint32_t)(a.member0 + m), (uint32_t)e, (uint64_t)n);
        int64_t *p = a.out + off + i0;
        const int64_t v0 = perm_at(key, (uint32_t)i0);
        if (i0 + 1 < n) {
            const int64_t v1 = perm_at(key, (uint32_t)(i0 + 1));
            if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
                *reinterpret_cast<longlong2 *>(p) = make_longlong2(v0, v1);
            } else {
                p[0] = v0;
                p[1] = v1;
            }
        } else {
            p[0] = v0;
        }
    }
}

} // namespace

int launch_perm(const PermLaunch &l, void *stream)
{
    if (!l.out || l.members < 1 || l.epochs < 1 || l.n < 1 || (uint64_t)l.n > kPermMaxN) return (int)hipErrorInvalidValue;
    if (l.slices && l.K < 1) return (int)hipErrorInvalidValue;
    const long long per_block = (long long)kPermBlock * kPermPerLane, rows = (long long)l.members * l.epochs;
    const unsigned gx = (unsigned)((l.n + per_block - 1) / per_block); // (n <= 2^32: at most 2^23 blocks)
    const unsigned gy = (unsigned)(rows < kPermMaxGridY ? rows : kPermMaxGridY);
    hipLaunchKernelGGL(perm_kernel, dim3(gx, gy), dim3(kPermBlock), 0, static_cast<hipStream_t>(stream), l);
    return (int)hipGetLastError();
}

} // namespace ssg
