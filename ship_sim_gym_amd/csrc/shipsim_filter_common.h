// shipsim_filter_common.h — the device helpers the two running-statistics translation units share: shipsim_filter.hip (observations)
// and shipsim_retfilter.hip (discounted returns).  Both reduce a member's rows in the order include/shipsim.h documents under
// "Observation filter": 256-row tiles with two halving trees, eight runs of consecutive tiles merged in tile order, a halving tree over
// the runs, then Chan's merge into the running state.  Device code only; include after shipsim_internal.h.
#pragma once
#include <cstdint>

#include "shipsim_internal.h"

namespace ssg {
namespace {

constexpr int kFltRuns = 8; // runs of consecutive tiles in the finalise launch

// x[0] + ... + x[255] as a halving tree (s[i] += s[i + h] for h = 128, 64, ..., 1) over one wave: lane l holds entries l, l + 64,
// l + 128 and l + 192.  The total is lane 0's; every lane returns it.
__device__ __forceinline__ double wave_tree_sum(double v0, double v1, double v2, double v3)
{
    const double a0 = v0 + v2, a1 = v1 + v3; // h = 128
    double s = a0 + a1;                      // h = 64
#pragma unroll
    for (int h = 32; h > 0; h >>= 1) s = s + __shfl_down(s, h, 64); // (lanes >= h hold values nothing below reads)
    return __shfl(s, 0, 64);
}

// member m's rows: [m*n, (m+1)*n), or its row {o_m, n_m, ...} of the slices table
__device__ __forceinline__ void member_rows(const int32_t *__restrict__ slices, int m, int n, size_t *row0, int *rows)
{
    if (slices) {
        const int32_t *row = slices + (size_t)m * SSG_POP_SLICE_ROW;
        *row0 = (size_t)row[0];
        *rows = row[1];
    } else {
        *row0 = (size_t)m * (size_t)n;
        *rows = n;
    }
}

struct Stat { double n, mean, m2; };

// a <- a merged with b, in the header's association; an empty side leaves the other as it is
__device__ __forceinline__ void merge(Stat &a, const Stat &b)
{
    if (b.n == 0.0) return;
    if (a.n == 0.0) { a = b; return; }
    const double n2 = a.n + b.n, w = b.n / n2, delta = b.mean - a.mean;
    a.mean = a.mean + delta * w;
    a.m2 = (a.m2 + b.m2) + (delta * delta) * (a.n * w);
    a.n = n2;
}

} // namespace
} // namespace ssg
