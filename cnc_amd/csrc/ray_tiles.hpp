// ray_tiles.hpp — the per-ray tile helpers of the kernels that walk flattened samples ray by ray
// (volrend.hip, distortion.hip).
//
// Mapping: 32 lanes per ray, two rays per 64-wide wave (as scan.hip), samples in tiles of 32.  A running sum over
// a ray uses scan.hip's tile tree with the carry folded into element 0 — the SAME float association as the
// reference's exclusive_sum; per-ray totals are a lane-strided partial sum + butterfly.
#pragma once

#include "common.hpp"

namespace cnc {

__device__ __forceinline__ float tile_sum_scan(float v, uint32_t j)
{
#pragma unroll
    for (uint32_t d = 1; d <= 16; d <<= 1) {
        const float up = __shfl_up(v, d, 32);
        if (((j + 1) & (2 * d - 1)) == 0) v = up + v;
    }
#pragma unroll
    for (uint32_t d = 8; d >= 1; d >>= 1) {
        const float up = __shfl_up(v, d, 32);
        if (((j + 1) & (2 * d - 1)) == d && (j + 1) >= 3 * d) v = up + v;
    }
    return v;
}

__device__ __forceinline__ float half_wave_sum(float v)
{
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) v += __shfl_xor(v, d, 32);
    return v;
}

struct RaySpan {
    int64_t  s0;
    uint32_t n, n_max;
};

// both rays of a wave run the same number of tiles (the shuffles need converged lanes)
__device__ __forceinline__ RaySpan ray_span(const int64_t* starts, const int64_t* cnts, uint32_t ray, uint32_t n_rays)
{
    RaySpan r;
    const bool live = ray < n_rays;
    r.s0 = live ? starts[ray] : 0;
    r.n = live ? (uint32_t)cnts[ray] : 0u;
    const uint32_t other = __shfl_xor(r.n, 32);
    r.n_max = r.n > other ? r.n : other;
    return r;
}

// exclusive running sum of `v` over the ray, tile by tile: returns the sum of all earlier elements
__device__ __forceinline__ float excl_step(float v, uint32_t j, float& total)
{
    const float before = total;
    if (j == 0) v = v + total;
    v = tile_sum_scan(v, j);
    total = __shfl(v, 31, 32);
    const float up = __shfl_up(v, 1, 32);
    return j == 0 ? before : up;
}

}  // namespace cnc
