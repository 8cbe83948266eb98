// distortion.hip — the interval-distortion loss of mip-NeRF 360 per ray, fused, for gfx950.
//
//   L_ray = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i        m = interval midpoints, d = widths
//
//   k_distortion_fwd   weights, t -> L_ray per ray
//   k_distortion_bwd   dL/dL_ray per ray -> dL/dw per sample (recomputed from the inputs, nothing saved)
//
// Arithmetic.  The textbook prefix form m_i W_<i - M_<i subtracts two large sums and loses every digit on a thin
// surface far from the origin.  Here, for midpoints that do not decrease along the ray,
//   g_i = m_i - m_{i-1} = 0.5 ((t0_i - t0_{i-1}) + (t1_i - t1_{i-1}))          differences of NEIGHBOURS only
//   A_i = sum_{j<i} w_j (m_i - m_j):   A_0 = 0,  A_i = A_{i-1} + g_i Winc_{i-1}      Winc = inclusive running sum of w
//   B_i = sum_{j>i} w_j (m_j - m_i):   the same recurrence back to front, with the inclusive suffix sum of w
//   L_ray = sum_i w_i (2 A_i + w_i d_i / 3)            dL_ray/dw_i = 2 (A_i + B_i) + (2/3) w_i d_i
// — sums of non-negative terms throughout, no prefix sum is subtracted from another.  Decreasing midpoints are a
// caller error and are not checked: the signed formula is what comes out.  No gradient to t.
//
// Mapping (volrend.hip's): 32 lanes per ray, two rays per wave, samples in tiles of 32; each recurrence is two chained
// tile scans (the running weight, then g times it).  No atomics: equal inputs give equal bits.
#include "ray_tiles.hpp"

namespace cnc {

// the ray's span from (chunk_starts, chunk_cnts), or — both NULL — row `ray` of the batched layout
__device__ __forceinline__ RaySpan ray_or_row_span(const int64_t* starts, const int64_t* cnts, uint32_t row_len, uint32_t ray,
                                                   uint32_t n_rays)
{
    if (starts) return ray_span(starts, cnts, ray, n_rays);
    RaySpan r;
    const bool live = ray < n_rays;
    r.s0 = live ? (int64_t)ray * (int64_t)row_len : 0;
    r.n = live ? row_len : 0u;
    const uint32_t other = __shfl_xor(r.n, 32);
    r.n_max = r.n > other ? r.n : other;
    return r;
}

// inclusive running sum of `v` over the ray, tile by tile (excl_step's tree; the element itself included)
__device__ __forceinline__ float incl_step(float v, uint32_t j, float& total)
{
    if (j == 0) v = v + total;
    v = tile_sum_scan(v, j);
    total = __shfl(v, 31, 32);
    return v;
}

// the neighbouring lane's (t0, t1): lane j - 1 of this tile, or what lane 31 of the tile before held; then the carry moves on
__device__ __forceinline__ void lane_before(float t0, float t1, uint32_t j, float& c0, float& c1, float& p0, float& p1)
{
    p0 = __shfl_up(t0, 1, 32);
    p1 = __shfl_up(t1, 1, 32);
    if (j == 0) {
        p0 = c0;
        p1 = c1;
    }
    c0 = __shfl(t0, 31, 32);
    c1 = __shfl(t1, 31, 32);
}

__global__ __launch_bounds__(256) void k_distortion_fwd(
    const int64_t* __restrict__ starts, const int64_t* __restrict__ cnts, uint32_t row_len,
    const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ weights,
    float* __restrict__ loss, uint32_t n_rays)
{
    const uint32_t j = threadIdx.x & 31;
    const uint32_t ray = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const RaySpan  sp = ray_or_row_span(starts, cnts, row_len, ray, n_rays);
    float run_w = 0.0f, run_a = 0.0f, c0 = 0.0f, c1 = 0.0f, acc = 0.0f;
    for (uint32_t col = 0; col < sp.n_max; col += 32) {
        const uint32_t e = col + j;
        const bool     on = e < sp.n;
        const int64_t  at = sp.s0 + e;
        float w = 0, t0 = 0, t1 = 0, p0, p1;
        if (on) {
            w = weights[at];
            t0 = t_starts[at];
            t1 = t_ends[at];
        }
        lane_before(t0, t1, j, c0, c1, p0, p1);
        const float g = (on && e > 0) ? 0.5f * ((t0 - p0) + (t1 - p1)) : 0.0f;
        const float w_before = excl_step(w, j, run_w);          // Winc of the sample in front
        const float a = incl_step(g * w_before, j, run_a);
        if (on) acc += w * (2.0f * a + w * (t1 - t0) / 3.0f);
    }
    acc = half_wave_sum(acc);
    if (j == 0 && ray < n_rays) loss[ray] = acc;
}

// B of a stretch of the ray is kept while A walks the same stretch: kKeepTiles tiles (1024 samples) per ray in LDS, each
// lane reading back only what it wrote itself (no barrier).  A longer ray goes stretch by stretch, front to back, and
// walks B from the ray's end once per stretch.
constexpr uint32_t kKeepTiles = 32;

__global__ __launch_bounds__(256) void k_distortion_bwd(
    const int64_t* __restrict__ starts, const int64_t* __restrict__ cnts, uint32_t row_len,
    const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ weights,
    const float* __restrict__ g_loss, float* __restrict__ g_weights, uint32_t n_rays)
{
    __shared__ float keep[kKeepTiles][256];
    const uint32_t j = threadIdx.x & 31;
    const uint32_t ray = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const RaySpan  sp = ray_or_row_span(starts, cnts, row_len, ray, n_rays);
    const float    gl = ray < n_rays ? g_loss[ray] : 0.0f;
    // tiles are counted from the ray's END, as k_volrend_bwd's: tile b holds the samples n-1-32b .. n-32-32b
    const uint32_t n_tiles = (sp.n_max >> 5) + ((sp.n_max & 31u) ? 1u : 0u);
    float a_w = 0.0f, a_a = 0.0f, a0 = 0.0f, a1 = 0.0f;
    for (uint32_t hi = n_tiles; hi > 0;) {
        const uint32_t lo = ((hi - 1) / kKeepTiles) * kKeepTiles;          // this stretch: tiles [lo, hi)
        // B, back to front from the ray's end: lane j of tile b has the sample 32b + j from the end
        float b_w = 0.0f, b_b = 0.0f, b0 = 0.0f, b1 = 0.0f;
        for (uint32_t b = 0; b < hi; b++) {
            const uint32_t e = b * 32 + j;
            const bool     on = e < sp.n;
            const int64_t  at = sp.s0 + (int64_t)(sp.n - 1 - e);
            float w = 0, t0 = 0, t1 = 0, q0, q1;
            if (on) {
                w = weights[at];
                t0 = t_starts[at];
                t1 = t_ends[at];
            }
            lane_before(t0, t1, j, b0, b1, q0, q1);                        // (q0, q1): the sample BEHIND this one
            const float g = (on && e > 0) ? 0.5f * ((q0 - t0) + (q1 - t1)) : 0.0f;
            const float w_behind = excl_step(w, j, b_w);
            const float bb = incl_step(g * w_behind, j, b_b);
            const float mine = __shfl(bb, 31 - j, 32);                     // to the lane that has this sample in the A walk
            if (b >= lo) keep[b - lo][threadIdx.x] = mine;
        }
        // A, front to back over the same tiles with the lanes turned round: lane j has the sample 32b + 31 - j from the end
        for (uint32_t b = hi; b-- > lo;) {
            const uint32_t e = b * 32 + (31 - j);
            const bool     on = e < sp.n;
            const int64_t  at = sp.s0 + (int64_t)(sp.n - 1 - e);
            float w = 0, t0 = 0, t1 = 0, p0, p1;
            if (on) {
                w = weights[at];
                t0 = t_starts[at];
                t1 = t_ends[at];
            }
            lane_before(t0, t1, j, a0, a1, p0, p1);
            const float g = (on && e + 1 < sp.n) ? 0.5f * ((t0 - p0) + (t1 - p1)) : 0.0f;       // not the ray's first sample
            const float w_before = excl_step(w, j, a_w);
            const float a = incl_step(g * w_before, j, a_a);
            if (on) g_weights[at] = gl * (2.0f * (a + keep[b - lo][threadIdx.x]) + 2.0f * (w * (t1 - t0) / 3.0f));
        }
        hi = lo;
    }
}

static inline dim3 ray_grid(uint32_t n_rays) { return dim3(div_up(n_rays, 256 / 32)); }

// NULL starts and counts together = the batched layout; its rows must fit the kernels' 32-bit sample index
static inline bool span_args_ok(const int64_t* starts, const int64_t* cnts, int64_t row_len)
{
    if ((starts == nullptr) != (cnts == nullptr)) return false;
    return starts != nullptr || (row_len >= 0 && row_len <= (int64_t)0x7fffffff);
}

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_distortion_forward(const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t row_len,
                                      const float* t_starts, const float* t_ends, const float* weights, float* loss,
                                      uint32_t n_rays, void* stream)
{
    if (n_rays == 0) return CNC_OK;
    if (!t_starts || !t_ends || !weights || !loss || !span_args_ok(chunk_starts, chunk_cnts, row_len))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_distortion_fwd, ray_grid(n_rays), dim3(256), 0, (hipStream_t)stream, chunk_starts, chunk_cnts,
                       (uint32_t)(chunk_starts ? 0 : row_len), t_starts, t_ends, weights, loss, n_rays);
    return launch_status();
}

extern "C" int cnc_distortion_backward(const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t row_len,
                                       const float* t_starts, const float* t_ends, const float* weights,
                                       const float* grad_loss, float* grad_weights, uint32_t n_rays, void* stream)
{
    if (n_rays == 0) return CNC_OK;
    if (!t_starts || !t_ends || !weights || !grad_loss || !grad_weights ||
        !span_args_ok(chunk_starts, chunk_cnts, row_len))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_distortion_bwd, ray_grid(n_rays), dim3(256), 0, (hipStream_t)stream, chunk_starts, chunk_cnts,
                       (uint32_t)(chunk_starts ? 0 : row_len), t_starts, t_ends, weights, grad_loss, grad_weights, n_rays);
    return launch_status();
}
