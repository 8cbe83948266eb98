// depth_loss.hip — depth supervision per ray, fused, and the depth fetch of a training batch, for gfx950.
//
//   e_i = 0.5 ((t0_i - D) + (t1_i - D))       the midpoint's signed distance from the ray's target distance D
//   S1 = sum_i w_i e_i        S2 = sum_i w_i e_i^2
//   L_ray = S1^2 + spread S2                  dL_ray/dw_i = 2 S1 e_i + spread e_i^2
//
//   k_depth_loss_fwd   weights, t, target -> L_ray and S1 per ray
//   k_depth_loss_bwd   dL/dL_ray and S1 per ray -> dL/dw per sample, one pass, nothing else saved
//   k_depth_fetch      (camera, pixel, ray direction) -> the measured distance ALONG THE RAY, 0 = no measurement
//
// Arithmetic.  e_i is formed per sample, as written: the differences t - D are exact wherever D / 2 <= t <= 2 D
// (Sterbenz), which is every sample near the surface the target describes.  The prefix form sum w m - D sum w subtracts
// two sums of the size of D and loses every digit on a thin surface far from the origin.  Order of the sums: the 32
// products of a tile through half_wave_sum's butterfly, the tiles' sums added to the ray's running sum one after the
// other from +0 (DESIGN §4.19 derives the bound from this).  No gradient to t or D.
//
// Validity.  A target that is not finite or is <= 0 is "no measurement": the ray's loss and S1 are exactly +0, every one
// of its samples' gradients is written as exactly +0 — none of its samples is loaded, grad_loss of such a ray is not
// multiplied in (a NaN there stays there).  Every sample a ray owns gets its gradient written, whatever it is: callers
// pass uninitialised memory.  Slots that belong to no ray are neither read nor written.
//
// Mapping (ray_tiles.hpp): 32 lanes per ray, two rays per wave, samples in tiles of 32.  No LDS, no atomics: equal
// inputs give equal bits.
#include "ray_tiles.hpp"

namespace cnc {
namespace {

// the ray's span from (chunk_starts, chunk_cnts), or — both NULL — row `ray` of the batched layout (distortion.hip's)
__device__ __forceinline__ RaySpan depth_ray_span(const int64_t* starts, const int64_t* cnts, uint32_t row_len, uint32_t ray,
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

__device__ __forceinline__ bool is_measurement(float D) { return isfinite(D) && D > 0.0f; }

__global__ __launch_bounds__(256) void k_depth_loss_fwd(
    const int64_t* __restrict__ starts, const int64_t* __restrict__ cnts, uint32_t row_len,
    const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ weights,
    const float* __restrict__ target, float spread, float* __restrict__ loss, float* __restrict__ s1_out, uint32_t n_rays)
{
    const uint32_t j = threadIdx.x & 31;
    const uint32_t ray = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const RaySpan  sp = depth_ray_span(starts, cnts, row_len, ray, n_rays);
    const float    D = ray < n_rays ? target[ray] : 0.0f;
    const bool     valid = is_measurement(D);
    float s1 = 0.0f, s2 = 0.0f;
    // both rays of the wave run n_max tiles: the butterflies need converged lanes
    for (uint32_t col = 0; col < sp.n_max; col += 32) {
        const uint32_t k = col + j;
        float a = 0.0f, b = 0.0f;
        if (valid && k < sp.n) {
            const int64_t at = sp.s0 + k;
            const float   e = 0.5f * ((t_starts[at] - D) + (t_ends[at] - D));
            a = weights[at] * e;
            b = a * e;
        }
        s1 = s1 + half_wave_sum(a);
        s2 = s2 + half_wave_sum(b);
    }
    if (j == 0 && ray < n_rays) {
        loss[ray] = valid ? s1 * s1 + spread * s2 : 0.0f;
        s1_out[ray] = valid ? s1 : 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_depth_loss_bwd(
    const int64_t* __restrict__ starts, const int64_t* __restrict__ cnts, uint32_t row_len,
    const float* __restrict__ t_starts, const float* __restrict__ t_ends, const float* __restrict__ target, float spread,
    const float* __restrict__ s1_in, const float* __restrict__ g_loss, float* __restrict__ g_weights, uint32_t n_rays)
{
    const uint32_t j = threadIdx.x & 31;
    const uint32_t ray = (blockIdx.x * blockDim.x + threadIdx.x) >> 5;
    const RaySpan  sp = depth_ray_span(starts, cnts, row_len, ray, n_rays);
    if (ray >= n_rays) return;          // (no shuffle below)
    const float D = target[ray];
    if (!is_measurement(D)) {
        for (uint32_t k = j; k < sp.n; k += 32) g_weights[sp.s0 + k] = 0.0f;
        return;
    }
    const float gl = g_loss[ray], two_s1 = 2.0f * s1_in[ray];
    for (uint32_t k = j; k < sp.n; k += 32) {
        const int64_t at = sp.s0 + k;
        const float   e = 0.5f * ((t_starts[at] - D) + (t_ends[at] - D));
        g_weights[at] = gl * (two_s1 * e + spread * (e * e));
    }
}

struct DepthFetch {
    const float *  planes, *cams, *dirs;
    const int64_t *cam_ids, *px, *py;
    float*         out;
    int64_t        n;
    int32_t        n_cams, height, width, euclidean;
    float          sign;
};

__device__ __forceinline__ int64_t into_range(int64_t v, int64_t count) { return v < 0 ? 0 : (v >= count ? count - 1 : v); }

// One ray per lane.  z-depth -> distance along the ray: the ray's unit direction d has the component c = +-(d . R[:, 2])
// along the optical axis (- for a camera that looks down -z), so a point at depth z along the axis lies at t = z / c.
__global__ __launch_bounds__(256) void k_depth_fetch(const DepthFetch a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    // every index is clamped for the loads, as cnc_camera_rays clamps them: nothing leaves the planes or the table
    const int64_t cam = into_range(a.cam_ids[i], a.n_cams);
    const int64_t x = into_range(a.px[i], a.width), y = into_range(a.py[i], a.height);
    const float   z = a.planes[(cam * a.height + y) * a.width + x];
    float t = z, c = 1.0f;
    if (!a.euclidean) {
        const float* row = a.cams + cam * CNC_CAMERA_ROW;
        const float  d0 = a.dirs[3 * i], d1 = a.dirs[3 * i + 1], d2 = a.dirs[3 * i + 2];
        c = a.sign * ((d0 * row[6] + d1 * row[10]) + d2 * row[14]);
        t = z / c;
    }
    a.out[i] = (isfinite(z) && z > 0.0f && c > 0.0f) ? t : 0.0f;
}

inline dim3 rays_grid(uint32_t n_rays) { return dim3(div_up(n_rays, 256 / 32)); }

// NULL starts and counts together = the batched layout; its rows must fit the kernels' 32-bit sample index
inline bool layout_args_ok(const int64_t* starts, const int64_t* cnts, int64_t row_len)
{
    if ((starts == nullptr) != (cnts == nullptr)) return false;
    return starts != nullptr || (row_len >= 0 && row_len <= (int64_t)0x7fffffff);
}

}  // namespace
}  // namespace cnc

using namespace cnc;

extern "C" int cnc_depth_loss_forward(const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t row_len,
                                      const float* t_starts, const float* t_ends, const float* weights, const float* target,
                                      float spread, float* loss, float* s1, uint32_t n_rays, void* stream)
{
    if (n_rays == 0) return CNC_OK;
    if (!t_starts || !t_ends || !weights || !target || !loss || !s1 || !layout_args_ok(chunk_starts, chunk_cnts, row_len))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_depth_loss_fwd, rays_grid(n_rays), dim3(256), 0, (hipStream_t)stream, chunk_starts, chunk_cnts,
                       (uint32_t)(chunk_starts ? 0 : row_len), t_starts, t_ends, weights, target, spread, loss, s1, n_rays);
    return launch_status();
}

extern "C" int cnc_depth_loss_backward(const int64_t* chunk_starts, const int64_t* chunk_cnts, int64_t row_len,
                                       const float* t_starts, const float* t_ends, const float* target, float spread,
                                       const float* s1, const float* grad_loss, float* grad_weights, uint32_t n_rays,
                                       void* stream)
{
    if (n_rays == 0) return CNC_OK;
    if (!t_starts || !t_ends || !target || !s1 || !grad_loss || !grad_weights ||
        !layout_args_ok(chunk_starts, chunk_cnts, row_len))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_depth_loss_bwd, rays_grid(n_rays), dim3(256), 0, (hipStream_t)stream, chunk_starts, chunk_cnts,
                       (uint32_t)(chunk_starts ? 0 : row_len), t_starts, t_ends, target, spread, s1, grad_loss, grad_weights,
                       n_rays);
    return launch_status();
}

extern "C" int cnc_depth_fetch(const float* planes, const float* cams, int32_t n_cams, int32_t height, int32_t width,
                               int32_t opengl, int32_t euclidean, const int64_t* cam_ids, const int64_t* px, const int64_t* py,
                               const float* viewdirs, int64_t n, float* depth, void* stream)
{
    if (n == 0) return CNC_OK;
    if (!planes || !cam_ids || !px || !py || !depth || n < 0 || n > (int64_t)0x7fffffff || n_cams <= 0 || height <= 0 ||
        width <= 0)
        return CNC_ERR_INVALID_VALUE;
    if (!euclidean && (!cams || !viewdirs)) return CNC_ERR_INVALID_VALUE;
    DepthFetch a;
    a.planes = planes;
    a.cams = cams;
    a.dirs = viewdirs;
    a.cam_ids = cam_ids;
    a.px = px;
    a.py = py;
    a.out = depth;
    a.n = n;
    a.n_cams = n_cams;
    a.height = height;
    a.width = width;
    a.euclidean = euclidean ? 1 : 0;
    a.sign = opengl ? -1.0f : 1.0f;
    hipLaunchKernelGGL(k_depth_fetch, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}
