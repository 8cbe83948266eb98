// exposure.hip — per-camera exposure compensation, for gfx950.
//
//   k_exposure_gains          log-gains e [C, 3] -> gains g [C, 3] = exp(e - mean over the cameras), one small launch
//   k_exposure_forward        per ray: the pixel the loss sees, p = g (c + (1 - a) b)  or  g c + (1 - a) b
//   k_exposure_backward_rays  per chunk of 256 consecutive rays: dL/dc and dL/da of every ray, and per camera the chunk's
//                             share of the gradient of the effective log-gain, in ray order
//   k_exposure_fold_cameras   per camera the chunks' shares in chunk order -> G_eff [C, 3], then the centring's transpose
//                             G = G_eff - mean over the cameras
//
// Arithmetic.  Contraction is off; every expression is evaluated as written, and include/cnc_hip.h spells the order out
// operation by operation so that tests/exposure_twin.py can restate it in NumPy float32 and agree bit for bit.  The one
// exception is exp: it is evaluated in double and rounded to float once (as pose.hip does for its Rodrigues
// coefficients) — expf is not correctly rounded, which no twin could follow; a double exp rounded once differs between
// libraries in the last float bit at most.
//
// Order of the fold.  G_eff[k] is a function of the ray indices alone, as in pose.hip: rays are cut into chunks of
// kExposureChunk = 256 consecutive rays; within a chunk the rays of camera k are added in ray order starting from +0; the
// chunks' sums are added in chunk order starting from +0.  Both means (of e and of G_eff) are sequential sums in camera
// order.  Neither the launch geometry nor the scheduling enters, and there are no atomics: two runs give equal bits, and a
// camera without rays gets exact +0 in G_eff.
#include "common.hpp"

namespace cnc {

constexpr uint32_t kExposureChunk = 256;

// One block = 256 (camera, channel) entries.  Threads 0..2 of EVERY block walk the cameras for their channel's mean (the
// table is a few hundred entries; a second launch or a grid-wide wait would cost more than the repeated walk).
__global__ __launch_bounds__(256) void k_exposure_gains(const float* __restrict__ e, int32_t n_cams, float* __restrict__ g)
{
    __shared__ float mean[3];
    if (threadIdx.x < 3) {
        float s = 0.0f;
        for (int32_t k = 0; k < n_cams; k++) s = s + e[(size_t)k * 3 + threadIdx.x];
        mean[threadIdx.x] = s / (float)n_cams;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)n_cams * 3u) return;
    const float eff = e[i] - mean[i % 3u];
    g[i] = (float)exp((double)eff);
}

__device__ __forceinline__ int32_t clamp_camera(int64_t id, int32_t n_cams)
{
    return (int32_t)(id < 0 ? 0 : (id >= n_cams ? n_cams - 1 : id));       // as cnc_camera_rays clamps it
}

// thread = one ray.  MODE 0: no background; 1: the gain on the whole pixel; 2: on the foreground only
template <int MODE>
__global__ __launch_bounds__(256) void k_exposure_forward(const float* __restrict__ rgb, const float* __restrict__ opacity,
                                                          const float* __restrict__ bkgd, uint32_t bkgd_stride,
                                                          const int64_t* __restrict__ cam_ids, const float* __restrict__ gains,
                                                          int32_t n_cams, uint32_t n, float* __restrict__ out)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const float* g = gains + (size_t)clamp_camera(cam_ids[r], n_cams) * 3;
    const float* c = rgb + (size_t)r * 3;
    float*       o = out + (size_t)r * 3;
    if (MODE == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[ch] = g[ch] * c[ch];
    } else {
        const float  t = 1.0f - opacity[r];
        const float* b = bkgd + (size_t)r * bkgd_stride;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float tb = t * b[ch];
            o[ch] = MODE == 1 ? g[ch] * (c[ch] + tb) : g[ch] * c[ch] + tb;
        }
    }
}

// block = one chunk, thread = one ray; then thread = one camera (striding by the block's width when n_cams > 256)
template <int MODE>
__global__ __launch_bounds__(256) void k_exposure_backward_rays(const float* __restrict__ g_out, const float* __restrict__ rgb,
                                                                const float* __restrict__ opacity,
                                                                const float* __restrict__ bkgd, uint32_t bkgd_stride,
                                                                const int64_t* __restrict__ cam_ids,
                                                                const float* __restrict__ gains, int32_t n_cams, uint32_t n,
                                                                float* __restrict__ g_rgb, float* __restrict__ g_opacity,
                                                                float* __restrict__ part)
{
    __shared__ float sq[kExposureChunk * 3];
    __shared__ __attribute__((aligned(16))) int32_t sc[kExposureChunk];
    const uint32_t r0 = blockIdx.x * kExposureChunk;
    const uint32_t m = min(kExposureChunk, n - r0);
    const uint32_t r = r0 + threadIdx.x;
    if (threadIdx.x < m) {
        const int32_t k = clamp_camera(cam_ids[r], n_cams);
        const float*  g = gains + (size_t)k * 3;
        const float*  c = rgb + (size_t)r * 3;
        const float*  gp = g_out + (size_t)r * 3;
        float         gc[3], x[3], bb[3] = {0.0f, 0.0f, 0.0f};
        if (MODE != 0) {
            const float* b = bkgd + (size_t)r * bkgd_stride;
#pragma unroll
            for (int ch = 0; ch < 3; ch++) bb[ch] = b[ch];
        }
        const float t = MODE == 1 ? 1.0f - opacity[r] : 0.0f;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            gc[ch] = g[ch] * gp[ch];
            x[ch] = MODE == 1 ? c[ch] + t * bb[ch] : c[ch];
            g_rgb[(size_t)r * 3 + ch] = gc[ch];
            sq[threadIdx.x * 3 + ch] = gp[ch] * (g[ch] * x[ch]);
        }
        sc[threadIdx.x] = k;
        if (MODE != 0 && g_opacity) {
            const float* u = MODE == 1 ? gc : gp;
            g_opacity[r] = -((u[0] * bb[0] + u[1] * bb[1]) + u[2] * bb[2]);
        }
    } else {
        sc[threadIdx.x] = -1;                       // behind a short last chunk: no camera's
    }
    __syncthreads();
    for (int32_t k = threadIdx.x; k < n_cams; k += 256) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        // every lane reads the same four ids (one 16-byte broadcast read), in ray order
        for (uint32_t j = 0; j < kExposureChunk; j += 4) {
            const int4    id4 = *reinterpret_cast<const int4*>(&sc[j]);
            const int32_t id[4] = {id4.x, id4.y, id4.z, id4.w};
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (id[u] != k) continue;
#pragma unroll
                for (int ch = 0; ch < 3; ch++) acc[ch] = acc[ch] + sq[(j + u) * 3 + ch];
            }
        }
        float* o = part + ((size_t)blockIdx.x * n_cams + k) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) o[ch] = acc[ch];
    }
}

// ONE block.  thread = one (camera, channel) entry, striding; then the mean of each channel, walked by threads 0..2
__global__ __launch_bounds__(256) void k_exposure_fold_cameras(const float* __restrict__ part, uint32_t n_chunks, int32_t n_cams,
                                                               float* __restrict__ G_eff, float* __restrict__ G)
{
    __shared__ float mean[3];
    const uint32_t n_entries = (uint32_t)n_cams * 3u;
    for (uint32_t i = threadIdx.x; i < n_entries; i += 256) {
        // sixteen chunks' sums are fetched together and then added one by one: the order of the additions is the chunks',
        // the loads' latency is paid once per sixteen instead of once per chunk (one block has nothing else to hide it)
        float    acc = 0.0f;
        uint32_t k = 0;
        for (; k + 16 <= n_chunks; k += 16) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = part[(size_t)(k + j) * n_entries + i];
#pragma unroll
            for (int j = 0; j < 16; j++) acc = acc + v[j];
        }
        for (; k < n_chunks; k++) acc = acc + part[(size_t)k * n_entries + i];
        G_eff[i] = acc;
    }
    __syncthreads();           // (one block: the stores above are visible to it behind the barrier)
    if (threadIdx.x < 3) {
        float s = 0.0f;
        for (int32_t k = 0; k < n_cams; k++) s = s + G_eff[(size_t)k * 3 + threadIdx.x];
        mean[threadIdx.x] = s / (float)n_cams;
    }
    __syncthreads();
    if (!G) return;
    for (uint32_t i = threadIdx.x; i < n_entries; i += 256) G[i] = G_eff[i] - mean[i % 3u];
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// (n_cams * 3 entries are indexed with 32 bits)
static inline bool cameras_ok(int32_t n_cams) { return n_cams > 0 && (uint64_t)n_cams * 3 <= 0x7FFFFFFFull; }

static inline int exposure_mode(const float* opacity, const float* bkgd, int32_t gain_background)
{
    if (!bkgd) return 0;
    if (!opacity) return -1;
    return gain_background ? 1 : 2;
}

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_exposure_gains(const float* log_gain, int32_t n_cams, float* gains, void* stream)
{
    if (n_cams == 0) return CNC_OK;
    if (!cameras_ok(n_cams) || !log_gain || !gains || !aligned_to(log_gain, 4) || !aligned_to(gains, 4))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_exposure_gains, dim3(div_up((uint32_t)n_cams * 3u, 256u)), dim3(256), 0, (hipStream_t)stream, log_gain,
                       n_cams, gains);
    return launch_status();
}

extern "C" int cnc_exposure_forward(const float* rgb, const float* opacity, const float* bkgd, int32_t bkgd_per_ray,
                                    int32_t gain_background, const int64_t* cam_ids, const float* gains, int32_t n_cams,
                                    int64_t n, float* out, void* stream)
{
    if (n == 0 || n_cams == 0) return CNC_OK;
    const int mode = exposure_mode(opacity, bkgd, gain_background);
    if (!cameras_ok(n_cams) || n < 0 || n > 0x7FFFFFFFll || mode < 0 || !rgb || !cam_ids || !gains || !out)
        return CNC_ERR_INVALID_VALUE;
    if (!aligned_to(rgb, 4) || !aligned_to(opacity, 4) || !aligned_to(bkgd, 4) || !aligned_to(gains, 4) || !aligned_to(out, 4)
        || !aligned_to(cam_ids, 8))
        return CNC_ERR_INVALID_VALUE;
    const dim3     grid(div_up((uint32_t)n, 256u)), block(256);
    const uint32_t bs = bkgd_per_ray ? 3u : 0u;
    hipStream_t    s = (hipStream_t)stream;
    if (mode == 0)
        hipLaunchKernelGGL(k_exposure_forward<0>, grid, block, 0, s, rgb, opacity, bkgd, bs, cam_ids, gains, n_cams, (uint32_t)n, out);
    else if (mode == 1)
        hipLaunchKernelGGL(k_exposure_forward<1>, grid, block, 0, s, rgb, opacity, bkgd, bs, cam_ids, gains, n_cams, (uint32_t)n, out);
    else
        hipLaunchKernelGGL(k_exposure_forward<2>, grid, block, 0, s, rgb, opacity, bkgd, bs, cam_ids, gains, n_cams, (uint32_t)n, out);
    return launch_status();
}

extern "C" uint64_t cnc_exposure_backward_workspace(int64_t n, int32_t n_cams)
{
    if (n_cams <= 0 || n < 0) return 0;
    const uint64_t n_chunks = ((uint64_t)n + kExposureChunk - 1) / kExposureChunk;
    return (n_chunks * (uint64_t)n_cams * 3 + (uint64_t)n_cams * 3) * sizeof(float);
}

extern "C" int cnc_exposure_backward(const float* g_out, const float* rgb, const float* opacity, const float* bkgd,
                                     int32_t bkgd_per_ray, int32_t gain_background, const int64_t* cam_ids, const float* gains,
                                     int32_t n_cams, int64_t n, void* workspace, uint64_t workspace_bytes, float* g_rgb,
                                     float* g_opacity, float* g_gain, float* g_log_gain, void* stream)
{
    if (n_cams == 0) return CNC_OK;
    if (!cameras_ok(n_cams) || n < 0 || n > 0x7FFFFFFFll || !(g_gain || g_log_gain)) return CNC_ERR_INVALID_VALUE;
    if (!workspace || !aligned_to(workspace, 4) || workspace_bytes < cnc_exposure_backward_workspace(n, n_cams)
        || !aligned_to(g_gain, 4) || !aligned_to(g_log_gain, 4))
        return CNC_ERR_INVALID_VALUE;
    hipStream_t    s = (hipStream_t)stream;
    const uint32_t n_chunks = div_up((uint32_t)n, kExposureChunk);
    float*         eff = reinterpret_cast<float*>(workspace);            // G_eff when the caller does not ask for it
    float*         part = eff + (size_t)n_cams * 3;
    if (n) {
        const int mode = exposure_mode(opacity, bkgd, gain_background);
        if (mode < 0 || !g_out || !rgb || !cam_ids || !gains || !g_rgb) return CNC_ERR_INVALID_VALUE;
        if (!aligned_to(g_out, 4) || !aligned_to(rgb, 4) || !aligned_to(opacity, 4) || !aligned_to(bkgd, 4)
            || !aligned_to(gains, 4) || !aligned_to(g_rgb, 4) || !aligned_to(g_opacity, 4) || !aligned_to(cam_ids, 8))
            return CNC_ERR_INVALID_VALUE;
        const dim3     grid(n_chunks), block(256);
        const uint32_t bs = bkgd_per_ray ? 3u : 0u;
        if (mode == 0)
            hipLaunchKernelGGL(k_exposure_backward_rays<0>, grid, block, 0, s, g_out, rgb, opacity, bkgd, bs, cam_ids, gains,
                               n_cams, (uint32_t)n, g_rgb, g_opacity, part);
        else if (mode == 1)
            hipLaunchKernelGGL(k_exposure_backward_rays<1>, grid, block, 0, s, g_out, rgb, opacity, bkgd, bs, cam_ids, gains,
                               n_cams, (uint32_t)n, g_rgb, g_opacity, part);
        else
            hipLaunchKernelGGL(k_exposure_backward_rays<2>, grid, block, 0, s, g_out, rgb, opacity, bkgd, bs, cam_ids, gains,
                               n_cams, (uint32_t)n, g_rgb, g_opacity, part);
    }
    hipLaunchKernelGGL(k_exposure_fold_cameras, dim3(1), dim3(256), 0, s, (const float*)part, n_chunks, n_cams,
                       g_gain ? g_gain : eff, g_log_gain);
    return launch_status();
}
