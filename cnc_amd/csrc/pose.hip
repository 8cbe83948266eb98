// pose.hip — camera pose refinement, for gfx950.
//
//   k_camera_pose_apply    (base camera table, delta = (omega, tau) per camera) -> the table cnc_camera_rays reads
//   k_ray_pose_q           stage 1 of cnc_ray_pose_grad: per ray, the position gradients of its samples -> q_r (6 floats)
//   k_pose_fold_chunks     stage 2a: per (chunk of 256 consecutive rays, camera), the chunk's q_r of that camera, in ray order
//   k_pose_fold_cameras    stage 2b: per camera, the chunks' sums in chunk order -> G [C, 6]
//
// Arithmetic.  Contraction is off; every expression is evaluated as written, and include/cnc_hip.h spells the order out
// operation by operation so that tests/pose_twin.py can restate it in NumPy float32 and agree bit for bit.  The closed
// branch of the Rodrigues coefficients is evaluated in double and rounded to float once (as camera.hip does for the
// fisheye's tan): in float, (1 - cos theta) / theta^2 has lost every digit where the series branch hands over
// (theta^2 = 2^-24: cos theta rounds to 1), and sinf / cosf are not correctly rounded, which no twin could follow.
//
// Order of the fold.  A ray's q_r is a sequential sum over its samples in sample order.  G[c] is a function of the ray
// indices alone: rays are cut into chunks of kPoseChunk = 256 consecutive rays; within a chunk the rays of camera c are
// added in ray order starting from +0; the chunks' sums are added in chunk order starting from +0.  Neither the launch
// geometry nor the scheduling enters, and there are no atomics: two runs give equal bits, and a camera without rays
// gets exact +0.
#include "common.hpp"

namespace cnc {

constexpr uint32_t kPoseChunk = 256;

__global__ __launch_bounds__(64) void k_camera_pose_apply(const float* __restrict__ base, const float* __restrict__ delta,
                                                          float* __restrict__ out, int32_t n_cams)
{
    const int32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cams) return;
    const float4* src = reinterpret_cast<const float4*>(base + (size_t)c * CNC_CAMERA_ROW);
    float4*       dst = reinterpret_cast<float4*>(out + (size_t)c * CNC_CAMERA_ROW);
    const float4  K = src[0], l0 = src[4], l1 = src[5];
    float4        r[3] = {src[1], src[2], src[3]};
    const float*  dl = delta + (size_t)c * 6;
    const float   w[3] = {dl[0], dl[1], dl[2]};
    const float   t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    if (t2 != 0.0f) {
        float A, B;
        if (t2 < 5.9604644775390625e-08f) {          // 2^-24
            A = 1.0f - t2 / 6.0f;
            B = 0.5f - t2 / 24.0f;
        } else {
            const double th = sqrt((double)t2), h = 0.5 * th;
            const double sh = sin(h) / h;
            A = (float)(sin(th) / th);
            B = (float)(0.5 * (sh * sh));             // (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2, without the cancellation
        }
        // E = I + A [w]x + B (w w^T - t2 I)
        float E[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                // [w]x: (0,1) = -w2, (0,2) = w1, (1,0) = w2, (1,2) = -w0, (2,0) = -w1, (2,1) = w0
                const float k = i == j ? 0.0f : (((j - i + 3) % 3 == 1) ? -w[3 - i - j] : w[3 - i - j]);
                const float s = i == j ? w[i] * w[j] - t2 : w[i] * w[j];
                E[i][j] = ((i == j ? 1.0f : 0.0f) + A * k) + B * s;
            }
        float R0[3][3] = {{r[0].x, r[0].y, r[0].z}, {r[1].x, r[1].y, r[1].z}, {r[2].x, r[2].y, r[2].z}};
        float R1[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) R1[i][j] = (E[i][0] * R0[0][j] + E[i][1] * R0[1][j]) + E[i][2] * R0[2][j];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r[i].x = R1[i][0];
            r[i].y = R1[i][1];
            r[i].z = R1[i][2];
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const float tau = dl[3 + i];
        if (tau != 0.0f) r[i].w = r[i].w + tau;
    }
    dst[0] = K;
    dst[1] = r[0];
    dst[2] = r[1];
    dst[3] = r[2];
    dst[4] = l0;
    dst[5] = l1;
}

__global__ __launch_bounds__(256) void k_ray_pose_q(const float* __restrict__ g_x, const float* __restrict__ t_starts,
                                                    const float* __restrict__ t_ends, const int64_t* __restrict__ starts,
                                                    const int64_t* __restrict__ counts, const float* __restrict__ dirs,
                                                    int64_t n_samples, uint32_t n_rays, float* __restrict__ q)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rays) return;
    // a (start, count) pair is cut to the samples there are: no load leaves the sample arrays whatever the table holds
    int64_t s0 = starts[r], n = counts[r];
    if (s0 < 0 || n < 0 || s0 > n_samples) { s0 = 0; n = 0; }
    const int64_t s1 = n > n_samples - s0 ? n_samples : s0 + n;
    float go[3] = {0.0f, 0.0f, 0.0f}, gd[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t s = s0; s < s1; s++) {
        const float m = (t_starts[s] + t_ends[s]) * 0.5f;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float g = g_x[s * 3 + a];
            go[a] = go[a] + g;
            gd[a] = gd[a] + m * g;
        }
    }
    const float d0 = dirs[(size_t)r * 3], d1 = dirs[(size_t)r * 3 + 1], d2 = dirs[(size_t)r * 3 + 2];
    float*      o = q + (size_t)r * 6;
    o[0] = d1 * gd[2] - d2 * gd[1];
    o[1] = d2 * gd[0] - d0 * gd[2];
    o[2] = d0 * gd[1] - d1 * gd[0];
    o[3] = go[0];
    o[4] = go[1];
    o[5] = go[2];
}

// block = one chunk; thread = one camera (striding by the block's width)
__global__ __launch_bounds__(64) void k_pose_fold_chunks(const float* __restrict__ q, const int64_t* __restrict__ cam_ids,
                                                         uint32_t n_rays, int32_t n_cams, float* __restrict__ part)
{
    __shared__ float   sq[kPoseChunk * 6];
    __shared__ int32_t sc[kPoseChunk];
    const uint32_t r0 = blockIdx.x * kPoseChunk;
    const uint32_t n = min(kPoseChunk, n_rays - r0);
    for (uint32_t k = threadIdx.x; k < n; k += 64) {
        const int64_t id = cam_ids[r0 + k];
        sc[k] = (int32_t)(id < 0 ? 0 : (id >= n_cams ? n_cams - 1 : id));       // clamped, as cnc_camera_rays clamps it
    }
    for (uint32_t k = threadIdx.x; k < n * 6; k += 64) sq[k] = q[(size_t)r0 * 6 + k];
    __syncthreads();
    for (int32_t c = threadIdx.x; c < n_cams; c += 64) {
        float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < n; k++) {
            if (sc[k] != c) continue;
#pragma unroll
            for (int a = 0; a < 6; a++) acc[a] = acc[a] + sq[k * 6 + a];
        }
        float* o = part + ((size_t)blockIdx.x * n_cams + c) * 6;
#pragma unroll
        for (int a = 0; a < 6; a++) o[a] = acc[a];
    }
}

// thread = one (camera, component)
__global__ __launch_bounds__(64) void k_pose_fold_cameras(const float* __restrict__ part, uint32_t n_chunks, int32_t n_cams,
                                                          float* __restrict__ G)
{
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    if (e >= (uint32_t)n_cams * 6u) return;
    float acc = 0.0f;
    for (uint32_t k = 0; k < n_chunks; k++) acc = acc + part[(size_t)k * n_cams * 6 + e];
    G[e] = acc;
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_camera_pose_apply(const float* cams_base, const float* delta, int32_t n_cams, float* cams_out, void* stream)
{
    if (n_cams == 0) return CNC_OK;
    if (n_cams < 0 || !cams_base || !delta || !cams_out || !aligned_to(cams_base, 16) || !aligned_to(cams_out, 16))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_camera_pose_apply, dim3(div_up((uint32_t)n_cams, 64u)), dim3(64), 0, (hipStream_t)stream, cams_base,
                       delta, cams_out, n_cams);
    return launch_status();
}

extern "C" uint64_t cnc_ray_pose_grad_workspace(uint32_t n_rays, int32_t n_cams)
{
    if (n_cams <= 0) return 0;
    const uint64_t n_chunks = ((uint64_t)n_rays + kPoseChunk - 1) / kPoseChunk;
    return ((uint64_t)n_rays * 6 + n_chunks * (uint64_t)n_cams * 6) * sizeof(float);
}

extern "C" int cnc_ray_pose_grad(const float* g_x, const float* t_starts, const float* t_ends, int64_t n_samples,
                                 const int64_t* chunk_starts, const int64_t* chunk_cnts, const float* dirs,
                                 const int64_t* cam_ids, uint32_t n_rays, int32_t n_cams, void* workspace,
                                 uint64_t workspace_bytes, float* G, void* stream)
{
    if (n_cams == 0) return CNC_OK;
    if (n_cams < 0 || !G || n_samples < 0 || n_rays > 0x7FFFFFFFu) return CNC_ERR_INVALID_VALUE;
    if ((uint64_t)n_cams * 6 > 0x7FFFFFFFull) return CNC_ERR_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n_chunks = div_up(n_rays, kPoseChunk);
    float* q = nullptr;
    float* part = nullptr;
    if (n_rays) {
        if (!chunk_starts || !chunk_cnts || !dirs || !cam_ids || !workspace || !aligned_to(workspace, 4)
            || workspace_bytes < cnc_ray_pose_grad_workspace(n_rays, n_cams))
            return CNC_ERR_INVALID_VALUE;
        if (n_samples && (!g_x || !t_starts || !t_ends)) return CNC_ERR_INVALID_VALUE;
        q = reinterpret_cast<float*>(workspace);
        part = q + (size_t)n_rays * 6;
        hipLaunchKernelGGL(k_ray_pose_q, dim3(div_up(n_rays, 256u)), dim3(256), 0, s, g_x, t_starts, t_ends, chunk_starts,
                           chunk_cnts, dirs, n_samples, n_rays, q);
        hipLaunchKernelGGL(k_pose_fold_chunks, dim3(n_chunks), dim3(64), 0, s, (const float*)q, cam_ids, n_rays, n_cams, part);
    }
    hipLaunchKernelGGL(k_pose_fold_cameras, dim3(div_up((uint32_t)n_cams * 6u, 64u)), dim3(64), 0, s, (const float*)part,
                       n_chunks, n_cams, G);
    return launch_status();
}
