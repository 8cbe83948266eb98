// envmap.hip — the learned environment-map background, for gfx950.
//
//   k_envmap_fwd          (dirs, rgb, opacity, T) -> out = rgb + (1 - opacity) env(dir), and per ray the lookup's cell and
//                         fractions for the backward; rgb == opacity == NULL: the pure lookup, out = env
//   k_envmap_bwd_rays     (g_out, opacity, cell, frac, T) -> g_opacity, s = (1 - opacity) g_out, and the four destination
//                         texels of each ray as integer sort keys
//   k_envmap_bwd_texture  per texel, the sum of its contributions w_k s in a fixed order -> g_T
//
// No launch caps its grid: one thread per ray (blocks of 256), one wave per texel (four to a block); nothing loops over
// a grid stride.
//
// Arithmetic.  Contraction is off; every expression is evaluated as written, include/cnc_hip.h spells the order out and
// tests/envmap_twin.py restates it in NumPy float32.  atan2f / acosf are the device library's and carry its error (a few
// ulp), which is why the forward is held to a tolerance and the backward — a function of the cell and fractions the
// forward stored — to the twin's bits.
//
// Order of the texture sum.  No float atomics, global or LDS.  The 4 n contributions (ray r, corner k) carry the index
// i = 4 r + k; the caller groups them by destination texel with a STABLE sort of the integer keys, so a texel's segment
// lists its contributions in ascending i.  One wave per texel: lane l adds the segment's elements l, l + 64, l + 128, ...
// in that order from +0, then the 64 partial sums are folded by the fixed tree p[l] += p[l + 32], 16, 8, 4, 2, 1.  The
// result is a function of the segment alone: equal inputs give equal bits, with no mode switch.
#include "common.hpp"

namespace cnc {

constexpr float kEnvTwoPi = 6.28318530717958647692f;
constexpr float kEnvPi = 3.14159265358979323846f;

// the four weights of a lookup, corner k = 2 (row yb ? 1 : 0) + (column xb ? 1 : 0)
__device__ __forceinline__ void env_weights(float fx, float fy, float (&w)[4])
{
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    w[0] = gx * gy;
    w[1] = fx * gy;
    w[2] = gx * fy;
    w[3] = fx * fy;
}

// cell = (y0 + 1) W + (x0 + 1) with x0 in [-1, W - 2], y0 in [-1, H - 1] -> the four texel indices (row-major, W columns).
// Whatever `cell` holds, the indices land inside the texture.
__device__ __forceinline__ void env_texels(int32_t cell, int32_t H, int32_t W, int32_t (&t)[4])
{
    int32_t y1 = cell / W, x1 = cell - y1 * W;           // y0 + 1, x0 + 1
    y1 = y1 < 0 ? 0 : (y1 > H ? H : y1);
    x1 = x1 < 0 ? 0 : (x1 > W - 1 ? W - 1 : x1);
    const int32_t ya = y1 - 1 < 0 ? 0 : y1 - 1;          // rows clamp: at a pole both rows are the same row
    const int32_t yb = y1 > H - 1 ? H - 1 : y1;
    const int32_t xa = x1 == 0 ? W - 1 : x1 - 1;         // columns wrap
    const int32_t xb = x1;                               // (x0 + 1 <= W - 1: never past the row)
    t[0] = ya * W + xa;
    t[1] = ya * W + xb;
    t[2] = yb * W + xa;
    t[3] = yb * W + xb;
}

__device__ __forceinline__ void env_colour(const float* __restrict__ T, const int32_t (&t)[4], const float (&w)[4], float (&e)[3])
{
#pragma unroll
    for (int c = 0; c < 3; c++)
        e[c] = ((w[0] * T[t[0] * 3 + c] + w[1] * T[t[1] * 3 + c]) + w[2] * T[t[2] * 3 + c]) + w[3] * T[t[3] * 3 + c];
}

__global__ __launch_bounds__(256) void k_envmap_fwd(const float* __restrict__ dirs, const float* __restrict__ rgb,
                                                    const float* __restrict__ opacity, const float* __restrict__ T, int32_t H,
                                                    int64_t n, float* __restrict__ out, int32_t* __restrict__ cell,
                                                    float* __restrict__ frac)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t W = 2 * H;
    const float dx = dirs[r * 3], dy = dirs[r * 3 + 1], dz = dirs[r * 3 + 2];
    // the finite check comes first: no index is ever formed from a NaN
    bool  live = isfinite(dx) && isfinite(dy) && isfinite(dz);
    float len = 0.0f;
    if (live) {
        len = sqrtf((dx * dx + dy * dy) + dz * dz);
        live = isfinite(len) && len > 0.0f;
    }
    float   e[3] = {0.0f, 0.0f, 0.0f};
    int32_t cl = -1;
    float   fx = 0.0f, fy = 0.0f;
    if (live) {
        float cz = dz / len;
        cz = cz < -1.0f ? -1.0f : (cz > 1.0f ? 1.0f : cz);
        const float phi = atan2f(dy, dx), theta = acosf(cz);
        const float u = (phi / kEnvTwoPi + 0.5f) * (float)W - 0.5f;
        const float v = (theta / kEnvPi) * (float)H - 0.5f;
        const float xf = floorf(u), yf = floorf(v);
        fx = u - xf;
        fy = v - yf;
        int32_t x0 = (int32_t)xf, y0 = (int32_t)yf;
        x0 = x0 < -1 ? -1 : (x0 > W - 1 ? W - 1 : x0);
        y0 = y0 < -1 ? -1 : (y0 > H - 1 ? H - 1 : y0);
        if (x0 == W - 1) x0 = -1;       // the same pair of columns (W - 1, 0) with the same fraction: one name for it
        cl = (y0 + 1) * W + (x0 + 1);
        int32_t t[4];
        float   w[4];
        env_texels(cl, H, W, t);
        env_weights(fx, fy, w);
        env_colour(T, t, w, e);
    }
    if (cell) cell[r] = cl;
    if (frac) {
        frac[r * 2] = fx;
        frac[r * 2 + 1] = fy;
    }
    if (rgb) {
        const float om = 1.0f - opacity[r];
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = rgb[r * 3 + c] + om * e[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = e[c];
    }
}

__global__ __launch_bounds__(256) void k_envmap_bwd_rays(const float* __restrict__ g_out, const float* __restrict__ opacity,
                                                         const int32_t* __restrict__ cell, const float* __restrict__ frac,
                                                         const float* __restrict__ T, int32_t H, int64_t n,
                                                         float* __restrict__ g_opacity, float* __restrict__ s,
                                                         int32_t* __restrict__ keys)
{
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t W = 2 * H;
    const int32_t cl = cell[r];
    const float   g[3] = {g_out[r * 3], g_out[r * 3 + 1], g_out[r * 3 + 2]};
    const float   om = opacity ? 1.0f - opacity[r] : 1.0f;
    float         go = 0.0f;
    int32_t       t[4] = {H * W, H * W, H * W, H * W};       // a dead ray: the bin behind the last texel, never summed
    if (cl >= 0) {
        float w[4], e[3];
        env_texels(cl, H, W, t);
        env_weights(frac[r * 2], frac[r * 2 + 1], w);
        env_colour(T, t, w, e);
        go = -((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2]);
    }
    if (g_opacity) g_opacity[r] = go;
#pragma unroll
    for (int c = 0; c < 3; c++) s[r * 3 + c] = om * g[c];
#pragma unroll
    for (int k = 0; k < 4; k++) keys[r * 4 + k] = t[k];
}

// one wave per texel, four waves to a block
__global__ __launch_bounds__(256) void k_envmap_bwd_texture(const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                            const float* __restrict__ frac, const float* __restrict__ s,
                                                            int32_t n_texels, int64_t n, float* __restrict__ g_T)
{
    const int32_t lane = threadIdx.x & 63;
    const int32_t texel = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (texel >= n_texels) return;
    // a segment is cut to the contributions there are: no load leaves `order`, `frac` or `s` whatever the tables hold
    const int64_t n4 = n * 4;
    int64_t lo = offsets[texel], hi = offsets[texel + 1];
    lo = lo < 0 ? 0 : (lo > n4 ? n4 : lo);
    hi = hi < lo ? lo : (hi > n4 ? n4 : hi);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int64_t j = lo + lane; j < hi; j += 64) {
        const int64_t i = order[j];
        if (i < 0 || i >= n4) continue;
        const int64_t r = i >> 2;
        float w[4];
        env_weights(frac[r * 2], frac[r * 2 + 1], w);
        const float wk = w[i & 3];
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + wk * s[r * 3 + c];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = acc[c] + __shfl_down(acc[c], off, 64);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) g_T[(size_t)texel * 3 + c] = acc[c];
    }
}

static inline bool env_size_ok(int32_t H, int64_t n) { return H >= 2 && H <= 64 && H % 2 == 0 && n >= 0 && n <= 0x1FFFFFFF; }

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_envmap_forward(const float* dirs, const float* rgb, const float* opacity, const float* texture, int32_t H,
                                  int64_t n, float* out, int32_t* cell, float* frac, void* stream)
{
    if (!env_size_ok(H, n) || (rgb == nullptr) != (opacity == nullptr)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;
    if (!dirs || !texture || !out) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_envmap_fwd, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dirs, rgb, opacity,
                       texture, H, n, out, cell, frac);
    return launch_status();
}

extern "C" int cnc_envmap_backward_rays(const float* g_out, const float* opacity, const int32_t* cell, const float* frac,
                                        const float* texture, int32_t H, int64_t n, float* g_opacity, float* s, int32_t* keys,
                                        void* stream)
{
    if (!env_size_ok(H, n)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;
    if (!g_out || !cell || !frac || !texture || !s || !keys) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_envmap_bwd_rays, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_out, opacity,
                       cell, frac, texture, H, n, g_opacity, s, keys);
    return launch_status();
}

extern "C" int cnc_envmap_backward_texture(const int64_t* order, const int64_t* offsets, const float* frac, const float* s,
                                           int32_t H, int64_t n, float* g_texture, void* stream)
{
    if (!env_size_ok(H, n)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;          // nothing to sum and nothing touched: the gradient of no rays is the caller's zeros
    if (!order || !offsets || !frac || !s || !g_texture) return CNC_ERR_INVALID_VALUE;
    const int32_t n_texels = H * 2 * H;
    hipLaunchKernelGGL(k_envmap_bwd_texture, dim3(div_up((uint32_t)n_texels, 4u)), dim3(256), 0, (hipStream_t)stream, order,
                       offsets, frac, s, n_texels, n, g_texture);
    return launch_status();
}
