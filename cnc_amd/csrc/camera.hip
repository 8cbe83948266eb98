// camera.hip — lens undistortion and pixel -> world ray, for gfx950.
//
//   k_lens_undistort<5 | 8 | 12>   distorted (u, v) -> ideal (x, y), OpenCV's rational-radial + tangential (+ thin-prism) model
//   k_lens_undistort<4>            the same for OpenCV's fisheye model (k1..k4 on theta)
//   k_camera_rays<model, frame>    pixel -> (origin, unit direction) in world space, optionally with the pixel's colour
//
// Written from the published camera models (OpenCV calib3d: "Pinhole camera model", "Fisheye camera model", and the
// fixed-point iteration of undistortPoints).  With r = x^2 + y^2:
//   q(r)  = (1 + k1 r + k2 r^2 + k3 r^3) / (1 + k4 r + k5 r^2 + k6 r^3)
//   xd    = x q + p1 (2 x y) + p2 (r + 2 x^2)            yd = y q + p2 (2 x y) + p1 (r + 2 y^2)
// Layouts 5 and 8 solve g(x, y) = (xd, yd)(x, y) - (u, v) = 0 by Newton's method from (x, y) = (u, v), with the analytic
// 2x2 Jacobian J: the step is -J^-1 g by Cramer's rule.  It stops when |det J| < eps (the point stays where it is), when
// both step components are below eps after the update, or after `iters` rounds.  Layout 12 is OpenCV's own iteration
// x <- (u - dx(x, y)) / q(r), with the thin-prism terms in dx, dy; a negative 1 / q returns the input.
// Fisheye: theta_d = min(|uv|, pi/2), Newton on theta_d = theta (1 + k1 theta^2 + .. + k4 theta^8) from theta = theta_d,
// scale = tan(theta) / theta_d.
//
// Arithmetic.  Contraction is OFF for this file as for the whole library: every expression below is evaluated
// as written, IEEE fp32, division and sqrt correctly rounded — tests/camera_twin.py restates the same operations in NumPy
// float32 and agrees bit for bit on everything but the fisheye's tan.  The fisheye's Newton update is evaluated in
// double (theta itself is a float), and tan is the double one rounded to float once: the update divides a difference
// of nearly equal numbers, where float would cost the digits the iteration is there to find.
//
// Memory.  Element-wise kernels, one point per lane.  A coefficient row shared by all points, and the camera row of the
// full-frame form, sit at an address every lane shares: the compiler reads them with scalar loads into scalar registers
// (the kernels are instantiated for that case so that the address is provably uniform).  Per-point camera rows are four to
// six 16-byte loads from a table of 96-byte rows that stays in L2.  (u, v) pairs travel as one 8-byte access; the [n, 3]
// rows are written with one 12-byte vector store per lane (global_store_dwordx3: a wave writes 768 contiguous bytes per
// instruction; gathering four pixels per lane for 16-byte stores would leave a 37 k-ray batch with 36 waves for 256 CUs).
// Every output element is written exactly once, by plain vector stores; no atomics: equal inputs give equal bits.
#include "common.hpp"

namespace cnc {

constexpr float kHalfPi = 1.57079637050628662109375f;          // float(pi / 2)

__device__ __forceinline__ void undistort_newton(float u, float v, float k1, float k2, float p1, float p2, float k3, float k4,
                                                 float k5, float k6, float eps, int iters, float& x, float& y)
{
    x = u;
    y = v;
    for (int it = 0; it < iters; it++) {
        const float r = x * x + y * y;
        const float A = 1.0f + r * (k1 + r * (k2 + r * k3));
        const float B = 1.0f + r * (k4 + r * (k5 + r * k6));
        const float q = A / B;
        const float txy = 2.0f * x * y;
        const float gx = (x * q + (p1 * txy + p2 * (r + 2.0f * x * x))) - u;
        const float gy = (y * q + (p2 * txy + p1 * (r + 2.0f * y * y))) - v;
        // dq/dr, then dq/dx = 2 x dq/dr, dq/dy = 2 y dq/dr
        const float Ar = k1 + r * (2.0f * k2 + r * (3.0f * k3));
        const float Br = k4 + r * (2.0f * k5 + r * (3.0f * k6));
        const float qr = (Ar * B - A * Br) / (B * B);
        const float qx = 2.0f * x * qr;
        const float qy = 2.0f * y * qr;
        const float j00 = (q + x * qx) + 2.0f * (p1 * y + 3.0f * p2 * x);          // d gx / d x
        const float j01 = x * qy + 2.0f * (p1 * x + p2 * y);                      // d gx / d y
        const float j10 = y * qx + 2.0f * (p2 * y + p1 * x);                      // d gy / d x
        const float j11 = (q + y * qy) + 2.0f * (p2 * x + 3.0f * p1 * y);          // d gy / d y
        const float det = j00 * j11 - j01 * j10;
        if (fabsf(det) < eps) break;
        const float sx = (j01 * gy - j11 * gx) / det;
        const float sy = (j10 * gx - j00 * gy) / det;
        x = x + sx;
        y = y + sy;
        if (fabsf(sx) < eps && fabsf(sy) < eps) break;
    }
}

// c = k1 k2 k3 k4 k5 k6 p1 p2 s1 s2 s3 s4
__device__ __forceinline__ void undistort_fixed_point(float u, float v, const float (&c)[12], int iters, float& x, float& y)
{
    x = u;
    y = v;
    for (int it = 0; it < iters; it++) {
        const float r = x * x + y * y;
        const float inv = (1.0f + ((c[5] * r + c[4]) * r + c[3]) * r) / (1.0f + ((c[2] * r + c[1]) * r + c[0]) * r);
        if (inv < 0.0f) {
            x = u;
            y = v;
            return;
        }
        const float txy = 2.0f * x * y;
        const float dx = ((c[6] * txy + c[7] * (r + 2.0f * x * x)) + c[8] * r) + c[9] * r * r;
        const float dy = ((c[6] * (r + 2.0f * y * y) + c[7] * txy) + c[10] * r) + c[11] * r * r;
        x = (u - dx) * inv;
        y = (v - dy) * inv;
    }
}

__device__ __forceinline__ void undistort_fisheye(float u, float v, float k1, float k2, float k3, float k4, float eps, int iters,
                                                  float& x, float& y)
{
    float td = sqrtf(u * u + v * v);
    td = td > kHalfPi ? kHalfPi : td;
    float theta = td, scale = 0.0f;
    bool  converged = true;
    if (td > eps) {
        converged = false;
        for (int it = 0; it < iters; it++) {
            const double t = (double)theta;
            const double t2 = t * t, t4 = t2 * t2, t6 = t4 * t2, t8 = t4 * t4;
            const double a = (double)k1 * t2, b = (double)k2 * t4, c = (double)k3 * t6, d = (double)k4 * t8;
            const double fix = (t * ((((1.0 + a) + b) + c) + d) - (double)td) /
                               ((((1.0 + 3.0 * a) + 5.0 * b) + 7.0 * c) + 9.0 * d);
            theta = (float)(t - fix);
            if (fabs(fix) < (double)eps) {
                converged = true;
                break;
            }
        }
        scale = (float)tan((double)theta) / td;
    }
    const bool keep = converged && !(theta < 0.0f);          // theta_d >= 0: a negative theta has changed sign
    x = keep ? u * scale : u;
    y = keep ? v * scale : v;
}

// LAYOUT 5: k1 k2 p1 p2 k3;  8: + k4 k5 k6;  12: k1..k6 p1 p2 s1..s4;  4: the fisheye's k1..k4.
// SHARED: one row for all points — `params` itself, a uniform address.
template <int LAYOUT, bool SHARED>
__global__ __launch_bounds__(256) void k_lens_undistort(const float2* __restrict__ uv, const float* __restrict__ params,
                                                        int64_t stride, float eps, int iters, float2* __restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* row = SHARED ? params : params + i * stride;
    float c[LAYOUT];
#pragma unroll
    for (int k = 0; k < LAYOUT; k++) c[k] = row[k];
    const float2 p = uv[i];
    float2 o;
    if constexpr (LAYOUT == 5)
        undistort_newton(p.x, p.y, c[0], c[1], c[2], c[3], c[4], 0.0f, 0.0f, 0.0f, eps, iters, o.x, o.y);
    else if constexpr (LAYOUT == 8)
        undistort_newton(p.x, p.y, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], eps, iters, o.x, o.y);
    else if constexpr (LAYOUT == 12)
        undistort_fixed_point(p.x, p.y, c, iters, o.x, o.y);
    else
        undistort_fisheye(p.x, p.y, c[0], c[1], c[2], c[3], eps, iters, o.x, o.y);
    out[i] = o;
}

struct CameraRays {
    const float*   cams;
    const int64_t *cam_ids, *px, *py;
    const uint32_t* images;          // one RGBA pixel per word
    const float*    bkgd;
    float *         origins, *viewdirs, *pixels;
    int64_t         n;
    int32_t         n_cams, cam0, width, height, iters;
    float           flip, eps;
};

__device__ __forceinline__ void store_row3(float* base, int64_t i, float x, float y, float z)
{
    typedef float vec3 __attribute__((ext_vector_type(3), aligned(4)));
    vec3 v;
    v.x = x;
    v.y = y;
    v.z = z;
    *reinterpret_cast<vec3*>(base + 3 * i) = v;
}

__device__ __forceinline__ int64_t clamp_index(int64_t v, int64_t count) { return v < 0 ? 0 : (v >= count ? count - 1 : v); }

// FRAME: all width x height pixels of camera cam0 in row-major order; the camera row is then at a uniform address.
template <int MODEL, bool FRAME>
__global__ __launch_bounds__(256) void k_camera_rays(const CameraRays a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int64_t cam, x, y;
    if constexpr (FRAME) {
        const uint32_t row = (uint32_t)i / (uint32_t)a.width;
        cam = a.cam0;
        y = row;
        x = (uint32_t)i - row * (uint32_t)a.width;
    } else {
        cam = clamp_index(a.cam_ids[i], a.n_cams);          // the loads stay inside the table whatever the list holds
        x = a.px[i];
        y = a.py[i];
    }
    const float4* row = reinterpret_cast<const float4*>(a.cams + cam * CNC_CAMERA_ROW);
    const float4  K = row[0], r0 = row[1], r1 = row[2], r2 = row[3];
    float u = (((float)x - K.z) + 0.5f) / K.x;
    float v = (((float)y - K.w) + 0.5f) / K.y;
    if constexpr (MODEL != CNC_CAMERA_PINHOLE) {
        const float4 l0 = row[4], l1 = row[5];
        const float  ud = u, vd = v;
        if constexpr (MODEL == CNC_CAMERA_OPENCV)
            undistort_newton(ud, vd, l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w, a.eps, a.iters, u, v);
        else
            undistort_fisheye(ud, vd, l0.x, l0.y, l0.z, l0.w, a.eps, a.iters, u, v);
    }
    const float c0 = u, c1 = v * a.flip, c2 = a.flip;
    const float wx = (r0.x * c0 + r0.y * c1) + r0.z * c2;
    const float wy = (r1.x * c0 + r1.y * c1) + r1.z * c2;
    const float wz = (r2.x * c0 + r2.y * c1) + r2.z * c2;
    const float len = sqrtf((wx * wx + wy * wy) + wz * wz);
    store_row3(a.origins, i, r0.w, r1.w, r2.w);
    store_row3(a.viewdirs, i, wx / len, wy / len, wz / len);
    if (a.images) {
        const int64_t  at = (cam * a.height + clamp_index(y, a.height)) * a.width + clamp_index(x, a.width);
        const uint32_t w = a.images[at];
        const float    alpha = (float)(w >> 24) / 255.0f, rest = 1.0f - alpha;
        store_row3(a.pixels, i, (float)(w & 255u) / 255.0f * alpha + a.bkgd[0] * rest,
                   (float)((w >> 8) & 255u) / 255.0f * alpha + a.bkgd[1] * rest,
                   (float)((w >> 16) & 255u) / 255.0f * alpha + a.bkgd[2] * rest);
    }
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// n <= 2^31 - 1 points, 256 per block
static inline bool count_ok(int64_t n) { return n >= 0 && n <= (int64_t)0x7fffffff; }

template <int LAYOUT>
static int launch_undistort(const float* uv, const float* params, int64_t stride, float eps, int iters, float* out, int64_t n,
                            hipStream_t s)
{
    const dim3 grid((uint32_t)((n + 255) / 256));
    if (stride == 0)
        hipLaunchKernelGGL((k_lens_undistort<LAYOUT, true>), grid, dim3(256), 0, s, (const float2*)uv, params, stride, eps,
                           iters, (float2*)out, n);
    else
        hipLaunchKernelGGL((k_lens_undistort<LAYOUT, false>), grid, dim3(256), 0, s, (const float2*)uv, params, stride, eps,
                           iters, (float2*)out, n);
    return launch_status();
}

template <int MODEL>
static int launch_rays(const CameraRays& a, hipStream_t s)
{
    const dim3 grid((uint32_t)((a.n + 255) / 256));
    if (a.cam_ids)
        hipLaunchKernelGGL((k_camera_rays<MODEL, false>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((k_camera_rays<MODEL, true>), grid, dim3(256), 0, s, a);
    return launch_status();
}

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_lens_undistort(const float* uv, const float* params, int64_t param_stride, int32_t layout, float eps,
                                  int32_t iters, float* uv_out, int64_t n, void* stream)
{
    if (n == 0) return CNC_OK;
    if (!uv || !params || !uv_out || !count_ok(n) || !aligned_to(uv, 8) || !aligned_to(uv_out, 8)) return CNC_ERR_INVALID_VALUE;
    if (layout != 5 && layout != 8 && layout != 12) return CNC_ERR_INVALID_VALUE;
    if (param_stride != 0 && param_stride < layout) return CNC_ERR_INVALID_VALUE;
    hipStream_t s = (hipStream_t)stream;
    if (layout == 5) return launch_undistort<5>(uv, params, param_stride, eps, iters, uv_out, n, s);
    if (layout == 8) return launch_undistort<8>(uv, params, param_stride, eps, iters, uv_out, n, s);
    return launch_undistort<12>(uv, params, param_stride, eps, iters, uv_out, n, s);
}

extern "C" int cnc_lens_undistort_fisheye(const float* uv, const float* params, int64_t param_stride, float eps, int32_t iters,
                                          float* uv_out, int64_t n, void* stream)
{
    if (n == 0) return CNC_OK;
    if (!uv || !params || !uv_out || !count_ok(n) || !aligned_to(uv, 8) || !aligned_to(uv_out, 8)) return CNC_ERR_INVALID_VALUE;
    if (param_stride != 0 && param_stride < 4) return CNC_ERR_INVALID_VALUE;
    return launch_undistort<4>(uv, params, param_stride, eps, iters, uv_out, n, (hipStream_t)stream);
}

extern "C" int cnc_camera_rays(const float* cams, int32_t n_cams, int32_t model, int32_t opengl, const int64_t* cam_ids,
                               const int64_t* px, const int64_t* py, int32_t cam0, int32_t width, int32_t height, int64_t n,
                               float eps, int32_t iters, const uint8_t* images, const float* bkgd, float* origins,
                               float* viewdirs, float* pixels, void* stream)
{
    if (n == 0) return CNC_OK;
    if (!cams || !origins || !viewdirs || n_cams <= 0 || !count_ok(n) || !aligned_to(cams, 16)) return CNC_ERR_INVALID_VALUE;
    if (model != CNC_CAMERA_PINHOLE && model != CNC_CAMERA_OPENCV && model != CNC_CAMERA_FISHEYE) return CNC_ERR_INVALID_VALUE;
    if (cam_ids) {
        if (!px || !py) return CNC_ERR_INVALID_VALUE;
    } else {
        if (cam0 < 0 || cam0 >= n_cams || width <= 0 || height <= 0 || (int64_t)width * height != n) return CNC_ERR_INVALID_VALUE;
    }
    if (images && (!bkgd || !pixels || width <= 0 || height <= 0 || !aligned_to(images, 4))) return CNC_ERR_INVALID_VALUE;
    CameraRays a;
    a.cams = cams;
    a.cam_ids = cam_ids;
    a.px = px;
    a.py = py;
    a.images = reinterpret_cast<const uint32_t*>(images);
    a.bkgd = bkgd;
    a.origins = origins;
    a.viewdirs = viewdirs;
    a.pixels = pixels;
    a.n = n;
    a.n_cams = n_cams;
    a.cam0 = cam0;
    a.width = width;
    a.height = height;
    a.iters = iters;
    a.flip = opengl ? -1.0f : 1.0f;
    a.eps = eps;
    hipStream_t s = (hipStream_t)stream;
    if (model == CNC_CAMERA_PINHOLE) return launch_rays<CNC_CAMERA_PINHOLE>(a, s);
    if (model == CNC_CAMERA_OPENCV) return launch_rays<CNC_CAMERA_OPENCV>(a, s);
    return launch_rays<CNC_CAMERA_FISHEYE>(a, s);
}
