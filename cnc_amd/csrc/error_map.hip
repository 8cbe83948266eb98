// error_map.hip — error-map pixel sampling, for gfx950.
//
//   k_errmap_loss_fwd      per block of 256 rays: e_i = (1/3) sum_c (rgb - pix)^2 of every ray, and the block's partial sum
//                          of w_i sum_c (rgb - pix)^2 in a fixed tree
//   k_errmap_loss_fold     ONE block: the partials -> loss
//   k_errmap_loss_bwd      per ray: g_rgb = g 2 w_i (rgb - pix) / (3 n)
//   k_errmap_keys          per ray: the cell (camera, gy, gx) its pixel lies in, as an integer sort key
//   k_errmap_update        one wave per cell: the mean of the finite e of the cell's rays in a fixed order, folded into the map
//   k_errmap_cdf           ONE block: the map -> per-cell probabilities and their inclusive CDF
//   k_errmap_sample        per ray: three randoms -> (camera, px, py) and the weight 1 / (N_pix p(pixel))
//
// These are latency-bound kernels on 10^4..10^5 rays and at most 64 * 64 * n_cams cells: what they save is launches and a
// host round trip, not bandwidth.  No launch caps its grid.
//
// Arithmetic.  Contraction is off; every expression is evaluated as written, include/cnc_hip.h spells the order out and
// tests/errmap_twin.py restates it in NumPy float32.  There are no float atomics, global or LDS, and nothing depends on
// the launch geometry or the scheduling: equal inputs give equal bits, with no mode switch.
//
// Bounds.  Camera ids and pixel coordinates are clamped for the access, as cnc_camera_rays clamps them; list entries and
// segment bounds are cut to the arrays; the binary search ends inside the CDF whatever the randoms hold (a NaN compares
// false and lands on the last cell), and the pixel drawn is clamped into the image.
#include "common.hpp"

namespace cnc {

constexpr uint32_t kErrmapChunk = 64;           // cells per chunk of the CDF's scan
constexpr uint32_t kErrmapCdfThreads = 1024;
constexpr uint32_t kErrmapMaxChunks = 8192;     // LDS: one float per chunk

// first pixel row (or column) of cell g: g * size / G in integers
__device__ __forceinline__ int32_t cell_edge(int32_t g, int32_t size, int32_t G) { return (int32_t)(((int64_t)g * size) / G); }

// the cell row (or column) that holds pixel p of `size`: the largest g with cell_edge(g) <= p
__device__ __forceinline__ int32_t cell_of(int32_t p, int32_t size, int32_t G)
{
    return (int32_t)((((int64_t)p + 1) * G - 1) / size);
}

__device__ __forceinline__ int32_t clamp_i64(int64_t v, int32_t hi)          // into [0, hi]
{
    return (int32_t)(v < 0 ? 0 : (v > hi ? hi : v));
}

// p[t] = p[t] + p[t + s] for s = 128, 64, .., 1 over the block's 256 entries -> p[0]
__device__ __forceinline__ float block_tree_256(float* p)
{
    for (uint32_t s = 128; s >= 1; s >>= 1) {
        __syncthreads();
        if (threadIdx.x < s) p[threadIdx.x] = p[threadIdx.x] + p[threadIdx.x + s];
    }
    __syncthreads();
    return p[0];
}

__global__ __launch_bounds__(256) void k_errmap_loss_fwd(const float* __restrict__ rgb, const float* __restrict__ pix,
                                                         const float* __restrict__ weight, uint32_t n, float* __restrict__ err,
                                                         float* __restrict__ part)
{
    __shared__ float p[256];
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    float term = 0.0f;
    if (r < n) {
        const float d0 = rgb[(size_t)r * 3] - pix[(size_t)r * 3];
        const float d1 = rgb[(size_t)r * 3 + 1] - pix[(size_t)r * 3 + 1];
        const float d2 = rgb[(size_t)r * 3 + 2] - pix[(size_t)r * 3 + 2];
        const float sq = (d0 * d0 + d1 * d1) + d2 * d2;
        err[r] = sq / 3.0f;
        term = weight[r] * sq;
    }
    p[threadIdx.x] = term;
    const float total = block_tree_256(p);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// ONE block.  thread t adds partials t, t + 256, .. in that order from +0; then the same tree
__global__ __launch_bounds__(256) void k_errmap_loss_fold(const float* __restrict__ part, uint32_t n_part, uint32_t n,
                                                          float* __restrict__ loss)
{
    __shared__ float p[256];
    float acc = 0.0f;
    for (uint32_t k = threadIdx.x; k < n_part; k += 256) acc = acc + part[k];
    p[threadIdx.x] = acc;
    const float total = block_tree_256(p);
    if (threadIdx.x == 0) loss[0] = total / (float)(3ull * n);
}

__global__ __launch_bounds__(256) void k_errmap_loss_bwd(const float* __restrict__ g, const float* __restrict__ rgb,
                                                         const float* __restrict__ pix, const float* __restrict__ weight,
                                                         uint32_t n, float* __restrict__ g_rgb)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const float c = ((g[0] * 2.0f) * weight[r]) / (float)(3ull * n);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) g_rgb[(size_t)r * 3 + ch] = c * (rgb[(size_t)r * 3 + ch] - pix[(size_t)r * 3 + ch]);
}

__global__ __launch_bounds__(256) void k_errmap_keys(const int64_t* __restrict__ cam_ids, const int64_t* __restrict__ px,
                                                     const int64_t* __restrict__ py, uint32_t n, int32_t n_cams, int32_t H,
                                                     int32_t W, int32_t G, int32_t* __restrict__ keys)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int32_t k = clamp_i64(cam_ids[r], n_cams - 1);
    const int32_t gx = cell_of(clamp_i64(px[r], W - 1), W, G);
    const int32_t gy = cell_of(clamp_i64(py[r], H - 1), H, G);
    keys[r] = (k * G + gy) * G + gx;
}

// one wave per cell, four waves to a block
__global__ __launch_bounds__(256) void k_errmap_update(const int64_t* __restrict__ order, const int64_t* __restrict__ offsets,
                                                       const float* __restrict__ err, int64_t n, int32_t n_cells, float decay,
                                                       float* __restrict__ map)
{
    const int32_t lane = threadIdx.x & 63;
    const int32_t cell = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= n_cells) return;
    // a segment is cut to the rays there are: no load leaves `order` or `err` whatever the tables hold
    int64_t lo = offsets[cell], hi = offsets[cell + 1];
    lo = lo < 0 ? 0 : (lo > n ? n : lo);
    hi = hi < lo ? lo : (hi > n ? n : hi);
    float   acc = 0.0f;
    int32_t cnt = 0;
    for (int64_t j = lo + lane; j < hi; j += 64) {
        const int64_t i = order[j];
        if (i < 0 || i >= n) continue;
        const float e = err[i];
        const bool  ok = isfinite(e);            // a skipped step's NaN must not reach the map: selected out, no host wait
        acc = acc + (ok ? e : 0.0f);
        cnt += ok ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        acc = acc + __shfl_down(acc, off, 64);
        cnt += __shfl_down(cnt, off, 64);
    }
    if (lane == 0 && cnt > 0) {                  // a cell without a (finite) ray keeps its bits
        const float mean = acc / (float)cnt;
        map[cell] = decay * map[cell] + (1.0f - decay) * mean;
    }
}

// ONE block of 1024.  Chunk c = cells [64 c, 64 c + 64); thread t owns chunks t, t + 1024, ..
__global__ __launch_bounds__(kErrmapCdfThreads) void k_errmap_cdf(const float* __restrict__ map, int32_t n_cams, int32_t H,
                                                                  int32_t W, int32_t G, float u, float* __restrict__ prob,
                                                                  float* __restrict__ cdf)
{
    __shared__ float   part[kErrmapMaxChunks];
    __shared__ float   total;
    __shared__ int32_t last_live;
    const uint32_t GG = (uint32_t)G * (uint32_t)G;
    const uint32_t n_cells = (uint32_t)n_cams * GG;
    const uint32_t n_chunks = div_up(n_cells, kErrmapChunk);
    const float    n_pix = (float)((int64_t)n_cams * H * W);
    auto area = [&](uint32_t cell) -> float {
        const uint32_t rem = cell % GG;
        const int32_t  gy = (int32_t)(rem / (uint32_t)G), gx = (int32_t)(rem % (uint32_t)G);
        const int32_t  h = cell_edge(gy + 1, H, G) - cell_edge(gy, H, G), w = cell_edge(gx + 1, W, G) - cell_edge(gx, W, G);
        return (float)(h * w);
    };
    auto mass = [&](uint32_t cell) -> float {
        const float m = map[cell];
        return (m > 0.0f ? m : 0.0f) * area(cell);            // a negative or NaN entry counts as 0
    };
    if (threadIdx.x == 0) last_live = -1;
    // 1. S = the sum of m a: per chunk in cell order from +0, then the chunks' sums in chunk order from +0
    for (uint32_t c = threadIdx.x; c < n_chunks; c += kErrmapCdfThreads) {
        const uint32_t end = min(n_cells, (c + 1) * kErrmapChunk);
        float acc = 0.0f;
        for (uint32_t i = c * kErrmapChunk; i < end; i++) acc = acc + mass(i);
        part[c] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < n_chunks; c++) acc = acc + part[c];
        total = acc;
    }
    __syncthreads();
    const float S = total;
    const bool  uniform = !(S > 0.0f) || !isfinite(S);
    const float keep = 1.0f - u;
    __syncthreads();                                          // (`part` is rewritten below)
    // 2. p, and per chunk its sum in cell order from +0
    int32_t live = -1;
    for (uint32_t c = threadIdx.x; c < n_chunks; c += kErrmapCdfThreads) {
        const uint32_t end = min(n_cells, (c + 1) * kErrmapChunk);
        float acc = 0.0f;
        for (uint32_t i = c * kErrmapChunk; i < end; i++) {
            const float a = area(i);
            const float p = uniform ? a / n_pix : (keep * mass(i)) / S + (u * a) / n_pix;
            prob[i] = p;
            acc = acc + p;
            if (a > 0.0f) live = (int32_t)i;
        }
        part[c] = acc;
    }
    if (live >= 0) atomicMax(&last_live, live);               // (an integer maximum: order-free)
    __syncthreads();
    // 3. the chunks' exclusive prefix, in chunk order from +0
    if (threadIdx.x == 0) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < n_chunks; c++) {
            const float s = part[c];
            part[c] = acc;
            acc = acc + s;
        }
    }
    __syncthreads();
    // 4. cdf[i] = prefix[chunk] + (the chunk's running sum through i); exactly 1 from the last cell with pixels on
    const int32_t ones_from = last_live;
    for (uint32_t c = threadIdx.x; c < n_chunks; c += kErrmapCdfThreads) {
        const uint32_t end = min(n_cells, (c + 1) * kErrmapChunk);
        const float    base = part[c];
        float acc = 0.0f;
        for (uint32_t i = c * kErrmapChunk; i < end; i++) {
            acc = acc + prob[i];                              // (this thread's own store above)
            cdf[i] = (int32_t)i >= ones_from ? 1.0f : base + acc;
        }
    }
}

__global__ __launch_bounds__(256) void k_errmap_sample(const float* __restrict__ rnd, const float* __restrict__ cdf,
                                                       const float* __restrict__ prob, uint32_t n, int32_t n_cams, int32_t H,
                                                       int32_t W, int32_t G, int64_t* __restrict__ cam_ids,
                                                       int64_t* __restrict__ px, int64_t* __restrict__ py,
                                                       float* __restrict__ weight)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t GG = (uint32_t)G * (uint32_t)G;
    const uint32_t n_cells = (uint32_t)n_cams * GG;
    const float r0 = rnd[(size_t)r * 3], r1 = rnd[(size_t)r * 3 + 1], r2 = rnd[(size_t)r * 3 + 2];
    // the first entry greater than r0; none (or a NaN): the last cell
    uint32_t lo = 0, hi = n_cells;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cdf[mid] > r0) hi = mid;
        else lo = mid + 1;
    }
    const uint32_t cell = lo < n_cells ? lo : n_cells - 1;
    const int32_t  k = (int32_t)(cell / GG);
    const uint32_t rem = cell % GG;
    const int32_t  gy = (int32_t)(rem / (uint32_t)G), gx = (int32_t)(rem % (uint32_t)G);
    const int32_t  x0 = cell_edge(gx, W, G), y0 = cell_edge(gy, H, G);
    const int32_t  cw = cell_edge(gx + 1, W, G) - x0, ch = cell_edge(gy + 1, H, G) - y0;
    auto inside = [](float rr, int32_t size) -> int32_t {     // floor(rr size) clamped into [0, size - 1]; a NaN gives 0
        const float f = rr * (float)size;
        if (!(f >= 0.0f)) return 0;
        const int32_t i = f < (float)size ? (int32_t)f : size - 1;
        return i > size - 1 ? size - 1 : (i < 0 ? 0 : i);
    };
    int32_t x = x0 + inside(r1, cw), y = y0 + inside(r2, ch);
    x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);                  // (an empty cell, which no valid CDF selects, ends here)
    y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
    cam_ids[r] = k;
    px[r] = x;
    py[r] = y;
    const float inv_npix = 1.0f / (float)((int64_t)n_cams * H * W);
    const float a = (float)(cw * ch);
    const float ppix = prob[cell] / a;
    weight[r] = ppix > 0.0f ? inv_npix / ppix : 0.0f;
}

static inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static inline bool errmap_shape_ok(int32_t n_cams, int32_t H, int32_t W, int32_t G)
{
    if (n_cams <= 0 || H <= 0 || W <= 0 || G < 1 || G > 64) return false;
    if ((int64_t)H * W > 0x7FFFFFFFll || (int64_t)n_cams * H * W > (1ll << 40)) return false;
    const uint64_t cells = (uint64_t)n_cams * G * G;
    return cells <= (uint64_t)kErrmapChunk * kErrmapMaxChunks;          // (also: cell keys fit 31 bits)
}

static inline bool rays_ok(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }

}  // namespace cnc

using namespace cnc;

extern "C" uint64_t cnc_errmap_loss_workspace(int64_t n)
{
    if (n <= 0) return sizeof(float);
    return (((uint64_t)n + 255) / 256) * sizeof(float);
}

extern "C" int cnc_errmap_loss_forward(const float* rgb, const float* pixels, const float* weight, int64_t n, void* workspace,
                                       uint64_t workspace_bytes, float* loss, float* err, void* stream)
{
    if (!rays_ok(n) || n == 0 || !rgb || !pixels || !weight || !workspace || !loss || !err) return CNC_ERR_INVALID_VALUE;
    if (!aligned_to(rgb, 4) || !aligned_to(pixels, 4) || !aligned_to(weight, 4) || !aligned_to(workspace, 4)
        || !aligned_to(loss, 4) || !aligned_to(err, 4) || workspace_bytes < cnc_errmap_loss_workspace(n))
        return CNC_ERR_INVALID_VALUE;
    const uint32_t n_part = div_up((uint32_t)n, 256u);
    float*         part = reinterpret_cast<float*>(workspace);
    hipStream_t    s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_errmap_loss_fwd, dim3(n_part), dim3(256), 0, s, rgb, pixels, weight, (uint32_t)n, err, part);
    hipLaunchKernelGGL(k_errmap_loss_fold, dim3(1), dim3(256), 0, s, (const float*)part, n_part, (uint32_t)n, loss);
    return launch_status();
}

extern "C" int cnc_errmap_loss_backward(const float* g_loss, const float* rgb, const float* pixels, const float* weight,
                                        int64_t n, float* g_rgb, void* stream)
{
    if (!rays_ok(n) || n == 0 || !g_loss || !rgb || !pixels || !weight || !g_rgb) return CNC_ERR_INVALID_VALUE;
    if (!aligned_to(g_loss, 4) || !aligned_to(rgb, 4) || !aligned_to(pixels, 4) || !aligned_to(weight, 4) || !aligned_to(g_rgb, 4))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_errmap_loss_bwd, dim3(div_up((uint32_t)n, 256u)), dim3(256), 0, (hipStream_t)stream, g_loss, rgb,
                       pixels, weight, (uint32_t)n, g_rgb);
    return launch_status();
}

extern "C" int cnc_errmap_keys(const int64_t* cam_ids, const int64_t* px, const int64_t* py, int64_t n, int32_t n_cams,
                               int32_t height, int32_t width, int32_t resolution, int32_t* keys, void* stream)
{
    if (!rays_ok(n) || !errmap_shape_ok(n_cams, height, width, resolution)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;
    if (!cam_ids || !px || !py || !keys || !aligned_to(cam_ids, 8) || !aligned_to(px, 8) || !aligned_to(py, 8)
        || !aligned_to(keys, 4))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_errmap_keys, dim3(div_up((uint32_t)n, 256u)), dim3(256), 0, (hipStream_t)stream, cam_ids, px, py,
                       (uint32_t)n, n_cams, height, width, resolution, keys);
    return launch_status();
}

extern "C" int cnc_errmap_update(const int64_t* order, const int64_t* offsets, const float* err, int64_t n, int32_t n_cams,
                                 int32_t resolution, float decay, float* map, void* stream)
{
    if (!rays_ok(n) || !errmap_shape_ok(n_cams, 1, 1, resolution)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;                   // no ray: every cell keeps its bits
    if (!order || !offsets || !err || !map || !aligned_to(order, 8) || !aligned_to(offsets, 8) || !aligned_to(err, 4)
        || !aligned_to(map, 4))
        return CNC_ERR_INVALID_VALUE;
    const int32_t n_cells = n_cams * resolution * resolution;
    hipLaunchKernelGGL(k_errmap_update, dim3(div_up((uint32_t)n_cells, 4u)), dim3(256), 0, (hipStream_t)stream, order, offsets,
                       err, n, n_cells, decay, map);
    return launch_status();
}

extern "C" int cnc_errmap_cdf(const float* map, int32_t n_cams, int32_t height, int32_t width, int32_t resolution,
                              float uniform_floor, float* prob, float* cdf, void* stream)
{
    if (!errmap_shape_ok(n_cams, height, width, resolution) || !(uniform_floor >= 0.0f && uniform_floor <= 1.0f))
        return CNC_ERR_INVALID_VALUE;
    if (!map || !prob || !cdf || !aligned_to(map, 4) || !aligned_to(prob, 4) || !aligned_to(cdf, 4)) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_errmap_cdf, dim3(1), dim3(kErrmapCdfThreads), 0, (hipStream_t)stream, map, n_cams, height, width,
                       resolution, uniform_floor, prob, cdf);
    return launch_status();
}

extern "C" int cnc_errmap_sample(const float* rand, const float* cdf, const float* prob, int64_t n, int32_t n_cams,
                                 int32_t height, int32_t width, int32_t resolution, int64_t* cam_ids, int64_t* px, int64_t* py,
                                 float* weight, void* stream)
{
    if (!rays_ok(n) || !errmap_shape_ok(n_cams, height, width, resolution)) return CNC_ERR_INVALID_VALUE;
    if (n == 0) return CNC_OK;
    if (!rand || !cdf || !prob || !cam_ids || !px || !py || !weight) return CNC_ERR_INVALID_VALUE;
    if (!aligned_to(rand, 4) || !aligned_to(cdf, 4) || !aligned_to(prob, 4) || !aligned_to(weight, 4) || !aligned_to(cam_ids, 8)
        || !aligned_to(px, 8) || !aligned_to(py, 8))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_errmap_sample, dim3(div_up((uint32_t)n, 256u)), dim3(256), 0, (hipStream_t)stream, rand, cdf, prob,
                       (uint32_t)n, n_cams, height, width, resolution, cam_ids, px, py, weight);
    return launch_status();
}
