// mlp_tree.hip — the kernels of the entropy-coded MLP section ("tree1"; C ABI in include/cnc_hip.h).  An
// extension: the reference only estimates the size of its 13-bit MLP and never writes it.
//
// Every MLP tensor's `bits`-wide indices lie back to back in ONE uint16 vector.  A tensor's row of the descriptor table
// (CNC_MLP_TREE_DESC int32 each) says where it starts, how many elements it has, how many of its top bits are modelled
// (`depth`, 0..8), where its probability table starts, where its raw low bits start, and where its first symbol stands
// in each plane's stream.  A lane finds its tensor by bisecting the starts.  Everything is integer work; the only
// floats are the +-1 symbols and the table look-up, which round nothing.  No kernel trusts the descriptor for an
// address: every table index, stream position and byte offset is compared with the buffer's length before it is used,
// and every prefix is masked to the bits it can have, so a bad row gives wrong values and never an access outside.
#include "common.hpp"

namespace cnc {
namespace {

constexpr uint32_t kDesc = CNC_MLP_TREE_DESC;
constexpr uint32_t kOff = 0, kCount = 1, kDepth = 2, kTable = 3, kLow = 4, kPlane = 8;      // members of a row
constexpr uint32_t kHistElems = 1024;      // elements per workgroup of the histogram kernel

// The last tensor whose `field` (a start) is <= i.  Tensors without elements (or without raw bits) share their start
// with the next one, and the last of the equal starts is the one that has something.
__device__ __forceinline__ uint32_t tensor_of(const int32_t* __restrict__ desc, uint32_t T, uint32_t i, uint32_t field)
{
    uint32_t lo = 0, hi = T;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t)desc[mid * kDesc + field] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t depth_of(const int32_t* row, uint32_t bits)
{
    const uint32_t d = (uint32_t)row[kDepth];
    return d > 8u ? 8u : (d > bits ? bits : d);
}

// ---------------------------------------------------------------------------------------------- histograms
// hist[t][q >> (bits - 8)]: a workgroup takes 1024 consecutive elements and walks the tensors that overlap them, one
// 256-bin LDS histogram per tensor, flushed with one integer atomic per non-empty bin.  The trip count is the block's.
__global__ void __launch_bounds__(256) mlp_tree_hist_kernel(const uint16_t* __restrict__ q, uint32_t n, const int32_t* __restrict__ desc,
                                                            uint32_t T, uint32_t bits, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[256];
    const uint32_t tid = threadIdx.x;
    const uint32_t base = blockIdx.x * kHistElems;
    const uint32_t end = base + kHistElems < n ? base + kHistElems : n;
    const uint32_t mask = (1u << bits) - 1u;
    for (uint32_t t = tensor_of(desc, T, base, kOff); t < T; t++) {
        const uint32_t off = (uint32_t)desc[t * kDesc + kOff], cnt = (uint32_t)desc[t * kDesc + kCount];
        if (off >= end) break;
        const uint32_t t0 = off > base ? off : base;
        const uint32_t t1 = (uint64_t)off + cnt < end ? off + cnt : end;
        h[tid] = 0;
        __syncthreads();
        for (uint32_t i = t0 + tid; i < t1; i += 256) atomicAdd(&h[((q[i] & mask) >> (bits - 8u)) & 255u], 1u);
        __syncthreads();
        if (h[tid] != 0) atomicAdd(&hist[(size_t)t * 256 + tid], h[tid]);      // integer: the sum has no order
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------- encode: all planes
struct PlaneBase {
    int64_t at[8];
};

__global__ void __launch_bounds__(256) mlp_tree_emit_kernel(const uint16_t* __restrict__ q, uint32_t n, const int32_t* __restrict__ desc,
                                                            uint32_t T, uint32_t bits, const float* __restrict__ tables, int64_t n_tab,
                                                            PlaneBase base, float* __restrict__ sym, float* __restrict__ p, int64_t n_out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t* row = desc + (size_t)tensor_of(desc, T, i, kOff) * kDesc;
    const uint32_t e = i - (uint32_t)row[kOff];
    if (e >= (uint32_t)row[kCount]) return;
    const uint32_t d = depth_of(row, bits);
    const uint32_t v = q[i] & ((1u << bits) - 1u);
    for (uint32_t j = 0; j < d; j++) {
        const uint32_t node = (1u << j) - 1u + (v >> (bits - j));        // the j bits above this one: below 2^j
        const uint32_t bit = (v >> (bits - 1u - j)) & 1u;
        const int64_t pos = base.at[j] + (int64_t)(uint32_t)row[kPlane + j] + e;
        const int64_t ti = (int64_t)(uint32_t)row[kTable] + node;
        if (pos < 0 || pos >= n_out || ti >= n_tab) continue;
        sym[pos] = bit ? 1.0f : -1.0f;
        p[pos] = tables[ti];
    }
}

// ---------------------------------------------------------------------------------------------- decode: one plane
__global__ void __launch_bounds__(256) mlp_tree_probs_kernel(const uint16_t* __restrict__ prefix, uint32_t n, const int32_t* __restrict__ desc,
                                                             uint32_t T, uint32_t bits, uint32_t j, const float* __restrict__ tables,
                                                             int64_t n_tab, float* __restrict__ p, int64_t n_out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t* row = desc + (size_t)tensor_of(desc, T, i, kOff) * kDesc;
    const uint32_t e = i - (uint32_t)row[kOff];
    if (e >= (uint32_t)row[kCount] || j >= depth_of(row, bits)) return;
    const uint32_t node = (1u << j) - 1u + (prefix[i] & ((1u << j) - 1u));
    const int64_t pos = (int64_t)(uint32_t)row[kPlane + j] + e;
    const int64_t ti = (int64_t)(uint32_t)row[kTable] + node;
    if (pos >= n_out || ti >= n_tab) return;
    p[pos] = tables[ti];
}

__global__ void __launch_bounds__(256) mlp_tree_fold_kernel(const float* __restrict__ sym, int64_t n_sym, uint16_t* __restrict__ prefix,
                                                            uint32_t n, const int32_t* __restrict__ desc, uint32_t T, uint32_t bits,
                                                            uint32_t j)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t* row = desc + (size_t)tensor_of(desc, T, i, kOff) * kDesc;
    const uint32_t e = i - (uint32_t)row[kOff];
    if (e >= (uint32_t)row[kCount] || j >= depth_of(row, bits)) return;
    const int64_t pos = (int64_t)(uint32_t)row[kPlane + j] + e;
    if (pos >= n_sym) return;
    const uint32_t old = prefix[i] & ((1u << j) - 1u);
    prefix[i] = (uint16_t)((old << 1) | (sym[pos] > 0.0f ? 1u : 0u));
}

// ---------------------------------------------------------------------------------------------- raw low bits
// One lane per output byte: bit k of byte B of a tensor's run is bit (8 B + k) % r of element (8 B + k) / r.
__global__ void __launch_bounds__(256) mlp_tree_pack_low_kernel(const uint16_t* __restrict__ q, uint32_t n, const int32_t* __restrict__ desc,
                                                                uint32_t T, uint32_t bits, uint8_t* __restrict__ low, uint32_t n_low)
{
    const uint32_t B = blockIdx.x * 256 + threadIdx.x;
    if (B >= n_low) return;
    const int32_t* row = desc + (size_t)tensor_of(desc, T, B, kLow) * kDesc;
    const uint32_t r = bits - depth_of(row, bits);
    const uint32_t off = (uint32_t)row[kOff], cnt = (uint32_t)row[kCount];
    uint32_t byte = 0;
    if (r != 0) {
        const uint64_t first = 8ull * (B - (uint32_t)row[kLow]);
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint64_t e = (first + k) / r;
            const uint32_t b = (uint32_t)((first + k) % r);
            if (e < cnt && off + e < n) byte |= ((q[off + e] >> b) & 1u) << k;
        }
    }
    low[B] = (uint8_t)byte;
}

// One lane per element: q = prefix << r | its r raw bits (at most three bytes of the run).
__global__ void __launch_bounds__(256) mlp_tree_unpack_kernel(const uint16_t* __restrict__ prefix, uint32_t n, const int32_t* __restrict__ desc,
                                                              uint32_t T, uint32_t bits, const uint8_t* __restrict__ low, uint32_t n_low,
                                                              uint16_t* __restrict__ q)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t* row = desc + (size_t)tensor_of(desc, T, i, kOff) * kDesc;
    const uint32_t e = i - (uint32_t)row[kOff];
    if (e >= (uint32_t)row[kCount]) {
        q[i] = 0;
        return;
    }
    const uint32_t d = depth_of(row, bits), r = bits - d;
    uint32_t v = 0;
    if (r != 0) {
        const uint64_t bp = (uint64_t)e * r;
        const uint64_t at = (uint64_t)(uint32_t)row[kLow] + (bp >> 3);
        uint32_t word = 0;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
            if (at + k < n_low) word |= (uint32_t)low[at + k] << (8 * k);
        v = (word >> (uint32_t)(bp & 7)) & ((1u << r) - 1u);
    }
    q[i] = (uint16_t)(((prefix[i] & ((1u << d) - 1u)) << r) | v);
}

inline bool tree_args_ok(const void* a, int64_t n, const int32_t* desc, int32_t T, int32_t bits)
{
    return a && desc && n >= 1 && n <= 0x7fffffff && T >= 1 && T <= 65536 && bits >= 8 && bits <= 16;
}

inline uint32_t blocks256(int64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace
}  // namespace cnc

extern "C" int cnc_mlp_tree_hist(const uint16_t* q, int64_t n, const int32_t* desc, int32_t n_tensors, int32_t bits, uint32_t* hist,
                                 void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(q, n, desc, n_tensors, bits) || !hist) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(mlp_tree_hist_kernel, dim3((uint32_t)((n + kHistElems - 1) / kHistElems)), dim3(256), 0, (hipStream_t)stream, q,
                       (uint32_t)n, desc, (uint32_t)n_tensors, (uint32_t)bits, hist);
    return launch_status();
}

extern "C" int cnc_mlp_tree_emit(const uint16_t* q, int64_t n, const int32_t* desc, int32_t n_tensors, int32_t bits, const float* tables,
                                 int64_t n_tab, const int64_t* plane_base, float* sym, float* p, int64_t n_out, void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(q, n, desc, n_tensors, bits) || n_tab < 0 || n_out < 0 || !plane_base) return CNC_ERR_INVALID_VALUE;
    if (n_out == 0) return CNC_OK;                 // every tensor at depth 0: nothing is modelled
    if (!tables || !sym || !p || n_tab < 1) return CNC_ERR_INVALID_VALUE;
    PlaneBase base;
    for (int j = 0; j < 8; j++) base.at[j] = plane_base[j];
    hipLaunchKernelGGL(mlp_tree_emit_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, q, (uint32_t)n, desc,
                       (uint32_t)n_tensors, (uint32_t)bits, tables, n_tab, base, sym, p, n_out);
    return launch_status();
}

extern "C" int cnc_mlp_tree_probs(const uint16_t* prefix, int64_t n, const int32_t* desc, int32_t n_tensors, int32_t bits, int32_t plane,
                                  const float* tables, int64_t n_tab, float* p, int64_t n_out, void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(prefix, n, desc, n_tensors, bits) || plane < 0 || plane > 7 || n_tab < 0 || n_out < 0) return CNC_ERR_INVALID_VALUE;
    if (n_out == 0) return CNC_OK;
    if (!tables || !p || n_tab < 1) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(mlp_tree_probs_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, prefix, (uint32_t)n, desc,
                       (uint32_t)n_tensors, (uint32_t)bits, (uint32_t)plane, tables, n_tab, p, n_out);
    return launch_status();
}

extern "C" int cnc_mlp_tree_fold(const float* sym, int64_t n_sym, uint16_t* prefix, int64_t n, const int32_t* desc, int32_t n_tensors,
                                 int32_t bits, int32_t plane, void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(prefix, n, desc, n_tensors, bits) || plane < 0 || plane > 7 || n_sym < 0) return CNC_ERR_INVALID_VALUE;
    if (n_sym == 0) return CNC_OK;
    if (!sym) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(mlp_tree_fold_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, sym, n_sym, prefix, (uint32_t)n, desc,
                       (uint32_t)n_tensors, (uint32_t)bits, (uint32_t)plane);
    return launch_status();
}

extern "C" int cnc_mlp_tree_pack_low(const uint16_t* q, int64_t n, const int32_t* desc, int32_t n_tensors, int32_t bits, uint8_t* low,
                                     int64_t n_low, void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(q, n, desc, n_tensors, bits) || n_low < 0 || n_low > 0x7fffffff) return CNC_ERR_INVALID_VALUE;
    if (n_low == 0) return CNC_OK;                 // bits == 8 and every tensor at depth 8
    if (!low) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(mlp_tree_pack_low_kernel, dim3(blocks256(n_low)), dim3(256), 0, (hipStream_t)stream, q, (uint32_t)n, desc,
                       (uint32_t)n_tensors, (uint32_t)bits, low, (uint32_t)n_low);
    return launch_status();
}

extern "C" int cnc_mlp_tree_unpack(const uint16_t* prefix, int64_t n, const int32_t* desc, int32_t n_tensors, int32_t bits,
                                   const uint8_t* low, int64_t n_low, uint16_t* q, void* stream)
{
    using namespace cnc;
    if (!tree_args_ok(prefix, n, desc, n_tensors, bits) || !q || n_low < 0 || n_low > 0x7fffffff || (n_low > 0 && !low))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(mlp_tree_unpack_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, prefix, (uint32_t)n, desc,
                       (uint32_t)n_tensors, (uint32_t)bits, low, (uint32_t)n_low, q);
    return launch_status();
}
