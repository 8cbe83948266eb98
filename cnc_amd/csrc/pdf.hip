// pdf.hip — importance sampling (inverse-CDF resampling of ray segments) and searchsorted over ray segments, for
// gfx950.  Stands in for the two operations nerfacc binds from pdf.cu (nerfacc.cpp:73-86) behind include/cnc_hip.h;
// the semantics, the defined edge cases and the departures from the reference are documented there
// (cnc_importance_sampling, cnc_searchsorted) and in DESIGN.md "Proposal sampling".
//
// Shape.  One wave64 per ray (importance sampling) or per query row (searchsorted, batched queries).  The wave stages
// its ray's cdf and vals (or key row) in a per-wave LDS slice of kPdfCap edges and runs every lane's binary search
// there; lane l takes outputs l, l + 64, ...  The interval edges need each sample's neighbours, which the wave
// already holds: __shfl_up for the previous sample, a per-chunk carry from lane 63, and lane 1's sample for edge 0 —
// so samples and intervals come out of one launch (the reference launches twice and re-reads the samples).  A row
// longer than kPdfCap is searched in global memory by the same code (the "global route").  Searchsorted with a
// flattened query has no row per wave: one lane per query entry finds its ray from ray_indices, or else from a
// search of the query's chunk_starts, and searches the key in global memory, as the reference does.
//
// Arithmetic: -ffp-contract=off; the two contractions nvcc makes in the reference (u and t) are written as fmaf, so
// the result is bit-equal to the NumPy twin in tests/pdf_twin.py.
#include "common.hpp"

namespace cnc {
namespace {

constexpr int kPdfWaves = 4;      // waves per workgroup
constexpr int kPdfCap = 512;      // edges of one ray staged in LDS (4 KiB per wave for cdf + vals)

__device__ __forceinline__ void segment_of(const cnc_pdf_rows_t& r, int64_t row, int64_t& base, int64_t& cnt)
{
    if (r.n_edges_per_ray >= 0) {
        base = row * r.n_edges_per_ray;
        cnt = r.n_edges_per_ray;
    } else {
        base = r.seg.chunk_starts[row];
        cnt = r.seg.chunk_cnts[row];
    }
}

// First index in [lo, hi) whose value is > u; `!(v > u)` sends NaN (in u or in the row) to the right.
template <typename I, typename P>
__device__ __forceinline__ I upper_bound(P data, I lo, I hi, float u)
{
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (!(data[mid] > u)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename I>
__device__ __forceinline__ I clamp_to(I v, I lo, I hi)
{
    return v < lo ? lo : (v > hi ? hi : v);     // max(min(v, hi), lo) for lo <= hi
}

// The sample at u of one ray whose cdf / vals start at index 0 of `cdf` / `val`; last = edges - 1 (exclusive bound
// of the search, as the reference calls upper_bound).
template <typename I, typename P>
__device__ __forceinline__ float sample_at(P cdf, P val, I last, float u)
{
    const I p = upper_bound<I>(cdf, (I)0, last, u);
    const I p0 = clamp_to<I>(p - 1, 0, last), p1 = clamp_to<I>(p, 0, last);
    const float c0 = cdf[p0], c1 = cdf[p1], v0 = val[p0], v1 = val[p1];
    if (c1 - c0 < 1e-10f) return (v0 + v1) * 0.5f;
    return fmaf(u - c0, (v1 - v0) / (c1 - c0), v0);
}

// Writes the n samples and n + 1 interval edges of one ray.  Every lane of the wave calls it (the shuffles need the
// whole wave); lane l handles samples l, l + 64, ...
template <typename I, typename P>
__device__ __forceinline__ void sample_ray(P cdf, P val, I last, int64_t n, float bias, int lane, int64_t ray,
                                           float* __restrict__ s_vals, int64_t* __restrict__ s_ri,
                                           float* __restrict__ e_vals, int64_t* __restrict__ e_ri,
                                           uint8_t* __restrict__ e_left, uint8_t* __restrict__ e_right)
{
    const float u_floor = cdf[0], u_ceil = cdf[last];
    const float u_step = (u_ceil - u_floor) / (float)n;
    const float t_min = val[0], t_max = val[last];
    float carry = 0.0f;                          // sample 64 c - 1, for lane 0 of chunk c
    for (int64_t c = 0; c < n; c += kWave) {
        const int64_t sid = c + lane;
        float t = 0.0f;
        if (sid < n) t = sample_at<I>(cdf, val, last, fmaf((float)sid + bias, u_step, u_floor));
        float prev = __shfl_up(t, 1);
        if (lane == 0) prev = carry;
        carry = __shfl(t, kWave - 1);
        const float next0 = __shfl(t, 1);        // sample 1: edge 0 of chunk 0
        if (sid < n) {
            s_vals[sid] = t;
            if (s_ri) s_ri[sid] = ray;
            float e;
            if (sid == 0) e = n == 1 ? t_min : fmaxf(t - (next0 - t) * 0.5f, t_min);
            else e = (t + prev) * 0.5f;
            e_vals[sid] = e;
            if (e_ri) {
                e_ri[sid] = ray;
                e_left[sid] = 1;
                e_right[sid] = sid != 0;
            }
            if (sid == n - 1) {
                e_vals[n] = n == 1 ? t_max : fminf(t + (t - prev) * 0.5f, t_max);
                if (e_ri) {
                    e_ri[n] = ray;
                    e_left[n] = 0;
                    e_right[n] = 1;
                }
            }
        }
    }
}

__global__ __launch_bounds__(kWave * kPdfWaves) void k_importance_sampling(
    cnc_pdf_rows_t seg, const float* __restrict__ cdfs, const float* __restrict__ jitter, cnc_pdf_rows_t smp,
    cnc_pdf_rows_t itv)
{
    __shared__ float s_cdf[kPdfWaves][kPdfCap];
    __shared__ float s_val[kPdfWaves][kPdfCap];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t ray = (int64_t)blockIdx.x * kPdfWaves + w;
    if (ray >= seg.n_rays) return;

    int64_t base, ne;
    segment_of(seg, ray, base, ne);
    int64_t n, s0, e0;
    const bool packed = smp.n_edges_per_ray < 0;
    if (!packed) {
        n = smp.n_edges_per_ray;
        s0 = ray * n;
        e0 = ray * (n + 1);
    } else {
        n = smp.seg.chunk_cnts[ray];
        s0 = smp.seg.chunk_starts[ray];
        e0 = itv.seg.chunk_starts[ray];
    }
    if (n <= 0) {   // packed: nothing to write; batched n == 0: the one edge is the segment's first
        if (!packed && lane == 0) itv.seg.vals[e0] = ne > 0 ? seg.seg.vals[base] : __builtin_nanf("");
        return;
    }
    float* s_vals = smp.seg.vals + s0;
    int64_t* s_ri = packed ? smp.seg.ray_indices + s0 : nullptr;
    float* e_vals = itv.seg.vals + e0;
    int64_t* e_ri = packed ? itv.seg.ray_indices + e0 : nullptr;
    uint8_t* e_left = packed ? itv.seg.is_left + e0 : nullptr;
    uint8_t* e_right = packed ? itv.seg.is_right + e0 : nullptr;

    if (ne <= 0) {  // no segment to sample from: every sample and edge is NaN
        const float q = __builtin_nanf("");
        for (int64_t i = lane; i <= n; i += kWave) {
            if (i < n) {
                s_vals[i] = q;
                if (s_ri) s_ri[i] = ray;
            }
            e_vals[i] = q;
            if (e_ri) {
                e_ri[i] = ray;
                e_left[i] = i < n;
                e_right[i] = i > 0;
            }
        }
        return;
    }
    const float bias = jitter ? jitter[ray] : 0.5f;
    const float* g_cdf = cdfs + base;
    const float* g_val = seg.seg.vals + base;
    if (ne <= kPdfCap) {
        float* l_cdf = s_cdf[w];
        float* l_val = s_val[w];
        for (int i = lane; i < (int)ne; i += kWave) {
            l_cdf[i] = g_cdf[i];
            l_val[i] = g_val[i];
        }
        // the slice is the wave's own: order its LDS writes before its reads, no workgroup barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        sample_ray<int>(l_cdf, l_val, (int)ne - 1, n, bias, lane, ray, s_vals, s_ri, e_vals, e_ri, e_left, e_right);
    } else {
        sample_ray<int64_t>(g_cdf, g_val, ne - 1, n, bias, lane, ray, s_vals, s_ri, e_vals, e_ri, e_left, e_right);
    }
}

// (left, right) of value u in the key segment [base, base + cnt): p = upper bound in [base, last), both clamped to
// [base, last]; `local` subtracts base.
__device__ __forceinline__ void store_ids(int64_t p, int64_t base, int64_t last, bool local, int64_t* left,
                                          int64_t* right)
{
    int64_t l = p - 1 < last ? p - 1 : last;
    l = l > base ? l : base;
    int64_t r = p < last ? p : last;
    r = r > base ? r : base;
    *left = local ? l - base : l;
    *right = local ? r - base : r;
}

// batched query: one wave per query row, the key row staged in LDS when it fits; ids local to the row
__global__ __launch_bounds__(kWave * kPdfWaves) void k_searchsorted_rows(
    cnc_pdf_rows_t query, cnc_pdf_rows_t key, int64_t* __restrict__ ids_left, int64_t* __restrict__ ids_right)
{
    __shared__ float s_key[kPdfWaves][kPdfCap];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int64_t row = (int64_t)blockIdx.x * kPdfWaves + w;
    if (row >= query.n_rays) return;
    const int64_t nq = query.n_edges_per_ray;
    const float* q = query.seg.vals + row * nq;
    int64_t* out_l = ids_left + row * nq;
    int64_t* out_r = ids_right + row * nq;
    int64_t base, cnt;
    segment_of(key, row, base, cnt);
    const int64_t last = base + cnt - 1;
    if (cnt <= kPdfCap) {
        float* l_key = s_key[w];
        for (int i = lane; i < (int)cnt; i += kWave) l_key[i] = key.seg.vals[base + i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int hi = (int)cnt - 1 > 0 ? (int)cnt - 1 : 0;
        for (int64_t i = lane; i < nq; i += kWave) {
            const int64_t p = base + upper_bound<int>(l_key, 0, hi, q[i]);
            store_ids(p, base, last, true, out_l + i, out_r + i);
        }
    } else {
        for (int64_t i = lane; i < nq; i += kWave) {
            const int64_t p = upper_bound<int64_t>(key.seg.vals, base, last, q[i]);
            store_ids(p, base, last, true, out_l + i, out_r + i);
        }
    }
}

// flattened query: one lane per entry; its ray from ray_indices, or else the last chunk whose start is <= the entry
// (the reference's binary search of chunk_starts); ids index the flattened or batched key as a whole
__global__ __launch_bounds__(256) void k_searchsorted_entries(
    cnc_pdf_rows_t query, cnc_pdf_rows_t key, int64_t* __restrict__ ids_left, int64_t* __restrict__ ids_right)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= query.n_edges) return;
    int64_t ray;
    if (query.seg.ray_indices) {
        ray = query.seg.ray_indices[i];
    } else {
        int64_t lo = 0, hi = query.n_rays;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (!(query.seg.chunk_starts[mid] > i)) lo = mid + 1;
            else hi = mid;
        }
        ray = lo - 1;
    }
    if (ray < 0 || ray >= key.n_rays) {     // an entry outside every ray: no key segment to search
        ids_left[i] = -1;
        ids_right[i] = -1;
        return;
    }
    int64_t base, cnt;
    segment_of(key, ray, base, cnt);
    const int64_t last = base + cnt - 1;
    const int64_t p = upper_bound<int64_t>(key.seg.vals, base, last, query.seg.vals[i]);
    store_ids(p, base, last, false, ids_left + i, ids_right + i);
}

bool rows_ok(const cnc_pdf_rows_t* r)
{
    if (r == nullptr || r->n_rays < 0 || r->n_edges < 0) return false;
    if (r->n_rays > 0 && r->n_edges > 0 && r->seg.vals == nullptr) return false;
    if (r->n_edges_per_ray < 0 && r->n_rays > 0 && (r->seg.chunk_starts == nullptr || r->seg.chunk_cnts == nullptr))
        return false;
    return true;
}

}  // namespace
}  // namespace cnc

using namespace cnc;

extern "C" int cnc_importance_sampling(const cnc_pdf_rows_t* segments, const float* cdfs, const float* jitter,
                                       const cnc_pdf_rows_t* samples, const cnc_pdf_rows_t* intervals, void* stream)
{
    if (!rows_ok(segments) || samples == nullptr || intervals == nullptr) return CNC_ERR_INVALID_VALUE;
    if (segments->n_edges > 0 && cdfs == nullptr) return CNC_ERR_INVALID_VALUE;
    const bool packed = samples->n_edges_per_ray < 0;
    if (packed != (intervals->n_edges_per_ray < 0)) return CNC_ERR_INVALID_VALUE;
    if (!packed && intervals->n_edges_per_ray != samples->n_edges_per_ray + 1) return CNC_ERR_INVALID_VALUE;
    if (packed && (samples->seg.chunk_cnts == nullptr || samples->seg.chunk_starts == nullptr ||
                   intervals->seg.chunk_starts == nullptr || samples->seg.ray_indices == nullptr ||
                   intervals->seg.ray_indices == nullptr || intervals->seg.is_left == nullptr ||
                   intervals->seg.is_right == nullptr))
        return CNC_ERR_INVALID_VALUE;
    if (intervals->seg.vals == nullptr && segments->n_rays > 0) return CNC_ERR_INVALID_VALUE;
    if (segments->n_rays == 0) return CNC_OK;
    const uint64_t blocks = ((uint64_t)segments->n_rays + kPdfWaves - 1) / kPdfWaves;
    if (blocks > 0x7fffffffu) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(k_importance_sampling, dim3((uint32_t)blocks), dim3(kWave * kPdfWaves), 0,
                       (hipStream_t)stream, *segments, cdfs, jitter, *samples, *intervals);
    return launch_status();
}

extern "C" int cnc_searchsorted(const cnc_pdf_rows_t* query, const cnc_pdf_rows_t* key, int64_t* ids_left,
                                int64_t* ids_right, void* stream)
{
    if (!rows_ok(query) || !rows_ok(key)) return CNC_ERR_INVALID_VALUE;
    if (query->n_edges > 0 && (ids_left == nullptr || ids_right == nullptr)) return CNC_ERR_INVALID_VALUE;
    if (query->n_edges == 0) return CNC_OK;
    if (query->n_edges_per_ray >= 0) {
        if (key->n_rays < query->n_rays) return CNC_ERR_INVALID_VALUE;
        const uint64_t blocks = ((uint64_t)query->n_rays + kPdfWaves - 1) / kPdfWaves;
        if (blocks > 0x7fffffffu) return CNC_ERR_INVALID_VALUE;
        hipLaunchKernelGGL(k_searchsorted_rows, dim3((uint32_t)blocks), dim3(kWave * kPdfWaves), 0,
                           (hipStream_t)stream, *query, *key, ids_left, ids_right);
    } else {
        if (query->seg.ray_indices == nullptr && query->seg.chunk_starts == nullptr) return CNC_ERR_INVALID_VALUE;
        const uint64_t blocks = ((uint64_t)query->n_edges + 255) / 256;
        if (blocks > 0x7fffffffu) return CNC_ERR_INVALID_VALUE;
        hipLaunchKernelGGL(k_searchsorted_entries, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, *query,
                           *key, ids_left, ids_right);
    }
    return launch_status();
}
