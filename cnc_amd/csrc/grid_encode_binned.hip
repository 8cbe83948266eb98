// grid_encode_binned.hip — embedding-gradient scatter of the finest levels WITHOUT global atomics.
//
// Same result as kernel_grid_backward (gridencoder.cu:399-585) for the levels it is given; the
// coarser levels of the same call stay on the run-aggregated atomic kernel of grid_encode.hip.
//
// Why: on MI355X global fp32 atomics retire ~21 G (instruction, 64-byte segment) requests/s
// wherever the line lives (tools/atomic_probe.hip), and at the finest levels every sample sits in
// its own cell: 4 (y, z) corner pairs -> ~6 requests per (sample, level) that no amount of run
// merging removes.  tools/owner_probe.hip measured the alternative built here at 0.15 ms per
// 2^20-sample level against 0.31 ms for the atomic scatter:
//
//   pass 1  k_bwd_bin    every (sample, level) emits one 16-byte item per (dy, dz) corner pair —
//                        sample index, the two corner weights w/sum(w), the two slab-local rows —
//                        into the bin of the 256-row table slab that owns the pair's rows (two
//                        items if the x-neighbours straddle a slab edge).  Per workgroup the items are
//                        counted in an LDS histogram, space is reserved with ONE global atomic per
//                        (workgroup, non-empty bin), and the items are written at LDS-ranked slots.
//   pass 2  k_bwd_owner  one wave owns one slab (a bin far above the mean load is shared by several
//                        waves, which then add their partial slabs atomically): 256 rows x F floats
//                        of accumulators in LDS.  It
//                        streams its bin (items coalesced, the sample's gradient row gathered one
//                        batch ahead; the weights travel in the item, computed in pass 1 exactly as
//                        the scatter kernel computes them) and adds into LDS with plain
//                        read-modify-writes.  Claims of one batch on the same row are serialised
//                        with tickets from a per-row LDS counter (integer atomic), one round per
//                        ticket — LDS fp32 atomics were measured 5x slower than this.  The slab is then added to the gradient
//                        table with coalesced 16-byte accesses (STE mask applied there).
//
// A bin that fills up sends the excess items down the atomic path inside pass 1, so skewed inputs
// stay correct.  Summation order differs from the atomic kernel's (as it does between any two
// runs of that kernel); values agree to fp32 rounding.
#include "common.hpp"
#include "encoder_common.hpp"

#include <type_traits>

namespace cnc {

constexpr uint32_t kSlabLog2 = 8;                  // rows per owner wave (<= 12: item row fields)
constexpr uint32_t kSlab = 1u << kSlabLog2;
constexpr uint32_t kBinSamplesPerThread = 4;       // pass 1: 4096 samples per 1024-thread block
constexpr uint32_t kMaxBins = 4096;                // LDS histogram size (level_rows <= 2^20)
constexpr uint32_t kHeadBytes = 16;                // workspace bytes per bin counter (4 used)

// One corner pair of one sample at one level, as the owner wave needs it.  16 bytes, so a wave reads
// 64 items as one contiguous KiB and only the gradient row is left to gather (carrying just the sample
// index and recomputing the weights in pass 2 cost a second 64-byte sector per item for the point:
// PMC showed that pass HBM-bound at 175 B fetched per item).
struct Item {
    uint32_t sample;
    float    w0, w1;      // weight / sum of valid weights of corner x and corner x+1
    uint32_t rows;        // r0 | r1 << 12 | mask << 24; mask bit 0: add row r0, bit 1: add row r1
};
static_assert(sizeof(Item) == 16, "Item is read as one dwordx4");

struct BinnedArgs {
    const float*    grad;
    const float*    inputs;
    const float*    emb;
    const int32_t*  offsets;
    const int32_t*  resolutions;
    float*          grad_emb;
    uint32_t        N;
    uint32_t        first_level;     // binned levels are [first_level, first_level + n_binned)
    uint32_t        bins;            // slabs per level = ceil(level_rows / 256)
    uint32_t        cap;             // item slots per bin
    uint32_t        part;            // items one owner wave takes (a fuller bin is shared by several waves)
    uint32_t        parts;           // owner waves per bin = ceil(cap / part)
    uint32_t        n_pairs;         // owner pass: levels [0, 2 * n_pairs) are placed pairwise (owner_slab)
    uint32_t*       bin_count;       // [n_binned][bins]
    Item*           items;           // [n_binned][bins][cap]
    const uint32_t* clip_count;
    FeatLayout      lay;
};

template <uint32_t F, bool STE>
__device__ __forceinline__ void atomic_row(const BinnedArgs& a, bool mask_on, uint32_t abs_row,
                                           float tw, const float* __restrict__ g)
{
#pragma unroll
    for (uint32_t f = 0; f < F; f++) {
        const size_t at = (size_t)abs_row * F + f;
        if (mask_on) {
            const float e = a.emb[at];
            if (!(e >= -1.0f && e <= 1.0f)) continue;
        }
        unsafeAtomicAdd(a.grad_emb + at, tw * g[f]);
    }
}

template <uint32_t F, bool STE>
__global__ __launch_bounds__(1024) void k_bwd_bin(BinnedArgs a)
{
    __shared__ uint32_t s_cnt[kMaxBins];
    const uint32_t slot = a.first_level + blockIdx.y;
    const uint32_t off = (uint32_t)a.offsets[slot];
    const uint32_t hs = (uint32_t)a.offsets[slot + 1] - off;
    const uint32_t R = (uint32_t)a.resolutions[slot];
    // a level with more rows than the caller sized the bins for cannot be binned: all atomics
    const bool     binnable = div_up(hs, kSlab) <= a.bins;
    const bool     mask_on = STE && (a.clip_count == nullptr || *a.clip_count != 0);
    uint32_t*      bin_count = a.bin_count + (size_t)blockIdx.y * a.bins;
    Item*          items = a.items + (size_t)blockIdx.y * a.bins * a.cap;
    const uint32_t base_i = blockIdx.x * 1024 * kBinSamplesPerThread;
    LevelGeom3     lv;
    lv.init(R, hs);

    for (uint32_t b = threadIdx.x; b < a.bins; b += 1024) s_cnt[b] = 0;
    __syncthreads();

    // ---- count (rows and validity only; the level's kind decided once, see LevelGeom3) ----
    auto count = [&](auto hp2) {
#pragma unroll
        for (uint32_t k = 0; k < kBinSamplesPerThread; k++) {
            const uint32_t i = base_i + k * 1024 + threadIdx.x;
            float x[3];
            if (i < a.N && load_point<3>(a.inputs, i, x)) {
                corner_rows3<decltype(hp2)::value>(x, lv, [&](uint32_t p, bool v0, bool v1, uint32_t r0, uint32_t r1) {
                    const uint32_t b0 = r0 >> kSlabLog2, b1 = r1 >> kSlabLog2;
                    if (v0) atomicAdd(&s_cnt[b0], 1u);
                    if (v1 && !(v0 && b1 == b0)) atomicAdd(&s_cnt[b1], 1u);
                });
            }
        }
    };
    if (binnable) {
        if (lv.hashed_pow2()) count(std::true_type{});
        else count(std::false_type{});
    }
    __syncthreads();
    // ---- reserve: one global atomic per non-empty bin of this block ----
    for (uint32_t b = threadIdx.x; b < a.bins; b += 1024) {
        const uint32_t n = s_cnt[b];
        s_cnt[b] = n ? atomicAdd(&bin_count[b], n) : 0u;
    }
    __syncthreads();
    // ---- emit ----
#pragma unroll
    for (uint32_t k = 0; k < kBinSamplesPerThread; k++) {
        const uint32_t i = base_i + k * 1024 + threadIdx.x;
        float x[3];
        if (!(i < a.N && load_point<3>(a.inputs, i, x))) continue;
        Corners<3, false> c;
        c.setup(x, R, hs, 0, nullptr);
        uint32_t spill = 0;   // corners whose item found no room (or level not binnable)
#pragma unroll
        for (uint32_t p = 0; p < 4; p++) {
            const bool     v0 = c.valid[2 * p], v1 = c.valid[2 * p + 1];
            const uint32_t b0 = c.row[2 * p] >> kSlabLog2, b1 = c.row[2 * p + 1] >> kSlabLog2;
            if (!binnable) {
                spill |= (v0 ? 1u : 0u) << (2 * p) | (v1 ? 1u : 0u) << (2 * p + 1);
                continue;
            }
            const bool together = v0 && v1 && b1 == b0;
            Item it;
            it.sample = i;
            it.w0 = c.w[2 * p] * c.wn_re;
            it.w1 = c.w[2 * p + 1] * c.wn_re;
            const uint32_t lr = (c.row[2 * p] & (kSlab - 1)) | (c.row[2 * p + 1] & (kSlab - 1)) << 12;
            if (v0) {
                const uint32_t at = atomicAdd(&s_cnt[b0], 1u);
                it.rows = lr | (together ? 3u : 1u) << 24;
                if (at < a.cap) items[(size_t)b0 * a.cap + at] = it;
                else spill |= (together ? 3u : 1u) << (2 * p);
            }
            if (v1 && !together) {
                const uint32_t at = atomicAdd(&s_cnt[b1], 1u);
                it.rows = lr | 2u << 24;
                if (at < a.cap) items[(size_t)b1 * a.cap + at] = it;
                else spill |= 2u << (2 * p);
            }
        }
        // the slow path: spilled corners are added atomically
        if (spill) {
            constexpr uint32_t V = F < 4 ? F : 4;
            float        g[F];
            const float* gp = a.grad + feat_index(a.lay, slot, a.N, i, F);
#pragma unroll
            for (uint32_t q = 0; q < F; q += V) {
                float gv[V];
                load_vec<V>(gp + q, gv);
#pragma unroll
                for (uint32_t j = 0; j < V; j++) g[q + j] = gv[j];
            }
#pragma unroll
            for (uint32_t q = 0; q < 8; q++)
                if ((spill >> q) & 1u)
                    atomic_row<F, STE>(a, mask_on, off + c.row[q], c.w[q] * c.wn_re, g);
        }
    }
}

// ---- pass 1, second form: the block's items leave in BIN ORDER ------------------------------------------------
// k_bwd_bin above lets every lane store its own items: the 8 or so items a block adds to one bin are contiguous in
// memory but written by different lanes of different waves at different times, and the L2 merges only part of them
// into full sectors — rocprofv3 counts 9.6 M write requests per 7-level pass for 235 MB of items (1.5 items per
// 64-byte request), and with everything else overlapped the whole backward call sits on the L2 -> fabric request
// rate (53 M requests in 1.06 ms = 50 G/s, the ceiling of tools/fetch_calib.hip).  Here the block sorts the SOURCE
// IDS of its items by bin in LDS (a 16-bit id per item: 40 KB where the 16-byte payloads would need 256 KB) and then
// walks the sorted list: lane t rebuilds item t from its sample and stores it, so that a wave-instruction writes 64
// consecutive slots of the sorted order — whole (block, bin) runs, 128 contiguous bytes on average.
// The set-up runs once per sample to count and once per item in the walk, about 5.4 times per (sample, level), and the
// pass shares the SIMDs with the vector-issue-bound merge kernel of the coarse levels on the other stream: the count
// phase takes rows and validity only (corner_rows3) and the walk one corner pair (CornerPair3), not the general
// Corners::setup; the cold paths keep that one.  The weights' sum and its division are per sample, not per item: the
// count phase, which visits every sample once, computes 1 / sum as Corners::setup does and leaves it in LDS (s_wn, one
// float per sample of the block: 16 KB), and the walk's lane reads it for its item's sample.
constexpr uint32_t kSortBins = 2048;                                  // three LDS arrays of that many words
#ifndef CNC_SORT_SAMPLES_PER_THREAD
#define CNC_SORT_SAMPLES_PER_THREAD 4
#endif
constexpr uint32_t kSortSamplesPerThread = CNC_SORT_SAMPLES_PER_THREAD;   // 4096 samples per block: runs of 8 items per bin
constexpr uint32_t kSortItems = 1024 * kSortSamplesPerThread * 5;     // source ids per block (typically 4.2 per sample)

// The item of one corner pair from its two weights, rows and validity flags (half 0: the x corner's bin, carrying both
// corners when they share it; half 1: the x+1 corner's bin when it differs) — exactly what k_bwd_bin emits.  The one place
// that packs an item of the sorted pass.
__device__ __forceinline__ Item make_item(uint32_t sample, uint32_t half, float w0, float w1, uint32_t r0, uint32_t r1, bool v0,
                                          bool v1, float wn_re, uint32_t& bin, uint32_t& mask)
{
    const uint32_t b0 = r0 >> kSlabLog2, b1 = r1 >> kSlabLog2;
    const bool     together = v0 && v1 && b1 == b0;
    Item           it;
    it.sample = sample;
    it.w0 = w0 * wn_re;
    it.w1 = w1 * wn_re;
    mask = half ? 2u : (together ? 3u : 1u);
    bin = half ? b1 : b0;
    it.rows = (r0 & (kSlab - 1)) | (r1 & (kSlab - 1)) << 12 | mask << 24;
    return it;
}

// item of corner pair p of a full set-up
__device__ __forceinline__ Item pair_item(const Corners<3, false>& c, uint32_t sample, uint32_t p, uint32_t half, uint32_t& bin,
                                          uint32_t& mask)
{
    // p may be a run-time value: pick the pair with selects (indexing the corner arrays dynamically would send them
    // to scratch memory)
    bool     v0 = false, v1 = false;
    uint32_t r0 = 0, r1 = 0;
    float    w0 = 0, w1 = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
        const bool hit = q == p;
        v0 = hit ? c.valid[2 * q] : v0;
        v1 = hit ? c.valid[2 * q + 1] : v1;
        r0 = hit ? c.row[2 * q] : r0;
        r1 = hit ? c.row[2 * q + 1] : r1;
        w0 = hit ? c.w[2 * q] : w0;
        w1 = hit ? c.w[2 * q + 1] : w1;
    }
    return make_item(sample, half, w0, w1, r0, r1, v0, v1, c.wn_re, bin, mask);
}

// the same item from the one-pair set-up (the walk of k_bwd_bin_sorted): no selects over the corners
__device__ __forceinline__ Item pair_item(const CornerPair3& c, uint32_t sample, uint32_t half, uint32_t& bin, uint32_t& mask)
{
    return make_item(sample, half, c.w0, c.w1, c.row0, c.row1, c.valid0, c.valid1, c.wn_re, bin, mask);
}

template <uint32_t F, bool STE>
__global__ __launch_bounds__(1024) void k_bwd_bin_sorted(BinnedArgs a)
{
    __shared__ uint32_t s_start[kSortBins];       // items of this block per bin, then their first position in s_src
    __shared__ uint32_t s_base[kSortBins];        // first slot of the block's run inside the bin (global reservation)
    __shared__ uint16_t s_src[kSortItems];        // source ids in bin order: sample-in-block | pair << 13 | half << 15
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_total;
    __shared__ float    s_wn[1024 * kSortSamplesPerThread];   // 1 / (sum of the valid weights) per sample: count phase -> walk
    const uint32_t slot = a.first_level + blockIdx.y;
    const uint32_t off = (uint32_t)a.offsets[slot];
    const uint32_t hs = (uint32_t)a.offsets[slot + 1] - off;
    const uint32_t R = (uint32_t)a.resolutions[slot];
    const bool     binnable = div_up(hs, kSlab) <= a.bins;
    const bool     mask_on = STE && (a.clip_count == nullptr || *a.clip_count != 0);
    uint32_t*      bin_count = a.bin_count + (size_t)blockIdx.y * a.bins;
    Item*          items = a.items + (size_t)blockIdx.y * a.bins * a.cap;
    const uint32_t base_i = blockIdx.x * 1024 * kSortSamplesPerThread;
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t V = F < 4 ? F : 4;
    LevelGeom3     lv;
    lv.init(R, hs);

    // sample i's gradient row of this level: what a spilled corner adds atomically
    auto grad_row = [&](uint32_t i, float (&g)[F]) {
        const float* gp = a.grad + feat_index(a.lay, slot, a.N, i, F);
#pragma unroll
        for (uint32_t q = 0; q < F; q += V) {
            float gv[V];
            load_vec<V>(gp + q, gv);
#pragma unroll
            for (uint32_t j = 0; j < V; j++) g[q + j] = gv[j];
        }
    };
    auto spill_corners = [&](const Corners<3, false>& c, uint32_t i, uint32_t corners) {
        float g[F];
        grad_row(i, g);
#pragma unroll
        for (uint32_t q = 0; q < 8; q++)
            if ((corners >> q) & 1u) atomic_row<F, STE>(a, mask_on, off + c.row[q], c.w[q] * c.wn_re, g);
    };
    // the same for the corners `mask` of one pair, from the pair's own set-up: the item's weights are the products above
    auto spill_pair = [&](const CornerPair3& c, const Item& it, uint32_t mask) {
        float g[F];
        grad_row(it.sample, g);
        if (mask & 1u) atomic_row<F, STE>(a, mask_on, off + c.row0, it.w0, g);
        if (mask & 2u) atomic_row<F, STE>(a, mask_on, off + c.row1, it.w1, g);
    };

    if (!binnable) {      // a level with more rows than the bins were sized for: every corner goes to atomics
#pragma unroll
        for (uint32_t k = 0; k < kSortSamplesPerThread; k++) {
            const uint32_t i = base_i + k * 1024 + tid;
            float x[3];
            if (!(i < a.N && load_point<3>(a.inputs, i, x))) continue;
            Corners<3, false> c;
            c.setup(x, R, hs, 0, nullptr);
            uint32_t all = 0;
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) all |= (c.valid[q] ? 1u : 0u) << q;
            if (all) spill_corners(c, i, all);
        }
        return;
    }

    for (uint32_t b = tid; b < kSortBins; b += 1024) s_start[b] = 0;
    __syncthreads();
    // ---- count: every item takes its rank inside its bin; (bin, rank) stay in registers ----
    // (rows and validity only; the level's kind is decided once for the block, see LevelGeom3)
    uint32_t key[kSortSamplesPerThread][8];
    auto count = [&](auto hp2) {
#pragma unroll
        for (uint32_t k = 0; k < kSortSamplesPerThread; k++) {
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) key[k][q] = 0xFFFFFFFFu;
            const uint32_t i = base_i + k * 1024 + tid;
            float x[3];
            if (i < a.N && load_point<3>(a.inputs, i, x)) {
                s_wn[k * 1024 + tid] = CornerPair3::normaliser(x, lv);     // (an outside point's slot: never written, never read)
                corner_rows3<decltype(hp2)::value>(x, lv, [&](uint32_t p, bool v0, bool v1, uint32_t r0, uint32_t r1) {
                    const uint32_t b0 = r0 >> kSlabLog2, b1 = r1 >> kSlabLog2;
                    if (v0) key[k][2 * p] = b0 | atomicAdd(&s_start[b0], 1u) << 11;
                    if (v1 && !(v0 && b1 == b0)) key[k][2 * p + 1] = b1 | atomicAdd(&s_start[b1], 1u) << 11;
                });
            }
        }
    };
    if (lv.hashed_pow2()) count(std::true_type{});
    else count(std::false_type{});
    __syncthreads();
    // ---- reserve (one global atomic per non-empty bin of this block) and exclusive prefix over the bins ----
    const uint32_t n0 = s_start[2 * tid], n1 = s_start[2 * tid + 1];
    s_base[2 * tid] = (n0 && 2 * tid < a.bins) ? atomicAdd(&bin_count[2 * tid], n0) : 0u;
    s_base[2 * tid + 1] = (n1 && 2 * tid + 1 < a.bins) ? atomicAdd(&bin_count[2 * tid + 1], n1) : 0u;
    uint32_t incl = n0 + n1;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) before += (w < (tid >> 6)) ? s_wave[w] : 0u;
    const uint32_t excl = before + incl - (n0 + n1);
    s_start[2 * tid] = excl;
    s_start[2 * tid + 1] = excl + n0;
    if (tid == 1023) s_total = before + incl;
    __syncthreads();
    const uint32_t total = s_total;
    if (total > kSortItems) {
        // more items than the id list holds (straddling pairs everywhere): this block stores lane by lane, as
        // k_bwd_bin does
#pragma unroll
        for (uint32_t k = 0; k < kSortSamplesPerThread; k++) {
            const uint32_t i = base_i + k * 1024 + tid;
            float x[3];
            if (!(i < a.N && load_point<3>(a.inputs, i, x))) continue;
            Corners<3, false> c;
            c.setup(x, R, hs, 0, nullptr);
            uint32_t spill = 0;
#pragma unroll
            for (uint32_t q = 0; q < 8; q++) {
                if (key[k][q] == 0xFFFFFFFFu) continue;
                uint32_t bin, mask;
                const Item it = pair_item(c, i, q >> 1, q & 1u, bin, mask);
                const uint32_t at = s_base[bin] + (key[k][q] >> 11);
                if (at < a.cap) items[(size_t)bin * a.cap + at] = it;
                else spill |= mask << (q & ~1u);
            }
            if (spill) spill_corners(c, i, spill);
        }
        return;
    }
    // ---- source ids into bin order ----
#pragma unroll
    for (uint32_t k = 0; k < kSortSamplesPerThread; k++)
#pragma unroll
        for (uint32_t q = 0; q < 8; q++)
            if (key[k][q] != 0xFFFFFFFFu)
                s_src[s_start[key[k][q] & 0x7FFu] + (key[k][q] >> 11)] = (uint16_t)((k * 1024 + tid) | (q >> 1) << 13 | (q & 1u) << 15);
    __syncthreads();
    // ---- walk the sorted list: consecutive lanes, consecutive slots (one corner pair's set-up per item) ----
    auto walk = [&](auto hp2) {
        for (uint32_t pos = tid; pos < total; pos += 1024) {
            const uint32_t src = s_src[pos];
            const uint32_t i = base_i + (src & 0x1FFFu);
            float x[3];
            load_point<3>(a.inputs, i, x);
            CornerPair3 c;
            c.setup_pair<decltype(hp2)::value>(x, lv, (src >> 13) & 3u, s_wn[src & 0x1FFFu]);
            uint32_t bin, mask;
            const Item it = pair_item(c, i, (src >> 15) & 1u, bin, mask);
            const uint32_t at = s_base[bin] + (pos - s_start[bin]);
            if (at < a.cap) items[(size_t)bin * a.cap + at] = it;
            else spill_pair(c, it, mask);
        }
    };
    if (lv.hashed_pow2()) walk(std::true_type{});
    else walk(std::false_type{});
}

// LDS accumulators are stored by 16-byte chunk: acc[chunk][row][4 floats].  With row-major
// [row][F] a 16-byte access of random rows only ever touches every other 16-byte bank group (the
// first halves of 32-byte rows), doubling the conflicts of the read-modify-write that bounds pass 2.
template <uint32_t F>
__device__ __forceinline__ uint32_t acc_index(uint32_t row, uint32_t q)
{
    constexpr uint32_t V = F < 4 ? F : 4;
    return ((q / V) * kSlab + row) * V + (q % V);
}

// read-modify-write of one accumulator row (F floats) in LDS
template <uint32_t F>
__device__ __forceinline__ void lds_row_add(float* __restrict__ acc, uint32_t row, const float (&v)[F])
{
    constexpr uint32_t V = F < 4 ? F : 4;
    using T = typename vecf<V>::type;
#pragma unroll
    for (uint32_t q = 0; q < F; q += V) {
        T*     p = reinterpret_cast<T*>(acc + acc_index<F>(row, q));
        T      t = *p;
        float* f = reinterpret_cast<float*>(&t);
#pragma unroll
        for (uint32_t j = 0; j < V; j++) f[j] += v[q + j];
        *p = t;
    }
}

// ---- pass 2: which slab a workgroup of the 1-D owner grid takes ------------------------------------------------
// Workgroups are dealt round-robin over the chip's 8 XCDs (observed: ids w and w + 8 share one; tools/xcd_label_probe.hip
// checks it) and each XCD has its own L2.  The paired placement (CNC_FLAG_OWNER_XCD_PAIRS, a measurement switch) puts the
// owner waves of a level on 4 of the 8: levels 2p and 2p + 1 share one id range in which ids with (w % 8) < 4 enumerate
// the first level's (part, bin) slabs and the others the second's, 4 per 8 consecutive ids; `bins` is padded to a multiple
// of 8 there and the surplus ids own nothing.  The levels from 2 * n_pairs on (all of them with the flag unset, a trailing
// odd one with it) follow level by level, part * bins + bin within each, over all 8 labels.
// What it was built to test: if a 64-byte gradient sector, wanted by 8 items in 8 unrelated bins, were fetched once per
// XCD hosting one of them, 4 XCDs would need 3.60 fetches where 8 need 5.25.  Measured: read requests -2 %, time
// unchanged — the bins' waves are too far apart in the sample stream to share through an L2
// (profiles/r09_owner_xcd_placement.md); off by default.
// w % 8 is a group label, not an XCD id, and nothing depends on it for correctness: every id decodes to its own
// (level, bin, part) and the workgroup owns exactly that slab, so another dispatch order changes speed only.
// (tests/test_owner_grid.py holds a Python twin of this function.)
__host__ __device__ __forceinline__ uint32_t owner_bins_padded(uint32_t bins) { return (bins + 7u) & ~7u; }

__host__ __device__ __forceinline__ uint64_t owner_grid_size(uint32_t n_binned, uint32_t bins, uint32_t parts, uint32_t n_pairs)
{
    return (uint64_t)n_pairs * 2 * parts * owner_bins_padded(bins) + (uint64_t)(n_binned - 2 * n_pairs) * parts * bins;
}

__device__ __forceinline__ void owner_slab(uint32_t w, uint32_t bins, uint32_t parts, uint32_t n_pairs, uint32_t& level,
                                           uint32_t& bin, uint32_t& part)
{
    const uint32_t padded = owner_bins_padded(bins);
    const uint32_t pair_ids = 2 * parts * padded;       // a multiple of 16: every pair starts at label 0
    if (w < n_pairs * pair_ids) {
        const uint32_t pair = w / pair_ids, v = w % pair_ids;
        const uint32_t idx = (v >> 3) * 4 + (v & 3u);   // position among its half's ids
        level = 2 * pair + ((v >> 2) & 1u);
        part = idx / padded;
        bin = idx % padded;
    } else {
        const uint32_t v = w - n_pairs * pair_ids, per_level = parts * bins;
        const uint32_t u = v % per_level;
        level = 2 * n_pairs + v / per_level;
        part = u / bins;
        bin = u % bins;
    }
}

template <uint32_t F, bool STE>
__global__ __launch_bounds__(64) void k_bwd_owner(BinnedArgs a)
{
    constexpr uint32_t V = F < 4 ? F : 4;
    __shared__ __attribute__((aligned(16))) float s_acc[kSlab * F];
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[kSlab];
    static_assert(kSlab * sizeof(uint32_t) == 64 * sizeof(uint4), "one uint4 per lane clears the tickets");
    // Within a level the id runs as part * bins + bin: the waves that take the second, third ... `part` items of a
    // bin are scheduled after every bin's first wave — they exist only for bins far above the mean (thin slices of
    // space hash unevenly onto the slabs: up to 7.7x the mean at resolution 296 on the first chunk of the
    // bench frame, where one wave per bin made the pass 2x slower than on the other chunks)
    uint32_t level, bin, part;
    owner_slab(blockIdx.x, a.bins, a.parts, a.n_pairs, level, bin, part);
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = a.first_level + level;
    const uint32_t off = (uint32_t)a.offsets[slot];
    const uint32_t hs = (uint32_t)a.offsets[slot + 1] - off;
    if (bin >= a.bins || bin * kSlab >= hs) return;     // padding of the paired ranges, rows past the level's end
    uint32_t n = a.bin_count[(size_t)level * a.bins + bin];
    n = n < a.cap ? n : a.cap;
    if (n <= part * a.part) return;     // nothing (more) landed here: the table slab stays as it is
    const bool  shared_slab = n > a.part;
    const Item* my = a.items + ((size_t)level * a.bins + bin) * a.cap + (size_t)part * a.part;
    n = min(n - part * a.part, a.part);

    for (uint32_t k = lane * 4; k < kSlab * F; k += 64 * 4)     // 16-byte LDS stores
        *reinterpret_cast<float4*>(s_acc + k) = make_float4(0, 0, 0, 0);

    // Two loads deep: while batch i is accumulated, the gradient rows of batch i+1 and the items of
    // batch i+2 are in flight (the gradient address needs the item, so a one-deep prefetch waits for
    // the two latencies back to back in every iteration — the pass was bound by exactly that).
    // A batch takes kRun consecutive items from each of 64 / kRun regions of the bin rather
    // than 64 consecutive ones: items of one cell arrive clustered (neighbouring rays of one pass-1
    // block), and every extra claim on a row costs the batch another round.
    constexpr uint32_t kRun = 8, kRegions = 64 / kRun;         // consecutive items per region and batch
    const uint32_t region = (div_up(n, kRegions) + kRun - 1) & ~(kRun - 1);   // items per region
    uint32_t       step = 0;                                   // item batches requested so far
    uint4          it2 = make_uint4(0, 0, 0, 0), it1 = make_uint4(0, 0, 0, 0);
    bool           valid2 = false, valid1 = false;
    float          g1[F];
    auto           fetch_items = [&]() {
        const uint32_t in_region = step * kRun + (lane % kRun);
        const uint32_t j = (lane / kRun) * region + in_region;
        valid2 = in_region < region && j < n;
        if (valid2) it2 = *reinterpret_cast<const uint4*>(my + j);
        step++;
    };
    auto fetch_grad = [&]() {
        if (valid1) {
            const float* gp = a.grad + feat_index(a.lay, slot, a.N, it1.x, F);
#pragma unroll
            for (uint32_t q = 0; q < F; q += V) {
                float gv[V];
                load_vec<V>(gp + q, gv);
#pragma unroll
                for (uint32_t t = 0; t < V; t++) g1[q + t] = gv[t];
            }
        }
    };
    fetch_items();
    it1 = it2;
    valid1 = valid2;
    fetch_items();
    fetch_grad();
    __syncthreads();   // single wave: orders the zero-fill before the first accumulate

    while (__ballot(valid1) != 0) {
        uint32_t pend = 0, r0 = 0, r1 = 0;
        float    v0[F], v1[F];
        if (valid1) {
            pend = (it1.w >> 24) & 3u;
            r0 = it1.w & 0xFFFu;
            r1 = (it1.w >> 12) & 0xFFFu;
            const float w0 = __uint_as_float(it1.y), w1 = __uint_as_float(it1.z);
#pragma unroll
            for (uint32_t f = 0; f < F; f++) {
                v0[f] = w0 * g1[f];
                v1[f] = w1 * g1[f];
            }
        }
        it1 = it2;
        valid1 = valid2;
        fetch_items();
        fetch_grad();
        // Claims on the same row must not share an LDS instruction.  Every claim takes a ticket from
        // a per-row counter (one integer LDS atomic); round k serves the claims holding ticket k, so
        // all rows touched in a round are distinct and its reads and writes need no ordering among
        // themselves.  Rounds = the largest number of claims on one row.  The x and the x+1 rows of
        // the items are served in two phases with their own tickets: 64 instead of 128 claims on the
        // 256 rows per phase (64 random claims already put 2-3 on one row), and a round is 4 instead
        // of 8 16-byte LDS operations — 8.1 half-rounds per batch where the joint scheme needed 6.5
        // full ones (marched rays, 7 levels).  LDS instructions of a wave execute in order, which
        // orders the counter reset, the tickets and the rounds.
        reinterpret_cast<uint4*>(s_cnt)[lane] = make_uint4(0, 0, 0, 0);
        asm volatile("" ::: "memory");
        const int32_t t0 = (pend & 1u) ? (int32_t)atomicAdd(&s_cnt[r0], 1u) : -1;
        for (int32_t k = 0; __ballot(t0 >= k) != 0; k++) {
            if (t0 == k) lds_row_add<F>(s_acc, r0, v0);
            asm volatile("" ::: "memory");
        }
        reinterpret_cast<uint4*>(s_cnt)[lane] = make_uint4(0, 0, 0, 0);
        asm volatile("" ::: "memory");
        const int32_t t1 = (pend & 2u) ? (int32_t)atomicAdd(&s_cnt[r1], 1u) : -1;
        for (int32_t k = 0; __ballot(t1 >= k) != 0; k++) {
            if (t1 == k) lds_row_add<F>(s_acc, r1, v1);
            asm volatile("" ::: "memory");
        }
    }
    __syncthreads();

    // ---- slab -> gradient table ----
    const bool     mask_on = STE && (a.clip_count == nullptr || *a.clip_count != 0);
    const uint32_t rows = min(kSlab, hs - bin * kSlab);
    const size_t   base = ((size_t)off + (size_t)bin * kSlab) * F;
    constexpr uint32_t NI = kSlab * F / (64 * V);     // 8 at F = 8: all loads issued before the first use
    if (shared_slab) {
        // several waves hold partial sums of this slab: coalesced atomics instead of the read-modify-write
#pragma unroll
        for (uint32_t i = 0; i < NI; i++) {
            const uint32_t k = (i * 64 + lane) * V;
            if (k < rows * F) {
                float e[V];
                if (mask_on) load_vec<V>(a.emb + base + k, e);
#pragma unroll
                for (uint32_t q = 0; q < V; q++)
                    if (!mask_on || (e[q] >= -1.0f && e[q] <= 1.0f))
                        unsafeAtomicAdd(a.grad_emb + base + k + q, s_acc[acc_index<F>(k / F, k % F + q)]);
            }
        }
        return;
    }
    // this wave is the only writer of these rows in this pass
    float t[NI][V], e[NI][V];
#pragma unroll
    for (uint32_t i = 0; i < NI; i++) {
        const uint32_t k = (i * 64 + lane) * V;
        if (k < rows * F) {
            load_vec<V>(a.grad_emb + base + k, t[i]);
            if (mask_on) load_vec<V>(a.emb + base + k, e[i]);
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < NI; i++) {
        const uint32_t k = (i * 64 + lane) * V;
        if (k < rows * F) {
#pragma unroll
            for (uint32_t q = 0; q < V; q++) {
                const bool pass = !mask_on || (e[i][q] >= -1.0f && e[i][q] <= 1.0f);
                t[i][q] += pass ? s_acc[acc_index<F>(k / F, k % F + q)] : 0.0f;
            }
            store_vec<V>(a.grad_emb + base + k, t[i]);
        }
    }
}

template <uint32_t F>
static void launch_binned(const BinnedArgs& a, uint32_t n_binned, bool ste, bool sorted, hipStream_t s)
{
    sorted = sorted && a.bins <= kSortBins;
    const dim3 g1(div_up(a.N, 1024 * (sorted ? kSortSamplesPerThread : kBinSamplesPerThread)), n_binned),
        g2((uint32_t)owner_grid_size(n_binned, a.bins, a.parts, a.n_pairs));
    if (ste) {
        if (sorted) hipLaunchKernelGGL((k_bwd_bin_sorted<F, true>), g1, dim3(1024), 0, s, a);
        else hipLaunchKernelGGL((k_bwd_bin<F, true>), g1, dim3(1024), 0, s, a);
        hipLaunchKernelGGL((k_bwd_owner<F, true>), g2, dim3(64), 0, s, a);
    } else {
        if (sorted) hipLaunchKernelGGL((k_bwd_bin_sorted<F, false>), g1, dim3(1024), 0, s, a);
        else hipLaunchKernelGGL((k_bwd_bin<F, false>), g1, dim3(1024), 0, s, a);
        hipLaunchKernelGGL((k_bwd_owner<F, false>), g2, dim3(64), 0, s, a);
    }
}

}  // namespace cnc

using namespace cnc;

// mean bin load: 4 items per sample and level spread over the slabs
static uint64_t mean_load(uint32_t N, uint32_t bins) { return (4ull * N + bins - 1) / bins; }

// 8x the mean bin load, at least one batch.  Samples from a thin slice of space hash unevenly onto the slabs
// (the high bits of a row come from (y, z) alone): the fullest bin held 7.7x the mean on the first chunk
// of the bench frame at resolution 296, 2.4x in the middle of the frame.
static uint32_t default_cap(uint32_t N, uint32_t bins)
{
    const uint64_t cap = 8 * mean_load(N, bins) + 64;
    return (uint32_t)(cap > 0xFFFFFFFFull ? 0xFFFFFFFFull : cap);
}

// items per owner wave: 2x the mean (one wave per bin unless the bin is that far above it), whole batches
static uint32_t owner_part(uint32_t N, uint32_t bins, uint64_t cap)
{
    uint64_t part = (2 * mean_load(N, bins) + 63) / 64 * 64;     // 1.25x / 1.5x / 3x: the same; 1x: 13 % slower
    if (part < 64) part = 64;
    while ((cap + part - 1) / part > 16) part *= 2;      // a roomy caller-sized workspace: at most 16 waves per bin
    return (uint32_t)(part > 0xFFFFFFFFull ? 0xFFFFFFFFull : part);
}

extern "C" uint64_t cnc_grid_encode_backward_binned_workspace(uint32_t N, uint32_t n_binned,
                                                              uint32_t level_rows)
{
    if (n_binned == 0 || level_rows == 0) return 0;
    const uint64_t bins = div_up(level_rows, kSlab);
    return (uint64_t)n_binned * bins * (kHeadBytes + (uint64_t)default_cap(N, (uint32_t)bins) * sizeof(Item));
}

// cnc_grid_encode_backward_binned on a checked call (the overlapped entry hands its level groups in as calls of their own)
int cnc::grid_encode_backward_binned(const EncoderCall& c, uint32_t n_binned, uint32_t level_rows, void* workspace,
                                     uint64_t workspace_bytes)
{
    const uint32_t N = c.N, F = c.F, L = c.L;
    if (n_binned > L) return CNC_ERR_INVALID_VALUE;
    // what is not binned goes through the atomic kernel, with the same arguments
    if (L - n_binned > 0) {
        // scratch beyond what the bins were asked for (what cnc_grid_encode_backward_overlapped_workspace adds, when that
        // entry hands a call on as a whole): its tail holds the segment order of the merge kernel's depth-ranked tiles
        uint16_t* tile_order = split_scratch(N, n_binned, level_rows, false, workspace, workspace_bytes);
        const int rc = grid_encode_backward_with_scratch(coarse_levels(c, L - n_binned, tile_order));
        if (rc != CNC_OK) return rc;
    }
    if (n_binned == 0) return CNC_OK;
    if (c.D != 3 || !(F == 2 || F == 4 || F == 8)) return CNC_ERR_UNSUPPORTED;
    if (!layout_ok(c.lay, F, L)) return CNC_ERR_INVALID_VALUE;
    const uint32_t bins = div_up(level_rows, kSlab);
    if (bins == 0 || bins > kMaxBins || !workspace) return CNC_ERR_INVALID_VALUE;
    // layout: [heads x 16 B: bin counters, padded so the items stay 16-byte aligned][heads x cap items]
    const uint64_t heads = (uint64_t)n_binned * bins;
    if ((uintptr_t)workspace % 16 != 0) return CNC_ERR_INVALID_VALUE;
    if (workspace_bytes < heads * (kHeadBytes + 64 * sizeof(Item))) return CNC_ERR_INVALID_VALUE;   // one batch per bin
    uint64_t cap = (workspace_bytes - heads * kHeadBytes) / (heads * sizeof(Item));
    if (cap > 0x0FFFFFFFull) cap = 0x0FFFFFFFull;

    uint32_t* ws = (uint32_t*)workspace;
    if (hipMemsetAsync(ws, 0, heads * 4, c.stream) != hipSuccess) return CNC_ERR_LAUNCH;
    const uint32_t part = owner_part(N, bins, cap), parts = div_up((uint32_t)cap, part);
    // pairs of levels on complementary halves of the XCD labels (owner_slab); an odd level out stays on all eight
    const uint32_t n_pairs = (c.flags & CNC_FLAG_OWNER_XCD_PAIRS) ? n_binned / 2 : 0;
    if (owner_grid_size(n_binned, bins, parts, n_pairs) > 0x7FFFFFFFull) return CNC_ERR_INVALID_VALUE;
    const BinnedArgs a{c.grad, c.inputs, c.emb, c.offsets, c.resolutions, c.out, N, L - n_binned,
                       bins, (uint32_t)cap, part, parts, n_pairs, ws, (Item*)((char*)workspace + heads * kHeadBytes),
                       c.clip_count, c.plain_layout()};
    const bool sorted = (c.flags & CNC_FLAG_BIN_LANE_STORES) == 0;
    switch (F) {
    case 2: launch_binned<2>(a, n_binned, c.ste(), sorted, c.stream); break;
    case 4: launch_binned<4>(a, n_binned, c.ste(), sorted, c.stream); break;
    default: launch_binned<8>(a, n_binned, c.ste(), sorted, c.stream); break;
    }
    return launch_status();
}

extern "C" int cnc_grid_encode_backward_binned(const float* grad, const float* inputs,
                                               const float* embeddings, const int32_t* offsets,
                                               const int32_t* resolutions, float* grad_embeddings,
                                               uint32_t N, uint32_t D, uint32_t F, uint32_t L,
                                               uint32_t flags, const uint32_t* ste_clip_count,
                                               uint32_t grad_ld, uint32_t grad_col,
                                               uint32_t n_binned, uint32_t level_rows,
                                               void* workspace, uint64_t workspace_bytes,
                                               void* stream)
{
    EncoderCall c{grad, inputs, embeddings, offsets, resolutions, grad_embeddings, N, D, F, L, 0, nullptr, nullptr, nullptr,
                  nullptr, flags, ste_clip_count, nullptr, nullptr, nullptr, FeatLayout{grad_ld, grad_col},
                  (hipStream_t)stream};
    const int rc = validate(c, EncoderEntry::routed);
    return rc != CNC_OK || c.empty() ? rc : grid_encode_backward_binned(c, n_binned, level_rows, workspace, workspace_bytes);
}
