// grid_encode_merge.hip — backward scatter of the coarse levels with run merging across rays.
//
// k_grid_encode_bwd (grid_encode.hip) works on 256 consecutive samples per block: less than one ray of
// a marched frame (200-400 samples per ray), so the runs it merges are runs along ONE ray.  The rays of
// neighbouring pixels cross the same cells: of the runs in 1024 consecutive samples (3-4 rays) only 0.29
// (level 0) to 0.46 (resolution 214) open a cell no earlier run of the block visited; in 256 samples it is
// 0.93-0.96.  This kernel takes MB = 1024 (or 512) samples per block, finds the runs of equal cells through a
// small LDS hash table, lays the block's samples out by cell and sends ONE set of atomics per distinct cell (per
// CNC_MERGE_UNIT_CAP samples of it) — the coarse levels are bound by the
// memory-side atomic units (docs/engineering_log.md §4.2b), so the number of atomic instructions is what their time was
// made of.  Which 1024 samples a block takes: consecutive ones, or (levels of R >= kMergeTileMinRes, callers with scratch
// for the order) a depth slab of ~26 neighbouring rays, which merges as 4096 consecutive samples would: k_merge_tile_order.
//
// How it got here (9 coarse levels of the bench grid, ms per 2^20 marched samples; k_grid_encode_bwd: 0.523):
//   * first version, 8 stored weights per sample, block size 256 / 384 / 512 / 640 / 768 / 1024:
//     0.485 / 0.548 / 0.432 / 0.629 / 0.444 / 0.573 — more samples merge more, but the LDS they need
//     leaves fewer waves per CU;
//   * weights rebuilt from 4 floats per sample (half the LDS): 512 -> 0.426, 1024 -> 0.429; by then the
//     atomics were a sixth of the time (0.368 without them) and the per-sample loop was what was left
//     (a sample-minor LDS layout with 16-byte reads of 4 samples per lane was slower: 0.461);
//   * per-cell accumulation as an 8 x n by n x 8 product on v_mfma_f32_16x16x4_f32: 0.403;
//   * one packed LDS word per run and one 16-byte record per cell: 0.384;
//   * the cost now being per distinct cell, 1024 samples (75 KB of LDS, 2 blocks per CU): 0.365.
//   * the call's kernels compete for vector issue slots (profiles/r14_bin_pass_setup.md), and all lanes of a wave walk the
//     same chain: run records through readfirstlane (fields, lone-run split, step count and loop tests in scalar
//     registers: 31 -> 13 vector instructions per run pair outside the step loop), the per-wave prefixes as one 16-lane
//     DPP scan (two 16-term loops before), the valid-corner mask from six per-axis flags: 154.0 M -> 122.1 M vector
//     wave-instructions per call of the bench, 41 -> 32 vector registers, the bench frame +2.0 %
//     (profiles/r17_backward_issue_slots.md).
//   * a wave walked its cell's chain of run records two runs per MFMA step, a step of eight sample slots for runs of
//     one to three samples on the fine levels, 13 vector and 35 scalar instructions per pair around it, and one wave per
//     cell however long its chain.  Now every run takes its place in its cell with one LDS add, the samples' weights and
//     gradients are written to LDS at those places (they wait in registers until then), and a unit is a range of places:
//     ceil(n / 8) full steps in a counted loop, no records, no chain, units cut by arithmetic and handed to the waves
//     from a block-wide counter.  122.1 M -> 111.2 M vector and 97.5 M -> 60.9 M scalar wave-instructions per call of the
//     bench, the same 4.53 M atomic requests, the bench frame +3.5 % (profiles/r18_merge_wave_balance.md; balancing the
//     waves alone, over the chains as they were, was worth nothing next to the bin / owner passes).
//
// D = 3, F = 8 (one cell per wave at a time: 64 lanes = 8 corners x 8 features), no occupancy mask, no
// per-point level window: the coarse half of a binned backward call.  Everything else stays on
// k_grid_encode_bwd.  The cell key holds 16 bits per axis: the samples of a level of R > kCellKeyMaxRes
// (encoder_common.hpp) are left to k_grid_encode_bwd_wide, which scatters them one by one.
#include <cstdlib>

#include "common.hpp"
#include "encoder_common.hpp"

namespace cnc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// window and segment of the depth-ranked tiles of the 1024-sample blocks (k_merge_tile_order), in samples
#ifndef CNC_MERGE_TILE_WINDOW
#define CNC_MERGE_TILE_WINDOW 8192
#endif
#ifndef CNC_MERGE_TILE_SEGMENT
#define CNC_MERGE_TILE_SEGMENT 8
#endif
constexpr uint32_t kMergeTileWindow = CNC_MERGE_TILE_WINDOW, kMergeTileSegment = CNC_MERGE_TILE_SEGMENT;
// Levels below this resolution keep consecutive samples.  A tile of ~32 rays x 32 samples spans a handful of their
// cells: fewer cells than the block has waves, each of hundreds of samples.  When one wave walked a whole cell, ten copies
// of one level of the bench grid, middle chunk, took (ms, consecutive -> ranked, order from k_merge_tile_order): R = 18
// 0.224 -> 0.462, 24 0.216 -> 0.420, 32 0.227 -> 0.378, 44 0.253 -> 0.333, 60 0.340 -> 0.317, 82 0.376 -> 0.322,
// 113 0.458 -> 0.336, 155 0.619 -> 0.400, 214 0.859 -> 0.590, 296 1.190 -> 0.884.  With the samples laid out by cell
// (below) 32 and 0 were measured again: the call 1.0-2.9 % shorter on three chunks, the bench frame +0.6 % in every pair
// of runs, which is not enough for the project's keep rule (profiles/r18_merge_wave_balance.md).
#ifndef CNC_MERGE_TILE_MIN_RES
#define CNC_MERGE_TILE_MIN_RES 52
#endif
constexpr uint32_t kMergeTileMinRes = CNC_MERGE_TILE_MIN_RES;
// Most samples of one work unit of phase B.  A wave sums one unit at a time and takes the next from a block-wide
// counter, so a cell of hundreds of samples no longer keeps one wave busy while the others of the block, and the block's
// LDS, wait for it.  Every unit sends its own set of atomics: on the bench frame a cap of 32 adds 15-24 % of them and
// costs 4 % of the frame, 128 adds 10-60 % on the levels of R = 18 and 60, 512 adds none but 1.6 % on the first chunk's
// coarsest level (tools/merge_wave_load.py, profiles/r18_merge_wave_balance.md).
#ifndef CNC_MERGE_UNIT_CAP
#define CNC_MERGE_UNIT_CAP 512
#endif
constexpr uint32_t kMergeUnitCap = CNC_MERGE_UNIT_CAP;
static_assert(kMergeUnitCap >= 8 && kMergeUnitCap % 8 == 0, "whole steps of eight samples");

// Depth-ranked sample tiles.  Two samples of one ray never share a cell beyond one run: all merging beyond runs happens
// ACROSS rays, and 1024 consecutive samples are the full depth of only 3-4 rays.  So a block of the merge kernel need not
// take consecutive samples.  A window of TW consecutive samples is cut into TW / TS segments of TS consecutive samples,
// this kernel (one block per window, one segment per thread) orders the segments by depth along the rays, and each
// block of the window takes a slab of 1024 / TS of them: the same 1024 LDS slots hold a thin depth slab of ~26
// neighbouring rays, which merges as a 4,096-sample block would (0.57 of the distinct cells of the ten coarse levels on
// the bench frame's middle chunk), at the same LDS, block size and occupancy.  profiles/r10_merge_tiles.md.
//   * depth of a segment = its middle sample . axis; axis = the median-length one of three differences of neighbouring
//     samples of the window (a pair that straddles a ray boundary does not decide).  It only has to order depth.
//   * key = 22 bits of the depth in a monotonic integer form | segment index: a total order whatever the inputs are
//     (ties, a zero axis, NaN and points outside the cube: one sentinel, the index decides), so the tiling is a
//     permutation of the window's samples and a pure function of the inputs.  Segments past N rank last; they are
//     written like any other, and the merge kernel drops their samples because their indices are >= N.
//   * the window splits itself: the depths of consecutive segments fall once per ray boundary, so the descents count the
//     window's rays.  The best tile is about as many rays as samples per ray, i.e. a (sub-)window of ~32 ray lengths:
//     the window is cut into 1, 2, 4 ... TW / 1024 equal sub-windows, whichever is nearest, and ranked inside each.
//     With TW / 1024 sub-windows a block holds exactly the samples of the consecutive tiling.
//   * the order is a bitonic network on one key per thread (every merge ascending: first step against the mirrored
//     partner), shuffles inside a wave and double-buffered LDS words across waves, stopped at the sub-window size.
// order[window * TW / TS + i] = the segment (16 bits) at place i of the window's order.
template <uint32_t TW, uint32_t TS>
__global__ __launch_bounds__(1024) void k_merge_tile_order(const float* __restrict__ inputs, uint32_t N,
                                                           uint16_t* __restrict__ order)
{
    constexpr uint32_t MB = 1024;
    __shared__ uint32_t s_sort[2 * MB], s_cnt[MB / 64];
    const uint32_t base = blockIdx.x * TW;
    constexpr uint32_t kSegs = TW / TS, kTiles = TW / MB;
    constexpr uint32_t kPastEnd = 0x3FFFFFu, kUnusable = 0x3FFFFEu;
    static_assert(MB == 1024 && kSegs <= MB && kSegs * TS == TW && kTiles * MB == TW, "one segment per thread, 10 index bits");
    static_assert(TS >= 1 && TS <= 16 && (TS & (TS - 1)) == 0 && (kTiles & (kTiles - 1)) == 0 && kTiles <= 16,
                  "a tile is at least one wave of segments");
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n_in = min(N - base, TW), n_seg = div_up(n_in, TS);
    float ax[3] = {0.0f, 0.0f, 0.0f};
    if (n_in >= 2) {
        float cand[3][3], len[3];
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const size_t a = (size_t)base + min(k * 11u, n_in - 2);
#pragma unroll
            for (uint32_t d = 0; d < 3; d++) cand[k][d] = inputs[(a + 1) * 3 + d] - inputs[a * 3 + d];
            len[k] = (cand[k][0] * cand[k][0] + cand[k][1] * cand[k][1]) + cand[k][2] * cand[k][2];
        }
        const bool m0 = len[0] <= len[1] ? (len[1] > len[2] && len[0] > len[2]) : len[0] <= len[2];
        const bool m2 = len[0] <= len[1] ? (len[1] > len[2] && len[0] <= len[2]) : (len[0] > len[2] && len[1] <= len[2]);
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) ax[d] = m0 ? cand[0][d] : m2 ? cand[2][d] : cand[1][d];
    }
    uint32_t q = kPastEnd;
    if (tid < n_seg) {
        const size_t s = (size_t)base + min(tid * TS + TS / 2, n_in - 1);
        const float  x0 = inputs[s * 3], x1 = inputs[s * 3 + 1], x2 = inputs[s * 3 + 2];
        const float  dep = (x0 * ax[0] + x1 * ax[1]) + x2 * ax[2];
        const bool   usable = x0 >= 0 && x0 <= 1 && x1 >= 0 && x1 <= 1 && x2 >= 0 && x2 <= 1 && dep == dep;
        uint32_t     u = __float_as_uint(dep);
        u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;            // monotonic in the float's value
        q = usable ? min(u >> 10, kUnusable - 1) : kUnusable;
    }
    // rays of the window: descents of the depth in segment order (pairs across a wave boundary are not looked at)
    const uint32_t qp = (uint32_t)__shfl_up((int)q, 1);
    const uint64_t db = __ballot(lane != 0 && q < qp && qp < kUnusable);
    if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(db);
    uint32_t key = q << 10 | tid;
#pragma unroll
    for (uint32_t k = 2; k <= 64; k <<= 1) {
        uint32_t o = (uint32_t)__shfl_xor((int)key, (int)(k - 1));
        key = (lane & (k >> 1)) == 0 ? min(key, o) : max(key, o);
#pragma unroll
        for (uint32_t s = k >> 2; s >= 1; s >>= 1) {
            o = (uint32_t)__shfl_xor((int)key, (int)s);
            key = (lane & s) == 0 ? min(key, o) : max(key, o);
        }
    }
    __syncthreads();
    uint32_t n_rays = 1;
#pragma unroll
    for (uint32_t w = 0; w < MB / 64; w++) n_rays += s_cnt[w];
    // sub-windows: kSegs n_rays / (32 n_seg) of them would hold 32 ray lengths each; the nearest power of two
    const uint32_t have = n_rays * kSegs * 5u, want = n_seg * 32u * 7u;
    uint32_t       n_sub = have < want ? 1u : have < 2 * want ? 2u : have < 4 * want ? 4u : have < 8 * want ? 8u : 16u;
    n_sub = min(n_sub, kTiles);
    const uint32_t sub_segs = kSegs / n_sub;                   // >= MB / TS >= 64: block-uniform
    uint32_t p = 0;
    auto cross = [&](uint32_t mask, uint32_t bit) {
        s_sort[p * MB + tid] = key;
        __syncthreads();
        const uint32_t o = s_sort[p * MB + (tid ^ mask)];
        key = (tid & bit) == 0 ? min(key, o) : max(key, o);
        p ^= 1;                                                // (the next write must not meet this step's late readers)
    };
    for (uint32_t k = 128; k <= sub_segs; k <<= 1) {
        cross(k - 1, k >> 1);
        for (uint32_t s = k >> 2; s >= 64; s >>= 1) cross(s, s);
#pragma unroll
        for (uint32_t s = 32; s >= 1; s >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)key, (int)s);
            key = (lane & s) == 0 ? min(key, o) : max(key, o);
        }
    }
    if (tid < kSegs) order[(size_t)blockIdx.x * kSegs + tid] = (uint16_t)(key & (MB - 1));
}

// MB = samples (= threads) per block, a multiple of 64: 1024 for the frames of the bench (more samples per block merge
// more), 512 when the whole launch is only a few rounds of 1024-sample blocks — a training batch of 2^18 samples x 11
// levels is 2.8 k such blocks on 512 block slots, and ran 4x less efficiently than the 2^20-sample chunks.
// TW, TS: window and segment of the depth-ranked tiles (above), TW = 0: MB consecutive samples per block.
template <bool STE, uint32_t MB, uint32_t TW, uint32_t TS>
__global__ __launch_bounds__(MB) void k_grid_encode_bwd_merge(
    const float* __restrict__ grad, const float* __restrict__ inputs, const float* __restrict__ emb,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ resolutions,
    float* __restrict__ grad_emb, uint32_t N, const uint32_t* __restrict__ clip_count, FeatLayout lay,
    const uint16_t* __restrict__ tile_order)
{
    constexpr uint32_t kMB = MB;
    constexpr uint32_t kMW = kMB / 64;        // waves per block
    constexpr uint32_t kMSlots = kMB <= 512 ? 1024 : 2048;   // hash slots, power of two, >= 2 x the most runs a block can have
    constexpr uint32_t kCap = kMergeUnitCap;
    constexpr uint32_t D = 3, F = 8;
    static_assert(kMB <= 1024, "run records pack representative run / place in the cell / first thread, 10 bits each");
    // the three fractional positions and 1 / (sum of valid weights): the lane rebuilds its corner's
    // weight from them (same products, same order as Corners::setup) — half the LDS of 8 stored weights.
    // Both arrays are indexed by the sample's PLACE in the block's cell order (below), not by its thread.
    __shared__ __attribute__((aligned(16))) float s_w4[kMB][4];
    __shared__ float    s_g[kMB][F];
    // 16 bytes per thread, used twice: the sample keys (first half) and the hash table (second half)
    // until the runs are counted, then one record per unit {first place | end place << 16, key, validity}
    __shared__ __attribute__((aligned(16))) uint4 s_u[kMB];
    uint64_t* const s_key = reinterpret_cast<uint64_t*>(s_u);
    uint32_t* const h_slot = reinterpret_cast<uint32_t*>(s_u) + 2 * kMB;
    static_assert(kMSlots * 4 <= kMB * 8, "hash table fits the second half of s_u");
    __shared__ uint16_t s_run_start[kMB + 1];
    __shared__ uint32_t s_cell_n[kMB];          // per representative run of a cell: its samples so far, then its first place
    __shared__ uint32_t s_run_rec[kMB];         // representative run | place of the run in its cell << 10 | first thread << 20
    __shared__ uint32_t s_wave_heads[kMW];
    __shared__ uint32_t s_ctr[2];               // samples placed | units made << 16; the next unit phase B hands out

    // (the wave index through readfirstlane: the compiler cannot see that tid >> 6 is wave-uniform, and everything that
    // hangs on it — the prefix reads below, the unit loop of phase B — is scalar work once it can)
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool     mask_on = STE && (clip_count == nullptr || *clip_count != 0);
    // Exclusive prefix and total of one count per wave (s_wave_heads): lane l reads the word of wave
    // l % kMW, an inclusive scan inside the 16-lane row (four DPP row shifts that shift zeros in) and two readlanes at
    // wave-uniform lanes.  The counts of the waves in wave order, i.e. in sample order: runs keep their numbers.
    auto wave_prefix = [&](const uint32_t* counts, uint32_t& before, uint32_t& total) {
        static_assert(kMW == 8 || kMW == 16, "the counts of a block fit one DPP row");
        const uint32_t h = counts[lane & (kMW - 1)];
        uint32_t       x = h;
        x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);      // row_shr:1
        x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);      // row_shr:2
        x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);      // row_shr:4
        x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);      // row_shr:8
        before = (uint32_t)__builtin_amdgcn_readlane((int)(x - h), (int)wave);
        total = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)(kMW - 1));
    };
    // 1-D grid, level slot as the fast index (see k_grid_encode_bwd), slots walked last to first
    const uint32_t n_slots = lay.n_slots;
    const uint32_t chunk = blockIdx.x / n_slots;
    const uint32_t slot = n_slots - 1 - blockIdx.x % n_slots;
    uint32_t       b = chunk * kMB + tid;
    const uint32_t off = (uint32_t)offsets[slot];
    const uint32_t hs = (uint32_t)offsets[slot + 1] - off;
    const uint32_t R = (uint32_t)resolutions[slot];

    if constexpr (TW != 0) {
        // block = (window, tile, level slot): the order of the window's segments comes from k_merge_tile_order
        if (R >= kMergeTileMinRes) {
            constexpr uint32_t kTiles = TW / kMB, kSegs = TW / TS;
            const uint32_t win = chunk / kTiles, at = chunk % kTiles * (kMB / TS) + tid / TS;
            // (a segment past N, of the last window only, gives b >= N: no sample, as in a consecutive block's tail)
            b = win * TW + (uint32_t)tile_order[(size_t)win * kSegs + at] * TS + tid % TS;
        }
    }
    for (uint32_t i = tid; i < kMSlots; i += kMB) h_slot[i] = 0;
    s_cell_n[tid] = 0;
    if (tid < 2) s_ctr[tid] = tid == 0 ? 0u : kMW;         // (the first unit of a wave is its own number)

    // ---- phase A: lane = sample; weights and gradient stay in registers until the sample's place is known ----
    uint64_t key = ~0ull;
    uint32_t validmask = 0;
    float4   w4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float    g0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g1[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    {
        float    x[D];
        if (b < N && load_point<D>(inputs, b, x)) {
            Corners<D, false> c;
            c.setup(x, R, hs, 0, nullptr);
            key = (uint64_t)c.cell[0] | (uint64_t)c.cell[1] << 16 | (uint64_t)c.cell[2] << 32;
            if (R > kCellKeyMaxRes) key = ~0ull;               // cells the key cannot hold: k_grid_encode_bwd_wide
            // valid corners from the six per-axis border flags (a corner is valid iff none of its three coordinates
            // is 0 or R - 1: c.valid[i], without a select / shift / or per corner)
            {
                const uint32_t x1 = min(c.cell[0] + 1, R - 1), y1 = min(c.cell[1] + 1, R - 1), z1 = min(c.cell[2] + 1, R - 1);
                auto           border = [&](uint32_t q) { return (q == 0) | (q == R - 1); };
                const uint32_t inv = (border(c.cell[0]) ? 0x55u : 0u) | (border(x1) ? 0xAAu : 0u) | (border(c.cell[1]) ? 0x33u : 0u)
                    | (border(y1) ? 0xCCu : 0u) | (border(c.cell[2]) ? 0x0Fu : 0u) | (border(z1) ? 0xF0u : 0u);
                validmask = inv ^ 0xFFu;
            }
            w4 = make_float4(c.frac[0], c.frac[1], c.frac[2], c.wn_re);
            const float* gp = grad + feat_index(lay, slot, N, b, F);
            load_vec<4>(gp, g0);
            load_vec<4>(gp + 4, g1);
        }
        s_key[tid] = key;
    }
    __syncthreads();

    // ---- runs: consecutive samples with the same cell ----
    const bool     head = tid == 0 || s_key[tid - 1] != key;
    const uint64_t hb = __ballot(head);
    if (lane == 0) s_wave_heads[wave] = (uint32_t)__popcll(hb);
    __syncthreads();
    uint32_t before, total;
    wave_prefix(s_wave_heads, before, total);
    // the run of every thread, head or not: the heads up to and including its lane, after those of the earlier waves
    const uint32_t my_run = before + (uint32_t)__popcll(hb & ((2ull << lane) - 1ull)) - 1u;
    if (head) s_run_start[my_run] = (uint16_t)tid;
    if (tid == 0) s_run_start[total] = (uint16_t)kMB;
    __syncthreads();

    // ---- cells: every run takes its place among the samples of its cell ----
    // The run that claims the cell's hash slot represents the cell.  Every run of the cell, in whatever order they arrive,
    // adds its length to s_cell_n[representative]: what the add returns is where the run's samples start among the cell's.
    bool     claimer = false;
    if (head && key != ~0ull) {
        uint32_t sl = (((uint32_t)key ^ (uint32_t)(key >> 16) ^ (uint32_t)(key >> 32)) * 2654435761u) >> (32 - __builtin_ctz(kMSlots));
        uint32_t rep;
        for (;;) {
            const uint32_t seen = atomicCAS(&h_slot[sl], 0u, my_run + 1);
            if (seen == 0) { claimer = true; rep = my_run; break; }
            rep = seen - 1;
            if (s_key[s_run_start[rep]] == key) break;
            sl = (sl + 1) & (kMSlots - 1);
        }
        const uint32_t len = (uint32_t)s_run_start[my_run + 1] - tid;
        s_run_rec[my_run] = rep | atomicAdd(&s_cell_n[rep], len) << 10 | tid << 20;
    }
    __syncthreads();
    // ---- units: the cells laid out one after the other, each cut into units of at most kCap places ----
    // (the sync above also ends the life of the keys and the hash table: s_u is rewritten here)
    // A representative takes its cell's first place and its first unit record with ONE add on a packed counter (places in
    // the low half, records in the high half: a block has at most kMB of either, a unit holds at least one sample).
    if (claimer) {
        const uint32_t n = s_cell_n[my_run], units = (n + kCap - 1) / kCap;
        const uint32_t got = atomicAdd(&s_ctr[0], n | units << 16);
        const uint32_t first = got & 0xFFFFu, end = first + n;
        uint32_t       at = got >> 16;
        s_cell_n[my_run] = first;
        for (uint32_t p = first; p < end; p += kCap, at++)
            s_u[at] = make_uint4(p | min(p + kCap, end) << 16, (uint32_t)key, (uint32_t)(key >> 32), validmask);
    }
    __syncthreads();
    // ---- places: every sample moves to its cell's first place + its run's place in the cell + its place in the run ----
    if (key != ~0ull) {
        const uint32_t rr = s_run_rec[my_run];
        const uint32_t at = s_cell_n[rr & 0x3FFu] + ((rr >> 10) & 0x3FFu) + (tid - (rr >> 20));
        *reinterpret_cast<float4*>(s_w4[at]) = w4;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            s_g[at][j] = g0[j];
            s_g[at][4 + j] = g1[j];
        }
    }
    __syncthreads();
    const uint32_t n_units = __builtin_amdgcn_readfirstlane(s_ctr[0]) >> 16;

    // ---- phase B: lane = (corner, feature); a wave sums one unit at a time and takes the next from the block ----
    const uint32_t c = lane / F, f = lane % F;
    const uint32_t mi = lane & 15u, mk = lane >> 4;        // MFMA operand index (corner / feature of half A | B), sample slot
    const float    sx = (mi & 1u) ? 1.0f : -1.0f, ox = (mi & 1u) ? 0.0f : 1.0f;
    const float    sy = (mi & 2u) ? 1.0f : -1.0f, oy = (mi & 2u) ? 0.0f : 1.0f;
    const float    sz = (mi & 4u) ? 1.0f : -1.0f, oz = (mi & 4u) ? 0.0f : 1.0f;
    // my sample of a step's eight: 2 * slot + half, so that the eight gradient rows a step reads are 64 consecutive words
    const uint32_t mine = 2u * mk + ((mi >> 3) & 1u);
    auto flush = [&](uint32_t row, float v) {
        const size_t at = (size_t)row * F + f;
        if (mask_on) {
            const float e = emb[at];
            if (!(e >= -1.0f && e <= 1.0f)) return;
        }
        unsafeAtomicAdd(grad_emb + at, v);
    };
    // row of my corner in cell k (the arithmetic of Corners::setup, level geometry is block-uniform)
    uint32_t stride = 1, sd[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        sd[d] = stride;
        if (stride <= hs) stride *= R;
    }
    const bool hashed = stride > hs, pow2 = (hs & (hs - 1)) == 0;
    constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    // the cell is wave-uniform: both candidates per axis (cell, cell + 1 clamped; times the stride or the
    // hash prime) are scalar work, the lane only selects by its corner bits
    const bool cx = (c & 1u) != 0, cy = (c & 2u) != 0, cz = (c & 4u) != 0;
    const uint32_t m1 = hashed ? primes[1] : sd[1], m2 = hashed ? primes[2] : sd[2];
    auto row_of = [&](uint32_t k_lo, uint32_t k_hi) -> uint32_t {
        const uint32_t gx = k_lo & 0xFFFFu, gy = k_lo >> 16, gz = k_hi & 0xFFFFu;
        const uint32_t x0 = gx, x1 = min(gx + 1, R - 1);
        const uint32_t y0 = gy * m1, y1 = min(gy + 1, R - 1) * m1;
        const uint32_t z0 = gz * m2, z1 = min(gz + 1, R - 1) * m2;
        const uint32_t px = cx ? x1 : x0, py = cy ? y1 : y0, pz = cz ? z1 : z0;
        uint32_t index = hashed ? (px ^ py ^ pz) : (px + py + pz);
        if (pow2) index &= hs - 1;
        else if (index >= hs) index %= hs;
        return off + index;
    };

    // Rows two consecutive cells share (a ray leaving through a face) are NOT combined in registers here as
    // k_grid_encode_bwd does: with the cells merged across rays the atomics are no longer what the time is
    // made of, and the match (cell delta, partner lane, one more cross-lane read per cell) cost more issue
    // slots than the saved requests: 0.330 -> 0.305 ms for the 9 coarse levels, 1.091 -> 1.060 ms for the
    // whole backward call next to the bin / owner passes.
    for (uint32_t g = wave; g < n_units;) {
        const uint4 cell = s_u[g];                         // {first place | end place << 16, key, valid corners}
        // The unit is the wave's, not the lane's: its bounds and the cell go through readfirstlane, the step loop is a
        // counted scalar loop.
        const uint32_t span = __builtin_amdgcn_readfirstlane(cell.x);
        const uint32_t k_lo = __builtin_amdgcn_readfirstlane(cell.y);
        const uint32_t k_hi = __builtin_amdgcn_readfirstlane(cell.z);
        const uint32_t p_end = span >> 16;
        // S[corner][feature] = sum over the unit's samples of w[corner] * g[feature]: a K = n product of
        // an 8 x n and an n x 8 matrix on v_mfma_f32_16x16x4_f32.  Lane l feeds sample slot l / 16 with
        // operand index l % 16: its corner's weight (rebuilt from the 3 fractions — once per (corner, sample)
        // instead of once per (corner, feature, sample) as a lane-per-output loop would) and its feature's
        // gradient.  Eight samples per step: operand rows / columns 0..7 carry the even places, 8..15 the odd ones,
        // so the tile's two diagonal 8 x 8 blocks are two partial sums and every lane has work (the off-diagonal
        // cross terms are dropped).  The samples of a cell lie side by side whatever runs they came in: no run
        // records, no chain, ceil(n / 8) steps.
        f32x4 S = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t p = span & 0xFFFFu; p < p_end; p += 8) {
            const uint32_t ps = p + mine;
            float          a = 0.0f, bv = 0.0f;
            if (ps < p_end) {
                const float4 q = *reinterpret_cast<const float4*>(s_w4[ps]);
                // bit ? frac : 1 - frac, as one fma with (+1, 0) or (-1, 1): exact either way
                const float wx = __builtin_fmaf(q.x, sx, ox), wy = __builtin_fmaf(q.y, sy, oy),
                            wz = __builtin_fmaf(q.z, sz, oz);
                a = ((wx * wy) * wz) * q.w;
                bv = s_g[ps][mi & 7u];
            }
            S = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv, S, 0, 0, 0);
        }
        // the next unit: one lane asks the block's counter (before the epilogue, whose cross-lane reads wait on the same
        // LDS queue), the answer is the wave's through readfirstlane: the loop keeps its scalar control
        uint32_t taken = 0;
        if (lane == 0) taken = atomicAdd(&s_ctr[1], 1u);
        // tile element (row, col) sits in lane col + 16 * (row / 4), register row % 4; block B is 8 rows
        // and 8 columns further on = 40 lanes
        const int   src = (int)(f + 16u * (c >> 2));
        const float e0 = __shfl(S[0], src) + __shfl(S[0], src + 40), e1 = __shfl(S[1], src) + __shfl(S[1], src + 40),
                    e2 = __shfl(S[2], src) + __shfl(S[2], src + 40), e3 = __shfl(S[3], src) + __shfl(S[3], src + 40);
        if ((cell.w >> c) & 1u)
            flush(row_of(k_lo, k_hi), (c & 2u) ? ((c & 1u) ? e3 : e2) : ((c & 1u) ? e1 : e0));
        g = __builtin_amdgcn_readfirstlane(taken);
    }
}

// The levels of a merge call whose cells the 16-bit key fields cannot hold (R > kCellKeyMaxRes: k_grid_encode_bwd_merge
// gives their samples the key ~0 and leaves them alone): every sample goes out on its own.  A separate launch, so that
// the merge kernel's code stays what it was; its blocks leave at once on every other level.
template <bool STE>
__global__ __launch_bounds__(256) void k_grid_encode_bwd_wide(
    const float* __restrict__ grad, const float* __restrict__ inputs, const float* __restrict__ emb,
    const int32_t* __restrict__ offsets, const int32_t* __restrict__ resolutions,
    float* __restrict__ grad_emb, uint32_t N, const uint32_t* __restrict__ clip_count, FeatLayout lay)
{
    constexpr uint32_t D = 3, F = 8, C = 8;
    const uint32_t slot = blockIdx.y;
    const uint32_t R = (uint32_t)resolutions[slot];
    if (R <= kCellKeyMaxRes) return;
    const bool     mask_on = STE && (clip_count == nullptr || *clip_count != 0);
    const uint32_t off = (uint32_t)offsets[slot];
    const uint32_t hs = (uint32_t)offsets[slot + 1] - off;
    for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < N; b += gridDim.x * blockDim.x) {
        // (the corner set-up of Corners<D, false>, in a loop that is not unrolled: same cells, weights and validity)
        float x[D];
        if (load_point<D>(inputs, b, x)) {
            uint32_t cell[D];
            float    frac[D];
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                float p = x[d] * (float)(R - 2);
                p = p + 0.5f;
                const float fl = floorf(p);
                cell[d] = (uint32_t)fl;
                frac[d] = p - fl;
            }
            uint32_t valid = 0;
            float    wn = 0;
#pragma unroll 1
            for (uint32_t i = 0; i < C; i++) {
                float wi = 1;
                bool  border = false;
#pragma unroll
                for (uint32_t d = 0; d < D; d++) {
                    const bool     bit = (i >> d) & 1u;
                    const uint32_t q = bit ? min(cell[d] + 1, R - 1) : cell[d];
                    wi *= bit ? frac[d] : 1 - frac[d];
                    border |= (q == 0) | (q == R - 1);
                }
                valid |= (border ? 0u : 1u) << i;
                wn += border ? 0.0f : wi;
            }
            if (wn == 0) wn = 1e-9f;
            const float* gp = grad + feat_index(lay, slot, N, b, F);
            float        g[F];
            bool         nonzero = false;
#pragma unroll
            for (uint32_t k = 0; k < F; k++) {
                g[k] = gp[k];
                nonzero |= g[k] != 0.0f;
            }
            if (nonzero) scatter_point<D, F>(cell, frac, valid, 1.0f / wn, off, hs, R, g, emb, grad_emb, mask_on);
        }
    }
}

// scratch for the segment order of a call's windows (k_merge_tile_order), a multiple of 256 bytes
uint64_t merge_tile_order_bytes(uint32_t N)
{
    return ((uint64_t)div_up(N, kMergeTileWindow) * (kMergeTileWindow / kMergeTileSegment) * 2 + 255) / 256 * 256;
}

// grid_encode.hip launches this for the coarse half of a binned call (D = 3, F = 8)
void launch_bwd_merge(const EncoderCall& c)
{
    const uint32_t N = c.N, L = c.L;
    const bool     ste = c.ste();
    FeatLayout     lay = c.lay;
    lay.n_slots = L;
    // (round 3 measured this kernel with padded dynamic LDS — one block per CU, to leave room for the owner waves of
    // the binned levels: slower; the switch is gone, the library keeps no state between calls)
    const bool small = (uint64_t)div_up(N, 1024u) * L < 4096u;       // fewer than eight rounds of 1024-sample blocks
#define CNC_MERGE_GO(ST, MBS, W, S)                                                                                     \
    hipLaunchKernelGGL((k_grid_encode_bwd_merge<ST, MBS, W, S>), dim3(div_up(N, MBS) * L), dim3(MBS), 0, c.stream, c.grad, \
                       c.inputs, c.emb, c.offsets, c.resolutions, c.out, N, c.clip_count, lay, c.tile_order)
    if (small) {
        // training batches of unrelated short rays: consecutive samples
        if (ste) CNC_MERGE_GO(true, 512u, 0u, 0u);
        else CNC_MERGE_GO(false, 512u, 0u, 0u);
    } else if ((c.flags & CNC_FLAG_MERGE_CONSECUTIVE) || c.tile_order == nullptr) {
        // CNC_FLAG_MERGE_CONSECUTIVE (the tiling before the depth-ranked tiles, for comparisons inside one build), or a
        // caller without scratch for the segment order
        if (ste) CNC_MERGE_GO(true, 1024u, 0u, 0u);
        else CNC_MERGE_GO(false, 1024u, 0u, 0u);
    } else {
        // same grid: block id / L = window * (tiles per window) + tile, and a tile with a sample below N exists exactly
        // where a consecutive block does
        hipLaunchKernelGGL((k_merge_tile_order<kMergeTileWindow, kMergeTileSegment>), dim3(div_up(N, kMergeTileWindow)),
                           dim3(1024), 0, c.stream, c.inputs, N, c.tile_order);
        if (ste) CNC_MERGE_GO(true, 1024u, kMergeTileWindow, kMergeTileSegment);
        else CNC_MERGE_GO(false, 1024u, kMergeTileWindow, kMergeTileSegment);
    }
#undef CNC_MERGE_GO
    // (a few blocks per level slot: they leave at once unless the level is one of those, and the launch is all the call
    // pays for it.  On such a level the 4096 threads walk the samples grid-stride, 2^D F atomics each: slow for millions
    // of samples, but no encoder CNC builds has a level of R > 2^16, and the merge kernel keeps its speed)
    const dim3 wide(div_up(N, 256u) < 16u ? div_up(N, 256u) : 16u, L);
#define CNC_WIDE_GO(ST)                                                                                               \
    hipLaunchKernelGGL((k_grid_encode_bwd_wide<ST>), wide, dim3(256), 0, c.stream, c.grad, c.inputs, c.emb, c.offsets, \
                       c.resolutions, c.out, N, c.clip_count, lay)
    if (ste) CNC_WIDE_GO(true);
    else CNC_WIDE_GO(false);
#undef CNC_WIDE_GO
}

}  // namespace cnc
