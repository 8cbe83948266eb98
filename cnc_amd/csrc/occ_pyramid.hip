// occ_pyramid.hip — the kernels of the context-coded occupancy grid ("pyramid1"; C ABI in
// include/cnc_hip.h).  An extension: the reference only estimates the grid's size under one Bernoulli frequency.
//
// The grid is bytes [G, rx, ry, rz]; level k + 1 is the OR over the 2x2x2 blocks of level k.  A level's CANDIDATES are
// the eight children of every occupied parent, ordered by the parent's linear index (grid-major), then by octant
// o = ox << 2 | oy << 1 | oz: candidate 8 rank(parent) + o.  The rank is a prefix sum (count per 256 parents, one scan of
// the block sums), never an atomic counter, so the order — and the file — depends on the grid alone.  Everything here
// is integer work; the only floats are the +-1 symbols and the table look-up, which round nothing.
#include "common.hpp"

namespace cnc {
namespace {

constexpr uint32_t kRankBlock = 256;      // parents per rank block == threads of the count and emit kernels
constexpr uint32_t kScanThreads = 1024;

inline uint32_t rank_blocks(int64_t n_parents) { return (uint32_t)((n_parents + kRankBlock - 1) / kRankBlock); }

// ---------------------------------------------------------------------------------------------- reduce
struct ReduceArgs {
    const uint8_t* grid;
    uint8_t*       level[4];       // levels 1..4, NULL above `levels`
    int32_t        G, rx, ry, rz, levels;
    uint32_t       ntx, nty, ntz;
};

// One step of the tile's pyramid: dst (side D) from src (side 2 D), both in LDS; the tile's cells of the level that lie
// inside the grid also go to `out` (dims ox, oy, oz; the tile's origin at this level is (bx, by, bz) * D).
template <uint32_t D>
__device__ __forceinline__ void reduce_step(const uint8_t* src, uint8_t* dst, uint8_t* out, uint32_t g, uint32_t bx, uint32_t by,
                                            uint32_t bz, uint32_t ox, uint32_t oy, uint32_t oz)
{
    constexpr uint32_t S = 2 * D;
    for (uint32_t i = threadIdx.x; i < D * D * D; i += blockDim.x) {
        const uint32_t z = i % D, y = (i / D) % D, x = i / (D * D);
        uint32_t v = 0;
#pragma unroll
        for (uint32_t c = 0; c < 8; c++)
            v |= src[((2 * x + (c >> 2)) * S + 2 * y + ((c >> 1) & 1)) * S + 2 * z + (c & 1)];
        dst[i] = (uint8_t)v;
        const uint32_t X = bx * D + x, Y = by * D + y, Z = bz * D + z;
        if (out != nullptr && X < ox && Y < oy && Z < oz) out[(((size_t)g * ox + X) * oy + Y) * oz + Z] = (uint8_t)v;
    }
}

__global__ void __launch_bounds__(256) occ_reduce_kernel(ReduceArgs a)
{
    __shared__ uint8_t t0[4096], t1[512], t2[64], t3[8], t4[1];
    uint32_t b = blockIdx.x;
    const uint32_t bz = b % a.ntz; b /= a.ntz;
    const uint32_t by = b % a.nty; b /= a.nty;
    const uint32_t bx = b % a.ntx;
    const uint32_t g = b / a.ntx;
    const uint32_t rx = a.rx, ry = a.ry, rz = a.rz;
    for (uint32_t i = threadIdx.x; i < 4096; i += 256) {
        const uint32_t X = bx * 16 + (i >> 8), Y = by * 16 + ((i >> 4) & 15), Z = bz * 16 + (i & 15);
        uint8_t v = 0;
        if (X < rx && Y < ry && Z < rz) v = a.grid[(((size_t)g * rx + X) * ry + Y) * rz + Z] != 0;
        t0[i] = v;
    }
    __syncthreads();
    // the grid's sides are multiples of 2^levels, so a level-k cell inside the grid has all its children inside it
    reduce_step<8>(t0, t1, a.level[0], g, bx, by, bz, rx >> 1, ry >> 1, rz >> 1);
    __syncthreads();
    if (a.levels < 2) return;
    reduce_step<4>(t1, t2, a.level[1], g, bx, by, bz, rx >> 2, ry >> 2, rz >> 2);
    __syncthreads();
    if (a.levels < 3) return;
    reduce_step<2>(t2, t3, a.level[2], g, bx, by, bz, rx >> 3, ry >> 3, rz >> 3);
    __syncthreads();
    if (a.levels < 4) return;
    reduce_step<1>(t3, t4, a.level[3], g, bx, by, bz, rx >> 4, ry >> 4, rz >> 4);
}

// ---------------------------------------------------------------------------------------------- rank
__global__ void __launch_bounds__(256) occ_count_kernel(const uint8_t* __restrict__ parent, uint32_t n, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t w[4];
    const uint32_t i = blockIdx.x * kRankBlock + threadIdx.x;
    const bool occ = i < n && parent[i] != 0;
    const unsigned long long m = __ballot(occ);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = w[0] + w[1] + w[2] + w[3];
}

// One workgroup: counts[0, nb) -> exclusive offsets in place, counts[nb] = the total.  n_expected >= 0 (a decode): the
// header's candidate count, compared with 8 * total.
__global__ void __launch_bounds__(1024) occ_scan_kernel(uint32_t* counts, uint32_t nb, int64_t n_expected, uint32_t* status)
{
    __shared__ uint32_t s[kScanThreads];
    __shared__ uint32_t carry;
    const uint32_t t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += kScanThreads) {
        const uint32_t i = base + t;
        const uint32_t v = i < nb ? counts[i] : 0;
        s[t] = v;
        __syncthreads();
        for (uint32_t d = 1; d < kScanThreads; d <<= 1) {
            const uint32_t u = t >= d ? s[t - d] : 0;
            __syncthreads();
            s[t] += u;
            __syncthreads();
        }
        const uint32_t c = carry;
        if (i < nb) counts[i] = c + s[t] - v;
        __syncthreads();
        if (t == kScanThreads - 1) carry = c + s[t];
        __syncthreads();
    }
    if (t == 0) {
        counts[nb] = carry;
        if (n_expected >= 0 && status != nullptr && (int64_t)carry * 8 != n_expected) atomicOr(status, CNC_OCC_STATUS_COUNT);
    }
}

// ---------------------------------------------------------------------------------------------- emit
struct EmitArgs {
    const uint8_t*  parent;
    const uint8_t*  child;        // nullable (decode)
    const uint32_t* offsets;      // the rank's exclusive offsets per 256 parents
    int32_t         G, px, py, pz;
    uint32_t        n_par;
    int64_t         n_cap;
    int32_t*        idx;          // nullable
    uint8_t*        ctx;
    float*          sym;          // nullable
    uint32_t*       hist;         // nullable: [32][2] = (ones, total) per context
};

__device__ __forceinline__ uint32_t cell(const EmitArgs& a, uint32_t g, int32_t x, int32_t y, int32_t z)
{
    if ((uint32_t)x >= (uint32_t)a.px || (uint32_t)y >= (uint32_t)a.py || (uint32_t)z >= (uint32_t)a.pz) return 0;
    return a.parent[(((size_t)g * a.px + x) * a.py + y) * a.pz + z] != 0;
}

__global__ void __launch_bounds__(256) occ_emit_kernel(EmitArgs a)
{
    __shared__ uint32_t list[kRankBlock];
    __shared__ uint32_t wcnt[4];
    __shared__ uint32_t h[64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t i = blockIdx.x * kRankBlock + tid;
    const bool occ = i < a.n_par && a.parent[i] != 0;
    if (tid < 64) h[tid] = 0;
    const unsigned long long m = __ballot(occ);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, cnt = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; w++) {
        before += w < wave ? wcnt[w] : 0;
        cnt += wcnt[w];
    }
    if (occ) list[before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;
    __syncthreads();
    const int64_t first = 8 * (int64_t)a.offsets[blockIdx.x];
    const uint32_t ncand = 8 * cnt;
    for (uint32_t base = 0; base < ncand; base += kRankBlock) {       // the trip count is the block's: ballots below
        const uint32_t c = base + tid;
        const bool active = c < ncand;
        uint32_t cx = 0;
        bool one = false;
        if (active) {
            uint32_t P = list[c >> 3];
            const uint32_t o = c & 7;
            const int32_t z = (int32_t)(P % (uint32_t)a.pz); P /= (uint32_t)a.pz;
            const int32_t y = (int32_t)(P % (uint32_t)a.py); P /= (uint32_t)a.py;
            const int32_t x = (int32_t)(P % (uint32_t)a.px);
            const uint32_t g = P / (uint32_t)a.px;
            const int32_t ox = (o >> 2) & 1, oy = (o >> 1) & 1, oz = o & 1;
            const int32_t dx = 2 * ox - 1, dy = 2 * oy - 1, dz = 2 * oz - 1;
            const uint32_t near = cell(a, g, x + dx, y, z) + cell(a, g, x, y + dy, z) + cell(a, g, x, y, z + dz) +
                                  cell(a, g, x + dx, y + dy, z) + cell(a, g, x + dx, y, z + dz) + cell(a, g, x, y + dy, z + dz) +
                                  cell(a, g, x + dx, y + dy, z + dz);
            const uint32_t far = cell(a, g, x - dx, y, z) + cell(a, g, x, y - dy, z) + cell(a, g, x, y, z - dz);
            cx = near * 4 + far;
            const size_t ci = (((size_t)g * (2 * a.px) + (2 * x + ox)) * (2 * a.py) + (2 * y + oy)) * (2 * a.pz) + (2 * z + oz);
            if (a.child != nullptr) one = a.child[ci] != 0;
            const int64_t pos = first + c;
            if (pos < a.n_cap) {
                if (a.idx != nullptr) a.idx[pos] = (int32_t)ci;
                a.ctx[pos] = (uint8_t)cx;
                if (a.sym != nullptr) a.sym[pos] = one ? 1.0f : -1.0f;
            }
        }
        if (a.hist != nullptr) {
            // per wave: one ballot pair per context present among its lanes, then one LDS add by lane 0
            unsigned long long rem = __ballot(active);
            while (rem) {
                const uint32_t c0 = (uint32_t)__shfl((int)cx, __ffsll((long long)rem) - 1);
                const unsigned long long mm = __ballot(active && cx == c0);
                const unsigned long long m1 = __ballot(active && cx == c0 && one);
                if (lane == 0) {
                    atomicAdd(&h[2 * c0], (uint32_t)__popcll(m1));
                    atomicAdd(&h[2 * c0 + 1], (uint32_t)__popcll(mm));
                }
                rem &= ~mm;
            }
        }
    }
    if (a.hist != nullptr) {
        __syncthreads();
        if (tid < 64 && h[tid] != 0) atomicAdd(&a.hist[tid], h[tid]);      // integer: the sum has no order
    }
}

// ---------------------------------------------------------------------------------------------- probabilities, scatter
__global__ void __launch_bounds__(256) occ_probs_kernel(const uint8_t* __restrict__ ctx, int64_t n, const float* __restrict__ table,
                                                        float* __restrict__ p)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = table[ctx[i] & 31];
}

__global__ void __launch_bounds__(256) occ_scatter_kernel(const float* __restrict__ sym, const int32_t* __restrict__ idx, int64_t n_cap,
                                                          const uint32_t* __restrict__ total, uint8_t* __restrict__ child, int64_t n_child,
                                                          uint32_t* status)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t have = 8 * (int64_t)total[0];
    if (i >= (have < n_cap ? have : n_cap)) return;                      // the smaller of the header's and the grid's count
    const int64_t at = idx[i];
    if (at < 0 || at >= n_child) {
        if (status != nullptr) atomicOr(status, CNC_OCC_STATUS_INDEX);
        return;
    }
    if (sym[i] > 0.0f) child[at] = 1;
}

inline bool dims_ok(int32_t G, int32_t x, int32_t y, int32_t z, int64_t limit)
{
    if (G < 1 || x < 1 || y < 1 || z < 1) return false;
    const int64_t n = (int64_t)G * x;
    if (n > limit) return false;
    if (n * y > limit) return false;
    return n * y * z <= limit;
}

}  // namespace
}  // namespace cnc

extern "C" int cnc_occ_reduce(const uint8_t* grid, int32_t n_grids, int32_t rx, int32_t ry, int32_t rz, int32_t levels,
                              uint8_t* coarse, void* stream)
{
    using namespace cnc;
    if (!grid || !coarse || levels < 1 || levels > 4 || !dims_ok(n_grids, rx, ry, rz, 0x7fffffff)) return CNC_ERR_INVALID_VALUE;
    const int32_t mask = (1 << levels) - 1;
    if ((rx & mask) || (ry & mask) || (rz & mask)) return CNC_ERR_INVALID_VALUE;
    ReduceArgs a{};
    a.grid = grid;
    a.G = n_grids; a.rx = rx; a.ry = ry; a.rz = rz; a.levels = levels;
    uint8_t* at = coarse;
    for (int32_t k = 1; k <= levels; k++) {
        a.level[k - 1] = at;
        at += (size_t)n_grids * (rx >> k) * (ry >> k) * (rz >> k);
    }
    a.ntx = div_up(rx, 16); a.nty = div_up(ry, 16); a.ntz = div_up(rz, 16);
    const uint64_t blocks = (uint64_t)n_grids * a.ntx * a.nty * a.ntz;
    if (blocks > 0x7fffffffull) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(occ_reduce_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return launch_status();
}

extern "C" uint64_t cnc_occ_rank_scratch_bytes(int64_t n_parents)
{
    if (n_parents < 1 || n_parents > 0x7fffffff) return 0;
    return 4ull * (cnc::rank_blocks(n_parents) + 1ull);
}

extern "C" int cnc_occ_rank(const uint8_t* parent, int64_t n_parents, int64_t n_expected, void* scratch, uint64_t scratch_bytes,
                            uint32_t* status, void* stream)
{
    using namespace cnc;
    const uint64_t need = cnc_occ_rank_scratch_bytes(n_parents);
    if (!parent || need == 0 || !scratch || scratch_bytes < need || ((uintptr_t)scratch & 3)) return CNC_ERR_INVALID_VALUE;
    if (n_expected >= 0 && !status) return CNC_ERR_INVALID_VALUE;
    const uint32_t nb = rank_blocks(n_parents);
    uint32_t* counts = static_cast<uint32_t*>(scratch);
    hipLaunchKernelGGL(occ_count_kernel, dim3(nb), dim3(kRankBlock), 0, (hipStream_t)stream, parent, (uint32_t)n_parents, counts);
    if (launch_status() != CNC_OK) return CNC_ERR_LAUNCH;
    hipLaunchKernelGGL(occ_scan_kernel, dim3(1), dim3(kScanThreads), 0, (hipStream_t)stream, counts, nb, n_expected, status);
    return launch_status();
}

extern "C" int cnc_occ_emit(const uint8_t* parent, const uint8_t* child, int32_t n_grids, int32_t px, int32_t py, int32_t pz,
                            const void* rank_scratch, int64_t n_cap, int32_t* idx, uint8_t* ctx, float* sym, uint32_t* hist,
                            void* stream)
{
    using namespace cnc;
    // the CHILD level's linear indices are int32
    if (!parent || !rank_scratch || n_cap < 0 || !dims_ok(n_grids, px, py, pz, 0x7fffffff / 8)) return CNC_ERR_INVALID_VALUE;
    if (n_cap == 0) return CNC_OK;                 // a level without candidates: its (empty) buffers may be null
    if (!ctx) return CNC_ERR_INVALID_VALUE;
    EmitArgs a{};
    a.parent = parent; a.child = child; a.offsets = static_cast<const uint32_t*>(rank_scratch);
    a.G = n_grids; a.px = px; a.py = py; a.pz = pz;
    a.n_par = (uint32_t)((int64_t)n_grids * px * py * pz);
    a.n_cap = n_cap; a.idx = idx; a.ctx = ctx; a.sym = sym; a.hist = hist;
    hipLaunchKernelGGL(occ_emit_kernel, dim3(rank_blocks(a.n_par)), dim3(kRankBlock), 0, (hipStream_t)stream, a);
    return launch_status();
}

extern "C" int cnc_occ_probs(const uint8_t* ctx, int64_t n, const float* table, float* p, void* stream)
{
    if (n == 0) return CNC_OK;
    if (!ctx || !table || !p || n < 0 || n > 0x7fffffff) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(cnc::occ_probs_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctx, n, table, p);
    return cnc::launch_status();
}

extern "C" int cnc_occ_scatter(const float* sym, const int32_t* idx, int64_t n_cap, const void* rank_scratch, int64_t n_parents,
                               uint8_t* child, int64_t n_child, uint32_t* status, void* stream)
{
    using namespace cnc;
    if (n_cap == 0) return CNC_OK;
    if (!sym || !idx || !rank_scratch || !child || n_cap < 0 || n_cap > 0x7fffffff || n_child < 1 ||
        cnc_occ_rank_scratch_bytes(n_parents) == 0)
        return CNC_ERR_INVALID_VALUE;
    const uint32_t* total = static_cast<const uint32_t*>(rank_scratch) + rank_blocks(n_parents);
    hipLaunchKernelGGL(occ_scatter_kernel, dim3((uint32_t)((n_cap + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sym, idx, n_cap,
                       total, child, n_child, status);
    return launch_status();
}
