// components.hip — connected-component labelling of a 3-D lattice and of a face list (C ABI in
// include/cnc_hip.h).  An extension: the reference has nothing like it.
//
// A label is the smallest linear index of a component, so the result does not depend on the algorithm or on the order in
// which anything runs.  Every kernel keeps one invariant on its label array L: L[x] <= x, and L[x] is a member of x's
// component ("a parent is smaller").  A root is an x with L[x] == x; following parents from any x ends at a root.
//
//   unite(a, b)   find both roots; hook the larger under the smaller with a 32-bit integer atomicMin on the larger's
//                 slot; if the slot had already been lowered by somebody else, go on with the value it held.  Every trip
//                 of the loop lowers a or b, which are bounded below by 0: the loop ends whatever the other waves do, and
//                 nothing here waits for another wave or workgroup.  The link an atomicMin overwrites is the value it
//                 returns, and the loop goes on uniting exactly that value: no union is lost.
//   find(x)       follow parents.  A stale read returns an EARLIER parent, which is still a member of the component and
//                 still <= x, so staleness (a CU's L1 is not refreshed by other CUs' writes) costs trips, never a result:
//                 what decides is the atomicMin, which is coherent.  The merge kernels read through agent-scope loads to
//                 keep the chains short.
//
// Grid: (1) a workgroup of 512 lanes labels one 8x8x8 tile in LDS (LDS atomics) and stores each set cell's tile-local
// root as a global index; (2) one lane per cell unites it with its set neighbours in OTHER tiles, on the global array;
// (3) one lane per cell replaces its label by its root.  Each is a launch of its own, so each sees the one before it
// complete.  No launch caps its grid: one lane per cell (or face, or vertex), below 2^31 of them.
#include "common.hpp"

namespace cnc {
namespace {

constexpr int32_t kTile = 8;
constexpr int32_t kTileCells = kTile * kTile * kTile;

struct Grid {
    int32_t n, d0, d1, d2;
    int32_t t0, t1, t2;               // tiles per axis
    int32_t cells;                    // per grid
    int32_t total;                    // n * cells
};

inline bool grid_ok(int32_t n, int32_t d0, int32_t d1, int32_t d2, Grid& G)
{
    if (n < 1 || d0 < 1 || d1 < 1 || d2 < 1) return false;
    const uint64_t plane = (uint64_t)d1 * (uint64_t)d2;
    if (plane > 0x7fffffffull || plane * (uint64_t)d0 > 0x7fffffffull || plane * (uint64_t)d0 * (uint64_t)n > 0x7fffffffull) return false;
    G.n = n; G.d0 = d0; G.d1 = d1; G.d2 = d2;
    G.t0 = (d0 + kTile - 1) / kTile; G.t1 = (d1 + kTile - 1) / kTile; G.t2 = (d2 + kTile - 1) / kTile;
    G.cells = (int32_t)(plane * (uint64_t)d0);
    G.total = G.cells * n;
    return true;
}

inline uint32_t blocks256(uint64_t n) { return (uint32_t)((n + 255) / 256); }

__device__ __forceinline__ int32_t load_label(const int32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x.  x is a valid index with L[x] >= 0; a value outside [0, x] (a damaged array) ends the walk.
__device__ __forceinline__ int32_t find_root(const int32_t* L, int32_t x)
{
    for (;;) {
        const int32_t p = load_label(L + x);
        if (p < 0 || p >= x) return x;
        x = p;
    }
}

__device__ __forceinline__ void unite(int32_t* L, int32_t a, int32_t b)
{
    for (;;) {
        a = find_root(L, a);
        b = find_root(L, b);
        if (a == b) return;
        if (a > b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(L + b, a);         // b > a
        if (old == b) return;                            // b was a root and now hangs under a
        b = old;                                         // b's parent as it was (0 <= old < b): unite that with a
        if (b < 0) return;                               // a damaged array
    }
}

// Forward half of the neighbourhood: code k = 14..26 of (o0 + 1) * 9 + (o1 + 1) * 3 + (o2 + 1), the offsets whose first
// non-zero component is +1; the other half is the same pairs seen from the other cell.
__device__ __forceinline__ bool forward_offset(int32_t k, int32_t connectivity, int32_t (&o)[3])
{
    o[0] = k / 9 - 1; o[1] = (k / 3) % 3 - 1; o[2] = k % 3 - 1;
    if (connectivity == 26) return true;
    if (connectivity == 6) return (o[0] != 0) + (o[1] != 0) + (o[2] != 0) == 1;
    return o[0] >= 0 && o[1] >= 0 && o[2] >= 0;          // 14: the seven Kuhn directions
}

// ---------------------------------------------------------------------------------------------- grid: tiles
__global__ void __launch_bounds__(kTileCells) components_tile_kernel(const uint8_t* __restrict__ mask, Grid G, int32_t connectivity,
                                                                     int32_t* __restrict__ labels)
{
    __shared__ int32_t L[kTileCells];
    const int32_t t = (int32_t)threadIdx.x;
    int32_t b = (int32_t)blockIdx.x;
    const int32_t b2 = b % G.t2; b /= G.t2;
    const int32_t b1 = b % G.t1; b /= G.t1;
    const int32_t b0 = b % G.t0;
    const int32_t g = b / G.t0;                          // < G.n: the grid is n * t0 * t1 * t2 blocks
    const int32_t l[3] = {t >> 6, (t >> 3) & 7, t & 7};
    const int32_t c[3] = {b0 * kTile + l[0], b1 * kTile + l[1], b2 * kTile + l[2]};
    const bool inside = c[0] < G.d0 && c[1] < G.d1 && c[2] < G.d2;
    const int32_t lin = inside ? (c[0] * G.d1 + c[1]) * G.d2 + c[2] : 0;
    const size_t base = (size_t)g * (size_t)G.cells;
    const bool set = inside && mask[base + lin] != 0;
    L[t] = set ? t : -1;
    __syncthreads();
    if (set) {
        for (int32_t k = 14; k < 27; k++) {
            int32_t o[3];
            if (!forward_offset(k, connectivity, o)) continue;
            const int32_t m[3] = {l[0] + o[0], l[1] + o[1], l[2] + o[2]};
            if (m[0] < 0 || m[0] >= kTile || m[1] < 0 || m[1] >= kTile || m[2] < 0 || m[2] >= kTile) continue;
            const int32_t u = (m[0] * kTile + m[1]) * kTile + m[2];
            if (load_label(L + u) >= 0) unite(L, t, u);
        }
    }
    __syncthreads();
    if (inside) {
        int32_t out = -1;
        if (set) {
            const int32_t r = find_root(L, t);           // tile-local order is the grid's order: r's cell is <= this one
            out = ((b0 * kTile + (r >> 6)) * G.d1 + b1 * kTile + ((r >> 3) & 7)) * G.d2 + b2 * kTile + (r & 7);
        }
        labels[base + lin] = out;
    }
}

// ---------------------------------------------------------------------------------------------- grid: seams
__global__ void __launch_bounds__(256) components_seam_kernel(Grid G, int32_t connectivity, int32_t* __restrict__ labels)
{
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= (uint32_t)G.total) return;
    const int32_t g = (int32_t)(at / (uint32_t)G.cells), lin = (int32_t)(at % (uint32_t)G.cells);
    int32_t* L = labels + (size_t)g * (size_t)G.cells;
    if (load_label(L + lin) < 0) return;
    const int32_t c[3] = {lin / (G.d1 * G.d2), (lin / G.d2) % G.d1, lin % G.d2};
    for (int32_t k = 14; k < 27; k++) {
        int32_t o[3];
        if (!forward_offset(k, connectivity, o)) continue;
        const int32_t m[3] = {c[0] + o[0], c[1] + o[1], c[2] + o[2]};
        if (m[0] < 0 || m[0] >= G.d0 || m[1] < 0 || m[1] >= G.d1 || m[2] < 0 || m[2] >= G.d2) continue;
        if ((m[0] >> 3) == (c[0] >> 3) && (m[1] >> 3) == (c[1] >> 3) && (m[2] >> 3) == (c[2] >> 3)) continue;   // same tile: done
        const int32_t u = (m[0] * G.d1 + m[1]) * G.d2 + m[2];
        if (load_label(L + u) >= 0) unite(L, lin, u);
    }
}

// ---------------------------------------------------------------------------------------------- flatten
// labels[x] <- the root above x, for every x of `n_grids` arrays of `cells` labels.  Concurrent stores replace a parent by
// an ancestor: a reader finds the same root through either.
__global__ void __launch_bounds__(256) components_flatten_kernel(int32_t* __restrict__ labels, uint32_t cells, uint32_t total)
{
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    if (at >= total) return;
    const uint32_t g = at / cells, x = at % cells;
    int32_t* L = labels + (size_t)g * (size_t)cells;
    if (load_label(L + x) < 0) return;
    const int32_t r = find_root(L, (int32_t)x);
    if (r != (int32_t)x) L[x] = r;
}

// ---------------------------------------------------------------------------------------------- sizes
// One integer atomicAdd per (wave, root) where the wave's lanes agree with its first valid lane — the rule inside a large
// component — and one per lane elsewhere.
__global__ void __launch_bounds__(256) components_sizes_kernel(const int32_t* __restrict__ labels, uint32_t cells, uint32_t total,
                                                               int32_t* __restrict__ sizes)
{
    const uint32_t at = blockIdx.x * 256u + threadIdx.x;
    int32_t slot = -1;                                                   // index into sizes, -1: nothing to count
    if (at < total) {
        const int32_t r = labels[at];
        if (r >= 0 && (uint32_t)r < cells) slot = (int32_t)((at / cells) * cells + (uint32_t)r);
    }
    const uint64_t valid = __ballot(slot >= 0);
    if (valid == 0) return;
    const int lead = __ffsll((unsigned long long)valid) - 1;
    const int32_t lead_slot = __shfl(slot, lead);
    const uint64_t same = __ballot(slot == lead_slot);
    if (slot < 0) return;
    if (slot == lead_slot) {
        if ((int)(threadIdx.x & 63u) == lead) atomicAdd(sizes + slot, (int32_t)__popcll((unsigned long long)same));
    } else {
        atomicAdd(sizes + slot, 1);
    }
}

// ---------------------------------------------------------------------------------------------- graph
__global__ void __launch_bounds__(256) components_iota_kernel(int32_t* __restrict__ labels, uint32_t n)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v < n) labels[v] = (int32_t)v;
}

__global__ void __launch_bounds__(256) components_faces_kernel(const int32_t* __restrict__ faces, uint32_t n_faces, int32_t n_vertices,
                                                               int32_t* __restrict__ labels)
{
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
    const bool oa = a >= 0 && a < n_vertices, ob = b >= 0 && b < n_vertices, oc = c >= 0 && c < n_vertices;    // a bad index joins nothing
    if (oa && ob) unite(labels, a, b);
    if (ob && oc) unite(labels, b, c);
    if (oa && oc && !ob) unite(labels, a, c);
}

}  // namespace
}  // namespace cnc

extern "C" int cnc_components_label_grid(const uint8_t* mask, int32_t n_grids, int32_t d0, int32_t d1, int32_t d2, int32_t connectivity,
                                         int32_t* labels, void* stream)
{
    using namespace cnc;
    Grid G;
    if (!mask || !labels || !grid_ok(n_grids, d0, d1, d2, G) || (connectivity != 6 && connectivity != 14 && connectivity != 26))
        return CNC_ERR_INVALID_VALUE;
    const uint64_t tiles = (uint64_t)G.n * (uint64_t)G.t0 * (uint64_t)G.t1 * (uint64_t)G.t2;          // <= total < 2^31
    hipLaunchKernelGGL(components_tile_kernel, dim3((uint32_t)tiles), dim3(kTileCells), 0, (hipStream_t)stream, mask, G, connectivity,
                       labels);
    if (tiles > (uint64_t)G.n)
        hipLaunchKernelGGL(components_seam_kernel, dim3(blocks256((uint64_t)G.total)), dim3(256), 0, (hipStream_t)stream, G, connectivity,
                           labels);
    hipLaunchKernelGGL(components_flatten_kernel, dim3(blocks256((uint64_t)G.total)), dim3(256), 0, (hipStream_t)stream, labels,
                       (uint32_t)G.cells, (uint32_t)G.total);
    return launch_status();
}

extern "C" int cnc_components_sizes(const int32_t* labels, int32_t n_grids, int32_t d0, int32_t d1, int32_t d2, int32_t* sizes, void* stream)
{
    using namespace cnc;
    Grid G;
    if (!labels || !sizes || !grid_ok(n_grids, d0, d1, d2, G)) return CNC_ERR_INVALID_VALUE;
    if (hipMemsetAsync(sizes, 0, (size_t)G.total * sizeof(int32_t), (hipStream_t)stream) != hipSuccess) return CNC_ERR_LAUNCH;
    hipLaunchKernelGGL(components_sizes_kernel, dim3(blocks256((uint64_t)G.total)), dim3(256), 0, (hipStream_t)stream, labels,
                       (uint32_t)G.cells, (uint32_t)G.total, sizes);
    return launch_status();
}

extern "C" int cnc_components_label_graph(const int32_t* faces, int64_t n_faces, int32_t n_vertices, int32_t* labels, void* stream)
{
    using namespace cnc;
    if (n_vertices < 0 || n_faces < 0 || 3 * n_faces > 0x7fffffff || (n_faces > 0 && !faces)) return CNC_ERR_INVALID_VALUE;
    if (n_vertices == 0) return CNC_OK;
    if (!labels) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(components_iota_kernel, dim3(blocks256((uint64_t)n_vertices)), dim3(256), 0, (hipStream_t)stream, labels,
                       (uint32_t)n_vertices);
    if (n_faces > 0) {
        hipLaunchKernelGGL(components_faces_kernel, dim3(blocks256((uint64_t)n_faces)), dim3(256), 0, (hipStream_t)stream, faces,
                           (uint32_t)n_faces, n_vertices, labels);
        hipLaunchKernelGGL(components_flatten_kernel, dim3(blocks256((uint64_t)n_vertices)), dim3(256), 0, (hipStream_t)stream, labels,
                           (uint32_t)n_vertices, (uint32_t)n_vertices);
    }
    return launch_status();
}
