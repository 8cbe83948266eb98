// iso_surface.hip — the kernels of the mesh export (C ABI in include/cnc_hip.h).  An extension: the reference
// has no exporter.
//
// Marching tetrahedra over the Kuhn split of every cell of a float32 density lattice, (nx + 1)(ny + 1)(nz + 1) points, x
// fastest.  An edge belongs to its lower end (its OWNER) and has one of seven directions; a lattice point's byte says which
// of its seven edges carry a vertex, a cell's byte how many triangles it gives.  The caller scans both (exclusive prefix
// sums), and the two emit kernels write vertices and faces at the scanned offsets: no atomics, the order is the lattice's.
// One thread per lattice point / per cell, x fastest, so that the neighbour loads of adjacent threads fall on the same
// lines.  The (tetrahedron, mask) -> triangles table comes from the caller (cnc_amd/mesh.py tet_table()) as a device
// buffer of CNC_ISO_TABLE int8; only its codes' low six bits are used, so a bad table gives a wrong mesh and never an
// access outside.  Every write at a scanned offset is compared with the output's length first.
#include "common.hpp"

namespace cnc {
namespace {

constexpr uint32_t kRow = 7;          // int8 per (tetrahedron, mask): count, then 3 codes per triangle

struct Lattice {
    uint32_t nx, ny, nz;              // cells
    uint32_t px, py, pz;              // points
    uint32_t points;
};

struct Vec3 {
    float v[3];
};

inline bool lattice_ok(int32_t nx, int32_t ny, int32_t nz, Lattice& L)
{
    if (nx < 1 || ny < 1 || nz < 1) return false;
    const uint64_t points = ((uint64_t)nx + 1) * ((uint64_t)ny + 1);
    if (points > 0x7fffffffull || points * ((uint64_t)nz + 1) > 0x7fffffffull) return false;
    L.nx = (uint32_t)nx; L.ny = (uint32_t)ny; L.nz = (uint32_t)nz;
    L.px = L.nx + 1; L.py = L.ny + 1; L.pz = L.nz + 1;
    L.points = (uint32_t)(points * L.pz);
    return true;
}

inline uint32_t blocks256(uint64_t n) { return (uint32_t)((n + 255) / 256); }

__device__ __forceinline__ void split(const Lattice& L, uint32_t lin, uint32_t (&q)[3])
{
    q[0] = lin % L.px;
    const uint32_t r = lin / L.px;
    q[1] = r % L.py;
    q[2] = r / L.py;
}

__device__ __forceinline__ bool on_boundary(const Lattice& L, uint32_t x, uint32_t y, uint32_t z)
{
    return x == 0 || y == 0 || z == 0 || x == L.nx || y == L.ny || z == L.nz;
}

// corner c = dx | dy << 1 | dz << 2 of the cell whose corner 0 is point `lin`
__device__ __forceinline__ uint32_t corner_point(const Lattice& L, uint32_t lin, uint32_t c)
{
    return lin + (c & 1u) + ((c >> 1) & 1u) * L.px + (c >> 2) * L.px * L.py;
}

// direction k of the seven: 0 x, 1 y, 2 z, 3 xy, 4 yz, 5 xz, 6 xyz, as bits dx | dy << 1 | dz << 2
__device__ __forceinline__ uint32_t direction_bits(uint32_t k)
{
    return (0x7563421u >> (4 * k)) & 7u;
}

// ---------------------------------------------------------------------------------------------- occupancy skip
// active[lin] = 1 iff an occupancy cell that overlaps [p - h, p + h] is set.  Per axis, in integers: cell j of G overlaps
// the interval of point i of n cells iff j n <= (i + 1) G and (j + 1) n >= (i - 1) G (touching counts).
__device__ __forceinline__ void cell_range(uint32_t i, uint32_t n, uint32_t G, uint32_t& lo, uint32_t& hi)
{
    const uint64_t below = i == 0 ? 0 : (uint64_t)(i - 1) * G;
    const uint64_t first = (below + n - 1) / n;               // ceil
    lo = first == 0 ? 0 : (uint32_t)(first - 1);
    const uint64_t last = ((uint64_t)i + 1) * G / n;
    hi = last > G - 1 ? G - 1 : (uint32_t)last;
}

__global__ void __launch_bounds__(256) iso_active_kernel(const uint8_t* __restrict__ occ, uint32_t gx, uint32_t gy, uint32_t gz,
                                                         Lattice L, uint8_t* __restrict__ active)
{
    const uint32_t lin = blockIdx.x * 256 + threadIdx.x;
    if (lin >= L.points) return;
    uint32_t q[3], lo[3], hi[3];
    split(L, lin, q);
    cell_range(q[0], L.nx, gx, lo[0], hi[0]);
    cell_range(q[1], L.ny, gy, lo[1], hi[1]);
    cell_range(q[2], L.nz, gz, lo[2], hi[2]);
    uint32_t any = 0;
    for (uint32_t a = lo[0]; a <= hi[0]; a++)
        for (uint32_t b = lo[1]; b <= hi[1]; b++)
            for (uint32_t c = lo[2]; c <= hi[2]; c++) any |= occ[((size_t)a * gy + b) * gz + c];
    active[lin] = any ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------- positions
__global__ void __launch_bounds__(256) iso_positions_kernel(const int64_t* __restrict__ lin, int64_t first, uint32_t m, Lattice L,
                                                            Vec3 lo, Vec3 h, float* __restrict__ pos)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int64_t at = lin ? lin[i] : first + (int64_t)i;
    if (at < 0 || at >= (int64_t)L.points) at = 0;              // a bad list gives a wrong position, nothing else
    uint32_t q[3];
    split(L, (uint32_t)at, q);
#pragma unroll
    for (int a = 0; a < 3; a++) pos[(size_t)i * 3 + a] = lo.v[a] + (float)q[a] * h.v[a];
}

// ---------------------------------------------------------------------------------------------- classify
// A lane takes one lattice point: the point and its seven upper neighbours are the eight corners of the cell it is the
// corner of.  Capping is decided from the coordinates, never from what a neighbour's lane may already have stored, so the
// in-place store cannot race with the loads.
__global__ void __launch_bounds__(256) iso_classify_kernel(float* __restrict__ D, Lattice L, float threshold, uint32_t cap,
                                                           const int8_t* __restrict__ table, uint8_t* __restrict__ edge_mask,
                                                           uint8_t* __restrict__ cell_tris)
{
    const uint32_t lin = blockIdx.x * 256 + threadIdx.x;
    if (lin >= L.points) return;
    uint32_t q[3];
    split(L, lin, q);
    uint32_t inside = 0, present = 0;                           // bit c: corner c = dx | dy << 1 | dz << 2
#pragma unroll
    for (uint32_t c = 0; c < 8; c++) {
        const uint32_t x = q[0] + (c & 1u), y = q[1] + ((c >> 1) & 1u), z = q[2] + (c >> 2);
        if (x > L.nx || y > L.ny || z > L.nz) continue;
        present |= 1u << c;
        float d = 0.0f;
        if (!(cap && on_boundary(L, x, y, z))) d = D[corner_point(L, lin, c)];
        if (d >= threshold) inside |= 1u << c;                  // NaN is outside
    }
    if (cap && on_boundary(L, q[0], q[1], q[2])) D[lin] = 0.0f;
    uint32_t mask = 0;
    const uint32_t own = inside & 1u;
#pragma unroll
    for (uint32_t k = 0; k < 7; k++) {
        const uint32_t c = direction_bits(k);
        if (((present >> c) & 1u) && (((inside >> c) & 1u) != own)) mask |= 1u << k;
    }
    edge_mask[lin] = (uint8_t)mask;
    if (present == 0xffu) {
        uint32_t tris = 0;
#pragma unroll
        for (uint32_t t = 0; t < 6; t++) {
            const uint32_t c1 = 1u << (t >> 1);                                  // e_p1
            const uint32_t rest0 = (t >> 1) == 0 ? 1u : 0u, rest1 = (t >> 1) == 2 ? 1u : 2u;
            const uint32_t c2 = c1 | (1u << ((t & 1u) ? rest1 : rest0));        // e_p1 + e_p2
            const uint32_t m = (inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
            tris += (uint32_t)table[(t * 16 + m) * kRow] & 3u;
        }
        cell_tris[((size_t)q[2] * L.ny + q[1]) * L.nx + q[0]] = (uint8_t)tris;
    }
}

// ---------------------------------------------------------------------------------------------- vertices
// Gradient of D at a lattice point: central differences over 2 h, one-sided over h on the boundary.
__device__ __forceinline__ void gradient(const float* __restrict__ D, const Lattice& L, const uint32_t (&q)[3], uint32_t lin,
                                         const Vec3& h, float (&g)[3])
{
    const uint32_t n[3] = {L.nx, L.ny, L.nz};
    const uint32_t stride[3] = {1u, L.px, L.px * L.py};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (q[a] == 0) g[a] = (D[lin + stride[a]] - D[lin]) / h.v[a];
        else if (q[a] == n[a]) g[a] = (D[lin] - D[lin - stride[a]]) / h.v[a];
        else g[a] = (D[lin + stride[a]] - D[lin - stride[a]]) / (2.0f * h.v[a]);
    }
}

__global__ void __launch_bounds__(256) iso_vertices_kernel(const float* __restrict__ D, Lattice L, float threshold, Vec3 lo, Vec3 h,
                                                           const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ scan,
                                                           int64_t n_vertices, float* __restrict__ vertices, float* __restrict__ normals)
{
    const uint32_t lin = blockIdx.x * 256 + threadIdx.x;
    if (lin >= L.points) return;
    const uint32_t mask = edge_mask[lin] & 0x7fu;
    if (mask == 0) return;
    uint32_t q[3];
    split(L, lin, q);
    const float da = D[lin];
    float pa[3], ga[3];
#pragma unroll
    for (int a = 0; a < 3; a++) pa[a] = lo.v[a] + (float)q[a] * h.v[a];
    if (normals) gradient(D, L, q, lin, h, ga);
    int64_t at = (int64_t)scan[lin];
    for (uint32_t k = 0; k < 7; k++) {
        if (!((mask >> k) & 1u)) continue;
        const uint32_t c = direction_bits(k);
        const uint32_t qb[3] = {q[0] + (c & 1u), q[1] + ((c >> 1) & 1u), q[2] + (c >> 2)};
        const int64_t out = at++;
        if (qb[0] > L.nx || qb[1] > L.ny || qb[2] > L.nz || out < 0 || out >= n_vertices) continue;      // a mask that does not fit
        const uint32_t lb = corner_point(L, lin, c);
        const float db = D[lb];
        const float t = (threshold - da) / (db - da);
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float pb = lo.v[a] + (float)qb[a] * h.v[a];
            vertices[out * 3 + a] = pa[a] + t * (pb - pa[a]);
        }
        if (normals) {
            float gb[3], nv[3];
            gradient(D, L, qb, lb, h, gb);
#pragma unroll
            for (int a = 0; a < 3; a++) nv[a] = -(ga[a] + t * (gb[a] - ga[a]));
            // sqrtf: correctly rounded under the build's flags (hipcc's __fsqrt_rn is the native square root, 1 ulp)
            const float len = sqrtf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
            if (len != 0.0f) {
#pragma unroll
                for (int a = 0; a < 3; a++) nv[a] = nv[a] / len;
            }
#pragma unroll
            for (int a = 0; a < 3; a++) normals[out * 3 + a] = nv[a];
        }
    }
}

// ---------------------------------------------------------------------------------------------- faces
__global__ void __launch_bounds__(256) iso_faces_kernel(const float* __restrict__ D, Lattice L, float threshold,
                                                        const int8_t* __restrict__ table, const uint8_t* __restrict__ edge_mask,
                                                        const int32_t* __restrict__ vertex_scan, const uint8_t* __restrict__ cell_tris,
                                                        const int32_t* __restrict__ cell_scan, int64_t n_vertices, int64_t n_faces,
                                                        int32_t* __restrict__ faces)
{
    const uint32_t cell = blockIdx.x * 256 + threadIdx.x;
    if (cell >= L.nx * L.ny * L.nz) return;
    if (cell_tris[cell] == 0) return;
    const uint32_t x = cell % L.nx, r = cell / L.nx, y = r % L.ny, z = r / L.ny;
    const uint32_t lin = (z * L.py + y) * L.px + x;
    uint32_t inside = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; c++)
        if (D[corner_point(L, lin, c)] >= threshold) inside |= 1u << c;
    int64_t at = (int64_t)cell_scan[cell];
#pragma unroll
    for (uint32_t t = 0; t < 6; t++) {
        const uint32_t c1 = 1u << (t >> 1);
        const uint32_t rest0 = (t >> 1) == 0 ? 1u : 0u, rest1 = (t >> 1) == 2 ? 1u : 2u;
        const uint32_t c2 = c1 | (1u << ((t & 1u) ? rest1 : rest0));
        const uint32_t m = (inside & 1u) | (((inside >> c1) & 1u) << 1) | (((inside >> c2) & 1u) << 2) | (((inside >> 7) & 1u) << 3);
        const int8_t* row = table + (t * 16 + m) * kRow;
        const uint32_t count = (uint32_t)row[0] & 3u;
        for (uint32_t f = 0; f < count && f < 2; f++) {
            const int64_t out = at++;
            if (out < 0 || out >= n_faces) continue;
#pragma unroll
            for (uint32_t e = 0; e < 3; e++) {
                const uint32_t code = (uint32_t)row[1 + 3 * f + e] & 63u;
                const uint32_t owner = corner_point(L, lin, code >> 3), k = code & 7u;       // arithmetic: no indexed array
                const int64_t v = (int64_t)vertex_scan[owner] + __popc(edge_mask[owner] & ((1u << k) - 1u));
                faces[out * 3 + e] = v >= 0 && v < n_vertices ? (int32_t)v : 0;
            }
        }
    }
}

inline Vec3 vec3_of(const float* p)
{
    Vec3 v;
    for (int a = 0; a < 3; a++) v.v[a] = p[a];
    return v;
}

}  // namespace
}  // namespace cnc

extern "C" int cnc_iso_active_points(const uint8_t* occupancy, int32_t gx, int32_t gy, int32_t gz, int32_t nx, int32_t ny, int32_t nz,
                                     uint8_t* active, void* stream)
{
    using namespace cnc;
    Lattice L;
    if (!occupancy || !active || gx < 1 || gy < 1 || gz < 1 || (uint64_t)gx * (uint64_t)gy * (uint64_t)gz > 0x7fffffffull ||
        !lattice_ok(nx, ny, nz, L))
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(iso_active_kernel, dim3(blocks256(L.points)), dim3(256), 0, (hipStream_t)stream, occupancy, (uint32_t)gx,
                       (uint32_t)gy, (uint32_t)gz, L, active);
    return launch_status();
}

extern "C" int cnc_iso_lattice_positions(const int64_t* lin, int64_t first, int64_t m, int32_t nx, int32_t ny, int32_t nz,
                                         const float* lo, const float* h, float* positions, void* stream)
{
    using namespace cnc;
    Lattice L;
    if (!lattice_ok(nx, ny, nz, L) || m < 0 || m > 0x7fffffff || first < 0 || !lo || !h) return CNC_ERR_INVALID_VALUE;
    if (!lin && first + m > (int64_t)L.points) return CNC_ERR_INVALID_VALUE;
    if (m == 0) return CNC_OK;
    if (!positions) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(iso_positions_kernel, dim3(blocks256((uint64_t)m)), dim3(256), 0, (hipStream_t)stream, lin, first, (uint32_t)m, L,
                       vec3_of(lo), vec3_of(h), positions);
    return launch_status();
}

extern "C" int cnc_iso_classify(float* density, int32_t nx, int32_t ny, int32_t nz, float threshold, int32_t cap, const int8_t* table,
                                uint8_t* edge_mask, uint8_t* cell_tris, void* stream)
{
    using namespace cnc;
    Lattice L;
    if (!density || !table || !edge_mask || !cell_tris || !lattice_ok(nx, ny, nz, L) || !(threshold > 0.0f) || threshold > 3.4028235e38f)
        return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(iso_classify_kernel, dim3(blocks256(L.points)), dim3(256), 0, (hipStream_t)stream, density, L, threshold,
                       cap ? 1u : 0u, table, edge_mask, cell_tris);
    return launch_status();
}

extern "C" int cnc_iso_emit_vertices(const float* density, int32_t nx, int32_t ny, int32_t nz, float threshold, const float* lo,
                                     const float* h, const uint8_t* edge_mask, const int32_t* vertex_scan, int64_t n_vertices,
                                     float* vertices, float* normals, void* stream)
{
    using namespace cnc;
    Lattice L;
    if (!density || !lo || !h || !edge_mask || !vertex_scan || !lattice_ok(nx, ny, nz, L) || n_vertices < 0 || n_vertices > 0x7fffffff)
        return CNC_ERR_INVALID_VALUE;
    if (n_vertices == 0) return CNC_OK;
    if (!vertices) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(iso_vertices_kernel, dim3(blocks256(L.points)), dim3(256), 0, (hipStream_t)stream, density, L, threshold,
                       vec3_of(lo), vec3_of(h), edge_mask, vertex_scan, n_vertices, vertices, normals);
    return launch_status();
}

extern "C" int cnc_iso_emit_faces(const float* density, int32_t nx, int32_t ny, int32_t nz, float threshold, const int8_t* table,
                                  const uint8_t* edge_mask, const int32_t* vertex_scan, const uint8_t* cell_tris,
                                  const int32_t* cell_scan, int64_t n_vertices, int64_t n_faces, int32_t* faces, void* stream)
{
    using namespace cnc;
    Lattice L;
    if (!density || !table || !edge_mask || !vertex_scan || !cell_tris || !cell_scan || !lattice_ok(nx, ny, nz, L) || n_vertices < 0 ||
        n_vertices > 0x7fffffff || n_faces < 0 || 3 * n_faces > 0x7fffffff)
        return CNC_ERR_INVALID_VALUE;
    if (n_faces == 0) return CNC_OK;
    if (!faces) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(iso_faces_kernel, dim3(blocks256((uint64_t)L.nx * L.ny * L.nz)), dim3(256), 0, (hipStream_t)stream, density, L,
                       threshold, table, edge_mask, vertex_scan, cell_tris, cell_scan, n_vertices, n_faces, faces);
    return launch_status();
}
