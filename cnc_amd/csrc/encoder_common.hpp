// encoder_common.hpp — device code shared by the hash-grid encoder translation units:
// vector load/store helpers, the per-(point, level) corner set-up and the point loader; and, host side (at the end),
// the one descriptor of an encoder call with its validator, level ranges and the scratch split of the binned routes.
#pragma once

#include "common.hpp"

namespace cnc {

template <uint32_t V> struct vecf;
template <> struct vecf<1> { using type = float; };
template <> struct vecf<2> { using type = float2; };
template <> struct vecf<4> { using type = float4; };

template <uint32_t V>
__device__ __forceinline__ void load_vec(const float* __restrict__ p, float (&v)[V])
{
    using T = typename vecf<V>::type;
    T t = *reinterpret_cast<const T*>(p);
    const float* f = reinterpret_cast<const float*>(&t);
#pragma unroll
    for (uint32_t i = 0; i < V; i++) v[i] = f[i];
}

template <uint32_t V>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float (&v)[V])
{
    using T = typename vecf<V>::type;
    T t;
    float* f = reinterpret_cast<float*>(&t);
#pragma unroll
    for (uint32_t i = 0; i < V; i++) f[i] = v[i];
    *reinterpret_cast<T*>(p) = t;
}

// Streaming store: the line is not kept in the L2 (the encoder's output is read back much later by another kernel; the
// bit plane / table it gathers from should keep the cache).
template <uint32_t V>
__device__ __forceinline__ void store_vec_nt(float* __restrict__ p, const float (&v)[V])
{
    if constexpr (V == 4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        f4 t = {v[0], v[1], v[2], v[3]};
        __builtin_nontemporal_store(t, reinterpret_cast<f4*>(p));
    } else if constexpr (V == 2) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        f2 t = {v[0], v[1]};
        __builtin_nontemporal_store(t, reinterpret_cast<f2*>(p));
    } else {
        __builtin_nontemporal_store(v[0], p);
    }
}

// The merging backward kernels (k_grid_encode_bwd, k_grid_encode_bwd_merge, k_grid_encode_bwd_cells) key a cell by its
// integer coordinates, 16 bits per axis, and rebuild corner rows (coordinate + 1) or probe x-neighbours (key +- 1) from
// those fields.  Cell coordinates reach R - 2 and their +1 neighbours R - 1, so the key holds a level exactly when
// R <= kCellKeyMaxRes.  A point on a finer level joins no run or cell and is scattered on its own, one atomic per valid
// corner and feature (scatter_point): inside the run and the cell kernels, by k_grid_encode_bwd_wide after the merge
// kernel (whose own code measured 2 % slower on the bench with the branch in it).
constexpr uint32_t kCellKeyMaxRes = 1u << 16;

// Corner set-up for one (point, level): weights, validity and row indices.
// Mirrors gridencoder.cu:166-291 (forward) / :443-562 (backward).
template <uint32_t D, bool VXL>
struct Corners {
    static constexpr uint32_t C = 1u << D;
    float    w[C];
    uint32_t row[C];
    bool     valid[C];
    float    wn_re;
    uint32_t cell[D];     // integer cell coordinates (floor of the scaled position)
    float    frac[D];     // fractional position inside the cell

    __device__ __forceinline__ void setup(const float (&x)[D], uint32_t R, uint32_t hs,
                                          uint32_t Rb, const uint8_t* __restrict__ vxl,
                                          const int32_t* __restrict__ sat = nullptr,
                                          const uint32_t* __restrict__ vplane = nullptr)
    {
        float    pos[D];
        uint32_t g[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            float p = x[d] * (float)(R - 2);   // float*float, rounded
            p = p + 0.5f;                      // == (float)((double)p + 0.5)
            const float fl = floorf(p);
            g[d] = (uint32_t)fl;
            cell[d] = g[d];
            pos[d] = p - fl;
            frac[d] = pos[d];
        }
        // Row index per corner = grid_row(q, hs, R), assembled from per-axis terms: every axis has
        // only two candidate coordinates, so the 32-bit multiplies (quarter rate on CDNA) are done
        // once per axis and value (2 D of them) instead of once per corner and axis (D 2^D), and the
        // dense / hashed decision is made once (it is wave-uniform whenever the level is).
        constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u,
                                        2097192037u, 1434869437u, 2165219737u};
        uint32_t qa[D][2], part[D][2];
        uint32_t stride = 1, sd[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {                 // the stride walk of grid_row
            sd[d] = stride;
            if (stride <= hs) stride *= R;
        }
        const bool hashed = stride > hs;
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            qa[d][0] = g[d];
            qa[d][1] = min(g[d] + 1, R - 1);
            const uint32_t m = hashed ? primes[d] : sd[d];
#pragma unroll
            for (uint32_t b = 0; b < 2; b++) part[d][b] = d == 0 ? (hashed ? qa[d][b] : qa[d][b] * m) : qa[d][b] * m;
        }
        // dense vertex index per axis value for the vertex bit plane (x fastest: the two x-neighbours of a corner
        // pair share a word)
        uint32_t vpart[D][2];
        if constexpr (VXL) {
            uint32_t vs = 1;
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                vpart[d][0] = qa[d][0] * vs;
                vpart[d][1] = qa[d][1] * vs;
                vs *= R;
            }
        }
        const bool pow2 = (hs & (hs - 1)) == 0;
        float wn = 0;
#pragma unroll
        for (uint32_t i = 0; i < C; i++) {
            float    wi = 1;
            uint32_t q[D];
            uint32_t index = 0;
            bool     border = false;
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                const uint32_t bit = (i >> d) & 1u;
                wi *= bit ? pos[d] : 1 - pos[d];
                q[d] = qa[d][bit];
                index = hashed ? index ^ part[d][bit] : index + part[d][bit];
                border |= (q[d] == 0) | (q[d] == R - 1);
            }
            bool ok = !border;
            if constexpr (VXL) {
                // the reference evaluates the box for every corner; its result only matters
                // for non-border ones, so skip the (expensive) scan otherwise
                // (a level with a vertex bit plane — the same predicate evaluated once per vertex and occupancy
                // update — reads ONE bit here instead of 2^D table entries)
                if (ok) {
                    if (vplane) {
                        uint32_t vi = 0;
#pragma unroll
                        for (uint32_t d = 0; d < D; d++) vi += vpart[d][(i >> d) & 1u];
                        ok = (vplane[vi >> 5] >> (vi & 31u)) & 1u;
                    } else {
                        ok = sat ? box_any_sat<D>(q, R, Rb, sat) : box_any<D>(q, R, Rb, vxl);
                    }
                }
            }
            if (pow2) index &= hs - 1;
            else if (index >= hs) index %= hs;
            w[i] = wi;
            valid[i] = ok;
            row[i] = ok ? index : 0u;
            wn += ok ? wi : 0.0f;
        }
        if (wn == 0) wn = 1e-9f;   // (float)(0.0 + 1e-9)
        wn_re = 1.0f / wn;         // == (float)(1.0 / (double)wn)
    }
};

// Two cut-down forms of Corners<3, false>::setup for callers that need part of it and are bound by vector issue (the
// bin pass of grid_encode_binned.hip).  BIT-IDENTICAL to it in what they do return: the same float operations in the
// same order (the file is built with -ffp-contract=off), the same integer values.
//
// What a level fixes is worked out once (scalar registers): dense or hashed by the stride walk of grid_row, the
// multiplier of every axis (a stride or a prime; x always has 1), power-of-two rows or not.
// HP2 = true is the form for a level that is hashed into a power-of-two number of rows (`hashed_pow2()`, wave-uniform:
// the caller branches on it once, outside its loops): the multipliers are the primes as literals and a row is
// xor & (rows - 1), with no branch per corner.  HP2 = false handles every level — dense ones, other row counts — with
// the run-time decisions of Corners::setup, the modulo behind its wave-uniform test.
struct LevelGeom3 {
    uint32_t R, hs;
    uint32_t m[3];
    bool     hashed, pow2;

    __device__ __forceinline__ void init(uint32_t R_, uint32_t hs_)
    {
        constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
        R = R_;
        hs = hs_;
        uint32_t stride = 1, sd[3];
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) {
            sd[d] = stride;
            if (stride <= hs) stride *= R;
        }
        hashed = stride > hs;
        pow2 = (hs & (hs - 1)) == 0;
#pragma unroll
        for (uint32_t d = 0; d < 3; d++) m[d] = hashed ? primes[d] : sd[d];
    }

    __device__ __forceinline__ bool hashed_pow2() const { return hashed && pow2; }

    template <bool HP2>
    __device__ __forceinline__ uint32_t mul(uint32_t d) const
    {
        constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
        return HP2 ? primes[d] : m[d];
    }

    // one corner's row from its three per-axis parts, as Corners::setup finishes it
    template <bool HP2>
    __device__ __forceinline__ uint32_t fold(uint32_t px, uint32_t py, uint32_t pz) const
    {
        if constexpr (HP2) return (px ^ py ^ pz) & (hs - 1);
        uint32_t index = hashed ? px ^ py ^ pz : px + py + pz;
        if (pow2) index &= hs - 1;
        else if (index >= hs) index %= hs;
        return index;
    }

    // cell coordinate and fraction along one axis
    __device__ __forceinline__ uint32_t cell(float x, float& frac) const
    {
        float p = x * (float)(R - 2);
        p = p + 0.5f;
        const float fl = floorf(p);
        frac = p - fl;
        return (uint32_t)fl;
    }

    __device__ __forceinline__ bool border(uint32_t q) const { return (q == 0) | (q == R - 1); }
};

// Rows and validity of the eight corners, nothing else: no weight, no sum, no division.  Two 32-bit multiplies (y and
// z; x's multiplier is 1): the +1 neighbour's part is an add behind its axis' multiply, (g + 1) m == g m + m in
// uint32, and where the clamp min(g + 1, R - 1) bites (g + 1 > R - 1: no point of the unit box gets there, but the
// value stays Corners' for any input) the part is the wave-uniform (R - 1) m.
// Handed out pair by pair, fn(p, valid0, valid1, row0, row1) for p = 0 .. 3 (corners 2 p and 2 p + 1), and the flags
// kept in named scalars: an array of bool is an array of bytes to the compiler, which then keeps the flags in vector
// registers and combines them with 16-bit vector instructions instead of scalar lane-mask operations.
template <bool HP2, typename Fn>
__device__ __forceinline__ void corner_rows3(const float (&x)[3], const LevelGeom3& lv, Fn&& fn)
{
    float          frac;
    const uint32_t gx = lv.cell(x[0], frac), gy = lv.cell(x[1], frac), gz = lv.cell(x[2], frac);
    const uint32_t x1 = min(gx + 1, lv.R - 1), y1 = min(gy + 1, lv.R - 1), z1 = min(gz + 1, lv.R - 1);
    const bool     bx0 = lv.border(gx), bx1 = lv.border(x1);
    const bool     by0 = lv.border(gy), by1 = lv.border(y1);
    const bool     bz0 = lv.border(gz), bz1 = lv.border(z1);
    const uint32_t my = lv.mul<HP2>(1), mz = lv.mul<HP2>(2);
    const uint32_t py0 = gy * my, py1 = gy + 1 <= lv.R - 1 ? py0 + my : (lv.R - 1) * my;
    const uint32_t pz0 = gz * mz, pz1 = gz + 1 <= lv.R - 1 ? pz0 + mz : (lv.R - 1) * mz;
#pragma unroll
    for (uint32_t p = 0; p < 4; p++) {
        const bool     byz = ((p & 1u) ? by1 : by0) || ((p & 2u) ? bz1 : bz0);
        const uint32_t py = (p & 1u) ? py1 : py0, pz = (p & 2u) ? pz1 : pz0;
        const bool     v0 = !(bx0 || byz), v1 = !(bx1 || byz);
        fn(p, v0, v1, v0 ? lv.fold<HP2>(gx, py, pz) : 0u, v1 ? lv.fold<HP2>(x1, py, pz) : 0u);
    }
}

// Corner pair p (corners 2 p and 2 p + 1: the x-neighbours at y bit p & 1, z bit p >> 1) with everything an item of the
// bin pass carries: the pair's weights, rows and validity, and 1 / (sum of the valid weights of all eight corners).
// The eight weights are formed as Corners forms them, ((tx ty) tz), and summed over the valid corners in corner order;
// rows only for the pair (two multiplies, on the selected y and z coordinates).  p may be a run-time value.
struct CornerPair3 {
    float    w0, w1;
    uint32_t row0, row1;
    bool     valid0, valid1;
    float    wn_re;

    // 1 / (sum of the valid weights of all eight corners): a property of the sample, not of the pair.  The bin pass
    // computes it once per sample in its count phase and keeps it in LDS for the walk (k_bwd_bin_sorted).
    static __device__ __forceinline__ float normaliser(const float (&x)[3], const LevelGeom3& lv)
    {
        float          fx, fy, fz;
        const uint32_t gx = lv.cell(x[0], fx), gy = lv.cell(x[1], fy), gz = lv.cell(x[2], fz);
        const uint32_t x1 = min(gx + 1, lv.R - 1), y1 = min(gy + 1, lv.R - 1), z1 = min(gz + 1, lv.R - 1);
        const float    ex = 1 - fx, ey = 1 - fy, ez = 1 - fz;
        const bool     bx0 = lv.border(gx), bx1 = lv.border(x1);
        const bool     by0 = lv.border(gy), by1 = lv.border(y1);
        const bool     bz0 = lv.border(gz), bz1 = lv.border(z1);
        float          wn = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            float wi = 1;
            wi *= (i & 1u) ? fx : ex;
            wi *= (i & 2u) ? fy : ey;
            wi *= (i & 4u) ? fz : ez;
            const bool ok = !(((i & 1u) ? bx1 : bx0) || ((i & 2u) ? by1 : by0) || ((i & 4u) ? bz1 : bz0));
            wn += ok ? wi : 0.0f;
        }
        if (wn == 0) wn = 1e-9f;
        return 1.0f / wn;
    }

    // the pair alone, the normaliser handed in: two weights from the selected y and z factors (the same products, the
    // same bits as the eight of the sum), rows and validity of the pair
    template <bool HP2>
    __device__ __forceinline__ void setup_pair(const float (&x)[3], const LevelGeom3& lv, uint32_t p, float wn_re_)
    {
        float          fx, fy, fz;
        const uint32_t gx = lv.cell(x[0], fx), gy = lv.cell(x[1], fy), gz = lv.cell(x[2], fz);
        const uint32_t x1 = min(gx + 1, lv.R - 1), y1 = min(gy + 1, lv.R - 1), z1 = min(gz + 1, lv.R - 1);
        const float    ex = 1 - fx, ey = 1 - fy, ez = 1 - fz;
        const bool     bx0 = lv.border(gx), bx1 = lv.border(x1);
        wn_re = wn_re_;
        const bool  by = p & 1u, bz = p & 2u;
        const float ty = by ? fy : ey, tz = bz ? fz : ez;
        w0 = (ex * ty) * tz;
        w1 = (fx * ty) * tz;
        const uint32_t qy = by ? y1 : gy, qz = bz ? z1 : gz;
        const bool     byz = lv.border(qy) || lv.border(qz);     // (tested on the selected coordinates: no select of flags)
        const uint32_t py = qy * lv.mul<HP2>(1), pz = qz * lv.mul<HP2>(2);
        valid0 = !(bx0 || byz);
        valid1 = !(bx1 || byz);
        row0 = valid0 ? lv.fold<HP2>(gx, py, pz) : 0u;
        row1 = valid1 ? lv.fold<HP2>(x1, py, pz) : 0u;
    }

    template <bool HP2>
    __device__ __forceinline__ void setup(const float (&x)[3], const LevelGeom3& lv, uint32_t p)
    {
        setup_pair<HP2>(x, lv, p, normaliser(x, lv));
    }
};

// One point's gradient row g[0 .. F) scattered to the table rows of its valid corners (bit i of `valid`): the path of
// the points the merging kernels cannot key (kCellKeyMaxRes).  The STE mask (|param| <= 1) when mask_on.  Weights and
// rows are rebuilt corner by corner from the cell and the fractions with the arithmetic of Corners::setup and grid_row
// (the same values), in a loop that is not unrolled: the path is cold, and it stays small next to the kernels' own code.
// `g` indexes like an array: the lane's registers or its LDS row.
template <uint32_t D, uint32_t F, typename G>
__device__ __forceinline__ void scatter_point(const uint32_t (&cell)[D], const float (&frac)[D], uint32_t valid,
                                              float wn_re, uint32_t off, uint32_t hs, uint32_t R, const G& g,
                                              const float* __restrict__ emb, float* __restrict__ grad_emb, bool mask_on)
{
#pragma unroll 1
    for (uint32_t i = 0; i < (1u << D); i++) {
        if (!((valid >> i) & 1u)) continue;
        float    w = 1;
        uint32_t q[D];
#pragma unroll
        for (uint32_t d = 0; d < D; d++) {
            const bool bit = (i >> d) & 1u;
            w *= bit ? frac[d] : 1 - frac[d];
            q[d] = bit ? min(cell[d] + 1, R - 1) : cell[d];
        }
        const float  tw = w * wn_re;
        const size_t at = (size_t)(off + grid_row<D>(q, hs, R)) * F;
#pragma unroll
        for (uint32_t k = 0; k < F; k++) {
            if (mask_on && !(emb[at + k] >= -1.0f && emb[at + k] <= 1.0f)) continue;
            unsafeAtomicAdd(grad_emb + at + k, tw * g[k]);
        }
    }
}

// F sign bits of one table row from the bit plane cnc_pack_sign_bits writes (bit k of row r = table[r][k] >= 0)
template <uint32_t F>
__device__ __forceinline__ uint32_t load_row_bits(const uint8_t* __restrict__ bits, uint64_t row)
{
    if constexpr (F == 32) return *reinterpret_cast<const uint32_t*>(bits + row * 4);
    else if constexpr (F == 16) return *reinterpret_cast<const uint16_t*>(bits + row * 2);
    else if constexpr (F == 8) return bits[row];
    else {
        const uint64_t bit = row * F;
        return (bits[bit >> 3] >> (bit & 7)) & ((1u << F) - 1u);
    }
}

// One 16-byte record per unit, built by the caller from the encoders' level tables (cnc_fused_field_t.units): a lane
// needs ONE L1-resident load before it can form its corner rows.  Reading the level tables through the encoder array
// of the kernel arguments (a dynamically indexed pointer, then the table entry, then the sign bytes) put three
// dependent memory round trips in front of every unit.
struct UnitRec {
    uint32_t off, hs, R, enc;
};

// The same F features with the vector work cut down (566 -> ~370 instructions per 3-D unit; the kernel was 53 % vector
// issue, tools/pmc_field.sh), BIT-IDENTICAL to `unit_features` / k_grid_encode_fwd_bits on the units a GridEncoder makes:
//   * a level is either dense (R^D <= rows: index = q0 + q1 R + q2 R^2 < rows) or hashed into a power-of-two table
//     (index = xor of primes & (rows - 1)) — the host refuses anything else (`FusedFieldForward.supported`) — so every
//     index is in range by construction: no modulo, no per-corner branch around the gather (an invalid corner's byte
//     is read and multiplied by a zero weight), coordinates of an outside point are replaced by 0 first;
//   * per-axis work is shared by the corners: 2 D multiplies for the index parts, the D = 3 weights as four x-y
//     products times two z factors (same association (wx wy) wz), border tests per axis value;
//   * the sign goes into the weight with shift + v_bfi (the weight is non-negative) and is ADDED: fmaf(tw, +-1, acc)
//     is acc +- tw rounded once — the same value — at 3 instead of 4 instructions per (corner, feature).
// ... in two halves: everything up to the gathers (their results stay in flight in `u.rb`), then the weights' sum, the
// division and the features — so that a lane can have two units' gathers under way before it consumes either.
struct UnitFast {
    float    m[8];        // corner weight, 0 for a border corner or an outside point
    uint32_t rb[8];       // the corner rows' sign bits (bits 0 .. F-1)
    float    wn;          // sum of m in corner order
};

// Width in bytes of the aligned word that serves both x-neighbours of a corner pair on the paired path (PAIR = true
// below): 4, 8 or 16.  8 is what tools/gather_width_probe.hip and the per-level table favour
// (profiles/r13_forward_pair_gather.md).
#ifndef CNC_FWD_PAIR_BYTES
#define CNC_FWD_PAIR_BYTES 8
#endif

// Byte `at` (0 .. W-1) of a W-byte word held as W/4 dwords, in bits 0..7 of the result: one v_perm_b32 (W = 16: two
// selects first).  Bits 8..31 hold copies of the word's byte 0: the callers' consumers read bits 0..7 only.
template <uint32_t W>
__device__ __forceinline__ uint32_t pair_word_byte(const uint32_t (&w)[W / 4], uint32_t at)
{
    static_assert(W == 4 || W == 8 || W == 16, "one dword, dwordx2 or dwordx4 load");
    if constexpr (W == 4) return __builtin_amdgcn_perm(w[0], w[0], at);
    else if constexpr (W == 8) return __builtin_amdgcn_perm(w[1], w[0], at);
    else return __builtin_amdgcn_perm((at & 8u) ? w[3] : w[1], (at & 8u) ? w[2] : w[0], at & 7u);
}

// PAIR (F = 8, a hashed power-of-two level of hs >= W rows, off % W == 0, `bits` W-aligned: the caller checks, per
// wave): the gathers of the two x-neighbours of a corner pair become ONE aligned W-byte load where both bytes lie in
// the same word; see the comment at the loads.  PAIR = false is the instruction stream every other caller keeps.
template <uint32_t D, uint32_t F, bool PAIR = false>
__device__ __forceinline__ void unit_issue_fast(const float (&x_)[D], bool inside, const uint8_t* __restrict__ bits,
                                                const UnitRec& r, UnitFast& u)
{
    static_assert(D == 2 || D == 3, "planes and volumes");
    static_assert(!PAIR || F == 8, "the paired gathers take one byte per row");
    constexpr uint32_t C = 1u << D;
    float (&m)[8] = u.m;
    uint32_t (&rb)[8] = u.rb;
    const uint32_t R = r.R, hs = r.hs;
    // the stride walk of grid_row: hashed iff the level does not fit its table
    uint32_t stride = 1, sd[D];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        sd[d] = stride;
        if (stride <= hs) stride *= R;
    }
    const bool     hashed = stride > hs;
    const uint32_t mask = hashed ? hs - 1u : 0xFFFFFFFFu;
    constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
    uint32_t pa[D][2];
    float    wa[D][2];
    bool     ba[D][2];
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        const float xd = inside ? x_[d] : 0.0f;
        float p = xd * (float)(R - 2);
        p = p + 0.5f;
        const float    fl = floorf(p);
        const uint32_t g = (uint32_t)fl, q1 = min(g + 1u, R - 1u);
        wa[d][1] = p - fl;
        wa[d][0] = 1 - wa[d][1];
        ba[d][0] = (g == 0u) | (g == R - 1u);
        ba[d][1] = (q1 == 0u) | (q1 == R - 1u);
        if (d == 0) {
            pa[d][0] = g;
            pa[d][1] = q1;
        } else {
            // q1 = g + 1 here (x in [0, 1] puts g at R - 2 at most: the clamp never bites), so its part is one ADD behind
            // g's multiply — the same uint32 value as (g + 1) m — instead of a second quarter-rate v_mul_lo_u32
            const uint32_t m = hashed ? primes[d] : sd[d];
            pa[d][0] = g * m;
            pa[d][1] = pa[d][0] + m;
        }
    }
    float w01[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) w01[j] = wa[0][j & 1u] * wa[1][j >> 1];
    float    wn = 0;
    // (the level's first row goes into the 32-bit row, not into the pointer: with a wave-uniform `bits` the gathers are
    // scalar-base + 32-bit-offset loads — no 64-bit address pair per corner)
    uint32_t index[C];
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        const uint32_t b0 = i & 1u, b1 = (i >> 1) & 1u, b2 = D == 3 ? (i >> 2) & 1u : 0u;
        float    wi = w01[i & 3u];
        bool     border = ba[0][b0] | ba[1][b1];
        uint32_t ix = pa[0][b0] ^ pa[1][b1], ia = pa[0][b0] + pa[1][b1];
        if constexpr (D == 3) {
            wi = wi * wa[2][b2];
            border = border | ba[2][b2];
            ix ^= pa[2][b2];
            ia += pa[2][b2];
        }
        index[i] = (hashed ? ix : ia) & mask;
        m[i] = (!border && inside) ? wi : 0.0f;
        wn += m[i];
    }
    // One byte gather per corner, or (PAIR) one word per x-neighbour pair.  Round 5 served a pair with one 16-bit load
    // on EVERY level (adjacent bytes on a dense level, an aligned byte pair on a hashed one when the cell's x is even:
    // 50 %) while the kernel was bound by vector issue: level-major forward 0.218 -> 0.255 ms per 2^20 marched samples.
    // Since the sign table the hashed levels are bound by their gathers, and an aligned 8-byte word (7 cells of 8; a
    // wider load costs the address path nothing, tools/gather_width_probe.hip) measures, per level of the bench table:
    // R = 82 .. 563 faster (0.0113 .. 0.0158 -> 0.0106 .. 0.0145 ms, bound by L1 accesses, which fall 9.2 M -> 3.7 .. 5.6 M),
    // R = 778 .. 2049 SLOWER (bound by L2 -> L1 line fills: the i1 byte gather hit the line i0 had just fetched, so there
    // was nothing to save, and the paired path fetches 9 .. 37 % more lines).  Hence a per-level choice by the caller
    // (k_grid_encode_fwd_bits: kFwdPairMinRes / kFwdPairMaxRes); whole call 0.196 -> 0.180 ms in the bench
    // (profiles/r13_forward_pair_gather.md).
    if constexpr (PAIR) {
        // Hashed level, primes[0] == 1: the x-neighbours' rows are i0 = (g ^ h) & mask and i1 = ((g + 1) ^ h) & mask,
        // so i0 ^ i1 = (g ^ (g + 1)) & mask = 2^(t+1) - 1 with t the trailing one bits of g: both bytes lie in one
        // aligned W-byte word whenever that is < W (W = 8: g % 8 != 7, 7 lanes of 8) — tested on the indices
        // themselves, not on g, so it holds whatever q1 is.  The word starts at (off + i0) & ~(W - 1) >= off (off is a
        // multiple of W) and ends at or before off + hs (i0 < hs, hs a power of two >= W, hence a multiple of W): it
        // never leaves the level's plane.  The remaining lanes fetch their i1 bytes as before, in one branch for
        // all pairs.  pair_word_byte leaves junk above bit 7 of rb: unit_finish_fast shifts bit k < 8 up to bit 31 and
        // unit_finish_lut takes the two low nibbles, so nothing masks it off.
        constexpr uint32_t W = CNC_FWD_PAIR_BYTES;
        uint32_t word[C / 2][W / 4];
        bool     far = false;
#pragma unroll
        for (uint32_t p = 0; p < C / 2; p++) {
            const uint32_t a0 = r.off + index[2 * p];
            const uint8_t* at = bits + (a0 & ~(W - 1u));
            if constexpr (W == 4) word[p][0] = *reinterpret_cast<const uint32_t*>(at);
            else if constexpr (W == 8) {
                const uint2 v = *reinterpret_cast<const uint2*>(at);
                word[p][0] = v.x, word[p][1] = v.y;
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(at);
                word[p][0] = v.x, word[p][1] = v.y, word[p][2] = v.z, word[p][3] = v.w;
            }
            far = far | ((index[2 * p] ^ index[2 * p + 1]) >= W);
        }
        uint32_t lone[C / 2] = {};
        if (far) {
#pragma unroll
            for (uint32_t p = 0; p < C / 2; p++) lone[p] = bits[r.off + index[2 * p + 1]];
        }
#pragma unroll
        for (uint32_t p = 0; p < C / 2; p++) {
            rb[2 * p] = pair_word_byte<W>(word[p], (r.off + index[2 * p]) & (W - 1u));
            const uint32_t near = pair_word_byte<W>(word[p], (r.off + index[2 * p + 1]) & (W - 1u));
            rb[2 * p + 1] = far ? lone[p] : near;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < C; i++) rb[i] = load_row_bits<F>(bits, (uint64_t)(uint32_t)(r.off + index[i]));
    }
    u.wn = wn;
}

template <uint32_t D, uint32_t F>
__device__ __forceinline__ void unit_finish_fast(const UnitFast& u, float (&acc)[F])
{
    constexpr uint32_t C = 1u << D;
    float wn = u.wn;
    if (wn == 0) wn = 1e-9f;
    const float wn_re = 1.0f / wn;
#pragma unroll
    for (uint32_t k = 0; k < F; k++) acc[k] = 0;
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        const uint32_t tw = __builtin_bit_cast(uint32_t, u.m[i] * wn_re);        // >= +0
        const uint32_t nb = ~u.rb[i];                                            // bit k clear = feature +1
#pragma unroll
        for (uint32_t k = 0; k < F; k++) {
            // sign from bit k of nb, magnitude from tw: shift + v_bfi_b32 (the compiler's own choice for the C
            // expression is shift + and + or: VOP3 takes no literal on gfx9, so it will not form the bfi by itself)
            uint32_t sw;
            asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(sw) : "s"(0x80000000u), "v"(nb << (31u - k)), "v"(tw));
            acc[k] = acc[k] + __builtin_bit_cast(float, sw);
        }
    }
}

// The same sum with the signs from a table instead of shift + bfi per feature.  Entry n of the nibble table holds the
// four features of the sign nibble n as +-1.0f (bit j set: +1), 16 bytes per entry, 256 bytes in all: a corner's F
// signs are F/4 ds_read_b128, and two features at a time take one v_pk_fma_f32 with the weight in both halves.
// fmaf(tw, +-1, acc) is acc +- tw rounded once, the value the bfi form adds: BIT-IDENTICAL, same corner order.  The
// table's 16 entries are the 16 four-bank slots of one 256-byte bank row, so a ds_read_b128 lane group reads distinct
// slots or broadcasts: conflict-free whatever the patterns.  F = 4, 8, 16, 32 (a whole nibble per read).
#ifndef CNC_SIGN_LUT
#define CNC_SIGN_LUT 1          // 0: k_grid_encode_fwd_bits is built with unit_finish_fast alone
#endif

__device__ __forceinline__ float4 sign_nibble(uint32_t n)
{
    return make_float4((n & 1u) ? 1.0f : -1.0f, (n & 2u) ? 1.0f : -1.0f, (n & 4u) ? 1.0f : -1.0f,
                       (n & 8u) ? 1.0f : -1.0f);
}

// A workgroup's table: the first 16 lanes fill it; the caller puts a barrier between this and the first read.
__device__ __forceinline__ void fill_sign_lut(float4* lut)
{
    if (threadIdx.x < 16) lut[threadIdx.x] = sign_nibble(threadIdx.x);
}

template <uint32_t D, uint32_t F>
__device__ __forceinline__ void unit_finish_lut(const UnitFast& u, const float4* __restrict__ lut, float (&acc)[F])
{
    static_assert(F % 4 == 0, "whole nibbles");
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr uint32_t C = 1u << D;
    float wn = u.wn;
    if (wn == 0) wn = 1e-9f;
    const float wn_re = 1.0f / wn;
    f2 a[F / 2];
#pragma unroll
    for (uint32_t k = 0; k < F / 2; k++) a[k] = f2{0.0f, 0.0f};
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        const float tw = u.m[i] * wn_re;
        const f2    t2 = f2{tw, tw};
#pragma unroll
        for (uint32_t j = 0; j < F / 4; j++) {
            const float4 s = lut[(u.rb[i] >> (4 * j)) & 15u];
            a[2 * j] = __builtin_elementwise_fma(t2, f2{s.x, s.y}, a[2 * j]);
            a[2 * j + 1] = __builtin_elementwise_fma(t2, f2{s.z, s.w}, a[2 * j + 1]);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < F / 2; k++) {
        acc[2 * k] = a[k].x;
        acc[2 * k + 1] = a[k].y;
    }
}

template <uint32_t D, uint32_t F>
__device__ __forceinline__ void unit_features_fast(const float (&x)[D], bool inside, const uint8_t* __restrict__ bits,
                                                   const UnitRec& r, float (&acc)[F])
{
    UnitFast u;
    unit_issue_fast<D, F>(x, inside, bits, r, u);
    unit_finish_fast<D, F>(u, acc);
}

template <uint32_t D>
__device__ __forceinline__ bool load_point(const float* __restrict__ inputs, uint32_t b,
                                           float (&x)[D])
{
    bool oob = false;
#pragma unroll
    for (uint32_t d = 0; d < D; d++) {
        x[d] = inputs[(size_t)b * D + d];
        oob |= (x[d] < 0) | (x[d] > 1);
    }
    return !oob;
}

// ---------------------------------------------------------------------------------------------
// Host side: one encoder call between the C ABI and the launches.  Never a kernel parameter: the kernels take its
// members, or a struct built from it next to the kernel (CellsArgs, BinnedArgs).
// ---------------------------------------------------------------------------------------------
struct EncoderCall {
    // an entry point's raw arguments, in the order the backward entries list them
    const float*    grad;            // backward only
    const float*    inputs;
    const float*    emb;
    const int32_t*  offsets;
    const int32_t*  resolutions;
    float*          out;             // forward: outputs; backward: grad_embeddings
    uint32_t        N, D, F, L, Rb;
    const float*    dy_dx;           // backward only, with grad_inputs: both or neither
    float*          grad_inputs;
    const uint8_t*  vxl;
    const int32_t*  mli;
    uint32_t        flags;
    const uint32_t* clip_count;      // backward + STE only
    const int32_t*  sat;             // optional summed-volume table of the occupancy grid: kept only with vxl
    const uint32_t* vbits;           // optional vertex bit planes: attached to `lay` only with vxl and both pointers
    const int32_t*  vboff;
    FeatLayout      lay;             // {ld, col} where outputs (forward) / gradients (backward) live
    hipStream_t     stream;
    const uint8_t*  bits = nullptr;  // forward_bits: the table's sign bit plane, in the place of emb
    // scratch of merge_tile_order_bytes(N) a caller inside the library lends k_grid_encode_bwd_merge for the segment
    // order of its depth-ranked tiles (nullptr: consecutive samples)
    uint16_t*       tile_order = nullptr;

    bool empty() const { return N == 0 || L == 0; }
    bool ste() const { return (flags & CNC_FLAG_STE_BINARY) != 0; }
    // what kernel_input_backward and the binned passes take: where the gradients live, nothing else
    FeatLayout plain_layout() const { return FeatLayout{lay.ld, lay.col}; }
};

// forward: cnc_grid_encode_forward, _forward_bits.  backward: cnc_grid_encode_backward, whose layout
// grid_encode_backward_with_scratch checks (for the library's own sub-calls too).  routed: _backward_ordered, _binned,
// _overlapped, which have checks of their own in front of the layout's (they call layout_ok where they always did) and
// fix the order of the level slots themselves.
enum class EncoderEntry { forward, backward, routed };

// The checks the entry points share, in the order each of them makes them; completes the descriptor.  CNC_OK on an
// empty call too: `if (rc != CNC_OK || c.empty()) return rc;`
inline int validate(EncoderCall& c, EncoderEntry e)
{
    const bool bwd = e != EncoderEntry::forward;
    if (bwd && (c.dy_dx == nullptr) != (c.grad_inputs == nullptr)) return CNC_ERR_INVALID_VALUE;   // both or neither
    if (c.empty()) return CNC_OK;
    if ((bwd && !c.grad) || !c.inputs || !(c.emb || c.bits) || !c.offsets || !c.resolutions || !c.out)
        return CNC_ERR_INVALID_VALUE;
    if (!c.vxl) c.sat = nullptr;
    if (e == EncoderEntry::backward) c.lay.finest_first = (c.flags & CNC_FLAG_LEVELS_FINEST_FIRST) ? 1u : 0u;
    if (!bwd && !layout_ok(c.lay, c.F, c.L)) return CNC_ERR_INVALID_VALUE;
    if (c.vxl && c.vbits && c.vboff) { c.lay.vbits = c.vbits; c.lay.vboff = c.vboff; }
    return CNC_OK;
}

// Levels [first, first + count) of a call as a call of its own (the binned routes: no mask, no per-point level windows).
inline EncoderCall levels(const EncoderCall& c, uint32_t first, uint32_t count)
{
    EncoderCall s = c;
    s.offsets += first;
    s.resolutions += first;
    s.L = count;
    // level-major [L, N, F]: the levels start first * N * F floats in; point-major: first * F columns to the right
    if (c.lay.ld == 0) s.grad += (uint64_t)first * c.N * c.F;
    else s.lay.col += first * c.F;
    return s;
}

// The coarse half of a binned call: levels [0, count) on the atomic kernels, finest first.
inline EncoderCall coarse_levels(const EncoderCall& c, uint32_t count, uint16_t* tile_order)
{
    EncoderCall s = levels(c, 0, count);
    s.flags |= CNC_FLAG_LEVELS_FINEST_FIRST;
    s.lay.finest_first = 1;
    s.tile_order = tile_order;
    return s;
}

// Scratch of the binned routes: the bins first, the merge kernel's tile order (2 KB per window) in the aligned tail.
constexpr uint64_t kScratchAlign = 256;
inline uint64_t scratch_round_up(uint64_t v) { return (v + kScratchAlign - 1) / kScratchAlign * kScratchAlign; }

// Bytes a caller brings for both.  `groups` (the overlapped entry): two groups pad their shares to kScratchAlign; every
// split of the levels in two needs the same amount (a level's bytes do not depend on its group) and one group needs
// less, so this covers whatever split the call chooses; the serial fallback (small N, no coarse levels) needs the
// whole set of bins in one piece.
inline uint64_t scratch_bytes(uint32_t N, uint32_t n_binned, uint32_t level_rows, bool groups)
{
    uint64_t bins = cnc_grid_encode_backward_binned_workspace(N, n_binned, level_rows);
    if (groups && n_binned >= 2) {
        const uint64_t two = scratch_round_up(cnc_grid_encode_backward_binned_workspace(N, 1, level_rows))
                             + scratch_round_up(cnc_grid_encode_backward_binned_workspace(N, n_binned - 1, level_rows));
        if (two > bins) bins = two;
    }
    return scratch_round_up(bins) + merge_tile_order_bytes(N);
}

// The tile order's place in a workspace of that size or more, `bins_bytes` (in: the workspace's) cut down to what is
// in front of it; nullptr and all of it for the bins when the caller brought less.
inline uint16_t* split_scratch(uint32_t N, uint32_t n_binned, uint32_t level_rows, bool groups, void* workspace,
                               uint64_t& bins_bytes)
{
    if (!workspace || (uintptr_t)workspace % 16 != 0 || bins_bytes < scratch_bytes(N, n_binned, level_rows, groups))
        return nullptr;
    bins_bytes = (bins_bytes - merge_tile_order_bytes(N)) / kScratchAlign * kScratchAlign;
    return reinterpret_cast<uint16_t*>((char*)workspace + bins_bytes);
}

// The F ladder of the launchers: CALL with FF = F as a constant
#define CNC_F_SWITCH(F, CALL)                             \
    switch (F) {                                          \
    case 1: { constexpr uint32_t FF = 1; CALL; } break;   \
    case 2: { constexpr uint32_t FF = 2; CALL; } break;   \
    case 4: { constexpr uint32_t FF = 4; CALL; } break;   \
    case 8: { constexpr uint32_t FF = 8; CALL; } break;   \
    case 16: { constexpr uint32_t FF = 16; CALL; } break; \
    case 32: { constexpr uint32_t FF = 32; CALL; } break; \
    default: return CNC_ERR_INVALID_VALUE;                \
    }

// (grid_encode.hip's grid_encode_backward_with_scratch: common.hpp)
// grid_encode_cells.hip; false = not built for this shape (the caller keeps its own kernel)
bool launch_bwd_cells(const EncoderCall& c);
// grid_encode_merge.hip
void launch_bwd_merge(const EncoderCall& c);
// grid_encode_binned.hip: cnc_grid_encode_backward_binned on a checked call
int grid_encode_backward_binned(const EncoderCall& c, uint32_t n_binned, uint32_t level_rows, void* workspace,
                                uint64_t workspace_bytes);
// grid_input_grad.hip
int launch_dy_dx(const float* inputs, const float* emb, const int32_t* offsets, const int32_t* resolutions,
                 float* dy_dx, uint32_t N, uint32_t D, uint32_t F, uint32_t L, const int32_t* mli, bool ste,
                 hipStream_t s);
int launch_input_backward(const EncoderCall& c);

}  // namespace cnc
