// field_position_grad.hip — dL/dx of the radiance field's N samples, for gfx950.
//
//   k_field_position_grad<F>   (dX encoder columns, dS raw-coordinate + sinusoid columns) -> g_x [N, 3] in world units
//
// What it differentiates.  The first layer's input row of a sample is [3-D units | xy | xz | yz units (F columns each) |
// x (3) | sin(f_k x), cos(f_k x) (3 + 3 per frequency)], all of the unit-cube position x = (p - min) / (max - min).  For
// one (encoder, level) unit the forward (Corners::setup, encoder_common.hpp) forms, per axis d,
//     p_d = x_d (R - 2) + 0.5,  cell_d = floor(p_d),  t_d = p_d - cell_d                   (float32, nothing fused)
//     w_i = prod_d (bit_d(i) ? t_d : 1 - t_d),   V = the corners with no coordinate on the border ring (0 or R - 1)
//     wn  = sum_V w_i (1e-9 when that is 0),     y_c = sum_V w_i e_ic / wn,   e_ic = +-1 (the sign bit plane)
// and this kernel recomputes exactly that set-up — the same device function, so cell and fraction are the forward's
// bits — and takes its derivative, the normaliser's included:
//     d y_c / d x_a = (R - 2) sum_V d_a w_i (e_ic - y_c) / wn,      d_a w_i = +- prod_{d != a} (bit_d(i) ? t_d : 1 - t_d)
// which is 0 where wn was replaced (V is empty) and the plain tri-/bilinear derivative where every corner is valid.
// With the unit's F gradient columns g_c the contribution to g_unit[a] is regrouped per corner,
//     (R - 2) / wn  sum_V d_a w_i (s_i - T),      s_i = sum_c g_c e_ic,   T = sum_c g_c y_c = sum_V w_i s_i / wn,
// 2^D F sign-flipped adds instead of 2^D F D products.  The tail adds dS[a] (the raw coordinate's column) and, per
// frequency f, f (cos(x_a f) dS_sin - sin(x_a f) dS_cos) with the argument x_a f formed in float32 as the forward
// forms it.  g_world[a] = g_unit[a] / (max_a - min_a).  The view direction's path is not differentiated.
//
// Work split.  Four lanes per sample: lane j of a sample's quad takes the units u = j, j + 4, ... and the frequencies
// k = j, j + 4, ..., so that the quad reads 4 F consecutive floats of the sample's dX row per round (one 128-byte line
// at F = 8) and a sample's 24 units' gathers are in flight on four lanes instead of queued on one.  The four partial
// sums meet in a fixed tree, (lane 0 + lane 1) + (lane 2 + lane 3), by two xor-shuffles inside the quad: the order is a
// function of the lane index alone.  No atomics; every element of g_x is written exactly once, by a plain store of
// the quad's lane 0; a row whose selector is 0 (or whose position is outside the box) gets +0.
//
// Nothing is stored by the forward for this: the corner rows and sign bytes are gathered again (one bit per table
// entry, through load_row_bits as the bit-plane forward does).  Built with contraction off like the whole library.
#include "encoder_common.hpp"
#include "field_common.hpp"

namespace cnc {

struct PositionGradArgs {
    const float*   pos;          // [N, 3] world
    const float*   aabb;         // 6 floats
    const uint8_t* selector;     // [>= N]
    const float*   dX;           // [>= N, ld_x]
    const float*   dS;           // [>= N, ld_s] or nullptr
    const float*   freqs;
    const uint4*   units;        // {first row, rows, resolution, encoder} per unit
    const uint8_t* bits[4];
    float*         g_x;          // [N, 3]
    uint32_t       N, ld_x, ld_s, n_units, n_freqs;
};

// One unit's contribution to the gradient of ITS D coordinates (unit-cube units); `grow`: the unit's F columns of dX.
template <uint32_t D, uint32_t F>
__device__ __forceinline__ void unit_position_grad(const float (&x)[D], const uint8_t* __restrict__ bits, const UnitRec& r,
                                                   const float* __restrict__ grow, float (&g)[D])
{
    constexpr uint32_t C = 1u << D;
    constexpr uint32_t V = F < 4 ? F : 4;
    Corners<D, false> c;
    c.setup(x, r.R, r.hs, 128u, nullptr);
    uint32_t rb[C];
#pragma unroll
    for (uint32_t i = 0; i < C; i++) rb[i] = load_row_bits<F>(bits, (uint64_t)r.off + c.row[i]);     // an invalid corner reads row 0
    float gc[F];
#pragma unroll
    for (uint32_t k = 0; k < F; k += V) {
        float v[V];
        load_vec<V>(grow + k, v);
#pragma unroll
        for (uint32_t j = 0; j < V; j++) gc[k + j] = v[j];
    }
    // s_i = sum_c g_c e_ic, in column order;  T = (sum_V w_i s_i) / wn, in corner order
    float s[C], T = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        float a = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < F; k++) a = a + (((rb[i] >> k) & 1u) ? gc[k] : -gc[k]);
        s[i] = a;
        T = T + (c.valid[i] ? c.w[i] * a : 0.0f);
    }
    T = T * c.wn_re;
    const float scale = (float)(r.R - 2) * c.wn_re;
#pragma unroll
    for (uint32_t a = 0; a < D; a++) {
        float acc = 0.0f;
#pragma unroll
        for (uint32_t i = 0; i < C; i++) {
            float dw = ((i >> a) & 1u) ? 1.0f : -1.0f;
#pragma unroll
            for (uint32_t d = 0; d < D; d++) {
                if (d == a) continue;
                dw = dw * (((i >> d) & 1u) ? c.frac[d] : 1 - c.frac[d]);
            }
            acc = acc + (c.valid[i] ? dw * (s[i] - T) : 0.0f);
        }
        g[a] = acc * scale;
    }
}

template <uint32_t F>
__global__ __launch_bounds__(256) void k_field_position_grad(const PositionGradArgs p)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = t >> 2, j = t & 3u;
    const bool     row = i < p.N;                     // the whole quad agrees
    float amin[3], aext[3], x[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        amin[a] = p.aabb[a];
        aext[a] = p.aabb[3 + a] - p.aabb[a];
    }
    bool live = false;
    if (row) live = field_unit_position(p.pos + (size_t)i * 3, amin, aext, false, x) && p.selector[i] != 0;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        // every coordinate is in (0, 1): cells reach R - 2 at most and every corner row lies in its level's table
        const float* grow = p.dX + (size_t)i * p.ld_x;
        for (uint32_t u = j; u < p.n_units; u += 4) {
            const uint4   v = p.units[u];
            const UnitRec rec{v.x, v.y, v.z, v.w};
            if (rec.enc == 0) {
                float gu[3];
                unit_position_grad<3, F>(x, p.bits[0], rec, grow + u * F, gu);
                g[0] = g[0] + gu[0];
                g[1] = g[1] + gu[1];
                g[2] = g[2] + gu[2];
            } else {
                const uint32_t pl = rec.enc - 1;                                  // plane 0 = xy, 1 = xz, 2 = yz
                const float    x2[2] = {pl == 2 ? x[1] : x[0], pl == 0 ? x[1] : x[2]};
                const uint8_t* b = pl == 0 ? p.bits[1] : (pl == 1 ? p.bits[2] : p.bits[3]);
                float gu[2];
                unit_position_grad<2, F>(x2, b, rec, grow + u * F, gu);
                if (pl == 0) { g[0] = g[0] + gu[0]; g[1] = g[1] + gu[1]; }
                else if (pl == 1) { g[0] = g[0] + gu[0]; g[2] = g[2] + gu[1]; }
                else { g[1] = g[1] + gu[0]; g[2] = g[2] + gu[1]; }
            }
        }
        if (p.dS) {
            const float* srow = p.dS + (size_t)i * p.ld_s;
            if (j == 0) {
#pragma unroll
                for (int a = 0; a < 3; a++) g[a] = g[a] + srow[a];
            }
            for (uint32_t k = j; k < p.n_freqs; k += 4) {
                const float f = p.freqs[k];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    float sn, cs;
                    sincosf(x[a] * f, &sn, &cs);
                    g[a] = g[a] + f * (cs * srow[3 + 6 * k + a] - sn * srow[6 + 6 * k + a]);
                }
            }
        }
    }
    // (lane 0 + lane 1) + (lane 2 + lane 3): every lane of the wave takes part, rows past N carry zeros
#pragma unroll
    for (int a = 0; a < 3; a++) {
        g[a] = g[a] + __shfl_xor(g[a], 1);
        g[a] = g[a] + __shfl_xor(g[a], 2);
    }
    if (row && j == 0) {
        float* o = p.g_x + (size_t)i * 3;
#pragma unroll
        for (int a = 0; a < 3; a++) o[a] = live ? g[a] / aext[a] : 0.0f;
    }
}

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_field_position_grad(const cnc_fused_field_t* field, const float* positions, const uint8_t* selector,
                                       const float* dX, uint32_t ld_x, const float* dS, uint32_t ld_s, uint32_t N, float* g_x,
                                       void* stream)
{
    if (!field) return CNC_ERR_INVALID_VALUE;
    if (field->flags & CNC_FIELD_CONTRACT) return CNC_ERR_UNSUPPORTED;          // bounded fields only
    if (N == 0) return CNC_OK;
    const uint32_t F = field->n_features;
    uint32_t       n_units = 0;
    for (int k = 0; k < 4; k++) {
        if (field->n_levels[k] && !field->bits[k]) return CNC_ERR_INVALID_VALUE;
        n_units += field->n_levels[k];
    }
    if (!positions || !selector || !dX || !g_x || !field->aabb || !field->units || n_units == 0
        || ((uintptr_t)field->units & 15u) != 0)
        return CNC_ERR_INVALID_VALUE;
    if (F != 2 && F != 4 && F != 8) return CNC_ERR_UNSUPPORTED;
    // the dX rows are read F columns at a time with 8- / 16-byte loads
    if (ld_x % 4 != 0 || ld_x < n_units * F || ((uintptr_t)dX & 15u) != 0) return CNC_ERR_INVALID_VALUE;
    if (dS && (!field->freqs || ld_s < 3 + 6 * field->n_freqs)) return CNC_ERR_INVALID_VALUE;
    if (N > 0x3FFFFFFFu) return CNC_ERR_INVALID_VALUE;                          // four lanes per sample in a 32-bit index
    PositionGradArgs a;
    a.pos = positions;
    a.aabb = field->aabb;
    a.selector = selector;
    a.dX = dX;
    a.dS = dS;
    a.freqs = field->freqs;
    a.units = reinterpret_cast<const uint4*>(field->units);
    for (int k = 0; k < 4; k++) a.bits[k] = field->bits[k];
    a.g_x = g_x;
    a.N = N;
    a.ld_x = ld_x;
    a.ld_s = ld_s;
    a.n_units = n_units;
    a.n_freqs = dS ? field->n_freqs : 0;
    const dim3  grid(div_up(N, 64u));
    hipStream_t s = (hipStream_t)stream;
    if (F == 2) hipLaunchKernelGGL((k_field_position_grad<2>), grid, dim3(256), 0, s, a);
    else if (F == 4) hipLaunchKernelGGL((k_field_position_grad<4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_field_position_grad<8>), grid, dim3(256), 0, s, a);
    return launch_status();
}
