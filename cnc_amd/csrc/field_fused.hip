// field_fused.hip — the gradient-free radiance field as ONE kernel: world positions -> density (-> rgb).  This file holds
// the entry point (cnc_field_fused_forward) and the EXACT fp32 form of the kernel, k_field_fused: the whole call when the
// caller does not ask for the fp16 form, and otherwise the fp16 range guard's fallback, enqueued behind every launch of
// the fp16 kernel (k_field_fused16w2, field_fused2.hip: two waves per tile, the default).
//
// Reference chain (examples/radiance_fields/ngp.py:506-547, compose_3D_2D_embed :620-645): normalise to the unit cube,
// four binarised hash-grid encoders (xyz + the xy / xz / yz planes) and the 63-wide sinusoid embedding concatenated
// into a [N, 255] matrix, base MLP 255 -> H (ReLU) -> 1 + geo, density = trunc_exp(x - 1) * selector; for colours
// [SH4(dir) | geo] -> H -> H -> 3, sigmoid.  The product ran that as encoder launches writing a [N, 256] matrix to HBM
// (1 KB per sample each way), library GEMMs and glue kernels.  Every sample of the sampler's visibility pass, of the
// occupancy refresh and of the evaluation render takes this path without gradients: 6-8x the samples of the
// gradient pass.
//
// In k_field_fused one 64-lane wave owns 32 samples end to end; nothing but positions (and directions) is read and
// nothing but densities (and colours) is written:
//   * layer 1 runs K-chunk by K-chunk.  A chunk is 32 consecutive columns of the feature row; lane (i, h) computes the
//     16 columns [16 h, 16 h + 16) of sample i — whole (encoder, level) units through the same Corners / sign-bit-plane
//     / fmaf chain as k_grid_encode_fwd_bits (bit-identical features), or sinusoid columns — into a 32 x 32 LDS tile
//     that feeds v_mfma_f32_32x32x2_f32 as the A operand; the 32 x H accumulators stay in registers for all chunks.
//     fp32 MFMA = an exact k-ordered fmaf chain, 64 cycles per instruction and SIMD: with 8 K-steps x NT tiles = 80
//     MFMAs per chunk (H = 160) the matrix pipe is the floor (0.55 ms per 2^20 samples at K = 256) and the gather is
//     vector work that a second wave on the same SIMD overlaps with it — hence one-wave workgroups, no block barriers,
//     <= 256 registers.
//   * weights come from a buffer packed in fragment order (cnc_field_pack_all: Wp): one wave-instruction reads 1 KB
//     contiguous, prefetched one K-step ahead, also across the gather of the next chunk.
//   * density only: the second layer's unit 0 is a dot product over the ReLU'd accumulators (vector ALU + an LDS
//     transpose), no further MFMA.  With colours: activations go through LDS (C layout -> row-major, bias + ReLU) between
//     layers; one LDS region per wave is reused for the chunk tile, h1, the head input and the head's hidden layers
//     (a wave's LDS operations execute in order, and every read of a layer is issued before its results exist).
#include "field_fused_common.hpp"

namespace cnc {

// CONTRACT (CNC_FIELD_CONTRACT): the unbounded field's map of the position.  A template parameter, not a run-time test: the
// test cost the bounded kernels registers (profiles/unbounded_field.md).
template <uint32_t F, int NT, bool RGB, bool CONTRACT = false>
__global__ __launch_bounds__(64, 2) void k_field_fused(FusedFieldArgs p)
{
    extern __shared__ float lds[];
    // launched behind an fp16 kernel as its fallback: runs only if that kernel (or the weight packer) raised the flag
    if (p.only_if_flagged && *reinterpret_cast<volatile const uint32_t*>(p.guard) != p.call_id) return;
    const uint32_t lane = threadIdx.x, i = lane & 31u, h = lane >> 5;
    constexpr uint32_t ldh = NT * 32 + kPadH;
    const uint32_t n_rows = rows_of(p);       // p.N, or a count the device holds (cnc_fused_field_t.n_rows_dev) — a LOCAL: writing
                                              // to the by-value argument block would move all of it into scratch memory
    const uint32_t tiles = (n_rows + 31u) / 32u;
    float amin[3], aext[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        amin[a] = p.aabb[a];
        aext[a] = p.aabb[3 + a] - p.aabb[a];
    }
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t row0 = tile * 32, row = row0 + i;
        const bool     live = row < n_rows;
        // unit-cube position and selector of sample i (k_field_prepare: same helper)
        float xu[3] = {-1.0f, -1.0f, -1.0f};
        bool  sel = live;
        if (live) sel = field_unit_position(p.pos + (size_t)row * 3, amin, aext, CONTRACT, xu);
        [[maybe_unused]] const uint64_t selmask = __ballot(sel);          // bit r (< 32) = selector of sample r

        // ---- layer 1, chunk by chunk ----
        f32x16 acc[NT];
        zero_acc<NT>(acc);
        float4 wn[NT];
        const wrsrc_t W1 = weight_rsrc(p.Wp[0]);
        load_w<NT>(W1, 0, lane, wn);
        float* trow = lds + i * kChunkPitch;
        for (uint32_t c = 0; c * 4 < p.nkb1; c++) {
            fill_window<F, !RGB>(p, xu, c * 32 + 16 * h, RowF32{trow});
            wave_lds_order();
#pragma unroll
            for (uint32_t kb = 0; kb < 4; kb++) {
                const uint32_t g = c * 4 + kb;
                const float4   a = *reinterpret_cast<const float4*>(trow + kb * 8 + 4 * h);
                float4 w[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) w[t] = wn[t];
                if (g + 1 < p.nkb1) load_w<NT>(W1, g + 1, lane, wn);
                mfma_step<NT>(a, w, acc);
            }
            wave_lds_order();
        }

        if constexpr (!RGB) {
            // density_raw = b2[0] + sum_j relu(h1[j]) * W2[0][j]: per lane its 16 samples' partial sums over the
            // columns it holds, transposed through LDS, summed per sample
            float part[16];
#pragma unroll
            for (int v = 0; v < 16; v++) part[v] = 0.0f;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const float b = p.Bp[0][t * 32 + i], w2 = p.w2row[t * 32 + i];
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    float x = acc[t][v] + b;
                    x = x > 0 ? x : 0;
                    part[v] = __builtin_fmaf(x, w2, part[v]);
                }
            }
#pragma unroll
            for (int v = 0; v < 16; v++) lds[(8 * (v >> 2) + 4 * h + (v & 3)) * kChunkPitch + i] = part[v];
            wave_lds_order();
            if (h == 0) {
                float s = 0.0f;
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const float4 v4 = *reinterpret_cast<const float4*>(lds + i * kChunkPitch + 4 * q);
                    s += v4.x; s += v4.y; s += v4.z; s += v4.w;
                }
                if (live) p.density[row] = sel ? expf((s + p.Bp[1][0]) - 1.0f) : 0.0f;
            }
            wave_lds_order();
        } else {
            // ---- h1 -> LDS; layer 2 (H -> 1 + geo) ----
            acc_to_lds<true, NT>(lds, ldh, p.Bp[0], acc, lane);
            wave_lds_order();
            constexpr int NT2 = NT == 5 ? 3 : 2;          // 1 + geo <= 96 (H = 160) / 64 (H = 64)
            f32x16 acc2[NT2];
            layer_lds<NT2>(lds, ldh, NT * 4, p.Wp[1], acc2, lane);
            // outputs: column 0 = density_raw, columns 1..geo = geo features -> head input columns 16 + (c - 1);
            // head input = [SH4(dir) (16) | geo | zero padding], K = 8 nkbh <= H columns, in the region (and with the
            // pitch: every LDS offset stays an immediate) h1 occupied — every read of layer 2 has been issued
            const uint32_t Kh = p.nkbh * 8;
            constexpr uint32_t ldi = ldh;
            wave_lds_order();
#pragma unroll
            for (int t = 0; t < NT2; t++) {
                const uint32_t col = t * 32 + i;
                const float    b = p.Bp[1][col];
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const uint32_t r = 8 * (v >> 2) + 4 * h + (v & 3);
                    const float    x = acc2[t][v] + b;
                    if (col == 0) {
                        if (row0 + r < n_rows) p.density[row0 + r] = ((selmask >> r) & 1ull) ? expf(x - 1.0f) : 0.0f;
                    } else if (15 + col < Kh) {
                        lds[r * ldi + 15 + col] = col <= p.geo ? x : 0.0f;
                    }
                }
            }
            {   // SH4 of sample i's direction: lane (i, h) writes harmonics 8 h .. 8 h + 7
                float d3[3] = {0.0f, 0.0f, 1.0f};
                if (live) {
#pragma unroll
                    for (int a = 0; a < 3; a++) d3[a] = ((p.dirs[(size_t)row * 3 + a] + 1.0f) / 2.0f) * 2.0f - 1.0f;
                }
#pragma unroll
                for (uint32_t q = 0; q < 2; q++) {
                    float4 v = sh4_quad(2 * h + q, d3[0], d3[1], d3[2]);
                    if (p.sh_fp16) {
                        v.x = round_through_half(v.x); v.y = round_through_half(v.y);
                        v.z = round_through_half(v.z); v.w = round_through_half(v.w);
                    }
                    *reinterpret_cast<float4*>(lds + i * ldi + 8 * h + 4 * q) = v;
                }
            }
            wave_lds_order();
            // ---- head: (16 + geo) -> H -> H -> 3 ----
            layer_lds<NT>(lds, ldi, p.nkbh, p.Wp[2], acc, lane);
            wave_lds_order();
            acc_to_lds<true, NT>(lds, ldh, p.Bp[2], acc, lane);
            wave_lds_order();
            layer_lds<NT>(lds, ldh, NT * 4, p.Wp[3], acc, lane);
            wave_lds_order();
            acc_to_lds<true, NT>(lds, ldh, p.Bp[3], acc, lane);
            wave_lds_order();
            f32x16 acc5[1];
            layer_lds<1>(lds, ldh, NT * 4, p.Wp[4], acc5, lane);
            if (i < 3) {
                const float b = p.Bp[4][i];
#pragma unroll
                for (int v = 0; v < 16; v++) {
                    const uint32_t r = 8 * (v >> 2) + 4 * h + (v & 3);
                    if (row0 + r < n_rows) p.rgb[(size_t)(row0 + r) * 3 + i] = 1.0f / (1.0f + expf(-(acc5[0][v] + b)));
                }
            }
            wave_lds_order();
        }
    }
}

using FieldKernel = void (*)(FusedFieldArgs);

template <uint32_t F, int NT>
static FieldKernel exact_kernel(bool rgb, bool contract)
{
    if (contract) return rgb ? k_field_fused<F, NT, true, true> : k_field_fused<F, NT, false, true>;
    return rgb ? k_field_fused<F, NT, true> : k_field_fused<F, NT, false>;
}

}  // namespace cnc

using namespace cnc;

extern "C" int cnc_field_fused_forward(const cnc_fused_field_t* f, const float* positions, const float* dirs, uint32_t N,
                                       float* density, float* rgb, void* stream)
{
    if (N == 0) return CNC_OK;
    if (!f || !positions || !density || !f->aabb) return CNC_ERR_INVALID_VALUE;
    const bool want_rgb = rgb != nullptr;
    if (want_rgb && !dirs) return CNC_ERR_INVALID_VALUE;
    const uint32_t F = f->n_features, H = f->n_neurons;
    if (!(F == 2 || F == 4 || F == 8) || !(H == 64 || H == 160)) return CNC_ERR_UNSUPPORTED;
    FusedFieldArgs p{};
    p.pos = positions; p.dirs = dirs; p.aabb = f->aabb; p.N = N;
    p.n_dev = f->n_rows_dev;
    uint32_t units = 0;
    for (int e = 0; e < 4; e++) {
        if (!f->bits[e] || !f->offsets[e] || !f->resolutions[e] || f->n_levels[e] == 0) return CNC_ERR_INVALID_VALUE;
        p.enc[e] = FieldEnc{f->bits[e], f->offsets[e], f->resolutions[e], f->n_levels[e]};
        units += f->n_levels[e];
    }
    if (f->n_levels[1] != f->n_levels[2] || f->n_levels[1] != f->n_levels[3]) return CNC_ERR_UNSUPPORTED;
    if (!f->units) return CNC_ERR_INVALID_VALUE;
    p.units = reinterpret_cast<const uint4*>(f->units);
    if (f->n_freqs == 0) return CNC_ERR_UNSUPPORTED;
    if (!f->freqs) return CNC_ERR_INVALID_VALUE;
    p.freqs = f->freqs; p.n_freqs = f->n_freqs; p.n_units = units;
    const uint32_t K0 = units * F + 3 + 6 * f->n_freqs;
    p.nkb1 = (K0 + 31) / 32 * 4;
    p.geo = f->geo_feat_dim;
    const uint32_t NT = H / 32, NT2 = NT == 5 ? 3u : 2u;
    p.nkbh = (16 + p.geo + 7) / 8;
    // the second layer's output tiles and the head's input (kept inside the hidden layers' LDS region) bound geo
    if (1 + p.geo > NT2 * 32 || p.nkbh * 8 > H) return CNC_ERR_UNSUPPORTED;
    for (int l = 0; l < 5; l++) {
        p.Wp[l] = f->packed_weights[l];
        p.Bp[l] = f->packed_biases[l];
    }
    if (!p.Wp[0] || !p.Bp[0] || !p.Bp[1]) return CNC_ERR_INVALID_VALUE;
    p.w2row = f->w2_row0;
    if (want_rgb) {
        for (int l = 1; l < 5; l++)
            if (!p.Wp[l] || !p.Bp[l]) return CNC_ERR_INVALID_VALUE;
    } else if (!p.w2row) {
        return CNC_ERR_INVALID_VALUE;
    }
    p.density = density; p.rgb = rgb;
    p.sh_fp16 = (f->flags & CNC_FIELD_SH_FP16) ? 1u : 0u;
    const bool contract = (f->flags & CNC_FIELD_CONTRACT) != 0;
    // the fp16 form is the two-wave kernel (field_fused2.hip): 16x16x32 fragments, head input [SH4 | raw density | geo]
    const bool f16x3 = (f->flags & CNC_FIELD_MFMA_F16X3) != 0;
    p.nk16_1 = p.nkb1 / 2;
    p.nk32_h = (17 + p.geo + 31) / 32;
    if (f16x3) {
        if (p.nk32_h * 32 > H) return CNC_ERR_UNSUPPORTED;
        // the range guard is part of the fp16 form: without it a value above 65504 would come out as inf / NaN
        if (!f->guard || f->call_id == 0 || f->pack_id == 0) return CNC_ERR_INVALID_VALUE;
        p.guard = f->guard; p.call_id = f->call_id; p.pack_id = f->pack_id;
        if (f->debug_features) {         // test hook: the density kernel only, rows wide enough for K padded to 32
            if (want_rgb || f->debug_ld < p.nkb1 * 8) return CNC_ERR_UNSUPPORTED;
            p.dbg_features = f->debug_features; p.dbg_ld = f->debug_ld;
        }
        for (int l = 0; l < (want_rgb ? 5 : 1); l++) {
            if (!f->packed_weights16q[l]) return CNC_ERR_INVALID_VALUE;
            p.Wq16[l] = reinterpret_cast<const half_t_*>(f->packed_weights16q[l]);
        }
        if (1 + p.geo > (NT == 5 ? 80u : 64u)) return CNC_ERR_UNSUPPORTED;
    }
    const bool saving = f->save.feat != nullptr;
    if (saving) {                        // the gradient pass's forward: the fp16 colour kernel, saving variant
        const cnc_field_save_t& sv = f->save;
        if (!f16x3 || !want_rgb || f->debug_features) return CNC_ERR_UNSUPPORTED;
        if (!sv.h1 || !sv.h3 || !sv.h4 || !sv.head_in || !sv.raw || !sv.selector || !sv.xyz || !sv.xy || !sv.xz || !sv.yz ||
            sv.ld_feat < p.nkb1 * 8 || sv.ld_feat % 4 != 0 || sv.ld_head != p.nk32_h * 32 || sv.n_live > N)
            return CNC_ERR_INVALID_VALUE;
        p.save = FieldSave{sv.feat, sv.ld_feat, sv.h1, sv.h3, sv.h4, sv.head_in, sv.ld_head, sv.raw, sv.selector,
                           sv.xyz, sv.xy, sv.xz, sv.yz, sv.n_live};
    }
    hipStream_t s = (hipStream_t)stream;
    if (f16x3) {
        const int rc = launch_field_fused_w2(p, want_rgb, contract, F, H, (f->flags & CNC_FIELD_WAVES4) ? 4 : 3, s);
        if (rc != CNC_OK || saving) return rc;              // the saving variant saturates: nothing runs behind it
    }
    // the exact form: the whole call without the fp16 flag, the guard's conditional fallback with it
    p.only_if_flagged = f16x3 ? 1u : 0u;
    FieldKernel kern = nullptr;
    switch (F * 10 + NT) {
    case 85: kern = exact_kernel<8, 5>(want_rgb, contract); break;
    case 82: kern = exact_kernel<8, 2>(want_rgb, contract); break;
    case 45: kern = exact_kernel<4, 5>(want_rgb, contract); break;
    case 42: kern = exact_kernel<4, 2>(want_rgb, contract); break;
    case 25: kern = exact_kernel<2, 5>(want_rgb, contract); break;
    default: kern = exact_kernel<2, 2>(want_rgb, contract); break;
    }
    const size_t lds_bytes = (want_rgb ? 32 * (H + kPadH) : 32 * kChunkPitch) * sizeof(float);
    // The grid is what is RESIDENT at once (the waves loop over the tiles): registers allow 8 one-wave workgroups per
    // CU, the colour variant's LDS 7 — with 8 per CU launched the eighth of every CU ran as a second round on an
    // otherwise idle chip (2.65 instead of 1.72 ms per 2^20 samples).
    uint32_t resident = 0;
    const int rc = resident_grid(kern, 64, lds_bytes, 8, &resident);
    if (rc != CNC_OK) return rc;
    // the guard's conditional launch returns at once in all but pathological calls: a quarter of the resident grid
    // keeps the empty launch short (its waves loop over the tiles when it does run)
    if (p.only_if_flagged) resident /= 4;
    const uint32_t tiles = (N + 31) / 32;
    hipLaunchKernelGGL(kern, dim3(tiles < resident ? tiles : resident), dim3(64), lds_bytes, s, p);
    return launch_status();
}
