// grid_encode_ordered.hip — cnc_grid_encode_backward_ordered: the table-gradient scatter of the hash-grid encoder with
// every sum carried in ONE fixed order, the order of the serial CPU oracle (oracle/cnc_oracle.c, orc_bwd_point under
// threads == 1): per table element, level slot by level slot, point by point, corner by corner, each term
// (w[c] * wn_re) * grad rounded twice and added with one rounded fp32 add.  The result is bit-equal to the oracle's and
// therefore the same from run to run, stream to stream and rank to rank.  A mode for reproducibility, debugging and
// exact regression tests: several times slower than the atomic routes, which stay the default.
//
// Per level slot, three steps on the caller's stream, no atomics anywhere:
//   emit    lane = point b: item seq = b * 2^D + c of every corner c gets a 32-bit key (the corner's absolute table row;
//           kNoRow for a border / masked corner or a point outside [0,1]^D), the value seq, and weight[seq] = w[c] * wn_re.
//           The layout is a pure function of the inputs.
//   sort    rocprim::radix_sort_pairs, stable, on the keys: equal rows keep their seq order = (point, corner).
//   reduce  the lane group at a segment head (key[i] != key[i-1]) owns the row: it loads the row of grad_embeddings,
//           walks its segment in order and stores the row with plain vector stores.  One lane carries one channel's sum
//           from start to end (F/4 lanes with four channels each for F >= 4): nothing is reassociated.  The loads of
//           the next kAhead items are issued before the adds of the current ones, since the chain of fp adds is the
//           only serial part and a coarse level's row has thousands of terms.
// Slots run one after another, each adding to what the previous one left in grad_embeddings: that is the oracle's
// slot-major order, also where per-point level windows (min_level_id) make different slots hit the same rows.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.hpp"
#include "encoder_common.hpp"

namespace cnc {

namespace {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;   // sorts behind every row: offsets are int32, a row is < 2^31
constexpr uint32_t kAhead = 8;             // items in flight per owner lane

template <uint32_t D, bool VXL>
__global__ __launch_bounds__(256) void k_ordered_emit(const float* __restrict__ inputs, const int32_t* __restrict__ offsets,
                                                      const int32_t* __restrict__ resolutions, uint32_t N, uint32_t slot,
                                                      uint32_t Rb, const uint8_t* __restrict__ vxl,
                                                      const int32_t* __restrict__ min_level_id,
                                                      const int32_t* __restrict__ sat, FeatLayout lay,
                                                      uint32_t* __restrict__ keys, uint32_t* __restrict__ seqs,
                                                      float* __restrict__ weights)
{
    constexpr uint32_t C = 1u << D;
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= N) return;
    uint32_t key[C];
    float    tw[C];
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        key[i] = kNoRow;
        tw[i] = 0;
    }
    float x[D];
    if (load_point<D>(inputs, b, x)) {
        const uint32_t level = slot + (min_level_id ? (uint32_t)min_level_id[b] : 0u);
        const uint32_t off = (uint32_t)offsets[level];
        const uint32_t hs = (uint32_t)offsets[level + 1] - off;
        const uint32_t R = (uint32_t)resolutions[level];
        Corners<D, VXL> c;
        c.setup(x, R, hs, Rb, vxl, sat, vertex_plane(lay, level));
#pragma unroll
        for (uint32_t i = 0; i < C; i++) {
            if (c.valid[i]) key[i] = off + c.row[i];
            tw[i] = c.w[i] * c.wn_re;
        }
    }
    const uint32_t s0 = b * C;
#pragma unroll
    for (uint32_t i = 0; i < C; i++) {
        keys[s0 + i] = key[i];
        seqs[s0 + i] = s0 + i;
        weights[s0 + i] = tw[i];
    }
}

// keys / seqs: the M items sorted by (row, seq).  Lane t serves item t / G, channels [h V, h V + V) with h = t % G.
template <uint32_t F, bool STE>
__global__ __launch_bounds__(256) void k_ordered_reduce(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ seqs,
                                                        const float* __restrict__ weights, const float* __restrict__ grad,
                                                        const float* __restrict__ emb, float* __restrict__ grad_emb,
                                                        const uint32_t* __restrict__ clip_count, uint32_t M, uint32_t N,
                                                        uint32_t log2_C, uint32_t slot, FeatLayout lay)
{
    constexpr uint32_t V = F < 4 ? F : 4;
    constexpr uint32_t G = F / V;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t i = (uint32_t)(t / G), h = (uint32_t)(t % G);
    if (i >= M) return;
    const uint32_t row = keys[i];
    if (row == kNoRow || (i != 0 && keys[i - 1] == row)) return;     // not a segment head

    const size_t at = (size_t)row * F + h * V;
    float acc[V];
    load_vec<V>(grad_emb + at, acc);
    bool keep[V];
#pragma unroll
    for (uint32_t k = 0; k < V; k++) keep[k] = true;
    if (STE && (clip_count == nullptr || *clip_count != 0)) {   // STE_binary.backward: gradient only where |param| <= 1
        float e[V];
        load_vec<V>(emb + at, e);
#pragma unroll
        for (uint32_t k = 0; k < V; k++) keep[k] = e[k] >= -1.0f && e[k] <= 1.0f;
    }
    const uint32_t seq_head = seqs[i];
    for (uint32_t j = i;; j += kAhead) {
        bool  in[kAhead];
        float w[kAhead], g[kAhead][V];
        // an item past the segment is replaced by the head's (always a valid address) and its term dropped below
#pragma unroll
        for (uint32_t u = 0; u < kAhead; u++) {
            const uint32_t jj = j + u < M ? j + u : M - 1;           // (j + u does not wrap: j < M <= 2^32 - 1 - kAhead)
            in[u] = j + u < M && keys[jj] == row;
            const uint32_t sj = seqs[jj];
            const uint32_t s = in[u] ? sj : seq_head;
            w[u] = weights[s];
            load_vec<V>(grad + feat_index(lay, slot, N, s >> log2_C, F) + h * V, g[u]);
        }
#pragma unroll
        for (uint32_t u = 0; u < kAhead; u++) {
            if (!in[u]) break;
#pragma unroll
            for (uint32_t k = 0; k < V; k++) {
                const float term = w[u] * g[u][k];                   // -ffp-contract=off: never an fma with the add
                if (keep[k]) acc[k] = acc[k] + term;
            }
        }
        if (!in[kAhead - 1]) break;
    }
    store_vec<V>(grad_emb + at, acc);
}

constexpr uint64_t round256(uint64_t n) { return (n + 255) / 256 * 256; }

// bytes of rocPRIM's own scratch for M pairs and keys of `bits` bits; 0 on error
uint64_t sort_scratch_bytes(uint32_t M, uint32_t bits, hipStream_t s)
{
    size_t bytes = 0;
    rocprim::double_buffer<uint32_t> k(nullptr, nullptr), v(nullptr, nullptr);
    if (rocprim::radix_sort_pairs(nullptr, bytes, k, v, M, 0, bits, s) != hipSuccess) return 0;
    return bytes ? bytes : 1;
}

struct OrderedScratch {
    uint32_t *keys[2], *seqs[2];
    float*   weights;
    void*    sort;
    uint64_t sort_bytes, total;
};

// the workspace's parts (each 256-byte aligned); keys of 32 bits size rocPRIM's scratch, the most any call needs
bool ordered_scratch(uint32_t N, uint32_t D, void* base, hipStream_t s, OrderedScratch& o)
{
    const uint64_t M = (uint64_t)N << D;
    if (D < 1 || D > 3 || M > 0xFFFFFFFFull - kAhead) return false;
    const uint64_t arr = round256(M * 4);
    o.sort_bytes = sort_scratch_bytes((uint32_t)M, 32, s);
    if (o.sort_bytes == 0) return false;
    char* p = static_cast<char*>(base);
    o.keys[0] = reinterpret_cast<uint32_t*>(p);
    o.keys[1] = reinterpret_cast<uint32_t*>(p + arr);
    o.seqs[0] = reinterpret_cast<uint32_t*>(p + 2 * arr);
    o.seqs[1] = reinterpret_cast<uint32_t*>(p + 3 * arr);
    o.weights = reinterpret_cast<float*>(p + 4 * arr);
    o.sort = p + 5 * arr;
    o.total = 5 * arr + round256(o.sort_bytes);
    return true;
}

template <uint32_t D>
void launch_emit(const EncoderCall& a, uint32_t slot, const OrderedScratch& o)
{
    const dim3 grid(div_up(a.N, 256));
    if (a.vxl)
        hipLaunchKernelGGL((k_ordered_emit<D, true>), grid, dim3(256), 0, a.stream, a.inputs, a.offsets, a.resolutions, a.N,
                           slot, a.Rb, a.vxl, a.mli, a.sat, a.lay, o.keys[0], o.seqs[0], o.weights);
    else
        hipLaunchKernelGGL((k_ordered_emit<D, false>), grid, dim3(256), 0, a.stream, a.inputs, a.offsets, a.resolutions, a.N,
                           slot, a.Rb, a.vxl, a.mli, a.sat, a.lay, o.keys[0], o.seqs[0], o.weights);
}

template <uint32_t F>
int launch_reduce(const EncoderCall& a, uint32_t slot, const uint32_t* keys, const uint32_t* seqs,
                  const OrderedScratch& o)
{
    constexpr uint32_t G = F / (F < 4 ? F : 4);
    const uint32_t M = a.N << a.D;
    const uint64_t blocks = ((uint64_t)M * G + 255) / 256;
    if (blocks >= (1ull << 31)) return CNC_ERR_INVALID_VALUE;
    const dim3 grid((uint32_t)blocks);
    if (a.ste())
        hipLaunchKernelGGL((k_ordered_reduce<F, true>), grid, dim3(256), 0, a.stream, keys, seqs, o.weights, a.grad, a.emb,
                           a.out, a.clip_count, M, a.N, a.D, slot, a.lay);
    else
        hipLaunchKernelGGL((k_ordered_reduce<F, false>), grid, dim3(256), 0, a.stream, keys, seqs, o.weights, a.grad, a.emb,
                           a.out, a.clip_count, M, a.N, a.D, slot, a.lay);
    return CNC_OK;
}

// key_bits: the sort's, enough for every row of the tables
int run_ordered(const EncoderCall& a, uint32_t key_bits, const OrderedScratch& o)
{
    const uint32_t M = a.N << a.D;
    for (uint32_t slot = 0; slot < a.L; slot++) {
        switch (a.D) {
        case 1: launch_emit<1>(a, slot, o); break;
        case 2: launch_emit<2>(a, slot, o); break;
        default: launch_emit<3>(a, slot, o); break;
        }
        rocprim::double_buffer<uint32_t> k(o.keys[0], o.keys[1]), v(o.seqs[0], o.seqs[1]);
        size_t bytes = o.sort_bytes;
        if (rocprim::radix_sort_pairs(o.sort, bytes, k, v, M, 0, key_bits, a.stream) != hipSuccess) return CNC_ERR_LAUNCH;
        int rc = CNC_OK;
        CNC_F_SWITCH(a.F, rc = launch_reduce<FF>(a, slot, k.current(), v.current(), o))
        if (rc != CNC_OK) return rc;
    }
    return CNC_OK;
}

}  // namespace
}  // namespace cnc

using namespace cnc;

extern "C" uint64_t cnc_grid_encode_backward_ordered_workspace(uint32_t N, uint32_t D, uint64_t rows_total)
{
    OrderedScratch o;
    if (N == 0 || rows_total >= kNoRow || !ordered_scratch(N, D, nullptr, nullptr, o)) return 0;
    return o.total;
}

extern "C" int cnc_grid_encode_backward_ordered(const float* grad, const float* inputs, const float* embeddings,
                                                const int32_t* offsets, const int32_t* resolutions,
                                                float* grad_embeddings, uint32_t N, uint32_t D, uint32_t F, uint32_t L,
                                                uint32_t Rb, const float* dy_dx, float* grad_inputs,
                                                const uint8_t* binary_vxl, const int32_t* min_level_id, uint32_t flags,
                                                const uint32_t* ste_clip_count, const int32_t* occ_sat,
                                                const uint32_t* vertex_bits, const int32_t* vertex_bit_offsets,
                                                uint32_t grad_ld, uint32_t grad_col, void* workspace,
                                                uint64_t workspace_bytes, void* stream)
{
    EncoderCall c{grad, inputs, embeddings, offsets, resolutions, grad_embeddings, N, D, F, L, Rb, dy_dx, grad_inputs,
                  binary_vxl, min_level_id, flags, ste_clip_count, occ_sat, vertex_bits, vertex_bit_offsets,
                  FeatLayout{grad_ld, grad_col}, (hipStream_t)stream};
    int rc = validate(c, EncoderEntry::routed);
    if (rc != CNC_OK || c.empty()) return rc;
    if (!workspace) return CNC_ERR_INVALID_VALUE;
    if (!(F == 1 || F == 2 || F == 4 || F == 8 || F == 16 || F == 32)) return CNC_ERR_INVALID_VALUE;
    OrderedScratch o;
    if (!ordered_scratch(N, D, workspace, c.stream, o) || workspace_bytes < o.total ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0)
        return CNC_ERR_INVALID_VALUE;
    uint32_t key_bits = (flags >> CNC_ORDERED_KEY_BITS_SHIFT) & 63u;
    if (key_bits == 0 || key_bits > 32) key_bits = 32;
    if (!layout_ok(c.lay, F, L)) return CNC_ERR_INVALID_VALUE;
    rc = run_ordered(c, key_bits, o);
    if (rc == CNC_OK && dy_dx) rc = launch_input_backward(c);   // per point, no atomics: already exact
    return rc != CNC_OK ? rc : launch_status();
}
