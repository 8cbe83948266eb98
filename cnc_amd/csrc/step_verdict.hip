// step_verdict.hip — the training step's verdict, reached on the device before the optimizer's update: go, or skip.
//
// The reference scales its loss with GradScaler(2**10) and never calls scaler.step (train_CNC_nerf_synthetic.py:211,361-363):
// a non-finite gradient goes straight into Adam's moments.  Here the step's small gradients (MLPs, context heads, the loss
// scalars: well under a megabyte) are scanned for non-finite values, the fused training forward's fp16 range guard
// (cnc_fused_field_t.guard) is evaluated where it lives, and the result is left in a caller-owned cnc_step_verdict_t that the
// guarded Adam kernel (cnc_table_adam_guarded, table_adam.hip) and torch's fused Adam (`found_inf`) read.  No host wait.
//
//   k_verdict_scan   up to 48 tensors per launch, grid-stride, 16-byte loads over the aligned body of each tensor and 4-byte
//                    loads over its unaligned head and tail; one ballot per wave and reason, one atomicOr from one lane of a
//                    wave that found something.  A clean step writes nothing to the verdict.
//   k_verdict_seal   one wave behind the step's scans: accumulation word -> `skip`, found_inf, and on go the bias
//                    corrections of the update that follows, from two running products b1^t, b2^t (one IEEE double
//                    multiplication a step: a NumPy twin reproduces every bit, which a library pow would not allow) and the
//                    zeroing of the sign planes' clip counters.  On skip none of these moves.
#include <math.h>

#include "common.hpp"

namespace cnc {

constexpr uint32_t kScanThreads = 256, kScanMaxBlocks = 64;

__device__ __forceinline__ uint32_t nonfinite_bits(uint32_t w) { return (w & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

__global__ __launch_bounds__(kScanThreads) void k_verdict_scan(cnc_verdict_scan_t a)
{
    const uint64_t gtid = (uint64_t)blockIdx.x * kScanThreads + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * kScanThreads;
    uint32_t       bad = 0;
    for (uint32_t t = 0; t < a.n_tensors; t++) {
        const float*   ptr = a.ptr[t];
        const uint64_t n = a.n[t];
        if (ptr == nullptr || n == 0) continue;
        // [0, head): 4-byte loads up to the first 16-byte boundary; [head, head + 4 nvec): uint4 loads; the rest: 4-byte loads
        uint64_t head = ((16u - (uint32_t)((uintptr_t)ptr & 15u)) & 15u) >> 2;
        if (head > n) head = n;
        const uint64_t  nvec = (n - head) >> 2;
        const uint64_t  tail0 = head + (nvec << 2);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(ptr);
        const uint4*    body = reinterpret_cast<const uint4*>(w + head);
        for (uint64_t i = gtid; i < nvec; i += stride) {
            const uint4 q = body[i];
            bad |= nonfinite_bits(q.x) | nonfinite_bits(q.y) | nonfinite_bits(q.z) | nonfinite_bits(q.w);
        }
        const uint64_t edge = head + (n - tail0);            // at most 3 + 3 elements
        if (gtid < edge) {
            const uint64_t j = gtid < head ? gtid : tail0 + (gtid - head);
            bad |= nonfinite_bits(w[j]);
        }
    }
    uint32_t fired = 0;
    if (gtid == 0 && (a.guard != nullptr || a.poison != nullptr)) {
        if (a.guard != nullptr) {
            // check_range_guard's predicate (cnc_amd/field.py): a saving forward since `guard_seen` saturated, or a layer of
            // the current pack holds a weight beyond fp16's range
            const uint32_t g0 = a.guard[0];
            fired = (g0 != 0u && g0 >= a.guard_seen) ? 1u : 0u;
#pragma unroll
            for (uint32_t k = 1; k < 6; k++) fired |= a.guard[k] == a.pack_id ? 1u : 0u;
        }
        if (a.poison != nullptr) *a.poison = fired ? INFINITY : 0.0f;
    }
    const bool any_bad = __ballot(bad != 0u) != 0ull, any_fired = __ballot(fired != 0u) != 0ull;
    if ((any_bad || any_fired) && (threadIdx.x & (kWave - 1)) == 0)
        atomicOr(&a.verdict->acc, (any_bad ? CNC_VERDICT_NONFINITE : 0u) | (any_fired ? CNC_VERDICT_RANGE_GUARD : 0u));
}

__global__ __launch_bounds__(kWave) void k_verdict_seal(cnc_verdict_seal_t a)
{
    if (threadIdx.x != 0) return;
    cnc_step_verdict_t* v = a.verdict;
    const uint32_t      reasons = v->acc;
    v->acc = 0u;
    v->skip = reasons;
    if (a.found_inf != nullptr) *a.found_inf = reasons ? 1.0f : 0.0f;
    if (reasons) {
        v->skipped += 1u;
        v->reasons_seen |= reasons;
        return;
    }
    const double b1t = v->b1_pow * a.beta1, b2t = v->b2_pow * a.beta2;
    v->b1_pow = b1t;
    v->b2_pow = b2t;
    v->lr_over_bc1 = a.lr / (1.0 - b1t);
    v->one_minus_b1 = 1.0 - a.beta1;
    v->b2 = a.beta2;
    v->one_minus_b2 = 1.0 - a.beta2;
    v->bc2_sqrt = sqrt(1.0 - b2t);
    v->eps = a.eps;
    v->wd = a.weight_decay;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (a.clip_count[k] != nullptr) *a.clip_count[k] = 0u;
}

}   // namespace cnc

extern "C" int cnc_step_verdict_scan(const cnc_verdict_scan_t* scan, void* stream)
{
    if (!scan || !scan->verdict || scan->n_tensors > CNC_VERDICT_MAX_TENSORS) return CNC_ERR_INVALID_VALUE;
    if ((uintptr_t)scan->verdict & 7) return CNC_ERR_INVALID_VALUE;
    uint64_t vecs = 0;
    for (uint32_t t = 0; t < scan->n_tensors; t++) {
        if (!scan->ptr[t] || scan->n[t] == 0) continue;
        if ((uintptr_t)scan->ptr[t] & 3) return CNC_ERR_INVALID_VALUE;
        vecs += scan->n[t] / 4 + 1;
    }
    if (vecs == 0 && !scan->guard && !scan->poison) return CNC_OK;          // nothing to look at
    if (((uintptr_t)scan->guard | (uintptr_t)scan->poison) & 3) return CNC_ERR_INVALID_VALUE;
    // 4 uint4 loads a lane before the grid widens; 64 blocks of 256 lanes cover a megabyte in 4 rounds
    uint64_t blocks = (vecs + cnc::kScanThreads * 4 - 1) / (cnc::kScanThreads * 4);
    blocks = blocks < 1 ? 1 : blocks > cnc::kScanMaxBlocks ? cnc::kScanMaxBlocks : blocks;
    hipLaunchKernelGGL(cnc::k_verdict_scan, dim3((uint32_t)blocks), dim3(cnc::kScanThreads), 0, (hipStream_t)stream, *scan);
    return cnc::launch_status();
}

extern "C" int cnc_step_verdict_seal(const cnc_verdict_seal_t* seal, void* stream)
{
    if (!seal || !seal->verdict || ((uintptr_t)seal->verdict & 7) || ((uintptr_t)seal->found_inf & 3)) return CNC_ERR_INVALID_VALUE;
    if (!(seal->beta1 >= 0.0 && seal->beta1 < 1.0 && seal->beta2 >= 0.0 && seal->beta2 < 1.0)) return CNC_ERR_INVALID_VALUE;
    for (uint32_t k = 0; k < 4; k++)
        if ((uintptr_t)seal->clip_count[k] & 3) return CNC_ERR_INVALID_VALUE;
    hipLaunchKernelGGL(cnc::k_verdict_seal, dim3(1), dim3(cnc::kWave), 0, (hipStream_t)stream, *seal);
    return cnc::launch_status();
}
