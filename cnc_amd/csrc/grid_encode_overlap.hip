// grid_encode_overlap.hip — the backward of one encoder call scheduled over three HIP streams, behind the C ABI.
//
// The coarse levels (run-merging atomic kernel) and the finest levels (bin + owner passes, grid_encode_binned.hip)
// write disjoint table rows and lean on different units (memory-side atomics vs. HBM reads / writes), so they
// overlap: measured 1.12 -> 1.07 ms per 2^20 samples (docs/engineering_log.md §4.2b).  Until ABI v20 the fork / join lived in the
// Python mirror; a C or C++ integrator calling cnc_grid_encode_backward_binned got the serial 1.12 ms.  Here the
// streams and events belong to a plan object the caller creates once (no globals in the library), and one call
// does:   fork event on `stream`  ->  finest levels in one or two groups on the plan's side streams
//                                 ->  coarse levels on `stream`  ->  `stream` waits for the groups.
// (one group unless CNC_BWD_GROUP_SPLIT asks for two: split_groups)
// Everything the call touches is ordered on `stream` again when it returns.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>

#include "cnc_hip.h"
#include "common.hpp"
#include "encoder_common.hpp"      // EncoderCall, levels, split_scratch

struct cnc_backward_plan {
    hipStream_t side[2];
    hipEvent_t  fork;
    hipEvent_t  join[2];
    int         device;
    int         group_split;    // CNC_BWD_GROUP_SPLIT (split_groups); 0: not set
};

namespace {
constexpr uint32_t kMinOverlapPoints = 1u << 16;   // below that the events cost more than the overlap returns

// The finest levels run as ONE group: the bin pass of all of them, then their owner pass, on one side stream.  Until
// round 8 four or more levels went as two halves on the two side streams (the bin pass of one next to the owner pass of
// the other: 1.122 -> 1.083 ms in the round-2 bench; at parity in round 3); with today's kernels the halves cost 2.4 %
// of the bench frame: call 1.034 -> 1.010 ms, profiles/r09_owner_xcd_placement.md.  One group is also what
// CNC_FLAG_OWNER_XCD_PAIRS needs: the two levels of a pair sit on complementary halves of the workgroup labels, which
// means something only inside one launch.  Measurement switch CNC_BWD_GROUP_SPLIT=k, read when the plan is created: the
// first k levels and the rest as two groups (an odd k cuts a pair, which costs speed only).
inline int split_groups(uint32_t n_binned, int group_split, uint32_t first[2], uint32_t count[2])
{
    if (group_split > 0 && (uint32_t)group_split < n_binned) {
        count[0] = (uint32_t)group_split; count[1] = n_binned - count[0];
        first[0] = 0; first[1] = count[0];
        return 2;
    }
    first[0] = 0; count[0] = n_binned;
    return 1;
}
}  // namespace

extern "C" int cnc_backward_plan_create(cnc_backward_plan** out)
{
    if (!out) return CNC_ERR_INVALID_VALUE;
    cnc_backward_plan* p = new (std::nothrow) cnc_backward_plan();
    if (!p) return CNC_ERR_LAUNCH;
    bool ok = hipGetDevice(&p->device) == hipSuccess;
    // The side streams (the finest levels: the longer half, request-bound) run at the LOWEST stream priority: the coarse
    // kernel on the caller's stream is dispatched first and the bin / owner blocks fill in around it — 0.983 -> 0.972 ms
    // per 2^20 samples (three alternating runs; above the caller's priority: 0.982).  CNC_BWD_SIDE_PRIORITY overrides.
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    const char* pr = getenv("CNC_BWD_SIDE_PRIORITY");
    const int   prio = pr ? atoi(pr) : least;
    const char* gs = getenv("CNC_BWD_GROUP_SPLIT");
    p->group_split = gs ? atoi(gs) : 0;
    for (int i = 0; i < 2 && ok; ++i) {
        ok = hipStreamCreateWithPriority(&p->side[i], hipStreamNonBlocking, prio) == hipSuccess
             && hipEventCreateWithFlags(&p->join[i], hipEventDisableTiming) == hipSuccess;
    }
    ok = ok && hipEventCreateWithFlags(&p->fork, hipEventDisableTiming) == hipSuccess;
    if (!ok) { delete p; return CNC_ERR_LAUNCH; }     // partially created handles are leaked only on a broken runtime
    *out = p;
    return CNC_OK;
}

extern "C" int cnc_backward_plan_destroy(cnc_backward_plan* p)
{
    if (!p) return CNC_OK;
    for (int i = 0; i < 2; ++i) {
        (void)hipStreamSynchronize(p->side[i]);
        (void)hipStreamDestroy(p->side[i]);
        (void)hipEventDestroy(p->join[i]);
    }
    (void)hipEventDestroy(p->fork);
    delete p;
    return CNC_OK;
}

extern "C" uint64_t cnc_grid_encode_backward_overlapped_workspace(uint32_t N, uint32_t n_binned, uint32_t level_rows)
{
    return cnc::scratch_bytes(N, n_binned, level_rows, true);
}

extern "C" int cnc_grid_encode_backward_overlapped(cnc_backward_plan* plan, const float* grad, const float* inputs,
                                                   const float* embeddings, const int32_t* offsets,
                                                   const int32_t* resolutions, float* grad_embeddings,
                                                   uint32_t N, uint32_t D, uint32_t F, uint32_t L, uint32_t flags,
                                                   const uint32_t* ste_clip_count, uint32_t grad_ld, uint32_t grad_col,
                                                   uint32_t n_binned, uint32_t level_rows,
                                                   void* workspace, uint64_t workspace_bytes, void* stream)
{
    using namespace cnc;
    EncoderCall c{grad, inputs, embeddings, offsets, resolutions, grad_embeddings, N, D, F, L, 0, nullptr, nullptr, nullptr,
                  nullptr, flags, ste_clip_count, nullptr, nullptr, nullptr, FeatLayout{grad_ld, grad_col},
                  (hipStream_t)stream};
    int rc = validate(c, EncoderEntry::routed);
    if (rc != CNC_OK || c.empty()) return rc;
    if (n_binned > L) return CNC_ERR_INVALID_VALUE;
    const uint32_t coarse = L - n_binned;
    if (!plan || coarse == 0 || n_binned == 0 || N < kMinOverlapPoints)
        return grid_encode_backward_binned(c, n_binned, level_rows, workspace, workspace_bytes);
    if (!workspace || (uintptr_t)workspace % 16 != 0) return CNC_ERR_INVALID_VALUE;
    // a caller that brought all the scratch asked for lends its tail to the coarse call; with less, the bins keep all of
    // it and the merge kernel's blocks take consecutive samples
    uint16_t* tile_order = split_scratch(N, n_binned, level_rows, true, workspace, workspace_bytes);
    uint32_t first[2], count[2];
    const int groups = split_groups(n_binned, plan->group_split, first, count);
    // each group gets a share of the caller's scratch proportional to its level count (deeper bins when the caller
    // passes more than the minimum)
    if (hipEventRecord(plan->fork, c.stream) != hipSuccess) return CNC_ERR_LAUNCH;
    uint64_t used = 0;
    for (int g = 0; g < groups; ++g) {
        uint64_t share = g + 1 < groups ? workspace_bytes * count[g] / n_binned / kScratchAlign * kScratchAlign : workspace_bytes - used;
        char* ws = (char*)workspace + used;
        used += share;
        if (hipStreamWaitEvent(plan->side[g], plan->fork, 0) != hipSuccess) return CNC_ERR_LAUNCH;
        EncoderCall gc = levels(c, coarse + first[g], count[g]);
        gc.stream = plan->side[g];
        const int rg = grid_encode_backward_binned(gc, count[g], level_rows, ws, share);
        if (rg != CNC_OK && rc == CNC_OK) rc = rg;
        if (hipEventRecord(plan->join[g], plan->side[g]) != hipSuccess) return CNC_ERR_LAUNCH;
    }
    // the coarse levels fill in next to the (longer) bin + owner passes, on the caller's stream
    const int rc0 = grid_encode_backward_with_scratch(coarse_levels(c, coarse, tile_order));
    for (int g = 0; g < groups; ++g)
        if (hipStreamWaitEvent(c.stream, plan->join[g], 0) != hipSuccess) return CNC_ERR_LAUNCH;
    return rc0 != CNC_OK ? rc0 : rc;
}
