// xcd_label_probe.hip — do workgroup ids w with (w % 8) < 4 and those with (w % 8) >= 4 run on disjoint sets of XCDs?
//
// The paired owner placement (CNC_FLAG_OWNER_XCD_PAIRS, cnc_amd/csrc/grid_encode_binned.hip: owner_slab) rests on the
// observed round-robin dealing of a 1-D grid's workgroups over the 8 XCDs.  That is behaviour, not a contract, so every
// measurement session runs this once: each workgroup records HW_REG_XCC_ID against its linear id, for
//   * a plain 1-D grid of short 64-thread workgroups,
//   * a grid of the owner pass's size and shape: 9 KB of LDS per workgroup, 3 pairs x 5 parts x 2 x 2048 ids, of which
//     only the first 2 x 2048 of each pair (every bin's first wave) stay for a while and the rest leave at once.
// Prints, per label w % 8, how many workgroups each XCD got, and whether labels 0-3 and 4-7 met disjoint XCD sets.
// Not part of the library and not called from the product.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/xcd_label_probe tools/xcd_label_probe.hip && tools/xcd_label_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

// ids below `stay_ids` of every `period` ids spin for `spin` dependent FMAs, the others return at once
__global__ __launch_bounds__(64) void census(uint32_t* out, uint32_t n, uint32_t period, uint32_t stay_ids, int spin, int lds_words)
{
    __shared__ float s_pad[9 * 256];                                    // 9 KB, as k_bwd_owner at F = 8
    const uint32_t w = blockIdx.x;
    if (w >= n) return;
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xFu;   // HW_REG_XCC_ID (a register read)
    float a = threadIdx.x;
    if (lds_words > 0) s_pad[threadIdx.x % lds_words] = a;              // keeps the LDS allocation alive
    if (w % period < stay_ids)
        for (int i = 0; i < spin; ++i) a = a * 1.0001f + 0.5f;
    if (threadIdx.x == 0) out[w] = xcc;
    if (a == 12345.f) out[0] = (uint32_t)s_pad[0];
}

static bool report(const char* name, const std::vector<uint32_t>& xcc)
{
    uint32_t hist[8][16] = {};
    for (size_t w = 0; w < xcc.size(); ++w) hist[w % 8][xcc[w] & 15u]++;
    printf("%s: %zu workgroups\n  label :", name, xcc.size());
    for (int x = 0; x < 8; ++x) printf("  xcd%d", x);
    printf("\n");
    uint32_t set[8] = {}, pure = 0;
    for (int l = 0; l < 8; ++l) {
        printf("  %5d :", l);
        uint32_t most = 0, all = 0;
        for (int x = 0; x < 8; ++x) {
            printf(" %5u", hist[l][x]);
            if (hist[l][x]) set[l] |= 1u << x;
            most = hist[l][x] > most ? hist[l][x] : most;
            all += hist[l][x];
        }
        printf("\n");
        pure += most == all;
    }
    const uint32_t lo = set[0] | set[1] | set[2] | set[3], hi = set[4] | set[5] | set[6] | set[7];
    const bool disjoint = (lo & hi) == 0;
    printf("  labels with a single XCD: %u of 8;  XCD sets of labels 0-3 / 4-7: 0x%02x / 0x%02x -> %s\n", pure, lo, hi,
           disjoint ? "DISJOINT" : "OVERLAPPING");
    return disjoint;
}

int main()
{
    const uint32_t plain = 8192, owner = 3 * 5 * 2 * 2048;
    uint32_t* d = nullptr;
    CHECK(hipMalloc(&d, owner * sizeof(uint32_t)));
    std::vector<uint32_t> h;
    bool ok = true;
    for (int rep = 0; rep < 2; ++rep) {
        CHECK(hipMemset(d, 0xFF, owner * sizeof(uint32_t)));
        hipLaunchKernelGGL(census, dim3(plain), dim3(64), 0, 0, d, plain, 1u, 1u, 2000, 0);
        CHECK(hipDeviceSynchronize());
        h.assign(plain, 0);
        CHECK(hipMemcpy(h.data(), d, plain * sizeof(uint32_t), hipMemcpyDeviceToHost));
        ok = report("plain 1-D grid", h) && ok;

        CHECK(hipMemset(d, 0xFF, owner * sizeof(uint32_t)));
        hipLaunchKernelGGL(census, dim3(owner), dim3(64), 0, 0, d, owner, 5u * 2 * 2048, 2u * 2048, 200000, 64);
        CHECK(hipDeviceSynchronize());
        h.assign(owner, 0);
        CHECK(hipMemcpy(h.data(), d, owner * sizeof(uint32_t), hipMemcpyDeviceToHost));
        ok = report("owner-pass grid", h) && ok;
    }
    CHECK(hipFree(d));
    printf("verdict: label halves %s\n", ok ? "disjoint in every launch" : "NOT disjoint in every launch");
    return 0;
}
