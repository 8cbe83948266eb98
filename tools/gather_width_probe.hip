// gather_width_probe.hip — what does a divergent gather cost per lane as the loaded word gets wider?
//
// The bit-plane forward (cnc_amd/csrc/encoder_common.hpp, unit_issue_fast) reads one sign byte per corner from a
// 512 KiB plane per level, every lane at a row of its own.  Its paired path replaces two such byte loads with one
// aligned wider word; that pays only if the texture-address path does not charge a divergent 8- or 16-byte load more
// than a divergent byte load.  Here every lane of every wave gathers from pseudo-random ALIGNED positions of a table with
// global_load_ubyte, _dword, _dwordx2 and _dwordx4, 8 waves per SIMD (2,048 workgroups of 256 lanes on 256 CUs), the
// addresses independent of the loaded data, 8 gathers in flight per lane.  Two tables: 512 KiB (the size of one
// level's plane: L2-resident, far more lines than an L1 holds, so every gather is a line fill) and 16 KiB (L1-resident:
// the address path and the L1 alone).  Prints lane-gathers per second for each form.
// Not part of the library and not called from the product.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/gather_width_probe tools/gather_width_probe.hip && tools/gather_width_probe
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

constexpr uint32_t kTableBytes = 512u << 10;          // allocated; the kernels use the first `bytes` of it
constexpr uint32_t kBlocks = 256 * 8, kThreads = 256, kIters = 512, kInFlight = 8;

template <uint32_t W>
__device__ __forceinline__ uint32_t gather(const uint8_t* __restrict__ table, uint32_t at)
{
    // at < bytes <= kTableBytes and a multiple of W: the W bytes lie inside the table
    if constexpr (W == 1) return table[at];
    else if constexpr (W == 4) return *reinterpret_cast<const uint32_t*>(table + at);
    else if constexpr (W == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(table + at);
        return v.x ^ v.y;
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(table + at);
        return v.x ^ v.y ^ v.z ^ v.w;
    }
}

template <uint32_t W>
__global__ __launch_bounds__(256) void k_gather(const uint8_t* __restrict__ table, uint32_t bytes, uint32_t* __restrict__ sink)
{
    uint32_t h = (blockIdx.x * kThreads + threadIdx.x) * 2654435761u + 12345u, acc = 0;
#pragma unroll 1
    for (uint32_t it = 0; it < kIters; it++) {
        uint32_t v[kInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kInFlight; j++) {
            h = h * 1664525u + 1013904223u;
            v[j] = gather<W>(table, (h >> 9) & (bytes - 1u) & ~(W - 1u));
        }
#pragma unroll
        for (uint32_t j = 0; j < kInFlight; j++) acc ^= v[j];
    }
    sink[blockIdx.x * kThreads + threadIdx.x] = acc;
}

template <uint32_t W>
static double run(const uint8_t* table, uint32_t bytes, uint32_t* sink)
{
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const int reps = 20;
    for (int i = 0; i < 3; i++) hipLaunchKernelGGL(k_gather<W>, dim3(kBlocks), dim3(kThreads), 0, 0, table, bytes, sink);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < reps; i++) hipLaunchKernelGGL(k_gather<W>, dim3(kBlocks), dim3(kThreads), 0, 0, table, bytes, sink);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
    return (double)ms / reps;
}

int main()
{
    uint8_t*  table = nullptr;
    uint32_t* sink = nullptr;
    CHECK(hipMalloc(&table, kTableBytes));
    CHECK(hipMalloc(&sink, (size_t)kBlocks * kThreads * sizeof(uint32_t)));
    std::vector<uint8_t> h(kTableBytes);
    for (uint32_t i = 0; i < kTableBytes; i++) h[i] = (uint8_t)(i * 197u + (i >> 8));
    CHECK(hipMemcpy(table, h.data(), kTableBytes, hipMemcpyHostToDevice));
    const double gathers = (double)kBlocks * kThreads * kIters * kInFlight;
    printf("%u x %u lanes, %u gathers per lane, %u in flight\n", kBlocks, kThreads, kIters * kInFlight, kInFlight);
    printf("%-8s %-10s %10s %18s %14s\n", "table", "form", "ms", "lane-gathers / s", "bytes / s");
    for (int pass = 0; pass < 2; pass++)            // twice: the spread between the passes is the noise
        for (uint32_t bytes : {kTableBytes, 16u << 10}) {   // powers of two <= kTableBytes
            const double t1 = run<1>(table, bytes, sink), t4 = run<4>(table, bytes, sink), t8 = run<8>(table, bytes, sink),
                         t16 = run<16>(table, bytes, sink);
            const struct { const char* name; double ms; uint32_t w; } rows[4] = {
                {"ubyte", t1, 1}, {"dword", t4, 4}, {"dwordx2", t8, 8}, {"dwordx4", t16, 16}};
            for (const auto& r : rows)
                printf("%4u KiB %-10s %10.4f %18.4g %14.4g\n", bytes >> 10, r.name, r.ms, gathers / (r.ms * 1e-3),
                       gathers * r.w / (r.ms * 1e-3));
        }
    CHECK(hipFree(table));
    CHECK(hipFree(sink));
    return 0;
}
