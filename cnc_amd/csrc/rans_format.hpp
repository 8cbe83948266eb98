// rans_format.hpp — the "rans1" stream format's arithmetic, shared by the host twin (rans_coder.cpp) and the device
// coder (rans_coder.hip).  The format itself is written down in include/cnc_codec.h and DESIGN §4.8.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CNC_RANS_HD __host__ __device__ inline
#else
#define CNC_RANS_HD inline
#endif

namespace rans {

constexpr uint32_t kFormatId = 0x72;         // 'r'
constexpr uint32_t kL = 1u << 23;            // lower bound of the normalised state
constexpr uint32_t kHeaderBytes = 6;         // format id, directory entry width, K as u32 LE
constexpr uint32_t kStateBytes = 4;

// c1 = P(-1) * 2^16 in [1, 65535]: the range coder's quantisation (range_coder.cpp, cdf_one), with the clamp and the
// NaN case made explicit.  float32, round half to even; the library is built with contraction off.
CNC_RANS_HD uint32_t c1_of(float p_one)
{
    float r = __builtin_rintf((1.0f - p_one) * 65534.0f);
    if (r != r) return 32768u;
    r = r < 0.0f ? 0.0f : (r > 65534.0f ? 65534.0f : r);
    return static_cast<uint32_t>(r) + 1u;
}

CNC_RANS_HD int64_t lanes_of(int64_t n, int64_t symbols_per_lane)
{
    return n <= 0 ? 0 : (n + symbols_per_lane - 1) / symbols_per_lane;
}

// symbols of lane j of K: j, j + K, ... below n
CNC_RANS_HD int64_t lane_symbols(int64_t n, int64_t K, int64_t j) { return (n - j + K - 1) / K; }

// A lane emits at most two bytes per symbol (x < 2^31 comes down to below f << 15 >= 2^15 in two shifts).  The
// directory entry width is the smallest that holds that worst case for the longest lane: fixed by (n, K) alone, so
// every builder writes the same bytes.
CNC_RANS_HD uint32_t dir_width(int64_t n, int64_t K)
{
    if (K <= 0) return 1;
    const uint64_t worst = 2ull * static_cast<uint64_t>(lane_symbols(n, K, 0));
    return worst < (1ull << 8) ? 1u : worst < (1ull << 16) ? 2u : worst < (1ull << 24) ? 3u : 4u;
}

// One encoder step after the renormalisation: x in [f << 7, f << 15) -> [2^23, 2^31).
CNC_RANS_HD uint32_t push(uint32_t x, uint32_t f, uint32_t c) { return ((x / f) << 16) + (x % f) + c; }

}  // namespace rans
