// rans_coder.cpp — host twin of the device entropy coder (rans_coder.hip): the "rans1" stream format of
// include/cnc_codec.h, lane by lane on one thread.  Same bytes as the device coder; it is what the tests and the
// host-side check of a file run, not a hot path.
#include <cstdint>
#include <cstring>
#include <vector>

#include "cnc_codec.h"
#include "rans_format.hpp"

namespace {

inline uint64_t get_le(const uint8_t* p, uint32_t width)
{
    uint64_t v = 0;
    for (uint32_t b = 0; b < width; ++b) v |= static_cast<uint64_t>(p[b]) << (8 * b);
    return v;
}

inline void put_le(uint8_t* p, uint64_t v, uint32_t width)
{
    for (uint32_t b = 0; b < width; ++b) p[b] = static_cast<uint8_t>(v >> (8 * b));
}

struct Header {
    int64_t  K;
    uint32_t width;
    int64_t  payload;          // first byte of lane 0's sub-stream
};

// header + directory of in[0, len) for n symbols: 0 and `h`, or -3
int parse(const uint8_t* in, int64_t len, int64_t n, Header& h)
{
    if (n < 0 || len < static_cast<int64_t>(rans::kHeaderBytes) || in[0] != rans::kFormatId) return -3;
    h.width = in[1];
    h.K = static_cast<int64_t>(get_le(in + 2, 4));
    if (h.width < 1 || h.width > 4 || h.K > n || (h.K == 0) != (n == 0)) return -3;
    // K <= n and 6 + K * width <= len before any product can overflow
    if (h.K > (len - rans::kHeaderBytes) / static_cast<int64_t>(h.width)) return -3;
    h.payload = rans::kHeaderBytes + h.K * h.width;
    int64_t left = len - h.payload;
    for (int64_t j = 0; j < h.K; ++j) {
        const int64_t need = static_cast<int64_t>(get_le(in + rans::kHeaderBytes + j * h.width, h.width)) + rans::kStateBytes;
        if (need > left) return -3;
        left -= need;
    }
    return 0;
}

}  // namespace

extern "C" uint32_t cnc_rans_c1(float p_one) { return rans::c1_of(p_one); }

extern "C" int64_t cnc_rans_bound(int64_t n, int64_t symbols_per_lane)
{
    if (n < 0 || symbols_per_lane < 1) return -1;
    const int64_t K = rans::lanes_of(n, symbols_per_lane);
    return rans::kHeaderBytes + K * (rans::dir_width(n, K) + rans::kStateBytes) + 2 * n;
}

extern "C" int64_t cnc_rans_encode_pm1_host(const float* p_one, int64_t p_stride, const float* x_pm1, int64_t n,
                                            int64_t symbols_per_lane, uint8_t* out, int64_t cap)
{
    if (n < 0 || symbols_per_lane < 1 || (p_stride != 0 && p_stride != 1)) return -2;
    const int64_t  K = rans::lanes_of(n, symbols_per_lane);
    if (K > 0xFFFFFFFFll) return -2;
    const uint32_t width = rans::dir_width(n, K);
    // every lane codes into its own region of 2 bytes per symbol, backwards, so that the bytes lie in decode order
    std::vector<uint8_t>  region(static_cast<size_t>(2 * n));
    std::vector<int64_t>  first(static_cast<size_t>(K)), count(static_cast<size_t>(K));
    std::vector<uint32_t> state(static_cast<size_t>(K));
    int64_t total = rans::kHeaderBytes + K * (width + rans::kStateBytes), end = 0;
    for (int64_t j = 0; j < K; ++j) {
        const int64_t m = rans::lane_symbols(n, K, j);
        end += 2 * m;
        int64_t  pos = end;
        uint32_t x = rans::kL;
        for (int64_t t = m - 1; t >= 0; --t) {
            const int64_t  i = j + t * K;
            const uint32_t c1 = rans::c1_of(p_one[i * p_stride]);
            const bool     one = x_pm1[i] > 0;
            const uint32_t f = one ? 0x10000u - c1 : c1, c = one ? c1 : 0u;
            while (x >= (f << 15)) {
                region[static_cast<size_t>(--pos)] = static_cast<uint8_t>(x & 0xFF);
                x >>= 8;
            }
            x = rans::push(x, f, c);
        }
        first[j] = pos;
        count[j] = end - pos;
        state[j] = x;
        total += count[j];
    }
    if (total > cap) return -1;
    if (out == nullptr) return -2;
    out[0] = static_cast<uint8_t>(rans::kFormatId);
    out[1] = static_cast<uint8_t>(width);
    put_le(out + 2, static_cast<uint64_t>(K), 4);
    int64_t at = rans::kHeaderBytes + K * width;
    for (int64_t j = 0; j < K; ++j) {
        put_le(out + rans::kHeaderBytes + j * width, static_cast<uint64_t>(count[j]), width);
        put_le(out + at, state[j], 4);
        if (count[j]) std::memcpy(out + at + 4, region.data() + first[j], static_cast<size_t>(count[j]));
        at += 4 + count[j];
    }
    return total;
}

extern "C" int64_t cnc_rans_check(const uint8_t* in, int64_t len, int64_t n)
{
    Header h;
    if (in == nullptr || parse(in, len, n, h) != 0) return -3;
    return h.K;
}

extern "C" int cnc_rans_decode_pm1_host(const float* p_one, int64_t p_stride, int64_t n, const uint8_t* in, int64_t len,
                                        float* x_pm1)
{
    Header h;
    if (in == nullptr || (p_stride != 0 && p_stride != 1) || parse(in, len, n, h) != 0) return -3;
    bool    good = true;
    int64_t at = h.payload;
    for (int64_t j = 0; j < h.K; ++j) {
        const int64_t cnt = static_cast<int64_t>(get_le(in + rans::kHeaderBytes + j * h.width, h.width));
        const uint8_t* sub = in + at + 4;              // parse(): [at, at + 4 + cnt) lies inside [0, len)
        uint32_t x = static_cast<uint32_t>(get_le(in + at, 4));
        int64_t  used = 0;
        good = good && x >= rans::kL && x < 0x80000000u;
        const int64_t m = rans::lane_symbols(n, h.K, j);
        for (int64_t t = 0; t < m; ++t) {
            const int64_t  i = j + t * h.K;
            const uint32_t c1 = rans::c1_of(p_one[i * p_stride]);
            const uint32_t slot = x & 0xFFFFu;
            const bool     one = slot >= c1;
            const uint32_t f = one ? 0x10000u - c1 : c1, c = one ? c1 : 0u;
            x_pm1[i] = one ? 1.0f : -1.0f;
            x = f * (x >> 16) + slot - c;
            // a well-formed lane needs at most two bytes here (the encoder left x >= f << 7); a state that is still
            // below L after two is the mark of a damaged stream, and is left as it is
            for (int r = 0; r < 2 && x < rans::kL; ++r) {
                x = (x << 8) | (used < cnt ? sub[used] : 0u);     // past the sub-stream: zeros
                ++used;
            }
        }
        good = good && x == rans::kL && used == cnt;
        at += 4 + cnt;
    }
    return good ? 0 : -3;
}
