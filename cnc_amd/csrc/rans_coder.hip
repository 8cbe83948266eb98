// rans_coder.hip — the device entropy coder: interleaved rANS over a table of streams ("rans1", include/cnc_codec.h,
// DESIGN §4.8).  One thread per rANS lane, one wave per block (a lane is a long dependent chain: waves are spread over
// the CUs rather than packed into blocks); a call codes every stream of its table in one launch (two for the encoder:
// the lanes, then the pass that lays the stream out).  The host twin, byte for byte: rans_coder.cpp.
#include "common.hpp"
#include "rans_format.hpp"

namespace cnc {

constexpr uint32_t kRansBatch = 24;          // streams per launch: their descriptors travel as a kernel argument
constexpr int      kRansAhead = 8;           // symbols of a lane whose p (and x) are fetched ahead of the state chain
constexpr uint32_t kRansDecodeBlocks = 256;  // per stream: the decoder learns K on the device and strides over the lane groups

struct RansBatch {
    cnc_rans_stream_t s[kRansBatch];
    uint64_t scratch_at[kRansBatch];         // encoder: the stream's part of the scratch
    uint32_t K[kRansBatch];                  // encoder: lanes
    uint32_t first_block[kRansBatch + 1];
    uint32_t n;                              // streams in this launch
    uint32_t first_stream;                   // index of s[0] in the caller's table (sizes_dev / status_dev)
};

// Encoder scratch of one stream: K x {bytes emitted, final state} (u32 each), then K regions of 2 * ceil(n / K) bytes,
// each filled from its end downwards.
__host__ __device__ inline uint64_t rans_lane_cap(int64_t n, int64_t K) { return 2ull * (uint64_t)rans::lane_symbols(n, K, 0); }
__host__ __device__ inline uint64_t rans_stream_scratch(int64_t n, int64_t K)
{
    return K == 0 ? 0 : ((8ull * (uint64_t)K + (uint64_t)K * rans_lane_cap(n, K) + 15ull) & ~15ull);
}

__device__ __forceinline__ uint32_t rans_stream_of_block(const RansBatch& b, uint32_t blk)
{
    uint32_t s = 0;
    while (s + 1 < b.n && blk >= b.first_block[s + 1]) s++;
    return s;
}

__global__ void __launch_bounds__(64) k_rans_encode_lanes(const RansBatch b, uint8_t* __restrict__ scratch)
{
    const uint32_t s = rans_stream_of_block(b, blockIdx.x);
    const int64_t  K = b.K[s], n = b.s[s].n;
    const int64_t  j = (int64_t)(blockIdx.x - b.first_block[s]) * 64 + threadIdx.x;
    if (j >= K) return;
    const float* __restrict__ p = b.s[s].p;
    const float* __restrict__ x = b.s[s].x;
    const int64_t  ps = b.s[s].p_stride;
    uint8_t*       mine = scratch + b.scratch_at[s];
    const uint64_t cap = rans_lane_cap(n, K);
    uint8_t*       end = mine + 8 * K + (uint64_t)(j + 1) * cap;
    uint8_t*       pos = end;
    const int64_t  m = rans::lane_symbols(n, K, j);
    uint32_t       st = rans::kL;
    // p and x of the next kRansAhead symbols are in flight while this batch's state updates run: a step of a lane is a new
    // cache line (the lanes of a wave read consecutive symbols), and only `st` is a chain
    float pb[kRansAhead], xb[kRansAhead];
    auto fetch = [&](int64_t t_hi, float (&pp)[kRansAhead], float (&xx)[kRansAhead]) {
#pragma unroll
        for (int k = 0; k < kRansAhead; k++) {
            const int64_t t = t_hi - k, i = j + (t < 0 ? 0 : t) * K;      // past the lane's first symbol: symbol 0 again, unused
            pp[k] = p[i * ps];
            xx[k] = x[i];
        }
    };
    fetch(m - 1, pb, xb);
    for (int64_t t_hi = m - 1; t_hi >= 0; t_hi -= kRansAhead) {
        float pn[kRansAhead], xn[kRansAhead];
        const bool more = t_hi >= kRansAhead;
        if (more) fetch(t_hi - kRansAhead, pn, xn);
#pragma unroll
        for (int k = 0; k < kRansAhead; k++) {
            if (t_hi - k < 0) break;
            const uint32_t c1 = rans::c1_of(pb[k]);
            const bool     one = xb[k] > 0;
            const uint32_t f = one ? 0x10000u - c1 : c1, c = one ? c1 : 0u;
            const uint32_t lim = f << 15;
            if (st >= lim) {              // at most twice: st < 2^31, lim >= 2^15
                *--pos = (uint8_t)st;
                st >>= 8;
                if (st >= lim) {
                    *--pos = (uint8_t)st;
                    st >>= 8;
                }
            }
            st = rans::push(st, f, c);
        }
        if (more) {
#pragma unroll
            for (int k = 0; k < kRansAhead; k++) {
                pb[k] = pn[k];
                xb[k] = xn[k];
            }
        }
    }
    uint32_t* meta = reinterpret_cast<uint32_t*>(mine);
    meta[2 * j] = (uint32_t)(end - pos);
    meta[2 * j + 1] = st;
}

// Lays a stream out: header, directory, then every lane's state and bytes at the running sum of the lanes before
// it.  Block g of a stream places lanes 64 g .. 64 g + 63; every block sums the directory for itself.
__global__ void __launch_bounds__(256) k_rans_pack(const RansBatch b, const uint8_t* __restrict__ scratch, int64_t* __restrict__ sizes)
{
    __shared__ uint64_t red[2][256];
    __shared__ uint64_t lane_at[64];
    const uint32_t s = rans_stream_of_block(b, blockIdx.x);
    const int64_t  K = b.K[s], n = b.s[s].n, cap_out = b.s[s].cap_or_len;
    const uint32_t g = blockIdx.x - b.first_block[s];
    const int64_t  j0 = (int64_t)g * 64;
    const uint8_t* mine = scratch + b.scratch_at[s];
    const uint32_t* meta = reinterpret_cast<const uint32_t*>(mine);
    const uint32_t tid = threadIdx.x;
    uint64_t before = 0, all = 0;
    for (int64_t i = tid; i < K; i += 256) {
        const uint64_t v = (uint64_t)meta[2 * i] + rans::kStateBytes;
        all += v;
        if (i < j0) before += v;
    }
    red[0][tid] = before;
    red[1][tid] = all;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (tid < h) {
            red[0][tid] += red[0][tid + h];
            red[1][tid] += red[1][tid + h];
        }
        __syncthreads();
    }
    before = red[0][0];
    all = red[1][0];
    const uint32_t w = rans::dir_width(n, K);
    const uint64_t payload = rans::kHeaderBytes + (uint64_t)K * w;
    const uint64_t total = payload + all;
    const bool     fits = cap_out >= 0 && total <= (uint64_t)cap_out;
    if (g == 0 && tid == 0) sizes[b.first_stream + s] = fits ? (int64_t)total : -1;
    if (!fits) return;                        // nothing of this stream is written
    uint8_t* out = b.s[s].bytes;
    if (g == 0) {
        if (tid == 0) {
            out[0] = (uint8_t)rans::kFormatId;
            out[1] = (uint8_t)w;
            for (uint32_t k = 0; k < 4; k++) out[2 + k] = (uint8_t)((uint32_t)K >> (8 * k));
        }
        for (int64_t i = tid; i < K; i += 256) {
            const uint32_t v = meta[2 * i];
            for (uint32_t k = 0; k < w; k++) out[rans::kHeaderBytes + i * w + k] = (uint8_t)(v >> (8 * k));
        }
    }
    if (tid == 0) {                           // 64 lanes: a serial running sum
        uint64_t at = payload + before;
        for (uint32_t l = 0; l < 64 && j0 + l < K; l++) {
            lane_at[l] = at;
            at += (uint64_t)meta[2 * (j0 + l)] + rans::kStateBytes;
        }
    }
    __syncthreads();
    const uint64_t lane_cap = rans_lane_cap(n, K);
    const uint32_t wave = tid >> 6, l64 = tid & 63;
    for (uint32_t l = wave; l < 64 && j0 + l < K; l += 4) {
        const int64_t  j = j0 + l;
        const uint32_t cnt = meta[2 * j], st = meta[2 * j + 1];
        uint8_t*       dst = out + lane_at[l];
        const uint8_t* src = mine + 8 * K + (uint64_t)(j + 1) * lane_cap - cnt;
        if (l64 < 4) dst[l64] = (uint8_t)(st >> (8 * l64));
        for (uint32_t k = l64; k < cnt; k += 64) dst[4 + k] = src[k];
    }
}

// Bytes of [lo, hi) as seen through aligned 32-bit words: a word wholly inside is one load, a word that straddles an
// end is put together from the bytes inside, the rest of it zeros.  Nothing outside [lo, hi) is read.
__device__ __forceinline__ uint32_t rans_word(uintptr_t a, uintptr_t lo, uintptr_t hi)
{
    if (a >= lo && a + 4 <= hi) return *reinterpret_cast<const uint32_t*>(a);
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (a + k >= lo && a + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + k)) << (8 * k);
    return v;
}

// The next bytes of a lane's sub-stream in registers: 4 .. 8 in `win`, one more word already requested.  The refill
// depends on how many bytes were taken, never on the loaded values, so its latency stays off the chain on the state.
struct RansWindow {
    uint64_t  win;
    uint32_t  nb, nxt;
    uintptr_t a, lo, hi;
    __device__ __forceinline__ void open(uintptr_t lo_, uintptr_t hi_)
    {
        lo = lo_;
        hi = hi_ > lo_ ? hi_ : lo_;
        a = lo & ~(uintptr_t)3;
        const uint32_t skip = (uint32_t)(lo - a);
        win = (uint64_t)rans_word(a, lo, hi) >> (8 * skip);
        nb = 4 - skip;
        nxt = rans_word(a + 4, lo, hi);
        a += 8;
        refill();
    }
    __device__ __forceinline__ void refill()
    {
        if (nb <= 4) {
            win |= (uint64_t)nxt << (8 * nb);
            nb += 4;
            nxt = rans_word(a, lo, hi);
            a += 4;
        }
    }
    __device__ __forceinline__ uint32_t take()
    {
        const uint32_t v = (uint32_t)win & 0xFFu;
        win >>= 8;
        nb--;
        return v;
    }
};

__device__ __forceinline__ uint64_t rans_dir_entry(const uint8_t* __restrict__ in, int64_t i, uint32_t w)
{
    uint32_t v = 0;
    for (uint32_t k = 0; k < w; k++) v |= (uint32_t)in[rans::kHeaderBytes + i * w + k] << (8 * k);
    return v;
}

__device__ __forceinline__ uint64_t rans_wave_sum(uint64_t v)
{
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ void __launch_bounds__(64) k_rans_decode(const RansBatch b, int32_t* __restrict__ status)
{
    const uint32_t s = rans_stream_of_block(b, blockIdx.x);
    const uint32_t g0 = blockIdx.x - b.first_block[s], n_blocks = b.first_block[s + 1] - b.first_block[s];
    const int64_t  n = b.s[s].n, len = b.s[s].cap_or_len;
    const uint8_t* __restrict__ in = b.s[s].bytes;
    const float* __restrict__   p = b.s[s].p;
    float* __restrict__         x = b.s[s].x;
    const int64_t  ps = b.s[s].p_stride;
    const uint32_t tid = threadIdx.x;
    int32_t* bad = status + b.first_stream + s;
    // header (cnc_rans_check has passed on the host; a stream that fails here is refused whole)
    bool     ok = len >= (int64_t)rans::kHeaderBytes;
    uint32_t w = 1;
    int64_t  K = 0;
    if (ok) {
        w = in[1];
        K = (int64_t)((uint32_t)in[2] | (uint32_t)in[3] << 8 | (uint32_t)in[4] << 16 | (uint32_t)in[5] << 24);
        ok = in[0] == rans::kFormatId && w >= 1 && w <= 4 && K <= n && (K == 0) == (n == 0) &&
             K <= (len - (int64_t)rans::kHeaderBytes) / (int64_t)w;
    }
    if (!ok) {
        if (g0 == 0 && tid == 0) *bad = -3;
        return;
    }
    const uint64_t payload = rans::kHeaderBytes + (uint64_t)K * w;
    for (int64_t grp = g0; grp * 64 < K; grp += n_blocks) {
        const int64_t j0 = grp * 64, j = j0 + tid;
        uint64_t before = 0;
        for (int64_t i = tid; i < j0; i += 64) before += rans_dir_entry(in, i, w) + rans::kStateBytes;
        before = rans_wave_sum(before);
        const uint64_t cnt = j < K ? rans_dir_entry(in, j, w) : 0;
        uint64_t incl = j < K ? cnt + rans::kStateBytes : 0;          // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = __shfl_up((uint32_t)incl, d, 64), hi = __shfl_up((uint32_t)(incl >> 32), d, 64);
            if (tid >= (uint32_t)d) incl += ((uint64_t)hi << 32) | lo;
        }
        if (j >= K) continue;
        const uint64_t start = payload + before + incl - (cnt + rans::kStateBytes);
        // the lane's bytes, clamped to the stream
        const uint64_t ulen = (uint64_t)len;
        const uint64_t lo_at = start < ulen ? start : ulen;
        const uint64_t hi_at = start + rans::kStateBytes + cnt < ulen ? start + rans::kStateBytes + cnt : ulen;
        RansWindow rd;
        rd.open((uintptr_t)in + lo_at, (uintptr_t)in + hi_at);
        uint32_t st = rd.take();
        st |= rd.take() << 8;
        st |= rd.take() << 16;
        st |= rd.take() << 24;
        rd.refill();
        bool     good = st >= rans::kL && st < 0x80000000u && hi_at - lo_at == rans::kStateBytes + cnt;
        uint64_t used = 0;
        const int64_t m = rans::lane_symbols(n, K, j);
        float pb[kRansAhead];
        auto fetch = [&](int64_t t_lo, float (&pp)[kRansAhead]) {
#pragma unroll
            for (int k = 0; k < kRansAhead; k++) {
                const int64_t t = t_lo + k;
                pp[k] = p[(j + (t < m ? t : m - 1) * K) * ps];           // past the lane's last symbol: that one again, unused
            }
        };
        fetch(0, pb);
        for (int64_t t_lo = 0; t_lo < m; t_lo += kRansAhead) {
            float pn[kRansAhead];
            const bool more = t_lo + kRansAhead < m;
            if (more) fetch(t_lo + kRansAhead, pn);
#pragma unroll
            for (int k = 0; k < kRansAhead; k++) {
                if (t_lo + k >= m) break;
                const uint32_t c1 = rans::c1_of(pb[k]);
                const uint32_t slot = st & 0xFFFFu;
                const bool     one = slot >= c1;
                const uint32_t f = one ? 0x10000u - c1 : c1, c = one ? c1 : 0u;
                x[j + (t_lo + k) * K] = one ? 1.0f : -1.0f;
                st = f * (st >> 16) + slot - c;
                if (st < rans::kL) {          // at most two bytes in a well-formed lane; past the sub-stream: zeros
                    st = (st << 8) | rd.take();
                    used++;
                    if (st < rans::kL) {
                        st = (st << 8) | rd.take();
                        used++;
                    }
                }
                rd.refill();
            }
            if (more) {
#pragma unroll
                for (int k = 0; k < kRansAhead; k++) pb[k] = pn[k];
            }
        }
        good = good && st == rans::kL && used == cnt;
        if (!good) *bad = -3;
    }
}

// the table (HOST memory) -> launches of up to kRansBatch streams; `blocks_of` gives a stream's block count
template <typename Fill, typename Launch>
int rans_for_batches(const cnc_rans_stream_t* streams, uint32_t n_streams, Fill fill, Launch launch)
{
    for (uint32_t s0 = 0; s0 < n_streams; s0 += kRansBatch) {
        RansBatch b = {};
        b.n = n_streams - s0 < kRansBatch ? n_streams - s0 : kRansBatch;
        b.first_stream = s0;
        uint64_t blocks = 0;
        for (uint32_t k = 0; k < b.n; k++) {
            b.s[k] = streams[s0 + k];
            b.first_block[k] = (uint32_t)blocks;
            blocks += fill(b, k, s0 + k);
            if (blocks > 0x7fffffffull) return CNC_ERR_INVALID_VALUE;
        }
        b.first_block[b.n] = (uint32_t)blocks;
        launch(b, (uint32_t)blocks);
        if (launch_status() != CNC_OK) return CNC_ERR_LAUNCH;
    }
    return CNC_OK;
}

inline bool rans_stream_ok(const cnc_rans_stream_t& t, bool encode)
{
    if (t.n < 0 || t.cap_or_len < 0 || (t.p_stride != 0 && t.p_stride != 1)) return false;
    if (encode && (t.symbols_per_lane < 1 || rans::lanes_of(t.n, t.symbols_per_lane) > 0xFFFFFFFFll)) return false;
    if (t.n > 0 && (!t.p || !t.x)) return false;
    if (t.cap_or_len > 0 && !t.bytes) return false;
    return true;
}

}  // namespace cnc

extern "C" uint64_t cnc_rans_scratch_bytes(const cnc_rans_stream_t* streams, uint32_t n_streams)
{
    uint64_t total = 0;
    if (!streams) return 0;
    for (uint32_t s = 0; s < n_streams; s++) {
        if (!cnc::rans_stream_ok(streams[s], true)) return 0;
        total += cnc::rans_stream_scratch(streams[s].n, rans::lanes_of(streams[s].n, streams[s].symbols_per_lane));
    }
    return total;
}

extern "C" int cnc_rans_encode_pm1(const cnc_rans_stream_t* streams, uint32_t n_streams, void* scratch, uint64_t scratch_bytes,
                                   int64_t* sizes_dev, void* stream)
{
    if (n_streams == 0) return CNC_OK;
    if (!streams || !sizes_dev) return CNC_ERR_INVALID_VALUE;
    for (uint32_t s = 0; s < n_streams; s++)
        if (!cnc::rans_stream_ok(streams[s], true)) return CNC_ERR_INVALID_VALUE;
    const uint64_t need = cnc_rans_scratch_bytes(streams, n_streams);
    if (scratch_bytes < need || (need && (!scratch || ((uintptr_t)scratch & 15)))) return CNC_ERR_INVALID_VALUE;
    uint64_t at = 0;
    auto fill = [&](cnc::RansBatch& b, uint32_t k, uint32_t) -> uint64_t {
        const int64_t K = rans::lanes_of(b.s[k].n, b.s[k].symbols_per_lane);
        b.K[k] = (uint32_t)K;
        b.scratch_at[k] = at;
        at += cnc::rans_stream_scratch(b.s[k].n, K);
        return K == 0 ? 1 : (uint64_t)((K + 63) / 64);       // an empty stream still gets its header written
    };
    auto launch = [&](const cnc::RansBatch& b, uint32_t blocks) {
        hipLaunchKernelGGL(cnc::k_rans_encode_lanes, dim3(blocks), dim3(64), 0, (hipStream_t)stream, b, (uint8_t*)scratch);
        hipLaunchKernelGGL(cnc::k_rans_pack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b, (const uint8_t*)scratch, sizes_dev);
    };
    return cnc::rans_for_batches(streams, n_streams, fill, launch);
}

extern "C" int cnc_rans_decode_pm1(const cnc_rans_stream_t* streams, uint32_t n_streams, int32_t* status_dev, void* stream)
{
    if (n_streams == 0) return CNC_OK;
    if (!streams || !status_dev) return CNC_ERR_INVALID_VALUE;
    for (uint32_t s = 0; s < n_streams; s++)
        if (!cnc::rans_stream_ok(streams[s], false)) return CNC_ERR_INVALID_VALUE;
    if (hipMemsetAsync(status_dev, 0, sizeof(int32_t) * n_streams, (hipStream_t)stream) != hipSuccess) return CNC_ERR_LAUNCH;
    auto fill = [&](cnc::RansBatch& b, uint32_t k, uint32_t) -> uint64_t {
        const uint64_t groups = (uint64_t)((b.s[k].n + 63) / 64);
        return groups < 1 ? 1 : (groups < cnc::kRansDecodeBlocks ? groups : cnc::kRansDecodeBlocks);
    };
    auto launch = [&](const cnc::RansBatch& b, uint32_t blocks) {
        hipLaunchKernelGGL(cnc::k_rans_decode, dim3(blocks), dim3(64), 0, (hipStream_t)stream, b, status_dev);
    };
    return cnc::rans_for_batches(streams, n_streams, fill, launch);
}
