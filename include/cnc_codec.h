/*
 * cnc_codec.h — C ABI of libcnc_codec.so: the CPU entropy coder for the ±1 hash-grid embeddings.
 *
 * Replaces the reference's use of torchac==0.9.3 (requirements.txt:32) behind
 * `encoder(x, p, file_name)` / `decoder(p, file_name)` (examples/utils_bpp_acc.py:77-110):
 *     torchac.encode_float_cdf(cat([0, 1-p, 1]), sym=(x+1)//2)   ->  cnc_rc_encode_pm1
 *     torchac.decode_float_cdf(cat([0, 1-p, 1]), bytes) * 2 - 1   ->  cnc_rc_decode_pm1
 * The coder is sequential and runs on the host in the reference as well (torchac is a CPU
 * extension fed by .cpu() copies); it is not part of the GPU data path.
 *
 * Bitstream: torchac's published format — 16-bit CDF c1 = round_half_even((1-p)*65534)+1,
 * 32-bit low/high interval coder with pending-bit carry resolution, MSB-first, one terminating
 * bit (+pending), zero padded to a byte.  torchac itself is absent from the reference tree, so
 * byte-level parity with it is UNPINNED; round-trip exactness and size-vs-entropy are tested.
 */
#ifndef CNC_CODEC_H
#define CNC_CODEC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Upper bound of the encoded size in bytes for n symbols (worst case 16 bits/symbol + tail). */
int64_t cnc_rc_bound(int64_t n);

/* The 16-bit quantity the pm1 coders derive from a probability: c1 = P(x=-1) * 2^16, what cnc_rc_encode_pm1 /
 * cnc_rc_decode_pm1 narrow with (cnc_rc_c1) and what the rans1 coders code with (cnc_rans_c1, clamped to [1, 65535]).
 * Exported so that a caller that stores c1 itself (the occupancy pyramid's tables) can check that the
 * float it hands over gives that c1 back. */
uint32_t cnc_rc_c1(float p_one);
uint32_t cnc_rans_c1(float p_one);

/* x_pm1[i] in {-1,+1} (any value > 0 codes as +1), p_one[i] = P(x=+1) in (0,1).
 * Returns the number of bytes written, or -1 if cap < cnc_rc_bound(n) was too small. */
int64_t cnc_rc_encode_pm1(const float* p_one, const float* x_pm1, int64_t n, uint8_t* out,
                          int64_t cap);

/* Inverse: fills x_pm1[0..n) with -1.0f / +1.0f.  Returns 0. */
int cnc_rc_decode_pm1(const float* p_one, int64_t n, const uint8_t* in, int64_t len,
                      float* x_pm1);

/* General alphabets — what `torchac.encode_int16_normalized_cdf(cdf_int, sym)` / `decode_int16_normalized_cdf`
 * bind (and, after the float -> 16-bit conversion done by the Python shim cnc_amd/backends/torchac.py exactly as
 * torchac's `_convert_to_int_and_normalize` publishes it, `encode_float_cdf` / `decode_float_cdf`, the two calls of
 * examples/utils_bpp_acc.py:87,108).  cdf: [n, Lp] uint16 rows, row[0] = 0, non-decreasing, the LAST entry stands
 * for 2^16 whatever it holds (torchac stores 65536 wrapped to 0); sym[i] in [0, Lp-2].
 * encode: bytes written, -1 if cap < cnc_rc_bound(n), -2 for a symbol outside the alphabet.  decode: 0 / -2. */
int64_t cnc_rc_encode_cdf16(const uint16_t* cdf, const int16_t* sym, int64_t n, int32_t Lp, uint8_t* out,
                            int64_t cap);
int cnc_rc_decode_cdf16(const uint16_t* cdf, int64_t n, int32_t Lp, const uint8_t* in, int64_t len,
                        int16_t* sym);

/* ---- "rans1": the stream format of the device entropy coder (cnc_rans_encode_pm1 / cnc_rans_decode_pm1 of
 * cnc_hip.h) and its host twin below.  A second coder next to the range coder above, for the same ±1 symbols and
 * probabilities; the two formats are unrelated, and a container says which one wrote it.
 *
 * Probabilities: c1 = clamp(rint((1 - p) * 65534), 0, 65534) + 1 in float32, round half to even, NaN -> 32768 — the
 *   range coder's quantisation.  P(-1) = c1 / 2^16, P(+1) = (2^16 - c1) / 2^16; both frequencies are >= 1.
 * Lanes: n symbols at S symbols per lane are coded by K = ceil(n / S) independent lanes (K = 0 for n = 0); lane j
 *   codes the symbols j, j + K, j + 2K, ...
 * A lane: rANS, 32-bit state, byte renormalisation, 16 probability bits, L = 2^23.  With (f, c) = (2^16 - c1, c1) for
 *   +1 and (c1, 0) for -1 the encoder starts at x = L and takes its symbols LAST TO FIRST:
 *       while (x >= f << 15) { emit(x & 0xFF); x >>= 8; }      x = ((x / f) << 16) + x % f + c;
 *   the decoder starts from the stored state and takes them first to last:
 *       slot = x & 0xFFFF; one = slot >= c1; x = f * (x >> 16) + slot - c; while (x < L) x = x << 8 | next_byte;
 *   reading the bytes in the reverse of the order they were emitted — at most two per symbol.  x stays below 2^31.
 *   After its last symbol a lane is back at x = L and has read all its bytes: the integrity check.
 * Layout: byte 0 the format id 0x72, byte 1 the directory entry width w in 1..4, bytes 2..5 K (u32 LE); K directory
 *   entries of w bytes LE, the number of renormalisation bytes of each lane; then the lanes' sub-streams in lane
 *   order: the final state (u32 LE), then the lane's bytes in the order the decoder reads them.  w is the smallest
 *   width that holds 2 * ceil(n / K), the most a lane can emit, so a stream is a function of (p, x, n, S) alone.
 *   n is not stored: the decoder knows it from p, as with the range coder.
 * Size: 8 * bytes <= ideal_q + 40 K + 8 (6 + K w) + a rounding term, ideal_q = sum -log2(f_i / 2^16)
 *   (tests/test_rans_twin.py holds it to 1.002 ideal_q + 64).                                                      */

/* Upper bound of the encoded size in bytes (2 bytes per symbol + headers), -1 for n < 0 or symbols_per_lane < 1. */
int64_t cnc_rans_bound(int64_t n, int64_t symbols_per_lane);

/* x_pm1[i] > 0 codes as +1; P(+1) of symbol i is p_one[i * p_stride], p_stride 0 (one probability for the whole
 * stream) or 1.  Returns the bytes written, -1 if cap is too small (nothing is written then), -2 for bad arguments. */
int64_t cnc_rans_encode_pm1_host(const float* p_one, int64_t p_stride, const float* x_pm1, int64_t n,
                                 int64_t symbols_per_lane, uint8_t* out, int64_t cap);

/* Fills x_pm1[0..n) with -1.0f / +1.0f.  0, or -3 for a stream that fails cnc_rans_check or whose lanes do not all
 * end at L with their bytes used up.  Whatever `in` holds, nothing outside in[0, len) is read and nothing outside
 * x_pm1[0, n) written; a lane that runs off its sub-stream reads zeros. */
int cnc_rans_decode_pm1_host(const float* p_one, int64_t p_stride, int64_t n, const uint8_t* in, int64_t len,
                             float* x_pm1);

/* Header and directory of in[0, len) as a stream of n symbols: the format id, 1 <= w <= 4, K <= n, K = 0 only for
 * n = 0, and header + directory + every lane's state and bytes fit len.  Returns K, or -3. */
int64_t cnc_rans_check(const uint8_t* in, int64_t len, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
