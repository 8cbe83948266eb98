"""CPU-only: the host twin of the device entropy coder (cnc_amd/csrc/rans_coder.cpp, libcnc_codec.so) against the NumPy
restatement of the "rans1" format in tests/rans_twin.py: same bytes, each decodes the other, the size bound, the worst
case, and malformed streams."""
import numpy as np
import pytest

import rans_twin as tw


@pytest.fixture(scope="module")
def lib():
    from cnc_amd import build
    build.build_codec()
    from cnc_amd import _codec
    return _codec.lib()


def host_encode(L, p, x, S, cap=None):
    """(bytes written or negative code, buffer).  p of one element: p_stride = 0."""
    p = np.ascontiguousarray(p, np.float32).reshape(-1)
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    stride = 0 if (p.size == 1 and x.size != 1) else 1
    cap = int(L.cnc_rans_bound(x.size, S)) if cap is None else cap
    buf = np.full(cap + 16, 0xA5, np.uint8)
    got = L.cnc_rans_encode_pm1_host(p.ctypes.data, stride, x.ctypes.data, x.size, S, buf.ctypes.data, cap)
    assert np.all(buf[max(cap, 0):] == 0xA5), "wrote past cap"
    if got >= 0:
        assert np.all(buf[got:] == 0xA5)
    return got, buf


def host_decode(L, p, n, stream):
    p = np.ascontiguousarray(p, np.float32).reshape(-1)
    stride = 0 if (p.size == 1 and n != 1) else 1
    s = np.frombuffer(bytes(stream), np.uint8).copy()
    out = np.full(n + 8, 7.0, np.float32)
    rc = L.cnc_rans_decode_pm1_host(p.ctypes.data, stride, n, s.ctypes.data, s.size, out.ctypes.data)
    assert np.all(out[n:] == 7.0), "wrote past x_out[n)"
    return rc, out[:n]


def draw(rng, p, n):
    return np.where(rng.uniform(size=n) < np.broadcast_to(p, (n,)), 1.0, -1.0).astype(np.float32)


def extreme(n):
    """The pattern of test_range_coder_roundtrip_and_size: 1e-6 / 1 - 1e-6 with likely and unlikely symbols."""
    p = np.resize(np.array([1e-6, 1 - 1e-6, 1e-6, 1 - 1e-6, 0.5], np.float32), n)
    x = np.resize(np.array([1, -1, -1, 1, 1], np.float32), n)
    return p, x


def tie_sweep():
    """A dense sweep of p with each value's float32 neighbours: the rounding ties of c1 lie at (1 - p) * 65534 = k + 1/2."""
    k = np.arange(0, 65534, 7, dtype=np.float64)
    base = (1.0 - (k + 0.5) / 65534.0).astype(np.float32)
    p = np.concatenate([np.nextafter(base, np.float32(0)), base, np.nextafter(base, np.float32(1)),
                        np.array([0.0, 1.0, 1e-6, 1 - 1e-6, 0.5, -0.25, 1.5, np.nan], np.float32)])
    return p.astype(np.float32)


CASES = [(n, 16) for n in (0, 1, 2, 15, 16, 17, 1029, 20000)] + [(100000, 1024), (100000, 4096)]


def _both_ways(L, p, x, S):
    n = x.size
    want = tw.encode(p, x, S)
    got, buf = host_encode(L, p, x, S)
    assert got == len(want) and buf[:got].tobytes() == want
    assert L.cnc_rans_check(buf.ctypes.data, got, n) == tw.lanes(n, S) == tw.check(want, n)
    rc, back = host_decode(L, p, n, want)                 # the library decodes the twin's bytes
    assert rc == 0 and np.array_equal(back, x)
    st, back = tw.decode(p, n, buf[:got].tobytes())       # the twin decodes the library's
    assert st == 0 and np.array_equal(back, x)
    return got


@pytest.mark.parametrize("n,S", CASES)
def test_same_bytes_and_round_trip_uniform(lib, n, S):
    rng = np.random.default_rng(n + S)
    p = rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32)
    x = draw(rng, p, n)
    nbytes = _both_ways(lib, p, x, S)
    if n >= 20000:
        K = tw.lanes(n, S)
        ideal = tw.ideal_bits(p, x)
        assert ideal <= 8 * nbytes <= 1.002 * ideal + 40 * K + 8 * (6 + K * tw.dir_width(n, K)) + 64


@pytest.mark.parametrize("n,S", CASES)
def test_same_bytes_and_round_trip_extreme(lib, n, S):
    p, x = extreme(n)
    nbytes = _both_ways(lib, p, x, S)
    if n >= 20000:
        K = tw.lanes(n, S)
        ideal = tw.ideal_bits(p, x)
        assert ideal <= 8 * nbytes <= 1.002 * ideal + 40 * K + 8 * (6 + K * tw.dir_width(n, K)) + 64


@pytest.mark.parametrize("n,S", CASES)
@pytest.mark.parametrize("pg", [0.5, 0.999, 0.031])
def test_same_bytes_and_round_trip_one_probability(lib, n, S, pg):
    """p_stride = 0: one Pg for the whole stream, as for the levels coded without a context."""
    rng = np.random.default_rng(n + S + 1)
    p = np.array([pg], np.float32)
    x = draw(rng, p, n)
    nbytes = _both_ways(lib, p, x, S)
    if n > 1:                                             # the same stream from expanded probabilities
        got, buf = host_encode(lib, np.full(n, pg, np.float32), x, S)
        assert got == nbytes and buf[:got].tobytes() == tw.encode(p, x, S)
    if n >= 20000:
        K = tw.lanes(n, S)
        ideal = tw.ideal_bits(p, x)
        assert ideal <= 8 * nbytes <= 1.002 * ideal + 40 * K + 8 * (6 + K * tw.dir_width(n, K)) + 64


# (n, S, directory width): the default lane length, either side of both width boundaries (a lane of m symbols emits at
# most 2 m bytes: 2 * 128 and 2 * 32768 no longer fit one and two bytes), and one symbol per lane
LANE_CASES = [(100000, 16384, 2), (3 * 32768, 32768, 3), (3 * 32767, 32767, 2), (313 * 128, 128, 2), (313 * 127, 127, 1),
              (16454, 1, 1)]


@pytest.mark.parametrize("pattern", ["uniform", "worst"])
@pytest.mark.parametrize("n,S,w", LANE_CASES)
def test_same_bytes_and_round_trip_at_the_directory_width_boundaries(lib, n, S, w, pattern):
    """`worst` is two bytes for every symbol: the longest lane's count is the largest value its width has to hold, so a
    boundary one step too high would truncate the entry and the stream would not decode."""
    if pattern == "uniform":
        rng = np.random.default_rng(n + S)
        p = rng.uniform(1e-6, 1 - 1e-6, size=n).astype(np.float32)
        x = draw(rng, p, n)
    else:
        p, x = np.full(n, 1.0, np.float32), -np.ones(n, np.float32)
    K = tw.lanes(n, S)
    assert tw.dir_width(n, K) == w
    nbytes = _both_ways(lib, p, x, S)
    got, buf = host_encode(lib, p, x, S)
    assert got == nbytes and buf[0] == tw.FORMAT_ID and buf[1] == w and int.from_bytes(buf[2:6].tobytes(), "little") == K
    at, cnt = tw.lane_starts(buf[:got].tobytes())
    assert len(cnt) == K and at[-1] + 4 + cnt[-1] == got
    if pattern == "worst":
        assert nbytes == tw.bound(n, S) == int(lib.cnc_rans_bound(n, S))
        assert cnt.max() == 2 * -(-n // K) and (w == 1 or cnt.max() >= 1 << (8 * (w - 1)))


def test_quantisation_ties(lib):
    """c1 over the sweep: the twin's and the library's streams agree symbol for symbol, so a tie rounded the other way
    (or a fused multiply-subtract) would change bytes; c1 itself against exact rational arithmetic."""
    p = tie_sweep()
    c1 = tw.c1_of(p)
    assert c1.min() >= 1 and c1.max() <= 65535 and c1[-1] == 32768
    from fractions import Fraction
    for v, c in list(zip(p[:3000:13], c1[:3000:13])) + list(zip(p[-8:-1], c1[-8:-1])):
        u = np.float32(1.0) - np.float32(v)                          # float32 subtraction, then float32 product
        prod = np.float32(u * np.float32(65534.0))
        r = round(Fraction(float(prod)))                             # Python rounds exact halves to even
        assert c == min(max(r, 0), 65534) + 1
    rng = np.random.default_rng(3)
    for x in (draw(rng, np.nan_to_num(np.clip(p, 0, 1), nan=0.5), p.size), np.ones(p.size, np.float32), -np.ones(p.size, np.float32)):
        _both_ways(lib, p, x, 16)
        _both_ways(lib, p, x, 4096)


@pytest.mark.parametrize("n,S", [(1025, 16), (20000, 16), (5000, 4096)])
def test_worst_case_fits_the_bound_and_a_short_cap_is_refused(lib, n, S):
    """Every symbol the improbable one at f = 1: two bytes per symbol."""
    p = np.full(n, 1.0, np.float32)                       # c1 = 1: P(-1) = 1 / 2^16
    x = -np.ones(n, np.float32)
    assert int(tw.c1_of(p[:1])[0]) == 1
    bound = int(lib.cnc_rans_bound(n, S))
    assert bound == tw.bound(n, S)
    got = _both_ways(lib, p, x, S)
    assert got == bound                                   # x = 2^23 -> two bytes -> 2^7 -> push -> 2^23, every symbol
    short, buf = host_encode(lib, p, x, S, cap=got - 1)
    assert short == -1 and np.all(buf == 0xA5)            # nothing written at all
    exact, _ = host_encode(lib, p, x, S, cap=got)
    assert exact == got


def malformed_cases():
    """name -> (p, n, bytes, must_fail_check): streams the decoder has to refuse or survive."""
    rng = np.random.default_rng(11)
    n, S = 1029, 16
    p = rng.uniform(0.02, 0.98, size=n).astype(np.float32)
    x = draw(rng, p, n)
    good = bytearray(tw.encode(p, x, S))
    K, w = tw.lanes(n, S), tw.dir_width(n, tw.lanes(n, S))
    out = {"truncated": (p, n, bytes(good[:len(good) - 5]), True),
           "truncated_in_directory": (p, n, bytes(good[:6 + K // 2]), True),
           "header_only": (p, n, bytes(good[:6]), True),
           "short_header": (p, n, bytes(good[:3]), True)}
    big = bytearray(good)
    big[6 + 3 * w] = 0xFF                                  # one entry larger than the whole stream
    out["directory_sum"] = (p, n, bytes(big), True)
    many = bytearray(good)
    many[2:6] = (n + 1).to_bytes(4, "little")
    out["more_lanes_than_symbols"] = (p, n, bytes(many), True)
    huge = bytearray(good)
    huge[2:6] = (0xFFFFFFFF).to_bytes(4, "little")
    out["lanes_overflow"] = (p, n, bytes(huge), True)
    none = bytearray(good)
    none[2:6] = (0).to_bytes(4, "little")
    out["no_lanes"] = (p, n, bytes(none), True)
    for name, at, val in (("bad_id", 0, 0x00), ("bad_width", 1, 9), ("zero_width", 1, 0)):
        b = bytearray(good)
        b[at] = val
        out[name] = (p, n, bytes(b), True)
    flip = bytearray(good)
    flip[len(good) // 2] ^= 0x10
    out["flipped_payload_byte"] = (p, n, bytes(flip), False)
    st = bytearray(good)
    st[6 + K * w + 3] = 0xFF                              # lane 0's stored state >= 2^31
    out["state_out_of_range"] = (p, n, bytes(st), False)
    shift = bytearray(good)                                # one byte moved from lane 1 to lane 0: the sum still fits
    shift[6] += 1
    shift[6 + w] -= 1
    out["directory_shifted"] = (p, n, bytes(shift), False)
    return out, x


MALFORMED, MALFORMED_X = malformed_cases()


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_streams(lib, name):
    p, n, stream, fails_check = MALFORMED[name]
    s = np.frombuffer(stream, np.uint8).copy()
    # the stream sits at the very end of its allocation's used part, followed by a guard the decoder must not need
    k = lib.cnc_rans_check(s.ctypes.data, s.size, n)
    rc, back = host_decode(lib, p, n, stream)
    st, tback = tw.decode(p, n, stream)
    if fails_check:
        assert k == -3 and rc == -3 and st == -3 and tw.check(stream, n) == -3
    else:
        assert k == tw.lanes(n, 16)
        assert rc == st
        assert rc == -3 or not np.array_equal(back, MALFORMED_X)
        assert np.array_equal(back, tback)                # zeros past a sub-stream, on both sides


# damage -> (passes cnc_rans_check, status of the decoder): what a decoder that has only (p, n, bytes, len) must say
DAMAGE = {"payload_bit": (True, -3), "state_high": (True, -3), "state_low": (True, -3), "directory_shift": (True, -3),
          "trailing_bytes": (True, 0), "one_byte_short": (False, -3), "directory_only": (False, -3), "five_bytes": (False, -3),
          "more_lanes_than_symbols": (False, -3), "no_lanes": (False, -3), "zero_width": (False, -3), "width_five": (False, -3),
          "format_id": (False, -3)}


def damage(name, good, n):
    """(buffer, len) from the sound stream `good` of n symbols at w = 1: the decoder is handed buffer[:len]; the buffer is
    never shorter than the sound stream, so a `len` below it leaves the rest in place behind the end."""
    b = bytearray(good)
    K, w = int.from_bytes(good[2:6], "little"), good[1]
    at, cnt = tw.lane_starts(good)
    assert w == 1 and K >= 8
    length = len(good)
    if name == "payload_bit":
        j = next(j for j in range(K // 2, K) if cnt[j] > 0)           # a middle lane that has payload
        b[at[j] + 4 + cnt[j] // 2] ^= 0x10
    elif name == "state_high":
        b[at[K // 2]:at[K // 2] + 4] = (0x80000000).to_bytes(4, "little")
    elif name == "state_low":
        b[at[K // 3]:at[K // 3] + 4] = (1 << 22).to_bytes(4, "little")
    elif name == "directory_shift":
        j = next(j for j in range(K // 2, K - 1) if cnt[j + 1] > 0)
        b[6 + j] += 1
        b[6 + j + 1] -= 1
    elif name == "trailing_bytes":
        b += bytes([0x00, 0xFF, 0x72, 0x01, 0x80])
        length += 5
    elif name == "one_byte_short":
        length -= 1
    elif name == "directory_only":
        length = 6 + K * w
    elif name == "five_bytes":
        length = 5
    elif name == "more_lanes_than_symbols":
        b[2:6] = (n + 1).to_bytes(4, "little")
    elif name == "no_lanes":
        b[2:6] = (0).to_bytes(4, "little")
    elif name == "zero_width":
        b[1] = 0
    elif name == "width_five":
        b[1] = 5
    elif name == "format_id":
        b[0] = 0x52
    else:
        raise KeyError(name)
    return bytes(b), length


def damaged_table():
    """[(name or None, p, x, buffer, len)]: every damage of DAMAGE between sound streams, a sound one first and last;
    n <= 1100 at S = 16, so K <= 69 lanes of a few bytes each."""
    rng = np.random.default_rng(1)
    out = []
    for name in sorted(DAMAGE):
        for which in (None, name):
            n = 1000 + 7 * len(out) % 101
            p = rng.uniform(0.02, 0.98, size=n).astype(np.float32)
            x = draw(rng, p, n)
            good = tw.encode(p, x, 16)
            buf, length = (good, len(good)) if which is None else damage(which, good, n)
            out.append((which, p, x, buf, length))
    n = 1100
    p = rng.uniform(0.02, 0.98, size=n).astype(np.float32)
    x = draw(rng, p, n)
    good = tw.encode(p, x, 16)
    return out + [(None, p, x, good, len(good))]


def twin_verdict(p, n, buf, length):
    """(passes the check, status, symbols or None) by the NumPy twin."""
    st, back = tw.decode(p, n, buf[:length])
    return tw.check(buf[:length], n) >= 0, st, back


def test_damaged_streams_get_the_same_verdict_from_the_twin_and_the_library(lib):
    table = damaged_table()
    assert len(table) == 2 * len(DAMAGE) + 1 and [t[0] for t in table[::2]] == [None] * (len(DAMAGE) + 1)
    assert sorted(t[0] for t in table[1::2]) == sorted(DAMAGE)
    for name, p, x, buf, length in table:
        n = x.size
        assert n <= 1100
        passes, status = (True, 0) if name is None else DAMAGE[name]
        t_passes, t_status, t_back = twin_verdict(p, n, buf, length)
        assert (t_passes, t_status) == (passes, status), name
        s = np.frombuffer(buf, np.uint8).copy()
        k = lib.cnc_rans_check(s.ctypes.data, length, n)
        assert k == (tw.lanes(n, 16) if passes else -3), name
        rc, back = host_decode(lib, p, n, buf[:length])
        assert rc == status, name
        if status == 0:
            assert np.array_equal(back, x) and np.array_equal(t_back, x), name
        elif passes:
            assert np.array_equal(back, t_back), name      # the two wrap a damaged state alike


def test_every_single_bit_flip_behind_the_directory_is_refused(lib):
    """A flipped bit in a lane's state or payload leaves the header and directory sound, so only the lanes' end states and
    byte counts can tell: the library and the twin agree on every one of them (seed fixed: each is refused)."""
    rng = np.random.default_rng(1)
    n = 200
    p = rng.uniform(0.02, 0.98, size=n).astype(np.float32)
    x = draw(rng, p, n)
    good = tw.encode(p, x, 16)
    first = 6 + tw.lanes(n, 16)
    for at in range(first, len(good)):
        for bit in range(8):
            b = bytearray(good)
            b[at] ^= 1 << bit
            st, back = tw.decode(p, n, bytes(b))
            rc, hback = host_decode(lib, p, n, bytes(b))
            assert st == rc == -3, (at, bit)
            assert np.array_equal(back, hback), (at, bit)


def test_ctypes_struct_has_the_layout_of_the_header(tmp_path):
    import subprocess
    import ctypes as C
    import os
    from cnc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f[0] for f in _lib.RansStream._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cnc_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cnc_rans_stream_t));']
    lines += [f'  printf("{n} %zu\\n", offsetof(cnc_rans_stream_t, {n}));' for n in names] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(root, "include"), "-o", str(tmp_path / "layout"),
                    str(tmp_path / "layout.c")], check=True)
    out = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(_lib.RansStream)
    for n in names:
        assert int(out[n]) == getattr(_lib.RansStream, n).offset, n
