"""NumPy restatement of the "rans1" stream format (include/cnc_codec.h), independent of the C++ and HIP
coders: all lanes of a stream advance together as vectors, one symbol per lane and step."""
import numpy as np

FORMAT_ID = 0x72
L = 1 << 23


def c1_of(p):
    """P(-1) * 2^16 in [1, 65535] from float32 P(+1): float32 arithmetic, round half to even, NaN -> 32768."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint((np.float32(1.0) - p) * np.float32(65534.0))
    c1 = np.clip(np.nan_to_num(r, nan=0.0), 0.0, 65534.0).astype(np.int64) + 1
    return np.where(np.isnan(r), 32768, c1)


def lanes(n, S):
    return 0 if n == 0 else -(-n // S)


def dir_width(n, K):
    if K == 0:
        return 1
    worst = 2 * (-(-n // K))
    return 1 if worst < 1 << 8 else 2 if worst < 1 << 16 else 3 if worst < 1 << 24 else 4


def bound(n, S):
    K = lanes(n, S)
    return 6 + K * (dir_width(n, K) + 4) + 2 * n


def freqs(p, x):
    """(f, c) per symbol."""
    c1 = c1_of(p)
    one = np.asarray(x) > 0
    return np.where(one, 65536 - c1, c1), np.where(one, c1, 0)


def ideal_bits(p, x):
    f, _ = freqs(p, x)
    return float(np.sum(-np.log2(f / 65536.0)))


def _le(v, width):
    return bytes((int(v) >> (8 * b)) & 0xFF for b in range(width))


def encode(p, x, S):
    """p: float32 [n] (or one value: p_stride = 0), x: [n] of +-1.  Returns the stream as bytes."""
    x = np.asarray(x, np.float32).reshape(-1)
    n = x.size
    p = np.broadcast_to(np.asarray(p, np.float32).reshape(-1), (n,))
    K = lanes(n, S)
    w = dir_width(n, K)
    if K == 0:
        return bytes([FORMAT_ID, w]) + _le(0, 4)
    f_all, c_all = freqs(p, x)
    M = -(-n // K)
    emitted = np.zeros((K, 2 * M), np.uint8)        # in emission order
    cnt = np.zeros(K, np.int64)
    st = np.full(K, L, np.int64)
    lane = np.arange(K)
    for t in range(M - 1, -1, -1):
        i = lane + t * K
        act = i < n
        f = np.ones(K, np.int64)
        c = np.zeros(K, np.int64)
        f[act], c[act] = f_all[i[act]], c_all[i[act]]
        for _ in range(2):
            out = act & (st >= (f << 15))
            emitted[lane[out], cnt[out]] = (st[out] & 0xFF).astype(np.uint8)
            cnt[out] += 1
            st[out] >>= 8
        assert not np.any(act & (st >= (f << 15)))
        st = np.where(act, ((st // f) << 16) + st % f + c, st)
    assert np.all((st >= L) & (st < 1 << 31))
    parts = [bytes([FORMAT_ID, w]), _le(K, 4)]
    parts += [_le(cnt[j], w) for j in range(K)]
    for j in range(K):
        parts.append(_le(st[j], 4))
        parts.append(emitted[j, :cnt[j]][::-1].tobytes())
    return b"".join(parts)


def check(stream, n):
    """K, or -3."""
    s = bytes(stream)
    if len(s) < 6 or s[0] != FORMAT_ID or not 1 <= s[1] <= 4:
        return -3
    w, K = s[1], int.from_bytes(s[2:6], "little")
    if K > n or (K == 0) != (n == 0) or 6 + K * w > len(s):
        return -3
    cnt = [int.from_bytes(s[6 + j * w:6 + (j + 1) * w], "little") for j in range(K)]
    if 6 + K * w + sum(cnt) + 4 * K > len(s):
        return -3
    return K


def lane_starts(stream):
    """(at, cnt) of a stream whose header and directory are sound: lane j's 4-byte state lies at at[j], its cnt[j]
    payload bytes behind it."""
    s = bytes(stream)
    w, K = s[1], int.from_bytes(s[2:6], "little")
    cnt = np.frombuffer(s[6:6 + K * w], np.uint8).reshape(K, w).astype(np.int64) @ (1 << (8 * np.arange(w, dtype=np.int64)))
    return 6 + K * w + np.cumsum(cnt + 4) - (cnt + 4), cnt


def decode(p, n, stream):
    """(status, x): status 0 or -3, x float32 [n] (None when the header or directory is refused)."""
    s = np.frombuffer(bytes(stream), np.uint8)
    K = check(stream, n)
    if K < 0:
        return -3, None
    p = np.broadcast_to(np.asarray(p, np.float32).reshape(-1), (n,))
    c1_all = c1_of(p)
    x = np.zeros(n, np.float32)
    if K == 0:
        return 0, x
    w = int(s[1])
    cnt = np.array([int.from_bytes(s[6 + j * w:6 + (j + 1) * w].tobytes(), "little") for j in range(K)], np.int64)
    start = 6 + K * w + np.concatenate([[0], np.cumsum(cnt + 4)[:-1]])
    st = np.array([int.from_bytes(s[a:a + 4].tobytes(), "little") for a in start], np.int64)
    good = bool(np.all((st >= L) & (st < 1 << 31)))
    sub = start + 4
    used = np.zeros(K, np.int64)
    lane = np.arange(K)
    padded = np.concatenate([s, np.zeros(8, np.uint8)])
    for t in range(-(-n // K)):
        i = lane + t * K
        act = i < n
        ia = i[act]
        c1 = np.ones(K, np.int64)
        c1[act] = c1_all[ia]
        slot = st & 0xFFFF
        one = slot >= c1
        f = np.where(one, 65536 - c1, c1)
        c = np.where(one, c1, 0)
        x[ia] = np.where(one[act], 1.0, -1.0)
        st = np.where(act, (f * (st >> 16) + slot - c) & 0xFFFFFFFF, st)
        for _ in range(2):
            need = act & (st < L)
            inside = need & (used < cnt)
            byte = np.zeros(K, np.int64)
            byte[inside] = padded[(sub + used)[inside]]
            st = np.where(need, (st << 8) | byte, st)
            used += need
    good = good and bool(np.all(st == L)) and bool(np.all(used == cnt))
    return (0 if good else -3), x
