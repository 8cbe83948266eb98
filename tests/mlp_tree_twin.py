"""NumPy twin of the "tree1" MLP section, written from the format's description and independent of
cnc_amd/mlp_codec.py and the kernels: everything is counted from the indices themselves (never from the product's
256-bin histograms), one plane at a time.  `model` gives, for a list of index vectors, the depths, the c1 tables, every
plane's symbols / probabilities / ideal code length, the raw low bytes and the section's fixed parts; `decode` walks the
planes back to the indices through a caller-supplied stream decoder."""
import math

import numpy as np

MAX_DEPTH = 8


def c1_of_counts(ones, total):
    """P(bit = 0) * 2^16, rounded half up, inside [1, 65535]; 32768 where nothing was counted."""
    if total == 0:
        return 32768
    return min(65535, max(1, (2 * (total - ones) * 65536 + total) // (2 * total)))


def p_of_c1(c1):
    """The float32 P(+1) both coders quantise back to c1."""
    return (1.0 - (np.asarray(c1, np.float64) - 1.0) / 65534.0).astype(np.float32)


def hist256(q, bits):
    return np.bincount(np.asarray(q, np.int64).reshape(-1) >> (bits - 8), minlength=256).astype(np.int64)


def plane_of(q, bits, j):
    """(prefix, bit) of every index at plane j: the j bits above bit bits - 1 - j, and that bit."""
    q = np.asarray(q, np.int64).reshape(-1)
    return q >> (bits - j), (q >> (bits - 1 - j)) & 1


def node_counts(q, bits, j):
    """(zeros, ones) per prefix of plane j, counted from the indices."""
    prefix, bit = plane_of(q, bits, j)
    ones = np.bincount(prefix[bit == 1], minlength=1 << j)
    zeros = np.bincount(prefix[bit == 0], minlength=1 << j)
    return zeros.astype(np.int64), ones.astype(np.int64)


def tables(q, bits, d):
    out = np.zeros((1 << d) - 1, np.uint16)
    for j in range(d):
        zeros, ones = node_counts(q, bits, j)
        for pi in range(1 << j):
            out[(1 << j) - 1 + pi] = c1_of_counts(int(ones[pi]), int(zeros[pi] + ones[pi]))
    return out


def depth_costs(q, bits):
    """cost(d), d = 0..8, in bits (float64; nodes in heap order, a node's zeros before its ones)."""
    n = int(np.asarray(q).size)
    costs, coded = [float(n * bits)], 0.0
    for j in range(MAX_DEPTH):
        zeros, ones = node_counts(q, bits, j)
        for pi in range(1 << j):
            z, o = int(zeros[pi]), int(ones[pi])
            if z + o:
                c1 = c1_of_counts(o, z + o)
                coded += z * -math.log2(c1 / 65536.0)
                coded += o * -math.log2(1.0 - c1 / 65536.0)
        costs.append(16.0 * (2 ** (j + 1) - 1) + coded + float(n * (bits - j - 1)))
    return costs


def choose_depth(q, bits):
    costs = depth_costs(q, bits)
    best = 0
    for d in range(1, MAX_DEPTH + 1):
        if costs[d] < costs[best]:
            best = d
    return best


def pack_low(q, r):
    """The r low bits of every index, value i's bit b at bit i r + b of a little-endian bit string, zero-padded to bytes."""
    if r == 0:
        return b""
    q = np.asarray(q, np.int64).reshape(-1)
    m = ((q[:, None] >> np.arange(r)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(m, bitorder="little").tobytes()


def unpack_low(buf, n, r):
    if r == 0:
        return np.zeros(n, np.int64)
    m = np.unpackbits(np.frombuffer(buf, np.uint8), bitorder="little")[:n * r].reshape(n, r).astype(np.int64)
    return (m << np.arange(r)).sum(axis=1)


def low_len(n, r):
    return (n * r + 7) // 8


def model(qs, bits, depths=None):
    """qs: the tensors' index vectors, in order."""
    qs = [np.asarray(q, np.int64).reshape(-1) for q in qs]
    if depths is None:
        depths = [choose_depth(q, bits) for q in qs]
    c1 = [tables(q, bits, d) for q, d in zip(qs, depths)]
    D = max(depths)
    planes = []
    for j in range(D):
        sym, p, c1s = [], [], []
        for q, d, tab in zip(qs, depths, c1):
            if d > j:
                prefix, bit = plane_of(q, bits, j)
                node = (1 << j) - 1 + prefix
                sym.append(np.where(bit == 1, 1.0, -1.0).astype(np.float32))
                p.append(p_of_c1(tab[node]))
                c1s.append(tab[node].astype(np.float64))
        sym, p, c1s = np.concatenate(sym), np.concatenate(p), np.concatenate(c1s)
        ideal = float(np.sum(np.where(sym > 0, -np.log2(1.0 - c1s / 65536.0), -np.log2(c1s / 65536.0))))
        planes.append(dict(sym=sym, p=p, n=int(sym.size), ideal_bits=ideal))
    low = [pack_low(q, bits - d) for q, d in zip(qs, depths)]
    return dict(bits=bits, counts=[int(q.size) for q in qs], depths=list(depths), c1=c1, D=D, planes=planes, low=low,
                hist=[hist256(q, bits) for q in qs], fixed_bytes=2 * sum(t.size for t in c1) + sum(len(b) for b in low),
                ideal_bytes=2 * sum(t.size for t in c1) + sum(len(b) for b in low) + sum(pl["ideal_bits"] for pl in planes) / 8.0)


def join_payload(c1, low, streams):
    return b"".join(np.asarray(t).astype("<u2").tobytes() for t in c1) + b"".join(low) + b"".join(streams)


def split_payload(payload, counts, depths, bits, sizes):
    """(c1 tables, low byte runs, streams) of a payload; AssertionError when the length does not fit."""
    at, c1, low, streams = 0, [], [], []
    for d in depths:
        k = 2 * ((1 << d) - 1)
        c1.append(np.frombuffer(payload[at:at + k], "<u2").astype(np.uint16))
        at += k
    for n, d in zip(counts, depths):
        k = low_len(n, bits - d)
        low.append(payload[at:at + k])
        at += k
    for s in sizes:
        streams.append(payload[at:at + s])
        at += s
    assert at == len(payload) and len(sizes) == max(depths)
    return c1, low, streams


def decode(c1, low, counts, depths, bits, decode_stream):
    """decode_stream(j, p) -> plane j's symbols (float32 +-1) for the float32 probabilities p.  Returns the index vectors."""
    prefix = [np.zeros(n, np.int64) for n in counts]
    for j in range(max(depths)):
        p = np.concatenate([p_of_c1(tab[(1 << j) - 1 + pre]) for pre, d, tab in zip(prefix, depths, c1) if d > j])
        sym = np.asarray(decode_stream(j, p))
        assert sym.shape == p.shape
        at = 0
        for t, (n, d) in enumerate(zip(counts, depths)):
            if d > j:
                prefix[t] = (prefix[t] << 1) | (sym[at:at + n] > 0)
                at += n
    return [(pre << (bits - d)) | unpack_low(b, n, bits - d) for pre, b, n, d in zip(prefix, low, counts, depths)]


def plane_positions(counts, depths):
    """[t][j]: where tensor t's first symbol stands in plane j's stream (0 for a plane the tensor is not in... the running
    count of the planes' symbols before it, which the kernels' descriptor rows hold either way)."""
    run = [0] * MAX_DEPTH
    out = []
    for n, d in zip(counts, depths):
        out.append(list(run))
        for j in range(d):
            run[j] += n
    return out


def laplace_indices(n, bits, seed):
    """min/max-quantised indices of n Laplace samples: what a weight tensor with outliers gives."""
    w = np.random.default_rng(seed).laplace(size=n)
    lo, hi = w.min(), w.max()
    return np.clip(np.floor((w - lo) / ((hi - lo) / (2 ** bits - 1) + 1e-6)), 0, 2 ** bits - 1).astype(np.int64)
