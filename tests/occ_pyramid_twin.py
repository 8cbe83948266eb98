"""NumPy twin of the occupancy grid's "pyramid1" model, written from its specification, not from the
kernels: the levels, the candidate order, the contexts, the histograms, the c1 tables, the raw coarsest level, the payload
layout and the ideal code length.  Slow and plain on purpose; the GPU tests hold the kernels to it integer for integer.

    grid      uint8 / bool [G, rx, ry, rz], C order
    K         min(4, trailing zero bits of gcd(rx, ry, rz)); 0 -> ValueError
    level k+1 OR over the 2x2x2 blocks of level k; level K is stored raw
    candidates of level k: the 8 children of every occupied cell of level k+1, by ascending linear parent index (grid-major),
              then octant o = ox<<2 | oy<<1 | oz; candidate 8 rank(parent) + o
    context   d_a = +1 if the octant's bit on axis a is set else -1; cells outside the grid are empty
              near = occupied among P+d_x, P+d_y, P+d_z, P+d_x+d_y, P+d_x+d_z, P+d_y+d_z, P+d_x+d_y+d_z     (0..7)
              far  = occupied among P-d_x, P-d_y, P-d_z                                                       (0..3)
              ctx  = near * 4 + far
    c1        per (level, ctx): P(symbol = -1) * 2^16 = empty / total rounded half up, inside [1, 65535]; 32768 if unused
    symbol    +1 occupied, -1 empty; the coders take P(+1) as a float32 p with quantiser(p) == c1
"""
import numpy as np

N_CTX = 32


def levels_of(shape):
    if len(shape) != 4:
        raise ValueError("expected [G, rx, ry, rz]")
    K = 0
    while K < 4 and all(int(s) % (2 << K) == 0 for s in shape[1:]):
        K += 1
    if K == 0:
        raise ValueError("a grid with an odd side has no coarser level")
    return K


def reduce(grid):
    """[level 0, ..., level K] as uint8 0/1 arrays."""
    g = (np.asarray(grid) != 0).astype(np.uint8)
    out = [g]
    for _ in range(levels_of(g.shape)):
        G, x, y, z = out[-1].shape
        out.append(out[-1].reshape(G, x // 2, 2, y // 2, 2, z // 2, 2).max(axis=(2, 4, 6)))
    return out


def candidates(parent):
    """(idx int32 [n]: linear index in the child level, ctx uint8 [n]) of the level below `parent`."""
    parent = np.asarray(parent, dtype=np.uint8)
    G, px, py, pz = parent.shape
    pad = np.zeros((G, px + 2, py + 2, pz + 2), dtype=np.int64)
    pad[:, 1:-1, 1:-1, 1:-1] = parent
    occ = np.flatnonzero(parent.reshape(-1))                       # ascending linear index: grid-major
    g, x, y, z = np.unravel_index(occ, parent.shape)
    idx = np.empty((occ.size, 8), dtype=np.int64)
    ctx = np.empty((occ.size, 8), dtype=np.int64)
    at = lambda ax, ay, az: pad[g, x + 1 + ax, y + 1 + ay, z + 1 + az]
    for o in range(8):
        ox, oy, oz = (o >> 2) & 1, (o >> 1) & 1, o & 1
        dx, dy, dz = 2 * ox - 1, 2 * oy - 1, 2 * oz - 1
        near = (at(dx, 0, 0) + at(0, dy, 0) + at(0, 0, dz) + at(dx, dy, 0) + at(dx, 0, dz) + at(0, dy, dz) + at(dx, dy, dz))
        far = at(-dx, 0, 0) + at(0, -dy, 0) + at(0, 0, -dz)
        ctx[:, o] = near * 4 + far
        idx[:, o] = np.ravel_multi_index((g, 2 * x + ox, 2 * y + oy, 2 * z + oz), (G, 2 * px, 2 * py, 2 * pz))
    return idx.reshape(-1).astype(np.int32), ctx.reshape(-1).astype(np.uint8)


def c1_of_counts(ones, total):
    if total == 0:
        return 32768
    return min(65535, max(1, (2 * (total - ones) * 65536 + total) // (2 * total)))


def p_of_c1(c1):
    return (1.0 - (np.asarray(c1, dtype=np.float64) - 1.0) / 65534.0).astype(np.float32)


def ideal_bits(ctx, sym, c1):
    """Sum of -log2(c / 2^16) over a level's candidates, c the 16-bit frequency of the symbol coded."""
    c_minus = np.asarray(c1, dtype=np.float64)[ctx]
    c = np.where(sym > 0, 65536.0 - c_minus, c_minus)
    return float(-np.log2(c / 65536.0).sum())


def model(grid):
    """Everything an encoder derives from the grid, per level k = 0..K-1:
    idx, ctx, sym (+-1 float32), hist [32, 2] = (ones, total), c1 [32], n, ideal_bits; plus levels, K and raw."""
    lv = reduce(grid)
    K = len(lv) - 1
    per = []
    for k in range(K):
        idx, ctx = candidates(lv[k + 1])
        sym = np.where(lv[k].reshape(-1)[idx] != 0, 1.0, -1.0).astype(np.float32)
        hist = np.zeros((N_CTX, 2), dtype=np.int64)
        np.add.at(hist[:, 0], ctx[sym > 0], 1)
        np.add.at(hist[:, 1], ctx, 1)
        c1 = np.array([c1_of_counts(int(o), int(t)) for o, t in hist], dtype=np.uint16)
        per.append(dict(idx=idx, ctx=ctx, sym=sym, hist=hist, c1=c1, n=int(idx.size), ideal_bits=ideal_bits(ctx, sym, c1)))
    return dict(K=K, levels=lv, per=per, raw=pack_raw(lv[K]))


def pack_raw(top):
    """Bit i of the coarsest level (C order over all grids) at bit i & 7 of byte i >> 3."""
    bits = np.asarray(top, dtype=np.uint8).reshape(-1)
    out = np.zeros((bits.size + 7) // 8, dtype=np.uint8)
    for i in np.flatnonzero(bits):
        out[i >> 3] |= 1 << (i & 7)
    return out.tobytes()


def unpack_raw(raw, shape):
    n = int(np.prod(shape))
    b = np.frombuffer(raw, dtype=np.uint8)
    return np.array([(b[i >> 3] >> (i & 7)) & 1 for i in range(n)], dtype=np.uint8).reshape(shape)


def split_payload(payload, shape, n, stream_sizes):
    """raw | K x 32 u16 LE tables, level 0 first | the levels' streams, coarse to fine.  -> (top level, c1 [K, 32], streams by level)."""
    K = levels_of(shape)
    top_shape = (shape[0], shape[1] >> K, shape[2] >> K, shape[3] >> K)
    n_raw = (int(np.prod(top_shape)) + 7) // 8
    top = unpack_raw(payload[:n_raw], top_shape)
    c1 = np.frombuffer(payload[n_raw:n_raw + 64 * K], dtype="<u2").reshape(K, N_CTX)
    at, streams = n_raw + 64 * K, [b""] * K
    for k in range(K - 1, -1, -1):
        streams[k] = payload[at:at + stream_sizes[k]]
        at += stream_sizes[k]
    assert at == len(payload)
    return top, c1, streams


def decode(top, c1, n, decode_stream):
    """Coarse to fine: decode_stream(k, p float32 [n_k]) -> +-1 symbols of level k.  Returns level 0 as uint8."""
    parent = np.asarray(top, dtype=np.uint8)
    for k in range(len(n) - 1, -1, -1):
        G, px, py, pz = parent.shape
        child = np.zeros((G, 2 * px, 2 * py, 2 * pz), dtype=np.uint8)
        idx, ctx = candidates(parent)
        assert idx.size == n[k], (k, idx.size, n[k])
        if idx.size:
            sym = np.asarray(decode_stream(k, p_of_c1(c1[k])[ctx]))
            child.reshape(-1)[idx[sym > 0]] = 1
        parent = child
    return parent


# ------------------------------------------------------------------------------------------------ test grids
def ball(res, radius=0.42, shell=None):
    """Cells whose centre lies within radius x half width of the centre (a shell `shell` thick if given)."""
    c = (np.arange(res) + 0.5) / res * 2 - 1
    r = np.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    m = r <= radius
    if shell is not None:
        m &= r >= radius - shell
    return m[None].astype(np.uint8)


def blobs_and_rods(res, seed, n_blobs=12, n_rods=6):
    rng = np.random.default_rng(seed)
    c = (np.arange(res) + 0.5) / res * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    m = np.zeros((res, res, res), dtype=bool)
    for _ in range(n_blobs):
        cx, cy, cz = rng.uniform(-0.7, 0.7, 3)
        r = rng.uniform(0.05, 0.22)
        m |= (X - cx) ** 2 + (Y - cy) ** 2 + (Z - cz) ** 2 <= r * r
    for _ in range(n_rods):
        a, b = rng.uniform(-0.8, 0.8, 3), rng.uniform(-0.8, 0.8, 3)
        d = b - a
        t = np.clip(((X - a[0]) * d[0] + (Y - a[1]) * d[1] + (Z - a[2]) * d[2]) / (d @ d), 0, 1)
        m |= (X - a[0] - t * d[0]) ** 2 + (Y - a[1] - t * d[1]) ** 2 + (Z - a[2] - t * d[2]) ** 2 <= (1.5 / res) ** 2
    return m[None].astype(np.uint8)
