"""NumPy twin of the error-map kernels (csrc/error_map.hip), from the arithmetic include/cnc_hip.h documents — not from the
kernels' code.  Two modes: `np.float64` is the mathematics (sums in any order); `np.float32` follows the stated order of
operations step by step, so that the kernels and the torch restatement can be compared with it bit for bit.

    geometry:  cell_edges, cell_of, areas, pixel_cells
    cdf(map, ...)                  -> (prob, cdf)
    sample(rand, cdf, prob, ...)   -> (cam_ids, px, py, weight)
    keys(cam_ids, px, py, ...)     -> cell of every ray
    update(map, keys, err, decay)  -> the new map
    loss_forward / loss_backward
"""
import numpy as np

CHUNK = 64          # cells per chunk of the CDF's scan
BLOCK = 256         # rays per block of the loss
WAVE = 64


def cell_edges(size, G):
    """[G + 1]: first pixel of every cell along one axis, g * size // G."""
    return (np.arange(G + 1, dtype=np.int64) * int(size)) // int(G)


def cell_of(p, size, G):
    return ((np.asarray(p, np.int64) + 1) * int(G) - 1) // int(size)


def areas(n_cams, H, W, G):
    """int64 [n_cams * G * G]: the pixel count of every cell."""
    h, w = np.diff(cell_edges(H, G)), np.diff(cell_edges(W, G))
    return np.tile((h[:, None] * w[None, :]).reshape(-1), n_cams)


def pixel_cells(n_cams, H, W, G):
    """int64 [n_cams, H, W]: the cell of every pixel."""
    gy, gx = cell_of(np.arange(H), H, G), cell_of(np.arange(W), W, G)
    k = np.arange(n_cams, dtype=np.int64)
    return (k[:, None, None] * G + gy[None, :, None]) * G + gx[None, None, :]


def _chunk_rows(v):
    """v padded with +0 to whole chunks, [n_chunks, CHUNK]."""
    n = v.shape[0]
    pad = (-n) % CHUNK
    return np.concatenate([v, np.zeros(pad, v.dtype)]).reshape(-1, CHUNK)


def _seq_sum(rows, axis):
    """Sequential sums in the array's own precision (accumulate never pairs)."""
    return np.add.accumulate(rows, axis=axis, dtype=rows.dtype)


def cdf(m, n_cams, H, W, G, u, dtype=np.float32):
    """-> (prob [cells], cdf [cells])."""
    a_int = areas(n_cams, H, W, G)
    cells = a_int.shape[0]
    m = np.asarray(m, dtype).reshape(-1)
    assert m.shape[0] == cells
    a = a_int.astype(dtype)
    N = dtype(n_cams * H * W)
    u = dtype(u)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mm = np.where(m > 0, m, dtype(0))
        t = mm * a
        if dtype == np.float64:
            S = t.sum()
        else:
            S = _seq_sum(_seq_sum(_chunk_rows(t), 1)[:, -1], 0)[-1]
        if S > 0 and np.isfinite(S):
            prob = ((dtype(1) - u) * t) / S + (u * a) / N
        else:
            prob = a / N
    prob = prob.astype(dtype)
    if dtype == np.float64:
        c = np.cumsum(prob)
    else:
        run = _seq_sum(_chunk_rows(prob), 1)
        sums = run[:, -1]
        P = np.zeros_like(sums)
        acc = dtype(0)
        for k in range(sums.shape[0]):
            P[k] = acc
            acc = dtype(acc + sums[k])
        c = (P[:, None] + run).reshape(-1)[:cells].astype(dtype)
    last_live = int(np.nonzero(a_int > 0)[0][-1])
    c[last_live:] = dtype(1)
    return prob, c


def sample(rand, cdf_, prob, n_cams, H, W, G, dtype=np.float32):
    """-> (cam_ids, px, py int64 [n], weight [n])."""
    rand = np.asarray(rand, dtype).reshape(-1, 3)
    cdf_ = np.asarray(cdf_, dtype)
    cells = cdf_.shape[0]
    cell = np.minimum(np.searchsorted(cdf_, rand[:, 0], side="right"), cells - 1)      # first entry > r
    cell = np.where(np.isnan(rand[:, 0]), cells - 1, cell)
    GG = G * G
    k, rem = cell // GG, cell % GG
    gy, gx = rem // G, rem % G
    ex, ey = cell_edges(W, G), cell_edges(H, G)
    x0, y0 = ex[gx], ey[gy]
    cw, ch = ex[gx + 1] - x0, ey[gy + 1] - y0

    def inside(r, size):
        with np.errstate(invalid="ignore"):
            sf = size.astype(dtype)
            f = r * sf
            i = np.where(f < sf, np.trunc(np.where((f >= 0) & (f < sf), f, 0)).astype(np.int64), size - 1)
            i = np.where(f >= 0, i, 0)
        return np.clip(i, 0, np.maximum(size - 1, 0))
    px = np.clip(x0 + inside(rand[:, 1], cw), 0, W - 1)
    py = np.clip(y0 + inside(rand[:, 2], ch), 0, H - 1)
    inv = dtype(1) / dtype(n_cams * H * W)
    with np.errstate(invalid="ignore", divide="ignore"):
        pp = (np.asarray(prob, dtype)[cell] / (cw * ch).astype(dtype)).astype(dtype)
        weight = np.where(pp > 0, inv / pp, dtype(0)).astype(dtype)
    return k.astype(np.int64), px.astype(np.int64), py.astype(np.int64), weight


def keys(cam_ids, px, py, n_cams, H, W, G):
    k = np.clip(np.asarray(cam_ids, np.int64), 0, n_cams - 1)
    gx = cell_of(np.clip(np.asarray(px, np.int64), 0, W - 1), W, G)
    gy = cell_of(np.clip(np.asarray(py, np.int64), 0, H - 1), H, G)
    return ((k * G + gy) * G + gx).astype(np.int32)


def _wave_sum(v):
    """The fixed order of one wave over a segment: lane l adds elements l, l + 64, .. from +0, then the tree."""
    pad = (-v.shape[0]) % WAVE
    p = _seq_sum(np.concatenate([v, np.zeros(pad, v.dtype)]).reshape(-1, WAVE), 0)[-1].copy()
    o = WAVE // 2
    while o >= 1:
        p[:o] = p[:o] + p[o:2 * o]
        o //= 2
    return p[0]


def update(m, keys_, err, decay, dtype=np.float32):
    """The map after one observation; cells without a finite ray keep their bits."""
    out = np.array(m, dtype).reshape(-1).copy()
    err = np.asarray(err, dtype)
    decay = dtype(decay)
    keys_ = np.asarray(keys_, np.int64)
    for c in np.unique(keys_):
        e = err[keys_ == c]                      # ascending ray index: what the stable sort lists
        ok = np.isfinite(e)
        cnt = int(ok.sum())
        if cnt == 0:
            continue
        e = np.where(ok, e, dtype(0))
        s = e.sum() if dtype == np.float64 else _wave_sum(e)
        mean = dtype(s / dtype(cnt))
        out[c] = dtype(decay * out[c]) + dtype(dtype(dtype(1) - decay) * mean)
    return out.reshape(np.shape(m))


def _tree(p):
    """p[j] = p[j] + p[j + s], s = 128 .. 1, along the last axis of [.., 256]."""
    p = p.copy()
    s = BLOCK // 2
    while s >= 1:
        p[..., :s] = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def loss_forward(rgb, pix, w, dtype=np.float32):
    """-> (loss, err [n])."""
    rgb, pix, w = np.asarray(rgb, dtype), np.asarray(pix, dtype), np.asarray(w, dtype)
    n = rgb.shape[0]
    d = rgb - pix
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    err = (sq / dtype(3)).astype(dtype)
    t = (w * sq).astype(dtype)
    if dtype == np.float64:
        return t.sum() / (3.0 * n), err
    part = _tree(np.concatenate([t, np.zeros((-n) % BLOCK, dtype)]).reshape(-1, BLOCK))
    q = _seq_sum(np.concatenate([part, np.zeros((-part.shape[0]) % BLOCK, dtype)]).reshape(-1, BLOCK), 0)[-1]
    return dtype(_tree(q) / dtype(3 * n)), err


def loss_backward(g, rgb, pix, w, dtype=np.float32):
    rgb, pix, w = np.asarray(rgb, dtype), np.asarray(pix, dtype), np.asarray(w, dtype)
    n = rgb.shape[0]
    c = ((dtype(g) * dtype(2)) * w) / dtype(3 * n)
    return (c[:, None].astype(dtype) * (rgb - pix)).astype(dtype)
