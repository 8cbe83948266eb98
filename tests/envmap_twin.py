"""NumPy restatement of the environment-map background (include/cnc_hip.h): the lookup, the composite and
both sides of the gradient, in a float64 mode (the definition) and a float32 mode that follows the kernels' operation order
— every product and sum rounded where csrc/envmap.hip rounds it.  The backward is a pure function of
(cell, frac, opacity, g_out): fed the device's own cell and frac, the float32 mode gives the device's bits."""
import numpy as np

LANES = 64


def check_resolution(H):
    if int(H) != H or H < 2 or H > 64 or H % 2:
        raise ValueError(f"H must be even with 2 <= H <= 64, got {H}")
    return int(H)


def coords(dirs, H, dtype=np.float64):
    """-> (cell i32 [n], frac [n, 2]); cell = (y0 + 1) W + (x0 + 1) with x0 = W - 1 renamed -1, or -1 for a dead ray."""
    H = check_resolution(H)
    W = 2 * H
    f = np.dtype(dtype).type
    d = np.asarray(dirs, dtype=dtype).reshape(-1, 3)
    n = d.shape[0]
    cell = np.full(n, -1, np.int32)
    frac = np.zeros((n, 2), dtype)
    with np.errstate(all="ignore"):
        live = np.isfinite(d).all(axis=1)
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        live &= np.isfinite(length) & (length > 0)
    if not live.any():
        return cell, frac
    x, y, z, length = d[live, 0], d[live, 1], d[live, 2], length[live]
    cz = np.clip(z / length, f(-1), f(1))
    phi, theta = np.arctan2(y, x), np.arccos(cz)
    two_pi, pi = (f(np.float32(2 * np.pi)), f(np.float32(np.pi))) if dtype == np.float32 else (f(2 * np.pi), f(np.pi))
    u = (phi / two_pi + f(0.5)) * f(W) - f(0.5)
    v = (theta / pi) * f(H) - f(0.5)
    assert u.dtype == dtype and v.dtype == dtype
    xf, yf = np.floor(u), np.floor(v)
    x0 = np.clip(xf.astype(np.int64), -1, W - 1)
    y0 = np.clip(yf.astype(np.int64), -1, H - 1)
    x0[x0 == W - 1] = -1
    cell[live] = ((y0 + 1) * W + (x0 + 1)).astype(np.int32)
    frac[live, 0] = u - xf
    frac[live, 1] = v - yf
    return cell, frac


def texels(cell, H):
    """cell [n] -> the four texel indices [n, 4] (corner k = 2 [row yb] + [column xb]); H W for a dead ray."""
    W = 2 * H
    cell = np.asarray(cell, np.int64)
    y1, x1 = np.divmod(np.maximum(cell, 0), W)
    y1, x1 = np.clip(y1, 0, H), np.clip(x1, 0, W - 1)
    ya, yb = np.maximum(y1 - 1, 0), np.minimum(y1, H - 1)
    xa, xb = np.where(x1 == 0, W - 1, x1 - 1), x1
    t = np.stack([ya * W + xa, ya * W + xb, yb * W + xa, yb * W + xb], axis=1)
    t[cell < 0] = H * W
    return t


def weights(frac):
    fx, fy = frac[:, 0], frac[:, 1]
    one = frac.dtype.type(1)
    gx, gy = one - fx, one - fy
    return np.stack([gx * gy, fx * gy, gx * fy, fx * fy], axis=1)


def env_at(cell, frac, T):
    """The bilinear mix ((w0 T0 + w1 T1) + w2 T2) + w3 T3 per channel, 0 for a dead ray; in frac's precision."""
    dtype = frac.dtype
    H = T.shape[0]
    Tf = np.asarray(T, dtype).reshape(-1, 3)
    Tf = np.concatenate([Tf, np.zeros((1, 3), dtype)])        # the dead rays' bin
    t, w = texels(cell, H), weights(frac)
    e = ((w[:, 0:1] * Tf[t[:, 0]] + w[:, 1:2] * Tf[t[:, 1]]) + w[:, 2:3] * Tf[t[:, 2]]) + w[:, 3:4] * Tf[t[:, 3]]
    e[np.asarray(cell) < 0] = 0
    return e


def forward(dirs, T, rgb=None, opacity=None, dtype=np.float64):
    """-> (out [n, 3], cell, frac).  rgb and opacity None: the pure lookup."""
    cell, frac = coords(dirs, T.shape[0], dtype)
    e = env_at(cell, frac, T)
    if rgb is None:
        return e, cell, frac
    om = dtype(1) - np.asarray(opacity, dtype).reshape(-1)
    return np.asarray(rgb, dtype).reshape(-1, 3) + om[:, None] * e, cell, frac


def backward_rays(cell, frac, opacity, g_out, T):
    """-> (g_opacity [n], s [n, 3], keys [n, 4]) in frac's precision."""
    dtype = frac.dtype
    g = np.asarray(g_out, dtype).reshape(-1, 3)
    e = env_at(cell, frac, T)
    go = -((g[:, 0] * e[:, 0] + g[:, 1] * e[:, 1]) + g[:, 2] * e[:, 2])
    go[np.asarray(cell) < 0] = 0
    om = dtype.type(1) - np.asarray(opacity, dtype).reshape(-1) if opacity is not None else np.ones(g.shape[0], dtype)
    return go, om[:, None] * g, texels(cell, T.shape[0]).astype(np.int32)


def backward_texture(cell, frac, s, H):
    """g_T [H, 2H, 3] in the documented order: per texel its contributions (ray r, corner k) in ascending 4 r + k; lane l of
    64 adds elements l, l + 64, ... of that sequence from +0, then p[l] += p[l + o] for o = 32 .. 1.  Also returns the
    per-texel (count, sum of |contribution|) the tests' bounds are made of."""
    dtype = frac.dtype
    W = 2 * H
    t = texels(cell, H).reshape(-1)
    contrib = (weights(frac)[:, :, None] * np.asarray(s, dtype)[:, None, :]).reshape(-1, 3)      # [4 n, 3]: one rounded product
    order = np.argsort(t, kind="stable")
    ts = t[order]
    bounds = np.searchsorted(ts, np.arange(H * W + 1))
    g = np.zeros((H * W, 3), dtype)
    count = np.diff(bounds)
    mag = np.zeros((H * W, 3), np.float64)
    live = np.nonzero(count)[0]
    if live.size:
        J = int(-(-count[live].max() // LANES))
        pad = np.zeros((live.size, J * LANES, 3), dtype)        # +0 behind a segment's end: p + 0 = p (p is never -0)
        for row, texel in enumerate(live):
            seg = contrib[order[bounds[texel]:bounds[texel + 1]]]
            pad[row, :seg.shape[0]] = seg
            mag[texel] = np.abs(seg.astype(np.float64)).sum(axis=0)
        pad = pad.reshape(live.size, J, LANES, 3)
        p = np.zeros((live.size, LANES, 3), dtype)
        for j in range(J):
            p = p + pad[:, j]
        off = LANES // 2
        while off >= 1:
            p = p[:, :off] + p[:, off:2 * off]
            off //= 2
        g[live] = p[:, 0]
    return g.reshape(H, W, 3), count, mag.reshape(H, W, 3)


def loss_and_grads64(dirs, T, rgb, opacity, g_out):
    """The float64 definition end to end: sum(g_out * out) and its gradients with respect to (rgb, opacity, T)."""
    out, cell, frac = forward(dirs, T, rgb, opacity, np.float64)
    go, s, _ = backward_rays(cell, frac, opacity, g_out, np.asarray(T, np.float64))
    gT, _, _ = backward_texture(cell, frac, s, T.shape[0])
    return float((np.asarray(g_out, np.float64) * out).sum()), np.asarray(g_out, np.float64).copy(), go, gT


def sky(d):
    """The test scenes' background: 1/2 + 1/2 d for unit d."""
    d = np.asarray(d, np.float64)
    return 0.5 + 0.5 * d / np.linalg.norm(d, axis=-1, keepdims=True)
