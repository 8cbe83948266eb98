"""Host mirror of the error-map entry points (csrc/error_map.hip, include/cnc_hip.h): the weighted loss, the
map's update — the grouped mean in HIP behind a stable integer sort made with torch, as the environment map's texture
gradient is — the CDF and the sampler; and the torch restatement of each for host tensors, which follows the header's order
of operations in float32 (tests/errmap_twin.py holds it to the bits).  The callee allocates and returns its outputs, like
the other mirrors; the restatements are `*_torch`, and a mirror given a host tensor raises (no CPU fallback).
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream

G_MIN, G_MAX = 1, 64
MAX_CELLS = 1 << 19
CHUNK, BLOCK, WAVE = 64, 256, 64


def check_shape(n_cams, height, width, resolution):
    for name, v in (("n_cams", n_cams), ("height", height), ("width", width), ("resolution", resolution)):
        if isinstance(v, bool) or int(v) != v or v < 1:
            raise ValueError(f"error map: {name} must be a positive integer, got {v!r}")
    if not G_MIN <= resolution <= G_MAX:
        raise ValueError(f"error map: the resolution G must lie in {G_MIN}..{G_MAX}, got {resolution!r}")
    if n_cams * resolution * resolution > MAX_CELLS:
        raise ValueError(f"error map: {n_cams} cameras at resolution {resolution} are more than {MAX_CELLS} cells")
    return int(n_cams), int(height), int(width), int(resolution)


def _f32(t, name, shape):
    check_input(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"errmap: {name} must be float32 {list(shape)}, got {t.dtype} {list(t.shape)}")


def _i64(t, name, n):
    check_input(t, name)
    if t.dtype != torch.int64 or tuple(t.shape) != (n,):
        raise RuntimeError(f"errmap: {name} must be int64 [{n}]")


# ------------------------------------------------------------------------------------------------ the HIP entry points
def loss_forward(rgb, pixels, weight):
    """cnc_errmap_loss_forward -> (loss f32 [], err f32 [n]): loss = (1 / 3n) sum_i w_i sum_c (rgb - pixels)^2 in the
    header's fixed order, err_i = (1 / 3) sum_c (rgb - pixels)^2, one launch for both and one for the fold."""
    n = rgb.shape[0]
    if n == 0:
        raise RuntimeError("errmap: the loss of no rays")
    _f32(rgb, "rgb", (n, 3))
    _f32(pixels, "pixels", (n, 3))
    _f32(weight, "weight", (n,))
    dev = rgb.device
    L = _lib.lib()
    ws = torch.empty(int(L.cnc_errmap_loss_workspace(n)) // 4, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    err = torch.empty((n,), dtype=torch.float32, device=dev)
    check(L.cnc_errmap_loss_forward(ptr(rgb), ptr(pixels), ptr(weight), n, ptr(ws), ws.numel() * 4, ptr(loss), ptr(err),
                                    stream(dev)), "errmap_loss_forward")
    return loss, err


def loss_backward(g_loss, rgb, pixels, weight):
    """cnc_errmap_loss_backward -> g_rgb f32 [n, 3]; g_loss is the device scalar autograd hands over (no host read)."""
    n = rgb.shape[0]
    _f32(g_loss, "g_loss", ())
    _f32(rgb, "rgb", (n, 3))
    _f32(pixels, "pixels", (n, 3))
    _f32(weight, "weight", (n,))
    g_rgb = torch.empty_like(rgb)
    check(_lib.lib().cnc_errmap_loss_backward(ptr(g_loss), ptr(rgb), ptr(pixels), ptr(weight), n, ptr(g_rgb),
                                              stream(rgb.device)), "errmap_loss_backward")
    return g_rgb


def keys(cam_ids, px, py, n_cams, height, width, resolution):
    """cnc_errmap_keys -> i32 [n]: every ray's cell."""
    n_cams, height, width, resolution = check_shape(n_cams, height, width, resolution)
    n = cam_ids.shape[0]
    for name, t in (("cam_ids", cam_ids), ("px", px), ("py", py)):
        _i64(t, name, n)
    out = torch.empty((n,), dtype=torch.int32, device=cam_ids.device)
    if n:
        check(_lib.lib().cnc_errmap_keys(ptr(cam_ids), ptr(px), ptr(py), n, n_cams, height, width, resolution, ptr(out),
                                         stream(cam_ids.device)), "errmap_keys")
    return out


def update(map_, cell_keys, err, decay):
    """cnc_errmap_update, in place on map f32 [n_cams, G, G]: map <- decay map + (1 - decay) mean(finite err of the cell's
    rays) for every cell with such a ray; every other cell keeps its bits.  The grouping is plumbing — a stable sort of the n
    integer keys and one searchsorted for the segment bounds; the sum is the kernel."""
    check_input(map_, "map")
    if map_.dtype != torch.float32 or map_.dim() != 3 or map_.shape[1] != map_.shape[2]:
        raise RuntimeError("errmap: map must be float32 [n_cams, G, G]")
    n = cell_keys.shape[0]
    check_input(cell_keys, "keys")
    if cell_keys.dtype != torch.int32 or tuple(cell_keys.shape) != (n,):
        raise RuntimeError("errmap: keys must be int32 [n]")
    _f32(err, "err", (n,))
    if n == 0:
        return map_
    dev = map_.device
    sorted_keys, order = torch.sort(cell_keys, stable=True)
    bounds = torch.arange(map_.numel() + 1, dtype=torch.int32, device=dev)
    offsets = torch.searchsorted(sorted_keys, bounds).contiguous()               # int64 [cells + 1]
    check(_lib.lib().cnc_errmap_update(ptr(order), ptr(offsets), ptr(err), n, map_.shape[0], map_.shape[1], float(decay),
                                       ptr(map_), stream(dev)), "errmap_update")
    return map_


def cdf(map_, height, width, uniform_floor, out=None):
    """cnc_errmap_cdf -> (prob f32 [cells], cdf f32 [cells]); `out` = a pair of buffers to write into."""
    check_input(map_, "map")
    if map_.dtype != torch.float32 or map_.dim() != 3 or map_.shape[1] != map_.shape[2]:
        raise RuntimeError("errmap: map must be float32 [n_cams, G, G]")
    n_cams, height, width, G = check_shape(map_.shape[0], height, width, map_.shape[1])
    if not 0.0 <= float(uniform_floor) <= 1.0:
        raise ValueError("error map: the uniform floor must lie in [0, 1]")
    cells = map_.numel()
    prob, c = out if out is not None else (torch.empty(cells, dtype=torch.float32, device=map_.device) for _ in range(2))
    _f32(prob, "prob", (cells,))
    _f32(c, "cdf", (cells,))
    check(_lib.lib().cnc_errmap_cdf(ptr(map_), n_cams, height, width, G, float(uniform_floor), ptr(prob), ptr(c),
                                    stream(map_.device)), "errmap_cdf")
    return prob, c


def sample(rand, cdf_, prob, n_cams, height, width, resolution):
    """cnc_errmap_sample -> (cam_ids, px, py i64 [n], weight f32 [n]) from rand f32 [n, 3] in [0, 1)."""
    n_cams, height, width, resolution = check_shape(n_cams, height, width, resolution)
    n, cells = rand.shape[0], n_cams * resolution * resolution
    _f32(rand, "rand", (n, 3))
    _f32(cdf_, "cdf", (cells,))
    _f32(prob, "prob", (cells,))
    dev = rand.device
    ids, px, py = (torch.empty((n,), dtype=torch.int64, device=dev) for _ in range(3))
    weight = torch.empty((n,), dtype=torch.float32, device=dev)
    if n:
        check(_lib.lib().cnc_errmap_sample(ptr(rand), ptr(cdf_), ptr(prob), n, n_cams, height, width, resolution, ptr(ids),
                                           ptr(px), ptr(py), ptr(weight), stream(dev)), "errmap_sample")
    return ids, px, py, weight


# ------------------------------------------------------------------------------------------------ the torch restatement
def cell_edges(size, G, device=None):
    return (torch.arange(G + 1, dtype=torch.int64, device=device) * int(size)) // int(G)


def cell_of(p, size, G):
    return ((p + 1) * int(G) - 1) // int(size)


def areas(n_cams, height, width, G, device=None):
    """i64 [n_cams G G]: every cell's pixel count."""
    h, w = cell_edges(height, G, device).diff(), cell_edges(width, G, device).diff()
    return (h[:, None] * w[None, :]).reshape(-1).repeat(n_cams)


def _rows(v, width):
    pad = (-v.shape[0]) % width
    return torch.cat([v, v.new_zeros(pad)]).reshape(-1, width)


def _running(rows, dim):
    """Sequential float32 running sums along `dim` (torch.cumsum accumulates wider on a host device)."""
    out = rows.clone()
    prev = None
    for piece in out.unbind(dim):
        if prev is not None:
            piece.copy_(prev + piece)
        prev = piece
    return out


def _tree(p, width):
    p = p.clone()
    s = width // 2
    while s >= 1:
        p[..., :s] = p[..., :s] + p[..., s:2 * s]
        s //= 2
    return p[..., 0]


def cdf_torch(map_, height, width, uniform_floor):
    n_cams, height, width, G = check_shape(map_.shape[0], height, width, map_.shape[1])
    dev = map_.device
    a_int = areas(n_cams, height, width, G, dev)
    cells = a_int.shape[0]
    a = a_int.to(torch.float32)
    N = torch.tensor(float(n_cams * height * width), dtype=torch.float32, device=dev)
    u = torch.tensor(float(uniform_floor), dtype=torch.float32, device=dev)
    m = map_.reshape(-1).to(torch.float32)
    t = torch.where(m > 0, m, torch.zeros_like(m)) * a
    S = _running(_running(_rows(t, CHUNK), 1)[:, -1], 0)[-1]
    if bool(S > 0) and bool(torch.isfinite(S)):
        prob = ((1.0 - u) * t) / S + (u * a) / N
    else:
        prob = a / N
    run = _running(_rows(prob, CHUNK), 1)
    sums = run[:, -1]
    P = _running(torch.cat([sums.new_zeros(1), sums[:-1]]), 0)
    c = (P[:, None] + run).reshape(-1)[:cells].clone()
    c[int(torch.nonzero(a_int > 0)[-1]):] = 1.0
    return prob, c


def sample_torch(rand, cdf_, prob, n_cams, height, width, resolution):
    n_cams, height, width, G = check_shape(n_cams, height, width, resolution)
    dev = rand.device
    cells = cdf_.shape[0]
    r0 = rand[:, 0].contiguous()
    cell = torch.searchsorted(cdf_.contiguous(), r0, right=True).clamp(max=cells - 1)
    cell = torch.where(torch.isnan(r0), torch.full_like(cell, cells - 1), cell)
    k, rem = cell // (G * G), cell % (G * G)
    gy, gx = rem // G, rem % G
    ex, ey = cell_edges(width, G, dev), cell_edges(height, G, dev)
    x0, y0 = ex[gx], ey[gy]
    cw, ch = ex[gx + 1] - x0, ey[gy + 1] - y0

    def inside(r, size):
        sf = size.to(torch.float32)
        f = r * sf
        i = torch.where(f < sf, torch.where((f >= 0) & (f < sf), f, torch.zeros_like(f)).to(torch.int64), size - 1)
        i = torch.where(f >= 0, i, torch.zeros_like(i))
        return torch.minimum(i.clamp(min=0), (size - 1).clamp(min=0))
    px = (x0 + inside(rand[:, 1], cw)).clamp(0, width - 1)
    py = (y0 + inside(rand[:, 2], ch)).clamp(0, height - 1)
    inv = torch.tensor(1.0, dtype=torch.float32, device=dev) / torch.tensor(float(n_cams * height * width),
                                                                              dtype=torch.float32, device=dev)
    pp = prob[cell] / (cw * ch).to(torch.float32)
    weight = torch.where(pp > 0, inv / pp, torch.zeros_like(pp))
    return k, px, py, weight


def keys_torch(cam_ids, px, py, n_cams, height, width, resolution):
    G = int(resolution)
    k = cam_ids.clamp(0, n_cams - 1)
    gx = cell_of(px.clamp(0, width - 1), width, G)
    gy = cell_of(py.clamp(0, height - 1), height, G)
    return ((k * G + gy) * G + gx).to(torch.int32)


def update_torch(map_, cell_keys, err, decay):
    """In place, like `update`."""
    flat = map_.view(-1)
    decay = torch.tensor(float(decay), dtype=torch.float32, device=map_.device)
    for c in torch.unique(cell_keys).tolist():
        e = err[cell_keys == c]
        ok = torch.isfinite(e)
        cnt = int(ok.sum())
        if cnt == 0:
            continue
        lanes = _running(_rows(torch.where(ok, e, torch.zeros_like(e)), WAVE), 0)[-1]
        mean = _tree(lanes, WAVE) / torch.tensor(float(cnt), dtype=torch.float32, device=map_.device)
        flat[c] = decay * flat[c] + (1.0 - decay) * mean
    return map_


def loss_forward_torch(rgb, pixels, weight):
    """Differentiable by torch's own autograd (the forward's value follows the header's order; its gradient is torch's)."""
    n = rgb.shape[0]
    d = rgb - pixels
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    err = (sq / 3.0).detach()
    t = weight * sq
    part = _tree(_rows(t, BLOCK), BLOCK)
    rows = _rows(part, BLOCK)
    q = rows[0]
    for k in range(1, rows.shape[0]):
        q = q + rows[k]
    return _tree(q, BLOCK) / torch.tensor(float(3 * n), dtype=torch.float32, device=rgb.device), err


def loss_backward_torch(g_loss, rgb, pixels, weight):
    n = rgb.shape[0]
    c = ((g_loss * 2.0) * weight) / torch.tensor(float(3 * n), dtype=torch.float32, device=rgb.device)
    return c[:, None] * (rgb - pixels)
