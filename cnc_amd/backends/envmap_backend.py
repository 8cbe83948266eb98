"""Host mirror of the environment-map entry points (csrc/envmap.hip, include/cnc_hip.h): the lookup and
composite, the ray side of the backward, and the texture side — the grouped sum in HIP behind a stable integer sort made
with torch.  The callee allocates and returns its outputs, like the other mirrors; host tensors raise (no CPU fallback).
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream

H_MIN, H_MAX = 2, 64


def check_resolution(H) -> int:
    """H of a texture [H, 2H, 3]: even, 2 <= H <= 64."""
    if isinstance(H, bool) or int(H) != H or H < H_MIN or H > H_MAX or int(H) % 2:
        raise ValueError(f"environment map: the resolution H must be even with {H_MIN} <= H <= {H_MAX}, got {H!r}")
    return int(H)


def _f32(t, name, shape):
    check_input(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"envmap: {name} must be float32 {list(shape)}, got {t.dtype} {list(t.shape)}")


def _texture(texture) -> int:
    check_input(texture, "texture")
    if texture.dtype != torch.float32 or texture.dim() != 3 or texture.shape[2] != 3 or texture.shape[1] != 2 * texture.shape[0]:
        raise RuntimeError("envmap: texture must be float32 [H, 2H, 3]")
    return check_resolution(texture.shape[0])


def envmap_forward(dirs, texture, rgb=None, opacity=None, want_coords=True):
    """-> (out [n, 3], cell i32 [n] | None, frac [n, 2] | None).  out = rgb + (1 - opacity) env(dirs); rgb and opacity both
    None: the pure lookup.  n == 0 launches nothing."""
    H = _texture(texture)
    n = dirs.shape[0]
    _f32(dirs, "dirs", (n, 3))
    if (rgb is None) != (opacity is None):
        raise RuntimeError("envmap: rgb and opacity come together")
    if rgb is not None:
        _f32(rgb, "rgb", (n, 3))
        _f32(opacity, "opacity", (n,))
    dev = dirs.device
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    cell = torch.empty((n,), dtype=torch.int32, device=dev) if want_coords else None
    frac = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_coords else None
    if n:
        check(_lib.lib().cnc_envmap_forward(ptr(dirs), ptr(rgb), ptr(opacity), ptr(texture), H, n, ptr(out), ptr(cell),
                                            ptr(frac), stream(dev)), "envmap_forward")
    return out, cell, frac


def envmap_backward_rays(g_out, opacity, cell, frac, texture):
    """-> (g_opacity [n] | None (opacity None), s [n, 3], keys i32 [n, 4])."""
    H = _texture(texture)
    n = g_out.shape[0]
    _f32(g_out, "g_out", (n, 3))
    _f32(frac, "frac", (n, 2))
    check_input(cell, "cell")
    if cell.dtype != torch.int32 or tuple(cell.shape) != (n,):
        raise RuntimeError("envmap: cell must be int32 [n]")
    if opacity is not None:
        _f32(opacity, "opacity", (n,))
    dev = g_out.device
    g_opacity = torch.empty((n,), dtype=torch.float32, device=dev) if opacity is not None else None
    s = torch.empty((n, 3), dtype=torch.float32, device=dev)
    keys = torch.empty((n, 4), dtype=torch.int32, device=dev)
    if n:
        check(_lib.lib().cnc_envmap_backward_rays(ptr(g_out), ptr(opacity), ptr(cell), ptr(frac), ptr(texture), H, n,
                                                  ptr(g_opacity), ptr(s), ptr(keys), stream(dev)), "envmap_backward_rays")
    return g_opacity, s, keys


def envmap_backward_texture(keys, frac, s, H):
    """-> g_texture [H, 2H, 3]: per texel the sum of its contributions in the fixed order of the header.  The grouping is
    plumbing — a stable sort of the 4 n integer keys and one searchsorted for the segment bounds; the sum is the kernel.
    n == 0: zeros, no launch."""
    H = check_resolution(H)
    n = keys.shape[0]
    check_input(keys, "keys")
    if keys.dtype != torch.int32 or tuple(keys.shape) != (n, 4):
        raise RuntimeError("envmap: keys must be int32 [n, 4]")
    _f32(frac, "frac", (n, 2))
    _f32(s, "s", (n, 3))
    dev = keys.device
    if n == 0:
        return torch.zeros((H, 2 * H, 3), dtype=torch.float32, device=dev)
    g_texture = torch.empty((H, 2 * H, 3), dtype=torch.float32, device=dev)
    sorted_keys, order = torch.sort(keys.view(-1), stable=True)
    bounds = torch.arange(2 * H * H + 1, dtype=torch.int32, device=dev)
    offsets = torch.searchsorted(sorted_keys, bounds).contiguous()           # int64 [H W + 1]
    check(_lib.lib().cnc_envmap_backward_texture(ptr(order), ptr(offsets), ptr(frac), ptr(s), H, n, ptr(g_texture),
                                                 stream(dev)), "envmap_backward_texture")
    return g_texture
