"""Thin mirror of the connected-component kernels (cnc_amd/csrc/components.hip, include/cnc_hip.h).

Every function writes buffers the caller owns; nothing is allocated here and nothing waits for the device.  `mask` is
uint8 [n_grids, d0, d1, d2] (non-zero = set), `labels` and `sizes` int32 of the same shape, `faces` int32 [F, 3].
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream

CONNECTIVITIES = (6, 14, 26)


def _grid(t, dtype, name):
    check_input(t, name)
    if t.dtype != dtype or t.dim() != 4:
        raise RuntimeError(f"{name}: expected a {dtype} tensor [n_grids, d0, d1, d2], got {t.dtype} with {t.dim()} dimensions")
    if min(t.shape) < 1 or t.numel() >= 2 ** 31:
        raise RuntimeError(f"{name}: a grid of shape {tuple(t.shape)} is empty or has 2^31 cells or more")
    return tuple(int(v) for v in t.shape)


def _same(t, shape, dtype, name):
    check_input(t, name)
    if t.dtype != dtype or tuple(t.shape) != shape:
        raise RuntimeError(f"{name}: expected a {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")


def label_grid(mask, connectivity, labels):
    """labels[g, i0, i1, i2] = the smallest linear index within grid g of the cell's component, -1 for an unset cell."""
    if int(connectivity) not in CONNECTIVITIES:
        raise RuntimeError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity}")
    n, d0, d1, d2 = shape = _grid(mask, torch.uint8, "mask")
    _same(labels, shape, torch.int32, "labels")
    check(_lib.lib().cnc_components_label_grid(ptr(mask), n, d0, d1, d2, int(connectivity), ptr(labels), stream(mask.device)),
          "components_label_grid")


def sizes(labels, out):
    """out = the component's cell count at every root (labels[i] == i), 0 everywhere else; zeroed by the call."""
    n, d0, d1, d2 = shape = _grid(labels, torch.int32, "labels")
    _same(out, shape, torch.int32, "sizes")
    check(_lib.lib().cnc_components_sizes(ptr(labels), n, d0, d1, d2, ptr(out), stream(labels.device)), "components_sizes")


def label_graph(faces, n_vertices, labels):
    """labels[v] = the smallest vertex index of v's component under the faces' edges; v itself where no face uses it."""
    check_input(faces, "faces")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces: expected an int32 [F, 3] tensor")
    n_vertices = int(n_vertices)
    if n_vertices < 0 or n_vertices >= 2 ** 31 or 3 * faces.shape[0] >= 2 ** 31:
        raise RuntimeError(f"label_graph: {n_vertices} vertices and {faces.shape[0]} faces: V and 3 F must stay below 2^31")
    check_input(labels, "labels")
    if labels.dtype != torch.int32 or labels.dim() != 1 or labels.shape[0] != n_vertices:
        raise RuntimeError(f"labels: expected an int32 vector of {n_vertices} elements")
    check(_lib.lib().cnc_components_label_graph(ptr(faces) if faces.shape[0] else None, int(faces.shape[0]), n_vertices,
                                                ptr(labels) if n_vertices else None, stream(labels.device)),
          "components_label_graph")
