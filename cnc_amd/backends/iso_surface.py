"""Thin mirror of the mesh export's kernels (cnc_amd/csrc/iso_surface.hip, include/cnc_hip.h).

Every function writes buffers the caller owns; nothing is allocated here and nothing waits for the device.  `n` is the
lattice's cell count (nx, ny, nz); the density lattice is float32 [nz + 1, ny + 1, nx + 1] (any shape with that many
elements), masks and counts are uint8, the two prefix sums int32, `lo` / `h` three host float32 each
(cnc_amd.mesh.spacing), `table` the int8 vector of cnc_amd.mesh.tet_table().
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import check, check_cuda, check_input, ptr, stream

TABLE = _lib.CNC_ISO_TABLE


def _cells(n):
    nx, ny, nz = (int(v) for v in n)
    if min(nx, ny, nz) < 1 or (nx + 1) * (ny + 1) * (nz + 1) >= 2 ** 31:
        raise RuntimeError(f"iso_surface: a lattice of {(nx, ny, nz)} cells is empty or has 2^31 points or more")
    return nx, ny, nz, (nx + 1) * (ny + 1) * (nz + 1), nx * ny * nz


def _buffer(t, dtype, name, numel, exact=True):
    check_input(t, name)
    if t.dtype != dtype or (t.numel() != numel if exact else t.numel() < numel):
        raise RuntimeError(f"{name}: expected a {dtype} tensor of {'' if exact else 'at least '}{numel} elements, "
                           f"got {t.dtype} with {t.numel()}")


def _vec3(v, name):
    a = np.asarray(v, np.float32).reshape(-1)
    if a.size != 3:
        raise RuntimeError(f"{name}: expected three numbers")
    return (C.c_float * 3)(*a.tolist())


def _table(table):
    _buffer(table, torch.int8, "table", TABLE)


def active_points(occupancy, n, active):
    """active[lin] = 1 where a set cell of `occupancy` (bool or uint8 [Gx, Gy, Gz] over the lattice's box) overlaps
    [p - h, p + h], else 0; active: uint8, one per lattice point."""
    nx, ny, nz, points, _ = _cells(n)
    check_input(occupancy, "occupancy")
    if occupancy.dim() != 3 or occupancy.dtype not in (torch.bool, torch.uint8) or occupancy.numel() < 1:
        raise RuntimeError("occupancy: expected a non-empty bool or uint8 tensor [Gx, Gy, Gz]")
    _buffer(active, torch.uint8, "active", points)
    gx, gy, gz = occupancy.shape
    check(_lib.lib().cnc_iso_active_points(ptr(occupancy), gx, gy, gz, nx, ny, nz, ptr(active), stream(active.device)),
          "iso_active_points")


def lattice_positions(lin, first, m, n, lo, h, positions):
    """positions[i] = the position of lattice point lin[i] (int64 vector), or of point first + i when lin is None;
    positions: float32, at least [m, 3]."""
    nx, ny, nz, points, _ = _cells(n)
    m = int(m)
    if lin is not None:
        _buffer(lin, torch.int64, "lin", m, exact=False)
    elif int(first) < 0 or int(first) + m > points:
        raise RuntimeError(f"lattice_positions: points [{first}, {int(first) + m}) are not all in a lattice of {points}")
    _buffer(positions, torch.float32, "positions", 3 * m, exact=False)
    check(_lib.lib().cnc_iso_lattice_positions(ptr(lin), int(first), m, nx, ny, nz, _vec3(lo, "lo"), _vec3(h, "h"), ptr(positions),
                                               stream(positions.device)), "iso_lattice_positions")


def classify(density, n, threshold, cap, table, edge_mask, cell_tris):
    """The capping of `density` in place (cap), a point's 7-bit edge mask and a cell's triangle count (0..12)."""
    nx, ny, nz, points, cells = _cells(n)
    _buffer(density, torch.float32, "density", points)
    _table(table)
    _buffer(edge_mask, torch.uint8, "edge_mask", points)
    _buffer(cell_tris, torch.uint8, "cell_tris", cells)
    check(_lib.lib().cnc_iso_classify(ptr(density), nx, ny, nz, float(threshold), 1 if cap else 0, ptr(table), ptr(edge_mask),
                                      ptr(cell_tris), stream(density.device)), "iso_classify")


def emit_vertices(density, n, threshold, lo, h, edge_mask, vertex_scan, vertices, normals=None):
    """vertices (and normals, when given): float32 [V, 3], V = the masks' total popcount; vertex_scan: the exclusive
    prefix sum of the masks' popcounts, int32."""
    nx, ny, nz, points, _ = _cells(n)
    _buffer(density, torch.float32, "density", points)
    _buffer(edge_mask, torch.uint8, "edge_mask", points)
    _buffer(vertex_scan, torch.int32, "vertex_scan", points)
    check_input(vertices, "vertices")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices: expected a float32 [V, 3] tensor")
    if normals is not None:
        _buffer(normals, torch.float32, "normals", vertices.numel())
    check(_lib.lib().cnc_iso_emit_vertices(ptr(density), nx, ny, nz, float(threshold), _vec3(lo, "lo"), _vec3(h, "h"), ptr(edge_mask),
                                           ptr(vertex_scan), vertices.shape[0], ptr(vertices), ptr(normals),
                                           stream(vertices.device)), "iso_emit_vertices")


def emit_faces(density, n, threshold, table, edge_mask, vertex_scan, cell_tris, cell_scan, n_vertices, faces):
    """faces: int32 [F, 3], F = the cells' total triangle count; cell_scan: the exclusive prefix sum of cell_tris, int32."""
    nx, ny, nz, points, cells = _cells(n)
    _buffer(density, torch.float32, "density", points)
    _table(table)
    _buffer(edge_mask, torch.uint8, "edge_mask", points)
    _buffer(vertex_scan, torch.int32, "vertex_scan", points)
    _buffer(cell_tris, torch.uint8, "cell_tris", cells)
    _buffer(cell_scan, torch.int32, "cell_scan", cells)
    check_input(faces, "faces")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError("faces: expected an int32 [F, 3] tensor")
    check(_lib.lib().cnc_iso_emit_faces(ptr(density), nx, ny, nz, float(threshold), ptr(table), ptr(edge_mask), ptr(vertex_scan),
                                        ptr(cell_tris), ptr(cell_scan), int(n_vertices), faces.shape[0], ptr(faces),
                                        stream(faces.device)), "iso_emit_faces")
