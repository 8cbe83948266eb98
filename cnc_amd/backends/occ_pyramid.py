"""Thin mirror of the occupancy pyramid's kernels (cnc_amd/csrc/occ_pyramid.hip, include/cnc_hip.h).

Every function writes buffers the caller owns; nothing is allocated here and nothing waits for the device.  Grids and
levels are uint8 [n_grids, x, y, z] tensors, candidates int32 / uint8 / float32 vectors.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream


def _grid4(t, name):
    check_input(t, name)
    if t.dtype != torch.uint8 or t.dim() != 4:
        raise RuntimeError(f"{name}: expected a uint8 [n_grids, x, y, z] tensor")
    return [int(s) for s in t.shape]


def reduce(grid, levels, coarse):
    """Levels 1..levels of `grid` into `coarse` (uint8, level 1 first, back to back)."""
    G, rx, ry, rz = _grid4(grid, "grid")
    check_input(coarse, "coarse")
    need = sum(G * (rx >> k) * (ry >> k) * (rz >> k) for k in range(1, int(levels) + 1))
    if coarse.dtype != torch.uint8 or coarse.numel() < need:
        raise RuntimeError(f"coarse: expected at least {need} uint8 elements")
    check(_lib.lib().cnc_occ_reduce(ptr(grid), G, rx, ry, rz, int(levels), ptr(coarse), stream(grid.device)), "occ_reduce")


def rank_scratch_words(n_parents):
    """int32 elements of `rank`'s scratch for a parent level of n_parents cells."""
    nbytes = int(_lib.lib().cnc_occ_rank_scratch_bytes(int(n_parents)))
    if nbytes == 0:
        raise RuntimeError(f"occ_rank: unsupported parent level of {n_parents} cells")
    return nbytes // 4


def rank(parent, scratch, n_expected=-1, status=None):
    """Exclusive offsets of the occupied parents per 256-parent block into `scratch` (int32), their number in its last
    word.  n_expected >= 0: compared with 8 x that number on the device, `status` (int32 [1]) flags a difference."""
    _grid4(parent, "parent")
    check_input(scratch, "scratch")
    if status is not None:
        check_input(status, "status")
    if scratch.dtype != torch.int32 or (status is not None and status.dtype != torch.int32):
        raise RuntimeError("occ_rank: scratch and status are int32 tensors")
    check(_lib.lib().cnc_occ_rank(ptr(parent), parent.numel(), int(n_expected), ptr(scratch), scratch.numel() * 4, ptr(status),
                                  stream(parent.device)), "occ_rank")


def emit(parent, scratch, n_cap, ctx, idx=None, child=None, sym=None, hist=None):
    """Candidates [0, n_cap) of the level below `parent`: ctx (uint8), idx (int32, optional); with `child` also the
    symbols sym (float32 +-1) and the (ctx -> ones, total) histogram hist (int32 [32, 2], zeroed by the caller)."""
    G, px, py, pz = _grid4(parent, "parent")
    check_input(scratch, "scratch")
    check_input(ctx, "ctx")
    n_cap = int(n_cap)
    if ctx.dtype != torch.uint8 or ctx.numel() < n_cap:
        raise RuntimeError("ctx: expected a uint8 tensor of n_cap elements")
    if idx is not None:
        check_input(idx, "idx")
        if idx.dtype != torch.int32 or idx.numel() < n_cap:
            raise RuntimeError("idx: expected an int32 tensor of n_cap elements")
    if child is not None:
        if _grid4(child, "child") != [G, 2 * px, 2 * py, 2 * pz]:
            raise RuntimeError("child: expected the level below parent")
    if sym is not None:
        check_input(sym, "sym")
        if child is None or sym.dtype != torch.float32 or sym.numel() < n_cap:
            raise RuntimeError("sym: expected a float32 tensor of n_cap elements, and child")
    if hist is not None:
        check_input(hist, "hist")
        if child is None or hist.dtype != torch.int32 or hist.numel() != 64:
            raise RuntimeError("hist: expected an int32 [32, 2] tensor, and child")
    if scratch.dtype != torch.int32 or scratch.numel() < rank_scratch_words(parent.numel()):
        raise RuntimeError("scratch: expected what rank() filled for this parent level")
    check(_lib.lib().cnc_occ_emit(ptr(parent), ptr(child), G, px, py, pz, ptr(scratch), n_cap, ptr(idx), ptr(ctx), ptr(sym),
                                  ptr(hist), stream(parent.device)), "occ_emit")


def probs(ctx, table, p):
    """p[i] = table[ctx[i]] for the len(p) first candidates; table: float32 [32]."""
    check_input(ctx, "ctx")
    check_input(table, "table")
    check_input(p, "p")
    if ctx.dtype != torch.uint8 or table.dtype != torch.float32 or p.dtype != torch.float32:
        raise RuntimeError("occ_probs: expected uint8 ctx, float32 table and p")
    if table.numel() != 32 or ctx.numel() < p.numel():
        raise RuntimeError("occ_probs: expected a 32-entry table and len(ctx) >= len(p)")
    check(_lib.lib().cnc_occ_probs(ptr(ctx), p.numel(), ptr(table), ptr(p), stream(p.device)), "occ_probs")


def scatter(sym, idx, scratch, n_parents, child, status):
    """child[idx[i]] = 1 where sym[i] > 0, for the candidates both the header (len(sym)) and the parent level have."""
    check_input(sym, "sym")
    check_input(idx, "idx")
    check_input(scratch, "scratch")
    check_input(status, "status")
    _grid4(child, "child")
    if sym.dtype != torch.float32 or idx.dtype != torch.int32 or idx.numel() < sym.numel():
        raise RuntimeError("occ_scatter: expected float32 sym and an int32 idx at least as long")
    if scratch.dtype != torch.int32 or status.dtype != torch.int32 or scratch.numel() < rank_scratch_words(n_parents):
        raise RuntimeError("occ_scatter: scratch (what rank() filled) and status are int32 tensors")
    check(_lib.lib().cnc_occ_scatter(ptr(sym), ptr(idx), sym.numel(), ptr(scratch), int(n_parents), ptr(child), child.numel(),
                                     ptr(status), stream(child.device)), "occ_scatter")
