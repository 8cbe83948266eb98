"""Thin mirror of the MLP section's kernels (cnc_amd/csrc/mlp_tree.hip, include/cnc_hip.h).

Every function writes buffers the caller owns; nothing is allocated here and nothing waits for the device.  Indices and
prefixes are int16 tensors that carry uint16 bits, the descriptor table is int32 [n_tensors, 16] (cnc_amd.mlp_codec
builds it), symbols and probabilities are float32 vectors, raw low bits uint8.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream

DESC = _lib.CNC_MLP_TREE_DESC


def _common(q, desc, bits, name):
    check_input(q, name)
    check_input(desc, "desc")
    if q.dtype != torch.int16 or q.dim() != 1 or q.numel() < 1:
        raise RuntimeError(f"{name}: expected a non-empty int16 vector (uint16 bits)")
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != DESC or desc.shape[0] < 1:
        raise RuntimeError(f"desc: expected an int32 [n_tensors, {DESC}] tensor")
    if not 8 <= int(bits) <= 16:
        raise RuntimeError(f"mlp_tree: bits must be 8 ... 16, got {bits}")
    return q.numel(), int(desc.shape[0])


def _vector(t, dtype, name, at_least=0):
    check_input(t, name)
    if t.dtype != dtype or t.numel() < at_least:
        raise RuntimeError(f"{name}: expected a {dtype} tensor of at least {at_least} elements")


def hist(q, desc, bits, out):
    """out[t, q >> (bits - 8)] += 1; out: int32 [n_tensors, 256], zeroed by the caller."""
    n, T = _common(q, desc, bits, "q")
    _vector(out, torch.int32, "hist")
    if out.numel() != T * 256:
        raise RuntimeError("hist: expected an int32 [n_tensors, 256] tensor")
    check(_lib.lib().cnc_mlp_tree_hist(ptr(q), n, ptr(desc), T, int(bits), ptr(out), stream(q.device)), "mlp_tree_hist")


def emit(q, desc, bits, tables, plane_base, sym, p):
    """Every plane's symbols and probabilities in one launch; plane j's stream starts at plane_base[j] (8 host ints) of
    sym / p (float32, equally long)."""
    n, T = _common(q, desc, bits, "q")
    if len(plane_base) != 8:
        raise RuntimeError("plane_base: expected 8 integers")
    _vector(sym, torch.float32, "sym")
    _vector(p, torch.float32, "p", sym.numel())
    if sym.numel():
        _vector(tables, torch.float32, "tables", 1)
    base = (C.c_int64 * 8)(*[int(v) for v in plane_base])
    check(_lib.lib().cnc_mlp_tree_emit(ptr(q), n, ptr(desc), T, int(bits), ptr(tables), 0 if tables is None else tables.numel(),
                                       base, ptr(sym), ptr(p), sym.numel(), stream(q.device)), "mlp_tree_emit")


def probs(prefix, desc, bits, plane, tables, p):
    """Plane `plane`'s probabilities from the bits decoded so far; p: float32, the plane's symbol count long."""
    n, T = _common(prefix, desc, bits, "prefix")
    _vector(p, torch.float32, "p")
    _vector(tables, torch.float32, "tables", 1)
    check(_lib.lib().cnc_mlp_tree_probs(ptr(prefix), n, ptr(desc), T, int(bits), int(plane), ptr(tables), tables.numel(), ptr(p),
                                        p.numel(), stream(p.device)), "mlp_tree_probs")


def fold(sym, prefix, desc, bits, plane):
    """prefix = prefix << 1 | (sym > 0) for the elements plane `plane` codes."""
    n, T = _common(prefix, desc, bits, "prefix")
    _vector(sym, torch.float32, "sym")
    check(_lib.lib().cnc_mlp_tree_fold(ptr(sym), sym.numel(), ptr(prefix), n, ptr(desc), T, int(bits), int(plane),
                                       stream(prefix.device)), "mlp_tree_fold")


def pack_low(q, desc, bits, low):
    """Every tensor's raw low bits into `low` (uint8, all of it written)."""
    n, T = _common(q, desc, bits, "q")
    _vector(low, torch.uint8, "low")
    check(_lib.lib().cnc_mlp_tree_pack_low(ptr(q), n, ptr(desc), T, int(bits), ptr(low), low.numel(), stream(q.device)),
          "mlp_tree_pack_low")


def unpack(prefix, desc, bits, low, q):
    """q = prefix << r | raw low bits, for every element."""
    n, T = _common(prefix, desc, bits, "prefix")
    _vector(low, torch.uint8, "low")
    _vector(q, torch.int16, "q", n)
    check(_lib.lib().cnc_mlp_tree_unpack(ptr(prefix), n, ptr(desc), T, int(bits), ptr(low) if low.numel() else None, low.numel(),
                                         ptr(q), stream(q.device)), "mlp_tree_unpack")
