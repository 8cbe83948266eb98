"""Context-coded occupancy grid: the "pyramid1" model.

The grid's levels are ORs over 2x2x2 blocks; the coarsest level is stored raw, every finer level codes only the eight
children of its occupied parents, each with a static probability per (level, context) where the context counts the
occupied parent-level neighbours on the child's side (`near`, 0..7) and on the opposite faces (`far`, 0..3).  Every
probability of a level is known before its first symbol is coded, so a level is ONE stream of independent symbols for
the host range coder and for the device coder alike.

    payload = raw coarsest level (bit-packed, C order, bit i of byte i >> 3 at i & 7)
            | c1 tables: levels x 32 x u16 LE, level 0 first        (c1 = P(empty) * 2^16, what the coders quantise to)
            | one stream per level with candidates, coarse to fine  (sizes in info["stream_sizes"])

The candidate lists, contexts, symbols and histograms are built on the device (backends/occ_pyramid.py); an encode
reads the device once (counts, histograms and the coarsest level together) before it hands the streams to the coder.
The module imports without a GPU; its host helpers are what tests/occ_pyramid_twin.py is compared with.
"""
from __future__ import annotations

import os
import tempfile
from typing import Dict, List, Tuple

import numpy as np
import torch

MODEL = "pyramid1"
MAX_LEVELS = 4
N_CTX = 32
UNUSED_C1 = 32768


def levels_of(shape) -> int:
    """K = min(4, trailing zero bits of gcd(rx, ry, rz)); ValueError when that is 0 (the caller keeps the iid coder)."""
    if len(shape) != 4 or min(int(s) for s in shape) < 1:
        raise ValueError(f"occupancy pyramid: expected a [n_grids, rx, ry, rz] grid, got {list(shape)}")
    g = int(np.gcd.reduce([int(s) for s in shape[1:]]))
    K = min(MAX_LEVELS, (g & -g).bit_length() - 1)
    if K == 0:
        raise ValueError(f"occupancy pyramid: a grid of {list(shape[1:])} has an odd side and no coarser level")
    return K


def level_shape(shape, k) -> Tuple[int, int, int, int]:
    return (int(shape[0]), int(shape[1]) >> k, int(shape[2]) >> k, int(shape[3]) >> k)


def c1_of_counts(ones: int, total: int) -> int:
    """c1 = P(symbol = -1) * 2^16 of a context with `ones` occupied children among `total` candidates: the empty
    fraction rounded half up to 16 bits and kept inside [1, 65535]; 32768 for a context nobody used."""
    if total == 0:
        return UNUSED_C1
    return min(65535, max(1, ((total - ones) * 131072 + total) // (2 * total)))


def p_of_c1(c1) -> np.ndarray:
    """The float32 P(+1) whose quantisation by either coder (rans::c1_of, the range coder's cdf_one) is c1 again, for
    every c1 in [1, 65535] (tests/test_occ_pyramid_twin.py walks all of them)."""
    c1 = np.asarray(c1, dtype=np.float64)
    return (1.0 - (c1 - 1.0) / 65534.0).astype(np.float32)


def _check_header(info) -> Tuple[List[int], int, List[int], List[int]]:
    if info.get("model") != MODEL:
        raise RuntimeError(f"occupancy section: unknown model {info.get('model')!r}")
    shape = [int(s) for s in info["shape"]]
    K = levels_of(shape)
    n, sizes = [int(v) for v in info["n"]], [int(v) for v in info["stream_sizes"]]
    if int(info["levels"]) != K or len(n) != K or len(sizes) != K:
        raise RuntimeError("occupancy section: header does not describe the grid's levels")
    for k in range(K):
        if n[k] < 0 or n[k] % 8 or n[k] > int(np.prod(level_shape(shape, k))) or sizes[k] < 0 or (n[k] == 0) != (sizes[k] == 0):
            raise RuntimeError(f"occupancy section: impossible candidate count or stream size at level {k}")
    return shape, K, n, sizes


def split_payload(payload: bytes, info) -> Tuple[np.ndarray, np.ndarray, List[bytes]]:
    """(coarsest level as uint8 [G, x, y, z], c1 tables uint16 [K, 32], streams by level: b"" where a level has none).
    RuntimeError for a payload whose length is not what the header says."""
    shape, K, n, sizes = _check_header(info)
    top = level_shape(shape, K)
    n_top = int(np.prod(top))
    n_raw, n_tab = (n_top + 7) // 8, K * N_CTX * 2
    if len(payload) != n_raw + n_tab + sum(sizes):
        raise RuntimeError(f"occupancy section: {len(payload)} bytes, the header describes {n_raw + n_tab + sum(sizes)}")
    raw = np.unpackbits(np.frombuffer(payload[:n_raw], dtype=np.uint8), bitorder="little")[:n_top].reshape(top)
    c1 = np.frombuffer(payload[n_raw:n_raw + n_tab], dtype="<u2").astype(np.uint16).reshape(K, N_CTX)
    if int(c1.min()) < 1:
        raise RuntimeError("occupancy section: a zero probability in the tables")
    streams, at = [b""] * K, n_raw + n_tab
    for k in range(K - 1, -1, -1):
        streams[k] = payload[at:at + sizes[k]]
        at += sizes[k]
    return raw, c1, streams


def join_payload(top_level: np.ndarray, c1: np.ndarray, streams: List[bytes]) -> bytes:
    raw = np.packbits(np.asarray(top_level, dtype=np.uint8).reshape(-1), bitorder="little").tobytes()
    return raw + np.asarray(c1).astype("<u2").tobytes() + b"".join(streams[k] for k in range(len(streams) - 1, -1, -1))


@torch.no_grad()
def encode_occupancy(binaries: torch.Tensor, coder: str = "host", symbols_per_lane=None) -> Tuple[bytes, Dict]:
    """binaries: bool / uint8 [n_grids, rx, ry, rz] on the GPU.  Returns (payload, info); info is the section's header
    entry (plus `c1`, which the payload carries and a header need not repeat)."""
    from .backends import occ_pyramid as B
    from .coders import make_coder
    if not binaries.is_cuda:
        raise RuntimeError("binaries must be a CUDA tensor")
    shape = [int(s) for s in binaries.shape]
    K = levels_of(shape)
    dev = binaries.device
    coders = make_coder(coder, symbols_per_lane)
    g0 = binaries.contiguous()
    g0 = g0.view(torch.uint8) if g0.dtype == torch.bool else g0.to(torch.uint8)
    shapes = [level_shape(shape, k) for k in range(K + 1)]
    cells = [int(np.prod(s)) for s in shapes]
    coarse = torch.empty(sum(cells[1:]), dtype=torch.uint8, device=dev)
    B.reduce(g0, K, coarse)
    levels, at = [g0], 0
    for k in range(1, K + 1):
        levels.append(coarse[at:at + cells[k]].view(shapes[k]))
        at += cells[k]
    # one int32 block: the K histograms, then every level's rank scratch — read back in one copy with the coarsest level
    words = [B.rank_scratch_words(cells[k + 1]) for k in range(K)]
    work = torch.zeros(K * 64 + sum(words), dtype=torch.int32, device=dev)
    scr, at = [], K * 64
    for k in range(K):
        scr.append(work[at:at + words[k]])
        at += words[k]
    ctx = [torch.empty(cells[k], dtype=torch.uint8, device=dev) for k in range(K)]       # at most every child is a candidate
    sym = [torch.empty(cells[k], dtype=torch.float32, device=dev) for k in range(K)]
    for k in range(K - 1, -1, -1):
        B.rank(levels[k + 1], scr[k])
        B.emit(levels[k + 1], scr[k], cells[k], ctx[k], child=levels[k], sym=sym[k], hist=work[k * 64:(k + 1) * 64])
    host = torch.cat([work.view(torch.uint8), levels[K].reshape(-1)]).cpu().numpy()      # the encode's one host read
    wh = host[:work.numel() * 4].view(np.int32)
    top = host[work.numel() * 4:]
    n, at = [], K * 64
    for k in range(K):
        n.append(8 * int(wh[at + words[k] - 1]))
        at += words[k]
    hist = wh[:K * 64].reshape(K, N_CTX, 2).astype(np.int64)
    c1 = np.array([[c1_of_counts(int(o), int(t)) for o, t in hist[k]] for k in range(K)], dtype=np.uint16)
    tables = torch.from_numpy(p_of_c1(c1)).to(dev)
    streams = [b""] * K
    with tempfile.TemporaryDirectory() as td:
        files = {}
        for k in range(K - 1, -1, -1):
            if n[k] == 0:
                continue
            p = torch.empty(n[k], dtype=torch.float32, device=dev)
            B.probs(ctx[k], tables[k], p)
            files[k] = os.path.join(td, f"occ{k}.b")
            coders.encode(sym[k][:n[k]], p, files[k])
        coders.finish()
        for k, f in files.items():
            with open(f, "rb") as fin:
                streams[k] = fin.read()
    coders.shutdown()
    info = dict(model=MODEL, shape=shape, levels=K, n=n, c1=c1.astype(int).tolist(), stream_sizes=[len(s) for s in streams],
                coder="rans1" if coder == "device" else "range")
    return join_payload(top, c1, streams), info


@torch.no_grad()
def decode_occupancy(payload: bytes, info: Dict, device, coder=None) -> torch.Tensor:
    """Inverse of encode_occupancy: the bool grid on `device` (a GPU).  `coder`: what wrote the streams, default what the
    header names.  RuntimeError for a payload or header that does not fit the grid it describes."""
    from .backends import occ_pyramid as B
    from .coders import make_coder
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_occupancy: a pyramid1 occupancy section decodes on the GPU only (no CPU path)")
    fmt = info.get("coder", "range")
    if fmt not in ("range", "rans1"):
        raise RuntimeError(f"occupancy section: streams in an unknown format {fmt!r}")
    if coder is None:
        coder = "device" if fmt == "rans1" else "host"
    coders = make_coder(coder)
    shape, K, n, _ = _check_header(info)
    top, c1, streams = split_payload(payload, info)
    tables = torch.from_numpy(p_of_c1(c1)).to(device)
    shapes = [level_shape(shape, k) for k in range(K + 1)]
    cells = [int(np.prod(s)) for s in shapes]
    status = torch.zeros(1, dtype=torch.int32, device=device)
    parent = torch.from_numpy(np.ascontiguousarray(top)).to(device)
    with tempfile.TemporaryDirectory() as td:
        for k in range(K - 1, -1, -1):
            child = torch.zeros(shapes[k], dtype=torch.uint8, device=device)
            scratch = torch.empty(B.rank_scratch_words(cells[k + 1]), dtype=torch.int32, device=device)
            B.rank(parent, scratch, n_expected=n[k], status=status)
            if n[k] > 0:
                idx = torch.zeros(n[k], dtype=torch.int32, device=device)
                ctx = torch.zeros(n[k], dtype=torch.uint8, device=device)
                B.emit(parent, scratch, n[k], ctx, idx=idx)
                p = torch.empty(n[k], dtype=torch.float32, device=device)
                B.probs(ctx, tables[k], p)
                f = os.path.join(td, f"occ{k}.b")
                with open(f, "wb") as fout:
                    fout.write(streams[k])
                sym, = coders.decode_group([(p, f)])
                B.scatter(sym, idx, scratch, cells[k + 1], child, status)
            parent = child
    coders.check()
    coders.shutdown()
    flags = int(status.item())                                                         # the decode's one wait
    if flags:
        raise RuntimeError(f"occupancy section: the header's candidate counts do not fit the decoded grid (status {flags})")
    return parent.view(torch.bool) if parent.dtype == torch.uint8 else parent
