"""Entropy-coded MLP section: the "tree1" model.

Every MLP tensor is quantised exactly as the packed sections quantise it (container.quantize_tensor: `bits`-wide indices,
`lo`, `interval`), so the decoded MLP is bit for bit the packed one.  Per tensor a depth d in 0..8: the top d bits of an
index walk a binary tree whose node for plane j (bit bits - 1 - j) under the j bits above it, `pi`, has heap index
2^j - 1 + pi and carries c1 = P(bit = 0) * 2^16 from the tensor's own counts; the low r = bits - d bits are stored raw.
All probabilities of plane j are known once planes 0..j-1 are decoded, so a plane — over every tensor deep enough — is
ONE stream of independent symbols for the host range coder and for the device coder alike: at most 8 rounds a decode.

    payload = c1 tables: tensor by tensor, (2^d - 1) x u16 LE in heap order
            | low bits: tensor by tensor, N values of r bits in the bit order of container._pack_bits, each tensor padded
                        to a whole byte (nothing for r = 0)
            | D = max depth streams, plane 0 first           (sizes in info["stream_sizes"])

Histograms, symbols, probabilities and the raw bits are built on the device (backends/mlp_tree.py); once the tensors are
quantised, an encode reads the device once (the histograms) before it hands the streams to the coder.  The module
imports without a GPU; its host helpers are what tests/mlp_tree_twin.py is compared with.
"""
from __future__ import annotations

import math
import os
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .occupancy_codec import c1_of_counts, p_of_c1

MODEL = "tree1"
MAX_DEPTH = 8
MIN_BITS, MAX_BITS = 8, 16
DESC = 16                       # int32 per tensor of the kernels' descriptor table (CNC_MLP_TREE_DESC)
MAX_TENSORS = 65536


def check_bits(bits) -> int:
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not MIN_BITS <= int(bits) <= MAX_BITS:
        raise ValueError(f"the tree1 MLP coder takes bits in {MIN_BITS} ... {MAX_BITS}, got {bits!r}")
    return int(bits)


def _node_counts(hist, j):
    """(zeros, ones) of the 2^j nodes of plane j, by prefix, from a 256-bin histogram of the indices' top 8 bits."""
    g = np.asarray(hist, dtype=np.int64).reshape(1 << (j + 1), -1).sum(axis=1)
    return g[0::2], g[1::2]


def tables_of_hist(hist, depth: int) -> np.ndarray:
    """The c1 of a tensor's 2^depth - 1 nodes in heap order (uint16); 32768 for a node no element visits."""
    out = np.empty((1 << depth) - 1, dtype=np.uint16)
    for j in range(depth):
        zeros, ones = _node_counts(hist, j)
        for pi in range(1 << j):
            out[(1 << j) - 1 + pi] = c1_of_counts(int(ones[pi]), int(zeros[pi] + ones[pi]))
    return out


def depth_costs(hist, n: int, bits: int) -> List[float]:
    """cost(d) in bits, d = 0..8: 16 (2^d - 1) for the tables, the code length of the modelled bits under the 16-bit
    probabilities the coders use, N (bits - d) for the raw rest.  float64, nodes in heap order."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1)
    if hist.size != 256 or int(hist.sum()) != int(n) or int(hist.min()) < 0:
        raise ValueError("depth_costs: expected a 256-bin histogram of n elements")
    costs, coded = [float(n * bits)], 0.0
    for j in range(MAX_DEPTH):
        zeros, ones = _node_counts(hist, j)
        for pi in range(1 << j):
            z, o = int(zeros[pi]), int(ones[pi])
            if z + o == 0:
                continue
            c1 = c1_of_counts(o, z + o)
            coded += z * -math.log2(c1 / 65536.0)
            coded += o * -math.log2(1.0 - c1 / 65536.0)
        d = j + 1
        costs.append(16.0 * ((1 << d) - 1) + coded + float(n * (bits - d)))
    return costs


def choose_depth(hist, n: int, bits: int) -> int:
    """The depth of smallest cost; ties go to the smaller depth."""
    costs = depth_costs(hist, n, check_bits(bits))
    return int(min(range(MAX_DEPTH + 1), key=lambda d: (costs[d], d)))


def low_bytes(n: int, r: int) -> int:
    return (n * r + 7) // 8


def layout(counts: Sequence[int], depths: Sequence[int], bits: int) -> Dict:
    """Where everything of the section lies: the kernels' descriptor table (int32 [T, 16]: first element, elements, depth,
    first table entry, first low byte, 0, 0, 0, first symbol in planes 0..7), the totals and the planes' symbol counts."""
    T = len(counts)
    desc = np.zeros((T, DESC), dtype=np.int64)
    off = tab = low = 0
    plane_n = [0] * MAX_DEPTH
    for t, (n, d) in enumerate(zip(counts, depths)):
        desc[t, :5] = (off, n, d, tab, low)
        for j in range(MAX_DEPTH):
            desc[t, 8 + j] = plane_n[j]
            if j < d:
                plane_n[j] += n
        off += n
        tab += (1 << d) - 1
        low += low_bytes(n, bits - d)
    if off > 2 ** 31 - 1 or low > 2 ** 31 - 1:
        raise RuntimeError("mlp section: more than 2^31 - 1 elements or raw bytes")
    D = max(depths) if T else 0
    return dict(desc=desc.astype(np.int32), n=off, n_tab=tab, n_low=low, plane_n=plane_n, D=D, tab_at=desc[:, 3].tolist())


def _check_header(info) -> Tuple[int, List[Tuple], List[int], Dict]:
    """(bits, [(name, shape, n, lo, interval, depth)], stream sizes, layout) of a header entry that describes a possible
    section; RuntimeError otherwise."""
    if not isinstance(info, dict) or info.get("model") != MODEL:
        raise RuntimeError(f"mlp section: unknown model {info.get('model')!r}" if isinstance(info, dict) else "mlp section: no header")
    if info.get("coder", "range") not in ("range", "rans1"):
        raise RuntimeError(f"mlp section: streams in an unknown format {info.get('coder')!r}")
    try:
        bits = check_bits(info["bits"])
        entries, sizes = list(info["tensors"]), [int(v) for v in info["stream_sizes"]]
        if not 1 <= len(entries) <= MAX_TENSORS:
            raise ValueError("tensor count")
        tensors, seen = [], set()
        for e in entries:
            name, shape = e["name"], [int(s) for s in e["shape"]]
            depth, lo, interval = e["depth"], float(e["lo"]), float(e["interval"])
            if not isinstance(name, str) or name in seen:
                raise ValueError("tensor name")
            if isinstance(depth, bool) or not isinstance(depth, int) or not 0 <= depth <= MAX_DEPTH:
                raise ValueError("depth")
            if any(s < 1 for s in shape) or math.prod(shape) > 2 ** 31 - 1 or not (math.isfinite(lo) and math.isfinite(interval)):
                raise ValueError("shape or range")
            seen.add(name)
            tensors.append((name, shape, math.prod(shape), lo, interval, depth))
    except (KeyError, TypeError, ValueError) as err:
        raise RuntimeError(f"mlp section: the header does not describe a tree1 section ({err})") from None
    lay = layout([t[2] for t in tensors], [t[5] for t in tensors], bits)
    if len(sizes) != lay["D"] or any(s < 1 for s in sizes):
        raise RuntimeError("mlp section: the header's stream sizes do not fit the tensors' depths")
    return bits, tensors, sizes, lay


def split_payload(payload: bytes, info) -> Tuple[List[np.ndarray], bytes, List[bytes]]:
    """(c1 tables by tensor (uint16, heap order), the raw low bits of every tensor, streams by plane).  RuntimeError for a
    payload whose length is not what the header says, or with a zero probability."""
    _, tensors, sizes, lay = _check_header(info)
    n_tab, n_low = 2 * lay["n_tab"], lay["n_low"]
    if len(payload) != n_tab + n_low + sum(sizes):
        raise RuntimeError(f"mlp section: {len(payload)} bytes, the header describes {n_tab + n_low + sum(sizes)}")
    c1 = np.frombuffer(payload[:n_tab], dtype="<u2").astype(np.uint16)
    if c1.size and int(c1.min()) < 1:
        raise RuntimeError("mlp section: a zero probability in the tables")
    tables = [c1[a:a + (1 << t[5]) - 1] for a, t in zip(lay["tab_at"], tensors)]
    streams, at = [], n_tab + n_low
    for s in sizes:
        streams.append(payload[at:at + s])
        at += s
    return tables, payload[n_tab:n_tab + n_low], streams


def join_payload(tables: Sequence[np.ndarray], low: bytes, streams: Sequence[bytes]) -> bytes:
    return b"".join(np.asarray(c, dtype=np.uint16).astype("<u2").tobytes() for c in tables) + bytes(low) + b"".join(streams)


def _device_vector(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@torch.no_grad()
def encode_mlp(state: Dict[str, torch.Tensor], bits: int = 13, coder: str = "host", symbols_per_lane=None,
               depths: Optional[Sequence[int]] = None) -> Tuple[bytes, Dict]:
    """state: {name: tensor on the GPU}, in the order the section keeps.  Returns (payload, info); info is the section's
    header entry.  `depths` forces the per-tensor depths instead of choosing them by cost: it exists so that tests and the
    measurement can visit every (depth, low-bit width) pair on tiny tensors, and nothing in the product passes it."""
    from .backends import mlp_tree as B
    from .container import quantize_tensor
    from .coders import make_coder
    bits = check_bits(bits)
    coders = make_coder(coder, symbols_per_lane)
    if not state:
        raise ValueError("encode_mlp: no tensors")
    for name, p in state.items():
        if not p.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
        if p.numel() < 1:
            raise ValueError(f"encode_mlp: {name} has no elements")
    names = list(state)
    dev = state[names[0]].device
    qs, los, intervals = [], [], []
    for name in names:
        q, lo, interval = quantize_tensor(state[name].detach().float(), bits)      # what the packed sections hold
        qs.append(q.reshape(-1).astype(np.uint16))
        los.append(lo)
        intervals.append(interval)
    counts = [int(q.size) for q in qs]
    T = len(names)
    if depths is not None:
        depths = [int(d) for d in depths]
        if len(depths) != T or any(not 0 <= d <= MAX_DEPTH for d in depths):
            raise ValueError(f"depths: expected {T} integers in 0 ... {MAX_DEPTH}")
    qd = _device_vector(np.concatenate(qs).view(np.int16), dev)
    hist = torch.zeros((T, 256), dtype=torch.int32, device=dev)
    B.hist(qd, _device_vector(layout(counts, [0] * T, bits)["desc"], dev), bits, hist)
    hist = hist.cpu().numpy().astype(np.int64)                                      # the encode's one read before the streams
    if depths is None:
        depths = [choose_depth(hist[t], counts[t], bits) for t in range(T)]
    c1 = [tables_of_hist(hist[t], depths[t]) for t in range(T)]
    lay = layout(counts, depths, bits)
    desc = _device_vector(lay["desc"], dev)
    base = [0] * MAX_DEPTH
    for j in range(1, MAX_DEPTH):
        base[j] = base[j - 1] + lay["plane_n"][j - 1]
    n_out = sum(lay["plane_n"])
    sym = torch.empty(n_out, dtype=torch.float32, device=dev)
    p = torch.empty(n_out, dtype=torch.float32, device=dev)
    tables = _device_vector(p_of_c1(np.concatenate(c1)), dev) if lay["n_tab"] else None
    B.emit(qd, desc, bits, tables, base, sym, p)
    low = torch.empty(lay["n_low"], dtype=torch.uint8, device=dev)
    B.pack_low(qd, desc, bits, low)
    streams = []
    with tempfile.TemporaryDirectory() as td:
        files = [os.path.join(td, f"mlp{j}.b") for j in range(lay["D"])]
        for j, f in enumerate(files):
            a, b = base[j], base[j] + lay["plane_n"][j]
            coders.encode(sym[a:b], p[a:b], f)
        low_host = low.cpu().numpy().tobytes()
        coders.finish()
        for f in files:
            with open(f, "rb") as fin:
                streams.append(fin.read())
    coders.shutdown()
    info = dict(model=MODEL, coder="rans1" if coder == "device" else "range", bits=bits,
                tensors=[dict(name=n, shape=[int(s) for s in state[n].shape], lo=los[t], interval=intervals[t], depth=depths[t])
                         for t, n in enumerate(names)],
                stream_sizes=[len(s) for s in streams])
    return join_payload(c1, low_host, streams), info


@torch.no_grad()
def decode_indices(payload: bytes, info: Dict, device) -> Dict[str, np.ndarray]:
    """The tensors' quantisation indices (uint32, in their shapes) of a tree1 section, through the coder the header names.
    RuntimeError, before anything is launched, for a payload or a header that do not fit each other; a damaged stream
    gives wrong indices or the device coder's own RuntimeError."""
    from .backends import mlp_tree as B
    from .coders import make_coder
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("decode_mlp: a tree1 MLP section decodes on the GPU only (no CPU path)")
    bits, tensors, _, lay = _check_header(info)
    c1, low, streams = split_payload(payload, info)
    coders = make_coder("device" if info.get("coder", "range") == "rans1" else "host")
    desc = _device_vector(lay["desc"], device)
    tables = _device_vector(p_of_c1(np.concatenate(c1)), device) if lay["n_tab"] else None
    prefix = torch.zeros(lay["n"], dtype=torch.int16, device=device)
    with tempfile.TemporaryDirectory() as td:
        for j in range(lay["D"]):
            p = torch.empty(lay["plane_n"][j], dtype=torch.float32, device=device)
            B.probs(prefix, desc, bits, j, tables, p)
            f = os.path.join(td, f"mlp{j}.b")
            with open(f, "wb") as fout:
                fout.write(streams[j])
            sym, = coders.decode_group([(p, f)])
            B.fold(sym, prefix, desc, bits, j)
    q = torch.empty(lay["n"], dtype=torch.int16, device=device)
    B.unpack(prefix, desc, bits, _device_vector(np.frombuffer(low, dtype=np.uint8).copy(), device), q)
    coders.check()
    coders.shutdown()
    q = q.cpu().numpy().view(np.uint16).astype(np.uint32)
    out, at = {}, 0
    for name, shape, n, _, _, _ in tensors:
        out[name] = q[at:at + n].reshape(shape)
        at += n
    return out


@torch.no_grad()
def decode_mlp(payload: bytes, info: Dict, device) -> Dict[str, torch.Tensor]:
    """Inverse of encode_mlp: {name: dequantised float32 tensor on `device`}, computed from the indices exactly as
    read_container computes the packed sections' (on the host, then moved), so the two are bit-equal."""
    q = decode_indices(payload, info, device)
    out = {}
    for e in info["tensors"]:
        v = torch.from_numpy(q[e["name"]].reshape(-1).astype(np.float32))
        out[e["name"]] = (v * e["interval"] + e["lo"]).view(*e["shape"]).to(device)
    return out
