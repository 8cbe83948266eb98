"""Single-file bitstream container.

The reference leaves its result scattered: one `.b` file per level/chunk (utils_bpp_acc.py:722,752,
793,854), the 24 level frequencies `Pgs_dict` only in memory (:710), the occupancy grid and the
13-bit MLP only *estimated* (train_CNC_nerf_synthetic.py:53-68,508-556) and the context models not
stored at all.  This module writes everything a decoder needs into ONE file, so "size (KB)" is a
real file size:

    magic "CNC1" | u32 header_len | header JSON | payload sections (offsets in the header)

sections: every arithmetic-coded table stream, the occupancy grid (arithmetic-coded with its own
frequency, or — `occupancy_coder="pyramid"`, the section then says `model: "pyramid1"` — context-coded
from a pyramid of itself, occupancy_codec.py), the radiance-field MLP tensors uniformly quantised to
`mlp_bits` (13) bits and bit-packed (`mlp/<name>` sections) or — `mlp_coder="tree"`, one `mlp` section that says
`model: "tree1"` — the same indices entropy-coded with a per-tensor bit-tree model (mlp_codec.py) whenever that is smaller,
the context-model weights in fp32, and — only when a run learned one — the environment-map background's texture as raw
uint8 (`envmap`).
"""
from __future__ import annotations

import io
import json
import os
import struct
import tempfile
from typing import Dict

import numpy as np
import torch

from .context import decoder, encoder

MAGIC = b"CNC1"


def _pack_bits(values: np.ndarray, bits: int) -> bytes:
    """values: uint32 < 2^bits -> little-endian bit stream."""
    v = values.astype(np.uint64).reshape(-1)
    out = np.zeros((v.size * bits + 7) // 8 + 8, dtype=np.uint8)
    pos = np.arange(v.size, dtype=np.uint64) * np.uint64(bits)
    for b in range(bits):                       # bit-plane at a time (vectorised)
        bit = ((v >> np.uint64(b)) & np.uint64(1)).astype(np.uint8)
        p = pos + np.uint64(b)
        np.bitwise_or.at(out, (p >> np.uint64(3)).astype(np.int64), bit << (p & np.uint64(7)).astype(np.uint8))
    return out[: (v.size * bits + 7) // 8].tobytes()


def _unpack_bits(buf: bytes, n: int, bits: int) -> np.ndarray:
    raw = np.frombuffer(buf, dtype=np.uint8)
    allbits = np.unpackbits(raw, bitorder="little")[: n * bits].reshape(n, bits).astype(np.uint32)
    return (allbits << np.arange(bits, dtype=np.uint32)).sum(axis=1).astype(np.uint32)


def quantize_tensor(p: torch.Tensor, bits: int):
    """(p - min) // interval, interval = (max - min) / (2^bits - 1) + 1e-6
    (quantize_params, train_CNC_nerf_synthetic.py:30-50)."""
    lo, hi = float(p.min()), float(p.max())
    interval = (hi - lo) / (2 ** bits - 1) + 1e-6
    q = torch.div(p - lo, interval, rounding_mode="floor").clamp_(0, 2 ** bits - 1)
    return q.to(torch.int64).cpu().numpy().astype(np.uint32), lo, interval


def write_container(path: str, *, meta: Dict, table_streams: Dict[str, bytes], binaries: torch.Tensor,
                    field_mlp: Dict[str, torch.Tensor], context_state: Dict[str, torch.Tensor],
                    mlp_bits: int = 13, occupancy_coder: str = "iid", coder: str = "host", symbols_per_lane=None,
                    mlp_coder: str = "packed", envmap=None) -> int:
    """Returns the file size in bytes.  envmap: None, or the learned background's uint8 [H, 2H, 3] texture
    (`EnvMapBackground.quantized()`), written raw as the last section, `envmap`; without it the file is what it was.  occupancy_coder: "iid" (one Bernoulli frequency, the host range coder) or
    "pyramid" (occupancy_codec.encode_occupancy with `coder`, "host" or "device": the coder of the table streams).
    mlp_coder: "packed" (the `mlp/<name>` sections) or "tree" (mlp_codec.encode_mlp with `coder`; the packed sections
    still, byte for byte, when the tree1 section would not be smaller than their sum)."""
    if occupancy_coder not in ("iid", "pyramid"):
        raise ValueError(f"occupancy_coder must be 'iid' or 'pyramid', got {occupancy_coder!r}")
    if mlp_coder not in ("packed", "tree"):
        raise ValueError(f"mlp_coder must be 'packed' or 'tree', got {mlp_coder!r}")
    if mlp_coder == "tree":
        from .mlp_codec import check_bits
        check_bits(mlp_bits)
    sections, payload = {}, io.BytesIO()

    def add(name, blob, **extra):
        sections[name] = dict(offset=payload.tell(), size=len(blob), **extra)
        payload.write(blob)

    for name, blob in table_streams.items():
        add("table/" + name, blob)
    if occupancy_coder == "pyramid":
        from .occupancy_codec import levels_of
        try:
            levels_of(binaries.shape)
        except ValueError:
            occupancy_coder = "iid"      # a grid with an odd side has no pyramid: it keeps the Bernoulli section
    if occupancy_coder == "pyramid":
        from .occupancy_codec import encode_occupancy
        blob, info = encode_occupancy(binaries, coder=coder, symbols_per_lane=symbols_per_lane)
        info.pop("c1")                   # the payload holds the tables; the header does not repeat them
        add("occupancy", blob, **info)
    else:
        # occupancy grid: Bernoulli(Pg) arithmetic code, what get_binary_vxl_size only estimates
        occ = binaries.reshape(-1).to(torch.float32).cpu()
        pg = float(occ.mean().clamp(1e-6, 1 - 1e-6))
        with tempfile.TemporaryDirectory() as td:
            f = os.path.join(td, "occ.b")
            encoder(occ * 2 - 1, torch.full_like(occ, pg), f)
            add("occupancy", open(f, "rb").read(), shape=list(binaries.shape), pg=pg)
    tree = None
    if mlp_coder == "tree" and field_mlp:
        from .mlp_codec import encode_mlp
        blob, info = encode_mlp(field_mlp, bits=mlp_bits, coder=coder, symbols_per_lane=symbols_per_lane)
        packed = sum((int(p.numel()) * mlp_bits + 7) // 8 for p in field_mlp.values())
        if len(blob) < packed:           # never larger: a section that saves nothing leaves the packed ones in place
            tree = (blob, info)
    if tree is not None:
        add("mlp", tree[0], **tree[1])
    else:
        for name, p in field_mlp.items():
            q, lo, interval = quantize_tensor(p.detach().float(), mlp_bits)
            add("mlp/" + name, _pack_bits(q, mlp_bits), shape=list(p.shape), lo=lo, interval=interval, bits=mlp_bits)
    for name, p in context_state.items():
        add("ctx/" + name, p.detach().float().cpu().numpy().tobytes(), shape=list(p.shape))
    if envmap is not None:
        u8 = torch.as_tensor(envmap).detach().cpu()
        if u8.dtype != torch.uint8 or u8.dim() != 3 or u8.shape[2] != 3 or u8.shape[1] != 2 * u8.shape[0]:
            raise ValueError(f"envmap must be uint8 [H, 2H, 3], got {u8.dtype} {list(u8.shape)}")
        add("envmap", u8.contiguous().numpy().tobytes(), shape=list(u8.shape))
    header = json.dumps(dict(meta=meta, sections=sections)).encode()
    with open(path, "wb") as fo:
        fo.write(MAGIC)
        fo.write(struct.pack("<I", len(header)))
        fo.write(header)
        fo.write(payload.getvalue())
    return os.path.getsize(path)


def section_sizes(path: str) -> Dict[str, int]:
    """Bytes of every section of a container, from its header alone."""
    with open(path, "rb") as fi:
        assert fi.read(4) == MAGIC, "not a CNC1 container"
        (hlen,) = struct.unpack("<I", fi.read(4))
        return {name: int(s["size"]) for name, s in json.loads(fi.read(hlen))["sections"].items()}


def read_envmap(path: str):
    """The `envmap` section of a container as uint8 [H, 2H, 3] (on the host), or None when it has none."""
    with open(path, "rb") as fi:
        assert fi.read(4) == MAGIC, "not a CNC1 container"
        (hlen,) = struct.unpack("<I", fi.read(4))
        s = json.loads(fi.read(hlen))["sections"].get("envmap")
        if s is None:
            return None
        fi.seek(int(s["offset"]), os.SEEK_CUR)
        data = fi.read(int(s["size"]))
    shape = [int(v) for v in s["shape"]]
    if len(shape) != 3 or shape[2] != 3 or shape[1] != 2 * shape[0] or len(data) != int(np.prod(shape)):
        raise RuntimeError(f"{path}: malformed envmap section (shape {shape}, {len(data)} bytes)")
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).view(*shape)


def read_container(path: str, device="cpu"):
    """Returns (meta, table_streams, binaries, field_mlp (dequantised), context_state).  A learned background, when the file
    has one, is read by `read_envmap`: section names this function does not know are ignored."""
    with open(path, "rb") as fi:
        assert fi.read(4) == MAGIC, "not a CNC1 container"
        (hlen,) = struct.unpack("<I", fi.read(4))
        header = json.loads(fi.read(hlen))
        blob = fi.read()
    sec = header["sections"]

    def get(name):
        s = sec[name]
        return blob[s["offset"]: s["offset"] + s["size"]], s

    tables, mlp, ctx = {}, {}, {}
    binaries = None
    for name in sec:
        data, s = get(name)
        if name.startswith("table/"):
            tables[name[6:]] = data
        elif name == "occupancy" and "model" in s:
            from .occupancy_codec import decode_occupancy
            binaries = decode_occupancy(data, s, device)      # raises for a model it does not know and for device="cpu"
        elif name == "occupancy":
            n = int(np.prod(s["shape"]))
            with tempfile.TemporaryDirectory() as td:
                f = os.path.join(td, "occ.b")
                open(f, "wb").write(data)
                x = decoder(torch.full((n,), s["pg"], dtype=torch.float32), f)
            binaries = (x > 0).view(*s["shape"]).to(device)
        elif name == "mlp":
            from .mlp_codec import decode_mlp
            mlp.update(decode_mlp(data, s, device))            # raises for a model it does not know and for device="cpu"
        elif name.startswith("mlp/"):
            n = int(np.prod(s["shape"]))
            q = _unpack_bits(data, n, s["bits"]).astype(np.float32)
            mlp[name[4:]] = (torch.from_numpy(q) * s["interval"] + s["lo"]).view(*s["shape"]).to(device)
        elif name.startswith("ctx/"):
            arr = np.frombuffer(data, dtype=np.float32).copy()
            ctx[name[4:]] = torch.from_numpy(arr).view(*s["shape"]).to(device)
    return header["meta"], tables, binaries, mlp, ctx
