"""Host range coder against the device entropy coder on ONE trained full-size state (F = 8, 12 x 3-D levels at T = 2^19 +
3 x 4 plane levels at T = 2^17, the procedural scene after a few hundred steps): encode / decode wall time, the size
of the .b files and of the container, and where the host path's time goes.  Results: profiles/device_coder.md.

    python tools/bench_device_coder.py --steps 300 --state /tmp/coder_state.pt --out device_coder.json
    rocprofv3 --kernel-trace --stats -d prof -- python tools/bench_device_coder.py --state /tmp/coder_state.pt --kernels-only 16384

The first form trains, saves the state and measures every row from it; the second loads the saved state and runs one
device encode + decode, for a kernel trace of its own.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from cnc_amd import _lib, coders
from cnc_amd._codec import lib as codec_lib
from cnc_amd.trainer import TrainConfig, Trainer

LANE_SIZES = (1 << 12, 1 << 14, 1 << 16)


def make_trainer(device_coder=False, S=None):
    cfg = TrainConfig(n_features=8, sample_num=150000, max_steps=20000, image_size=200, out_dir=tempfile.mkdtemp(prefix="cnc_coder_"),
                      device_coder=device_coder, symbols_per_lane=S)
    return Trainer(cfg, device=torch.device("cuda:0"))


def save_state(tr, path):
    torch.save({"field": tr.field.state_dict(), "context": tr.context.state_dict(), "binaries": tr.estimator.binaries}, path)


def load_state(tr, path):
    blob = torch.load(path, map_location=tr.device)
    tr.field.load_state_dict(blob["field"])
    tr.context.load_state_dict(blob["context"])
    tr.estimator.binaries = blob["binaries"].to(tr.device)


def tables(tr):
    e = tr.field.mlp_base
    return [t.params.data for t in (e.encoding_xyz, e.encoding_xy, e.encoding_xz, e.encoding_yz)]


class KernelTimer:
    """Device time of the coder's C calls, from events around them."""

    def __init__(self):
        self.L = _lib.lib()
        self.spans = {"cnc_rans_encode_pm1": [], "cnc_rans_decode_pm1": []}
        self.real = {n: getattr(self.L, n) for n in self.spans}
        for n in self.spans:
            setattr(self.L, n, self._wrap(n))

    def _wrap(self, name):
        def call(*a):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = self.real[name](*a)
            t1.record()
            self.spans[name].append((t0, t1))
            return rc
        return call

    def take(self):
        torch.cuda.synchronize()
        out = {n: sum(a.elapsed_time(b) for a, b in v) for n, v in self.spans.items()}
        for v in self.spans.values():
            v.clear()
        return out


def round_trip(tr, coder, S, reps, timer, want):
    """Median wall time of encode and decode (+ the coder calls' device time), sizes, and the decoded tables checked."""
    tr.cfg.device_coder, tr.cfg.symbols_per_lane = coder == "device", S
    enc, dec, k_enc, k_dec = [], [], [], []
    for rep in range(reps + 1):           # the first round warms caches and allocators up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Pgs, est_MB, coded_MB, prefix = tr.encode()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        spans = timer.take()
        k_enc.append(spans["cnc_rans_encode_pm1"])
        keep = [t.clone() for t in tables(tr)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tr.decode_into_field(Pgs, prefix)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        k_dec.append(timer.take()["cnc_rans_decode_pm1"])
        for got, q in zip(tables(tr), want):
            coded = ~(got == 1).all(dim=1)
            assert torch.equal(got[coded], q[coded]), "decode differs from what was encoded"
        tr.field.update_embedding_params(*keep)      # the next round codes the trained tables again
        enc.append(t1 - t0)
        dec.append(t3 - t2)
    d = os.path.dirname(prefix)
    files = [f for f in os.listdir(d) if f.endswith(".b")]
    lanes = 0
    if coder == "device":
        lanes = sum(int.from_bytes(open(os.path.join(d, f), "rb").read(6)[2:6], "little") for f in files)
    with tempfile.TemporaryDirectory() as td:
        info = tr.save_container(os.path.join(td, "scene.cnc"))
        container = os.path.getsize(os.path.join(td, "scene.cnc"))
    return {"coder": coder, "S": S, "encode_s": statistics.median(enc[1:]), "decode_s": statistics.median(dec[1:]),
            "encode_all_s": enc, "decode_all_s": dec, "coder_encode_ms": statistics.median(k_enc[1:]),
            "coder_decode_ms": statistics.median(k_dec[1:]), "b_files": len(files),
            "b_bytes": sum(os.path.getsize(os.path.join(d, f)) for f in files), "estimate_bytes": est_MB * 1024 * 1024,
            "container_bytes": container, "lanes": lanes}


class _Collect:
    """Stands in for CoderPool: keeps the streams, codes nothing — what is left of `encode` is the probability kernels."""
    streams = []

    def __init__(self, *a, **k):
        pass

    def encode(self, x, p, file_name):
        _Collect.streams.append((x.detach().reshape(-1), p.detach().reshape(-1)))

        class Done:
            def result(self):
                return 0
        return Done()

    def finish(self):
        return 0

    def shutdown(self):
        pass


def host_split(tr, reps):
    """The host path's parts, each alone: the probability kernels; the device -> host copies; the range coder."""
    tr.cfg.device_coder = False
    real = coders.CoderPool          # the name `coders.make_coder` looks up
    coders.CoderPool = _Collect
    prob = []
    try:
        for _ in range(reps + 1):
            _Collect.streams = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.encode()
            torch.cuda.synchronize()
            prob.append(time.perf_counter() - t0)
    finally:
        coders.CoderPool = real
    streams = _Collect.streams
    n_sym = sum(x.numel() for x, _ in streams)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [(x.to(torch.float32).cpu().contiguous(), p.to(torch.float32).cpu().contiguous()) for x, p in streams]
    copies = time.perf_counter() - t0
    L = codec_lib()
    per_stream = []
    for x, p in host:
        n = x.numel()
        buf = np.empty(int(L.cnc_rc_bound(n)), np.uint8)
        t0 = time.perf_counter()
        L.cnc_rc_encode_pm1(p.data_ptr(), x.data_ptr(), n, buf.ctypes.data, buf.size)
        per_stream.append(time.perf_counter() - t0)
    return {"probabilities_s": statistics.median(prob[1:]), "copies_pageable_s": copies, "symbols": n_sym, "streams": len(streams),
            "range_coder_one_thread_s": sum(per_stream), "range_coder_longest_stream_s": max(per_stream),
            "largest_stream_symbols": max(x.numel() for x, _ in streams)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--state", default=os.path.join(tempfile.gettempdir(), "cnc_coder_state.pt"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", type=int, default=None, metavar="S",
                    help="load --state, one device encode + decode at S symbols per lane, nothing else")
    args = ap.parse_args()
    tr = make_trainer()
    if args.kernels_only:
        load_state(tr, args.state)
        tr.cfg.device_coder, tr.cfg.symbols_per_lane = True, args.kernels_only
        for _ in range(2):
            keep = [t.clone() for t in tables(tr)]
            Pgs, _, coded_MB, prefix = tr.encode()
            tr.decode_into_field(Pgs, prefix)
            tr.field.update_embedding_params(*keep)
        torch.cuda.synchronize()
        print(f"kernels-only: S = {args.kernels_only}, coded {coded_MB * 1024:.1f} KB")
        return
    for step in range(args.steps):
        tr.train_step(step)
    torch.cuda.synchronize()
    save_state(tr, args.state)
    want = [torch.where(t >= 0, 1.0, -1.0) for t in tables(tr)]
    timer = KernelTimer()
    rows = [round_trip(tr, "host", None, args.reps, timer, want)]
    for S in LANE_SIZES:
        rows.append(round_trip(tr, "device", S, args.reps, timer, want))
    split = host_split(tr, args.reps)
    host = rows[0]
    for r in rows:
        r["container_vs_host"] = r["container_bytes"] / host["container_bytes"]
        if r["lanes"]:
            r["bits_per_lane_over_host"] = 8.0 * (r["b_bytes"] - host["b_bytes"]) / r["lanes"]
            r["ns_per_symbol_encode"] = 1e6 * r["coder_encode_ms"] / r["S"]
            r["ns_per_symbol_decode"] = 1e6 * r["coder_decode_ms"] / r["S"]
    ok = [r["S"] for r in rows[1:] if r["container_vs_host"] <= 1.01]
    result = {"steps": args.steps, "rows": rows, "host_split": split, "default_S": min(ok) if ok else LANE_SIZES[-1],
              "none_qualified": not ok}
    print(f"{'coder':8} {'S':>6} {'encode s':>9} {'decode s':>9} {'.b bytes':>10} {'container':>10} {'vs host':>8} {'lanes':>6} "
          f"{'enc ms':>7} {'dec ms':>7}")
    for r in rows:
        print(f"{r['coder']:8} {str(r['S'] or '-'):>6} {r['encode_s']:9.3f} {r['decode_s']:9.3f} {r['b_bytes']:10d} "
              f"{r['container_bytes']:10d} {r['container_vs_host']:8.4f} {r['lanes']:6d} {r['coder_encode_ms']:7.2f} "
              f"{r['coder_decode_ms']:7.2f}")
    print("host path alone:", json.dumps(split))
    print("default S:", result["default_S"], "(none within 1 %)" if result["none_qualified"] else "")
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
