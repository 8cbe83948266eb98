"""The container's occupancy section, iid against the "pyramid1" model, on ONE trained full-size state (the model of
tools/bench_device_coder.py: the procedural scene after a few hundred steps).  Section and container bytes with both
coders, and the wall time of the occupancy part of a write and of a read.  Results: profiles/occ_pyramid.md.

    python tools/bench_occ_pyramid.py --steps 300 --reps 5 --out occ_pyramid.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cnc_amd import occupancy_codec as oc
from cnc_amd.container import read_container, section_sizes, write_container
from bench_device_coder import make_trainer


def timed(fn, reps):
    fn()                                         # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tr = make_trainer()
    for step in range(args.steps):
        tr.train_step(step)
    grid = tr.estimator.binaries
    dev = grid.device
    td = tempfile.mkdtemp(prefix="cnc_occ_")
    res = {"steps": args.steps, "shape": list(grid.shape), "occupied": float(grid.float().mean())}

    # the iid section alone: write_container / read_container with nothing else in the file
    f = os.path.join(td, "iid.cnc")
    only = dict(meta={}, table_streams={}, field_mlp={}, context_state={})
    t_enc, _ = timed(lambda: write_container(f, binaries=grid, **only), args.reps)
    t_dec, back = timed(lambda: read_container(f, device=dev)[2], args.reps)
    assert torch.equal(back, grid)
    res["iid"] = {"bytes": section_sizes(f)["occupancy"], "encode_s": t_enc, "decode_s": t_dec}
    for coder in ("host", "device"):
        t_enc, (payload, info) = timed(lambda: oc.encode_occupancy(grid, coder=coder), args.reps)
        t_dec, back = timed(lambda: oc.decode_occupancy(payload, info, dev), args.reps)
        assert torch.equal(back, grid)
        res["pyramid_" + coder] = {"bytes": len(payload), "encode_s": t_enc, "decode_s": t_dec, "n": info["n"],
                                   "stream_sizes": info["stream_sizes"]}
    # the whole container, all four combinations
    for dc in (False, True):
        tr.cfg.device_coder = dc
        for occ in ("iid", "pyramid"):
            tr.cfg.occupancy_coder = occ
            info = tr.save_container(os.path.join(td, "all.cnc"))
            sizes = section_sizes(os.path.join(td, "all.cnc"))
            res[f"container_{'device' if dc else 'host'}_{occ}"] = {
                "file_bytes": int(round(info["file_KB"] * 1024)), "occupancy_bytes": sizes["occupancy"],
                "tables_bytes": sum(v for k, v in sizes.items() if k.startswith("table/")),
                "mlp_bytes": sum(v for k, v in sizes.items() if k.startswith("mlp/")),
                "ctx_bytes": sum(v for k, v in sizes.items() if k.startswith("ctx/"))}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)


if __name__ == "__main__":
    main()
