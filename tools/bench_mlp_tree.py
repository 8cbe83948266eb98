"""The container's MLP, packed against the "tree1" section, on trained full-size states (F = 8, 12 x 3-D
levels at T = 2^19 + 3 x 4 plane levels at T = 2^17, the procedural scene): per tensor the chosen depth and the model's
bits per weight, the section and the whole file either way and for both coders, and the wall time of writing and reading
the MLP against the packed path's (`quantize_tensor` + `_pack_bits`, `_unpack_bits` + dequantisation: the parent
commit's code, untouched).  Results: profiles/mlp_tree.md.

    python tools/bench_mlp_tree.py --steps 300 --out mlp_tree_300.json                       # the protocol of profiles/device_coder.md
    python tools/bench_mlp_tree.py --steps 5000 --procedural --out mlp_tree_5000.json        # one 5000-step procedural run
    python tools/bench_mlp_tree.py --laplace --out mlp_tree_laplace.json                     # the size test's tensor: coded / ideal
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cnc_amd import mlp_codec as mc
from cnc_amd.container import _pack_bits, _unpack_bits, quantize_tensor, section_sizes
from cnc_amd.trainer import TrainConfig, Trainer


def make_trainer(steps, procedural):
    kw = dict(n_features=8, sample_num=150000, max_steps=20000, image_size=200, out_dir=tempfile.mkdtemp(prefix="cnc_mlp_tree_"))
    if procedural:       # python -m cnc_amd.train --dataset procedural --image_size 400 --n_features 8 --sample_num 150000 --max_steps N
        f = steps / 20000.0
        kw.update(max_steps=steps, image_size=400, milestones=tuple(int(m * f) for m in (9000, 12000, 15000, 17000, 19000)),
                  warmup_iters=max(1, int(1000 * f)))
    return Trainer(TrainConfig(**kw), device=torch.device("cuda:0"))


def timed(fn, reps):
    """Median wall time of fn() after one warm-up call, a device synchronisation on either side."""
    out, times = None, []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, statistics.median(times[1:]), times


def packed_write(state, bits=13):
    return {k: (_pack_bits(q, bits), lo, iv, tuple(p.shape)) for k, p in state.items()
            for q, lo, iv in [quantize_tensor(p.detach().float(), bits)]}


def packed_read(blobs, dev, bits=13):
    out = {}
    for k, (b, lo, iv, shape) in blobs.items():
        q = _unpack_bits(b, int(np.prod(shape)), bits).astype(np.float32)
        out[k] = (torch.from_numpy(q) * iv + lo).view(*shape).to(dev)
    return out


def measure_state(tr, reps):
    state = tr._mlp_state()
    dev = tr.device
    blobs, t_pw, all_pw = timed(lambda: packed_write(state), reps)
    ref, t_pr, all_pr = timed(lambda: packed_read(blobs, dev), reps)
    packed_bytes = sum(len(b[0]) for b in blobs.values())
    res = {"weights": sum(int(p.numel()) for p in state.values()), "packed_section_bytes": packed_bytes,
           "packed_write_s": t_pw, "packed_read_s": t_pr, "packed_write_all_s": all_pw, "packed_read_all_s": all_pr, "coders": {}}
    for coder in ("host", "device"):
        (payload, info), t_enc, all_enc = timed(lambda: mc.encode_mlp(state, coder=coder), reps)
        got, t_dec, all_dec = timed(lambda: mc.decode_mlp(payload, info, dev), reps)
        assert all(torch.equal(got[k], ref[k]) for k in ref), "tree1 decode differs from the packed path"
        tr.cfg.device_coder = coder == "device"
        files = {}
        with tempfile.TemporaryDirectory() as td:
            for name in ("packed", "tree"):
                tr.cfg.mlp_coder = name
                tr.save_container(os.path.join(td, name + ".cnc"))
                sizes = section_sizes(os.path.join(td, name + ".cnc"))
                files[name] = {"file_bytes": os.path.getsize(os.path.join(td, name + ".cnc")),
                               "mlp_bytes": sum(v for k, v in sizes.items() if k == "mlp" or k.startswith("mlp/")),
                               "tree_section": "mlp" in sizes}
        tr.cfg.mlp_coder = "packed"
        res["coders"][coder] = {"section_bytes": len(payload), "stream_sizes": info["stream_sizes"], "encode_s": t_enc, "decode_s": t_dec,
                                "encode_all_s": all_enc, "decode_all_s": all_dec, "files": files}
    # per tensor, from the indices the section holds: the depth, the model's cost and a zero-order entropy for scale
    tensors = []
    for e in info["tensors"]:
        q = quantize_tensor(state[e["name"]].detach().float(), 13)[0].reshape(-1).astype(np.int64)
        hist = np.bincount(q >> 5, minlength=256)
        costs = mc.depth_costs(hist, q.size, 13)
        assert mc.choose_depth(hist, q.size, 13) == e["depth"]
        tensors.append({"name": e["name"], "shape": e["shape"], "depth": e["depth"], "bits_per_weight": costs[e["depth"]] / q.size,
                        "bits_per_weight_by_depth": [c / q.size for c in costs]})
    res["tensors"] = tensors
    return res


def measure_laplace():
    """The tensor of tests/test_gpu_mlp_tree.py::test_size_against_the_ideal: section bytes over the ideal bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mlp_tree_twin as twin
    dev = torch.device("cuda:0")
    w = torch.from_numpy(np.random.default_rng(7).laplace(size=(160, 255)).astype(np.float32)).to(dev)
    m = twin.model([quantize_tensor(w, 13)[0].reshape(-1).astype(np.int64)], 13)
    out = {"ideal_bytes": m["ideal_bytes"], "packed_bytes": (w.numel() * 13 + 7) // 8, "depth": m["depths"][0],
           "plane_symbols": [pl["n"] for pl in m["planes"]], "plane_ideal_bytes": [pl["ideal_bits"] / 8 for pl in m["planes"]]}
    for coder in ("host", "device"):
        payload, info = mc.encode_mlp({"w": w}, coder=coder)
        out[coder] = {"section_bytes": len(payload), "stream_sizes": info["stream_sizes"], "excess": len(payload) / m["ideal_bytes"] - 1.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--procedural", action="store_true", help="the schedule of a --max_steps STEPS procedural run at image size 400")
    ap.add_argument("--laplace", action="store_true", help="only the size test's synthetic tensor")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.laplace:
        result = {"laplace": measure_laplace()}
    else:
        tr = make_trainer(args.steps, args.procedural)
        t0 = time.perf_counter()
        for step in range(args.steps):
            tr.train_step(step)
        torch.cuda.synchronize()
        result = {"steps": args.steps, "procedural": args.procedural, "train_s": time.perf_counter() - t0}
        result.update(measure_state(tr, args.reps))
    print(json.dumps(result, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
