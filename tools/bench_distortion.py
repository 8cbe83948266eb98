#!/usr/bin/env python3
"""The distortion-loss kernels (cnc_amd/csrc/distortion.hip) against the plain-torch chain a user would assemble from this
package's own `exclusive_sum` / `accumulate_along_rays`, on the same GPU in the same session.

    python tools/bench_distortion.py [--reps 20] [--json out.jsonl] [--large] [--trainer] [--weights 0,0.01]

Forward + backward of sum(per-ray loss), milliseconds per call (median of --reps timed windows of 10 calls each, device
events), at 2^18 packed samples over ~37 k rays (the training step's shape: ~7 samples per ray) and at batched
(4096, 256).  The chain is the textbook prefix form w_i (2 (m_i W_<i - M_<i) + w_i d_i / 3): two exclusive sums, the
element-wise ops, one index_add_ and autograd's replay of them.  `max_rel_diff` compares the per-ray losses of the two
(the chain's own cancellation shows there).  `fwd kernel` / `bwd kernel`: the two mirrors alone, no autograd around them.

--trainer: the full-size training step (bench.py's configuration) with each of --weights as
`TrainConfig.distortion_weight`: 240 warm-up steps, then three blocks of 20 steps, ms per step of each block."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def torch_chain(w, t0, t1, ray_indices, n_rays, packed_info):
    """Per-ray loss from this package's scans and per-ray sums: the prefix form."""
    from cnc_amd.nerfacc.scan import exclusive_sum
    from cnc_amd.nerfacc.volrend import accumulate_along_rays
    m = (t0 + t1) * 0.5
    inner = m * exclusive_sum(w, packed_info) - exclusive_sum(w * m, packed_info)
    per_sample = w * (2.0 * inner + w * (t1 - t0) / 3.0)
    if ray_indices is None:
        return per_sample.sum(-1)
    return accumulate_along_rays(per_sample, None, ray_indices, n_rays).squeeze(-1)


def sorted_intervals(shape, dev, g):
    edges = torch.sort(torch.rand(*shape[:-1], shape[-1] + 1, device=dev, generator=g) * 6.0, -1).values
    return edges[..., :-1].contiguous(), edges[..., 1:].contiguous()


def kernels(a, dev):
    from cnc_amd.backends import volrend_backend as K
    from cnc_amd.nerfacc.losses import distortion
    g = torch.Generator(device=dev).manual_seed(0)
    out = []

    def run(name, w, t0, t1, ray_indices, n_rays, info, n_samples):
        w = w.requires_grad_(True)

        def both(fn):
            def call():
                w.grad = None
                fn().sum().backward()
            return call
        hip = both(lambda: distortion(w, t0, t1, ray_indices=ray_indices, n_rays=n_rays, packed_info=info))
        ref = both(lambda: torch_chain(w, t0, t1, ray_indices, n_rays, info))
        with torch.no_grad():
            lh = distortion(w, t0, t1, ray_indices=ray_indices, n_rays=n_rays, packed_info=info).double()
            lt = torch_chain(w, t0, t1, ray_indices, n_rays, info).double()
        hip(); gh = w.grad.clone()
        ref(); gt = w.grad.clone()
        r = {"shape": name, "n_rays": n_rays, "n_samples": n_samples,
             "max_rel_diff_loss": ((lh - lt).abs() / lh.abs().clamp_min(1e-30)).max().item(),
             "max_abs_diff_grad": (gh - gt).abs().max().item()}
        r["hip_ms"], r["hip_min"], r["hip_max"] = timed(hip, a.reps)
        r["torch_ms"], r["torch_min"], r["torch_max"] = timed(ref, a.reps)
        r["speedup"] = r["torch_ms"] / r["hip_ms"]
        # the two kernels alone, through their mirrors (one allocation + one launch each; no autograd around them)
        sc = K.split_packed(info) if info is not None else (None, None)
        wd, gl = w.detach(), torch.ones(lh.shape, device=dev)
        r["fwd_kernel_ms"], _, _ = timed(lambda: K.distortion_forward(sc[0], sc[1], t0, t1, wd), a.reps)
        r["bwd_kernel_ms"], _, _ = timed(lambda: K.distortion_backward(sc[0], sc[1], t0, t1, wd, gl), a.reps)
        # fwd reads w, t0, t1 (+ the layout); bwd reads them again and writes g_w
        r["bytes"] = n_samples * 4 * 7 + n_rays * (16 * 2 + 8)
        r["kernels_GBps"] = r["bytes"] / ((r["fwd_kernel_ms"] + r["bwd_kernel_ms"]) * 1e-3) / 1e9
        out.append(r)
        print(json.dumps(r), flush=True)

    def packed(n_rays):
        cnts = torch.randint(0, 15, (n_rays,), device=dev, generator=g)          # 7 on average: 2^18 samples within 0.5 %
        starts = torch.cumsum(cnts, 0) - cnts
        info = torch.stack([starts, cnts], -1)
        ri = torch.repeat_interleave(torch.arange(n_rays, device=dev), cnts)
        N = int(cnts.sum())
        t0 = torch.rand(N, device=dev, generator=g) * 5e-3 + (torch.arange(N, device=dev) - starts[ri]) * 5e-3 + 2.0
        run(f"packed, {N} samples", torch.rand(N, device=dev, generator=g) * 0.2, t0, t0 + 5e-3, ri, n_rays, info, N)

    def batched(R, S):
        b0, b1 = sorted_intervals((R, S), dev, g)
        run(f"batched ({R}, {S})", torch.rand(R, S, device=dev, generator=g) * 0.05, b0, b1, None, R, None, R * S)

    packed(37449)            # the training step's shape: 2^18 samples, ~7 per ray
    batched(4096, 256)       # proposal-sampled rows
    if a.large:              # 16x either: where the launches no longer hide the kernels
        packed(16 * 37449)
        batched(65536, 256)
    return out


def trainer_steps(a, dev):
    from cnc_amd.trainer import TrainConfig, Trainer
    out = []
    for weight in [float(x) for x in a.weights.split(",")]:
        kw = {"distortion_weight": weight} if weight > 0 else {}
        tr = Trainer(TrainConfig(n_features=8, sample_num=150000, image_size=400, out_dir="/tmp/cnc_bench_bits", **kw), device=dev)
        for step in range(240):
            tr.train_step(step, want_stats=False)
        torch.cuda.synchronize()
        blocks, step = [], 240
        for _ in range(3):
            t = time.perf_counter()
            for _ in range(20):
                tr.train_step(step, want_stats=False)
                step += 1
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t) / 20 * 1e3)
        s = tr.train_step(step)
        r = {"trainer_step": True, "distortion_weight": weight, "ms_per_step_blocks": blocks,
             "ms_per_step": sorted(blocks)[1], "stats": s}
        out.append(r)
        print(json.dumps(r), flush=True)
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    ap.add_argument("--weights", default="0,0.01")
    ap.add_argument("--large", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    if a.trainer:            # first: a Trainer made before other streams exist gets a hardware queue per stream
        out += trainer_steps(a, dev)
    if a.kernels:
        out += kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    rows = [r for r in out if "shape" in r]
    if rows:
        print("| shape | rays | samples | HIP ms (min .. max) | torch chain ms (min .. max) | speedup | fwd kernel ms | "
              "bwd kernel ms | kernels GB/s |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            print(f"| {r['shape']} | {r['n_rays']} | {r['n_samples']} | {r['hip_ms']:.4f} ({r['hip_min']:.4f} .. "
                  f"{r['hip_max']:.4f}) | {r['torch_ms']:.4f} ({r['torch_min']:.4f} .. {r['torch_max']:.4f}) | "
                  f"{r['speedup']:.1f}x | {r['fwd_kernel_ms']:.4f} | {r['bwd_kernel_ms']:.4f} | {r['kernels_GBps']:.0f} |")
    for r in out:
        if r.get("trainer_step"):
            print(f"trainer step, distortion_weight={r['distortion_weight']}: "
                  + ", ".join(f"{b:.3f}" for b in r["ms_per_step_blocks"]) + " ms per step (blocks of 20)")


if __name__ == "__main__":
    main()
