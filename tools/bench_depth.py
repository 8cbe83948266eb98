#!/usr/bin/env python3
"""Depth supervision (cnc_amd/csrc/depth_loss.hip) against the plain-torch chains a user would assemble from this package's
own ops, on the same GPU in the same session.

    python tools/bench_depth.py [--reps 20] [--json out.jsonl] [--trainer] [--no-kernels] [--weights 0,1]

Kernels: `cnc_depth_loss_forward`, the backward, and forward + backward of sum(per-ray loss) through autograd, milliseconds
per call (median of --reps timed windows of 10 calls each, device events), at 2^18 packed samples over ~37 k rays (the
training step's shape).  The chain is the same loss — e per sample, two `accumulate_along_rays`, the validity mask — with
autograd replaying it.  Fetch: `cnc_depth_fetch` at 37 k rays against `depth_fetch_torch` on the device.

--trainer: the full-size training step (bench.py's configuration) with each of --weights as `TrainConfig.depth_weight`: 240
warm-up steps, then three blocks of 20 steps, ms per step of each block.  Weight 0 builds the configuration without naming
the option, so the same command runs on a commit from before it."""
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


def torch_chain(w, t0, t1, target, ray_indices, n_rays, spread):
    """Per-ray loss from element-wise ops and this package's per-ray sums."""
    from cnc_amd.nerfacc.volrend import accumulate_along_rays
    valid = torch.isfinite(target) & (target > 0)
    D = torch.where(valid, target, torch.ones_like(target))[ray_indices]
    e = 0.5 * ((t0 - D) + (t1 - D))
    a = w * e
    s1 = accumulate_along_rays(a, None, ray_indices, n_rays).squeeze(-1)
    s2 = accumulate_along_rays(a * e, None, ray_indices, n_rays).squeeze(-1)
    return torch.where(valid, s1 * s1 + spread * s2, torch.zeros_like(s1))


def kernels(a, dev):
    from cnc_amd.backends import camera_backend as CB
    from cnc_amd.backends import volrend_backend as K
    from cnc_amd.nerfacc.losses import depth_loss
    g = torch.Generator(device=dev).manual_seed(0)
    n_rays = 37449
    cnts = torch.randint(0, 15, (n_rays,), device=dev, generator=g)          # 7 on average: 2^18 samples within 0.5 %
    starts = torch.cumsum(cnts, 0) - cnts
    info = torch.stack([starts, cnts], -1)
    ri = torch.repeat_interleave(torch.arange(n_rays, device=dev), cnts)
    N = int(cnts.sum())
    t0 = torch.rand(N, device=dev, generator=g) * 5e-3 + (torch.arange(N, device=dev) - starts[ri]) * 5e-3 + 2.0
    t1 = t0 + 5e-3
    w = (torch.rand(N, device=dev, generator=g) * 0.2).requires_grad_(True)
    target = 2.0 + torch.rand(n_rays, device=dev, generator=g) * 0.07
    target[::5] = 0.0                                                        # a fifth of the rays without a measurement

    def both(fn):
        def call():
            w.grad = None
            fn().sum().backward()
        return call
    hip = both(lambda: depth_loss(w, t0, t1, target, ray_indices=ri, n_rays=n_rays, packed_info=info, spread=1.0))
    ref = both(lambda: torch_chain(w, t0, t1, target, ri, n_rays, 1.0))
    with torch.no_grad():
        lh = depth_loss(w, t0, t1, target, packed_info=info, spread=1.0).double()
        lt = torch_chain(w, t0, t1, target, ri, n_rays, 1.0).double()
    hip(); gh = w.grad.clone()
    ref(); gt = w.grad.clone()
    r = {"kernel": "depth_loss", "n_rays": n_rays, "n_samples": N,
         "max_abs_diff_loss": (lh - lt).abs().max().item(), "max_abs_diff_grad": (gh - gt).abs().max().item()}
    r["hip_ms"], r["hip_min"], r["hip_max"] = timed(hip, a.reps)
    r["torch_ms"], r["torch_min"], r["torch_max"] = timed(ref, a.reps)
    r["speedup"] = r["torch_ms"] / r["hip_ms"]
    wd, gl = w.detach(), torch.ones(n_rays, device=dev)
    _, s1 = K.depth_loss_forward(starts, cnts, t0, t1, wd, target, 1.0)
    r["fwd_kernel_ms"], r["fwd_min"], r["fwd_max"] = timed(lambda: K.depth_loss_forward(starts, cnts, t0, t1, wd, target, 1.0), a.reps)
    r["bwd_kernel_ms"], r["bwd_min"], r["bwd_max"] = timed(
        lambda: K.depth_loss_backward(starts, cnts, t0, t1, wd, target, 1.0, s1, gl), a.reps)
    print(json.dumps(r), flush=True)
    # the fetch: 100 cameras of 200 x 200, z-depth
    n_cams, H, W = 100, 200, 200
    planes = torch.rand(n_cams, H, W, device=dev, generator=g) * 4.0 + 1.0
    cams = torch.zeros(n_cams, 24, device=dev)
    cams[:, :4] = torch.tensor([280.0, 280.0, 100.0, 100.0], device=dev)
    cams[:, 4], cams[:, 9], cams[:, 14] = 1.0, 1.0, 1.0
    ids = torch.randint(0, n_cams, (n_rays,), device=dev, generator=g)
    px = torch.randint(0, W, (n_rays,), device=dev, generator=g)
    py = torch.randint(0, H, (n_rays,), device=dev, generator=g)
    _, dirs, _ = CB.camera_rays(cams, 0, False, ids, px, py)
    f = {"kernel": "depth_fetch", "n_rays": n_rays,
         "max_abs_diff": (CB.depth_fetch(planes, cams, False, False, ids, px, py, dirs)
                          - CB.depth_fetch_torch(planes, cams, False, False, ids, px, py, dirs)).abs().max().item()}
    f["hip_ms"], f["hip_min"], f["hip_max"] = timed(lambda: CB.depth_fetch(planes, cams, False, False, ids, px, py, dirs), a.reps)
    f["torch_ms"], f["torch_min"], f["torch_max"] = timed(
        lambda: CB.depth_fetch_torch(planes, cams, False, False, ids, px, py, dirs), a.reps)
    f["speedup"] = f["torch_ms"] / f["hip_ms"]
    print(json.dumps(f), flush=True)
    return [r, f]


def trainer_steps(a, dev):
    from cnc_amd.trainer import TrainConfig, Trainer
    out = []
    for weight in [float(x) for x in a.weights.split(",")]:
        kw = {"depth_weight": weight} if weight > 0 else {}
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
        r = {"trainer_step": True, "depth_weight": weight, "ms_per_step_blocks": blocks,
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
    ap.add_argument("--weights", default="0,1")
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
    for r in out:
        if r.get("trainer_step"):
            print(f"trainer step, depth_weight={r['depth_weight']}: "
                  + ", ".join(f"{b:.3f}" for b in r["ms_per_step_blocks"]) + " ms per step (blocks of 20)")


if __name__ == "__main__":
    main()
