#!/usr/bin/env python3
"""Pose refinement: what its kernels cost, and what the option costs a training step.

    python tools/bench_pose_refine.py [--reps 20] [--json out.jsonl] [--trainer] [--no-kernels] [--cameras 100]

Kernels: milliseconds per call (median, min .. max of --reps timed windows of 10 calls each, device events) at 2^18
samples on the full-size model (12 3-D levels at T = 2^19 + 3 x 4 plane levels at T = 2^17, F = 8, H = 160):
cnc_field_position_grad (on random dX / dS and positions uniform in the box), the library GEMM that makes dS from G1, and
cnc_ray_pose_grad / cnc_camera_pose_apply at the step's ~37 k rays and --cameras cameras.

--trainer: the full-size training step (bench.py's configuration) on a capture this tool writes — the procedural ball,
--cameras views of 200 x 200 pixels as PNGs + transforms.json, read back through `TransformsLoader` — with
`pose_lr` = 0 and 1e-4: 240 warm-up steps, then three blocks of 20 steps, ms per step of each block.  The Trainer runs are
made first: a Trainer made before other streams exist gets a hardware queue per stream."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FULL = dict(n_features_per_level=8, n_neurons=160, resolutions_list=(18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514),
            log2_hashmap_size=19, resolutions_list_2D=(130, 258, 514, 1026), log2_hashmap_size_2D=17)


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


def kernels(a, dev):
    from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
    from cnc_amd.poses import pose_apply, ray_pose_grad
    out = []
    g = torch.Generator(device=dev).manual_seed(0)
    f = NGPRadianceField_mygrid_2D3D(aabb=[-1.5] * 3 + [1.5] * 3, **FULL).to(dev)
    with torch.no_grad():
        for e in f.mlp_base._encoders():
            e.params.uniform_(-1, 1)
    ff = FusedFieldForward(f)
    N = 1 << 18
    x = torch.rand(N, 3, device=dev, generator=g) * 2.98 - 1.49
    d = torch.nn.functional.normalize(torch.randn(N, 3, device=dev, generator=g), dim=-1)
    ff.save_forward(x, d, N)                                             # builds the unit table and the bit planes
    n_enc = sum(e.n_output_dims for e in f.mlp_base._encoders())
    ld = f.mlp_base._layout()[0]
    dX = torch.randn(N, ld, device=dev, generator=g)
    G1 = torch.randn(N, 160, device=dev, generator=g)
    W1 = f.mlp_base.network[0].weight.detach()
    sel = torch.ones(N, dtype=torch.uint8, device=dev)
    dS = G1 @ W1[:, n_enc:n_enc + 63]

    def row(name, fn, nbytes=None):
        ms, lo, hi = timed(fn, a.reps)
        r = {"kernel": name, "ms": ms, "min": lo, "max": hi}
        if nbytes:
            r["GBps"] = nbytes / (ms * 1e-3) / 1e9
        out.append(r)
        print(json.dumps(r), flush=True)

    # algorithmic bytes: positions 12 + selector 1 + dX n_enc * 4 + dS 63 * 4 + g_x 12 per sample (the sign gathers hit L2)
    row(f"cnc_field_position_grad, 2^18 samples, {n_enc} encoder columns", lambda: ff.position_grad(x, sel, dX, dS),
        N * (12 + 1 + n_enc * 4 + 63 * 4 + 12))
    row("dS = G1 @ W1[:, sinusoid columns] (library GEMM)", lambda: G1 @ W1[:, n_enc:n_enc + 63])
    n_rays, C = 37449, a.cameras
    cnts = torch.randint(0, 15, (n_rays,), device=dev, generator=g)
    starts = torch.cumsum(cnts, 0) - cnts
    M = int(cnts.sum())
    t0 = torch.rand(M, device=dev, generator=g) * 4 + 2
    g_x = torch.randn(M, 3, device=dev, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(n_rays, 3, device=dev, generator=g), dim=-1)
    ids = torch.randint(0, C, (n_rays,), device=dev, generator=g)
    G = torch.empty(C, 6, device=dev)
    row(f"cnc_ray_pose_grad, {M} samples, {n_rays} rays, {C} cameras",
        lambda: ray_pose_grad(g_x, t0, t0 + 5e-3, starts, cnts, dirs, ids, C, out=G), M * 20 + n_rays * (16 + 12 + 8 + 48))
    base = torch.randn(C, 24, device=dev, generator=g)
    delta = torch.randn(C, 6, device=dev, generator=g) * 0.01
    table = torch.empty_like(base)
    row(f"cnc_camera_pose_apply, {C} cameras", lambda: pose_apply(base, delta, out=table))
    return out


def write_capture(root, scene, n_views, size, dev):
    """The procedural ball's training views as PNGs + transforms.json (camera_angle_x, OpenGL poses, the default box)."""
    from PIL import Image
    from cnc_amd.datasets import SyntheticBallDataset
    ball = SyntheticBallDataset(size, n_train_views=n_views, device=dev, seed=0)
    images = (ball._train_images() * 255).round().to(torch.uint8).cpu().numpy()
    os.makedirs(os.path.join(root, scene, "images"), exist_ok=True)
    frames = []
    for i, (img, pose) in enumerate(zip(images, ball.train_c2w.cpu().numpy())):
        Image.fromarray(img, "RGBA").save(os.path.join(root, scene, "images", f"{i:04d}.png"))
        m = np.concatenate([pose, [[0.0, 0.0, 0.0, 1.0]]]).astype(np.float64)
        frames.append({"file_path": f"images/{i:04d}", "transform_matrix": m.tolist()})
    doc = {"camera_angle_x": 0.6911, "w": size, "h": size, "aabb": [-1.5] * 3 + [1.5] * 3, "frames": frames}
    with open(os.path.join(root, scene, "transforms.json"), "w") as fp:
        json.dump(doc, fp)


def trainer_steps(a, dev):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    from cnc_amd.trainer import TrainConfig, Trainer
    out = []
    with tempfile.TemporaryDirectory() as root:
        write_capture(root, "ball", a.cameras, 200, dev)
        for lr in (0.0, 1e-4):
            train = TransformsLoader("ball", root, "train", num_rays=1024, color_bkgd_aug="random", device=dev)
            test = TransformsLoader("ball", root, "test", device=dev)
            kw = {"pose_lr": lr} if lr > 0 else {}
            tr = Trainer(TrainConfig(n_features=8, sample_num=150000, image_size=200, out_dir=os.path.join(root, "bits"), **kw),
                         device=dev, dataset=LoaderDataset(train, test))
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
            r = {"trainer_step": True, "pose_lr": lr, "ms_per_step_blocks": blocks, "ms_per_step": sorted(blocks)[1], "stats": s}
            if tr.pose_refiner is not None:
                r["mean_tau"], r["mean_omega"] = tr.pose_refiner.mean_magnitudes()
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
    ap.add_argument("--cameras", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = []
    if a.trainer:
        out += trainer_steps(a, dev)
    if a.kernels:
        out += kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    rows = [r for r in out if "kernel" in r]
    if rows:
        print("| kernel | ms (min .. max) | GB/s |")
        print("|---|---|---|")
        for r in rows:
            print(f"| {r['kernel']} | {r['ms']:.4f} ({r['min']:.4f} .. {r['max']:.4f}) | "
                  + (f"{r['GBps']:.0f}" if "GBps" in r else "") + " |")
    for r in out:
        if r.get("trainer_step"):
            print(f"trainer step, pose_lr={r['pose_lr']}: " + ", ".join(f"{b:.3f}" for b in r["ms_per_step_blocks"])
                  + " ms per step (blocks of 20)")


if __name__ == "__main__":
    main()
