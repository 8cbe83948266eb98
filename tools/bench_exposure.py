#!/usr/bin/env python3
"""Per-camera exposure compensation (cnc_amd/csrc/exposure.hip): the op at the training step's ray count next
to the torch chain, the full-size training step with the option off and on, and a from-scratch run on a procedural capture
whose training frames carry known gains.

    python tools/bench_exposure.py [--reps 20] [--rays 37000] [--cameras 100] [--json out.jsonl]
                                   [--step synthetic|capture] [--recover STEPS] [--no-kernels] [--package-root DIR]

Kernels (milliseconds per call: median, min and max of --reps windows of 10 calls, device events, after 3 warm-up calls):
the gain table; the forward and the backward through their mirrors, for both composite forms; forward + backward through
`ExposureCompensation` and autograd, as a training step runs them; and the same in torch ops — index the table, multiply,
composite, and for the gradient autograd's `index_add_`.

--step synthetic: the full-size training step (bench.py's configuration) on the built-in scene, without any option: 240
warm-up steps, then five blocks of 20 steps, ms per step of each block.  With --package-root pointing at a checkout of
another commit (its library built) the same loop times that commit in the same session.
--step capture: the same loop on a procedural capture (the ball, --cameras views of 200 x 200 through `TransformsLoader`),
with the option off and on.

--recover STEPS: two from-scratch runs of STEPS steps on that capture from one seed, option off and on.  The training
frames' RGB is scaled to 0.7 and multiplied by exp(e*_k), e* fixed, centred per channel, max |e*| = 0.3; the held-out
frames are scaled to 0.7 only.  Reports the test PSNR, the container's size and mean |e - e*| against mean |e*|.  One
synthetic scene, an untuned rate (--lr)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch


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
    return {"ms": times[len(times) // 2], "min": times[0], "max": times[-1]}


def kernels(a, dev):
    from cnc_amd.backends import exposure_backend as K
    from cnc_amd.exposure import ExposureCompensation
    g = torch.Generator(device=dev).manual_seed(0)
    n, C, out = a.rays, a.cameras, []
    rgb = torch.rand(n, 3, device=dev, generator=g).requires_grad_(True)
    op = torch.rand(n, device=dev, generator=g).requires_grad_(True)
    bkgd = torch.rand(3, device=dev, generator=g)
    ids = torch.randint(0, C, (n,), device=dev, generator=g)
    g_out = torch.randn(n, 3, device=dev, generator=g)
    ex = ExposureCompensation(C, dev)
    with torch.no_grad():
        ex.log_gain.copy_(torch.rand(C, 3, device=dev, generator=g) * 0.6 - 0.3)
    gains = ex.gains()

    def row(name, fn, **kw):
        r = dict({"kernel": name, "n_rays": n, "n_cameras": C}, **timed(fn, a.reps), **kw)
        out.append(r)
        print(json.dumps(r), flush=True)

    row("gain table", lambda: K.exposure_gains(ex.log_gain.detach()))
    for form, whole in (("whole pixel", True), ("foreground only", False)):
        def both():
            ex.log_gain.grad = rgb.grad = op.grad = None
            ex(rgb, ids, op, bkgd, gain_background=whole).backward(g_out)

        def chain():
            ex.log_gain.grad = rgb.grad = op.grad = None
            K.exposure_torch(ex.log_gain, rgb, ids, op, bkgd, whole).backward(g_out)
        row("forward", lambda: K.exposure_forward(rgb.detach(), ids, gains, op.detach(), bkgd, whole), form=form)
        row("backward", lambda: K.exposure_backward(g_out, rgb.detach(), ids, gains, op.detach(), bkgd, whole), form=form)
        row("forward + backward, autograd", both, form=form)
        row("torch chain forward", lambda: K.exposure_torch(ex.log_gain.detach(), rgb.detach(), ids, op.detach(), bkgd, whole),
            form=form)
        row("torch chain forward + backward, autograd", chain, form=form)
    return out


def true_log_gains(C):
    e = np.random.default_rng(4).uniform(-1.0, 1.0, (C, 3))
    e -= e.mean(axis=0)
    return e * (0.3 / np.abs(e).max())


def write_capture(root, scene, n_views, size, dev, gains=False):
    """The procedural ball's views as PNGs + transforms.json (camera_angle_x, OpenGL poses, the default box), every 8th
    held out by the loader.  `gains`: RGB scaled to 0.7 everywhere and times exp(e*_k) on the training frames -> e*."""
    from PIL import Image
    from cnc_amd.datasets import SyntheticBallDataset
    ball = SyntheticBallDataset(size, n_train_views=n_views, device=dev, seed=0)
    images = ball._train_images().clone()
    training = [i for i in range(n_views) if i % 8 != 0]
    e_true = true_log_gains(len(training))
    if gains:
        images[..., :3] *= 0.7
        images[training, :, :, :3] *= torch.exp(torch.from_numpy(e_true).to(dev).float())[:, None, None, :]
        assert float(images[..., :3].max()) < 254.5 / 255.0
    images = (images * 255).round().to(torch.uint8).cpu().numpy()
    os.makedirs(os.path.join(root, scene, "images"), exist_ok=True)
    frames = []
    for i, (img, pose) in enumerate(zip(images, ball.train_c2w.cpu().numpy())):
        Image.fromarray(img, "RGBA").save(os.path.join(root, scene, "images", f"{i:04d}.png"))
        m = np.concatenate([pose, [[0.0, 0.0, 0.0, 1.0]]]).astype(np.float64)
        frames.append({"file_path": f"images/{i:04d}", "transform_matrix": m.tolist()})
    doc = {"camera_angle_x": 0.6911, "w": size, "h": size, "aabb": [-1.5] * 3 + [1.5] * 3, "frames": frames}
    with open(os.path.join(root, scene, "transforms.json"), "w") as fp:
        json.dump(doc, fp)
    return e_true


def capture_trainer(root, scene, dev, **kw):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    from cnc_amd.trainer import TrainConfig, Trainer
    train = TransformsLoader(scene, root, "train", num_rays=1024, color_bkgd_aug="random", device=dev)
    test = TransformsLoader(scene, root, "test", device=dev)
    train.seed_sampling(11)
    data = LoaderDataset(train, test)
    data._gen = torch.Generator().manual_seed(5)
    cfg = TrainConfig(n_features=8, sample_num=150000, image_size=200, out_dir=os.path.join(root, "bits_" + scene), **kw)
    return Trainer(cfg, device=dev, dataset=data)


def step_blocks(tr, label, extra):
    for step in range(240):
        tr.train_step(step, want_stats=False)
    torch.cuda.synchronize()
    blocks, step = [], 240
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(20):
            tr.train_step(step, want_stats=False)
            step += 1
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t) / 20 * 1e3)
    s = tr.train_step(step)
    r = dict({"trainer_step": label, "package": os.path.dirname(sys.modules["cnc_amd"].__file__),
              "ms_per_step_blocks": blocks, "ms_per_step": sorted(blocks)[2], "stats": s}, **extra)
    print(json.dumps(r), flush=True)
    return r


def trainer_steps(a, dev):
    from cnc_amd.trainer import TrainConfig, Trainer
    out = []
    if a.step == "synthetic":
        cfg = TrainConfig(n_features=8, sample_num=150000, image_size=400, out_dir="/tmp/cnc_bench_bits")
        out.append(step_blocks(Trainer(cfg, device=dev), "synthetic, no option", {}))
        return out
    with tempfile.TemporaryDirectory() as root:
        write_capture(root, "ball", a.cameras, 200, dev)
        for lr in (0.0, a.lr):
            tr = capture_trainer(root, "ball", dev, **({"exposure_lr": lr} if lr > 0 else {}))
            extra = {"exposure_lr": lr}
            out.append(step_blocks(tr, "capture", extra))
            if tr.exposure is not None:
                out[-1]["mean_abs_log_gain"] = tr.exposure.mean_magnitude()
            del tr
            torch.cuda.empty_cache()
    return out


def recover(a, dev):
    out = []
    with tempfile.TemporaryDirectory() as root:
        e_true = write_capture(root, "gained", a.cameras, 200, dev, gains=True)
        for lr in (0.0, a.lr):
            torch.manual_seed(1234)
            tr = capture_trainer(root, "gained", dev, max_steps=a.recover, **({"exposure_lr": lr} if lr > 0 else {}))
            for step in range(a.recover):
                tr.train_step(step, want_stats=False)
            torch.cuda.synchronize()
            psnr = tr.evaluate(len(tr.dataset.test))
            path = os.path.join(root, f"scene_{lr}.cnc")
            tr.save_container(path)
            r = {"recover": True, "steps": a.recover, "exposure_lr": lr, "test_views": len(tr.dataset.test),
                 "test_psnr": psnr, "container_bytes": os.path.getsize(path), "mean_abs_true": float(np.abs(e_true).mean())}
            if tr.exposure is not None:
                e = tr.exposure.effective().double().cpu().numpy()
                r["mean_abs_error"] = float(np.abs(e - e_true).mean())
                r["max_abs_error"] = float(np.abs(e - e_true).max())
            out.append(r)
            print(json.dumps(r), flush=True)
            del tr
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=37000)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--lr", type=float, default=5e-3, help="the gains' learning rate where the option is on (untuned)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=["synthetic", "capture"], default=None)
    ap.add_argument("--recover", type=int, default=0, metavar="STEPS")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    ap.add_argument("--package-root", dest="package_root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    dev = torch.device("cuda:0")
    out = []
    if a.step:               # first: a Trainer made before other streams exist gets a hardware queue per stream
        out += trainer_steps(a, dev)
    if a.recover:
        out += recover(a, dev)
    if a.kernels:
        out += kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    rows = [r for r in out if "kernel" in r]
    if rows:
        print("| call | form | ms: median (min .. max) |")
        print("|---|---|---|")
        for r in rows:
            print(f"| {r['kernel']} | {r.get('form', '')} | {r['ms']:.4f} ({r['min']:.4f} .. {r['max']:.4f}) |")
    for r in out:
        if r.get("trainer_step"):
            print(f"trainer step, {r['trainer_step']}, exposure_lr={r.get('exposure_lr', 0.0)}: "
                  + ", ".join(f"{b:.3f}" for b in r["ms_per_step_blocks"]) + " ms per step (blocks of 20)")


if __name__ == "__main__":
    main()
