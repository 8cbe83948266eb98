#!/usr/bin/env python3
"""Error-map pixel sampling (cnc_amd/csrc/error_map.hip): the kernels at the training step's ray count next to
the torch calls they replace, the full-size training step with the option off and on, and one convergence experiment.

    python tools/bench_error_map.py [--reps 20] [--rays 37000] [--cameras 100] [--json out.jsonl]
                                    [--step synthetic|capture] [--converge STEPS] [--no-kernels] [--package-root DIR]

Kernels (milliseconds per call: median, min and max of --reps windows of 10 calls, device events, after 3 warm-up calls,
through the Python mirrors — allocation of the outputs included): the draw (one `torch.rand` and the sampler's launch) next
to the three `randint` calls; the weighted loss forward, and forward + backward through autograd, next to `F.mse_loss`;
the cell keys, the stable sort + segment bounds, the update kernel behind them, and the CDF.

--step synthetic: the full-size training step (bench.py's configuration) on the built-in scene, without any option: 240
warm-up steps, then five blocks of 20 steps, ms per step of each block.  With --package-root pointing at a checkout of
another commit (its library built) the same loop times that commit in the same session.
--step capture: the same loop on a procedural capture (the ball, --cameras views of 200 x 200 through `TransformsLoader`),
with the option off and on.

--converge STEPS: two from-scratch runs of STEPS steps from one seed, option off and on, on a capture whose object fills a
small part of each frame: the ball through a wide lens (camera_angle_x = 1.2: about 7 % of the pixels), opaque frames
over a smooth sky, the learned environment-map background.  Reports the test PSNR, the container's size and errmap_cover
over time.  One synthetic scene; the floor, the decay and the refresh interval are the untuned defaults."""
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
    import torch.nn.functional as F
    from cnc_amd.backends import errmap_backend as K
    from cnc_amd.error_map import ErrorMapSampler, weighted_mse
    g = torch.Generator(device=dev).manual_seed(0)
    n, C, H, W, G, out = a.rays, a.cameras, 200, 200, a.resolution, []
    sm = ErrorMapSampler(C, H, W, resolution=G, device=dev)
    sm.map.copy_(torch.rand(C, G, G, device=dev, generator=g) ** 3)
    sm.refresh()
    ids, px, py, w = sm.draw(n, g)
    rgb = torch.rand(n, 3, device=dev, generator=g).requires_grad_(True)
    pix = torch.rand(n, 3, device=dev, generator=g)
    err = torch.rand(n, device=dev, generator=g)
    keys = K.keys(ids, px, py, C, H, W, G)
    sorted_keys, order = torch.sort(keys, stable=True)
    bounds = torch.arange(C * G * G + 1, dtype=torch.int32, device=dev)
    offsets = torch.searchsorted(sorted_keys, bounds).contiguous()
    from cnc_amd import _lib

    def row(name, fn, **kw):
        r = dict({"kernel": name, "n_rays": n, "n_cameras": C, "resolution": G}, **timed(fn, a.reps), **kw)
        out.append(r)
        print(json.dumps(r), flush=True)

    def three_randint():
        torch.randint(0, C, (n,), device=dev, generator=g)
        torch.randint(0, W, (n,), device=dev, generator=g)
        torch.randint(0, H, (n,), device=dev, generator=g)

    def loss_both():
        rgb.grad = None
        (weighted_mse(rgb, pix, w)[0] * 1024.0).backward()

    def mse_both():
        rgb.grad = None
        (F.mse_loss(rgb, pix) * 1024.0).backward()

    def update_kernel():
        _lib.check(_lib.lib().cnc_errmap_update(order.data_ptr(), offsets.data_ptr(), err.data_ptr(), n, C, G, 0.9,
                                                sm.map.data_ptr(), _lib.stream(dev)), "update")

    def sort_and_bounds():
        sk, _ = torch.sort(keys, stable=True)
        torch.searchsorted(sk, bounds)
    row("draw: torch.rand [n, 3] + cnc_errmap_sample", lambda: sm.draw(n, g))
    row("replaced: three torch.randint", three_randint)
    row("cnc_errmap_loss_forward (two launches)", lambda: K.loss_forward(rgb.detach(), pix, w))
    row("weighted loss forward + backward, autograd", loss_both)
    row("replaced: F.mse_loss forward", lambda: F.mse_loss(rgb.detach(), pix))
    row("replaced: F.mse_loss forward + backward, autograd", mse_both)
    row("cnc_errmap_keys", lambda: K.keys(ids, px, py, C, H, W, G))
    row("torch.sort (stable) + searchsorted", sort_and_bounds)
    row("cnc_errmap_update (the kernel alone)", update_kernel)
    row("observe: keys + sort + bounds + update", lambda: sm.observe(ids, px, py, err))
    row("cnc_errmap_cdf (one block; every refresh_every-th step)", sm.refresh)
    return out


def write_capture(root, scene, n_views, size, dev, wide=False):
    """The procedural ball's views as PNGs + transforms.json (OpenGL poses, the default box), every 8th held out by the
    loader.  `wide`: camera_angle_x = 1.2 instead of 0.6911 and opaque RGB frames, the ball over a smooth sky."""
    from PIL import Image
    from cnc_amd.datasets import SyntheticBallDataset
    ball = SyntheticBallDataset(size, n_train_views=n_views, device=dev, seed=0)
    angle = 1.2 if wide else 0.6911
    ball.focal = 0.5 * size / math.tan(0.5 * angle)
    if wide:
        ys, xs = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
        x, y = xs.reshape(-1).float(), ys.reshape(-1).float()
        views = []
        for c2w in ball.train_c2w:
            o, d = ball._rays(c2w[None].expand(x.shape[0], 3, 4), x, y)
            rgb, alpha = ball._shade(o, d)
            sky = torch.stack([0.35 + 0.25 * d[:, 2], torch.full_like(d[:, 2], 0.5), 0.65 - 0.25 * d[:, 2]], dim=-1)
            views.append((rgb * alpha + sky * (1 - alpha)).view(size, size, 3))
        images, mode = torch.stack(views), "RGB"
        cover = float(torch.stack([ball._shade(*ball._rays(c[None].expand(x.shape[0], 3, 4), x, y))[1].mean()
                                   for c in ball.train_c2w[:4]]).mean())
    else:
        images, mode, cover = ball._train_images().clone(), "RGBA", None
    images = (images * 255).round().to(torch.uint8).cpu().numpy()
    os.makedirs(os.path.join(root, scene, "images"), exist_ok=True)
    frames = []
    for i, (img, pose) in enumerate(zip(images, ball.train_c2w.cpu().numpy())):
        Image.fromarray(img, mode).save(os.path.join(root, scene, "images", f"{i:04d}.png"))
        m = np.concatenate([pose, [[0.0, 0.0, 0.0, 1.0]]]).astype(np.float64)
        frames.append({"file_path": f"images/{i:04d}", "transform_matrix": m.tolist()})
    doc = {"camera_angle_x": angle, "w": size, "h": size, "aabb": [-1.5] * 3 + [1.5] * 3, "frames": frames}
    with open(os.path.join(root, scene, "transforms.json"), "w") as fp:
        json.dump(doc, fp)
    return cover


def capture_trainer(root, scene, dev, sub="", **kw):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    from cnc_amd.trainer import TrainConfig, Trainer
    train = TransformsLoader(scene, root, "train", num_rays=1024, color_bkgd_aug="random", device=dev)
    test = TransformsLoader(scene, root, "test", device=dev)
    train.seed_sampling(11)
    data = LoaderDataset(train, test)
    data._gen = torch.Generator().manual_seed(5)
    cfg = TrainConfig(n_features=8, sample_num=150000, image_size=200, out_dir=os.path.join(root, "bits_" + scene + sub), **kw)
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
    if getattr(tr, "error_map", None) is not None:
        extra = dict(extra, errmap_cover=tr.error_map.effective_fraction())
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
        for on in (False, True):
            tr = capture_trainer(root, "ball", dev, **({"error_map": True, "error_map_resolution": a.resolution} if on else {}))
            out.append(step_blocks(tr, "capture", {"error_map": on}))
            del tr
            torch.cuda.empty_cache()
    return out


def converge(a, dev):
    out = []
    with tempfile.TemporaryDirectory() as root:
        cover = write_capture(root, "far", a.cameras, 200, dev, wide=True)
        for on in (False, True):
            torch.manual_seed(1234)
            kw = {"error_map": True, "error_map_resolution": a.resolution} if on else {}
            tr = capture_trainer(root, "far", dev, sub=str(int(on)), max_steps=a.converge, background="envmap", **kw)
            covers = []
            for step in range(a.converge):
                tr.train_step(step, want_stats=False)
                if on and (step + 1) % max(a.converge // 8, 1) == 0:
                    covers.append((step + 1, round(tr.error_map.effective_fraction(), 4)))
            torch.cuda.synchronize()
            psnr = tr.evaluate(len(tr.dataset.test))
            path = os.path.join(root, f"scene_{int(on)}.cnc")
            tr.save_container(path)
            r = {"converge": True, "steps": a.converge, "error_map": on, "resolution": a.resolution,
                 "object_share_of_pixels": cover, "test_views": len(tr.dataset.test), "test_psnr": psnr,
                 "container_bytes": os.path.getsize(path), "errmap_cover": covers}
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
    ap.add_argument("--resolution", type=int, default=16, help="G of the map (the untuned default)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", choices=["synthetic", "capture"], default=None)
    ap.add_argument("--converge", type=int, default=0, metavar="STEPS")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    ap.add_argument("--package-root", dest="package_root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    dev = torch.device("cuda:0")
    out = []
    if a.step:               # first: a Trainer made before other streams exist gets a hardware queue per stream
        out += trainer_steps(a, dev)
    if a.converge:
        out += converge(a, dev)
    if a.kernels:
        out += kernels(a, dev)
    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    rows = [r for r in out if "kernel" in r]
    if rows:
        print("| call | ms: median (min .. max) |")
        print("|---|---|")
        for r in rows:
            print(f"| {r['kernel']} | {r['ms']:.4f} ({r['min']:.4f} .. {r['max']:.4f}) |")
    for r in out:
        if r.get("trainer_step"):
            print(f"trainer step, {r['trainer_step']}, error_map={r.get('error_map', False)}: "
                  + ", ".join(f"{b:.3f}" for b in r["ms_per_step_blocks"]) + " ms per step (blocks of 20)")


if __name__ == "__main__":
    main()
