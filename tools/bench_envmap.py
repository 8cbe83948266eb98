#!/usr/bin/env python3
"""The environment-map background (cnc_amd/csrc/envmap.hip): its launches at the training step's ray count and
the full-size training step with the option on and off.

    python tools/bench_envmap.py [--reps 20] [--rays 37000] [--json out.jsonl] [--trainer] [--backgrounds solid,envmap]
                                 [--scene default|sky] [--no-kernels] [--package-root DIR]

Kernels (per H in 16, 64; milliseconds per call, median of --reps windows of 10 calls, device events): the composite
forward through its mirror; the ray side of the backward; the stable sort + searchsorted that group the 4 N contributions
(torch); the grouped sum; forward + backward through `EnvMapBackground` and autograd, as a training step runs them.

--trainer: the full-size training step (bench.py's configuration) per entry of --backgrounds: 240 warm-up steps, then three
blocks of 20 steps, ms per step of each block.  `solid` passes no option at all, so with --package-root pointing at a
checkout of another commit (its library built) the same loop times that commit in the same session.  --scene sky: the
procedural ball in front of sky(d) = 1/2 + 1/2 d instead of a per-batch random colour behind transparent pixels — an OPAQUE
scene, what the option is meant for (on the default scene the map cannot explain a colour that changes every batch, the
field fills the box with density instead and the ray count collapses: a caution, not a measurement of the option)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

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
    return times[len(times) // 2]


def kernels(a, dev):
    from cnc_amd.backends import envmap_backend as K
    from cnc_amd.envmap import EnvMapBackground
    g = torch.Generator(device=dev).manual_seed(0)
    n, out = a.rays, []
    d = torch.randn(n, 3, device=dev, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    rgb = torch.rand(n, 3, device=dev, generator=g).requires_grad_(True)
    op = torch.rand(n, device=dev, generator=g).requires_grad_(True)
    g_out = torch.randn(n, 3, device=dev, generator=g)
    for H in (16, 64):
        env = EnvMapBackground(H, device=dev)
        with torch.no_grad():
            env.texture.copy_(torch.rand(H, 2 * H, 3, device=dev, generator=g))
        T = env.texture.detach()
        _, cell, frac = K.envmap_forward(d, T, rgb.detach(), op.detach())
        _, s, keys = K.envmap_backward_rays(g_out, op.detach(), cell, frac, T)

        def group():
            sk, order = torch.sort(keys.view(-1), stable=True)
            return order, torch.searchsorted(sk, torch.arange(2 * H * H + 1, dtype=torch.int32, device=dev))
        order, offsets = group()
        gT = torch.empty_like(T)
        L, ptr, stream = K._lib.lib(), K.ptr, K.stream

        def both():
            env.texture.grad = rgb.grad = op.grad = None
            env(rgb, op, d).backward(g_out)
        r = {"H": H, "n_rays": n, "section_bytes": H * 2 * H * 3,
             "forward_ms": timed(lambda: K.envmap_forward(d, T, rgb.detach(), op.detach()), a.reps),
             "lookup_ms": timed(lambda: K.envmap_forward(d, T, want_coords=False), a.reps),
             "backward_rays_ms": timed(lambda: K.envmap_backward_rays(g_out, op.detach(), cell, frac, T), a.reps),
             "group_sort_ms": timed(group, a.reps),
             "backward_texture_kernel_ms": timed(lambda: L.cnc_envmap_backward_texture(
                 ptr(order), ptr(offsets), ptr(frac), ptr(s), H, n, ptr(gT), stream(dev)), a.reps),
             "backward_texture_ms": timed(lambda: K.envmap_backward_texture(keys, frac, s, H), a.reps),
             "forward_backward_autograd_ms": timed(both, a.reps)}
        r["backward_ms"] = r["backward_rays_ms"] + r["backward_texture_ms"]
        # the longest segment a texel gets from this batch (the grouped sum's critical path: ceil(len / 64) rounds)
        r["longest_segment"] = int((offsets[1:] - offsets[:-1])[:-1].max()) if 2 * H * H > 1 else 0
        out.append(r)
        print(json.dumps(r), flush=True)
    return out


def sky_ball(image_size, dev, seed):
    from cnc_amd.datasets import SyntheticBallDataset
    from cnc_amd.render import Rays

    class BallUnderASky(SyntheticBallDataset):
        has_alpha = False        # every pixel is opaque: the sky stands where the parent class blends a colour

        def fetch(self, num_rays=None):
            n = self.num_rays if num_rays is None else num_rays
            img = torch.randint(0, self.train_c2w.shape[0], (n,), device=self.device, generator=self.gen)
            xi = torch.randint(0, self.W, (n,), device=self.device, generator=self.gen)
            yi = torch.randint(0, self.H, (n,), device=self.device, generator=self.gen)
            o, d = self._rays(self.train_c2w[img], xi.float(), yi.float())
            rgba = self._train_images()[img, yi, xi]
            return {"rays": Rays(o, d), "pixels": rgba[:, :3] * rgba[:, 3:] + (0.5 + 0.5 * d) * (1 - rgba[:, 3:]),
                    "color_bkgd": torch.ones(3, device=self.device)}

    return BallUnderASky(image_size, device=dev, seed=seed)


def trainer_steps(a, dev):
    from cnc_amd.trainer import TrainConfig, Trainer
    out = []
    for background in a.backgrounds.split(","):
        kw = {"background": background} if background != "solid" else {}
        cfg = TrainConfig(n_features=8, sample_num=150000, image_size=400, out_dir="/tmp/cnc_bench_bits", **kw)
        tr = Trainer(cfg, device=dev, dataset=sky_ball(cfg.image_size, dev, cfg.seed) if a.scene == "sky" else None)
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
        r = {"trainer_step": True, "background": background, "scene": a.scene, "package": os.path.dirname(sys.modules["cnc_amd"].__file__),
             "ms_per_step_blocks": blocks, "ms_per_step": sorted(blocks)[1], "stats": s}
        out.append(r)
        print(json.dumps(r), flush=True)
        del tr
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rays", type=int, default=37000)
    ap.add_argument("--json", default=None)
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--no-kernels", dest="kernels", action="store_false")
    ap.add_argument("--backgrounds", default="solid,envmap")
    ap.add_argument("--scene", choices=["default", "sky"], default="default")
    ap.add_argument("--package-root", dest="package_root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
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


if __name__ == "__main__":
    main()
