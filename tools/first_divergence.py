"""Where do two training runs from one seed first differ?

Builds two Trainers from the same seeds in ONE process and steps them in lock step (each with its own copy of the CPU
and GPU generators' states, swapped in around its step).  After every step: the step's result (loss, rate, sample
counts), every gradient, parameter and Adam moment and the occupancy grid are compared bit for bit; the first step and
tensor that differ are printed with the number of differing elements, and the tool stops there.

    python tools/first_divergence.py --steps 20 --reproducible --interfere      # the mode: expected to report nothing
    python tools/first_divergence.py --steps 20                                  # the default step

--interfere keeps a side stream busy with large matmuls during the second Trainer's steps (one process, one extra
stream: nothing else is started).  --shape toy|toy_fused|bench picks the configuration (the toy ones are the tests').
Exit status 1 when the runs diverge."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cnc_amd.trainer import TrainConfig, Trainer

TOY = dict(lmbda=2e-3, Pg_level=5, Pg_level_2D=3, log2_hashmap_size=12, log2_hashmap_size_2D=9, sample_num=3000,
           max_context_layer_num=3, n_features=2, n_neurons=32, resolutions_list=(10, 14, 18, 26, 34),
           resolutions_list_2D=(18, 34, 66), skip_levels_3D=(0, 1, 2), skip_levels_2D=(0,), max_steps=150,
           init_batch_size=512, target_sample_batch_size=1 << 14, grid_resolution=16, render_step_size=2e-2,
           milestones=(100, 130), warmup_iters=20, test_views=2, image_size=48)
SHAPES = {"toy": TOY, "toy_fused": dict(TOY, n_neurons=64),
          "bench": dict(n_features=8, sample_num=150000, max_steps=2000, image_size=400)}


class Run:
    def __init__(self, cfg, device, seed):
        torch.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
        self.tr = Trainer(cfg, device=device)
        self.rng = (torch.get_rng_state(), torch.cuda.get_rng_state(device))
        self.device = device

    def step(self, s):
        torch.set_rng_state(self.rng[0])
        torch.cuda.set_rng_state(self.rng[1], self.device)
        out = self.tr.train_step(s)
        torch.cuda.synchronize()
        self.rng = (torch.get_rng_state(), torch.cuda.get_rng_state(self.device))
        return out

    def tensors(self):
        tr, out = self.tr, {}
        for name, mod in (("field", tr.field), ("context", tr.context)):
            for n, p in mod.named_parameters():
                if p.grad is not None:
                    out[f"grad  {name}.{n}"] = p.grad
        for name, mod in (("field", tr.field), ("context", tr.context)):
            for n, p in mod.named_parameters():
                out[f"param {name}.{n}"] = p.detach()
        names = {id(p): f"{name}.{n}" for name, mod in (("field", tr.field), ("context", tr.context))
                 for n, p in mod.named_parameters()}
        for opt in (tr.opt, tr.opt2):
            for group in opt.param_groups:
                for p in group["params"]:
                    for k, v in opt.state.get(p, {}).items():
                        if isinstance(v, torch.Tensor):
                            out[f"adam  {names.get(id(p), '?')}.{k}"] = v
        out["occupancy binaries"] = tr.estimator.binaries
        return out


def first_difference(a, b, res_a, res_b):
    if (res_a is None) != (res_b is None):
        return "result (one run had no samples)", 1, 1
    for k in (res_a or {}):
        if res_a[k] != res_b.get(k):
            return f"result[{k!r}]: {res_a[k]!r} vs {res_b.get(k)!r}", 1, 1
    ta, tb = a.tensors(), b.tensors()
    if set(ta) != set(tb):
        return f"tensor sets differ: {sorted(set(ta) ^ set(tb))}", 1, 1
    for k in ta:
        x, y = ta[k], tb[k]
        if x.shape != y.shape:
            return f"{k}: shapes {tuple(x.shape)} vs {tuple(y.shape)}", x.numel(), x.numel()
        xb = x.contiguous().reshape(-1).view(torch.uint8).view(x.numel(), -1)
        yb = y.contiguous().reshape(-1).view(torch.uint8).view(y.numel(), -1)
        n = int((xb != yb).any(dim=1).sum())
        if n:
            return k, n, x.numel()
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="toy")
    ap.add_argument("--reproducible", action="store_true")
    ap.add_argument("--interfere", action="store_true")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out_dir", default="./bitstreams/first_divergence")
    args = ap.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    cfg = TrainConfig(**SHAPES[args.shape], reproducible=args.reproducible, out_dir=args.out_dir)
    a, b = Run(cfg, device, args.seed), Run(cfg, device, args.seed)
    side = torch.cuda.Stream(device) if args.interfere else None
    m = torch.randn(4096, 4096, device=device) if args.interfere else None
    d = first_difference(a, b, {}, {})
    if d:
        print(f"before the first step: {d[0]}: {d[1]} of {d[2]} elements differ")
        return 1
    for s in range(args.steps):
        res_a = a.step(s)
        if side is not None:
            with torch.cuda.stream(side):
                for _ in range(8):
                    m @ m
        res_b = b.step(s)
        d = first_difference(a, b, res_a, res_b)
        if d:
            print(f"step {s}: first difference in {d[0]}: {d[1]} of {d[2]} elements differ "
                  f"(mode {'on' if args.reproducible else 'off'}, shape {args.shape}, interfere {args.interfere})")
            return 1
    print(f"no divergence in {args.steps} steps (mode {'on' if args.reproducible else 'off'}, shape {args.shape}, "
          f"interfere {args.interfere})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
