#!/usr/bin/env python
"""The radiance field at the reference composition (F = 8, H = 160), bounded and unbounded: gradient-free density /
colour calls at 2^20 points and the gradient pass (forward + backward) at 2^18 (profiles/unbounded_field.md).

    python tools/bench_unbounded.py unbounded      # fused (CNC_FIELD_CONTRACT) against fused_unbounded=False, alternating blocks
    python tools/bench_unbounded.py bounded        # the bounded fused calls of the tree the script imports
    python tools/bench_unbounded.py bounded --tree PATH      # ... of another checkout (its own built library): for an
                                                             # A/B against a parent commit, run both alternately

Positions: the unbounded tests' shared set (tests/contract_twin.py) for the unbounded field, uniform in the box for the
bounded one.  Times are device events around a block of calls, per call; a figure is the median over the blocks and
the spread is (min, max) over them."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FULL = dict(n_features_per_level=8, n_neurons=160, resolutions_list=(18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514),
            log2_hashmap_size=19, resolutions_list_2D=(130, 258, 514, 1026), log2_hashmap_size_2D=17)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bounded", "unbounded"])
    ap.add_argument("--tree", default=ROOT, help="checkout whose cnc_amd (and built library) is measured")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--n-grad", type=int, default=1 << 18)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import contract_twin as T
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda")
    torch.manual_seed(1)
    f = NGPRadianceField_mygrid_2D3D(aabb=torch.from_numpy(T.BOX.copy()), unbounded=a.what == "unbounded", **FULL).to(dev)
    with torch.no_grad():
        for e in f.mlp_base._encoders():
            e.params.uniform_(-1, 1)

    def inputs(n):
        if a.what == "unbounded":
            x = torch.from_numpy(T.points(n, seed=5)).to(dev)
        else:
            rng = np.random.default_rng(5)
            x = torch.from_numpy((T.BOX[:3] + (T.BOX[3:] - T.BOX[:3]) * rng.uniform(0, 1, (n, 3))).astype(np.float32)).to(dev)
        g = torch.Generator(device=dev).manual_seed(2)
        d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=-1)
        return x, d

    x, d = inputs(a.n)
    xg, dg = inputs(a.n_grad)
    g1, g2 = torch.randn(a.n_grad, 3, device=dev), torch.randn(a.n_grad, 1, device=dev)

    def density():
        with torch.no_grad():
            f.query_density(x)

    def colour():
        with torch.no_grad():
            f(x, d)

    def grad_pass():
        f.zero_grad(set_to_none=True)
        rgb, den = f(xg, dg)
        ((rgb * g1).sum() + (den * g2).sum()).backward()

    def block(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    variants = [("fused", True), ("op_chain", False)] if a.what == "unbounded" else [("fused", True)]
    jobs = (("density", density, a.n), ("colour", colour, a.n), ("grad_pass", grad_pass, a.n_grad))
    times = {(v, j): [] for v, _ in variants for j, _, _ in jobs}
    for v, on in variants:                     # warm up every shape of every variant
        f.fused_unbounded = on
        for _, fn, _ in jobs:
            fn(); fn()
    torch.cuda.synchronize()
    for _ in range(a.blocks):                  # alternate the variants block by block
        for v, on in variants:
            f.fused_unbounded = on
            for j, fn, _ in jobs:
                times[v, j].append(block(fn))
    assert f.fused_train, "the fused training route was left during the run"
    for (v, j), ts in times.items():
        ts = sorted(ts)
        print(json.dumps({"what": a.what, "label": a.label or os.path.abspath(a.tree), "variant": v, "job": j,
                          "samples": dict((k, n) for k, _, n in jobs)[j], "ms_median": round(ts[len(ts) // 2], 4),
                          "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4), "blocks": len(ts), "calls_per_block": a.calls}),
              flush=True)


if __name__ == "__main__":
    main()
