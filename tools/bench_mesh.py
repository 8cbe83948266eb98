"""Mesh export on the full-size procedural model (profiles/mesh_export.md): time of `Trainer.extract_mesh` split into
density evaluation, extraction and colours, the share of lattice points the occupancy grid spares, V, F and the largest
component's share of the faces.

    python tools/bench_mesh.py [--steps 300] [--resolutions 256 512] [--repeats 3] [--out FILE.json]

Times are host clocks around work that ends in a device synchronise; the first export of every resolution is a warm-up
and is not reported.  The density share is measured inside the export (a synchronise around every chunk's field call);
"extraction" is the export without colours minus that share: the five kernels, the two scans, the `nonzero` and the
allocations.  One JSON line per resolution.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh needs a GPU"
    from cnc_amd.backends import iso_surface as iso
    from cnc_amd.trainer import TrainConfig, Trainer
    f = args.steps / 20000.0
    cfg = TrainConfig(max_steps=args.steps, milestones=tuple(int(m * f) for m in (9000, 12000, 15000, 17000, 19000)),
                      warmup_iters=max(1, int(1000 * f)), out_dir=tempfile.mkdtemp())
    tr = Trainer(cfg, device="cuda")
    t0 = _sync_time()
    tr.train(steps=args.steps, log=None)
    train_s = _sync_time() - t0
    field = tr.field
    inner = field.query_density
    spent = {"density": 0.0, "points": 0}

    def timed_density(x):
        t = _sync_time()
        y = inner(x)
        spent["density"] += _sync_time() - t
        spent["points"] += x.shape[0]
        return y
    lines = []
    for res in args.resolutions:
        rows = []
        for rep in range(args.repeats + 1):
            field.query_density = timed_density
            spent.update(density=0.0, points=0)
            t = _sync_time()
            mesh = tr.extract_mesh(resolution=res, colors=False)
            no_colors = _sync_time() - t
            density, points = spent["density"], spent["points"]
            t = _sync_time()
            mesh = tr.extract_mesh(resolution=res, colors=True)
            with_colors = _sync_time() - t
            field.query_density = inner
            if rep:
                rows.append((no_colors, density, with_colors))
        no_colors, density, with_colors = (float(np.median([r[k] for r in rows])) for k in range(3))
        n = (res,) * 3
        lattice = (res + 1) ** 3
        comp = mesh.components()
        line = {"resolution": res, "train_steps": args.steps, "train_s": round(train_s, 2), "lattice_points": lattice,
                "evaluated_points": points, "spared_share": round(1 - points / lattice, 4),
                "export_ms": round(1e3 * with_colors, 1), "density_ms": round(1e3 * density, 1),
                "extraction_ms": round(1e3 * (no_colors - density), 1), "colors_ms": round(1e3 * (with_colors - no_colors), 1),
                "V": int(mesh.vertices.shape[0]), "F": int(mesh.faces.shape[0]), "components": int(comp.shape[0]),
                "largest_component_share": round(float(comp[0]) / max(int(comp.sum()), 1), 4) if comp.shape[0] else None,
                "threshold": float(np.log(2.0) / cfg.render_step_size), "repeats": args.repeats,
                "peak_memory_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del mesh
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(lines, fh, indent=1)


if __name__ == "__main__":
    main()
