"""The numbers of profiles/floater_pruning.md, one JSON line per measurement, on one MI355X:

    python tools/bench_components.py

Label + sizes per connectivity on random 128^3 grids, on the occupancy grid of the full-size model after 300 steps of
the procedural protocol and on the 257^3 / 513^3 lattices of its mesh export (device events, 3 warm-up calls, 10 timed);
the 800x800 evaluation render, the occupancy sections and the container before and after `Trainer.prune_floaters`;
`Mesh.components(on_device=True)` against the host path.  The first error ends the run."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cnc_amd.backends import components as C             # noqa: E402

dev = torch.device("cuda:0")


def say(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return {"median_ms": round(out[len(out) // 2], 4), "min_ms": round(out[0], 4), "max_ms": round(out[-1], 4), "reps": reps}


def label_and_sizes(name, mask):
    m = mask.to(dev).contiguous()
    m4 = (m.view(torch.uint8) if m.dtype == torch.bool else m).reshape((1,) + tuple(m.shape[-3:]))
    labels, sizes = torch.empty(m4.shape, dtype=torch.int32, device=dev), torch.empty(m4.shape, dtype=torch.int32, device=dev)
    for c in (6, 14, 26):
        t_l = timed(lambda: C.label_grid(m4, c, labels))
        t_s = timed(lambda: C.sizes(labels, sizes))
        n = int((sizes > 0).sum())
        say(what="label+sizes", grid=name, shape=list(m4.shape[1:]), set_cells=int(m4.ne(0).sum()), connectivity=c, components=n,
            largest=int(sizes.max()), label=t_l, sizes=t_s)


try:
    for p in (0.18, 0.31):
        label_and_sizes(f"random p={p}", torch.from_numpy(np.random.default_rng(9).random((128, 128, 128)) < p))
except Exception as e:      # noqa: BLE001
    say(error=f"random: {type(e).__name__}: {e}")
    sys.exit(3)          # nothing more on the GPU after an error

tr = None
try:
    from cnc_amd.trainer import TrainConfig, Trainer
    out_dir = tempfile.mkdtemp()
    cfg = TrainConfig(n_features=8, sample_num=150000, image_size=400, out_dir=out_dir)
    tr = Trainer(cfg, device=dev)
    t0 = time.perf_counter()
    for step in range(300):
        tr.train_step(step, want_stats=False)
    torch.cuda.synchronize()
    say(what="trained", steps=300, seconds=round(time.perf_counter() - t0, 1), grid=list(tr.estimator.binaries.shape))
    label_and_sizes("trained occupancy grid, 300 steps", tr.estimator.binaries[0])
except Exception as e:      # noqa: BLE001
    say(error=f"train: {type(e).__name__}: {e}")
    sys.exit(3)          # nothing more on the GPU after an error


def occupancy_bytes(binaries):
    from cnc_amd import container
    from cnc_amd.occupancy_codec import encode_occupancy
    occ = binaries.reshape(-1).to(torch.float32).cpu()
    pg = float(occ.mean().clamp(1e-6, 1 - 1e-6))
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "occ.b")
        container.encoder(occ * 2 - 1, torch.full_like(occ, pg), f)
        iid = os.path.getsize(f)
    blob, _ = encode_occupancy(binaries, coder="host")
    return {"iid_bytes": iid, "pyramid_bytes": len(blob)}


def eval_render():
    from cnc_amd.render import render_image_with_occgrid_test
    from cnc_amd.trainer import SyntheticBallDataset
    c = tr.cfg
    tr.field.eval(); tr.estimator.eval()
    view = SyntheticBallDataset(800, device=dev, seed=0).view(0)
    args = dict(near_plane=c.near_plane, render_step_size=c.render_step_size, render_bkgd=view["color_bkgd"],
                cone_angle=c.cone_angle, alpha_thre=c.alpha_thre)
    with torch.no_grad():
        for _ in range(2):
            render_image_with_occgrid_test(1024, tr.field, tr.estimator, view["rays"], **args)
        torch.cuda.synchronize()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            rgb, _, _, n_shaded = render_image_with_occgrid_test(1024, tr.field, tr.estimator, view["rays"], **args)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        mse = torch.nn.functional.mse_loss(rgb, view["pixels"]).item()
    ts.sort()
    tr.field.train(); tr.estimator.train()
    return {"median_ms": round(ts[2], 2), "min_ms": round(ts[0], 2), "max_ms": round(ts[-1], 2), "shaded_samples": int(n_shaded),
            "psnr": round(-10.0 * float(np.log10(max(mse, 1e-12))), 4)}


if tr is not None:
    try:
        keep = (tr.estimator.binaries.clone(), tr.estimator.occs.clone())
        before = {"render": eval_render(), "occupancy": occupancy_bytes(tr.estimator.binaries), "set_cells": int(tr.estimator.binaries.sum())}
        say(what="full-size run, before pruning", **before)
        for n, c in ((2, 26), (8, 26), (64, 26), (8, 6)):
            tr.estimator.binaries, tr.estimator.occs = keep[0].clone(), keep[1].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats = tr.prune_floaters(min_cells=n, connectivity=c)
            torch.cuda.synchronize()
            say(what="full-size run, pruned", min_cells=n, connectivity=c, stats=stats, prune_call_ms=round((time.perf_counter() - t0) * 1e3, 2),
                render=eval_render(), occupancy=occupancy_bytes(tr.estimator.binaries), set_cells=int(tr.estimator.binaries.sum()))
        tr.estimator.binaries, tr.estimator.occs = keep[0].clone(), keep[1].clone()
    except Exception as e:      # noqa: BLE001
        say(error=f"prune: {type(e).__name__}: {e}")
        sys.exit(3)          # nothing more on the GPU after an error
    for res in (256, 512):
        try:
            thr = float(np.log(2.0) / tr.cfg.render_step_size)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh, lattice = tr.extract_mesh(resolution=res, colors=False, return_lattice=True)
            torch.cuda.synchronize()
            t_plain = time.perf_counter() - t0
            say(what="mesh", resolution=res, vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]), extract_s=round(t_plain, 3))
            label_and_sizes(f"mesh lattice, resolution {res}", lattice >= thr)
            del lattice
            t_dev = timed(lambda: mesh.components(on_device=True), warm=1, reps=5)
            t0 = time.perf_counter()
            dev_counts = mesh.components(on_device=True)
            t_dev_wall = time.perf_counter() - t0
            t0 = time.perf_counter()
            host_counts = mesh.components()
            t_host = time.perf_counter() - t0
            say(what="Mesh.components", resolution=res, faces=int(mesh.faces.shape[0]), components=int(host_counts.size),
                largest=int(host_counts[0]) if host_counts.size else 0, identical=bool(np.array_equal(dev_counts, host_counts)),
                on_device=t_dev, on_device_wall_s=round(t_dev_wall, 4), host_s=round(t_host, 2))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pruned = tr.extract_mesh(resolution=res, colors=False, min_component_points=64)
            torch.cuda.synchronize()
            say(what="mesh, min_component_points=64", resolution=res, faces=int(pruned.faces.shape[0]),
                components=int(pruned.components(on_device=True).size), extract_s=round(time.perf_counter() - t0, 3))
            del mesh, pruned
        except Exception as e:      # noqa: BLE001
            say(error=f"mesh {res}: {type(e).__name__}: {e}")
            sys.exit(3)          # nothing more on the GPU after an error
    try:
        for n in (8,):
            for tag, binaries in (("unpruned", keep[0]), ("pruned", None)):
                tr.estimator.binaries, tr.estimator.occs = keep[0].clone(), keep[1].clone()
                if binaries is None:
                    tr.prune_floaters(min_cells=n, connectivity=26)
                path = os.path.join(out_dir, f"{tag}.cnc")
                info = tr.save_container(path)
                from cnc_amd.container import section_sizes
                say(what="container", grid=tag, min_cells=n, file_bytes=os.path.getsize(path), occupancy_section=section_sizes(path).get("occupancy"),
                    coder=tr.occupancy_coder_name())
        tr.estimator.binaries, tr.estimator.occs = keep[0].clone(), keep[1].clone()
    except Exception as e:      # noqa: BLE001
        say(error=f"container: {type(e).__name__}: {e}")
        sys.exit(3)          # nothing more on the GPU after an error
