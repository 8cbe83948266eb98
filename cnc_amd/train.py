"""`python -m cnc_amd.train` — the CNC protocol end to end with the reference driver's flags.

Flag names and defaults are those of examples/train_CNC_nerf_synthetic.py:71-133 (and
train_CNC_tank_temples.py for `--dataset tanks`); everything the reference hard-codes (:135-186: resolutions,
20000 steps, 2^18 target samples, lr 6e-3, schedules, aabb +-1.5 / bbox*1.2, step 5e-3 / 4e-3|1e-3) is the
default of `TrainConfig`.  What runs: train -> evaluate -> encode (.b files) -> wipe + decode -> evaluate ->
13-bit MLP quantisation -> evaluate, then ONE tab-separated results line with the reference's columns
(:562-613) appended to ./results/<dataset>/output.txt.

No dataset ships with this repository (no network): `--dataset procedural` (default when --data_root does not
exist) trains on the built-in analytic scene so the whole protocol can be exercised anywhere.
Extensions: --max_steps, --test_views (subset of the test images), --results, --dataset, `--dataset transforms`
(+ --aabb): a capture of one's own in the instant-ngp / nerfstudio transforms.json layout, lens distortion included, and
--save-mesh (+ --mesh-resolution, --mesh-threshold): the trained scene's surface as a PLY, and --refine-poses LR
(+ --refine-poses-from STEP): a capture's training poses refined next to the field, written to
<out_dir>/transforms_refined.json, and --background envmap (+ --envmap-resolution H, --envmap-lr LR): a learned
environment-map background behind the field, for opaque captures; the run then also writes <out_dir>/scene.cnc, the
container that holds the map, and --prune-floaters N (+ --prune-connectivity): the occupancy grid's small connected
components cleared once, after training and before the first evaluation, and --mesh-min-component N:
the same for the lattice a --save-mesh mesh is cut from, and --refine-exposure LR (+ --refine-exposure-from STEP): one
log-gain per training camera and colour channel learned next to the field, written to
<out_dir>/exposures.json, and --depth-weight W (+ --depth-spread K): depth supervision against a capture's measured
depth, or the procedural scene's exact one.
"""
from __future__ import annotations

import argparse
import math
import os
import pathlib
import time

import numpy as np
import torch

from .render import NERF_SYNTHETIC_SCENES, TANKS_SCENES
from .trainer import LoaderDataset, TrainConfig, Trainer, quantize_params

NAMED_SCENES = NERF_SYNTHETIC_SCENES + TANKS_SCENES + ["ball"]


class _Parser(argparse.ArgumentParser):
    """--scene was a closed list of choices; it stays one unless the run is on a capture (`dataset_kind`)."""

    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        try:
            dataset_kind(ns)
        except SystemExit as e:
            self.error(str(e))
        return ns


def build_parser():
    ap = _Parser(prog="python -m cnc_amd.train")
    ap.add_argument("--data_root", type=str, default=str(pathlib.Path.cwd() / "data/nerf_synthetic"),
                    help="the root dir of the dataset")
    ap.add_argument("--train_split", type=str, default="train", choices=["train", "trainval"],
                    help="which train split to use")
    ap.add_argument("--scene", type=str, default="chair",
                    help="which scene to use: one of " + ", ".join(NAMED_SCENES) + "; with --dataset transforms (or a "
                         "<data_root>/<scene>/transforms*.json and no --dataset) any directory name under --data_root")
    ap.add_argument("--lmbda", type=float, default=2e-3)
    ap.add_argument("--Pg_level", type=int, default=12)
    ap.add_argument("--Pg_level_2D", type=int, default=4)
    ap.add_argument("--log2_hashmap_size", type=int, default=19)
    ap.add_argument("--log2_hashmap_size_2D", type=int, default=17)
    ap.add_argument("--sample_num", type=int, default=200000)
    ap.add_argument("--max_context_layer_num", type=int, default=3)
    ap.add_argument("--n_features", type=int, default=4)
    # extensions
    ap.add_argument("--dataset", choices=["nerf_synthetic", "tanks", "procedural", "transforms"], default=None,
                    help="transforms: a capture in the instant-ngp / nerfstudio transforms.json layout, lens distortion "
                         "included (DESIGN.md §4.11); bounded scenes only, so give the box in the file or with --aabb")
    ap.add_argument("--aabb", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                    help="--dataset transforms: the scene box; overrides the file's `aabb`, which overrides the default")
    ap.add_argument("--max_steps", type=int, default=20000)
    ap.add_argument("--test_views", type=int, default=None, help="evaluate this many test images (default: all)")
    ap.add_argument("--image_size", type=int, default=200, help="procedural scene only")
    ap.add_argument("--seed", type=int, default=42, help="set_random_seed value (the reference drivers fix 42, train:135)")
    ap.add_argument("--results", type=str, default=None, help="results file (default ./results/<dataset>/output.txt)")
    ap.add_argument("--out_dir", type=str, default=None, help="bitstream directory (default ./bitstreams/<scene>)")
    ap.add_argument("--reproducible", action="store_true",
                    help="the reproducible mode: ordered reductions, one host thread, one stream (DESIGN.md §5); two runs "
                         "from one seed give the same bits on one GPU")
    ap.add_argument("--guarded-step", dest="guarded_step", action="store_true",
                    help="the guarded step: an optimizer update whose gradients or loss are non-finite, or whose forward "
                         "tripped the fp16 range guard, is skipped, decided on the device (DESIGN.md §13)")
    ap.add_argument("--device-coder", dest="device_coder", action="store_true",
                    help="code the tables with the device entropy coder (interleaved rANS on the GPU, DESIGN.md §4.8) "
                         "instead of the host range coder; the .b files are then in the rans1 format")
    ap.add_argument("--occupancy-coder", dest="occupancy_coder", choices=["iid", "pyramid"], default="iid",
                    help="the container's occupancy section: one Bernoulli frequency for every cell (iid), or the grid "
                         "coded from a pyramid of itself with the tables' coder (pyramid, DESIGN.md §4.9)")
    ap.add_argument("--mlp-coder", dest="mlp_coder", choices=["packed", "tree"], default="packed",
                    help="the container's MLP: every tensor's 13-bit indices bit-packed (packed), or the same indices coded "
                         "with a per-tensor bit-tree model and the tables' coder where that is smaller (tree, DESIGN.md "
                         "§4.12); lossless either way")
    ap.add_argument("--distortion-weight", dest="distortion_weight", type=float, default=0.0,
                    help="weight of mip-NeRF 360's interval-distortion loss on the rendered samples, added to the ray loss "
                         "(mean over the batch's rays; DESIGN.md §4.10); 0 = off")
    ap.add_argument("--depth-weight", dest="depth_weight", type=float, default=0.0, metavar="W",
                    help="weight of depth supervision, added to the ray loss: the batch mean of (sum w e)^2 + K sum w e^2 over "
                         "the rendered samples, e = a sample's distance from the ray's measured depth (DESIGN.md §4.19).  "
                         "--dataset transforms with a depth_file_path per frame, or --dataset procedural; one process; "
                         "0 = off.  UNTUNED: nobody has run this on a real capture here")
    ap.add_argument("--depth-spread", dest="depth_spread", type=float, default=1.0, metavar="K",
                    help="--depth-weight: the weight K of the line-of-sight term sum w e^2 inside the depth loss; >= 0")
    ap.add_argument("--save-mesh", dest="save_mesh", type=str, default=None, metavar="PATH",
                    help="at the very end, write the scene's surface as a binary PLY: marching tetrahedra on the density of "
                         "the model a receiver would hold (decoded tables, 13-bit MLP; DESIGN.md §4.13); default: off")
    ap.add_argument("--mesh-resolution", dest="mesh_resolution", type=int, default=256,
                    help="--save-mesh: lattice cells along the box's longest side")
    ap.add_argument("--mesh-threshold", dest="mesh_threshold", type=float, default=None,
                    help="--save-mesh: the density of the surface; default ln 2 / render_step_size (one render step half "
                         "opaque), which scales with the scene and has not been tuned")
    ap.add_argument("--refine-poses", dest="refine_poses", type=float, default=0.0, metavar="LR",
                    help="--dataset transforms: learn a correction (rotation vector, translation) of every training "
                         "camera's pose at this Adam learning rate (DESIGN.md §4.14) and write the capture with the refined "
                         "poses to <out_dir>/transforms_refined.json; 0 = off.  The rate has no tuned default")
    ap.add_argument("--refine-poses-from", dest="refine_poses_from", type=int, default=0, metavar="STEP",
                    help="--refine-poses: the first step that moves the poses")
    ap.add_argument("--refine-exposure", dest="refine_exposure", type=float, default=0.0, metavar="LR",
                    help="--dataset transforms: learn a log-gain per training camera and colour channel (exposure and white "
                         "balance, DESIGN.md §4.17) at this Adam learning rate and write them to <out_dir>/exposures.json; "
                         "evaluation, the mesh and the container render at gain 1, the geometric mean of the training "
                         "exposures; 0 = off.  The rate has no tuned default: nobody has run this on a real capture here")
    ap.add_argument("--refine-exposure-from", dest="refine_exposure_from", type=int, default=0, metavar="STEP",
                    help="--refine-exposure: the first step that moves the gains")
    ap.add_argument("--error-map-sampling", dest="error_map_sampling", action="store_true",
                    help="--dataset transforms: draw the training pixels in proportion to a coarse per-image map of the "
                         "recent loss instead of uniformly, every ray's loss divided by its sampling density (instant-ngp's "
                         "error map without its sharpness term, DESIGN.md §4.18); one process only.  The uniform floor "
                         "(0.5), the map's decay (0.9) and the steps between rebuilds of the CDF (16) are untuned")
    ap.add_argument("--error-map-resolution", dest="error_map_resolution", type=int, default=16, metavar="G",
                    help="--error-map-sampling: the map holds G x G cells per training image; 1..64.  The default is untuned")
    ap.add_argument("--background", choices=["solid", "envmap"], default="solid",
                    help="what lies behind the field: the batch's colour (solid), or a learned equirectangular texture "
                         "indexed by ray direction (envmap, DESIGN.md §4.15) for opaque captures without an alpha channel; "
                         "one process only.  With envmap the run also writes <out_dir>/scene.cnc, the container with the map")
    ap.add_argument("--envmap-resolution", dest="envmap_resolution", type=int, default=16, metavar="H",
                    help="--background envmap: the texture is [H, 2H, 3]; H even, 2..64.  The default is untuned")
    ap.add_argument("--envmap-lr", dest="envmap_lr", type=float, default=1e-2, metavar="LR",
                    help="--background envmap: the constant Adam rate of the texture.  The default is untuned")
    ap.add_argument("--prune-floaters", dest="prune_floaters", type=int, default=0, metavar="N",
                    help="after training and before the first evaluation, clear every connected component of the occupancy "
                         "grid with fewer than N cells (the largest always stays; DESIGN.md §4.16); the test views are "
                         "evaluated before and after, so that the cut's cost shows.  0 = off.  N has no tuned value")
    ap.add_argument("--prune-connectivity", dest="prune_connectivity", type=int, choices=[6, 14, 26], default=26,
                    help="--prune-floaters: which cells count as neighbours; 26 merges most and removes least")
    ap.add_argument("--mesh-min-component", dest="mesh_min_component", type=int, default=0, metavar="N",
                    help="--save-mesh: drop the components of the lattice's inside set with fewer than N points before the "
                         "surface is cut (the largest always stays); 0 = off.  N has no tuned value")
    return ap


def _has_transforms(data_root, scene):
    scene_dir = os.path.join(data_root, scene)
    return os.path.isdir(scene_dir) and any(f.startswith("transforms") and f.endswith(".json") for f in os.listdir(scene_dir))


def dataset_kind(args):
    """--dataset, or what --data_root / --scene imply.  A scene outside the named ones is a capture: it needs
    `--dataset transforms`, or a transforms*.json under <data_root>/<scene>."""
    kind = getattr(args, "dataset", None)
    named = args.scene in NAMED_SCENES
    if kind is None:
        if not named and _has_transforms(args.data_root, args.scene):
            kind = "transforms"
        elif named:
            root_has_scene = os.path.isdir(os.path.join(args.data_root, args.scene))
            kind = ("tanks" if args.scene in TANKS_SCENES else "nerf_synthetic") if root_has_scene else "procedural"
    if not named and kind != "transforms":
        raise SystemExit(f"--scene {args.scene!r}: not one of {', '.join(NAMED_SCENES)}; a scene of another name needs "
                         "--dataset transforms or a transforms*.json under <data_root>/<scene>")
    return kind


def make_config_and_data(args, device, rank=0, world=1):
    kind = dataset_kind(args)
    scene = args.scene if kind != "procedural" else "ball"
    kw = dict(scene=scene, lmbda=args.lmbda, Pg_level=args.Pg_level, Pg_level_2D=args.Pg_level_2D,
              log2_hashmap_size=args.log2_hashmap_size, log2_hashmap_size_2D=args.log2_hashmap_size_2D,
              sample_num=args.sample_num, max_context_layer_num=args.max_context_layer_num,
              n_features=args.n_features, max_steps=args.max_steps, image_size=args.image_size, seed=args.seed,
              out_dir=args.out_dir or f"./bitstreams/{scene}", reproducible=args.reproducible, guarded_step=args.guarded_step,
              device_coder=args.device_coder, occupancy_coder=args.occupancy_coder, mlp_coder=args.mlp_coder,
              distortion_weight=args.distortion_weight, depth_weight=args.depth_weight, depth_spread=args.depth_spread,
              save_mesh=args.save_mesh, mesh_resolution=args.mesh_resolution, mesh_threshold=args.mesh_threshold,
              pose_lr=args.refine_poses, pose_refine_from=args.refine_poses_from, exposure_lr=args.refine_exposure,
              exposure_from=args.refine_exposure_from, error_map=args.error_map_sampling,
              error_map_resolution=args.error_map_resolution, background=args.background,
              envmap_resolution=args.envmap_resolution, envmap_lr=args.envmap_lr, prune_floaters=args.prune_floaters,
              prune_connectivity=args.prune_connectivity,
              weight_decay=2e-5 if scene == "drums" else 2e-6)           # train:170-172
    if args.max_steps != 20000:      # the milestones of a shortened run keep their relative positions
        f = args.max_steps / 20000.0
        kw.update(milestones=tuple(int(m * f) for m in (9000, 12000, 15000, 17000, 19000)),
                  warmup_iters=max(1, int(1000 * f)))
    dataset = None
    if kind == "nerf_synthetic":
        from .datasets import SubjectLoader
        train = SubjectLoader(subject_id=scene, root_fp=args.data_root, split=args.train_split,
                              num_rays=1024, device=device)
        test = SubjectLoader(subject_id=scene, root_fp=args.data_root, split="test", num_rays=None, device=device)
        dataset = LoaderDataset(train, test)
    elif kind == "tanks":
        from .datasets import SubjectLoader_Tanks
        train = SubjectLoader_Tanks(subject_id=scene, root_fp=args.data_root, split="train", num_rays=1024, device=device)
        test = SubjectLoader_Tanks(subject_id=scene, root_fp=args.data_root, split="test", num_rays=None, device=device)
        # near_plane stays 0.0: the reference driver never hands the loader's NEAR to the sampler
        # (train_CNC_tank_temples.py:176)
        kw.update(aabb=tuple(float(v) for v in train.aabb.tolist()), render_step_size=train.render_step_size)
        dataset = LoaderDataset(train, test)
    elif kind == "transforms":
        from .datasets import TransformsLoader
        train = TransformsLoader(subject_id=scene, root_fp=args.data_root, split="train", num_rays=1024, device=device)
        test = TransformsLoader(subject_id=scene, root_fp=args.data_root, split="test", num_rays=None, device=device)
        box = getattr(args, "aabb", None)
        if box is None and train.aabb is not None:
            box = train.aabb.tolist()
        if box is not None:                       # --aabb, else the file's, else TrainConfig's default
            kw.update(aabb=tuple(float(v) for v in box))
        dataset = LoaderDataset(train, test)
    if dataset is not None and world > 1:
        # data parallelism: every rank draws its OWN images / pixels (the all-reduce then averages world different
        # batches); replica-identical draws (occupancy cells, context windows) stay on the global generators
        dataset.seed_sampling(42 + 1000 * rank)
    n_test = len(dataset) if dataset is not None else 4
    kw["test_views"] = n_test if args.test_views is None else min(args.test_views, n_test)
    return kind, TrainConfig(**kw), dataset


@torch.no_grad()
def evaluate(tr: Trainer, n_views: int):
    """(psnr, lpips, -ssim) averaged over the test views, as train:384-431 (LPIPS unavailable: NaN).
    world > 1: the views are sharded over the ranks (`cdist.shard_range`) and the two sums are
    all-reduced — every rank calls this at the same point of the protocol and gets the same three numbers."""
    from . import dist as cdist
    from .metrics import psnr, ssim
    tr.field.eval(); tr.estimator.eval()
    lo, hi = cdist.shard_range(n_views, tr.rank, tr.world)
    ps = ss = 0.0
    for i in range(lo, hi):
        d = tr.dataset.view(i)
        rgb = tr.render_test_view(d)
        ps += psnr(rgb, d["pixels"])
        ss += -ssim(rgb.permute(2, 0, 1).unsqueeze(0), d["pixels"].permute(2, 0, 1).unsqueeze(0))
    ps, ss = cdist.sum_over_ranks([ps, ss], tr.device)
    return ps / max(n_views, 1), float("nan"), ss / max(n_views, 1)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cnc_amd.train needs an MI355X (the HIP extension has no CPU fallback)")
    # under `torchrun --nproc-per-node N`: join the group first, so that the loaders are built on THIS rank's GPU
    from . import dist as cdist
    rank, _, world = cdist.init()
    device = torch.device("cuda", cdist.local_device_index() if world > 1 else 0)
    kind, cfg, dataset = make_config_and_data(args, device, rank, world)
    tr = Trainer(cfg, device=device, dataset=dataset)
    r4 = lambda v: str(np.round(v, decimals=4))

    tic = time.time()
    tr.train(steps=cfg.max_steps)
    elapsed = time.time() - tic
    # world > 1: the replicas are identical after training.  Every rank runs the whole tail — its share of each
    # evaluation (views sharded, sums all-reduced), and the codec round trip on files of its own (the coder is
    # deterministic: same bytes on every rank; decode is sequential over levels, so it cannot be sharded) — so no
    # rank waits in a barrier under the communicator's watchdog while another one works.  Rank 0's files are the
    # ones under the canonical prefix, and rank 0 prints and writes the results line.
    say = print if rank == 0 else (lambda *a, **k: None)
    if cfg.prune_floaters > 0:
        # once, before anything reads the grid: the evaluations, the codec, the container and the mesh then see the one
        # pruned grid (every rank prunes its replica's: same grid, same result).  A thin detached part of the scene can be
        # a small component, so the views are evaluated on the unpruned grid first
        psnr_before, _, _ = evaluate(tr, cfg.test_views)
        say(f"evaluation_before_pruning: psnr_avg={psnr_before}")
        stats = tr.prune_floaters()
        say(f"pruned: {stats['removed_components']} components / {stats['removed_cells']} cells removed, "
            f"{stats['components'] - stats['removed_components']} components kept")
    psnr_avg, lpips_avg, ssim_avg = evaluate(tr, cfg.test_views)
    say(f"evaluation: psnr_avg={psnr_avg}, lpips_avg={lpips_avg}, ssim_avg={ssim_avg}")

    tic = time.time()
    Pgs, embed_bits_MB, embed_bits_MB_codec, prefix = tr.encode(
        None if rank == 0 else os.path.join(cfg.out_dir, f".rank{rank}", "b"))
    encoding_time = time.time() - tic
    say(f"encoded: estimated {embed_bits_MB} MB, coded {embed_bits_MB_codec} MB in {encoding_time:.1f} s")
    tic = time.time()
    tr.decode_into_field(Pgs, prefix)
    decoding_time = time.time() - tic
    psnr_c, lpips_c, ssim_c = evaluate(tr, cfg.test_views)
    say(f"evaluation_decoded: psnr_avg_codec={psnr_c}, lpips_avg_codec={lpips_c}, ssim_avg_codec={ssim_c}, "
          f"size_codec={embed_bits_MB_codec}")

    if tr.envmap is not None and rank == 0:
        # the learned background travels in the container only (the .b files hold the tables): write one, from the model as
        # it stands here — decoded tables, the MLP not yet quantised (the container quantises it itself)
        box = os.path.join(cfg.out_dir, "scene.cnc")
        kb = tr.save_container(box)
        say(f"container with the learned background ({tr.envmap.texture.numel()} bytes of envmap): {box}, "
            f"{kb['file_KB']:.1f} KB")
    sizes = tr.sizes_MB(embed_bits_MB_codec)
    occ_note = ""
    if tr.occupancy_coder_name() == "pyramid" and all(int(s) % 2 == 0 for s in tr.estimator.binaries.shape[1:]):
        # the occupancy grid as the container would hold it: a coded section's size, not the reference's estimate
        # (a grid with an odd side has no pyramid and keeps the estimate, as its container keeps the Bernoulli section)
        from .occupancy_codec import encode_occupancy
        blob, _ = encode_occupancy(tr.estimator.binaries, coder=tr.coder_name(), symbols_per_lane=cfg.symbols_per_lane)
        occ_note = (f" (occupancy grid: pyramid1 section of {len(blob) / 1024:.2f} KB as coded, in place of the "
                    f"{sizes['occupancy_grid'] * 1024:.2f} KB estimate)")
        sizes["occupancy_grid"] = len(blob) / 1024.0 / 1024.0
    mlp = {n: p for n, p in tr.field.named_parameters() if "encoding" not in n}
    cols = [cfg.scene, r4(psnr_avg), r4(lpips_avg), r4(ssim_avg), r4(psnr_c), r4(lpips_c), r4(ssim_c),
            r4(embed_bits_MB), r4(embed_bits_MB_codec)]
    per_digit = []
    MBs_orig = 0.0
    for digit in [13]:
        MBs, MBs_orig, q_state = quantize_params(mlp, digits=digit)
        tr.field.load_state_dict(q_state, strict=False)
        p_q, l_q, s_q = evaluate(tr, cfg.test_views)
        total = embed_bits_MB_codec + sizes["context_models"] + sizes["occupancy_grid"] + MBs
        per_digit += [str(digit), r4(MBs), r4(p_q), r4(l_q), r4(s_q), r4(total)]
        say(f"{digit}-bit MLP: psnr={p_q}, total size {total * 1024:.1f} KB{occ_note}")
    cols += [r4(MBs_orig), r4(sizes["context_models"]), r4(sizes["occupancy_grid"])] + per_digit
    cols += [r4(elapsed), r4(encoding_time), r4(decoding_time)]

    if rank != 0:
        import shutil
        shutil.rmtree(os.path.join(cfg.out_dir, f".rank{rank}"), ignore_errors=True)
        return cols
    folder = {"nerf_synthetic": "Synthetic-NeRF", "tanks": "TanksAndTemple", "procedural": "procedural",
              "transforms": "transforms"}[kind]
    out = args.results or os.path.join("./results", folder, "output.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as fw:
        fw.write("\t".join(cols) + "\n")
    print(f"results line appended to {out}")
    if cfg.save_mesh:
        # last of all, on the decoded tables and the 13-bit MLP: the mesh of the model a receiver would hold
        mesh = tr.extract_mesh(cfg.save_mesh, resolution=cfg.mesh_resolution, threshold=cfg.mesh_threshold,
                               min_component_points=int(getattr(args, "mesh_min_component", 0)))
        print(f"mesh: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces written to {cfg.save_mesh}")
    return cols


if __name__ == "__main__":
    main()
