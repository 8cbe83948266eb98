"""End-to-end driver for the CNC protocol: train -> evaluate -> encode -> decode -> evaluate.

Follows the behaviour of examples/train_CNC_nerf_synthetic.py (hyper-parameters :135-186, optimisers
and schedules :257-297, loop :302-366, evaluation / codec :384-506), not its text: the reference
script cannot travel to the GPU box and its datasets are not available offline, so the scene here is
a procedural one (`cnc_amd.datasets.SyntheticBallDataset`, same `fetch`-style interface as
examples/datasets/nerf_synthetic.py:132-239).  Flag names of the reference's argparse are kept in
`TrainConfig`.

Data parallelism (new): one process per GPU; each rank draws its own rays, gradients of
ALL parameters live in one flat bucket that is all-reduced once per step (cnc_amd.dist.GradBucket);
the occupancy grid and the context-window draw are broadcast from rank 0 so replicas stay identical.
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _gradsink, _repro, _step_guard, _table_adam
from . import dist as cdist
from .context import CNC_context_models
from .datasets import LoaderDataset, SyntheticBallDataset, TransformsLoader  # noqa: F401  (re-exported: bench.py and the tests import them from here)
from .field import NGPRadianceField_mygrid_2D3D
from .nerfacc import OccGridEstimator
from .render import Rays, render_image_with_occgrid, render_image_with_occgrid_test, set_random_seed


@dataclass
class TrainConfig:
    # reference flags (train_CNC_nerf_synthetic.py:71-133)
    scene: str = "ball"
    lmbda: float = 2e-3
    Pg_level: int = 12
    Pg_level_2D: int = 4
    log2_hashmap_size: int = 19
    log2_hashmap_size_2D: int = 17
    sample_num: int = 200000
    max_context_layer_num: int = 3
    n_features: int = 4
    fused_features: bool = True      # encoders write straight into the base MLP's input matrix
    sh_fp16_round: bool = True       # direction encoding rounded through half, as tiny-cuda-nn hands it to the reference
    # hard-coded in the reference (:135-186)
    n_neurons: int = 160
    resolutions_list: Tuple[int, ...] = (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514)
    resolutions_list_2D: Tuple[int, ...] = (130, 258, 514, 1026)
    step_update: int = 16
    skip_levels_3D: Tuple[int, ...] = (0, 1, 2)
    skip_levels_2D: Tuple[int, ...] = (0,)
    max_steps: int = 20000
    init_batch_size: int = 1024
    target_sample_batch_size: int = 1 << 18
    weight_decay: float = 2e-6
    aabb: Tuple[float, ...] = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
    near_plane: float = 0.0
    far_plane: float = 1.0e10
    grid_resolution: int = 128
    grid_nlvl: int = 1
    render_step_size: float = 5e-3
    alpha_thre: float = 0.0
    cone_angle: float = 0.0
    lr: float = 6e-3
    milestones: Tuple[int, ...] = (9000, 12000, 15000, 17000, 19000)
    warmup_iters: int = 1000
    seed: int = 42
    # evaluation
    test_views: int = 4
    image_size: int = 200
    dimension_wise_resolution: Optional[int] = None   # default: finest 3-D resolution
    out_dir: str = "./bitstreams/ball"
    log_every: int = 200
    # the reproducible mode (cnc_amd._repro): every step of this Trainer under `cnc_amd.reproducible(True)`, on
    # the one-thread, one-stream schedule and without the planes' graph
    reproducible: bool = False
    # the guarded step (cnc_amd._step_guard): a step whose small gradients or loss scalars hold a non-finite
    # value, or whose forward tripped the fp16 range guard, updates nothing — decided on the device, no host wait.
    # Also CNC_GUARDED_STEP=1
    guarded_step: bool = False
    # the device entropy coder (cnc_amd.coders.DeviceCoder): `encode` / `save_container` code the tables on
    # the GPU in the "rans1" format instead of with the host range coder.  Also CNC_DEVICE_CODER=1.  Off by default.
    device_coder: bool = False
    symbols_per_lane: Optional[int] = None     # of the device coder; None = cnc_amd.coders.DEVICE_CODER_SYMBOLS_PER_LANE
    # the occupancy section of `save_container`: "iid" (one Bernoulli frequency for every cell) or "pyramid" (the grid coded
    # from a pyramid of itself with the tables' coder, cnc_amd.occupancy_codec).  Also CNC_OCC_CODER=pyramid.
    occupancy_coder: str = "iid"
    # the MLP of `save_container`: "packed" (every tensor's 13-bit indices bit-packed) or "tree" (the same indices coded with
    # a per-tensor bit-tree model and the tables' coder where that is smaller, cnc_amd.mlp_codec, DESIGN.md §4.12: lossless
    # against "packed").  Also CNC_MLP_CODER=tree.
    mlp_coder: str = "packed"
    # the distortion regulariser (cnc_amd.nerfacc.losses.distortion): the ray loss becomes mse + this weight
    # times the mean over the batch's rays of mip-NeRF 360's interval-distortion loss on the rendered samples.  0 = off: the
    # step makes exactly the calls it makes without it.  Read once, when the Trainer is built
    distortion_weight: float = 0.0
    # mesh export (cnc_amd.mesh): `python -m cnc_amd.train --save-mesh PATH` writes the trained scene's
    # iso-surface as a PLY at the very end of the run.  None = off: the run and its results line are what they were.
    # mesh_threshold None = ln 2 / render_step_size (`Trainer.extract_mesh`)
    save_mesh: Optional[str] = None
    mesh_resolution: int = 256
    mesh_threshold: Optional[float] = None
    # camera pose refinement (cnc_amd.poses): the learning rate of one (omega, tau) per training camera, from
    # step `pose_refine_from` on.  0 = off: no object, launch or batch key more than without it.  Also CNC_POSE_LR.  A capture
    # through `TransformsLoader` on the GPU, one process, a bounded field; the rate has no tuned default
    pose_lr: float = 0.0
    pose_refine_from: int = 0
    # the background behind the field: "solid" = the batch's colour, as ever — no object, launch, optimizer
    # or batch key more than before; "envmap" = a learned equirectangular texture [H, 2H, 3] indexed by ray direction
    # (cnc_amd.envmap), for opaque captures without an alpha channel.  envmap_resolution is H (even, 2..64; 16: a section of
    # 1,536 bytes).  envmap_lr: the constant rate of the texture's own Adam — UNTUNED, like the default resolution: nobody has
    # run this on a real capture here.  One process only
    background: str = "solid"
    envmap_resolution: int = 16
    envmap_lr: float = 1e-2
    # floater pruning (cnc_amd.components): `Trainer.prune_floaters()` clears the connected components of
    # the occupancy grid with fewer than this many cells (the largest always stays); `python -m cnc_amd.train
    # --prune-floaters N` calls it once, after training and before the first evaluation.  0 = off: no call, launch, log line
    # or container byte differs.  There is no tuned value: nobody has chosen one on a real capture.  prune_connectivity: 6,
    # 14 or 26; 26 merges most and so removes least
    prune_floaters: int = 0
    prune_connectivity: int = 26
    # per-camera exposure compensation (cnc_amd.exposure): the learning rate of one log-gain per training
    # camera and colour channel, from step `exposure_from` on.  0 = off: no object, launch, optimizer or batch key more than
    # without it.  Also CNC_EXPOSURE_LR.  A capture through `TransformsLoader`, one process; the rate has no tuned default
    exposure_lr: float = 0.0
    exposure_from: int = 0
    # error-map pixel sampling (cnc_amd.error_map): training pixels drawn in proportion to a coarse per-image
    # map of the recent loss ([n_cams, G, G], G = error_map_resolution in 1..64) instead of uniformly, every ray's loss
    # divided by its sampling density.  False = off: no object, launch, random draw, log field or batch key differs.  Also
    # CNC_ERROR_MAP=1.  A capture through `TransformsLoader`, one process.  The uniform floor (the least share of its uniform
    # probability a pixel keeps; weights <= 1 / floor), the map's decay and the steps between rebuilds of the CDF are
    # UNTUNED defaults: nobody has run this on a real capture here
    error_map: bool = False
    error_map_resolution: int = 16
    error_map_uniform_floor: float = 0.5
    error_map_decay: float = 0.9
    error_map_refresh_every: int = 16
    # depth supervision (cnc_amd.nerfacc.losses.depth_loss): the ray loss gains this weight times the mean over
    # the batch's rays of (sum w e)^2 + depth_spread sum w e^2, e = a sample's distance from the ray's measured depth; rays
    # without a measurement count as 0.  0 = off: no batch key, launch, log field or byte differs, and depth_spread is not
    # read.  Also CNC_DEPTH_WEIGHT.  A capture through `TransformsLoader` whose frames name depth files, or the procedural
    # scene; one process.  UNTUNED: nobody has run this on a real capture here
    depth_weight: float = 0.0
    depth_spread: float = 1.0


def quantize_params(state: Dict[str, torch.Tensor], digits=13):
    """Uniform `digits`-bit quantisation of each MLP tensor (train_CNC_nerf_synthetic.py:30-50).
    Returns (quantised MB, original MB, quantised state)."""
    bits = bits_orig = 0
    out = {}
    for n, p in state.items():
        lo, hi = torch.min(p), torch.max(p)
        interval = (hi - lo) / (2 ** digits - 1) + 1e-6
        q = (p - lo) // interval
        out[n] = q * interval + lo
        bits += digits * p.numel() + 64
        bits_orig += 32 * p.numel()
    return bits / 8.0 / 1024 / 1024, bits_orig / 8.0 / 1024 / 1024, out


def get_binary_vxl_size(binary_vxl):
    """Entropy bound of the occupancy grid in MB (train_CNC_nerf_synthetic.py:53-68)."""
    with torch.no_grad():
        n = binary_vxl.numel()
        pos = torch.sum(binary_vxl)
        Pg = pos / n
        bits = pos * (-torch.log2(Pg)) + (n - pos) * (-torch.log2(1 - Pg)) + 32
    return Pg, bits.item() / 8.0 / 1024 / 1024, n


_STEP_STREAMS = {}


def reserve_streams(device):
    """The three side streams of the training step on `device` (entropy pass; its planes' half; the look-ahead batch and
    march), created — and used once — NOW, one set per process and device, at the default priority.  Why there is such a
    call: the HIP runtime deals a process's streams onto four hardware queues in the order they first appear, the null
    stream included, and two streams on one queue run one after the other.  A Trainer made first gets a queue per stream
    (null, entropy, planes, look-ahead: four of four); made after other code has used streams of its own (the encoder
    backward's two side streams in bench.py's frame loop) its planes' stream landed on the null stream's queue and the step
    took 9.7 ms instead of 7.5.  A process that trains creates its Trainer first anyway; one that does other GPU work first
    calls this at start-up."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return None
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    dev = torch.device("cuda", key)
    if key not in _STEP_STREAMS:
        streams = [torch.cuda.Stream(device=dev) for _ in range(3)]      # entropy pass, its planes' half, look-ahead
        for st in streams:
            with torch.cuda.stream(st):
                torch.zeros(1, device=dev)
        _STEP_STREAMS[key] = streams
    return _STEP_STREAMS[key]


def _run_with_modes(grad_mode, autocast_on, autocast_dtype, device_type, fn, args):
    with torch.set_grad_enabled(grad_mode), torch.autocast(device_type, dtype=autocast_dtype, enabled=autocast_on):
        return fn(*args)


def _settle(future, stream, behind) -> None:
    """A worker may still be running behind an exception that is on its way up: wait for it (its own error, if any, is
    secondary) and order `stream` after what it enqueued on the stream `behind` (None: it had no stream of its own)."""
    if future is None:
        return
    try:
        future.result()
    except BaseException:
        pass
    if behind is not None:
        stream.wait_stream(behind)


class _StreamMismatchWarningOff:
    """`with` block that holds PyTorch's accumulate-grad stream-mismatch warning off: leaves are accumulated on the main
    stream, the entropy pass produces its gradients on the side stream — intended.  The switch is process-global, so it is
    held for the duration of a train_step only and put back to what the caller had (private getter when there is one).  One
    object per Trainer, entered once per step; `enabled=False`: does nothing."""

    def __init__(self, enabled: bool):
        self._set = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None) if enabled else None
        self._before = True

    def __enter__(self):
        if self._set is not None:
            self._before = bool(getattr(torch._C, "_warn_on_accumulate_grad_stream_mismatch", lambda: True)())
            self._set(False)

    def __exit__(self, *exc):
        if self._set is not None:
            self._set(self._before)
        return False


def _dataset_has_alpha(dataset) -> bool:
    """Do the training images carry alpha below 1?  What the dataset says of itself (`has_alpha`), else a loader's RGBA
    images, looked at once (a host read: construction only); a dataset that offers neither is taken to be opaque."""
    own = getattr(dataset, "has_alpha", None)
    if own is not None:
        return bool(own)
    images = getattr(getattr(dataset, "train", None), "images", None)
    if isinstance(images, torch.Tensor) and images.dim() == 4 and images.shape[-1] == 4 and images.numel():
        top = 255 if images.dtype == torch.uint8 else 1.0
        return bool((images[..., 3] < top).any())
    return False


# The ray-side options' records: one per option that is on, which the step's phases loop over instead of
# naming an option each.  Their order: the loss terms as the ray loss adds them, the learned parameters as the update steps them
_RECORD_ORDER = ("distortion", "depth", "pose", "exposure", "envmap")


@dataclass
class LossTerm:
    """One more term of the ray loss: `weight` times the mean over the batch's rays of `per_ray(extra, data, n_rays)` on the
    samples the render just composited.  `needs`: a batch key without which the term is off for that batch."""
    name: str
    weight: float
    per_ray: Callable
    needs: Optional[str] = None


@dataclass
class LearnedParam:
    """One learned parameter with an Adam of its own.  `live`, set per step behind the backward: the ray loss reached it;
    only a live one is scanned and stepped.  `prepare_grad(data, extra)`, behind the backward of a step that uses the
    parameter, leaves in `param.grad` what the Adam descends along, or None; `after_step()` runs right behind `opt.step()`."""
    name: str
    param: Any
    opt: Any
    prepare_grad: Callable = lambda data, extra: None
    after_step: Callable = lambda: None
    live: bool = False


class Trainer:
    def __init__(self, cfg: TrainConfig, device="cuda", dataset=None):
        """Built in dependency order: device, models and dataset, the guard's decision, optimizers, gradient sinks, the
        planes' graph, streams, buckets — and then ONE look at whether the tables' Adam kernel takes what this Trainer's
        steps will hand it (`_check_table_adam`).  Construction works on a CPU device (evaluation, the codec); a training
        step does not."""
        self.cfg = c = cfg
        # world > 1: join the process group (RCCL; gloo under CNC_DIST_BACKEND) and take this rank's GPU
        self.rank, self.local_rank, self.world = cdist.init()
        self.device = torch.device(device)
        self.dp = self.world > 1 or cdist.forced()       # data-parallel control flow (forced: a one-rank group, test hook)
        self._inv_world = float(torch.tensor(1.0, dtype=torch.float32) / self.world)     # 1 / world as a float32
        on_gpu = self.device.type == "cuda"
        if self.dp and on_gpu:
            self.device = torch.device("cuda", cdist.local_device_index())
        elif on_gpu and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())     # the worker threads select it by index
        set_random_seed(c.seed)
        # ---- the options: config + environment, looked at once; what needs no model to be refused is refused here
        want = self._resolve_options()
        if int(c.prune_floaters) < 0 or c.prune_connectivity not in (6, 14, 26):
            raise ValueError("floater pruning: prune_floaters must not be negative and prune_connectivity must be 6, 14 or 26")
        # ---- models and dataset
        aabb = torch.tensor(c.aabb, device=self.device)
        self.estimator = OccGridEstimator(roi_aabb=aabb, resolution=c.grid_resolution, levels=c.grid_nlvl).to(self.device)
        self.field = NGPRadianceField_mygrid_2D3D(
            aabb=self.estimator.aabbs[-1], n_features_per_level=c.n_features, n_neurons=c.n_neurons,
            resolutions_list=c.resolutions_list, log2_hashmap_size=c.log2_hashmap_size,
            resolutions_list_2D=c.resolutions_list_2D, log2_hashmap_size_2D=c.log2_hashmap_size_2D,
            ste_binary=True, Q=10, fused_features=c.fused_features, sh_fp16_round=c.sh_fp16_round).to(self.device)
        self.context = self.build_context()
        # `dataset`: anything with fetch() / view(i) / update_num_rays(n) (LoaderDataset for real scenes); the
        # procedural scene otherwise (no dataset ships with the repository)
        self.dataset = dataset if dataset is not None else \
            SyntheticBallDataset(c.image_size, device=self.device, seed=c.seed + 1000 * self.rank)
        self.dataset.update_num_rays(c.init_batch_size)
        # ---- the ray-side options: nothing unless asked for.  Each one that is on adds ONE record (`LossTerm`, `LearnedParam`) to
        # `_terms` or `_learned`, which the step's phases loop over; enabled at the end, in one block and in the lists' order
        self._terms, self._learned, self._log_fields = [], [], {}
        self.pose_refiner = self._pose_base = self.exposure = self.envmap = self.error_map = self.on_depth_loss = None
        self.opt_pose = self.opt_exposure = self.opt_env = None
        self._pose_from, self._pose_on, self._exposure_from, self._exposure_foreground, self._depth_weight = 0, False, 0, False, 0.0
        # ---- the guarded step's decision, taken here and nowhere else: `_make_optimizers` builds the verdict's buffer from
        # it, the gradient bucket sizes its tail from it
        self._guarded = want["guarded"]
        # The reproducible mode fixes what is not a kernel by taking the schedule that has nothing to fix: the entropy pass
        # on the main stream from the main thread, behind the render forward (one order of random draws on the default
        # generator, ONE backward call whose engine adds the gradient pieces in the graph's order), no captured graph.
        self.reproducible = bool(c.reproducible)
        # ---- optimizers; per-step gradient sinks (cnc_amd._gradsink): the encoder scatters and the context heads' weight
        # gradients add into ONE buffer per parameter and pass instead of a fresh zero-filled tensor per call
        # (CNC_GRAD_SINK=0: off)
        self._make_optimizers()
        self.loss_scale = 2.0 ** 10          # GradScaler(2**10), never unscaled (train:211,361-362)
        self._make_sinks()
        # ---- the planes' half of the entropy pass as one captured graph per refresh interval (CNC_PLANES_GRAPH=0: op by op)
        self.planes_graph = None
        if on_gpu and os.environ.get("CNC_PLANES_GRAPH", "1") == "1" and not self.reproducible:
            from ._planes_graph import PlanesGraph
            self.planes_graph = PlanesGraph(self)
        # ... in the data-parallel step as well (CNC_PLANES_GRAPH_DP=0: the joint entropy pass there), so that the step a
        # multi-GPU run measures is the single-GPU step + the exchange
        self.planes_graph_dp = os.environ.get("CNC_PLANES_GRAPH_DP", "1") == "1"
        self._planes_replayed = False
        # ---- streams and host threads.  The next batch is drawn at the end of a step (`prefetch`), with its march
        # (`premarch`), on a stream of their own (`premarch = False`: the batch only, on the main stream)
        self.prefetch = self.premarch = True
        self._next_data = self._next_ready = self._fwd_enqueued = None
        streams = reserve_streams(self.device) if on_gpu else None
        self.ahead_stream = streams[2] if on_gpu else None
        # The entropy pass (context forward and backward) runs on its own stream next to the render pass — see train_step —
        # and its planes' half on a third one (`ctx_stream_2D = None`: both halves on the side stream, one after the other)
        side = on_gpu and os.environ.get("CNC_CTX_STREAM", "1") == "1" and not self.reproducible
        self.ctx_stream = streams[0] if side else None
        self.ctx_stream_2D = streams[1] if side else None
        self._warning_off = _StreamMismatchWarningOff(enabled=side)
        # ... and from its own host thread, started before the render pass (`_context_pass`): the two passes are ~300
        # launches each and the step is otherwise bound by the host issuing them one after the other.  Off = the
        # sequential schedule, which keeps the reference's order of random draws (the trajectory goldens need it).
        self.ctx_thread = side and os.environ.get("CNC_CTX_THREAD", "1") == "1"
        self._workers = {}                  # name -> one-thread pool ("context", "planes"), made at first use
        # ---- data parallel: the gradient buckets, the lagged sample count, the shared window draw
        self.bucket = None
        self.time_comm = False          # bench hook: HIP events around the wait for the gradient all-reduce
        self._comm_events = []
        if self.dp:
            plist = list(self.field.parameters()) + list(self.context.parameters())
            # ray-loss gradients (all-reduced) + ONE tail slot: this rank's sample count, so that the sum over the
            # ranks arrives with the gradients instead of through a blocking collective in the middle of the step
            # (the guarded step: one more, the range guard's trip of any rank as +inf in the sum — `_step_guard`)
            self.bucket = cdist.GradBucket(plist, tail=2 if self._guarded else 1)
            self.bucket_ctx = cdist.GradBucket(plist)      # entropy-loss gradients (replica-identical)
            self._count_host = torch.zeros(1, dtype=torch.float32)
            if on_gpu:
                self._count_host = self._count_host.pin_memory()
            self._count_pending = None                     # (event, num_rays of the step the count belongs to)
            # how often the replicas had to be re-aligned (cdist.resync_parameters, every `step_update` steps)
            self.resync = {"checks": 0, "fired": 0, "tensors": 0, "bytes": 0}
            base = self.context.rand_like

            def synced_rand_like(t):
                # the threaded schedule draws (and broadcasts) on the MAIN thread before it forks: collectives of one
                # communicator must be issued in the same order on every rank, so the worker thread issues none
                if self._ctx_rand is not None:
                    r, self._ctx_rand = self._ctx_rand, None
                    return r
                r = base(t)
                torch.distributed.broadcast(r, 0)
                return r
            self._ctx_rand = None
            self.context.rand_like = synced_rand_like
        self._check_table_adam()
        # ---- the ray-side options that are on (nothing above looks at them, none of them draws a random number)
        if c.distortion_weight > 0:
            self._add(self._terms, LossTerm("distortion", float(c.distortion_weight), self._distortion_per_ray))
        if c.background == "envmap":
            self._enable_envmap()
        if want["pose_lr"] > 0:
            self.enable_pose_refinement(want["pose_lr"], int(c.pose_refine_from))
        if want["exposure_lr"] != 0:
            self.enable_exposure_compensation(want["exposure_lr"], int(c.exposure_from))
        if want["error_map"]:
            self.enable_error_map_sampling(c.error_map_resolution, c.error_map_uniform_floor, c.error_map_decay,
                                           c.error_map_refresh_every)
        if want["depth_weight"] != 0:
            self.enable_depth_supervision(want["depth_weight"])

    # -------------------------------------------------------------------------------- the ray-side options
    def _resolve_options(self) -> dict:
        """`cfg` + the environment's overrides, each looked at once (a float option: the config's value unless it is 0, then
        the environment's), and what can be refused before a model is built, refused."""
        c, env = self.cfg, os.environ.get
        if c.background not in ("solid", "envmap"):
            raise ValueError(f"background must be 'solid' or 'envmap', got {c.background!r}")
        if c.background == "envmap":
            from .backends.envmap_backend import check_resolution
            check_resolution(c.envmap_resolution)
            self._refuse_dp("the environment-map background")
            if not (c.envmap_lr > 0):
                raise ValueError("the environment-map background: envmap_lr must be positive")
        depth_weight = float(c.depth_weight) or float(env("CNC_DEPTH_WEIGHT", "0") or 0.0)
        if depth_weight != 0:
            self._refuse_dp("depth supervision")
        return dict(guarded=bool(c.guarded_step) or env("CNC_GUARDED_STEP", "0") == "1", depth_weight=depth_weight,
                    pose_lr=float(c.pose_lr) or float(env("CNC_POSE_LR", "0") or 0.0),
                    exposure_lr=float(c.exposure_lr) or float(env("CNC_EXPOSURE_LR", "0") or 0.0),
                    error_map=bool(c.error_map) or env("CNC_ERROR_MAP", "0") == "1")

    def _refuse_dp(self, option: str) -> None:
        if self.dp:
            raise ValueError(f"{option} is not built for data-parallel training (world > 1): it would need a collective of its own")

    def _add(self, records, rec):
        """`rec` into `records`, in place of an earlier one of its name, in `_RECORD_ORDER` whatever the order of calls."""
        records[:] = sorted([o for o in records if o.name != rec.name] + [rec], key=lambda o: _RECORD_ORDER.index(o.name))

    def _own_adam(self, param, lr: float):      # of one learned ray-side parameter: a constant rate, no weight decay
        return torch.optim.Adam([param], lr=float(lr), eps=1e-15, weight_decay=0.0, fused=self.device.type == "cuda")

    def _capture_loader(self, option: str) -> TransformsLoader:
        """The training `TransformsLoader`; ValueError naming `option` where it is not one on the GPU, or under data parallel."""
        loader = getattr(self.dataset, "train", None)
        if not isinstance(self.dataset, LoaderDataset) or not isinstance(loader, TransformsLoader) \
                or self.device.type != "cuda" or not loader.cameras.is_cuda:
            raise ValueError(f"{option} needs a capture with per-camera images and poses on the GPU: a LoaderDataset over a "
                             "TransformsLoader built with device=cuda (--dataset transforms)")
        self._refuse_dp(option)
        return loader

    # -------------------------------------------------------------------------------- depth supervision
    def enable_depth_supervision(self, weight: float) -> None:
        """From the next batch drawn on, the dataset also hands out every ray's measured distance ("depth", 0 = none) and the
        ray loss gains `weight` times the batch mean of `depth_loss` on the rendered samples, with
        `cfg.depth_spread` read at every step.  `on_depth_loss`, when set, is called with (extras, target, per-ray loss)
        right after the loss is formed (diagnostics).  ValueError where that cannot work: data parallel, a weight that is
        not positive, or a dataset without depth — neither the procedural scene nor a capture whose frames name depth files."""
        self._refuse_dp("depth supervision")
        if not (weight > 0) or not (float(self.cfg.depth_spread) >= 0):
            raise ValueError("depth supervision: depth_weight must be positive and depth_spread must not be negative")
        loader = getattr(self.dataset, "train", None)
        if isinstance(self.dataset, SyntheticBallDataset):
            self.dataset.with_depth = True
        elif isinstance(self.dataset, LoaderDataset) and isinstance(loader, TransformsLoader):
            loader.depth_planes()              # read now: a capture without depth files, or one of another size, fails HERE
            loader.with_depth = True
        else:
            raise ValueError("depth supervision needs a dataset with measured depth: a LoaderDataset over a TransformsLoader "
                             "whose frames name a depth_file_path (--dataset transforms), or the procedural scene")
        self._depth_weight = float(weight)
        self._add(self._terms, LossTerm("depth", self._depth_weight, self._depth_per_ray, needs="depth"))
        self._log_fields["depth"] = lambda s: f" | depth={s['depth']:.3e}" if "depth" in s else ""

    def _depth_per_ray(self, extra, data, num_rays: int):
        """Every ray's depth loss on the samples the render just composited: one kernel, one more behind the backward's root."""
        from .nerfacc.losses import depth_loss
        per_ray = depth_loss(extra["weights"], extra["t_starts"], extra["t_ends"], data["depth"].reshape(-1).float(),
                             ray_indices=extra["ray_indices"], n_rays=num_rays, packed_info=extra["packed_info"],
                             spread=float(self.cfg.depth_spread))
        if self.on_depth_loss is not None:
            self.on_depth_loss(extra, data["depth"], per_ray)
        return per_ray

    # -------------------------------------------------------------------------------- error-map pixel sampling
    def enable_error_map_sampling(self, resolution: int = 16, uniform_floor: float = 0.5, decay: float = 0.9,
                                  refresh_every: int = 16) -> None:
        """From the next batch drawn on, the training pixels come from an `ErrorMapSampler` over the training cameras
         instead of the loader's three uniform draws: one `torch.rand` from the loader's own generator and
        one launch; the batch carries every ray's camera, pixel and weight; the mse of the ray loss becomes the weighted
        loss kernel's (behind the exposure gain, so the map sees the error the loss sees), whose per-ray errors go into
        the map; the statistics keep the unweighted mse.  Order of events: the map takes step s's errors right behind
        step s's loss forward, and where (s + 1) % refresh_every == 0 the CDF is rebuilt right behind that — before the
        draw for step s + 1 on either schedule (a draw on the look-ahead stream waits for the rebuild's event).
        `uniform_floor`, `decay` and `refresh_every` have no tuned values.  ValueError where that cannot work
        (`_capture_loader`, or a loader that does not batch over its images)."""
        from .error_map import ErrorMapSampler
        loader = self._capture_loader("error-map sampling")
        if not loader.batch_over_images:
            raise ValueError("error-map sampling draws every batch over all training images: the TransformsLoader must be "
                             "built with batch_over_images=True")
        sampler = ErrorMapSampler(len(loader), loader.HEIGHT, loader.WIDTH, resolution, uniform_floor, decay, refresh_every,
                                  device=self.device)
        self.error_map = loader.sampler = sampler          # (a batch drawn ahead of this call carries no weights: plain mse)
        self._log_fields["errmap_cover"] = lambda s: f" | errmap_cover={self.error_map.effective_fraction():.3f}"

    # -------------------------------------------------------------------------------- per-camera exposure compensation
    def enable_exposure_compensation(self, lr: float, start: int = 0) -> None:
        """From step `start` on, every step also learns one log-gain per training camera and colour channel at rate `lr`
        (DESIGN.md §4.17): the render is made without a background, `ExposureCompensation` composites the batch's colour
        and applies the camera's gain (on the foreground only when the training images carry alpha: the loader blended the
        background in behind the photograph; with the learned background the render is complete as it is and the gain
        covers all of it), the mse is taken against that, and an Adam of its own (`_own_adam`) updates `log_gain`.  Evaluation,
        the mesh and the container render at gain 1.  ValueError: `_capture_loader`'s, or a rate that is not positive."""
        from .exposure import ExposureCompensation
        loader = self._capture_loader("exposure compensation")
        if not (lr > 0):
            raise ValueError("exposure compensation: the learning rate must be positive")
        loader.with_camera_ids = True
        self.exposure = ex = ExposureCompensation(len(loader), self.device)
        self._exposure_from, self._exposure_foreground = int(start), _dataset_has_alpha(self.dataset)
        self.opt_exposure = self._own_adam(ex.log_gain, lr)
        self._add(self._learned, LearnedParam("exposure", ex.log_gain, self.opt_exposure, self._exposure_gradient))
        self._log_fields["mean_abs_log_gain"] = lambda s: f" | mean_abs_log_gain={self.exposure.mean_magnitude():.3e}"

    def write_exposures(self, path: Optional[str] = None) -> str:
        """Every training frame's effective log-gain and gain, to `<out_dir>/exposures.json` (or `path`)."""
        path = path or os.path.join(self.cfg.out_dir, "exposures.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.exposure.write(path, self.dataset.train)
        return path

    # -------------------------------------------------------------------------------- camera pose refinement
    def enable_pose_refinement(self, lr: float, start: int = 0) -> None:
        """From step `start` on, every step also learns one (omega, tau) per training camera at rate `lr` (DESIGN.md
        §4.14): the render pass hands back dL/dx per sample, `CameraPoseRefiner.accumulate` folds it per camera, an Adam of
        its own (`_own_adam`) updates `delta`, and cnc_camera_pose_apply rewrites the loader's camera table from a copy of
        the file's.  ValueError: `_capture_loader`'s, an unbounded field, or a model outside the fused training path's
        shapes (the only path with position gradients)."""
        from .field import FusedFieldForward
        from .poses import CameraPoseRefiner
        loader = self._capture_loader("pose refinement")
        if self.field.unbounded:
            raise ValueError("pose refinement needs a bounded field: position gradients are not built for the contraction")
        if not (lr > 0):
            raise ValueError("pose refinement: the learning rate must be positive")
        probe = torch.zeros((1, 3), dtype=torch.float32, device=self.device)
        with torch.enable_grad():
            on_path = FusedFieldForward.shapes_ok(self.field) and self.field._train_ok(probe, probe)
        if not on_path:
            raise ValueError("pose refinement needs the fused training forward (position gradients exist on that path "
                             "only): a model of its shapes (64 or 160 neurons), CNC_FUSED_TRAIN / CNC_FUSED_FIELD on")
        loader.with_camera_ids = True
        self.pose_refiner = CameraPoseRefiner(len(loader), self.device)
        self._pose_base = loader.cameras.clone()
        self._pose_from, self._pose_on = int(start), True
        delta = self.pose_refiner.delta
        self.opt_pose = self._own_adam(delta, lr)
        self._add(self._learned, LearnedParam("pose", delta, self.opt_pose, self._pose_gradient, self._pose_apply))

    def _pose_step(self, step: int, data) -> bool:
        """Does this step refine poses?  Stops for good, with a warning, once the range guard has switched the fused
        training forward off: no other path provides position gradients."""
        if self._pose_on and not self.field.fused_train:
            import warnings
            warnings.warn("cnc_amd: pose refinement stops here: the fused training forward was switched off (fp16 range "
                          "guard) and no other path provides position gradients; the poses keep their current values")
            self._pose_on = False
        # (a batch drawn before refinement was enabled has no camera ids)
        return self._pose_on and step >= self._pose_from and "camera_ids" in data

    def _pose_gradient(self, data, extra) -> None:
        """Behind the render backward: dL/dx of the samples -> `delta.grad`, folded per camera (`accumulate` WRITES it: what
        `_clear_grads` set to None is never added to).  None: the ray loss reached no sample."""
        g_x = extra["positions"].grad if extra is not None and extra.get("positions") is not None else None
        self.pose_refiner.delta.grad = None
        if g_x is not None:
            from .render import _as_ray_list
            self.pose_refiner.accumulate(g_x, extra, _as_ray_list(data["rays"])[0], data["camera_ids"])

    def _exposure_gradient(self, data, extra) -> None:
        """Behind the render backward: what the gains' Adam descends along (None: the ray loss did not reach the gains).
        It is the gradient with respect to the EFFECTIVE log-gains (`effective_grad`), not its centred form that autograd
        left in `log_gain.grad`: the two differ by a multiple of (1, ..., 1) per channel, the direction along which no gain
        changes, but Adam normalises per element — of the centred form it would turn the small common term into a
        full-rate step of every camera that had no ray in the batch."""
        ex = self.exposure
        if ex.log_gain.grad is not None:
            ex.log_gain.grad = ex.effective_grad

    def _pose_apply(self) -> None:
        """Behind the poses' Adam step: the loader's table rewritten from the file's poses.  The look-ahead batch of the NEXT
        step has been drawn already, from the table as the step before left it: a one-step lag, the same every run — the
        rewrite waits for that draw, and the draw after it is ordered behind this step's kernels."""
        if self._next_ready is not None:
            torch.cuda.current_stream(self.device).wait_event(self._next_ready)
        self.pose_refiner.apply(self._pose_base, out=self.dataset.train.cameras)

    def write_refined_transforms(self, path: Optional[str] = None) -> str:
        """The capture's training file with the refined poses, to `<out_dir>/transforms_refined.json` (or `path`)."""
        loader = self.dataset.train
        path = path or os.path.join(self.cfg.out_dir, "transforms_refined.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.pose_refiner.write_transforms(loader.transforms_path, path, loader.frame_ids)
        return path

    # -------------------------------------------------------------------------------- the learned background
    def _enable_envmap(self) -> None:
        """`TrainConfig.background == "envmap"`: the texture, an Adam of its own (fused, no weight decay, a
        constant rate: no schedule) and one warning when the training images carry alpha below 1 — the option is meant for
        opaque captures; with RGBA images the loader still blends its pixels with its own background colour."""
        from .envmap import EnvMapBackground
        c = self.cfg
        self.envmap = env = EnvMapBackground(c.envmap_resolution, device=self.device)
        self.opt_env = self._own_adam(env.texture, c.envmap_lr)      # (`clamp_`: to what the container's uint8 section holds)
        self._add(self._learned, LearnedParam("envmap", env.texture, self.opt_env, after_step=env.clamp_))
        if _dataset_has_alpha(self.dataset):
            import warnings
            warnings.warn("cnc_amd: background='envmap' with training images that carry alpha below 1: the loader still "
                          "blends those pixels with its own background colour, which the map will then learn; the option "
                          "is meant for opaque captures")

    def render_test_view(self, d):
        """The evaluation render of one test view `d` (`dataset.view(i)`) -> rgb [H, W, 3]: behind the batch's colour, or
        behind the learned background when there is one.  `evaluate()` and the results line's loop both use it."""
        c = self.cfg
        rgb, _, _, _ = render_image_with_occgrid_test(
            1024, self.field, self.estimator, d["rays"], near_plane=c.near_plane, render_step_size=c.render_step_size,
            render_bkgd=d["color_bkgd"], cone_angle=c.cone_angle, alpha_thre=c.alpha_thre, background=self.envmap)
        return rgb

    def build_context(self):
        """The context models of this configuration (train:221-241).  Their vertex tables draw from the CPU
        generator (randperm of the dense levels, utils_bpp_acc.py:312), so a caller that wants a particular
        draw seeds, calls this and assigns the result to `self.context` — then `build_optimizers()` and `build_sinks()`,
        in that order; each of the two looks at the new models (`_check_table_adam`)."""
        c = self.cfg
        return CNC_context_models(
            num_dim=3, resolutions_list=c.resolutions_list, resolutions_list_2D=c.resolutions_list_2D,
            log2_hashmap_size=c.log2_hashmap_size, log2_hashmap_size_2D=c.log2_hashmap_size_2D,
            n_features=c.n_features, sample_num=c.sample_num, max_context_layer_num=c.max_context_layer_num,
            ste_binary=True, Q=10, Pg_level=c.Pg_level, Pg_level_2D=c.Pg_level_2D, Rb=c.grid_resolution,
            step_update=c.step_update, skip_levels_3D=c.skip_levels_3D, skip_levels_2D=c.skip_levels_2D,
            device=self.device,
            dimension_wise_resolution=c.dimension_wise_resolution or c.resolutions_list[-1])

    def build_sinks(self):
        """The step's gradient sinks for the CURRENT field and context models (a caller that replaces `self.context` —
        see `build_context` — calls `build_optimizers()` and this again: the entropy pass's sink holds one slot per
        context-head parameter, and the planes' graph refuses to record without them)."""
        self._make_sinks()
        self._check_table_adam()

    def _make_sinks(self):
        self.sink_render = self.sink_ctx = None
        if self.device.type == "cuda" and os.environ.get("CNC_GRAD_SINK", "1") == "1":
            tables = [e.params for e in self.field.mlp_base._encoders()]
            self.sink_render = _gradsink.GradSink(tables, [])
            self.sink_ctx = _gradsink.GradSink(tables, list(self.context.parameters()))

    def build_optimizers(self):
        """Both Adam groups and their chained schedules (train:257-297), for the CURRENT field and context models."""
        self._make_optimizers()
        self._check_table_adam()

    def _make_optimizers(self):
        c = self.cfg
        # one kernel per parameter list instead of the ~9 passes of the foreach implementation (0.8 -> 0.2 ms per step)
        one_pass = self.device.type == "cuda"
        # the four tables as a parameter group of their own (same hyper-parameters, same schedule): what `_table_adam` steps
        tables = [e.params for e in self.field.mlp_base._encoders()]
        tids = {id(p) for p in tables}
        self._tables, self._table_ids = tables, tids
        rest = [p for p in self.field.parameters() if id(p) not in tids]
        self.opt = torch.optim.Adam([{"params": rest}, {"params": tables}], lr=c.lr, eps=1e-15, weight_decay=c.weight_decay,
                                    fused=one_pass)
        self.opt2 = torch.optim.Adam(self.context.parameters(), lr=c.lr, eps=1e-15, fused=one_pass)
        # The tables' update reads the gradient pieces where they lie (one kernel instead of clone + multi-tensor add + the
        # library's Adam over the sum; CNC_TABLE_ADAM=0 or `self.fused_table_adam = False`: pieces flushed into `.grad`,
        # library step).  Data parallel too: the all-reduced sum is one more piece, the mean is taken inside the kernel.
        self.table_adam = None
        if one_pass and os.environ.get("CNC_TABLE_ADAM", "1") == "1" and all(t.numel() % 4 == 0 for t in tables):
            self.table_adam = _table_adam.TableAdam(self.opt, tables, self.field.mlp_base._encoders())
        self.fused_table_adam = self.table_adam is not None
        # the guarded step: the verdict's buffer, seeded with the step count of the optimizer as it stands
        self.step_guard = None
        if self._guarded:
            if not one_pass:
                raise RuntimeError("the guarded step needs a GPU: it hands the verdict to the library's fused Adam, the only "
                                   "form that takes a device-side `found_inf`")
            b1, b2 = self.opt.param_groups[1]["betas"]
            self.step_guard = _step_guard.StepGuard(self.device, b1, b2, self._table_steps_taken())

        def sched(o):
            return torch.optim.lr_scheduler.ChainedScheduler([
                torch.optim.lr_scheduler.LinearLR(o, start_factor=0.01, total_iters=c.warmup_iters),
                torch.optim.lr_scheduler.MultiStepLR(o, milestones=list(c.milestones), gamma=0.33)])
        self.sched, self.sched2 = sched(self.opt), sched(self.opt2)

    def _table_steps_taken(self) -> int:
        """The tables' step count as the optimizer's state has it (a synchronisation: construction and state loads only)."""
        st = self.opt.state.get(self.opt.param_groups[1]["params"][0], {})
        return int(float(st["step"])) if len(st) else 0

    def _check_table_adam(self) -> None:
        """Once per construction or rebuild, not in the middle of a step: what cnc_table_adam would refuse of the pieces this
        Trainer's schedules can hand it — then the steps take the `.grad` path (`fused_table_adam = False`), with one
        warning."""
        ta = self.table_adam
        if ta is None or not self.fused_table_adam:
            return
        # the one piece that is not table-sized: the 3-D table's finest level out of the planes' graph (_planes_graph.capture)
        off3 = getattr(self.context, "_off3_host", None)
        rows = {} if off3 is None or len(off3) < 2 else {id(ta.tables[0]): [(int(off3[-2]), int(off3[-1]))]}
        # the most pieces a step of THIS Trainer hands over for one table.  Single process: `.grad`, the render sink, the
        # entropy sink, the planes' graph; data parallel: `.grad` (the bucket: the render sink is flushed into it), the
        # entropy pass's returned gradient, the entropy sink, the planes' graph
        graph = self.planes_graph is not None
        if self.dp:
            pieces = 1 + 1 + (self.sink_ctx is not None) + (graph and self.planes_graph_dp)
        else:
            pieces = 1 + (self.sink_render is not None) + (self.sink_ctx is not None) + graph
        why = ta.refusal(rows, max_pieces=pieces)
        if why is None and self.bucket is not None:
            tids = {id(p) for p in ta.tables}
            for b in (self.bucket, self.bucket_ctx):
                if any(v.data_ptr() % 16 for p, v in zip(b.params, b.views) if id(p) in tids):
                    why = "a table's slice of the gradient bucket is not 16-byte aligned"
        if why is not None:
            import warnings
            warnings.warn(f"cnc_amd: the tables' Adam kernel is off, their gradients go through `.grad` ({why})")
            self.fused_table_adam = False

    def load_optimizer_state(self, opt_state, opt2_state=None) -> None:
        """`load_state_dict` of the field's (and the context models') optimizer.  The tables' kernel takes its bias corrections
        from a host mirror of the optimizer's step count: re-read here."""
        self.opt.load_state_dict(opt_state)
        if opt2_state is not None:
            self.opt2.load_state_dict(opt2_state)
        if self.table_adam is not None:
            self.table_adam.resync()
        if self.step_guard is not None:
            self.step_guard.seed(self._table_steps_taken())        # the running products b^t restart from the loaded count

    # -------------------------------------------------------------------------------- training: the entropy pass
    def _submit(self, worker: str, fn, *args):
        """`fn(*args)` on the one-thread pool `worker` (made at first use) under the SUBMITTING thread's grad and autocast
        modes: both are thread-local in PyTorch and a pool thread starts from the defaults."""
        pool = self._workers.get(worker)
        if pool is None:
            from concurrent.futures import ThreadPoolExecutor
            pool = self._workers[worker] = ThreadPoolExecutor(max_workers=1, thread_name_prefix="cnc-" + worker)
        kind = self.device.type
        return pool.submit(_run_with_modes, torch.is_grad_enabled(), torch.is_autocast_enabled(kind),
                           torch.get_autocast_dtype(kind), kind, fn, args)

    def _entropy_forward(self, step: int, stream_2D=None, planes=None):
        """The entropy loss forward with the entropy pass's sink active on the calling thread -> (bits per parameter, MB)."""
        e = self.field.mlp_base
        with _gradsink.activate(self.sink_ctx):
            return self.context.forward_binary_vxl_mixPg_3D2D(
                e.encoding_xyz, e.encoding_xy, e.encoding_xz, e.encoding_yz, self.estimator.binaries,
                sample_num=None, step=step, sync_MB=False, stream_2D=stream_2D, planes=planes)

    def _planes_thread_step(self, step: int, params) -> bool:
        """The planes' half of this step's entropy pass runs apart from the 3-D half (its own root, its own thread)."""
        c = self.cfg
        # (data parallel, `params` given: the 3-D half's gradients are returned to the caller, the planes' half leaves its own
        # in the sink and in the graph's static tensors as in a single-process step — both are added behind the collective)
        # On by default since round 6 (CNC_PLANES_GRAPH_DP=0 switches it off): RCCL at one rank (tests/test_gpu_rccl.py), 2 and
        # 8 ranks over gloo on one device (tests/test_gpu_multi.py: bit-identical replicas across five refreshes).
        if params is not None and not self.planes_graph_dp:
            return False
        return (self.planes_graph is not None and self.ctx_stream_2D is not None and c.lmbda > 0
                and step > c.step_update and torch.is_grad_enabled())

    def _planes_graph_step(self, step: int, params) -> bool:
        """... as a replay of the recorded graph: every such step but the occupancy-refresh ones."""
        return self._planes_thread_step(step, params) and step % self.cfg.step_update != 0

    def _planes_job(self, after, step: int, refresh: bool) -> None:
        """On the planes' thread: the planes' half on the planes' stream, ordered after the event `after` — one graph launch.
        On an occupancy-refresh step (`refresh`) first rebuild what that half is built on (vote plan, projections, vertex
        lists: host round trips on the planes' stream only) and, unless the grid did not change and the recorded graph still
        stands, run it op by op — next to the 3-D half, which needs none of it, instead of in front of it on one thread (the
        entropy pass's thread was the long pole of a refresh step: 14 ms against 7.5; 12 this way).  The graph for the steps
        that follow is recorded by the next step, in front of its fork: recording it here, behind this job, was built too —
        the 2.5 ms of host time it takes moved from the next step into this one (whose long pole is this thread), the sum did
        not change."""
        torch.cuda.set_device(self.device)
        with torch.cuda.stream(self.ctx_stream_2D), _gradsink.activate(self.sink_ctx):
            self.ctx_stream_2D.wait_event(after)
            if refresh:
                self.context.refresh_planes(self.estimator.binaries, step, self.field.mlp_base.encoding_xy.params)
                if not self.planes_graph.ready():
                    self.planes_graph.run_eager()
                    return
            self.planes_graph.replay()

    def _ensure_planes_graph(self, step: int, params) -> None:
        """Capture the planes' graph if this step replays one and the structures it was recorded for are gone (the first
        step behind an occupancy refresh).  On the thread that calls it, with NO other thread of the step running: a
        capture puts the device's default random generator into capture mode for its duration, and a draw from another
        thread (the sampler's jitter) fails meanwhile — so train_step calls this before it forks the entropy pass off."""
        if self._planes_graph_step(step, params) and not self.planes_graph.ready():
            try:
                with torch.cuda.stream(self.ctx_stream_2D), _gradsink.activate(self.sink_ctx):
                    self.planes_graph.capture()
            except Exception as e:       # an operation the runtime cannot record: the step falls back to the op-by-op pass
                if os.environ.get("CNC_PLANES_GRAPH_STRICT", "0") == "1":      # (the tests: a silent fallback there would
                    raise                                                       # hide a capture regression)
                import warnings
                warnings.warn(f"cnc_amd: capturing the planes' graph failed ({e}); continuing without it")
                self.planes_graph = None

    def _context_pass(self, step: int, fork, params=None):
        """Entropy loss forward + backward on the side stream (from whichever host thread calls it), ordered after the
        event `fork` of the main stream.  `params` = None: the gradient is accumulated into `.grad`; a parameter list:
        it is RETURNED (torch.autograd.grad, None for parameters the entropy loss does not reach) and `.grad` is left
        alone — the data-parallel step keeps the ray-loss gradient there for its all-reduce.
        Returns (bits_per_param, estimated MB, event that marks the end of the pass, gradients or None)."""
        c, side = self.cfg, self.ctx_stream
        torch.cuda.set_device(self.device)
        side.wait_event(fork)
        with torch.cuda.stream(side):
            # The planes' half as ONE graph launch (cnc_amd._planes_graph), between occupancy refreshes.  Captured at the
            # first step after a refresh (by train_step already when this is the worker thread).
            pg, planes, job = self.planes_graph, None, None
            self._planes_replayed = False
            self._ensure_planes_graph(step, params)
            if self._planes_thread_step(step, params):     # (asked behind the capture: a failed one switches the graph off)
                # The graph launch itself is ~2 ms of HOST time (the runtime enqueues the ~110 nodes one by one, outside the
                # interpreter lock): from a thread of its own, so that this one goes straight on to the 3-D half.  An
                # occupancy-refresh step: rebuilt and run op by op over there.
                refresh = not self._planes_graph_step(step, params)
                job = self._submit("planes", self._planes_job, side.record_event(), step, refresh)
                # the bits join the totals below, behind the backward
                planes = (None, sum(t.params.numel() for t in self.field.mlp_base._encoders()[1:]) if refresh else pg.n_params)
                self._planes_replayed = True
            # the planes' half of the pass on a stream of its own, next to the 3-D half (both directions: autograd runs a
            # node's backward on its forward's stream)
            # (Back-propagating the planes' share of the loss as soon as their forward is enqueued — a second backward call,
            # before the 3-D half is launched — was built and measured: 8.25 -> 8.95 ms.  The first half of the step is bound
            # by the two host threads' launches, and the extra call sits in front of the 3-D forward's.)
            try:
                bits_per_param, mb = self._entropy_forward(step, stream_2D=self.ctx_stream_2D, planes=planes)
                # issued from the side stream: the root gradient of a backward call is created on the ambient stream and
                # every node waits for it
                root = c.lmbda * bits_per_param * self.loss_scale
                grads = None
                if params is None:
                    root.backward()
                else:
                    grads = torch.autograd.grad(root, params, allow_unused=True)
            except BaseException:
                # the planes' job writes the sink and the graph's static gradients: never leave it running behind the error
                _settle(job, side, self.ctx_stream_2D)
                raise
            if job is not None:
                job.result()                               # the graph launch has been enqueued (and did not fail)
            if self.ctx_stream_2D is not None:
                side.wait_stream(self.ctx_stream_2D)       # the planes' backward kernels: part of what `done` marks
            if planes is not None:                         # the reported totals: + the planes' bits (no gradient here)
                n_all = sum(t.params.numel() for t in self.field.mlp_base._encoders())
                bits_per_param = bits_per_param.detach() + pg.step_bits / n_all
                mb = mb + pg.step_bits * (1.0 / 8388608.0)         # / 8 / 1024 / 1024 (a power of two: same value)
            done = side.record_event()
        return bits_per_param, mb, done, grads

    def _join_entropy_pass(self, result):
        """Order the main stream after the entropy pass; its outputs were allocated on the side stream."""
        bits_per_param, mb, done, grads = result
        main = torch.cuda.current_stream(self.device)
        main.wait_event(done)
        for t in (bits_per_param, mb) + tuple(g for g in (grads or ()) if g is not None):
            if isinstance(t, torch.Tensor):
                t.record_stream(main)
        return bits_per_param, mb, grads

    # -------------------------------------------------------------------------------- training: the step, phase by phase
    def train_step(self, step: int, want_stats: bool = True) -> Optional[Dict[str, float]]:
        """One optimisation step.  `want_stats=False` leaves mse / psnr / bpp / embed_bits_MB out of the result
        (reading them back is a device->host sync per step; the reference only looks at them every 200 steps,
        train:368-381) — `n_rendering_samples` and `num_rays` are always there.

        The phases: take the batch, refresh (occupancy, range guard, broadcast), clear the sinks, start the entropy pass
        (the threaded schedule: now; the other two: behind the render forward, `_backward_*`), render forward and loss,
        backward and gradient assembly, the guard's verdict, update, stats.  The schedule is chosen per step from
        `ctx_thread` / `ctx_stream` / `cfg.lmbda`."""
        if self.device.type != "cuda":
            raise RuntimeError(f"Trainer.train_step needs a GPU: this Trainer is on {self.device}, and the step's kernels "
                               "have no CPU form (a CPU Trainer evaluates, encodes and decodes only)")
        if self.reproducible and not _repro.explicitly_enabled():
            with _repro.reproducible(True):         # process-wide for the step: the backward kernels run on autograd's thread
                return self.train_step(step, want_stats)
        c = self.cfg
        self.field.train(); self.estimator.train(); self.context.train()
        self._planes_replayed = False       # (set by this step's entropy pass if the planes' half runs apart from it)
        # do the tables go through their Adam kernel this step (`fused_table_adam` is settable between steps): asked once
        tables_fused = self.table_adam is not None and self.fused_table_adam
        data = self._take_batch()
        self._refresh(step)
        for sink in (self.sink_render, self.sink_ctx):      # before either pass forks off: both are ordered after this
            if sink is not None:
                sink.zero()
        ctx_future = None
        with self._warning_off:
            try:
                if self.ctx_thread and self.ctx_stream is not None and c.lmbda > 0:
                    ctx_future = self._fork_entropy_pass(step)
                return self._render_and_update(step, want_stats, data, ctx_future, tables_fused)
            except BaseException:
                # Never leave the worker running behind an exception: it writes `.grad` and reads the tables.  Order the main
                # stream after whatever it enqueued, and drop the window draw that was made for it.
                _settle(ctx_future, torch.cuda.current_stream(self.device), self.ctx_stream)
                if self.bucket is not None:
                    self._ctx_rand = None
                raise

    def _take_batch(self):
        """The batch: drawn at the end of the step before (`_prefetch`), while that step's backward kept the GPU busy."""
        data, self._next_data = self._next_data, None
        if data is None:
            return self.dataset.fetch()
        if self._next_ready is not None:          # drawn on the look-ahead stream: join it, hand the tensors over
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._next_ready)
            self._next_ready = None
            for v in data.values():
                for t in (v if isinstance(v, tuple) else (v,)):
                    if isinstance(t, torch.Tensor) and t.is_cuda:
                        t.record_stream(cur)
        return data

    def _refresh(self, step: int) -> None:
        c = self.cfg
        self.estimator.update_every_n_steps(
            step=step, occ_eval_fn=lambda x: self.field.query_density(x) * c.render_step_size,
            occ_thre=1e-2, n=c.step_update)
        if step % c.step_update == 0 and step > 0:
            # the occupancy refresh has just synchronised the host: the moment to read the fused training forward's fp16
            # range guard (a saturated activation since the last look: the gradient pass leaves that kernel, with a warning)
            self.field.check_range_guard()
        if self.dp and step % c.step_update == 0:
            cdist.broadcast_module_buffers(self.estimator, ["occs", "binaries"])

    def _clear_grads(self, bucket=None) -> None:
        """Before a backward, at each schedule's own point: `.grad` = None, or (data parallel) its slice of the zeroed `bucket`."""
        bucket = self.bucket if bucket is None else bucket
        if bucket is None:
            self.opt.zero_grad(set_to_none=True)
            self.opt2.zero_grad(set_to_none=True)
            for rec in self._learned:       # every one: none of their gradients is read before this step's backward or
                rec.opt.zero_grad(set_to_none=True)                    # `prepare_grad` has written it anew
        else:
            bucket.zero()
            bucket.bind(force=True)

    def _fork_entropy_pass(self, step: int):
        """The threaded schedule: the entropy pass starts NOW, from a second host thread -> its future."""
        # The ray loss and the entropy loss share nothing but the parameters and the occupancy grid (just updated): the
        # entropy pass runs on the side stream next to the whole render pass.  What both passes read through a cache — the
        # sign bit planes of the tables — is made current on the main stream first; gradients are cleared before either
        # backward.  Data parallel: the worker returns its gradient instead of accumulating it (`.grad` = the bucket that is
        # all-reduced), and the window draw that every rank must share is made and broadcast here, on the main thread.
        for enc in self.field.mlp_base._encoders():
            if enc.ste_binary and enc.bitplane:
                enc._bit_plane(enc.params)
        self._clear_grads()
        params = None
        if self.bucket is not None:
            params = self.bucket.params
            self._ctx_rand = None
            self._ctx_rand = self.context.rand_like(self.context.utils_rand)
            self._ctx_rand.record_stream(self.ctx_stream)      # allocated here, read by the side stream
        self._ensure_planes_graph(step, params)
        return self._submit("context", self._context_pass, step, torch.cuda.current_stream(self.device).record_event(), params)

    def _prefetch(self, step: int = -1) -> None:
        """The NEXT step's batch, drawn now: the ray count it depends on has just been set (`update_num_rays`, from this
        step's sample count), this thread would otherwise wait for the entropy pass, and the ~25 small kernels of the draw
        run in the shadow of this step's backward instead of at the head of the next step, in front of everything (the
        entropy pass — the longer of the two — could not start before them: 0.5 ms).  The dataset draws from its own
        generator: the sequence of batches is the one `fetch()` at the top of each step produces.  Single-process steps
        only (data parallel: the ray count of the next step is known at ITS start, `_lagged_sample_count`)."""
        if not self.prefetch or self.dp:
            return
        c, pre = self.cfg, self.ahead_stream
        if pre is None:
            self._next_data = self.dataset.fetch()
            return
        # ... on the look-ahead stream, and with the batch also its MARCH (OccGridEstimator.premarch): rays and occupancy grid
        # are all the march reads, so the next step's two traversal passes and the host round trip for its sample count run
        # here, next to this step's backward, instead of at the head of the next step's render pass — the step's critical
        # chain.  Not in front of a refresh step: it replaces the grid.
        # (ordered after this step's render FORWARD on the main stream — the march that read `binaries`, the coarse occupancy
        # words computed lazily by whichever stream marches first; today a host sync earlier in the step already covers them —
        # not after its backward, which is what this runs next to)
        if self._fwd_enqueued is not None:
            pre.wait_event(self._fwd_enqueued)
        with torch.cuda.stream(pre):
            data = self.dataset.fetch()
            if self.premarch and step >= 0 and (step + 1) % c.step_update != 0:
                from .render import _as_ray_list
                rays, _ = _as_ray_list(data["rays"])
                self.estimator.premarch(rays.origins, rays.viewdirs, near_plane=c.near_plane, render_step_size=c.render_step_size,
                                        stratified=True, cone_angle=c.cone_angle)
            self._next_ready = pre.record_event()
        self._next_data = data

    def _lagged_sample_count(self, num_rays_now: int, n_samples: int) -> None:
        """Data-parallel ray budget without a collective of its own.  The reference resizes the next batch from this
        step's sample count (train:340-344); with N ranks the count that matters is the mean over the ranks, and asking
        for it here would put a blocking all-reduce + host sync between the render forward and its backward on every
        rank.  Instead this rank's count rides in the tail slot of the gradient bucket; the sum comes back with the
        gradients and is read at the NEXT step, right here — after the march has synchronised the host anyway — and
        resizes the batch after that: num_rays[k+1] = num_rays[k-1] * target / mean_count[k-1].  Same fixed point
        (target / samples-per-ray), one step later; every rank computes it from the same all-reduced number."""
        c = self.cfg
        if self._count_pending is not None:
            ev, rays_then = self._count_pending
            ev.synchronize()                        # long since complete: the step before this one
            mean = float(self._count_host[0]) / self.world
            if c.target_sample_batch_size > 0 and mean >= 1.0:
                self.dataset.update_num_rays(int(rays_then * (c.target_sample_batch_size / mean)))
        self._count_pending = None
        self.bucket.tail[:1].fill_(float(n_samples))    # enqueued before the backward; the bucket is zeroed before this

    def _render_and_update(self, step, want_stats, data, ctx_future, tables_fused):
        """The step behind its fork: render forward, ray loss, backward, the ray-side gradients, verdict, update, stats."""
        c, num_rays = self.cfg, len(data["pixels"])
        refine = self._pose_step(step, data)
        gained = self.exposure is not None and step >= self._exposure_from and "camera_ids" in data
        terms = [t for t in self._terms if t.needs is None or t.needs in data]     # the extra loss terms of this batch
        rgb, acc, n_samples, extra, range_guard = self._render_forward(data, refine, gained, with_samples=bool(terms))
        if not self.dp:
            if n_samples == 0:
                if ctx_future is not None:
                    torch.cuda.current_stream(self.device).wait_event(ctx_future.result()[2])
                if self.error_map is not None:
                    self._error_map_step(step, data, None)      # nothing to observe; a rebuild that is due is still made
                return None
            if c.target_sample_batch_size > 0:
                self.dataset.update_num_rays(int(num_rays * (c.target_sample_batch_size / float(n_samples))))
        # world > 1: no rank leaves the step (the collective below must be entered by everyone; a rank without samples
        # adds a zero ray gradient), and the ray budget follows the all-reduced count of the step before
        ray_loss, scalars = self._ray_loss(step, data, rgb, acc, extra, terms, gained)
        if self.bucket is None:
            bpp, mb, table_pieces = self._backward_single(step, ray_loss, ctx_future, tables_fused)
        else:
            bpp, mb, table_pieces = self._backward_dp(step, ray_loss, ctx_future, tables_fused, num_rays, n_samples, range_guard)
        for rec in self._learned:           # live: the ray loss reached the parameter (`_clear_grads` cleared every one)
            if {"pose": refine, "exposure": gained}.get(rec.name, True):
                rec.prepare_grad(data, extra)
            rec.live = rec.param.grad is not None
        if self.step_guard is not None:
            self._verdict([scalars["mse"], bpp] + [scalars[t.name] for t in terms], range_guard, tables_fused)
        self._update(step, table_pieces, tables_fused)
        if not want_stats:
            return {"n_rendering_samples": n_samples, "num_rays": num_rays}
        return self._stats(scalars, bpp, mb, n_samples, num_rays)

    def _render_forward(self, data, refine: bool, gained: bool, with_samples: bool):
        """The render forward -> (rgb, opacity, sample count, extras, the range guard's words for the verdict or None)."""
        c, rays, bkgd = self.cfg, data["rays"], data["color_bkgd"]
        # exposure compensation composites the batch's colour itself, behind this render
        if gained and self.envmap is None:
            bkgd = None
        # (`background=`: the learned background, when there is one, takes the place of the batch's colour; None = as ever)
        own = dict(position_grad=True) if refine else dict(with_samples=with_samples)
        with _gradsink.activate(self.sink_render):
            rgb, acc, depth, n_samples, extra = render_image_with_occgrid(
                self.field, self.estimator, rays, near_plane=c.near_plane, render_step_size=c.render_step_size,
                render_bkgd=bkgd, cone_angle=c.cone_angle, alpha_thre=c.alpha_thre, return_extra=True,
                background=self.envmap, **own)
        self._fwd_enqueued = torch.cuda.current_stream(self.device).record_event()
        # (the guarded step judges THIS forward's guard words on the device: whether the forward just enqueued was the
        # fused one is asked before the poll below can switch it off)
        ff = self.field._field_fused
        guard_live = self.step_guard is not None and bool(ff) and self.field.fused_train \
            and ff._buffers is not None and getattr(ff, "_train_calls", False)
        # the fused training forward's fp16 range guard, every step and without a wait: the words of the step before have
        # arrived by now (the sampler has synchronised the host since), this step's are sent on their way
        self.field.poll_range_guard()
        self.field.snapshot_range_guard()
        range_guard = (ff._buffers["guard"], self.field._guard_seen, ff._pack_id) if guard_live else None
        return rgb, acc, n_samples, extra, range_guard

    def _ray_loss(self, step, data, rgb, acc, extra, terms, gained: bool):
        """gain -> weighted or plain mse -> `terms`.  -> (what is back-propagated, the loss scalars by name: "mse", the terms)."""
        pixels = data["pixels"]
        if gained:
            # the pixel the loss sees: the camera's gain on the render — the learned background's output is complete as it
            # is; otherwise the batch's colour goes in here, under the gain or behind it (`enable_exposure_compensation`)
            if self.envmap is not None:
                rgb = self.exposure(rgb, data["camera_ids"])
            else:
                rgb = self.exposure(rgb, data["camera_ids"], acc, data["color_bkgd"],
                                    gain_background=not self._exposure_foreground)
        if self.error_map is not None and "ray_weight" in data:
            # error-map sampling: every ray's squared error over its sampling density, so that the gradient's expectation is
            # the uniform draw's; the per-ray errors go into the map, and their mean — the unweighted mse — keeps feeding
            # the statistics (and the verdict), so that a logged PSNR means what it meant
            from .error_map import weighted_mse
            ray_loss, err = weighted_mse(rgb, pixels, data["ray_weight"])
            mse = err.mean()
            self._error_map_step(step, data, err)
        else:
            ray_loss = mse = F.mse_loss(rgb, pixels)
        # + weight times each term's mean over this rank's rays, like the mse (`LossTerm`)
        scalars = {"mse": mse}
        for t in terms:
            scalars[t.name] = t.per_ray(extra, data, len(pixels)).sum() / float(max(len(pixels), 1))
            ray_loss = ray_loss + t.weight * scalars[t.name]
        return ray_loss, scalars

    def _stats(self, scalars, bpp, mb, n_samples, num_rays):
        """The step's scalars in one device->host copy -> the result dict: the fixed keys, then one per loss term."""
        mse, names = scalars["mse"], [n for n in scalars if n != "mse"]
        mse_f, bpp_f, mb_f, *rest = torch.stack([mse.detach(), torch.as_tensor(bpp, device=mse.device).detach().float(),
                                                 torch.as_tensor(mb, device=mse.device).detach().float()]
                                                + [scalars[n].detach() for n in names]).tolist()
        return {"mse": mse_f, "psnr": -10.0 * math.log10(max(mse_f, 1e-12)), "bpp": bpp_f, "embed_bits_MB": mb_f,
                "n_rendering_samples": n_samples, "num_rays": num_rays, **dict(zip(names, rest))}

    def _error_map_step(self, step: int, data, err) -> None:
        """Step `step`'s share of the error map, on the main stream right behind the loss forward: its rays' errors into the
        map, then — where (step + 1) % refresh_every == 0 — the CDF rebuilt from the map that includes them.  Both are
        enqueued before the next batch is drawn, whether `_prefetch` draws it during this step's backward (its stream waits
        for the rebuild's event, `ErrorMapSampler.draw`) or `fetch()` at the top of the next step: one sequence of batches."""
        em = self.error_map
        if err is not None and "ray_weight" in data:
            px, py = data["pixel_xy"]
            em.observe(data["camera_ids"], px, py, err)
        if (step + 1) % em.refresh_every == 0:
            em.refresh()

    @staticmethod
    def _distortion_per_ray(extra, data, num_rays: int):
        """Every ray's distortion loss on the samples the render just composited: one kernel, one more behind the backward."""
        from .nerfacc.losses import distortion
        return distortion(extra["weights"], extra["t_starts"], extra["t_ends"], ray_indices=extra["ray_indices"],
                          n_rays=num_rays, packed_info=extra["packed_info"])

    @staticmethod
    def _distortion(extra, num_rays: int):
        """Its mean over the batch's rays (`with_samples` extras)."""
        return Trainer._distortion_per_ray(extra, None, num_rays).sum() / float(max(num_rays, 1))

    def _backward_single(self, step, ray_loss, ctx_future, tables_fused):
        """Single process: both backward passes in this step's schedule -> (bits per parameter, MB, the tables' pieces)."""
        c = self.cfg
        bpp, mb = 0.0, 0.0
        if ctx_future is not None:
            (ray_loss * self.loss_scale).backward()
            self._prefetch(step)
            bpp, mb, _ = self._join_entropy_pass(ctx_future.result())
        elif self.ctx_stream is not None and c.lmbda > 0 and ray_loss.requires_grad:
            # The sequential schedule of the same idea (one host thread; the reference's order of random draws):
            #   render backward (main stream: few launches, GPU-heavy)
            #   || context forward + context backward (side stream: ~250 launches, host-bound forward)
            # The side stream forks BEFORE the render backward is enqueued; its host-side syncs (window bounds,
            # nonzero) wait for the side stream only.
            self._clear_grads()
            fork = torch.cuda.current_stream(self.device).record_event()
            (ray_loss * self.loss_scale).backward()
            bpp, mb, _ = self._join_entropy_pass(self._context_pass(step, fork))
        else:
            # The plain schedule: one stream, one thread, ONE backward call over the joint loss (the reproducible mode and the
            # trajectory goldens are this)
            loss = ray_loss
            if c.lmbda > 0:
                bpp, mb = self._entropy_forward(step)
                loss = loss + c.lmbda * bpp
            self._clear_grads()
            (loss * self.loss_scale).backward()
        # both passes are joined to this stream: what their kernels added to the sinks goes to `.grad`, once — or, for
        # the tables, straight into their Adam update (`_table_adam`: the pieces are summed there, in this order)
        table_pieces = {} if tables_fused else None
        for sink in (self.sink_render, self.sink_ctx):
            if sink is not None:
                sink.flush(table_pieces=table_pieces)
        if self._planes_replayed:
            self.planes_graph.flush(table_pieces=table_pieces)       # what autograd returned inside the planes' graph
        return bpp, mb, table_pieces

    def _backward_dp(self, step, ray_loss, ctx_future, tables_fused, num_rays, n_samples, range_guard):
        """Data parallel: the backward passes around the ray-loss gradient's all-reduce -> what `_backward_single` returns."""
        # The ray loss differs per rank, the entropy loss does not (same tables, same window draw on every rank): so only
        # the ray-loss gradient is exchanged, and its all-reduce runs on the communicator's stream WHILE the entropy pass is
        # still under way.  The entropy gradient is equal across ranks only up to the order of its float atomics (~1e-9
        # relative), so the replicas are compared at every occupancy refresh and re-aligned to rank 0 where they differ
        # (`_update`).
        c, sg = self.cfg, self.step_guard
        A, B = self.bucket, self.bucket_ctx
        bpp, mb = 0.0, 0.0
        if ctx_future is None:
            if c.lmbda > 0:
                bpp, mb = self._entropy_forward(step)
            self._clear_grads()
        self._lagged_sample_count(num_rays, n_samples)
        if ray_loss.requires_grad:          # a rank whose rays met no sample has nothing to add (its peers do): the
            (ray_loss * self.loss_scale).backward()     # collective below must still be entered by everyone
        if self.sink_render is not None:
            self.sink_render.flush()               # `.grad` = the bucket's views: the encoder scatters join it here
        if sg is not None:
            # this rank's range-guard trip as +inf (else 0) in the second tail slot: every rank reads it in the sum
            sg.scan((), range_guard=range_guard, poison=A.tail[1:2])
        work = A.allreduce(average=False, async_op=True)
        ctx_grads = None
        if ctx_future is not None:
            bpp, mb, ctx_grads = self._join_entropy_pass(ctx_future.result())
        elif c.lmbda > 0:
            self._clear_grads(B)
            (c.lmbda * bpp * self.loss_scale).backward()
            if self.sink_ctx is not None:
                self.sink_ctx.flush()              # into `.grad` = B's views
        if work is not None:
            if self.time_comm:      # how long the compute stream stalls for the collective (what was NOT hidden
                e0 = torch.cuda.Event(enable_timing=True)        # behind the entropy pass)
                e0.record()
            work.wait()
            if self.time_comm:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                self._comm_events.append((e0, e1))
        # the summed sample count goes to the host behind the collective; nobody waits for it before the next step
        self._count_host.copy_(A.tail[:1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._count_pending = (ev, num_rays)
        # The mean of the ray-loss gradient + the entropy gradient, in the bucket.  The tables' share, when their kernel steps
        # them, stays the SUM the collective left: it is the first piece of their Adam update, times 1 / world inside the
        # kernel; their entropy gradient follows as further pieces — autograd's (or B's view: autograd's + the entropy
        # sink's flush, as ONE piece), the entropy sink's buffer, the planes' graph's.
        pieces = cdist.fold_entropy_gradients(A, self._tables if tables_fused else (), self.world,
                                              grads=ctx_grads, other=B if ctx_grads is None and c.lmbda > 0 else None)
        table_pieces = pieces if tables_fused else None
        if ctx_grads is not None:
            if self.sink_ctx is not None:      # the heads' gradients into `.grad` = A's views (bound before the fork), behind
                self.sink_ctx.flush(table_pieces=table_pieces)       # the mean; the tables' buffers listed
            if self._planes_replayed:
                self.planes_graph.flush(table_pieces=table_pieces)
        A.bind(force=True)
        return bpp, mb, table_pieces

    def _verdict(self, losses, range_guard, tables_fused) -> None:
        """The guarded step's verdict, on the device and before any update.  `losses`: the step's loss scalars."""
        # Scanned: every gradient the two library optimizers will read (the tables' pieces are not: DESIGN.md §13), the
        # loss scalars, and the gradient of every live ray-side parameter, whose Adam takes the same word; data parallel:
        # what every rank holds alike — the bucket's summed non-table runs with the entropy gradient added, and the
        # all-reduced guard slot.
        sg, A = self.step_guard, self.bucket
        live = [rec for rec in self._learned if rec.live]
        if A is None:
            scan = [p.grad for o in (self.opt, self.opt2) for g in o.param_groups for p in g["params"]
                    if p.grad is not None and id(p) not in self._table_ids]
            scan += [t.detach().reshape(-1) for t in losses if isinstance(t, torch.Tensor) and t.dtype == torch.float32]
            scan += [rec.param.grad.reshape(-1) for rec in live]
            sg.scan(scan, range_guard=range_guard)
        else:
            sg.scan([A.flat[lo:hi] for lo, hi in A.runs_excluding(self._tables)] + [A.tail[1:2]])
        grp = self.opt.param_groups[1]
        sg.seal(grp["lr"], grp["eps"], grp["weight_decay"], self.table_adam.clip_counters() if tables_fused else ())
        self.opt.found_inf = self.opt2.found_inf = sg.found_inf
        for rec in self._learned:
            rec.opt.found_inf = sg.found_inf
        sg.poll()

    def _update(self, step, table_pieces, tables_fused) -> None:
        """Both optimizers (the tables through their kernel when `tables_fused`), the schedules, the resync, the ray-side Adams."""
        c = self.cfg
        if tables_fused:
            # leaves the tables' `.grad` None: the library's step skips them.  Data parallel: `.grad` is the bucket's view
            # with the sum over the ranks (bound by `_backward_dp`), the first piece; 1 / world as a float32
            self.table_adam.step(table_pieces, grad_scale=1.0 if self.bucket is None else self._inv_world, guard=self.step_guard)
        elif self.table_adam is not None:
            self.table_adam.steps_done += 1            # the library steps them below
        self.opt.step()
        if c.lmbda > 0:
            self.opt2.step()
        if tables_fused:
            self.table_adam.mark_planes_current()      # (the two steps above dropped every cache: the tables' planes stand)
        self.sched.step()
        if c.lmbda > 0:
            self.sched2.step()
        if self.bucket is not None and (step + 1) % c.step_update == 0:
            # Only the entropy gradient can differ between replicas (float atomics in another order); the tensors it
            # does not reach — the field's MLPs — stay bit-identical by construction.  Compare bit checksums (one
            # small collective) and broadcast only what differs, instead of all 161 MB every time.
            n, nbytes = cdist.resync_parameters(self.bucket.params)
            self.resync["checks"] += 1
            self.resync["fired"] += 1 if n else 0
            self.resync["tensors"] += n
            self.resync["bytes"] += nbytes
        for rec in self._learned:           # the ray-side parameters the loss reached: each one's Adam and what follows it
            if rec.live:
                rec.opt.step()
                rec.after_step()

    def train(self, steps: Optional[int] = None, log=print):
        steps = self.cfg.max_steps if steps is None else steps
        tic = time.time()
        last = None
        for step in range(steps + 1):
            logging = step % self.cfg.log_every == 0 or step == steps
            s = self.train_step(step, want_stats=logging)
            if s is not None and logging:
                last = s
            if log and s is not None and step % self.cfg.log_every == 0 and self.rank == 0:
                log(f"elapsed_time={time.time() - tic:.2f}s | step={step} | psnr={s['psnr']:.2f} | "
                    f"n_rendering_samples={s['n_rendering_samples']} | num_rays={s['num_rays']} | "
                    f"bits_per_param={s['bpp']:.3f} | embed_bits_MB={s['embed_bits_MB']:.3f}"
                    + (f" | skipped={self.step_guard.stats()['skipped']}" if self.step_guard is not None else "")
                    + "".join(self._log_fields[k](s) for k in ("depth", "mean_abs_log_gain", "errmap_cover")
                              if k in self._log_fields))
        if self.exposure is not None and self.rank == 0:
            path = self.write_exposures()
            if log:
                log(f"exposure compensation: mean |log gain|={self.exposure.mean_magnitude():.3e} | written to {path}")
        if self.pose_refiner is not None and self.rank == 0:
            path = self.write_refined_transforms()
            if log:
                tau, omega = self.pose_refiner.mean_magnitudes()
                log(f"pose refinement: mean |tau|={tau:.3e} | mean |omega|={omega:.3e} rad | refined poses written to {path}")
        return last

    # ------------------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def evaluate(self, n_views: Optional[int] = None) -> float:
        """Mean PSNR over test views; views are sharded over ranks and the mean is all-reduced."""
        c = self.cfg
        self.field.eval(); self.estimator.eval()
        n_views = c.test_views if n_views is None else n_views
        lo, hi = cdist.shard_range(n_views, self.rank, self.world)
        tot = 0.0
        for i in range(lo, hi):
            d = self.dataset.view(i)
            rgb = self.render_test_view(d)
            mse = F.mse_loss(rgb, d["pixels"])
            tot += -10.0 * math.log10(max(mse.item(), 1e-12))
        tot = cdist.sum_over_ranks(tot, self.device)
        return tot / max(n_views, 1)

    @torch.no_grad()
    def prune_floaters(self, min_cells: Optional[int] = None, connectivity: Optional[int] = None) -> Dict[str, int]:
        """Clear the occupancy grid's floaters: the connected components with fewer than `min_cells` cells,
        every level on its own, the largest always kept.  None: cfg.prune_floaters / cfg.prune_connectivity.  Everything that
        reads the grid afterwards — the evaluations, the codec, `save_container`, the mesh — sees the pruned one.  A thin
        detached part of the scene can be a small component too: compare `evaluate()` before and after.  `min_cells` has no
        tuned value.  -> {components, cells, removed_components, removed_cells}."""
        min_cells = int(self.cfg.prune_floaters if min_cells is None else min_cells)
        connectivity = int(self.cfg.prune_connectivity if connectivity is None else connectivity)
        return self.estimator.prune_small_components(min_cells, connectivity)

    # ------------------------------------------------------------------------------ codec
    def extract_mesh(self, path: Optional[str] = None, resolution: int = 256, threshold: Optional[float] = None,
                     colors: bool = True, return_lattice: bool = False, min_component_points: int = 0):
        """The scene's surface as a `cnc_amd.mesh.Mesh`: marching tetrahedra on a lattice of `resolution`
        cells along the box's longest side, the field's `query_density` evaluated where the estimator's level-0 grid does
        not rule a point out — the scene as the renderer sees it.  threshold None: the density at which one render step
        is half opaque, ln 2 / cfg.render_step_size; it scales with the scene and has not been tuned.  colors: the field
        once on the vertices, seen along -normal.  path: also written there as a binary PLY.  return_lattice (debugging):
        -> (mesh, the capped float32 lattice it was cut from).  min_component_points > 0: the lattice's inside components
        with fewer points are dropped first (`cnc_amd.mesh.extract_mesh`); untuned."""
        from .mesh import field_mesh
        out = field_mesh(self.field, self.estimator.aabbs[0], self.estimator.binaries[0], self.cfg.render_step_size,
                         resolution=resolution, threshold=threshold, colors=colors, return_lattice=return_lattice,
                         min_component_points=min_component_points)
        if path is not None:
            (out[0] if return_lattice else out).save(path)
        return out

    def coder_name(self) -> str:
        """"device" when this Trainer codes with the device coder (TrainConfig.device_coder or CNC_DEVICE_CODER=1)."""
        on = bool(self.cfg.device_coder) or os.environ.get("CNC_DEVICE_CODER", "0") == "1"
        return "device" if on else "host"

    def occupancy_coder_name(self) -> str:
        """"pyramid" when this Trainer's containers code the occupancy grid with the pyramid model
        (TrainConfig.occupancy_coder or CNC_OCC_CODER=pyramid), else "iid"."""
        name = os.environ.get("CNC_OCC_CODER") or self.cfg.occupancy_coder
        if name not in ("iid", "pyramid"):
            raise ValueError(f"occupancy coder must be 'iid' or 'pyramid', got {name!r}")
        return name

    def mlp_coder_name(self) -> str:
        """"tree" when this Trainer's containers code the MLP's indices with the bit-tree model (TrainConfig.mlp_coder or
        CNC_MLP_CODER=tree), else "packed"."""
        name = os.environ.get("CNC_MLP_CODER") or self.cfg.mlp_coder
        if name not in ("packed", "tree"):
            raise ValueError(f"mlp coder must be 'packed' or 'tree', got {name!r}")
        return name

    @torch.no_grad()
    def encode(self, prefix: Optional[str] = None, coder: Optional[str] = None):
        os.makedirs(self.cfg.out_dir, exist_ok=True)
        prefix = prefix or os.path.join(self.cfg.out_dir, "b")
        os.makedirs(os.path.dirname(os.path.abspath(prefix)), exist_ok=True)
        e = self.field.mlp_base
        self.context.eval()
        return self.context.encode_binary_vxl_mixPg_3D2D(e.encoding_xyz, e.encoding_xy, e.encoding_xz,
                                                         e.encoding_yz, self.estimator.binaries,
                                                         filename_prefix=prefix, coder=coder or self.coder_name(),
                                                         symbols_per_lane=self.cfg.symbols_per_lane) + (prefix,)

    @torch.no_grad()
    def decode_into_field(self, Pgs, prefix, coder: Optional[str] = None):
        """Wipe the four tables, decode them from the .b files, install them (train:445-470).  `coder`: what wrote the
        files (default: this Trainer's coder)."""
        e = self.field.mlp_base
        recs = [torch.ones_like(t.params.data) for t in (e.encoding_xyz, e.encoding_xy, e.encoding_xz, e.encoding_yz)]
        for t in (e.encoding_xyz, e.encoding_xy, e.encoding_xz, e.encoding_yz):
            t.params.zero_()             # under no_grad: bumps _version, which keys the sign-plane cache
            t.invalidate_caches()
        recs = self.context.decode_binary_vxl_mixPg_3D2D(e.encoding_xyz, e.encoding_xy, e.encoding_xz,
                                                         e.encoding_yz, *recs, self.estimator.binaries, Pgs,
                                                         filename_prefix=prefix, coder=coder or self.coder_name())
        self.field.update_embedding_params(*recs)

    def sizes_MB(self, coded_MB: float) -> Dict[str, float]:
        ctx_MB = sum(p.numel() * 32 for p in self.context.parameters()) / 8.0 / 1024 / 1024
        _, occ_MB, _ = get_binary_vxl_size(self.estimator.binaries)
        mlp = {k: v for k, v in self.field.state_dict().items() if "encoding" not in k and k != "aabb"}
        mlp_MB, _, _ = quantize_params(mlp, digits=13)
        sizes = {"embeddings": coded_MB, "context_models": ctx_MB, "occupancy_grid": occ_MB, "mlp_13bit": mlp_MB,
                 "total": coded_MB + ctx_MB + occ_MB + mlp_MB}
        if self.envmap is not None:          # the container's raw uint8 section
            sizes["envmap"] = self.envmap.texture.numel() / 1024.0 / 1024.0
            sizes["total"] += sizes["envmap"]
        return sizes

    # ------------------------------------------------------------------------------ container
    def _mlp_state(self):
        return {k: v for k, v in self.field.state_dict().items() if "encoding" not in k and k != "aabb"}

    @torch.no_grad()
    def save_container(self, path: str) -> Dict[str, float]:
        """Encode the tables and write everything a decoder needs into one file; returns sizes in KB."""
        from .container import section_sizes, write_container
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            Pgs, est_MB, coded_MB, prefix = self.encode(os.path.join(td, "b"))
            streams = {f[2:-2]: open(os.path.join(td, f), "rb").read()
                       for f in sorted(os.listdir(td)) if f.endswith(".b")}
        meta = {"Pgs": {k: float(v) for k, v in Pgs.items()}, "n_features": self.cfg.n_features,
                "resolutions_list": list(self.cfg.resolutions_list),
                "resolutions_list_2D": list(self.cfg.resolutions_list_2D),
                "log2_hashmap_size": self.cfg.log2_hashmap_size,
                "log2_hashmap_size_2D": self.cfg.log2_hashmap_size_2D}
        if self.coder_name() == "device":
            meta["coder"] = "rans1"       # the table streams' format; no key = the range coder's
        occ, mlp = self.occupancy_coder_name(), self.mlp_coder_name()
        size = write_container(path, meta=meta, table_streams=streams, binaries=self.estimator.binaries,
                               field_mlp=self._mlp_state(), context_state=self.context.state_dict(), occupancy_coder=occ,
                               coder=self.coder_name(), symbols_per_lane=self.cfg.symbols_per_lane,
                               mlp_coder=mlp, envmap=None if self.envmap is None else self.envmap.quantized())
        res = {"file_KB": size / 1024.0, "embeddings_KB": coded_MB * 1024.0, "estimate_KB": est_MB * 1024.0}
        if occ == "pyramid":       # the section as written (the Bernoulli one still, for a grid with an odd side)
            res["occupancy_KB"] = section_sizes(path)["occupancy"] / 1024.0
        if mlp == "tree":          # the section as written (the packed ones still, where the tree saved nothing)
            res["mlp_KB"] = sum(v for k, v in section_sizes(path).items() if k == "mlp" or k.startswith("mlp/")) / 1024.0
        return res

    @torch.no_grad()
    def load_container(self, path: str) -> None:
        """Inverse of save_container on a freshly constructed Trainer with the same config: restores
        occupancy, context models and the (13-bit) MLP, then decodes the four tables."""
        from .container import read_container, read_envmap
        import tempfile
        env = read_envmap(path)
        if (env is None) != (self.envmap is None):
            raise RuntimeError(f"{path} " + ("holds a learned background (an `envmap` section) and this Trainer has none: "
                                             "build it with background='envmap'" if self.envmap is None else
                                             "holds no learned background and this Trainer has one: build it with "
                                             "background='solid'"))
        if env is not None and tuple(env.shape) != tuple(self.envmap.texture.shape):
            raise RuntimeError(f"{path}: the background is {list(env.shape)}, this Trainer's {list(self.envmap.texture.shape)}"
                               " (envmap_resolution)")
        meta, streams, binaries, mlp, ctx = read_container(path, device=self.device)
        self.estimator.binaries = binaries.to(self.device)
        self.context.load_state_dict(ctx, strict=True)
        self.field.load_state_dict(mlp, strict=False)
        Pgs = {k: torch.tensor(v, device=self.device) for k, v in meta["Pgs"].items()}
        with tempfile.TemporaryDirectory() as td:
            for name, blob in streams.items():
                open(os.path.join(td, f"b_{name}.b"), "wb").write(blob)
            fmt = meta.get("coder")
            if fmt not in (None, "rans1"):
                raise RuntimeError(f"{path}: table streams in an unknown format {fmt!r}")
            self.decode_into_field(Pgs, os.path.join(td, "b"), coder="device" if fmt == "rans1" else "host")
        if env is not None:          # validated above, assigned last: a load that failed on the way leaves the map as it was
            self.envmap.load_quantized(env)
