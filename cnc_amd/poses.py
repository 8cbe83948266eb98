"""Camera pose refinement: one (omega, tau) per training camera, learned next to the field.

The pose of camera c is R_c = exp(omega_c) R0_c, t_c = t0_c + tau_c with (R0, t0) the pose of the capture's file.  The
gradient comes from the render pass itself: the field hands back dL/dx for every sample (cnc_field_position_grad), a
sample lies at x = t_c + m d with d = R_c (camera-frame direction), so per ray dL/dt = sum dL/dx and
dL/d(rotation) = d x sum m dL/dx, folded per camera in a fixed order (cnc_ray_pose_grad).  The rotational part is the
gradient with respect to a LEFT perturbation exp(phi) exp(omega) R0 at phi = 0: exact at omega = 0, and the chart
gradient up to the left Jacobian I + O(|omega|) elsewhere — instant-ngp's approximation.  The view direction's path
through the head is not differentiated.  Two kernels, no atomics: equal inputs give equal bits.
"""
from __future__ import annotations

import json
from typing import Optional, Sequence

import torch

from . import _lib


def pose_apply(base_table: torch.Tensor, delta: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cnc_camera_pose_apply: the camera table [C, CNC_CAMERA_ROW] with R' = exp(omega) R0, t' = t0 + tau of
    delta [C, 6] = (omega, tau); every other field copied.  `out`: a table to rewrite (not `base_table` itself)."""
    _lib.check_input(base_table, "base_table")
    _lib.check_input(delta, "delta")
    C = base_table.shape[0]
    if base_table.dtype != torch.float32 or base_table.dim() != 2 or base_table.shape[1] != _lib.CNC_CAMERA_ROW:
        raise RuntimeError(f"pose_apply: base_table must be float32 [C, {_lib.CNC_CAMERA_ROW}]")
    if delta.dtype != torch.float32 or tuple(delta.shape) != (C, 6):
        raise RuntimeError("pose_apply: delta must be float32 [C, 6]")
    if out is None:
        out = torch.empty_like(base_table)
    else:
        _lib.check_input(out, "out")
        if out.shape != base_table.shape or out.dtype != torch.float32 or out.data_ptr() == base_table.data_ptr():
            raise RuntimeError("pose_apply: out must be another float32 table of the base table's shape")
    _lib.check(_lib.lib().cnc_camera_pose_apply(base_table.data_ptr(), delta.detach().data_ptr(), C, out.data_ptr(),
                                                _lib.stream(base_table.device)), "camera_pose_apply")
    return out


def ray_pose_grad(g_x, t_starts, t_ends, starts, counts, dirs, cam_ids, n_cameras: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cnc_ray_pose_grad: G [n_cameras, 6] from the samples' position gradients g_x [N, 3], their (t_starts, t_ends), the
    per-ray (starts, counts) table (int64 [n_rays] each), the rays' unit directions [n_rays, 3] and cam_ids int64
    [n_rays].  The summation order is a function of the ray indices alone (include/cnc_hip.h)."""
    for name, t in (("g_x", g_x), ("t_starts", t_starts), ("t_ends", t_ends), ("starts", starts), ("counts", counts),
                    ("dirs", dirs), ("cam_ids", cam_ids)):
        _lib.check_input(t, name)
    n_rays, N = dirs.shape[0], g_x.shape[0]
    if any(t.dtype != torch.float32 for t in (g_x, t_starts, t_ends, dirs)) \
            or any(t.dtype != torch.int64 for t in (starts, counts, cam_ids)):
        raise RuntimeError("ray_pose_grad: float32 samples and directions, int64 starts / counts / cam_ids")
    if tuple(g_x.shape) != (N, 3) or t_starts.numel() != N or t_ends.numel() != N or tuple(dirs.shape) != (n_rays, 3) \
            or starts.numel() != n_rays or counts.numel() != n_rays or cam_ids.numel() != n_rays:
        raise RuntimeError("ray_pose_grad: shapes do not belong together")
    dev = dirs.device
    if out is None:
        out = torch.empty((n_cameras, 6), dtype=torch.float32, device=dev)
    L = _lib.lib()
    nbytes = int(L.cnc_ray_pose_grad_workspace(n_rays, n_cameras))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    _lib.check(L.cnc_ray_pose_grad(g_x.data_ptr(), t_starts.data_ptr(), t_ends.data_ptr(), N, starts.data_ptr(),
                                   counts.data_ptr(), dirs.data_ptr(), cam_ids.data_ptr(), n_rays, n_cameras, ws.data_ptr(),
                                   ws.numel() * 4, out.data_ptr(), _lib.stream(dev)), "ray_pose_grad")
    return out


class CameraPoseRefiner:
    """`delta` [C, 6] = (omega, tau) per training camera, a Parameter of zeros at the start: the file's poses.  (Not an
    nn.Module: `apply` is the pose map here.)"""

    def __init__(self, n_cameras: int, device):
        self.n_cameras = int(n_cameras)
        self.delta = torch.nn.Parameter(torch.zeros((self.n_cameras, 6), dtype=torch.float32, device=device))
        self._grad = torch.zeros_like(self.delta.data)

    def apply(self, base_table: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The camera table of the refined poses (one launch; `out`: the table to rewrite)."""
        return pose_apply(base_table, self.delta.data, out)

    @torch.no_grad()
    def accumulate(self, g_x: torch.Tensor, extras, rays, cam_ids: torch.Tensor) -> torch.Tensor:
        """dL/d(delta) of one render pass, WRITTEN into `delta.grad`: `g_x` = the `.grad` of the extras' `positions`
        (render_image_with_occgrid(..., position_grad=True)), `extras` that call's extras (t_starts, t_ends,
        packed_info), `rays` its rays, `cam_ids` the batch's "camera_ids"."""
        info = extras["packed_info"]
        if info is None:
            raise RuntimeError("accumulate: the extras hold no per-ray (start, count) table")
        dirs = rays.viewdirs.reshape(-1, 3).contiguous()
        ray_pose_grad(g_x.reshape(-1, 3).contiguous(), extras["t_starts"].contiguous(), extras["t_ends"].contiguous(),
                      info[:, 0].contiguous(), info[:, 1].contiguous(), dirs, cam_ids.reshape(-1).contiguous(),
                      self.n_cameras, out=self._grad)
        self.delta.grad = self._grad
        return self._grad

    @torch.no_grad()
    def poses(self, base_c2w: torch.Tensor) -> torch.Tensor:
        """[C, 4, 4] refined camera-to-world matrices of the base ones ([C, 3 | 4, 4])."""
        base = base_c2w.to(device=self.delta.device, dtype=torch.float32)
        C = base.shape[0]
        table = torch.zeros((C, _lib.CNC_CAMERA_ROW), dtype=torch.float32, device=base.device)
        table[:, 4:16] = base[:, :3, :4].reshape(C, 12)
        rows = self.apply(table)[:, 4:16].reshape(C, 3, 4)
        out = torch.zeros((C, 4, 4), dtype=torch.float32, device=base.device)
        out[:, :3] = rows
        out[:, 3, 3] = 1.0
        return out

    def mean_magnitudes(self):
        """(mean |tau|, mean |omega|) over the cameras, as floats (a synchronisation: logging only)."""
        d = self.delta.detach()
        return float(d[:, 3:].norm(dim=1).mean()), float(d[:, :3].norm(dim=1).mean())

    @torch.no_grad()
    def write_transforms(self, src_json: str, dst_json: str, frame_ids: Optional[Sequence[int]] = None) -> None:
        """`src_json` with the `transform_matrix` of every training frame replaced by the refined one, written to
        `dst_json`.  `frame_ids`: for camera c the index of its frame in the file's `frames` (default: frame c; the file
        must then hold exactly the cameras).  The file's own matrices are the base poses."""
        with open(src_json) as fp:
            doc = json.load(fp)
        frames = doc["frames"]
        ids = list(range(len(frames))) if frame_ids is None else [int(i) for i in frame_ids]
        if len(ids) != self.n_cameras:
            raise ValueError(f"{src_json}: {len(ids)} frames for {self.n_cameras} cameras")
        base = torch.tensor([frames[i]["transform_matrix"] for i in ids], dtype=torch.float32)
        refined = self.poses(base).cpu()
        for i, m in zip(ids, refined):
            old = frames[i]["transform_matrix"]
            new = [[float(v) for v in row] for row in m[:3]]
            new.append([float(v) for v in old[3]] if len(old) > 3 else [0.0, 0.0, 0.0, 1.0])
            frames[i]["transform_matrix"] = new
        with open(dst_json, "w") as fp:
            json.dump(doc, fp, indent=1)
