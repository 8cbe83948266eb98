"""Per-camera exposure compensation: one log-gain per training camera and colour channel, learned next
to the field — what instant-ngp calls `optimize_exposure`.

Camera k scales what the loss sees by g_k = exp(e_k - mean_j e_j).  The mean is taken out per channel so that the
field's brightness and a gain common to all cameras are not interchangeable: gain 1 is the geometric mean of the training
exposures, and it is what every evaluation, the mesh colours and a container's receiver render with.  The pixel is

    g_k (c + (1 - a) b)      the gain on the whole pixel: opaque photographs, exposure scaled all the light
    g_k c + (1 - a) b        the gain on the foreground only: the background was blended in behind the photograph

with c, a the field's composited colour and opacity and b the background colour ([3], [n, 3] or absent).  The table, the
composite and the gradients are HIP kernels (csrc/exposure.hip); the per-camera gradient is folded in an order fixed by
the ray indices, so equal inputs give equal bits.  Host tensors take the torch restatement.
"""
from __future__ import annotations

import json
from typing import Optional

import torch

from .backends import exposure_backend as _K


class _Exposure(torch.autograd.Function):
    """The gained composite over the three launches (table, forward; the backward's two).  `owner`: an object whose
    `effective_grad` buffer [C, 3] also receives the gradient with respect to the effective log-gain."""

    @staticmethod
    def forward(ctx, log_gain, rgb, opacity, bkgd, cam_ids, gain_background, owner):
        gains = _K.exposure_gains(log_gain)
        ctx.save_for_backward(rgb, opacity, bkgd, cam_ids, gains)
        ctx.gain_background, ctx.owner = gain_background, owner
        return _K.exposure_forward(rgb, cam_ids, gains, opacity, bkgd, gain_background)

    @staticmethod
    def backward(ctx, g_out):
        rgb, opacity, bkgd, cam_ids, gains = ctx.saved_tensors
        g_rgb, g_opacity, g_log_gain, g_eff = _K.exposure_backward(g_out.contiguous(), rgb, cam_ids, gains, opacity, bkgd,
                                                                   ctx.gain_background, want_effective=True)
        if ctx.owner is not None:
            ctx.owner.effective_grad.copy_(g_eff)
        return g_log_gain, g_rgb, g_opacity if opacity is not None else None, None, None, None, None


class ExposureCompensation:
    """`log_gain` [C, 3], a Parameter of zeros at the start: every camera at the common exposure.  (Not an nn.Module: it
    has one tensor and no state dict worth the name; the container holds no gains.)"""

    def __init__(self, n_cameras: int, device=None):
        self.n_cameras = int(n_cameras)
        if self.n_cameras < 1:
            raise ValueError("exposure compensation needs at least one camera")
        self.log_gain = torch.nn.Parameter(torch.zeros((self.n_cameras, 3), dtype=torch.float32, device=device))
        # dL/d(effective log-gain) of the last backward (before the centring's transpose): zero for a camera without rays
        self.effective_grad = torch.zeros_like(self.log_gain.data)

    @torch.no_grad()
    def effective(self) -> torch.Tensor:
        """log g [C, 3]: the log-gains with their per-channel mean over the cameras taken out."""
        e = self.log_gain.detach()
        return e - e.mean(dim=0, keepdim=True)

    @torch.no_grad()
    def gains(self) -> torch.Tensor:
        """g [C, 3] = exp(log_gain - mean over the cameras): one launch on the GPU."""
        e = self.log_gain.detach()
        if e.is_cuda:
            return _K.exposure_gains(e)
        return torch.exp(e - e.mean(dim=0, keepdim=True))

    def __call__(self, rgb, camera_ids, opacity=None, bkgd=None, gain_background: bool = True):
        """rgb [..., 3], camera_ids int64 [...], opacity [..., 1] or [...] and bkgd [3] or [..., 3] (both or neither
        needed; opacity alone is ignored) -> the pixel the loss sees, shaped like rgb.  `gain_background`: the gain on
        the whole pixel (True) or on the foreground only.  Gradients: rgb, opacity, `log_gain`."""
        lead = rgb.shape
        n = rgb.numel() // 3
        ids = camera_ids.reshape(n)
        if bkgd is None:
            opacity = None
        elif opacity is None:
            raise RuntimeError("exposure compensation: a background needs the opacity")
        if not rgb.is_cuda:
            out = _K.exposure_torch(self.log_gain, rgb.reshape(n, 3), ids, None if opacity is None else opacity.reshape(n),
                                    bkgd if bkgd is None or bkgd.dim() == 1 else bkgd.reshape(n, 3), gain_background)
            return out.view(lead)
        op = None if opacity is None else opacity.reshape(n).float().contiguous()
        if bkgd is not None:
            bkgd = bkgd.detach().float().contiguous() if bkgd.dim() == 1 else bkgd.detach().reshape(n, 3).float().contiguous()
        out = _Exposure.apply(self.log_gain, rgb.reshape(n, 3).float().contiguous(), op, bkgd, ids.contiguous(),
                              bool(gain_background), self)
        return out.view(lead)

    def mean_magnitude(self) -> float:
        """mean |effective log-gain| over cameras and channels, as a float (a synchronisation: logging only)."""
        return float(self.effective().abs().mean())

    @torch.no_grad()
    def write(self, path: str, loader) -> None:
        """`exposures.json`: per training frame of `loader` (a `TransformsLoader`) its `file_path`, the effective
        `log_gain` and the `gain`, three numbers each, in the order of the loader's cameras."""
        with open(loader.transforms_path) as fp:
            frames = json.load(fp)["frames"]
        ids = [int(i) for i in loader.frame_ids]
        if len(ids) != self.n_cameras:
            raise ValueError(f"{loader.transforms_path}: {len(ids)} frames for {self.n_cameras} cameras")
        e = self.log_gain.detach().double().cpu()
        e = e - e.mean(dim=0, keepdim=True)
        doc = {"transforms": loader.transforms_path,
               "frames": [{"file_path": frames[i]["file_path"], "log_gain": [float(v) for v in row],
                           "gain": [float(v) for v in torch.exp(row)]} for i, row in zip(ids, e)]}
        with open(path, "w") as fp:
            json.dump(doc, fp, indent=1)
