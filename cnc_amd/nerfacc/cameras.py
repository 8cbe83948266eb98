"""`nerfacc.cameras` of the reference (nerfacc/cameras.py): OpenCV lens distortion and its inverse.

`opencv_lens_undistortion` and `opencv_lens_undistortion_fisheye` run the HIP kernels of csrc/camera.hip on device tensors
(through `nerfacc.cuda`, as the reference does) and the pure-torch restatements below on host tensors, which double as the
readable spec.  None of it is differentiable.  A single coefficient row is never expanded to one row per point: the
broadcast view goes to the kernel as it is and is read as one row.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import Tensor

from . import cuda as _C
from ..backends.nerfacc_cuda import _shared_row


def _pad8(params: Tensor) -> Tensor:
    if params.shape[-1] not in (0, 1, 2, 4, 8):
        raise AssertionError(f"params must hold 0, 1, 2, 4 or 8 coefficients, not {params.shape[-1]}")
    return F.pad(params, (0, 8 - params.shape[-1]), "constant", 0.0) if params.shape[-1] < 8 else params


def _rows_for(uv: Tensor, params: Tensor) -> Tensor:
    """`params` broadcast to uv's batch shape, as a view when it is one row (the kernel's shared-row path), else packed."""
    params = torch.broadcast_to(params, uv.shape[:-1] + (params.shape[-1],))
    return params if _shared_row(params) else params.contiguous()


def opencv_lens_undistortion(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """Undistort OpenCV's rational-radial + tangential model.

    uv: (..., 2).  params: (..., N) or (N), N in {0, 1, 2, 4, 8}: {}, {k1}, {k1, k2}, {k1, k2, p1, p2},
    {k1, k2, p1, p2, k3, k4, k5, k6} (zero-padded to 8; N = 0 returns `uv` itself).  -> (..., 2)."""
    assert uv.shape[-1] == 2
    if params.shape[-1] == 0:
        return uv
    params = _pad8(params)
    if not uv.is_cuda:
        return _opencv_lens_undistortion(uv, params, eps, iters)
    return _C.opencv_lens_undistortion(uv.contiguous(), _rows_for(uv, params), eps, iters)


def opencv_lens_undistortion_fisheye(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """Undistort OpenCV's fisheye model {k1, k2, k3, k4}.  uv: (..., 2), params: (..., 4) or (4) -> (..., 2).
    A point that does not converge in `iters` rounds keeps its input."""
    assert uv.shape[-1] == 2
    assert params.shape[-1] == 4
    if not uv.is_cuda:
        return _opencv_lens_undistortion_fisheye(uv, params, eps, iters)
    return _C.opencv_lens_undistortion_fisheye(uv.contiguous(), _rows_for(uv, params), eps, iters)


def _opencv_lens_distortion(uv: Tensor, params: Tensor) -> Tensor:
    """The forward model: ideal (x, y) -> distorted, {k1, k2, p1, p2, k3, k4, k5, k6}
    (https://docs.opencv.org/3.4/d9/d0c/group__calib3d.html)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = torch.unbind(params, dim=-1)
    x, y = torch.unbind(uv, dim=-1)
    r = x * x + y * y
    q = (1 + r * (k1 + r * (k2 + r * k3))) / (1 + r * (k4 + r * (k5 + r * k6)))
    txy = 2 * x * y
    return torch.stack([x * q + p1 * txy + p2 * (r + 2 * x * x), y * q + p2 * txy + p1 * (r + 2 * y * y)], dim=-1)


def _opencv_lens_distortion_fisheye(uv: Tensor, params: Tensor, eps: float = 1e-10) -> Tensor:
    """The fisheye forward model {k1, k2, k3, k4} (https://docs.opencv.org/4.x/db/d58/group__calib3d__fisheye.html)."""
    assert params.shape[-1] == 4, f"Invalid params shape: {params.shape}"
    k1, k2, k3, k4 = torch.unbind(params, dim=-1)
    r = torch.sqrt((uv * uv).sum(-1))
    t = torch.atan(r)
    t2 = t * t
    theta_d = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    return uv * (theta_d / torch.clamp(r, min=eps))[..., None]


def _opencv_lens_undistortion(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """`opencv_lens_undistortion` in torch ops: Newton's method on g(x, y) = distort(x, y) - uv from (x, y) = uv, every
    point taking `iters` rounds; a round whose Jacobian has |det| <= eps leaves the point where it is."""
    assert uv.shape[-1] == 2
    if params.shape[-1] == 0:
        return uv
    k1, k2, p1, p2, k3, k4, k5, k6 = torch.unbind(_pad8(params), dim=-1)
    u, v = torch.unbind(uv, dim=-1)
    x, y = u, v
    for _ in range(iters):
        r = x * x + y * y
        A = 1 + r * (k1 + r * (k2 + r * k3))
        B = 1 + r * (k4 + r * (k5 + r * k6))
        q = A / B
        txy = 2 * x * y
        gx = x * q + p1 * txy + p2 * (r + 2 * x * x) - u
        gy = y * q + p2 * txy + p1 * (r + 2 * y * y) - v
        qr = ((k1 + r * (2 * k2 + r * 3 * k3)) * B - A * (k4 + r * (2 * k5 + r * 3 * k6))) / (B * B)
        qx, qy = 2 * x * qr, 2 * y * qr
        j00 = q + x * qx + 2 * (p1 * y + 3 * p2 * x)
        j01 = x * qy + 2 * (p1 * x + p2 * y)
        j10 = y * qx + 2 * (p2 * y + p1 * x)
        j11 = q + y * qy + 2 * (p2 * x + 3 * p1 * y)
        det = j00 * j11 - j01 * j10
        ok = det.abs() > eps
        safe = torch.where(ok, det, torch.ones_like(det))
        x = x + torch.where(ok, (j01 * gy - j11 * gx) / safe, torch.zeros_like(det))
        y = y + torch.where(ok, (j10 * gx - j00 * gy) / safe, torch.zeros_like(det))
    return torch.stack([x, y], dim=-1)


def _opencv_lens_undistortion_fisheye(uv: Tensor, params: Tensor, eps: float = 1e-6, iters: int = 10) -> Tensor:
    """`opencv_lens_undistortion_fisheye` in torch ops (the update in float64, as the kernel evaluates it): a point that
    has not converged after `iters` rounds, or whose theta changed sign, keeps its input."""
    assert uv.shape[-1] == 2 and params.shape[-1] == 4
    k1, k2, k3, k4 = (c.double() for c in torch.unbind(params, dim=-1))
    td = torch.sqrt((uv * uv).sum(-1)).clamp(max=math.pi / 2).double()
    theta = td
    done = td <= eps
    for _ in range(iters):
        t2 = theta * theta
        a, b, c, d = k1 * t2, k2 * t2 * t2, k3 * t2 * t2 * t2, k4 * t2 * t2 * t2 * t2
        fix = (theta * (1 + a + b + c + d) - td) / (1 + 3 * a + 5 * b + 7 * c + 9 * d)
        theta = torch.where(done, theta, theta - fix)
        done = done | (fix.abs() < eps)
    scale = torch.where(td > eps, torch.tan(theta) / td.clamp(min=1e-30), torch.zeros_like(td))
    keep = done & ~(theta < 0)
    return torch.where(keep[..., None], uv * scale.to(uv.dtype)[..., None], uv)
