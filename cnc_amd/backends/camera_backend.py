"""Host mirror of cnc_camera_rays (csrc/camera.hip, include/cnc_hip.h): pixels -> world rays in one launch, an extension
(the reference's loaders build rays with a chain of torch ops), and the torch restatement the loaders use on a host device.

A camera table is f32 [n_cams, 24]: fx fy cx cy | the rows of the 3x4 camera-to-world matrix | eight lens coefficients
(`camera_table`).  The callee allocates and returns its outputs, like the other mirrors.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream

MODELS = {"PINHOLE": _lib.CNC_CAMERA_PINHOLE, "OPENCV": _lib.CNC_CAMERA_OPENCV, "OPENCV_FISHEYE": _lib.CNC_CAMERA_FISHEYE}


def camera_table(intrinsics, camtoworlds, lens=None):
    """[n, 24] float32 from intrinsics [n, 4] (fx fy cx cy), camtoworlds [n, 3|4, 4] and lens [n, <= 8] (zero-padded)."""
    n = intrinsics.shape[0]
    table = torch.zeros(n, _lib.CNC_CAMERA_ROW, dtype=torch.float32, device=intrinsics.device)
    table[:, :4] = intrinsics
    table[:, 4:16] = camtoworlds[:, :3, :4].reshape(n, 12)
    if lens is not None:
        table[:, 16:16 + lens.shape[1]] = lens
    return table


def camera_rays(cams, model, opengl, cam_ids=None, px=None, py=None, *, cam0=0, width=0, height=0, images=None, bkgd=None,
                eps=1e-6, iters=10):
    """-> (origins, viewdirs, pixels | None), each [n, 3] float32.  `cam_ids, px, py` int64 [n] — or, with cam_ids None,
    the width x height pixels of camera `cam0` in row-major order (n = width * height).  images u8 [n_cams, H, W, 4] with
    bkgd f32 [3] on the device also fetches pixels = rgb * alpha + bkgd * (1 - alpha)."""
    check_input(cams, "cams")
    if cams.dtype != torch.float32 or cams.dim() != 2 or cams.shape[1] != _lib.CNC_CAMERA_ROW:
        raise RuntimeError(f"camera_rays: cams must be float32 [n_cams, {_lib.CNC_CAMERA_ROW}]")
    dev = cams.device
    if cam_ids is not None:
        for name, t in (("cam_ids", cam_ids), ("px", px), ("py", py)):
            if t is None:
                raise RuntimeError(f"camera_rays: {name} is missing")
            check_input(t, name)
            if t.dtype != torch.int64 or t.dim() != 1 or t.shape[0] != cam_ids.shape[0]:
                raise RuntimeError(f"camera_rays: {name} must be int64 [n]")
        n = cam_ids.shape[0]
    else:
        n = int(width) * int(height)
    if images is not None:
        check_input(images, "images")
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] != cams.shape[0] or images.shape[3] != 4:
            raise RuntimeError("camera_rays: images must be uint8 [n_cams, H, W, 4]")
        if bkgd is None:
            raise RuntimeError("camera_rays: a pixel fetch needs bkgd")
        check_input(bkgd, "bkgd")
        if bkgd.dtype != torch.float32 or bkgd.numel() != 3:
            raise RuntimeError("camera_rays: bkgd must be float32 [3]")
        if cam_ids is None and (images.shape[1] != height or images.shape[2] != width):
            raise RuntimeError("camera_rays: width and height must be the images'")
        height, width = images.shape[1], images.shape[2]
    origins = torch.empty((n, 3), dtype=torch.float32, device=dev)
    viewdirs = torch.empty((n, 3), dtype=torch.float32, device=dev)
    pixels = torch.empty((n, 3), dtype=torch.float32, device=dev) if images is not None else None
    rc = _lib.lib().cnc_camera_rays(ptr(cams), cams.shape[0], int(model), int(bool(opengl)), ptr(cam_ids), ptr(px), ptr(py),
                                    int(cam0), int(width), int(height), n, float(eps), int(iters), ptr(images),
                                    ptr(bkgd) if images is not None else None, ptr(origins), ptr(viewdirs), ptr(pixels),
                                    stream(dev))
    check(rc, "camera_rays")
    return origins, viewdirs, pixels


def depth_fetch(planes, cams, opengl, euclidean, cam_ids, px, py, viewdirs):
    """-> float32 [n]: the measured distance along each ray (cnc_depth_fetch), 0 = no measurement.  planes f32
    [n_cams, H, W]; cam_ids, px, py int64 [n]; viewdirs f32 [n, 3], what `camera_rays` returned for the same list."""
    for name, t, dtype in (("planes", planes, torch.float32), ("cams", cams, torch.float32), ("cam_ids", cam_ids, torch.int64),
                           ("px", px, torch.int64), ("py", py, torch.int64), ("viewdirs", viewdirs, torch.float32)):
        check_input(t, name)
        if t.dtype != dtype:
            raise RuntimeError(f"depth_fetch: {name} must be {dtype}")
    n = cam_ids.shape[0]
    if planes.dim() != 3 or cams.dim() != 2 or cams.shape[1] != _lib.CNC_CAMERA_ROW or planes.shape[0] != cams.shape[0]:
        raise RuntimeError(f"depth_fetch: planes must be [n_cams, H, W] next to cams [n_cams, {_lib.CNC_CAMERA_ROW}]")
    if cam_ids.dim() != 1 or px.shape != cam_ids.shape or py.shape != cam_ids.shape or tuple(viewdirs.shape) != (n, 3):
        raise RuntimeError("depth_fetch: cam_ids, px, py must be [n] and viewdirs [n, 3]")
    depth = torch.empty((n,), dtype=torch.float32, device=planes.device)
    check(_lib.lib().cnc_depth_fetch(ptr(planes), ptr(cams), planes.shape[0], planes.shape[1], planes.shape[2],
                                     int(bool(opengl)), int(bool(euclidean)), ptr(cam_ids), ptr(px), ptr(py), ptr(viewdirs),
                                     n, ptr(depth), stream(planes.device)), "depth_fetch")
    return depth


def depth_fetch_torch(planes, cams, opengl, euclidean, cam_ids, px, py, viewdirs):
    """The same in torch ops, for loaders on a host device."""
    z = planes[cam_ids, py, px]
    if euclidean:
        t, c = z, torch.ones_like(z)
    else:
        row = cams[cam_ids]
        c = (viewdirs[:, 0] * row[:, 6] + viewdirs[:, 1] * row[:, 10]) + viewdirs[:, 2] * row[:, 14]
        c = -c if opengl else c
        t = z / c
    ok = torch.isfinite(z) & (z > 0) & (c > 0)
    return torch.where(ok, t, torch.zeros_like(t))


def camera_rays_torch(cams, model, opengl, cam_ids, px, py, images=None, bkgd=None, eps=1e-6, iters=10):
    """The same in torch ops, for loaders on a host device (parsing and geometry testable without a GPU)."""
    from ..nerfacc import cameras
    row = cams[cam_ids]
    uv = torch.stack([(px - row[:, 2] + 0.5) / row[:, 0], (py - row[:, 3] + 0.5) / row[:, 1]], dim=-1)
    if model == _lib.CNC_CAMERA_OPENCV:
        uv = cameras._opencv_lens_undistortion(uv, row[:, 16:24], eps, iters)
    elif model == _lib.CNC_CAMERA_FISHEYE:
        uv = cameras._opencv_lens_undistortion_fisheye(uv, row[:, 16:20], eps, iters)
    flip = -1.0 if opengl else 1.0
    cam = torch.stack([uv[:, 0], uv[:, 1] * flip, torch.full_like(uv[:, 0], flip)], dim=-1)
    world = (row[:, 4:16].view(-1, 3, 4)[:, :, :3] * cam[:, None, :]).sum(-1)
    dirs = world / world.norm(dim=-1, keepdim=True)
    origins = row[:, 4:16].view(-1, 3, 4)[:, :, 3]
    pixels = None
    if images is not None:
        rgba = images[cam_ids, py, px].to(torch.float32) / 255.0
        pixels = rgba[:, :3] * rgba[:, 3:] + bkgd * (1.0 - rgba[:, 3:])
    return origins.contiguous(), dirs, pixels
