"""Host mirror of the exposure-compensation entry points (csrc/exposure.hip, include/cnc_hip.h): the gain table, the
gained composite and its backward — the ctypes calls and their argument checks — and the torch restatement for host
tensors.  The callee allocates and returns its outputs, like the other mirrors.
"""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import check, check_input, ptr, stream


def _check_table(t, name):
    check_input(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise RuntimeError(f"{name} must be float32 [n_cams, 3]")


def _check_rays(what, rgb, opacity, bkgd, cam_ids, gains, g_out=None):
    """-> (n, bkgd_per_ray): dtype, shape, contiguity and device of everything a ray kernel reads."""
    check_input(rgb, "rgb")
    if rgb.dtype != torch.float32 or rgb.dim() != 2 or rgb.shape[1] != 3:
        raise RuntimeError(f"{what}: rgb must be float32 [n, 3]")
    n, dev = rgb.shape[0], rgb.device
    _check_table(gains, "gains")
    check_input(cam_ids, "cam_ids")
    if cam_ids.dtype != torch.int64 or tuple(cam_ids.shape) != (n,):
        raise RuntimeError(f"{what}: cam_ids must be int64 [n]")
    if g_out is not None:
        check_input(g_out, "g_out")
        if g_out.dtype != torch.float32 or tuple(g_out.shape) != (n, 3):
            raise RuntimeError(f"{what}: g_out must be float32 [n, 3]")
    per_ray = False
    if bkgd is not None:
        if opacity is None:
            raise RuntimeError(f"{what}: a background needs the opacity")
        check_input(bkgd, "bkgd")
        per_ray = bkgd.dim() == 2
        if bkgd.dtype != torch.float32 or tuple(bkgd.shape) not in ((3,), (n, 3)):
            raise RuntimeError(f"{what}: bkgd must be float32 [3] or [n, 3]")
    if opacity is not None:
        check_input(opacity, "opacity")
        if opacity.dtype != torch.float32 or tuple(opacity.shape) != (n,):
            raise RuntimeError(f"{what}: opacity must be float32 [n]")
    for name, t in (("opacity", opacity), ("bkgd", bkgd), ("cam_ids", cam_ids), ("gains", gains), ("g_out", g_out)):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{what}: {name} is on {t.device}, rgb on {dev}")
    return n, per_ray


def exposure_gains(log_gain):
    """cnc_exposure_gains: log_gain f32 [C, 3] -> exp(log_gain - its mean over the cameras), f32 [C, 3]."""
    _check_table(log_gain, "log_gain")
    gains = torch.empty_like(log_gain)
    check(_lib.lib().cnc_exposure_gains(ptr(log_gain), log_gain.shape[0], ptr(gains), stream(log_gain.device)),
          "exposure_gains")
    return gains


def exposure_forward(rgb, cam_ids, gains, opacity=None, bkgd=None, gain_background=True):
    """cnc_exposure_forward -> out f32 [n, 3]: gains[cam_ids] (rgb + (1 - opacity) bkgd) with `gain_background`, else
    gains[cam_ids] rgb + (1 - opacity) bkgd; bkgd None: gains[cam_ids] rgb."""
    n, per_ray = _check_rays("exposure_forward", rgb, opacity, bkgd, cam_ids, gains)
    out = torch.empty_like(rgb)
    check(_lib.lib().cnc_exposure_forward(ptr(rgb), ptr(opacity), ptr(bkgd), int(per_ray), int(bool(gain_background)),
                                          ptr(cam_ids), ptr(gains), gains.shape[0], n, ptr(out), stream(rgb.device)),
          "exposure_forward")
    return out


def exposure_backward(g_out, rgb, cam_ids, gains, opacity=None, bkgd=None, gain_background=True, want_effective=False):
    """cnc_exposure_backward -> (g_rgb [n, 3], g_opacity [n] | None without a background, g_log_gain [C, 3]
    [, g_effective [C, 3] with `want_effective`: the gradient before the centring's transpose])."""
    n, per_ray = _check_rays("exposure_backward", rgb, opacity, bkgd, cam_ids, gains, g_out)
    dev, C = rgb.device, gains.shape[0]
    g_rgb = torch.empty_like(rgb)
    g_opacity = torch.empty((n,), dtype=torch.float32, device=dev) if bkgd is not None else None
    g_log_gain = torch.empty((C, 3), dtype=torch.float32, device=dev)
    g_eff = torch.empty((C, 3), dtype=torch.float32, device=dev) if want_effective else None
    L = _lib.lib()
    nbytes = int(L.cnc_exposure_backward_workspace(n, C))
    ws = torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=dev)
    check(L.cnc_exposure_backward(ptr(g_out), ptr(rgb), ptr(opacity), ptr(bkgd), int(per_ray), int(bool(gain_background)),
                                  ptr(cam_ids), ptr(gains), C, n, ptr(ws), ws.numel() * 4, ptr(g_rgb), ptr(g_opacity),
                                  ptr(g_eff), ptr(g_log_gain), stream(dev)), "exposure_backward")
    return (g_rgb, g_opacity, g_log_gain, g_eff) if want_effective else (g_rgb, g_opacity, g_log_gain)


def exposure_torch(log_gain, rgb, cam_ids, opacity=None, bkgd=None, gain_background=True):
    """The same in torch ops, differentiable by torch's own autograd: for host tensors (the model testable without a GPU)
    and as the definition the kernels are held to.  Any float dtype."""
    C = log_gain.shape[0]
    gains = torch.exp(log_gain - log_gain.mean(dim=0, keepdim=True))
    g = gains[cam_ids.clamp(0, C - 1)]
    if bkgd is None:
        return g * rgb
    behind = (1.0 - opacity.reshape(-1, 1)) * bkgd
    return g * (rgb + behind) if gain_background else g * rgb + behind
