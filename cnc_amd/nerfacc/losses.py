"""Regularisers on ray samples.  `distortion` is the interval-distortion loss of mip-NeRF 360 (Barron et al. 2022,
eq. 15), the standard defence against floaters:

    L_ray = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 d_i        m = interval midpoints, d = their widths

On the GPU it is ONE fused HIP kernel per direction (cnc_amd/csrc/distortion.hip) over either sample layout; on other
tensors the same recurrences in plain torch.  The arithmetic never subtracts one prefix sum from another (the textbook
form m_i W_<i - M_<i loses every digit on a thin surface far from the origin):

    g_i = m_i - m_{i-1} = 0.5 ((t0_i - t0_{i-1}) + (t1_i - t1_{i-1}))
    A_i = sum_{j<i} w_j (m_i - m_j):  A_0 = 0, A_i = A_{i-1} + g_i Winc_{i-1}         Winc = inclusive running sum of w
    B_i = sum_{j>i} w_j (m_j - m_i):  the same recurrence back to front
    L_ray = sum_i w_i (2 A_i + w_i d_i / 3),    dL_ray/dw_i = 2 (A_i + B_i) + (2/3) w_i d_i

Preconditions: w >= 0 and midpoints that do not decrease along a ray (gaps between intervals are fine).  Decreasing
midpoints are a caller error and are not checked: the signed formula is what comes out.  An empty ray gives 0, a ray
of one sample w^2 d / 3.  Gradients flow to the weights only: `t_starts` / `t_ends` are constants of the loss (every
sampler here draws them under no_grad).

`depth_loss` is depth supervision against a measured distance D per ray (csrc/depth_loss.hip):

    e_i = 0.5 ((t0_i - D) + (t1_i - D)),    S1 = sum_i w_i e_i,    S2 = sum_i w_i e_i^2
    L_ray = S1^2 + spread S2,               dL_ray/dw_i = 2 S1 e_i + spread e_i^2

with e_i formed per sample as written, never as sum w m - D sum w.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from ..backends import volrend_backend as _K
from .volrend import _ray_chunks


class _DistortionFused(torch.autograd.Function):
    """CUDA float32: cnc_distortion_forward / _backward.  `starts` = `counts` = None: batched rows."""

    @staticmethod
    def forward(ctx, weights, t_starts, t_ends, starts, counts):
        weights = weights.contiguous()
        ctx.save_for_backward(weights, t_starts, t_ends, starts, counts)
        return _K.distortion_forward(starts, counts, t_starts, t_ends, weights)

    @staticmethod
    def backward(ctx, g_loss):
        weights, t_starts, t_ends, starts, counts = ctx.saved_tensors
        return _K.distortion_backward(starts, counts, t_starts, t_ends, weights, g_loss.contiguous()), None, None, None, None


def _shifted(x: Tensor) -> Tensor:
    """x moved one place along the last axis, a zero in front."""
    return torch.nn.functional.pad(x[..., :-1], (1, 0))


def _rows_terms(w: Tensor, t0: Tensor, t1: Tensor):
    """(A, B, d) of batched rows (..., S): the module's recurrences as running sums along the last axis."""
    g = torch.zeros_like(w)
    g[..., 1:] = 0.5 * ((t0[..., 1:] - t0[..., :-1]) + (t1[..., 1:] - t1[..., :-1]))
    a = torch.cumsum(g * _shifted(torch.cumsum(w, -1)), -1)
    # back to front: the same on the reversed row, whose step in front of element k is g of the original element behind it
    wr, gr = w.flip(-1), _shifted(g.flip(-1))
    b = torch.cumsum(gr * _shifted(torch.cumsum(wr, -1)), -1).flip(-1)
    return a, b, t1 - t0


class _DistortionRows(torch.autograd.Function):
    """Any device and dtype, batched rows: the plain-torch restatement, with the gradient from its own recurrence (B)."""

    @staticmethod
    def forward(ctx, w, t0, t1):
        a, b, d = _rows_terms(w, t0, t1)
        ctx.save_for_backward(2.0 * (a + b) + 2.0 * (w * d / 3.0))
        return (w * (2.0 * a + w * d / 3.0)).sum(-1)

    @staticmethod
    def backward(ctx, g_loss):
        (dw,) = ctx.saved_tensors
        return g_loss.unsqueeze(-1) * dw, None, None


def _padded(chunks, n_samples: int):
    """Flattened rays as rows: (index (n_rays, longest), mask) — a row's tail repeats its last sample (weight masked to 0)."""
    starts, counts = chunks
    longest = int(counts.max().item()) if counts.numel() else 0
    k = torch.arange(longest, device=starts.device)[None, :]
    mask = k < counts[:, None]
    idx = starts[:, None] + torch.minimum(k, (counts[:, None] - 1).clamp_min(0))
    return idx.clamp(0, max(n_samples - 1, 0)), mask


def distortion(weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Optional[Tensor] = None,
               n_rays: Optional[int] = None, packed_info: Optional[Tensor] = None) -> Tensor:
    """The distortion loss of every ray.  Flattened samples ((N,) tensors with sorted `ray_indices` + `n_rays`, or
    `packed_info` (n_rays, 2)) return (n_rays,); batched samples (..., S) return `weights.shape[:-1]`.  Differentiable
    with respect to `weights` only.  CUDA float32 tensors take the fused kernels; everything else (CPU, float64) the
    same recurrences in plain torch, in the input dtype.

    >>> distortion(weights=[.5, .5], t_starts=[0., 2.], t_ends=[1., 3.], ray_indices=[0, 0], n_rays=1)
    [1.1667]        # 2 * .5 * .5 * |2.5 - .5| + (.25 * 1 + .25 * 1) / 3
    """
    if not (weights.shape == t_starts.shape == t_ends.shape):
        raise AssertionError("weights, t_starts and t_ends must have the same shape")
    t_starts, t_ends = t_starts.detach(), t_ends.detach()
    flat = ray_indices is not None or packed_info is not None
    if flat and weights.dim() != 1:
        raise AssertionError("flattened samples must have shape (N,)")
    chunks = _ray_chunks(weights, packed_info, ray_indices, n_rays) if flat else None
    if weights.is_cuda and weights.dtype == torch.float32 and t_starts.dtype == torch.float32 \
            and t_ends.dtype == torch.float32:
        starts, counts = chunks if flat else (None, None)
        return _DistortionFused.apply(weights, t_starts.contiguous(), t_ends.contiguous(), starts, counts)
    if not flat:
        if weights.shape[-1] == 0:
            return weights.new_zeros(weights.shape[:-1])
        return _DistortionRows.apply(weights, t_starts, t_ends)
    n = int(chunks[0].shape[0])
    if weights.shape[0] == 0 or n == 0:
        return weights.new_zeros((n,))
    idx, mask = _padded(chunks, weights.shape[0])
    w = torch.where(mask, weights[idx], weights.new_zeros(()))
    return _DistortionRows.apply(w, t_starts[idx], t_ends[idx])


class _DepthFused(torch.autograd.Function):
    """CUDA float32: cnc_depth_loss_forward / _backward.  `starts` = `counts` = None: batched rows."""

    @staticmethod
    def forward(ctx, weights, t_starts, t_ends, target, starts, counts, spread):
        weights = weights.contiguous()
        loss, s1 = _K.depth_loss_forward(starts, counts, t_starts, t_ends, weights, target, spread)
        ctx.save_for_backward(weights, t_starts, t_ends, target, starts, counts, s1)
        ctx.spread = spread
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        weights, t_starts, t_ends, target, starts, counts, s1 = ctx.saved_tensors
        g_w = _K.depth_loss_backward(starts, counts, t_starts, t_ends, weights, target, ctx.spread, s1, g_loss.contiguous())
        return g_w, None, None, None, None, None, None


class _DepthRows(torch.autograd.Function):
    """Any device and dtype, batched rows (..., S) with `mask` over the samples a row owns: the same formulas in plain
    torch, the gradient from its closed form."""

    @staticmethod
    def forward(ctx, w, t0, t1, target, mask, spread):
        valid = torch.isfinite(target) & (target > 0)
        D = torch.where(valid, target, torch.ones_like(target)).unsqueeze(-1)
        live = valid.unsqueeze(-1) & mask
        zero = w.new_zeros(())
        e = torch.where(live, 0.5 * ((t0 - D) + (t1 - D)), zero)
        a = torch.where(live, w, zero) * e
        s1, s2 = a.sum(-1), (a * e).sum(-1)
        ctx.save_for_backward(torch.where(live, (2.0 * s1).unsqueeze(-1) * e + spread * (e * e), zero), valid)
        return torch.where(valid, s1 * s1 + spread * s2, zero)

    @staticmethod
    def backward(ctx, g_loss):
        dw, valid = ctx.saved_tensors
        g = torch.where(valid, g_loss, g_loss.new_zeros(()))           # a NaN upstream of a ray without a measurement stays there
        return g.unsqueeze(-1) * dw, None, None, None, None, None


def depth_loss(weights: Tensor, t_starts: Tensor, t_ends: Tensor, target: Tensor, ray_indices: Optional[Tensor] = None,
               n_rays: Optional[int] = None, packed_info: Optional[Tensor] = None, spread: float = 1.0) -> Tensor:
    """Depth supervision of every ray against `target`, the measured distance ALONG THE RAY in scene units (one per ray:
    (n_rays,) for flattened samples, `weights.shape[:-1]` for batched ones; the layouts and the dispatch are `distortion`'s).

        L_ray = (sum_i w_i e_i)^2 + spread sum_i w_i e_i^2,      e_i = the midpoint of sample i minus the target

    The first term is instant-ngp's expected-depth error written about the target (for an opaque ray, (d - D)^2); the
    second is the line-of-sight term of Urban Radiance Fields / DS-NeRF: weight away from the measured surface costs
    w e^2 even where the expected depth comes out right on average.  Nothing here pushes opacity UP: a ray whose weights
    are all zero has loss 0 — making the surface opaque stays the colour loss's job.  `spread` >= 0.

    A target that is not finite or is <= 0 means "no measurement": that ray's loss is exactly 0 and its samples' gradients
    exactly +0, whatever flows in from upstream.  An empty ray gives 0.  Differentiable with respect to `weights` only.
    CUDA float32 tensors take the fused kernels; everything else (CPU, float64) the same formulas in plain torch, in the
    input dtype.

    >>> depth_loss(weights=[.5, .5], t_starts=[0., 2.], t_ends=[1., 3.], target=[2.], ray_indices=[0, 0], n_rays=1)
    [0.8125]        # (.5 * -1.5 + .5 * .5)^2 + (.5 * 2.25 + .5 * .25)
    """
    if not (weights.shape == t_starts.shape == t_ends.shape):
        raise AssertionError("weights, t_starts and t_ends must have the same shape")
    if not (spread >= 0):
        raise ValueError("depth_loss: spread must not be negative")
    t_starts, t_ends, target = t_starts.detach(), t_ends.detach(), target.detach()
    flat = ray_indices is not None or packed_info is not None
    if flat and weights.dim() != 1:
        raise AssertionError("flattened samples must have shape (N,)")
    chunks = _ray_chunks(weights, packed_info, ray_indices, n_rays) if flat else None
    lead = (int(chunks[0].shape[0]),) if flat else tuple(weights.shape[:-1])
    if tuple(target.shape) != lead:
        raise AssertionError(f"target must have one entry per ray: shape {lead}")
    if weights.is_cuda and weights.dtype == torch.float32 and t_starts.dtype == torch.float32 \
            and t_ends.dtype == torch.float32 and target.dtype == torch.float32:
        starts, counts = chunks if flat else (None, None)
        return _DepthFused.apply(weights, t_starts.contiguous(), t_ends.contiguous(), target.contiguous(), starts, counts,
                                 float(spread))
    target = target.to(weights.dtype)
    if not flat:
        if weights.shape[-1] == 0:
            return weights.new_zeros(lead)
        return _DepthRows.apply(weights, t_starts, t_ends, target, torch.ones_like(weights, dtype=torch.bool), float(spread))
    if weights.shape[0] == 0 or lead[0] == 0:
        return weights.new_zeros(lead)
    idx, mask = _padded(chunks, weights.shape[0])
    return _DepthRows.apply(weights[idx], t_starts[idx], t_ends[idx], target, mask, float(spread))
