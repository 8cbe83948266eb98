"""Proposal-network transmittance estimator of mip-NeRF 360 (reference: nerfacc/estimators/prop_net.py:17-256).

Each proposal level evaluates its network on the current intervals, turns the densities into a CDF of the
opacity along the ray (1 - transmittance at every edge) and resamples the ray from it with
`importance_sampling` (HIP, cnc_amd/csrc/pdf.hip); the last CDF gives the final samples.  With
`requires_grad` the levels' (intervals, cdf) pairs are kept, and `update_every_n_steps` trains the proposal
networks so that their histograms bound the radiance field's from above (`_pdf_loss`).

Works for scenes an occupancy grid cannot bound (no aabb, unbounded): samples are drawn between `near_plane` and
`far_plane` in `uniform` or `lindisp` (uniform in 1 / t) spacing."""
from typing import Callable, List, Literal, Optional, Tuple

import torch
from torch import Tensor

from ..data_specs import RayIntervals
from ..pdf import importance_sampling, searchsorted
from ..volrend import render_transmittance_from_density
from .base import AbstractEstimator

SamplingType = Literal["uniform", "lindisp"]


def _opacity_cdf(trans: Tensor) -> Tensor:
    """(n_rays, S) transmittance at the sample starts -> (n_rays, S + 1) CDF at the edges: 1 - T, closed by 1."""
    return 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)


class PropNetEstimator(AbstractEstimator):
    """Proposal network transmittance estimator ("Mip-NeRF 360: Unbounded Anti-Aliased Neural Radiance Fields").

    Args:
        optimizer: optimiser of the proposal networks' parameters (needed to train them).
        scheduler: its learning-rate scheduler, stepped at every `update_every_n_steps`.
    """

    def __init__(self, optimizer: Optional[torch.optim.Optimizer] = None,
                 scheduler: Optional[torch.optim.lr_scheduler._LRScheduler] = None) -> None:
        super().__init__()
        self.optimizer, self.scheduler = optimizer, scheduler
        # (intervals, cdf) of every proposal level of the last sampling(requires_grad=True), then (final intervals, None)
        self.prop_cache: List[Tuple[RayIntervals, Optional[Tensor]]] = []

    def _step_scheduler(self) -> None:
        if self.scheduler is not None:
            self.scheduler.step()

    @torch.no_grad()
    def sampling(self, prop_sigma_fns: List[Callable], prop_samples: List[int], num_samples: int,
                 n_rays: int, near_plane: float, far_plane: float,
                 sampling_type: SamplingType = "lindisp",
                 stratified: bool = False, requires_grad: bool = False) -> Tuple[Tensor, Tensor]:
        """(t_starts, t_ends), each (n_rays, num_samples).

        `prop_sigma_fns[i](t_starts, t_ends)` takes (n_rays, prop_samples[i]) interval bounds and returns the
        densities there, same shape.  The levels run in order, each on the intervals the previous CDF drew; the
        first starts from a uniform CDF over [near_plane, far_plane].  With `requires_grad` the densities are
        computed with gradients and every level's (intervals, cdf) is cached for `update_every_n_steps`."""
        if len(prop_sigma_fns) != len(prop_samples):
            raise AssertionError("prop_sigma_fns and prop_samples must have the same length")
        dev = self.device
        # the unit segment [0, 1] in s-space with the identity CDF: the first level samples uniformly
        cdf = torch.tensor([0.0, 1.0], device=dev).expand(n_rays, 2).contiguous()
        edges = RayIntervals(vals=cdf)
        for sigma_fn, n_level in zip(prop_sigma_fns, prop_samples):
            edges, _ = importance_sampling(edges, cdf, n_level, stratified)
            t = _transform_stot(sampling_type, edges.vals, near_plane, far_plane)
            t0, t1 = t[..., :-1], t[..., 1:]
            with torch.set_grad_enabled(bool(requires_grad)):
                sigmas = sigma_fn(t0, t1)
                if sigmas.shape != t0.shape:
                    raise AssertionError(f"a proposal level returned {tuple(sigmas.shape)}, expected {tuple(t0.shape)}")
                cdf = _opacity_cdf(render_transmittance_from_density(t0, t1, sigmas)[0])
            if requires_grad:
                self.prop_cache.append((edges, cdf))
        edges, _ = importance_sampling(edges, cdf, num_samples, stratified)
        t = _transform_stot(sampling_type, edges.vals, near_plane, far_plane)
        if requires_grad:
            self.prop_cache.append((edges, None))
        return t[..., :-1], t[..., 1:]

    @torch.enable_grad()
    def compute_loss(self, trans: Tensor, loss_scaler: float = 1.0) -> Tensor:
        """Sum over the cached proposal levels of the mean `_pdf_loss` of the final intervals (their CDF from the
        radiance field's transmittance `trans` (n_rays, num_samples), detached) against the level's CDF, times
        `loss_scaler`.  Empties the cache; zero when it is empty."""
        if not self.prop_cache:
            return self._dummy.new_zeros(())
        final, _ = self.prop_cache.pop()
        target = _opacity_cdf(trans).detach()
        total = 0.0
        for level_edges, level_cdf in reversed(self.prop_cache):
            total = total + _pdf_loss(final, target, level_edges, level_cdf).mean()
        self.prop_cache.clear()
        return total * loss_scaler

    @torch.enable_grad()
    def update_every_n_steps(self, trans: Tensor, requires_grad: bool = False, loss_scaler: float = 1.0) -> float:
        """One optimiser step of the proposal networks on the cached levels when `requires_grad` (the value passed
        to the `sampling` call of this step); the scheduler steps either way.  Returns the loss as a float."""
        if requires_grad:
            return self._update(trans, loss_scaler)
        self._step_scheduler()
        return 0.0

    @torch.enable_grad()
    def _update(self, trans: Tensor, loss_scaler: float = 1.0) -> float:
        if not self.prop_cache:
            raise AssertionError("no cached proposal levels: call sampling(..., requires_grad=True) first")
        if self.optimizer is None:
            raise AssertionError("No optimizer is provided.")
        opt = self.optimizer
        loss = self.compute_loss(trans, loss_scaler)
        opt.zero_grad()
        loss.backward()
        opt.step()
        self._step_scheduler()
        return float(loss.detach())


def get_proposal_requires_grad_fn(target: float = 5.0, num_steps: int = 1000) -> Callable:
    """step -> bool: whether to train the proposal networks at this step.  The gap between two training steps
    grows linearly from 0 to `target` over the first `num_steps` steps: a step trains when more steps than
    min(step / num_steps, 1) * target have passed since the last one that did."""
    since_last = 0

    def requires_grad_at(step: int) -> bool:
        nonlocal since_last
        train = since_last > min(step / num_steps, 1.0) * target
        since_last = 1 if train else since_last + 1
        return train

    return requires_grad_at


_SPACINGS = {"uniform": lambda x: x, "lindisp": lambda x: 1 / x}      # each its own inverse


def _transform_stot(transform_type: SamplingType, s_vals: Tensor, t_min, t_max) -> Tensor:
    """Normalised positions s in [0, 1] -> distances t: linear between t_min and t_max (`uniform`), or linear in
    1 / t (`lindisp`): t = g^-1(s g(t_max) + (1 - s) g(t_min)) with g = identity or reciprocal."""
    g = _SPACINGS.get(transform_type)
    if g is None:
        raise ValueError(f"unknown transform_type {transform_type!r} (uniform or lindisp)")
    g_min, g_max = g(t_min), g(t_max)
    return g(s_vals * g_max + (1 - s_vals) * g_min)


def _pdf_loss(segments_query: RayIntervals, cdfs_query: Tensor, segments_key: RayIntervals, cdfs_key: Tensor,
              eps: float = 1e-7) -> Tensor:
    """Per interval of the query histogram: max(w - w_outer, 0)^2 / (w + eps), w its weight (CDF increment) and
    w_outer the key histogram's weight over the key intervals that cover it (the mip-NeRF 360 proposal loss).

    A batched query ((n_rays, n) edges and CDF) takes a batched key; a flattened query (1-D, with `is_left` / `is_right`)
    takes a flattened or a batched key, and returns one value per query interval, ray after ray."""
    batched = segments_query.vals.ndim >= 2
    if batched and segments_key.vals.ndim < 2:        # the ids of a batched query count from the start of its row
        raise AssertionError(f"a batched query needs a batched key: the key's edges are "
                             f"{tuple(segments_key.vals.shape)}, the query's {tuple(segments_query.vals.shape)}")
    left, right = searchsorted(segments_key, segments_query)
    if batched:
        w = torch.diff(cdfs_query, dim=-1)
        lo, hi = left[..., :-1], right[..., 1:]
    else:
        if segments_query.is_left is None or segments_query.is_right is None:
            raise AssertionError("a flattened query needs is_left and is_right")
        w = cdfs_query[segments_query.is_right] - cdfs_query[segments_query.is_left]
        lo, hi = left[segments_query.is_left], right[segments_query.is_right]
        # the ids of a flattened query index the key's values as a whole, whether the key is flattened or batched
        cdfs_key = cdfs_key.reshape(-1)
    w_outer = cdfs_key.gather(-1, hi) - cdfs_key.gather(-1, lo)
    excess = (w - w_outer).clamp_min(0)
    return excess * excess / (w + eps)
