"""Inverse-transform sampling over ray segments and a per-ray searchsorted (reference: nerfacc/pdf.py:13-131), on
the HIP kernels of cnc_amd/csrc/pdf.hip.  Both accept batched records ((n_rays, n) values) and flattened ones
(`packed_info` / `ray_indices`), like the reference."""
from __future__ import annotations

from typing import Optional, Tuple, Union

from torch import Tensor

from .data_specs import RayIntervals, RaySamples
from . import cuda as _C


def searchsorted(sorted_sequence: Union[RayIntervals, RaySamples],
                 values: Union[RayIntervals, RaySamples]) -> Tuple[Tensor, Tensor]:
    """(ids_left, ids_right), LongTensors shaped like `values.vals`, such that within each ray the key at ids_left
    is <= the value < the key at ids_right; a value outside its ray's range gets the ids it would have if it were
    clipped to the range.  The ids count from the start of the row for batched values and index the flattened `sorted_sequence.vals` for
    flattened ones.

    >>> seq = RayIntervals(vals=torch.tensor([0., 1., 0., 1., 2.], device="cuda"),
    ...                    packed_info=torch.tensor([[0, 2], [2, 3]], device="cuda"))
    >>> vals = RayIntervals(vals=torch.tensor([0.5, 1.5, 2.5], device="cuda"),
    ...                     packed_info=torch.tensor([[0, 1], [1, 2]], device="cuda"))
    >>> searchsorted(seq, vals)
    (tensor([0, 3, 3]), tensor([1, 4, 4]))
    """
    left, right = _C.searchsorted(values._to_cpp(), sorted_sequence._to_cpp())
    return left, right


def importance_sampling(intervals: RayIntervals, cdfs: Tensor, n_intervals_per_ray: Union[Tensor, int],
                        stratified: bool = False, jitter: Optional[Tensor] = None) -> Tuple[RayIntervals, RaySamples]:
    """Resample every ray into `n_intervals_per_ray` intervals by inverting the piecewise-linear CDF given at the
    edges of `intervals` (`cdfs`, same shape as `intervals.vals`).  Returns (intervals, samples): for an int count,
    batched (n_rays, n + 1) edges and (n_rays, n) samples (leading axes of a batched input are kept); for a
    tensor of per-ray counts, flattened records with `packed_info` and `ray_indices` (and `is_left` / `is_right`
    on the intervals).

    `stratified` jitters each ray's samples by one bias drawn with torch.rand on the device, so the draws follow
    `torch.manual_seed` (the reference's stream is a different one).  `jitter` (extension): the per-ray biases,
    float32 (n_rays,), instead of drawing them.

    >>> iv = RayIntervals(vals=torch.tensor([0., 1., 0., 1., 2.], device="cuda"),
    ...                   packed_info=torch.tensor([[0, 2], [2, 3]], device="cuda"))
    >>> iv2, s = importance_sampling(iv, torch.tensor([0., .5, 0., .5, 1.], device="cuda"), 2)
    >>> iv2.vals, s.vals
    ([[0.0, 0.5, 1.0], [0.0, 1.0, 2.0]], [[0.25, 0.75], [0.5, 1.5]])
    """
    n = n_intervals_per_ray.contiguous() if isinstance(n_intervals_per_ray, Tensor) else n_intervals_per_ray
    out_intervals, samples = _C.importance_sampling(intervals._to_cpp(), cdfs.contiguous(), n, stratified,
                                                    None if jitter is None else jitter.contiguous())
    return RayIntervals._from_cpp(out_intervals), RaySamples._from_cpp(samples)
