"""Drop-in for the reference's `nerfacc.csrc` extension (nerfacc/cuda/csrc/nerfacc.cpp:100-129):
ray_aabb_intersect, traverse_grids, the six segmented scans, importance_sampling, searchsorted and the
RaySegmentsSpec record.

The callee allocates and returns tensors on the inputs' device, like the reference's host
functions; the allocation / cumsum logic of grid.cu:356-510 and data_spec.hpp:53-106 lives here
(torch ops), the kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import os

import torch

from .. import _lib
from .._lib import RaySegments, check, check_input, ptr, stream


class RaySegmentsSpec:
    """Mirror of RaySegmentsSpec (data_spec.hpp:6-13 / nerfacc.cpp:120-128): undefined tensors
    read as None from Python."""

    # alloc_starts (extension): where each ray's slots begin in `vals` when the march over-allocated
    # (chunk_starts is then recomputed from the true counts, data_spec.hpp:99-106, and no longer says)
    __slots__ = ("vals", "is_left", "is_right", "is_valid", "chunk_starts", "chunk_cnts",
                 "ray_indices", "alloc_starts")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)

    # data_spec.hpp:62-84
    def memalloc_data(self, size, alloc_masks=True, zero_init=True, alloc_valid=False):
        assert self.chunk_cnts is not None and self.vals is None
        dev = self.chunk_cnts.device
        mk = torch.zeros if zero_init else torch.empty
        self.vals = mk(size, dtype=torch.float32, device=dev)
        self.ray_indices = mk(size, dtype=torch.int64, device=dev)
        if alloc_masks:
            self.is_left = mk(size, dtype=torch.bool, device=dev)
            self.is_right = mk(size, dtype=torch.bool, device=dev)
        if alloc_valid:
            self.is_valid = torch.zeros(size, dtype=torch.bool, device=dev)

    # data_spec.hpp:86-96 (the .item() is the reference's host sync too)
    def memalloc_data_from_chunk(self, alloc_masks=True, zero_init=True, alloc_valid=False):
        assert self.chunk_cnts is not None and self.chunk_starts is None
        cumsum = torch.cumsum(self.chunk_cnts, 0, dtype=self.chunk_cnts.dtype)
        n_edges = int(cumsum[-1].item()) if cumsum.numel() else 0
        self.chunk_starts = cumsum - self.chunk_cnts
        self.memalloc_data(n_edges, alloc_masks, zero_init, alloc_valid)

    # data_spec.hpp:99-106
    def compute_chunk_start(self):
        if self.chunk_cnts is None:
            return
        cumsum = torch.cumsum(self.chunk_cnts, 0, dtype=self.chunk_cnts.dtype)
        self.chunk_starts = cumsum - self.chunk_cnts

    def _view(self) -> RaySegments:
        return RaySegments(ptr(self.vals), ptr(self.chunk_starts), ptr(self.chunk_cnts),
                           ptr(self.ray_indices), ptr(self.is_left), ptr(self.is_right),
                           ptr(self.is_valid))


def ray_aabb_intersect(rays_o, rays_d, aabbs, near_plane, far_plane, miss_value):
    n_rays, n_aabbs = rays_o.shape[0], aabbs.shape[0]
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("aabbs", aabbs)):
        check_input(t, name)
    t_mins = torch.empty((n_rays, n_aabbs), dtype=rays_o.dtype, device=rays_o.device)
    t_maxs = torch.empty((n_rays, n_aabbs), dtype=rays_o.dtype, device=rays_o.device)
    hits = torch.empty((n_rays, n_aabbs), dtype=torch.bool, device=rays_o.device)
    rc = _lib.lib().cnc_ray_aabb_intersect(ptr(rays_o), ptr(rays_d), ptr(aabbs), n_rays, n_aabbs,
                                           float(near_plane), float(far_plane), float(miss_value),
                                           ptr(t_mins), ptr(t_maxs), ptr(hits), stream(rays_o.device))
    check(rc, "ray_aabb_intersect")
    return [t_mins, t_maxs, hits]


def traverse_grids(rays_o, rays_d, rays_mask, binaries, aabbs, t_sorted, t_indices, hits,
                   near_planes, far_planes, step_size, cone_angle, compute_intervals,
                   compute_samples, compute_terminate_planes, traverse_steps_limit, over_allocate):
    """grid.cu:356-510."""
    if over_allocate and not traverse_steps_limit > 0:
        raise RuntimeError("traverse_steps_limit must be > 0 when over_allocate is true")
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("rays_mask", rays_mask),
                    ("binaries", binaries), ("aabbs", aabbs), ("t_sorted", t_sorted),
                    ("t_indices", t_indices), ("hits", hits), ("near_planes", near_planes),
                    ("far_planes", far_planes)):
        check_input(t, name)
    n_rays = rays_o.shape[0]
    n_grids = binaries.shape[0]
    dev = rays_o.device
    L = _lib.lib()
    intervals, samples = RaySegmentsSpec(), RaySegmentsSpec()
    terminate_planes = (torch.empty(n_rays, dtype=rays_o.dtype, device=dev)
                        if compute_terminate_planes else None)

    def launch(mask, first_pass, term):
        iv, sm = intervals._view(), samples._view()
        rc = L.cnc_traverse_grids(ptr(rays_o), ptr(rays_d), ptr(mask), n_rays, ptr(binaries),
                                  n_grids, binaries.shape[1], binaries.shape[2], binaries.shape[3],
                                  ptr(aabbs), ptr(hits), ptr(t_sorted), ptr(t_indices),
                                  ptr(near_planes), ptr(far_planes), float(step_size),
                                  float(cone_angle), int(traverse_steps_limit), int(first_pass),
                                  C.byref(iv), C.byref(sm), ptr(term), stream(rays_o.device))
        check(rc, "traverse_grids")

    if over_allocate:
        # single pass into an upper-bound allocation (grid.cu:400-440)
        if compute_intervals:
            intervals.chunk_cnts = torch.full((n_rays,), traverse_steps_limit * 2, dtype=torch.int64,
                                              device=dev) * rays_mask
            intervals.memalloc_data_from_chunk(True, True)
        if compute_samples:
            samples.chunk_cnts = torch.full((n_rays,), traverse_steps_limit, dtype=torch.int64,
                                            device=dev) * rays_mask
            samples.memalloc_data_from_chunk(False, True, True)
        n_out = (intervals.vals.numel() if compute_intervals else 0) + \
                (samples.vals.numel() if compute_samples else 0)
        if n_out > 0:   # every ray masked out: nothing to march
            launch(rays_mask, 0, terminate_planes)
        intervals.alloc_starts, samples.alloc_starts = intervals.chunk_starts, samples.chunk_starts
        intervals.compute_chunk_start()
        samples.compute_chunk_start()
    else:
        # count, allocate exactly, fill (grid.cu:441-507); note: rays_mask is NOT applied here
        if compute_intervals:
            intervals.chunk_cnts = torch.empty(n_rays, dtype=torch.int64, device=dev)
        if compute_samples:
            samples.chunk_cnts = torch.empty(n_rays, dtype=torch.int64, device=dev)
        launch(None, 1, None)
        if compute_intervals:
            intervals.memalloc_data_from_chunk(True, True)
        if compute_samples:
            samples.memalloc_data_from_chunk(False, False, True)
        n_out = (intervals.vals.numel() if compute_intervals else 0) + \
                (samples.vals.numel() if compute_samples else 0)
        if n_out > 0:   # with nothing to fill every ray is skipped (grid.cu:103-106): no launch needed
            launch(None, 0, terminate_planes)
    return intervals, samples, terminate_planes


_COARSE = {}
_COARSE_ON = os.environ.get("CNC_MARCH_COARSE", "1") == "1"      # measurement / test switch


def occupancy_coarse_bits(binaries):
    """(extension) the coarse occupancy of `binaries` [n_grids, rx, ry, rz] for the march (cnc_occupancy_coarse_bits: one
    bit per block of 4 x 4 x 4 cells), or None when the kernels take none for this shape.  Cached on the grid tensor
    (address, version, shape): the estimator replaces its grid at every occupancy update."""
    if not _COARSE_ON or binaries.dim() != 4 or binaries.dtype not in (torch.bool, torch.uint8):
        return None
    key = (binaries.data_ptr(), binaries._version, tuple(binaries.shape), str(binaries.device))
    hit = _COARSE.get(key)
    if hit is not None:
        return hit[1]
    L = _lib.lib()
    nw = int(L.cnc_occupancy_coarse_words(*[int(v) for v in binaries.shape]))
    words = None
    if nw:
        words = torch.empty(nw, dtype=torch.int32, device=binaries.device)
        check(L.cnc_occupancy_coarse_bits(ptr(binaries), *[int(v) for v in binaries.shape], ptr(words), stream(binaries.device)),
              "occupancy_coarse_bits")
    if len(_COARSE) >= 8:
        _COARSE.clear()
    _COARSE[key] = (binaries, words)        # (the grid is kept: its address stays unique while the entry lives)
    return words


def march_samples(rays_o, rays_d, rays_mask, binaries, aabbs, t_sorted, t_indices, hits, near_planes, far_planes,
                  step_size, cone_angle, traverse_steps_limit=-1, want_terminate_planes=False, clamped_total=None,
                  extras=None):
    """(extension) The march as the renderer consumes it — see cnc_march_samples in include/cnc_hip.h.
    Returns (ray_indices i64 [S], t_starts [S], t_ends [S], chunk_starts [n_rays], chunk_cnts [n_rays],
    terminate_planes or None).  Count pass, exclusive cumsum + ONE host sync (the sample total sizes the
    result, as in data_spec.hpp:86-96), fill pass.  `clamped_total` = {"at": w}: the same sync also brings
    sum(min(count, w)) back, under the key "total" (a caller that is about to take the first w samples of every ray).
    `extras` (dict, filled in place): what the fill pass emits besides — "positions": True -> [S,3] sample positions
    (o + d (t0 + t1) / 2, in the unit cube of extras["aabb"] (6 floats on the device) when given), "dirs": True ->
    [S,3] ray directions, "ray_indices": "int32" | None -> the ray ids as int32 / not at all (the first return value
    is then that tensor / None)."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("binaries", binaries), ("aabbs", aabbs),
                    ("t_sorted", t_sorted), ("t_indices", t_indices), ("hits", hits),
                    ("near_planes", near_planes), ("far_planes", far_planes)):
        check_input(t, name)
    if rays_mask is not None:
        check_input(rays_mask, "rays_mask")
    n_rays, dev = rays_o.shape[0], rays_o.device
    counts = torch.zeros(n_rays, dtype=torch.int64, device=dev)       # masked-out rays stay at 0
    term = torch.empty(n_rays, dtype=rays_o.dtype, device=dev) if want_terminate_planes else None
    L = _lib.lib()
    # where each ray's first sample was produced: left by the count pass, picked up by the fill pass, which then marches
    # only the span between a ray's first and last sample (CNC_MARCH_RESUME=0: both passes march the whole ray)
    resume = torch.empty((n_rays, 8), dtype=torch.int32, device=dev) if os.environ.get("CNC_MARCH_RESUME", "1") == "1" \
        else None
    ex = extras if extras is not None else {}
    ri_kind = ex.get("ray_indices", "int64")
    if ri_kind not in ("int64", "int32", None):
        raise RuntimeError("march_samples: extras['ray_indices'] must be 'int64', 'int32' or None")
    if ri_kind is None and not ex.get("positions"):
        raise RuntimeError("march_samples: without ray indices the fill pass must at least emit positions")
    box = ex.get("aabb")
    if box is not None:
        check_input(box, "extras['aabb']")
        if box.dtype != torch.float32 or box.numel() != 6:
            raise RuntimeError("march_samples: extras['aabb'] must be 6 float32 values on the device")

    coarse = occupancy_coarse_bits(binaries)      # empty blocks of 4^3 cells are skipped from LDS (same samples)

    def launch(starts, t0, t1, ri, tp, pos=None, dirs=None, ri32=None):
        rc = L.cnc_march_samples_coarse(ptr(rays_o), ptr(rays_d), ptr(rays_mask), n_rays, ptr(binaries), binaries.shape[0],
                                        binaries.shape[1], binaries.shape[2], binaries.shape[3], ptr(aabbs), ptr(hits),
                                        ptr(t_sorted), ptr(t_indices), ptr(near_planes), ptr(far_planes), float(step_size),
                                        float(cone_angle), int(traverse_steps_limit), ptr(counts), ptr(starts), ptr(t0),
                                        ptr(t1), ptr(ri), ptr(tp), ptr(resume), ptr(pos), ptr(dirs), ptr(ri32), ptr(box),
                                        ptr(coarse), stream(dev))
        check(rc, "march_samples")

    launch(None, None, None, None, term)
    ends = torch.cumsum(counts, 0)
    if clamped_total is not None and n_rays:
        total, clamped_total["total"] = torch.stack([ends[-1], counts.clamp(max=int(clamped_total["at"])).sum()]).tolist()
    else:
        total = int(ends[-1].item()) if n_rays else 0
    starts = ends - counts
    t_starts = torch.empty(total, dtype=torch.float32, device=dev)
    t_ends = torch.empty(total, dtype=torch.float32, device=dev)
    ray_indices = torch.empty(total, dtype=torch.int64, device=dev) if ri_kind == "int64" else None
    ri32 = torch.empty(total, dtype=torch.int32, device=dev) if ri_kind == "int32" else None
    pos = torch.empty((total, 3), dtype=torch.float32, device=dev) if ex.get("positions") else None
    dirs = torch.empty((total, 3), dtype=torch.float32, device=dev) if ex.get("dirs") else None
    if total:
        launch(starts, t_starts, t_ends, ray_indices, None, pos, dirs, ri32)
    if extras is not None:
        if ex.get("positions"):
            extras["positions"] = pos
        if ex.get("dirs"):
            extras["dirs"] = dirs
    return (ri32 if ri_kind == "int32" else ray_indices), t_starts, t_ends, starts, counts, term


def sample_positions(rays_o, rays_d, ray_indices, t_a, t_b=None, aabb=None, want_dirs=False):
    """(extension) positions [S,3] (and directions) of ray samples in one kernel; see
    cnc_sample_positions in include/cnc_hip.h."""
    for name, t in (("rays_o", rays_o), ("rays_d", rays_d), ("ray_indices", ray_indices), ("t_a", t_a)):
        check_input(t, name)
    if ray_indices.dtype != torch.int64 or rays_o.dtype != torch.float32 or t_a.dtype != torch.float32:
        raise RuntimeError("sample_positions: ray_indices must be int64, rays and t float32")
    S = ray_indices.shape[0]
    pos = torch.empty((S, 3), dtype=torch.float32, device=rays_o.device)
    dirs = torch.empty((S, 3), dtype=torch.float32, device=rays_o.device) if want_dirs else None
    if t_b is not None:
        check_input(t_b, "t_b")
    if aabb is not None:
        aabb = aabb.reshape(-1).to(torch.float32).contiguous()
        if aabb.numel() != 6:
            raise RuntimeError("sample_positions: aabb must hold 6 values")
    rc = _lib.lib().cnc_sample_positions(ptr(rays_o), ptr(rays_d), ptr(ray_indices), ptr(t_a), ptr(t_b),
                                         ptr(aabb), S, ptr(pos), ptr(dirs), stream(rays_o.device))
    check(rc, "sample_positions")
    return (pos, dirs) if want_dirs else pos


def _scan_checks(chunk_starts, chunk_cnts, inputs):
    check_input(chunk_starts, "chunk_starts")
    check_input(chunk_cnts, "chunk_cnts")
    check_input(inputs, "inputs")
    if chunk_starts.dim() != 1 or chunk_cnts.dim() != 1 or inputs.dim() != 1 \
            or chunk_starts.shape[0] != chunk_cnts.shape[0]:
        raise RuntimeError("Expected 1-D chunk_starts/chunk_cnts of equal length and 1-D inputs")


def _sum(fn_name, chunk_starts, chunk_cnts, inputs, normalize, backward):
    _scan_checks(chunk_starts, chunk_cnts, inputs)
    outputs = torch.empty_like(inputs)
    if inputs.shape[0] == 0:
        return outputs
    rc = getattr(_lib.lib(), fn_name)(ptr(chunk_starts), ptr(chunk_cnts), ptr(inputs), ptr(outputs),
                                      chunk_cnts.shape[0], inputs.shape[0], int(bool(normalize)),
                                      int(bool(backward)), stream(inputs.device))
    check(rc, fn_name)
    return outputs


def inclusive_sum(chunk_starts, chunk_cnts, inputs, normalize, backward):
    return _sum("cnc_inclusive_sum", chunk_starts, chunk_cnts, inputs, normalize, backward)


def exclusive_sum(chunk_starts, chunk_cnts, inputs, normalize, backward):
    return _sum("cnc_exclusive_sum", chunk_starts, chunk_cnts, inputs, normalize, backward)


def _prod_fwd(fn_name, chunk_starts, chunk_cnts, inputs):
    _scan_checks(chunk_starts, chunk_cnts, inputs)
    outputs = torch.empty_like(inputs)
    if inputs.shape[0] == 0:
        return outputs
    rc = getattr(_lib.lib(), fn_name)(ptr(chunk_starts), ptr(chunk_cnts), ptr(inputs), ptr(outputs),
                                      chunk_cnts.shape[0], inputs.shape[0], stream(inputs.device))
    check(rc, fn_name)
    return outputs


def inclusive_prod_forward(chunk_starts, chunk_cnts, inputs):
    return _prod_fwd("cnc_inclusive_prod_forward", chunk_starts, chunk_cnts, inputs)


def exclusive_prod_forward(chunk_starts, chunk_cnts, inputs):
    return _prod_fwd("cnc_exclusive_prod_forward", chunk_starts, chunk_cnts, inputs)


def _prod_bwd(fn_name, chunk_starts, chunk_cnts, inputs, outputs, grad_outputs):
    _scan_checks(chunk_starts, chunk_cnts, inputs)
    check_input(grad_outputs, "grad_outputs")
    grad_inputs = torch.empty_like(grad_outputs)
    if inputs.shape[0] == 0:
        return grad_inputs
    rc = getattr(_lib.lib(), fn_name)(ptr(chunk_starts), ptr(chunk_cnts), ptr(inputs),
                                      ptr(outputs.contiguous()), ptr(grad_outputs),
                                      ptr(grad_inputs), chunk_cnts.shape[0], inputs.shape[0],
                                      stream(inputs.device))
    check(rc, fn_name)
    return grad_inputs


def inclusive_prod_backward(chunk_starts, chunk_cnts, inputs, outputs, grad_outputs):
    return _prod_bwd("cnc_inclusive_prod_backward", chunk_starts, chunk_cnts, inputs, outputs,
                     grad_outputs)


def exclusive_prod_backward(chunk_starts, chunk_cnts, inputs, outputs, grad_outputs):
    return _prod_bwd("cnc_exclusive_prod_backward", chunk_starts, chunk_cnts, inputs, outputs,
                     grad_outputs)


def _rows(spec, name):
    """cnc_pdf_rows_t of a RaySegmentsSpec after the checks of data_spec.hpp:15-53: batched when vals has more than
    one axis (rows along the last), else flattened by chunk_starts / chunk_cnts."""
    if spec.vals is None:
        raise RuntimeError(f"{name}: vals must be defined")
    check_input(spec.vals, f"{name}.vals")
    if spec.vals.dtype != torch.float32:
        raise RuntimeError(f"{name}: vals must be float32")
    if spec.vals.dim() > 1:
        e = spec.vals.shape[-1]
        n_rays = spec.vals.numel() // e if e else int(torch.Size(spec.vals.shape[:-1]).numel())
        return _lib.PdfRows(spec._view(), n_rays, e, spec.vals.numel())
    if spec.chunk_starts is None or spec.chunk_cnts is None:
        raise RuntimeError(f"{name}: a flattened segment needs chunk_starts and chunk_cnts")
    for k in ("chunk_starts", "chunk_cnts", "ray_indices", "is_left", "is_right"):
        t = getattr(spec, k)
        if t is not None:
            check_input(t, f"{name}.{k}")
            if t.dim() != 1:
                raise RuntimeError(f"{name}.{k} must be 1-D")
    if spec.chunk_starts.numel() != spec.chunk_cnts.numel():
        raise RuntimeError(f"{name}: chunk_starts and chunk_cnts differ in length")
    if spec.chunk_starts.dtype != torch.int64 or spec.chunk_cnts.dtype != torch.int64:
        raise RuntimeError(f"{name}: chunk_starts and chunk_cnts must be int64")
    if spec.ray_indices is not None and (spec.ray_indices.numel() != spec.vals.numel()
                                         or spec.ray_indices.dtype != torch.int64):
        raise RuntimeError(f"{name}: ray_indices must be int64 with one entry per value")
    return _lib.PdfRows(spec._view(), spec.chunk_cnts.numel(), -1, spec.vals.numel())


def importance_sampling(ray_segments, cdfs, n_intervals_per_ray, stratified, jitter=None):
    """pdf.cu:294-424 -> [intervals, samples] (RaySegmentsSpec), one launch of cnc_importance_sampling.  An int
    n gives batched outputs ((..., n) and (..., n + 1), or (n_rays, n) for a flattened input) with no host
    synchronisation; a tensor [n_rays] gives flattened outputs sized by one host read of the two totals.
    stratified: one bias per ray drawn here with torch.rand on the device ([0, 1); the reference draws (0, 1] from
    its Philox stream inside the kernel); `jitter` (extension) supplies that f32 [n_rays] bias instead."""
    seg = _rows(ray_segments, "ray_segments")
    check_input(cdfs, "cdfs")
    if cdfs.dtype != torch.float32 or cdfs.numel() != ray_segments.vals.numel():
        raise RuntimeError("importance_sampling: cdfs must be float32 with one value per edge")
    dev = cdfs.device
    n_rays = seg.n_rays
    if jitter is None and stratified:
        jitter = torch.rand(n_rays, dtype=torch.float32, device=dev)
    if jitter is not None:
        check_input(jitter, "jitter")
        if jitter.dtype != torch.float32 or jitter.numel() != n_rays:
            raise RuntimeError("importance_sampling: jitter must be float32 [n_rays]")
    samples, intervals = RaySegmentsSpec(), RaySegmentsSpec()
    if isinstance(n_intervals_per_ray, torch.Tensor):
        check_input(n_intervals_per_ray, "n_intervals_per_ray")
        if n_intervals_per_ray.numel() != n_rays:
            raise RuntimeError("importance_sampling: n_intervals_per_ray must hold one count per ray")
        cnt = n_intervals_per_ray.reshape(-1).to(torch.int64)
        samples.chunk_cnts = cnt
        intervals.chunk_cnts = (cnt + 1) * (cnt > 0)
        ends_s, ends_i = torch.cumsum(samples.chunk_cnts, 0), torch.cumsum(intervals.chunk_cnts, 0)
        # the one host read (data_spec.hpp:86-96 makes it once per allocation; here both totals come together)
        n_s, n_i = torch.stack([ends_s[-1], ends_i[-1]]).tolist() if n_rays else (0, 0)
        samples.chunk_starts, intervals.chunk_starts = ends_s - samples.chunk_cnts, ends_i - intervals.chunk_cnts
        samples.memalloc_data(n_s, alloc_masks=False, zero_init=False)
        intervals.memalloc_data(n_i, alloc_masks=True, zero_init=False)
        smp_rows = _lib.PdfRows(samples._view(), n_rays, -1, n_s)
        itv_rows = _lib.PdfRows(intervals._view(), n_rays, -1, n_i)
    else:
        n = int(n_intervals_per_ray)
        if n < 0:
            raise RuntimeError("importance_sampling: n_intervals_per_ray must be >= 0")
        lead = list(ray_segments.vals.shape[:-1]) if ray_segments.vals.dim() > 1 else [n_rays]
        samples.vals = torch.empty(lead + [n], dtype=torch.float32, device=dev)
        intervals.vals = torch.empty(lead + [n + 1], dtype=torch.float32, device=dev)
        smp_rows = _lib.PdfRows(samples._view(), n_rays, n, samples.vals.numel())
        itv_rows = _lib.PdfRows(intervals._view(), n_rays, n + 1, intervals.vals.numel())
    if n_rays:
        rc = _lib.lib().cnc_importance_sampling(C.byref(seg), ptr(cdfs), ptr(jitter), C.byref(smp_rows),
                                                C.byref(itv_rows), stream(dev))
        check(rc, "importance_sampling")
    return [intervals, samples]


def searchsorted(query, key):
    """pdf.cu:424-456 -> [ids_left, ids_right] i64 shaped like query.vals: key[left] <= query < key[right] in the
    key segment of each query entry's ray, clamped to it; ids local to the row for a batched query, global for a
    flattened one (see cnc_searchsorted)."""
    q, k = _rows(query, "query"), _rows(key, "key")
    if q.n_edges_per_ray >= 0 and k.n_rays < q.n_rays:
        raise RuntimeError("searchsorted: the key has fewer rays than the batched query has rows")
    ids_left = torch.empty(query.vals.shape, dtype=torch.int64, device=query.vals.device)
    ids_right = torch.empty(query.vals.shape, dtype=torch.int64, device=query.vals.device)
    if q.n_edges:
        rc = _lib.lib().cnc_searchsorted(C.byref(q), C.byref(k), ptr(ids_left), ptr(ids_right),
                                         stream(query.vals.device))
        check(rc, "searchsorted")
    return [ids_left, ids_right]


def _shared_row(params):
    """True when `params` is one coefficient row seen through a broadcast: every axis in front of the last has stride 0
    (or one entry), as `torch.broadcast_to(row, batch + (N,))` leaves it.  Such a tensor is handed to the kernel as ONE row
    (param_stride 0) instead of being made contiguous."""
    return params.stride(-1) == 1 and all(st == 0 or sz == 1 for sz, st in zip(params.shape[:-1], params.stride()[:-1]))


def _undistort(name, uv, params, layouts):
    """Host checks of camera.cu:114-183: CHECK_INPUT on both, equal dimensionality, uv [..., 2], the row length.
    -> (number of points, param_stride)."""
    check_input(uv, "uv")
    _lib.check_cuda(params, "params")
    shared = params.numel() > 0 and _shared_row(params)
    if not shared:
        check_input(params, "params")
    if uv.dim() != params.dim():
        raise RuntimeError(f"{name}: uv and params must have the same number of dimensions")
    if uv.dim() < 1 or uv.shape[-1] != 2:
        raise RuntimeError("uv must have shape [..., 2]")
    if params.shape[-1] not in layouts:
        raise RuntimeError(f"{name}: params must have shape [..., {' | '.join(str(n) for n in layouts)}]")
    if uv.dtype != torch.float32 or params.dtype != torch.float32:
        raise RuntimeError(f"{name}: uv and params must be float32")
    n = uv.numel() // 2
    if not shared and params.numel() != n * params.shape[-1]:
        raise RuntimeError(f"{name}: params must hold one row per point")
    return n, (0 if shared else params.shape[-1])


def opencv_lens_undistortion(uv, params, eps, iters):
    """camera.cu:114-147 -> uv_out shaped like uv.  params [..., 5 | 8 | 12]: k1 k2 p1 p2 k3 [k4 k5 k6], or k1..k6 p1 p2
    s1..s4.  A broadcast view of one row (see `_shared_row`) is read as one row; anything else must be contiguous."""
    n, stride = _undistort("opencv_lens_undistortion", uv, params, (5, 8, 12))
    out = torch.empty_like(uv)
    rc = _lib.lib().cnc_lens_undistort(ptr(uv), ptr(params), stride, params.shape[-1], float(eps), int(iters), ptr(out), n,
                                       stream(uv.device))
    check(rc, "opencv_lens_undistortion")
    return out


def opencv_lens_undistortion_fisheye(uv, params, eps, iters):
    """camera.cu:149-183 -> uv_out shaped like uv.  params [..., 4] = k1..k4.  A point that does not converge returns its
    input (the reference leaves that element of its output uninitialised)."""
    n, stride = _undistort("opencv_lens_undistortion_fisheye", uv, params, (4,))
    out = torch.empty_like(uv)
    rc = _lib.lib().cnc_lens_undistort_fisheye(ptr(uv), ptr(params), stride, float(eps), int(iters), ptr(out), n,
                                               stream(uv.device))
    check(rc, "opencv_lens_undistortion_fisheye")
    return out
