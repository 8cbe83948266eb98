"""Connected components of a 3-D lattice and of a triangle list on the device — an extension, the
reference has nothing like it.  The consumers: pruning floaters from the occupancy grid (`OccGridEstimator.
prune_small_components`, `Trainer.prune_floaters`), from the lattice a mesh is cut from (`extract_mesh(...,
min_component_points=N)`), and counting a mesh's components (`Mesh.components(on_device=True)`).

A component's label is the smallest linear index of its cells, `(i0 * d1 + i1) * d2 + i2` within its grid, so the labels
are unique: they depend on the mask and the neighbourhood and on nothing else.  Three neighbourhoods:

    6    face neighbours
    26   face, edge and corner neighbours
    14   the Kuhn neighbourhood: plus and minus the seven `cnc_amd.mesh.DIRECTIONS`, the offsets whose non-zero components
         all have one sign — (+1, +1, +1) joins, (+1, +1, -1) does not.  These are exactly the lattice edges marching
         tetrahedra cuts, so "one component" means here what the mesh means by it

The labelling, the sizes and the graph labelling are HIP kernels (csrc/components.hip); the gather / compare / argmax glue
of `prune_small` is torch ops.  No CPU fallback.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

CONNECTIVITIES = (6, 14, 26)


def _as_grids(mask: torch.Tensor, name: str = "mask") -> torch.Tensor:
    """`mask` as a contiguous uint8 [n_grids, d0, d1, d2] view (a bool tensor's bytes are 0 / 1: no copy)."""
    from ._lib import check_cuda
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    check_cuda(mask, name)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{name}: expected a bool or uint8 tensor, got {mask.dtype}")
    if mask.dim() not in (3, 4):
        raise RuntimeError(f"{name}: expected 3 or 4 dimensions ([d0, d1, d2] or [n_grids, d0, d1, d2]), got {mask.dim()}")
    if min(mask.shape) < 1:
        raise RuntimeError(f"{name}: a grid of shape {tuple(mask.shape)} has no cells")
    m = mask.contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    return m if m.dim() == 4 else m.unsqueeze(0)


def _check_connectivity(connectivity) -> int:
    if connectivity not in CONNECTIVITIES:
        raise RuntimeError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")
    return int(connectivity)


@torch.no_grad()
def label_grid(mask: torch.Tensor, connectivity: int = 26) -> torch.Tensor:
    """int32 labels of `mask`'s shape (bool or uint8, [d0, d1, d2] or [n_grids, d0, d1, d2], every grid on its own): a set
    cell gets the smallest linear index within its grid of any cell of its component, an unset cell -1."""
    from .backends import components as _C
    connectivity = _check_connectivity(connectivity)
    grids = _as_grids(mask)
    labels = torch.empty(grids.shape, dtype=torch.int32, device=grids.device)
    _C.label_grid(grids, connectivity, labels)
    return labels.view(mask.shape)


def _sizes(labels4: torch.Tensor) -> torch.Tensor:
    from .backends import components as _C
    out = torch.empty_like(labels4)
    _C.sizes(labels4, out)
    return out


@torch.no_grad()
def component_sizes(labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(roots int64 [K] ascending, sizes int64 [K]) of the labels `label_grid` gave: every component's root — its label, as
    an index into the flattened `labels` (for [n_grids, ...] labels that is grid * cells + label) — and its cell count."""
    from .backends import components as _C
    _C.check_input(labels, "labels")
    if labels.dtype != torch.int32 or labels.dim() not in (3, 4):
        raise RuntimeError("labels: expected the int32 tensor of label_grid, 3-D or 4-D")
    sizes = _sizes(labels if labels.dim() == 4 else labels.unsqueeze(0)).view(-1)
    roots = sizes.nonzero().view(-1)
    return roots, sizes[roots].to(torch.int64)


@torch.no_grad()
def prune_small(mask: torch.Tensor, min_cells: int, connectivity: int = 26) -> Tuple[torch.Tensor, Dict[str, int]]:
    """(pruned bool mask of `mask`'s shape, stats): the components with fewer than `min_cells` cells cleared.  The largest
    component of every grid is always kept (of several largest ones, the one with the smallest root), so `min_cells <= 1`
    removes nothing and no `min_cells` empties a grid.  stats: `components` and `cells` before, `removed_components` and
    `removed_cells`, summed over the grids.  One host read, for the stats."""
    labels = label_grid(mask, connectivity)
    labels4 = labels if labels.dim() == 4 else labels.unsqueeze(0)
    n, cells = labels4.shape[0], labels4[0].numel()
    flat = labels4.view(n, cells)
    sizes = _sizes(labels4).view(n, cells).to(torch.int64)
    # the largest component, a tie to the smaller root: every key is distinct, so the argmax is unambiguous
    order = torch.arange(cells - 1, -1, -1, dtype=torch.int64, device=flat.device)
    best = torch.argmax(sizes * cells + order, dim=1, keepdim=True)
    keep = sizes >= int(min_cells)
    keep.scatter_(1, best, True)
    is_set = flat >= 0
    pruned = is_set & keep.gather(1, flat.clamp(min=0).to(torch.int64))
    gone = (sizes > 0) & ~keep
    counts = torch.stack([(sizes > 0).sum(), sizes.sum(), gone.sum(), (sizes * gone).sum()]).tolist()
    stats = dict(zip(("components", "cells", "removed_components", "removed_cells"), (int(v) for v in counts)))
    return pruned.view(mask.shape), stats


@torch.no_grad()
def label_graph(faces: torch.Tensor, n_vertices: int) -> torch.Tensor:
    """int32 [n_vertices]: the smallest vertex index of every vertex's component under the edges of `faces` (int32 [F, 3]);
    a vertex no face uses keeps its own index."""
    from .backends import components as _C
    _C.check_input(faces, "faces")
    labels = torch.empty(int(n_vertices), dtype=torch.int32, device=faces.device)
    _C.label_graph(faces, n_vertices, labels)
    return labels
