"""Mesh export: the iso-surface of a density field as an indexed triangle mesh — an extension, the
reference has no exporter.

Marching tetrahedra over the Kuhn split of every lattice cell: six tetrahedra per cell, all of them around the cell's
main diagonal, so that neighbouring cells split their shared face the same way and the surface is watertight by
construction.  The (tetrahedron, mask) -> triangles table is generated here (`tet_table`) and handed to the kernels
(csrc/iso_surface.hip) as a device buffer; classification, compaction and emission run on the device, the two prefix
sums and the `nonzero` of the occupancy skip are torch ops.  One host read sizes the outputs.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch

# the seven edge directions out of a lattice point: an edge belongs to its lower end, its OWNER
DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
# the six tetrahedra of a cell: the axis permutations in lexicographic order
PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TABLE_ROW = 7            # int8 per (tetrahedron, mask): the triangle count, then 3 codes per triangle (-1: unused)
MAX_POINTS = 2 ** 31     # the lattice, V and 3 F must each stay below it


def tet_vertices(tet: int):
    """Local vertices v0..v3 of tetrahedron `tet` in the unit cell: v0 = (0,0,0), v1 = v0 + e_p1, v2 = v1 + e_p2,
    v3 = (1,1,1)."""
    p = PERMUTATIONS[tet]
    v = [[0, 0, 0]]
    for axis in p:
        nxt = list(v[-1])
        nxt[axis] += 1
        v.append(nxt)
    return v


def _mask_triangles(verts, mask):
    """Triangles of one (tetrahedron, mask) as triples of local edges (i, j), i < j, wound counter-clockwise seen from the
    low-density side."""
    inside = [k for k in range(4) if mask >> k & 1]
    outside = [k for k in range(4) if not mask >> k & 1]
    if not inside or not outside:
        return []
    if len(inside) == 1 or len(outside) == 1:
        lone, rest = (inside[0], outside) if len(inside) == 1 else (outside[0], inside)
        tris = [[(lone, r) for r in rest]]
    else:
        (i0, i1), (o0, o1) = inside, outside
        q = [(i0, o0), (i0, o1), (i1, o1), (i1, o0)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    # orientation in integers: edge midpoints x 2, the centroids' difference x |inside| |outside|
    ref = [len(inside) * sum(verts[k][a] for k in outside) - len(outside) * sum(verts[k][a] for k in inside) for a in range(3)]
    out = []
    for tri in tris:
        a, b, c = ([verts[i][x] + verts[j][x] for x in range(3)] for i, j in tri)
        u, w = [b[x] - a[x] for x in range(3)], [c[x] - a[x] for x in range(3)]
        n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        dot = sum(n[x] * ref[x] for x in range(3))
        assert dot != 0
        out.append([tuple(sorted(e)) for e in (tri if dot > 0 else [tri[0], tri[2], tri[1]])])
    return out


def tet_table() -> np.ndarray:
    """int8 [6, 16, 7]: row (tetrahedron, mask) = the triangle count (0, 1 or 2), then three codes per triangle.  A code
    names the lattice edge that carries the triangle's vertex, relative to the cell: `corner * 8 + direction`, `corner` =
    dx | dy << 1 | dz << 2 the edge's owner among the cell's corners, `direction` an index into DIRECTIONS."""
    table = np.full((6, 16, TABLE_ROW), -1, np.int8)
    for tet in range(6):
        verts = tet_vertices(tet)
        for mask in range(16):
            tris = _mask_triangles(verts, mask)
            table[tet, mask, 0] = len(tris)
            for t, tri in enumerate(tris):
                for e, (i, j) in enumerate(tri):
                    owner, d = verts[i], tuple(verts[j][x] - verts[i][x] for x in range(3))
                    table[tet, mask, 1 + 3 * t + e] = (owner[0] | owner[1] << 1 | owner[2] << 2) * 8 + DIRECTIONS.index(d)
    return table


def lattice_cells(aabb, resolution: int) -> Tuple[int, int, int]:
    """(nx, ny, nz): `resolution` cells along the box's longest side, max(1, round(resolution * extent / longest)) along
    the others."""
    box = [float(v) for v in (aabb.tolist() if hasattr(aabb, "tolist") else aabb)]
    if len(box) != 6:
        raise ValueError("aabb: expected 6 numbers (x0, y0, z0, x1, y1, z1)")
    ext = [box[3 + a] - box[a] for a in range(3)]
    if not all(math.isfinite(e) and e > 0 for e in ext):
        raise ValueError(f"aabb: expected a box with a positive, finite extent, got {box}")
    if int(resolution) < 1:
        raise ValueError(f"resolution must be at least 1, got {resolution}")
    longest = max(ext)
    return tuple(max(1, int(round(int(resolution) * e / longest))) for e in ext)


def check_lattice(n) -> int:
    """The point count of an (nx, ny, nz)-cell lattice; refuses one of 2^31 points or more."""
    points = (int(n[0]) + 1) * (int(n[1]) + 1) * (int(n[2]) + 1)
    if min(n) < 1:
        raise ValueError(f"a lattice needs at least one cell per axis, got {tuple(n)}")
    if points >= MAX_POINTS:
        raise ValueError(f"a lattice of {tuple(n)} cells has {points} points: the limit is 2^31 - 1")
    return points


def resolve_threshold(threshold, render_step_size) -> float:
    """`threshold`, or for None the density at which one render step is half opaque, ln 2 / render_step_size — a default
    that scales with the scene and that nobody has tuned."""
    if threshold is None:
        if render_step_size is None:
            raise ValueError("threshold=None needs render_step_size: the default is ln 2 / render_step_size")
        if not float(render_step_size) > 0:
            raise ValueError(f"render_step_size must be positive, got {render_step_size}")
        threshold = math.log(2.0) / float(render_step_size)
    threshold = float(np.float32(threshold))
    if not (math.isfinite(threshold) and threshold > 0):
        raise ValueError(f"threshold must be positive and finite, got {threshold}")
    return threshold


def spacing(aabb, n):
    """(lo, h) as float32[3]: h = (hi - lo) / n in float32."""
    box = np.asarray(aabb.tolist() if hasattr(aabb, "tolist") else aabb, np.float32)
    lo, hi = box[:3].copy(), box[3:]
    return lo, ((hi - lo) / np.asarray(n, np.float32)).astype(np.float32)


@dataclass
class Mesh:
    vertices: torch.Tensor                      # float32 [V, 3]
    faces: torch.Tensor                         # int32 [F, 3], counter-clockwise seen from the low-density side
    normals: Optional[torch.Tensor] = None      # float32 [V, 3], unit length or zero
    colors: Optional[torch.Tensor] = None       # uint8 [V, 3]

    def save(self, path: str) -> None:
        """Binary little-endian PLY: x y z [nx ny nz] [red green blue] per vertex, `list uchar int vertex_indices` per
        face."""
        host = lambda t: t.detach().cpu().numpy()
        v = host(self.vertices).astype("<f4")
        fields, cols = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], [v[:, 0], v[:, 1], v[:, 2]]
        if self.normals is not None:
            nrm = host(self.normals).astype("<f4")
            fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
            cols += [nrm[:, 0], nrm[:, 1], nrm[:, 2]]
        if self.colors is not None:
            rgb = host(self.colors).astype(np.uint8)
            fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
            cols += [rgb[:, 0], rgb[:, 1], rgb[:, 2]]
        rec = np.empty(v.shape[0], dtype=fields)
        for (name, _), col in zip(fields, cols):
            rec[name] = col
        f = host(self.faces).astype("<i4")
        frec = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
        frec["n"] = 3
        frec["i"] = f
        kind = {"<f4": "float", "u1": "uchar"}
        head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
        head += [f"property {kind[t]} {name}" for name, t in fields]
        head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
        with open(path, "wb") as fh:
            fh.write(("\n".join(head) + "\n").encode("ascii"))
            fh.write(rec.tobytes())
            fh.write(frec.tobytes())

    def components(self, on_device: bool = False) -> np.ndarray:
        """Face count of every connected component, largest first (a floater is a small closed component).  A union-find
        on the host, over the vertices: roots hooked under the smaller root, paths halved until nothing moves.
        on_device=True: the same array from the device's union-find (`cnc_amd.components.label_graph`) and a bincount of
        the label of every face's first vertex; the faces stay where they are."""
        if on_device:
            from .components import label_graph
            if self.faces.shape[0] == 0:
                return np.zeros(0, np.int64)
            labels = label_graph(self.faces.contiguous(), int(self.vertices.shape[0]))
            counts = torch.bincount(labels[self.faces[:, 0].to(torch.int64)].to(torch.int64))
            counts = counts[counts > 0].cpu().numpy()
            return np.sort(counts)[::-1].astype(np.int64)
        f = self.faces.detach().cpu().numpy().astype(np.int64)
        if f.shape[0] == 0:
            return np.zeros(0, np.int64)
        parent = np.arange(int(self.vertices.shape[0]), dtype=np.int64)
        u, w = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
        while True:
            pu, pw = parent[u], parent[w]
            apart = pu != pw
            if not apart.any():
                break
            np.minimum.at(parent, np.maximum(pu, pw)[apart], np.minimum(pu, pw)[apart])
            while True:
                up = parent[parent]
                if np.array_equal(up, parent):
                    break
                parent = up
        _, counts = np.unique(parent[f[:, 0]], return_counts=True)
        return np.sort(counts)[::-1].astype(np.int64)


def _empty(device, normals: bool) -> Mesh:
    return Mesh(torch.zeros((0, 3), dtype=torch.float32, device=device), torch.zeros((0, 3), dtype=torch.int32, device=device),
                torch.zeros((0, 3), dtype=torch.float32, device=device) if normals else None)


_POPCOUNT = np.asarray([bin(m).count("1") for m in range(256)], np.uint8)


@torch.no_grad()
def extract_mesh(density: Union[Callable, torch.Tensor], aabb, resolution: int = 256, threshold: Optional[float] = None, *,
                 occupancy: Optional[torch.Tensor] = None, cap: bool = True, normals: bool = True,
                 render_step_size: Optional[float] = None, chunk: int = 1 << 20, device=None, return_lattice: bool = False,
                 min_component_points: int = 0):
    """The surface `density == threshold` inside the box `aabb` as a Mesh (tensors on the device).

    density      a callable [M, 3] -> [M] or [M, 1] (evaluated in chunks of `chunk` points, without gradients), or a ready
                 float32 device lattice [nz + 1, ny + 1, nx + 1] (then `resolution` is not used; it is not modified)
    resolution   cells along the box's longest side (`lattice_cells`)
    threshold    > 0 and finite; None: ln 2 / render_step_size, the density at which one render step is half opaque —
                 a default that scales with the scene and has not been tuned
    occupancy    bool [Gx, Gy, Gz] over the same box: a lattice point is evaluated only if an occupancy cell that overlaps
                 [p - h, p + h] is set, every other point gets density 0 (a callable only)
    cap          lattice points on the box's boundary get density 0, so that surfaces close at the box
    normals      also the unit normals, from the lattice's differences
    device       of a callable's lattice; default: the occupancy grid's, else the current GPU
    return_lattice   debugging: return (mesh, the float32 lattice the mesh was cut from, capping applied)
    min_component_points   > 0: prune floaters before the surface is cut.  The inside set — the lattice points with
                 density >= threshold (NaN is outside), the box's boundary excluded under `cap` — is labelled with the Kuhn
                 neighbourhood (connectivity 14: the lattice edges marching tetrahedra cuts), and the points
                 of every component with fewer points get density 0; the largest component always stays.  The mesh is
                 watertight as before, and a returned lattice is the pruned one.  A cavity inside the object is a
                 component of the OUTSIDE set and is left alone.  0 (default): off, nothing more is called.  Untuned
    """
    from .backends import iso_surface as iso
    if int(min_component_points) < 0:
        raise ValueError(f"min_component_points must not be negative, got {min_component_points}")
    threshold = resolve_threshold(threshold, render_step_size)
    ready = isinstance(density, torch.Tensor)
    if ready:
        if density.dim() != 3 or density.dtype != torch.float32:
            raise ValueError("density: a ready lattice is a float32 tensor [nz + 1, ny + 1, nx + 1]")
        if occupancy is not None:
            raise ValueError("occupancy skips evaluations of a callable density; a ready lattice has none to skip")
        n = (density.shape[2] - 1, density.shape[1] - 1, density.shape[0] - 1)
        lattice_cells(aabb, 1)
    else:
        if not callable(density):
            raise TypeError("density: expected a callable or a float32 lattice")
        n = lattice_cells(aabb, resolution)
    points = check_lattice(n)
    if int(chunk) < 1:
        raise ValueError(f"chunk must be at least 1, got {chunk}")
    lo, h = spacing(aabb, n)

    if ready:
        iso.check_cuda(density, "density")
        D = density.contiguous().clone()
        device = D.device
    else:
        if device is None:
            device = occupancy.device if occupancy is not None else torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("extract_mesh runs on the GPU (the HIP extension has no CPU fallback)")
        D = torch.zeros((n[2] + 1, n[1] + 1, n[0] + 1), dtype=torch.float32, device=device)
        flat = D.view(-1)
        lin = None
        total = points
        if occupancy is not None:
            if occupancy.dim() != 3 or occupancy.dtype != torch.bool:
                raise ValueError("occupancy: expected a bool tensor [Gx, Gy, Gz]")
            active = torch.empty(points, dtype=torch.uint8, device=device)
            iso.active_points(occupancy.contiguous(), n, active)
            lin = active.nonzero().view(-1)
            del active
            total = int(lin.numel())
        pos = torch.empty((min(int(chunk), max(total, 1)), 3), dtype=torch.float32, device=device)
        for first in range(0, total, int(chunk)):
            m = min(int(chunk), total - first)
            piece = None if lin is None else lin[first:first + m]
            iso.lattice_positions(piece, first, m, n, lo, h, pos[:m])
            val = density(pos[:m])
            if val.numel() != m:
                raise RuntimeError(f"density: expected {m} values for {m} points, got a tensor of shape {tuple(val.shape)}")
            val = val.reshape(m).to(torch.float32)
            if piece is None:
                flat[first:first + m] = val
            else:
                flat[piece] = val
        del pos, lin

    if int(min_component_points) > 0:
        from .components import prune_small
        inside = D >= threshold
        if cap:
            for axis in range(3):
                inside.select(axis, 0).fill_(False)
                inside.select(axis, -1).fill_(False)
        kept, _ = prune_small(inside, int(min_component_points), connectivity=14)
        D.masked_fill_(inside & ~kept, 0.0)
        del inside, kept

    table = torch.from_numpy(tet_table().reshape(-1)).to(device)
    edge_mask = torch.empty(points, dtype=torch.uint8, device=device)
    cell_tris = torch.empty(n[0] * n[1] * n[2], dtype=torch.uint8, device=device)
    iso.classify(D, n, threshold, cap, table, edge_mask, cell_tris)
    per_point = torch.from_numpy(_POPCOUNT).to(device).index_select(0, edge_mask.to(torch.int32))
    n_vertices, n_faces = torch.stack([per_point.sum(dtype=torch.int64), cell_tris.sum(dtype=torch.int64)]).tolist()
    if n_vertices >= MAX_POINTS or 3 * n_faces >= MAX_POINTS:
        raise ValueError(f"the mesh would have {n_vertices} vertices and {n_faces} faces: V and 3 F must stay below 2^31; "
                         "lower the resolution")
    if n_vertices == 0 or n_faces == 0:
        mesh = _empty(device, normals)
        return (mesh, D) if return_lattice else mesh
    vertex_scan = torch.cumsum(per_point, 0, dtype=torch.int32).sub_(per_point)
    del per_point
    cell_scan = torch.cumsum(cell_tris, 0, dtype=torch.int32).sub_(cell_tris)
    vertices = torch.empty((n_vertices, 3), dtype=torch.float32, device=device)
    nrm = torch.empty((n_vertices, 3), dtype=torch.float32, device=device) if normals else None
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=device)
    iso.emit_vertices(D, n, threshold, lo, h, edge_mask, vertex_scan, vertices, nrm)
    iso.emit_faces(D, n, threshold, table, edge_mask, vertex_scan, cell_tris, cell_scan, n_vertices, faces)
    mesh = Mesh(vertices, faces, nrm)
    return (mesh, D) if return_lattice else mesh


@torch.no_grad()
def field_mesh(field, aabb, occupancy, render_step_size, resolution: int = 256, threshold: Optional[float] = None,
               colors: bool = True, chunk: int = 1 << 20, return_lattice: bool = False, min_component_points: int = 0):
    """The mesh of a radiance field as its renderer sees it: `field.query_density` on the lattice points the occupancy
    grid does not rule out, the default threshold from `render_step_size`, and (colors=True) one call of the field on the
    vertices with view direction -normal, as uint8.  min_component_points: `extract_mesh`'s.  Bounded fields only."""
    if getattr(field, "unbounded", False):
        raise ValueError("mesh export needs a bounded field: an unbounded field (unbounded=True) has no box to march")
    threshold = resolve_threshold(threshold, render_step_size)
    check_lattice(lattice_cells(aabb, resolution))
    was_training = field.training
    field.eval()
    try:
        out = extract_mesh(lambda x: field.query_density(x), aabb, resolution, threshold, occupancy=occupancy, chunk=chunk,
                           device=aabb.device if isinstance(aabb, torch.Tensor) else None, return_lattice=return_lattice,
                           min_component_points=min_component_points)
        mesh = out[0] if return_lattice else out
        if colors:
            V = int(mesh.vertices.shape[0])
            mesh.colors = torch.empty((V, 3), dtype=torch.uint8, device=mesh.vertices.device)
            for first in range(0, V, int(chunk)):
                x = mesh.vertices[first:first + int(chunk)]
                rgb, _ = field(x, -mesh.normals[first:first + int(chunk)])
                mesh.colors[first:first + int(chunk)] = (rgb.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8)
    finally:
        field.train(was_training)
    return out
