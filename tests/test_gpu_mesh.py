"""The mesh export's kernels (csrc/iso_surface.hip) against the float32 NumPy twin (tests/mesh_twin.py):
vertices and normals bit for bit and in order, faces after rotating each triangle to its smallest index first and sorting;
the occupancy skip, empty results, the kernels' footprint under three sentinel fills, and run-to-run identity.

NaN vertices (an edge with a NaN or an infinite end: t = inf / inf) are compared by position, not by payload: which NaN
inf - inf gives is the hardware's choice (x86 SSE and gfx950 differ in its sign), every other value bit for bit."""
import numpy as np
import pytest
import torch

import mesh_twin as T
from guarded import Guarded, moved_with_fill, same_bits, under_fills

pytestmark = pytest.mark.gpu

UNIT = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
SMOOTH_BOX = ([-1.0, -0.5, -0.6], [1.0, 0.5, 0.6])
# name -> (lattice, box, threshold)
CASES = {
    "noise_4x5x6": (lambda: T.noise_lattice((4, 5, 6), 11), UNIT, 0.5),
    "noise_9x9x9": (lambda: T.noise_lattice((9, 9, 9), 12), UNIT, 0.5),          # visits all 84 pairs (test_mesh_twin.py)
    "ties_9x9x9": (lambda: T.tie_lattice((9, 9, 9), 14), UNIT, 0.5),
    "smooth_33x17x20": (lambda: T.smooth_lattice((33, 17, 20)), SMOOTH_BOX, 1.0),
    "nan_inf_7x6x5": (lambda: T.special_lattice((7, 6, 5), 31), UNIT, 0.5),
    "one_cell": (lambda: T.noise_lattice((1, 1, 1), 5), UNIT, 0.5),
    "cells_1x1x7": (lambda: T.noise_lattice((1, 1, 7), 6), UNIT, 0.5),
}
_twins = {}


def twin_of(name, cap):
    """(lattice, vertices, faces, normals) of a case, computed once and never changed."""
    if (name, cap) not in _twins:
        make, box, thr = CASES[name]
        D = make()
        v, f, nrm = T.extract(D, box[0], box[1], thr, cap=cap)
        for a in (D, v, f, nrm):
            a.setflags(write=False)
        _twins[name, cap] = (D, v, f, nrm)
    return _twins[name, cap]


def same_floats(got, want, nan_by_position=False):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    if not nan_by_position:
        return same_bits(got, want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    keep = ~np.isnan(want)
    return same_bits(got[keep], want[keep])


def assert_is_twin(mesh, v, f, nrm, nan_by_position=False):
    assert same_floats(mesh.vertices, v, nan_by_position), "vertices differ from the twin"
    if nrm is None:
        assert mesh.normals is None
    else:
        assert same_floats(mesh.normals, nrm, nan_by_position), "normals differ from the twin"
    assert mesh.faces.dtype == torch.int32 and tuple(mesh.faces.shape) == f.shape
    assert np.array_equal(T.canonical_faces(mesh.faces.cpu().numpy()), T.canonical_faces(f)), "faces differ from the twin"


@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no_normals"])
@pytest.mark.parametrize("cap", [True, False], ids=["cap", "no_cap"])
@pytest.mark.parametrize("name", list(CASES))
def test_ready_lattice_against_the_twin(cuda, name, cap, normals):
    from cnc_amd.mesh import extract_mesh
    D, v, f, nrm = twin_of(name, cap)
    _, box, thr = CASES[name]
    given = torch.from_numpy(D.copy()).to(cuda)
    mesh, lattice = extract_mesh(given, box[0] + box[1], threshold=thr, cap=cap, normals=normals, return_lattice=True)
    assert same_bits(given, D), "the caller's lattice was modified"
    assert same_bits(lattice, T.capped(D) if cap else D)                        # the capping, applied in place to the copy
    assert_is_twin(mesh, v, f, nrm if normals else None, nan_by_position=name.startswith("nan_inf"))
    if name in ("one_cell", "cells_1x1x7") and cap:
        assert v.shape[0] == 0                 # every point is on the boundary
    elif not name.startswith("nan_inf"):
        assert v.shape[0] > 0 and (not cap or T.is_directed_manifold(mesh.faces.cpu().numpy(), v.shape[0]))


def test_two_runs_give_identical_bytes(cuda):
    from cnc_amd.mesh import extract_mesh
    D = torch.from_numpy(twin_of("smooth_33x17x20", True)[0].copy()).to(cuda)
    a = extract_mesh(D, SMOOTH_BOX[0] + SMOOTH_BOX[1], threshold=1.0)
    b = extract_mesh(D, SMOOTH_BOX[0] + SMOOTH_BOX[1], threshold=1.0)
    assert same_bits(a.vertices, b.vertices) and same_bits(a.normals, b.normals) and same_bits(a.faces, b.faces)
    assert np.array_equal(a.faces.cpu().numpy(), twin_of("smooth_33x17x20", True)[2])      # the order too: cell, tetrahedron, triangle


def _ball_density(x):
    """1.45 - |x|, in elementwise float32 operations only: the same bits whatever the batch."""
    return 1.45 - torch.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])


def test_occupancy_skips_evaluations_and_matches_the_masked_twin(cuda):
    from cnc_amd.mesh import extract_mesh
    n, box = (16, 16, 16), ([-1.0] * 3, [1.0] * 3)
    c = (np.arange(8) + 0.5) / 4 - 1
    occ = (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) < 0.75 ** 2
    occ[7, 0, 3] = True                                        # a cell far from the surface: evaluated, gives no face
    pos = T.positions(box[0], box[1], n)
    active = T.active_points(occ, n)
    assert 0 < active.sum() < active.size
    full = _ball_density(torch.from_numpy(pos).to(cuda)).cpu().numpy().reshape(active.shape)
    masked = np.where(active, full, np.float32(0)).astype(np.float32)
    v, f, nrm = T.extract(masked, box[0], box[1], 1.0)
    assert f.shape[0] > 0 and T.euler_characteristic(f, v.shape[0]) == 2
    seen = []

    def counted(x):
        seen.append(x.clone())
        return _ball_density(x).view(-1, 1)                    # [M, 1], as the field returns it
    mesh, lattice = extract_mesh(counted, box[0] + box[1], 16, 1.0, occupancy=torch.from_numpy(occ).to(cuda), chunk=1000,
                                 return_lattice=True)
    got = torch.cat(seen).cpu().numpy()
    assert all(s.shape[0] <= 1000 for s in seen) and len(seen) == -(-int(active.sum()) // 1000)
    assert got.shape[0] == int(active.sum()) < pos.shape[0]                    # fewer points than the lattice holds
    assert same_bits(got, pos[active.reshape(-1)])                              # and exactly the active ones, in order
    assert same_bits(lattice, T.capped(masked))
    assert_is_twin(mesh, v, f, nrm)


def test_callable_density_in_chunks_that_do_not_divide_the_lattice(cuda):
    from cnc_amd.mesh import extract_mesh
    n, box = (9, 9, 9), ([-1.0] * 3, [1.0] * 3)
    f_ = lambda x: 1.0 + 0.5 * torch.sin(3.0 * x[:, 0]) * torch.cos(2.0 * x[:, 1]) + 0.4 * x[:, 2]
    pos = T.positions(box[0], box[1], n)
    D = f_(torch.from_numpy(pos).to(cuda)).cpu().numpy().reshape(10, 10, 10)
    v, f, nrm = T.extract(D, box[0], box[1], 1.0)
    sizes = []

    def chunked(x):
        sizes.append(x.shape[0])
        return f_(x)
    mesh = extract_mesh(chunked, box[0] + box[1], 9, 1.0, chunk=1000, device=cuda)
    assert sizes == [1000]
    sizes.clear()
    mesh = extract_mesh(chunked, box[0] + box[1], 9, 1.0, chunk=300, device=cuda)
    assert sizes == [300, 300, 300, 100] and f.shape[0] > 0
    assert_is_twin(mesh, v, f, nrm)
    # the default threshold: ln 2 / render_step_size
    again = extract_mesh(chunked, box[0] + box[1], 9, None, render_step_size=float(np.log(2.0)), chunk=300, device=cuda)
    assert same_bits(again.vertices, mesh.vertices) and same_bits(again.faces, mesh.faces)


@pytest.mark.parametrize("kind", ["all_inside_uncapped", "all_outside", "all_nan"])
def test_empty_results_launch_no_emit_kernel(cuda, kind, monkeypatch):
    from cnc_amd.backends import iso_surface as iso
    from cnc_amd.mesh import extract_mesh

    def never(*a, **k):
        raise AssertionError("an emit kernel was launched for an empty mesh")
    monkeypatch.setattr(iso, "emit_vertices", never)
    monkeypatch.setattr(iso, "emit_faces", never)
    value = {"all_inside_uncapped": 1.0, "all_outside": 0.0, "all_nan": float("nan")}[kind]
    D = torch.full((6, 5, 4), value, device=cuda)
    for normals in (True, False):
        m = extract_mesh(D, UNIT[0] + UNIT[1], threshold=0.5, cap=kind != "all_inside_uncapped", normals=normals)
        assert tuple(m.vertices.shape) == (0, 3) and m.vertices.dtype == torch.float32 and m.vertices.is_cuda
        assert tuple(m.faces.shape) == (0, 3) and m.faces.dtype == torch.int32
        assert (tuple(m.normals.shape) == (0, 3)) if normals else m.normals is None
        assert m.components().shape == (0,)


def test_entry_points_refuse_bad_arguments(cuda):
    from cnc_amd.backends import iso_surface as iso
    from cnc_amd.mesh import tet_table
    table = torch.from_numpy(tet_table().reshape(-1)).to(cuda)
    D, mask, tris = torch.zeros(27, device=cuda), torch.zeros(27, dtype=torch.uint8, device=cuda), torch.zeros(8, dtype=torch.uint8, device=cuda)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="invalid"):
            iso.classify(D, (2, 2, 2), bad, True, table, mask, tris)
    with pytest.raises(RuntimeError):
        iso.classify(D, (2, 2, 3), 0.5, True, table, mask, tris)               # buffers of another lattice
    with pytest.raises(RuntimeError):
        iso.classify(D, (2, 2, 2), 0.5, True, table[:100], mask, tris)


def test_footprint_under_three_fills(cuda):
    """Every buffer of the five entry points inside a sentinel allocation: nothing outside is written, no input changes,
    and the outputs do not move with the bytes around the inputs."""
    from cnc_amd.backends import iso_surface as iso
    from cnc_amd.mesh import spacing, tet_table
    D, v, f, nrm = twin_of("noise_9x9x9", True)
    n, thr = (9, 9, 9), 0.5
    points, cells = 1000, 729
    lo, h = spacing(UNIT[0] + UNIT[1], n)
    occ = np.random.default_rng(3).uniform(size=(4, 3, 5)) < 0.2
    active_want = T.active_points(occ, n).reshape(-1)
    lin = np.nonzero(active_want)[0].astype(np.int64)
    popcount = torch.tensor([bin(m).count("1") for m in range(256)], dtype=torch.uint8, device=cuda)

    def build(fill):
        g = lambda a: Guarded(a, cuda, fill=fill)
        e = lambda shape, dt: Guarded.empty(shape, dt, cuda, fill=fill)
        return {"density": g(D).out(), "table": g(tet_table().reshape(-1).view(np.uint8)), "occupancy": g(occ), "lin": g(lin),
                "edge_mask": e((points,), np.uint8), "cell_tris": e((cells,), np.uint8), "vertex_scan": e((points,), np.int32),
                "cell_scan": e((cells,), np.int32), "vertices": e(v.shape, np.float32), "normals": e(v.shape, np.float32),
                "faces": e(f.shape, np.int32), "active": e((points,), np.uint8), "positions": e((len(lin), 3), np.float32),
                "positions_all": e((points, 3), np.float32)}

    def run(b):
        t = {k: g.tensor() for k, g in b.items()}
        table = t["table"].view(torch.int8)
        iso.active_points(t["occupancy"], n, t["active"])
        iso.lattice_positions(t["lin"], 0, len(lin), n, lo, h, t["positions"])
        iso.lattice_positions(None, 0, points, n, lo, h, t["positions_all"])
        iso.classify(t["density"], n, thr, True, table, t["edge_mask"], t["cell_tris"])
        per_point = popcount.index_select(0, t["edge_mask"].to(torch.int32))
        assert int(per_point.sum()) == v.shape[0] and int(t["cell_tris"].sum(dtype=torch.int64)) == f.shape[0]
        t["vertex_scan"].copy_(torch.cumsum(per_point, 0, dtype=torch.int32) - per_point)
        t["cell_scan"].copy_(torch.cumsum(t["cell_tris"], 0, dtype=torch.int32) - t["cell_tris"])
        iso.emit_vertices(t["density"], n, thr, lo, h, t["edge_mask"], t["vertex_scan"], t["vertices"], t["normals"])
        iso.emit_faces(t["density"], n, thr, table, t["edge_mask"], t["vertex_scan"], t["cell_tris"], t["cell_scan"], v.shape[0],
                       t["faces"])
    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    out = res[0xA5]
    assert same_bits(out["density"], T.capped(D)) and same_bits(out["vertices"], v) and same_bits(out["normals"], nrm)
    assert np.array_equal(out["faces"], f)
    assert np.array_equal(out["active"].astype(bool), active_want)
    pos = T.positions(UNIT[0], UNIT[1], n)
    assert same_bits(out["positions_all"], pos) and same_bits(out["positions"], pos[lin])
    assert int(out["cell_tris"].max()) <= 12 and int(out["edge_mask"].max()) < 128
