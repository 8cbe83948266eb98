"""CPU-only: the mesh export's rule — the generated triangle table against the twin's direct rule, the twin's
meshes on noise, ties, a sphere and a torus, the refusals, the PLY writer and the new flags."""
import math

import numpy as np
import pytest
import torch

import mesh_twin as T

NONTRIVIAL = {(tet, m) for tet in range(6) for m in range(1, 15)}


def test_tet_table_is_the_direct_rule_for_every_pair():
    from cnc_amd.mesh import DIRECTIONS, tet_table
    table = tet_table()
    assert table.shape == (6, 16, 7) and table.dtype == np.int8
    for tet in range(6):
        V = T.tet_local(tet)
        for mask in range(16):
            want = T.direct_triangles(tet, mask)
            row = table[tet, mask]
            assert row[0] == len(want) == (0 if mask in (0, 15) else 1 if bin(mask).count("1") in (1, 3) else 2)
            assert (row[1 + 3 * len(want):] == -1).all()
            for t, tri in enumerate(want):
                for e, (i, j) in enumerate(tri):
                    code = int(row[1 + 3 * t + e])
                    corner, d = code >> 3, code & 7
                    assert [corner & 1, corner >> 1 & 1, corner >> 2] == V[i].tolist()
                    assert list(DIRECTIONS[d]) == (V[j] - V[i]).tolist()


def test_directions_and_tetrahedra_are_the_documented_ones():
    from cnc_amd import mesh
    assert np.array_equal(np.asarray(mesh.DIRECTIONS), T.DIRS)
    assert [tuple(p) for p in mesh.PERMUTATIONS] == T.PERMS
    for tet in range(6):
        assert np.array_equal(np.asarray(mesh.tet_vertices(tet)), T.tet_local(tet))


@pytest.mark.parametrize("name,n,seed,make", [("noise", (4, 5, 6), 11, T.noise_lattice), ("noise", (9, 9, 9), 12, T.noise_lattice),
                                              ("ties", (4, 5, 6), 13, T.tie_lattice), ("ties", (9, 9, 9), 14, T.tie_lattice)])
def test_twin_meshes_of_noise_are_closed_manifolds(name, n, seed, make):
    D = make(n, seed)
    if name == "ties":
        assert (D == 0.5).sum() > D.size // 10
    v, f, nrm, pairs = T.extract(D, [0, 0, 0], [1, 1, 1], 0.5, want_pairs=True)
    assert f.shape[0] > 0 and v.shape == nrm.shape and int(f.max()) == v.shape[0] - 1
    assert T.is_directed_manifold(f, v.shape[0])
    if n == (9, 9, 9):
        assert pairs == NONTRIVIAL           # the GPU tests reuse this lattice: it visits all 84 non-trivial pairs
    finite = np.isfinite(nrm).all(axis=1)
    length = np.linalg.norm(nrm[finite].astype(np.float64), axis=1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))


@pytest.mark.parametrize("cells,tol", [(16, 0.025), (32, 0.007)])
def test_twin_sphere(cells, tol):
    v, f, _ = T.extract(T.sphere_lattice(cells), [-1] * 3, [1] * 3, 1.0, normals=False)
    assert T.is_directed_manifold(f, v.shape[0]) and T.euler_characteristic(f, v.shape[0]) == 2
    vol, want = T.signed_volume(v, f), 4.0 / 3.0 * math.pi * 0.6 ** 3
    assert vol > 0 and abs(vol / want - 1) < tol, vol / want


def test_twin_torus():
    v, f, _ = T.extract(T.torus_lattice(24), [-1] * 3, [1] * 3, 1.0, normals=False)
    assert T.is_directed_manifold(f, v.shape[0]) and T.euler_characteristic(f, v.shape[0]) == 0
    vol, want = T.signed_volume(v, f), 2 * math.pi ** 2 * 0.55 * 0.2 ** 2
    assert vol > 0 and abs(vol / want - 1) < 0.035, vol / want


def test_twin_normals_point_out_of_the_sphere():
    v, f, nrm = T.extract(T.sphere_lattice(16), [-1] * 3, [1] * 3, 1.0)
    radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    assert np.einsum("ij,ij->i", radial, nrm.astype(np.float64)).min() > 0.9


def test_twin_float64_mode_agrees_with_float32():
    D = T.smooth_lattice((12, 7, 9))
    box = ([-1, -0.5, -0.6], [1, 0.5, 0.6])
    v32, f32, n32 = T.extract(D, *box, 1.0)
    v64, f64, n64 = T.extract(D, *box, 1.0, dtype=np.float64)
    assert v64.dtype == np.float64 and np.array_equal(f32, f64)
    assert np.abs(v32 - v64).max() < 1e-5


def test_twin_trivial_and_nan_lattices():
    shape = (4, 5, 6)
    box = ([0, 0, 0], [1, 1, 1])
    for D, cap in ((np.ones(shape, np.float32), False), (np.zeros(shape, np.float32), True), (np.zeros(shape, np.float32), False),
                   (np.full(shape, np.nan, np.float32), False), (np.full(shape, np.nan, np.float32), True)):
        v, f, nrm = T.extract(D, *box, 0.5, cap=cap)
        assert v.shape == (0, 3) and f.shape == (0, 3) and nrm.shape == (0, 3)
    v, f, _ = T.extract(np.ones(shape, np.float32), *box, 0.5, cap=True)        # all inside, capped: the box's inner block
    assert T.is_directed_manifold(f, v.shape[0]) and T.euler_characteristic(f, v.shape[0]) == 2
    D = T.noise_lattice((5, 4, 3), 3)
    D[2, 2, 2] = np.nan
    v, f, _ = T.extract(D, *box, 0.5)
    assert T.is_directed_manifold(f, v.shape[0])                                # NaN is outside: the topology holds


def test_active_points_of_the_twin():
    occ = np.zeros((8, 8, 8), bool)
    occ[3, 4, 5] = True
    act = T.active_points(occ, (16, 16, 16))
    z, y, x = np.nonzero(act)
    # cell 3 of 8 covers points 6..8 of 16; +-1 point of reach, touching included: 5..9
    assert (x.min(), x.max(), y.min(), y.max(), z.min(), z.max()) == (5, 9, 7, 11, 9, 13)
    assert T.active_points(np.ones((3, 5, 2), bool), (4, 9, 7)).all()
    assert not T.active_points(np.zeros((3, 5, 2), bool), (4, 9, 7)).any()


# ---------------------------------------------------------------------------------------------- the product, without a GPU
def test_lattice_cells_and_spacing():
    from cnc_amd import mesh
    assert mesh.lattice_cells([-1.5] * 3 + [1.5] * 3, 256) == (256, 256, 256)
    assert mesh.lattice_cells([0, 0, 0, 2, 1, 0.001], 10) == (10, 5, 1) == T.cells_of([0, 0, 0], [2, 1, 0.001], 10)
    assert mesh.lattice_cells(torch.tensor([-1.0, -0.5, -0.6, 1.0, 0.5, 0.6]), 33) == (33, 16, 20)
    lo, h = mesh.spacing([-1, -0.5, -0.6, 1, 0.5, 0.6], (33, 17, 20))
    lo_t, h_t = T.spacing([-1, -0.5, -0.6], [1, 0.5, 0.6], (33, 17, 20))
    assert lo.dtype == h.dtype == np.float32 and np.array_equal(lo, lo_t) and np.array_equal(h, h_t)


def test_refusals_need_arguments_alone():
    from cnc_amd import mesh

    def never(x):
        raise AssertionError("the density was evaluated")
    box = [-1.0] * 3 + [1.0] * 3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="threshold"):
            mesh.extract_mesh(never, box, 16, bad)
    with pytest.raises(ValueError, match="render_step_size"):
        mesh.extract_mesh(never, box, 16)
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.extract_mesh(never, box, 1300, 1.0)                # 1301^3 points
    with pytest.raises(ValueError, match="2\\^31"):
        mesh.check_lattice((2047, 1023, 1023))                 # exactly 2^31 points
    assert mesh.check_lattice((2046, 1023, 1023)) == 2047 * 1024 * 1024
    with pytest.raises(ValueError, match="aabb"):
        mesh.extract_mesh(never, [0, 0, 0, 1, 1, 0], 16, 1.0)
    assert mesh.resolve_threshold(None, 5e-3) == float(np.float32(math.log(2.0) / 5e-3))

    class Unbounded:
        unbounded = True

        def query_density(self, x):
            raise AssertionError("the density was evaluated")
    with pytest.raises(ValueError, match="bounded"):
        mesh.field_mesh(Unbounded(), torch.tensor(box), None, 5e-3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):       # like every mirror: no CPU fallback
        mesh.extract_mesh(torch.zeros(3, 3, 3), box, threshold=1.0)


def test_mirror_refuses_cpu_tensors():
    from cnc_amd.backends import iso_surface as iso
    from cnc_amd.mesh import tet_table
    n = (2, 2, 2)
    D, mask, tris = torch.zeros(27), torch.zeros(27, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)
    table = torch.from_numpy(tet_table().reshape(-1))
    assert table.numel() == iso.TABLE
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        iso.classify(D, n, 0.5, True, table, mask, tris)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        iso.active_points(torch.ones(2, 2, 2, dtype=torch.bool), n, mask)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        iso.lattice_positions(None, 0, 27, n, [0, 0, 0], [1, 1, 1], torch.zeros(27, 3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        iso.emit_vertices(D, n, 0.5, [0, 0, 0], [1, 1, 1], mask, torch.zeros(27, dtype=torch.int32), torch.zeros(1, 3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        iso.emit_faces(D, n, 0.5, table, mask, torch.zeros(27, dtype=torch.int32), tris, torch.zeros(8, dtype=torch.int32), 1,
                       torch.zeros(1, 3, dtype=torch.int32))


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, False), (False, True)])
def test_ply_round_trip(tmp_path, with_normals, with_colors):
    from cnc_amd.mesh import Mesh
    v, f, nrm = T.extract(T.noise_lattice((4, 5, 6), 21), [0, 0, 0], [1, 1, 1], 0.5)
    rgb = np.random.default_rng(5).integers(0, 256, size=v.shape).astype(np.uint8)
    m = Mesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(nrm) if with_normals else None,
             torch.from_numpy(rgb) if with_colors else None)
    m.save(str(tmp_path / "m.ply"))
    props, faces = T.parse_ply(tmp_path / "m.ply")
    assert list(props) == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert np.array_equal(np.stack([props[k] for k in "xyz"], -1), v) and np.array_equal(faces, f)
    if with_normals:
        assert np.array_equal(np.stack([props[k] for k in ("nx", "ny", "nz")], -1), nrm)
    if with_colors:
        assert np.array_equal(np.stack([props[k] for k in ("red", "green", "blue")], -1), rgb)


def test_empty_mesh_saves_and_has_no_components(tmp_path):
    from cnc_amd.mesh import Mesh
    m = Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3))
    m.save(str(tmp_path / "e.ply"))
    props, faces = T.parse_ply(tmp_path / "e.ply")
    assert props["x"].shape == (0,) and faces.shape == (0, 3) and m.components().shape == (0,)


def test_components_count_faces_per_blob():
    from cnc_amd.mesh import Mesh
    X, Y, Z = T.axes([-1] * 3, [1] * 3, (24,) * 3, np.float64)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    ball = lambda c, r: r - np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2)
    D = (1.0 + np.maximum(np.maximum(ball((-0.4, -0.3, 0), 0.35), ball((0.5, 0.4, 0.2), 0.2)), ball((0.5, -0.6, -0.5), 0.1))).astype(np.float32)
    v, f, _ = T.extract(D, [-1] * 3, [1] * 3, 1.0, normals=False)
    comp = Mesh(torch.from_numpy(v), torch.from_numpy(f)).components()
    assert comp.shape == (3,) and comp.sum() == f.shape[0] and comp[0] > comp[1] > comp[2] > 0
    # against a plain flood fill over shared vertices
    label = np.arange(v.shape[0])
    for _ in range(200):
        m = label[f].min(axis=1)
        before = label.copy()
        for c in range(3):
            np.minimum.at(label, f[:, c], m)
        if np.array_equal(before, label):
            break
    _, want = np.unique(label[f[:, 0]], return_counts=True)
    assert np.array_equal(np.sort(want)[::-1], comp)


def test_new_flags_and_their_defaults():
    from cnc_amd.train import build_parser
    from cnc_amd.trainer import TrainConfig
    c = TrainConfig()
    assert c.save_mesh is None and c.mesh_resolution == 256 and c.mesh_threshold is None
    a = build_parser().parse_args([])
    assert a.save_mesh is None and a.mesh_resolution == 256 and a.mesh_threshold is None
    a = build_parser().parse_args(["--save-mesh", "ball.ply", "--mesh-resolution", "64", "--mesh-threshold", "12.5"])
    assert (a.save_mesh, a.mesh_resolution, a.mesh_threshold) == ("ball.ply", 64, 12.5)
