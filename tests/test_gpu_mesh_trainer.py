"""`Trainer.extract_mesh` and `python -m cnc_amd.train --save-mesh` on the small configuration of
tests/test_gpu_trainer.py, 120 steps on the procedural ball.  Nothing here claims a shape for the ball after 120 steps:
the mesh must be a closed manifold inside the box and equal the twin's mesh of the same lattice."""
import math

import numpy as np
import pytest
import torch

import mesh_twin as T
from guarded import same_bits

pytestmark = pytest.mark.gpu

N_COLS = 9 + 3 + 6 + 3      # the results line of tests/test_gpu_cli.py


def _cfg(tmp_path, **kw):
    from cnc_amd.trainer import TrainConfig
    base = dict(lmbda=2e-3, Pg_level=5, Pg_level_2D=3, log2_hashmap_size=12, log2_hashmap_size_2D=9,
                sample_num=3000, max_context_layer_num=3, n_features=2, n_neurons=32,
                resolutions_list=(10, 14, 18, 26, 34), resolutions_list_2D=(18, 34, 66),
                skip_levels_3D=(0, 1, 2), skip_levels_2D=(0,), max_steps=150, init_batch_size=512,
                target_sample_batch_size=1 << 14, grid_resolution=16, render_step_size=2e-2,
                milestones=(100, 130), warmup_iters=20, test_views=2, image_size=48,
                out_dir=str(tmp_path / "bits"), log_every=50)
    base.update(kw)
    return TrainConfig(**base)


@pytest.fixture(scope="module")
def trained(cuda, tmp_path_factory):
    """One trainer after 120 steps, its mesh at resolution 48 with the lattice it was cut from, and the PLY."""
    from cnc_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("mesh")
    tr = Trainer(_cfg(tmp), device=cuda)
    tr.train(steps=120, log=None)
    before = {k: v.clone() for k, v in tr.field.state_dict().items()}
    training = tr.field.training
    mesh, lattice = tr.extract_mesh(str(tmp / "ball.ply"), resolution=48, return_lattice=True)
    assert tr.field.training == training
    assert all(torch.equal(v, before[k]) for k, v in tr.field.state_dict().items())        # an export changes no parameter
    return tr, mesh, lattice, tmp / "ball.ply"


def test_mesh_is_a_closed_manifold_inside_the_box(trained):
    tr, mesh, lattice, _ = trained
    V, F = mesh.vertices.shape[0], mesh.faces.shape[0]
    assert V > 0 and F > 0 and tuple(lattice.shape) == (49, 49, 49)
    assert T.is_directed_manifold(mesh.faces.cpu().numpy(), V)
    box = torch.tensor(tr.cfg.aabb, device=mesh.vertices.device)
    assert (mesh.vertices >= box[:3]).all() and (mesh.vertices <= box[3:]).all()
    assert tuple(mesh.colors.shape) == (V, 3) and mesh.colors.dtype == torch.uint8
    assert tuple(mesh.normals.shape) == (V, 3)
    length = mesh.normals.norm(dim=1)
    assert (((length - 1).abs() < 1e-5) | (length == 0)).all()
    comp = mesh.components()
    assert comp.sum() == F and comp[0] >= comp[-1] > 0


def test_mesh_is_the_twins_mesh_of_the_same_lattice(trained):
    tr, mesh, lattice, _ = trained
    D = lattice.cpu().numpy()
    assert same_bits(D, T.capped(D))                                            # the lattice comes back capped
    thr = math.log(2.0) / tr.cfg.render_step_size
    v, f, nrm = T.extract(D, tr.cfg.aabb[:3], tr.cfg.aabb[3:], thr)
    assert same_bits(mesh.vertices, v) and same_bits(mesh.normals, nrm)
    assert np.array_equal(T.canonical_faces(mesh.faces.cpu().numpy()), T.canonical_faces(f))
    # points the occupancy grid rules out were never evaluated: they hold exactly 0
    active = T.active_points(tr.estimator.binaries[0].cpu().numpy(), (48, 48, 48))
    assert not D[~active].any() and active.sum() < active.size


def test_ply_parses_back_to_the_same_arrays(trained):
    _, mesh, _, path = trained
    props, faces = T.parse_ply(path)
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert same_bits(np.stack([props[k] for k in "xyz"], -1), mesh.vertices)
    assert same_bits(np.stack([props[k] for k in ("nx", "ny", "nz")], -1), mesh.normals)
    assert np.array_equal(np.stack([props[k] for k in ("red", "green", "blue")], -1), mesh.colors.cpu().numpy())
    assert np.array_equal(faces, mesh.faces.cpu().numpy())


def test_colors_are_the_field_seen_along_minus_normal(trained):
    tr, mesh, _, _ = trained
    with torch.no_grad():
        tr.field.eval()
        rgb, _ = tr.field(mesh.vertices, -mesh.normals)
        tr.field.train()
    want = (rgb.clamp(0, 1) * 255 + 0.5).to(torch.uint8)
    assert torch.equal(want, mesh.colors)
    plain = tr.extract_mesh(resolution=48, colors=False)
    assert plain.colors is None and same_bits(plain.vertices, mesh.vertices) and same_bits(plain.faces, mesh.faces)


def test_cli_save_mesh_writes_a_file_and_the_usual_results_line(cuda, tmp_path, monkeypatch):
    from cnc_amd import train
    monkeypatch.chdir(tmp_path)
    argv = ["--max_steps", "40", "--n_features", "2", "--sample_num", "20000", "--test_views", "1",
            "--log2_hashmap_size", "14", "--log2_hashmap_size_2D", "12", "--results", str(tmp_path / "out.txt"),
            "--out_dir", str(tmp_path / "bits"), "--dataset", "procedural", "--image_size", "48",
            "--save-mesh", str(tmp_path / "ball.ply"), "--mesh-resolution", "32"]
    cols = train.main(argv)
    line = open(tmp_path / "out.txt").read().strip().split("\t")
    assert line == cols and len(line) == N_COLS and line[0] == "ball"
    props, faces = T.parse_ply(tmp_path / "ball.ply")
    assert list(props)[:3] == ["x", "y", "z"] and faces.shape[1] == 3
    assert faces.size == 0 or int(faces.max()) < props["x"].shape[0]
