"""GPU: camera pose refinement in the Trainer on the capture tests/test_gpu_transforms_loader.py writes —
the procedural ball through an OPENCV lens, 9 views of 24 x 18 pixels, 7 of them training views — at `_cfg`'s small
configuration with the guarded-step tests' shape (n_features = 2, n_neurons = 64: 32 neurons are not a shape of the fused
training forward, the only path with position gradients).

Recovery (c), measured on the MI355X: a displacement of 0.2915 ends at 0.1829 after 120 steps at POSE_LR (ratio 0.63),
falling at every look: 0.249, 0.229, 0.218, 0.212, 0.199, 0.183."""
import json
import os
import shutil
import warnings

import numpy as np
import pytest
import torch

import test_gpu_reproducible_step as R
from test_gpu_guarded_trainer import SHAPE, _nan_batch
from test_gpu_transforms_loader import capture  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
POSE_LR = 5e-3


def _trainer(cuda, tmp_path, root, scene="ball_lens", batch_over_images=True, **kw):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    from cnc_amd.trainer import Trainer
    train = TransformsLoader(scene, root, "train", num_rays=512, color_bkgd_aug="random", device=cuda,
                             batch_over_images=batch_over_images)
    test = TransformsLoader(scene, root, "test", device=cuda)
    train.seed_sampling(11)
    data = LoaderDataset(train, test)
    data._gen = torch.Generator().manual_seed(5)
    torch.manual_seed(1234)
    return Trainer(R._cfg(tmp_path, seed=3, aabb=tuple(train.aabb.tolist()), **SHAPE, **kw), device=cuda, dataset=data)


def test_off_by_default_nothing_is_added(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.delenv("CNC_POSE_LR", raising=False)
    tr = _trainer(cuda, tmp_path, capture[0])
    assert tr.cfg.pose_lr == 0.0 and tr.pose_refiner is None and tr.opt_pose is None
    before = tr.dataset.train.cameras.clone()
    keys = set()
    fetch = tr.dataset.fetch
    tr.dataset.fetch = lambda: (lambda d: (keys.update(d), d)[1])(fetch())
    for s in range(10):
        tr.train_step(s, want_stats=False)
    torch.cuda.synchronize()
    assert keys == {"pixels", "rays", "color_bkgd"}
    assert torch.equal(tr.dataset.train.cameras, before) and not tr.dataset.train.with_camera_ids
    assert not os.path.exists(os.path.join(tr.cfg.out_dir, "transforms_refined.json"))


def test_environment_variable_switches_it_on(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("CNC_POSE_LR", "2e-3")
    tr = _trainer(cuda, tmp_path, capture[0])
    assert tr.pose_refiner is not None and tr.opt_pose.param_groups[0]["lr"] == 2e-3
    assert tr.opt_pose.param_groups[0]["weight_decay"] == 0 and tr.opt_pose.param_groups[0]["fused"]


def test_reproducible_runs_give_equal_deltas(cuda, capture, tmp_path):  # noqa: F811
    """One image per batch (`batch_over_images=False`), so that some cameras never get a ray in 10 steps: their delta must
    stay exactly zero, every other camera's must move, and two runs from one seed agree bit for bit."""
    runs = []
    for k in range(2):
        tr = _trainer(cuda, tmp_path / str(k), capture[0], batch_over_images=False, reproducible=True, pose_lr=POSE_LR)
        seen = set()
        fetch = tr.dataset.fetch
        tr.dataset.fetch = lambda: (lambda d: (seen.update(d["camera_ids"].unique().tolist()), d)[1])(fetch())
        taken = [tr.train_step(s, want_stats=False) for s in range(10)]
        torch.cuda.synchronize()
        assert all(t is not None for t in taken)
        runs.append((tr.pose_refiner.delta.detach().clone(), tr.dataset.train.cameras.clone(), seen))
    (d0, cams0, seen0), (d1, cams1, seen1) = runs
    assert seen0 == seen1 and 0 < len(seen0) < d0.shape[0], seen0
    assert R._bits(d0).equal(R._bits(d1)) and R._bits(cams0).equal(R._bits(cams1))
    moved = set(torch.nonzero(d0.abs().sum(dim=1) > 0).view(-1).tolist())
    assert moved == seen0, (moved, seen0)
    assert bool(torch.isfinite(d0).all())


def test_a_displaced_camera_moves_back(cuda, capture, tmp_path):  # noqa: F811
    """Train on the true poses, displace one training camera's translation in the loader's table, continue with the
    field's learning rates at 0 and the poses' at POSE_LR: that camera's translation error ends below where it started.
    Only the decrease is asserted."""
    tr = _trainer(cuda, tmp_path, capture[0])
    for s in range(200):
        tr.train_step(s, want_stats=False)
    cam, shift = 3, torch.tensor([0.25, -0.15, 0.0], device=cuda)
    table = tr.dataset.train.cameras
    true_t = table[cam, [7, 11, 15]].clone()
    tr._next_data = None                                     # (drawn from the true table)
    table[cam, 7] += shift[0]
    table[cam, 11] += shift[1]
    for opt in (tr.opt, tr.opt2):
        for g in opt.param_groups:
            g["lr"] = 0.0
    tr.enable_pose_refinement(POSE_LR)
    field_before = [p.detach().clone() for p in tr.field.mlp_head.parameters()]
    start = float(shift.norm())
    errs = []
    for s in range(200, 320):
        tr.train_step(s, want_stats=False)
        if (s + 1) % 20 == 0:
            errs.append(float((tr.dataset.train.cameras[cam, [7, 11, 15]] - true_t).norm()))
    torch.cuda.synchronize()
    print(f"POSE RECOVERY: translation error {start:.4f} -> {errs} (ratio {errs[-1] / start:.3f})")
    assert all(torch.equal(a, b.detach()) for a, b in zip(field_before, tr.field.mlp_head.parameters())), "the field moved"
    assert errs[-1] < start


def test_guarded_step_skips_the_poses_too(cuda, capture, tmp_path):  # noqa: F811
    tr = _trainer(cuda, tmp_path, capture[0], reproducible=True, guarded_step=True, pose_lr=POSE_LR)
    for s in range(3):
        assert tr.train_step(s) is not None
    assert tr.step_guard.stats() == {"skipped": 0, "reasons": 0}

    def pose_state():
        torch.cuda.synchronize()
        st = tr.opt_pose.state[tr.pose_refiner.delta]
        return {"delta": tr.pose_refiner.delta.detach().clone(), "table": tr.dataset.train.cameras.clone(),
                **{k: v.detach().clone() for k, v in st.items() if isinstance(v, torch.Tensor)}}
    before = pose_state()
    assert {"exp_avg", "exp_avg_sq", "step"} <= set(before) and bool(before["delta"].abs().sum() > 0)
    tr._next_data = _nan_batch(tr)
    assert "camera_ids" in tr._next_data
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = tr.train_step(3)
    after = pose_state()
    assert out is not None and out["mse"] != out["mse"]
    assert tr.step_guard.stats()["skipped"] == 1
    for k in before:
        assert R._bits(before[k]).equal(R._bits(after[k])), k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tr.train_step(4) is not None
    later = pose_state()
    assert not torch.equal(later["delta"], before["delta"]) and float(later["step"]) == float(before["step"]) + 1
    assert bool(torch.isfinite(later["delta"]).all())


def test_requests_that_cannot_work_raise(cuda, capture, tmp_path):  # noqa: F811
    from cnc_amd.trainer import Trainer
    with pytest.raises(ValueError, match="TransformsLoader"):
        Trainer(R._cfg(tmp_path, seed=3, pose_lr=1e-3, **SHAPE), device=cuda)               # the synthetic dataset
    tr = _trainer(cuda, tmp_path, capture[0])
    tr.field.unbounded = True
    with pytest.raises(ValueError, match="bounded"):
        tr.enable_pose_refinement(1e-3)
    tr.field.unbounded = False
    tr.dp, tr.world = True, 2
    with pytest.raises(ValueError, match="data-parallel"):
        tr.enable_pose_refinement(1e-3)
    tr.dp, tr.world = False, 1
    with pytest.raises(ValueError, match="positive"):
        tr.enable_pose_refinement(0.0)
    assert tr.pose_refiner is None and not tr.dataset.train.with_camera_ids
    with pytest.raises(ValueError, match="fused training forward"):                          # 32 neurons: `_cfg`'s own shape
        Trainer(R._cfg(tmp_path / "h32", seed=3, aabb=tuple(tr.dataset.train.aabb.tolist()), pose_lr=1e-3), device=cuda,
                dataset=tr.dataset)
    assert not tr.dataset.train.with_camera_ids
    tr.enable_pose_refinement(1e-3)                          # ... and the plain one-process Trainer takes it
    assert tr.pose_refiner is not None and tr.dataset.train.with_camera_ids


def test_range_guard_fallback_stops_refinement_with_a_warning(cuda, capture, tmp_path):  # noqa: F811
    tr = _trainer(cuda, tmp_path, capture[0], reproducible=True, pose_lr=POSE_LR)
    for s in range(2):
        tr.train_step(s, want_stats=False)
    tr.field.fused_train = False                             # what `poll_range_guard` / `check_range_guard` leave behind
    delta = tr.pose_refiner.delta.detach().clone()
    with pytest.warns(UserWarning, match="pose refinement stops"):
        assert tr.train_step(2) is not None
    assert tr.train_step(3) is not None                      # the run continues, the poses stay
    torch.cuda.synchronize()
    assert torch.equal(tr.pose_refiner.delta.detach(), delta)


def test_cli_writes_the_refined_capture(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    from cnc_amd import train
    from cnc_amd.datasets import TransformsLoader
    root = capture[0]
    made = []

    class Recording(train.Trainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(train, "Trainer", Recording)
    monkeypatch.chdir(tmp_path)
    out_dir = tmp_path / "bits"
    a = train.build_parser().parse_args([])
    assert a.refine_poses == 0.0 and a.refine_poses_from == 0
    argv = ["--data_root", root, "--scene", "ball_lens", "--dataset", "transforms", "--max_steps", "40", "--n_features", "2",
            "--sample_num", "20000", "--test_views", "1", "--log2_hashmap_size", "14", "--log2_hashmap_size_2D", "12",
            "--results", str(tmp_path / "out.txt"), "--out_dir", str(out_dir), "--refine-poses", "2e-3",
            "--refine-poses-from", "5"]
    train.main(argv)
    tr = made[0]
    assert tr.cfg.pose_lr == 2e-3 and tr.cfg.pose_refine_from == 5 and tr.pose_refiner is not None
    path = out_dir / "transforms_refined.json"
    doc, src = json.load(open(path)), json.load(open(os.path.join(root, "ball_lens", "transforms.json")))
    assert [f["file_path"] for f in doc["frames"]] == [f["file_path"] for f in src["frames"]]
    assert {k: v for k, v in doc.items() if k != "frames"} == {k: v for k, v in src.items() if k != "frames"}
    held = [i for i in range(len(src["frames"])) if i % 8 == 0]
    for i, (a_, b_) in enumerate(zip(doc["frames"], src["frames"])):
        same = np.allclose(np.asarray(a_["transform_matrix"]), np.asarray(b_["transform_matrix"]), rtol=0, atol=1e-7)
        assert same == (i in held), i                       # the test frames keep the file's poses, the training frames moved
    # read back: the refined file as a capture of its own gives the Trainer's table
    scene = os.path.join(root, "ball_refined")
    shutil.copytree(os.path.join(root, "ball_lens"), scene)
    shutil.copy(path, os.path.join(scene, "transforms.json"))
    back = TransformsLoader("ball_refined", root, "train", device=cuda)
    assert float((back.cameras - tr.dataset.train.cameras).abs().max()) <= 2.0 ** -22        # float32 through decimal text
    assert float((back.cameras - tr._pose_base).abs().max()) > 1e-4
