"""GPU: per-camera exposure compensation in the Trainer on the capture
tests/test_gpu_transforms_loader.py writes — the procedural ball through an OPENCV lens, 9 views of 24 x 18 pixels with an
alpha channel, 7 of them training views — with the Trainer of tests/test_gpu_pose_trainer.py.

Recovery, measured on the MI355X: known gains with mean |e*| = 0.1365 are recovered to a mean error of 0.0224 in 120 steps
at EXPOSURE_LR, the field frozen (`test_known_gains_are_recovered`, which holds the trajectory)."""
import dataclasses
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import test_gpu_reproducible_step as R
from test_gpu_guarded_trainer import SHAPE, _nan_batch
from test_gpu_pose_trainer import _trainer
from test_gpu_transforms_loader import capture  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
EXPOSURE_LR = 5e-3


def test_off_by_default_nothing_is_added(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.delenv("CNC_EXPOSURE_LR", raising=False)
    tr = _trainer(cuda, tmp_path, capture[0])
    assert tr.cfg.exposure_lr == 0.0 and tr.cfg.exposure_from == 0
    assert tr.exposure is None and tr.opt_exposure is None
    keys = set()
    fetch = tr.dataset.fetch
    tr.dataset.fetch = lambda: (lambda d: (keys.update(d), d)[1])(fetch())
    lines = []
    tr.train(steps=6, log=lines.append)
    torch.cuda.synchronize()
    assert keys == {"pixels", "rays", "color_bkgd"}
    assert not tr.dataset.train.with_camera_ids
    assert not os.path.exists(os.path.join(tr.cfg.out_dir, "exposures.json"))
    assert lines and not any("gain" in ln or "exposure" in ln for ln in lines)


def test_environment_variable_switches_it_on(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    monkeypatch.setenv("CNC_EXPOSURE_LR", "2e-3")
    tr = _trainer(cuda, tmp_path, capture[0])
    grp = tr.opt_exposure.param_groups[0]
    assert tr.exposure is not None and grp["lr"] == 2e-3 and grp["weight_decay"] == 0 and grp["fused"]
    assert tr.dataset.train.with_camera_ids and tr._exposure_foreground            # the capture's images carry alpha
    assert tuple(tr.exposure.log_gain.shape) == (len(tr.dataset.train), 3) and not bool(tr.exposure.log_gain.any())
    assert torch.equal(tr.exposure.gains(), torch.ones_like(tr.exposure.log_gain))


@pytest.mark.parametrize("with_others", [False, True])
def test_reproducible_runs_give_equal_gains(cuda, capture, tmp_path, with_others):  # noqa: F811
    """One image per batch (`batch_over_images=False`), so that some cameras never get a ray in 10 steps: their log-gain
    must stay exactly zero, every other camera's must move, and two runs from one seed agree bit for bit — alone, and next
    to pose refinement and the distortion loss."""
    kw = dict(pose_lr=5e-3, distortion_weight=1e-3) if with_others else {}
    runs = []
    for k in range(2):
        tr = _trainer(cuda, tmp_path / str(k), capture[0], batch_over_images=False, reproducible=True,
                      exposure_lr=EXPOSURE_LR, **kw)
        seen = set()
        fetch = tr.dataset.fetch
        tr.dataset.fetch = lambda: (lambda d: (seen.update(d["camera_ids"].unique().tolist()), d)[1])(fetch())
        taken = [tr.train_step(s, want_stats=False) for s in range(10)]
        torch.cuda.synchronize()
        assert all(t is not None for t in taken)
        runs.append((tr.exposure.log_gain.detach().clone(), seen))
    (e0, seen0), (e1, seen1) = runs
    assert seen0 == seen1 and 0 < len(seen0) < e0.shape[0], seen0
    assert R._bits(e0).equal(R._bits(e1))
    moved = set(torch.nonzero(e0.abs().sum(dim=1) > 0).view(-1).tolist())
    assert moved == seen0, (moved, seen0)
    assert bool(torch.isfinite(e0).all())


def test_guarded_step_skips_the_gains_too(cuda, capture, tmp_path):  # noqa: F811
    tr = _trainer(cuda, tmp_path, capture[0], reproducible=True, guarded_step=True, exposure_lr=EXPOSURE_LR)
    for s in range(3):
        assert tr.train_step(s) is not None
    assert tr.step_guard.stats() == {"skipped": 0, "reasons": 0}

    def state():
        torch.cuda.synchronize()
        st = tr.opt_exposure.state[tr.exposure.log_gain]
        return {"log_gain": tr.exposure.log_gain.detach().clone(),
                **{k: v.detach().clone() for k, v in st.items() if isinstance(v, torch.Tensor)}}
    before = state()
    assert {"exp_avg", "exp_avg_sq", "step"} <= set(before) and bool(before["log_gain"].abs().sum() > 0)
    tr._next_data = _nan_batch(tr)
    assert "camera_ids" in tr._next_data
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = tr.train_step(3)
    after = state()
    assert out is not None and out["mse"] != out["mse"]
    assert tr.step_guard.stats()["skipped"] == 1
    for k in before:
        assert R._bits(before[k]).equal(R._bits(after[k])), k
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tr.train_step(4) is not None
    later = state()
    assert not torch.equal(later["log_gain"], before["log_gain"]) and float(later["step"]) == float(before["step"]) + 1
    assert bool(torch.isfinite(later["log_gain"]).all())


def test_envmap_render_is_taken_as_complete(cuda, capture, tmp_path):  # noqa: F811
    """With the learned background the render is called as without the option and the gain covers its whole output: the
    step runs, and the gains, the map and the field all move."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (the map's warning about a capture with alpha)
        tr = _trainer(cuda, tmp_path, capture[0], reproducible=True, background="envmap", envmap_resolution=4,
                      exposure_lr=EXPOSURE_LR)
    texture = tr.envmap.texture.detach().clone()
    for s in range(4):
        assert tr.train_step(s) is not None
    torch.cuda.synchronize()
    assert bool(tr.exposure.log_gain.abs().sum() > 0) and bool(torch.isfinite(tr.exposure.log_gain).all())
    assert not torch.equal(tr.envmap.texture.detach(), texture)


def test_known_gains_are_recovered(cuda, capture, tmp_path):  # noqa: F811
    """Every frame scaled down to 0.7 of itself (so that a gained value stays below 255: asserted); 200 steps with the
    option off; then training camera k's RGB becomes round(RGB exp(e*_k)) in the loader's device images, with e* fixed,
    centred per channel and max |e*| = 0.3; the field's learning rates go to 0, the option comes on, and after 120 more
    steps the mean |e - e*| over cameras and channels lies below its starting value mean |e*| with the field untouched.
    Only the decrease is asserted.

    Measured on the MI355X: mean |e - e*| = 0.1365 at the start ends at 0.0224 after 120 steps at EXPOSURE_LR (ratio
    0.16); at every 20th step: 0.0748, 0.0389, 0.0238, 0.0201, 0.0218, 0.0224 — it settles at a few steps of the rate."""
    tr = _trainer(cuda, tmp_path, capture[0])
    loader = tr.dataset.train
    C = len(loader)
    torch.cuda.synchronize()
    loader.images[..., :3] = torch.round(loader.images[..., :3].float() * 0.7).to(torch.uint8)
    tr._next_data = None                                     # (drawn from the images as they were)
    for s in range(200):
        tr.train_step(s, want_stats=False)
    torch.cuda.synchronize()
    e_true = np.random.default_rng(4).uniform(-1.0, 1.0, (C, 3))
    e_true -= e_true.mean(axis=0)
    e_true *= 0.3 / np.abs(e_true).max()
    assert np.abs(e_true).max() <= 0.3 + 1e-12 and np.allclose(e_true.mean(axis=0), 0.0, atol=1e-15)
    target = torch.from_numpy(e_true).to(cuda)
    gained = loader.images[..., :3].double() * torch.exp(target)[:, None, None, :]
    assert float(gained.max()) < 254.5                       # no value reaches 255: nothing clips
    loader.images[..., :3] = torch.round(gained).to(torch.uint8)
    tr._next_data = None
    for opt in (tr.opt, tr.opt2):
        for g in opt.param_groups:
            g["lr"] = 0.0
    tr.enable_exposure_compensation(EXPOSURE_LR)
    field_before = [p.detach().clone() for p in tr.field.parameters()]
    start = float(np.abs(e_true).mean())
    errs = []
    for s in range(200, 320):
        tr.train_step(s, want_stats=False)
        if (s + 1) % 20 == 0:
            errs.append(float((tr.exposure.effective().double() - target).abs().mean()))
    torch.cuda.synchronize()
    print(f"EXPOSURE RECOVERY: mean |e - e*| {start:.4f} -> {[round(v, 4) for v in errs]} (ratio {errs[-1] / start:.3f})")
    assert all(torch.equal(a, b.detach()) for a, b in zip(field_before, tr.field.parameters())), "the field moved"
    assert errs[-1] < start


def test_requests_that_cannot_work_raise(cuda, capture, tmp_path):  # noqa: F811
    from cnc_amd.trainer import Trainer
    with pytest.raises(ValueError, match="TransformsLoader"):
        Trainer(R._cfg(tmp_path, seed=3, exposure_lr=1e-3, **SHAPE), device=cuda)            # the synthetic dataset
    tr = _trainer(cuda, tmp_path, capture[0])
    tr.dp, tr.world = True, 2
    with pytest.raises(ValueError, match="data-parallel"):
        tr.enable_exposure_compensation(1e-3)
    tr.dp, tr.world = False, 1
    for rate in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="positive"):
            tr.enable_exposure_compensation(rate)
    assert tr.exposure is None and tr.opt_exposure is None and not tr.dataset.train.with_camera_ids
    with pytest.raises(ValueError, match="positive"):                                        # a negative rate in the config
        Trainer(R._cfg(tmp_path / "neg", seed=3, aabb=tuple(tr.dataset.train.aabb.tolist()), exposure_lr=-1.0, **SHAPE),
                device=cuda, dataset=tr.dataset)
    tr.enable_exposure_compensation(1e-3, start=5)           # ... and the plain one-process Trainer takes it
    assert tr.exposure is not None and tr.dataset.train.with_camera_ids and tr._exposure_from == 5
    for s in range(7):                                       # the gains stay until step 5
        tr.train_step(s, want_stats=False)
        torch.cuda.synchronize()
        assert bool(tr.exposure.log_gain.any()) == (s >= 5), s


def test_cli_writes_the_gains_and_the_container_holds_none(cuda, capture, tmp_path, monkeypatch):  # noqa: F811
    from cnc_amd import train
    from cnc_amd.container import section_sizes
    root = capture[0]
    made = []

    class Recording(train.Trainer):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    monkeypatch.setattr(train, "Trainer", Recording)
    monkeypatch.delenv("CNC_EXPOSURE_LR", raising=False)
    monkeypatch.chdir(tmp_path)
    out_dir = tmp_path / "bits"
    a = train.build_parser().parse_args([])
    assert a.refine_exposure == 0.0 and a.refine_exposure_from == 0
    argv = ["--data_root", root, "--scene", "ball_lens", "--dataset", "transforms", "--max_steps", "40", "--n_features", "2",
            "--sample_num", "20000", "--test_views", "1", "--log2_hashmap_size", "14", "--log2_hashmap_size_2D", "12",
            "--results", str(tmp_path / "out.txt"), "--out_dir", str(out_dir), "--refine-exposure", "2e-3",
            "--refine-exposure-from", "5"]
    train.main(argv)
    tr = made[0]
    assert tr.cfg.exposure_lr == 2e-3 and tr.cfg.exposure_from == 5 and tr.exposure is not None
    doc = json.load(open(out_dir / "exposures.json"))
    src = json.load(open(os.path.join(root, "ball_lens", "transforms.json")))
    training = [f["file_path"] for i, f in enumerate(src["frames"]) if i % 8 != 0]
    assert [f["file_path"] for f in doc["frames"]] == training and len(training) == len(tr.dataset.train)
    lg = np.asarray([f["log_gain"] for f in doc["frames"]])
    gain = np.asarray([f["gain"] for f in doc["frames"]])
    assert lg.shape == (len(training), 3) and np.abs(lg).max() > 0
    assert np.all(np.abs(lg.sum(axis=0)) <= len(training) * 2.0 ** -23 * np.abs(lg).max())  # zero within float32 rounding
    assert np.allclose(gain, np.exp(lg), rtol=1e-12)
    assert np.allclose(lg, tr.exposure.effective().cpu().numpy(), atol=1e-6)
    # the container holds no gains: a Trainer built without the option loads it and renders at gain 1
    path = str(tmp_path / "scene.cnc")
    tr.save_container(path)
    assert not any("exposure" in k or "gain" in k for k in section_sizes(path))
    from cnc_amd.trainer import Trainer
    fresh = Trainer(dataclasses.replace(tr.cfg, exposure_lr=0.0, exposure_from=0), device=cuda, dataset=tr.dataset)
    assert fresh.exposure is None
    fresh.load_container(path)
    assert math.isfinite(fresh.evaluate(1))
