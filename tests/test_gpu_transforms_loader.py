"""GPU: `TransformsLoader` end to end on a capture the test writes — the procedural ball seen through an OPENCV lens, 9
views of 24 x 18 pixels, colours from `SyntheticBallDataset._shade` on the twin's rays, as PNGs plus transforms.json —
and a Trainer at the small configuration of tests/test_gpu_distortion_trainer.py on it.  No PSNR claim at this size."""
import math
import os

import numpy as np
import pytest
import torch

import camera_twin as T
from test_camera_twin import write_capture
from test_gpu_cameras import ULP, VIEWDIR_BOUND
from test_gpu_reproducible_step import _cfg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N, W, H = 9, 24, 18
LENS = {"k1": -0.28, "k2": 0.07, "p1": 2e-4, "p2": -1e-4}
INTR = {"fl_x": 26.0, "fl_y": 26.0, "cx": 12.0, "cy": 9.0, "w": W, "h": H}
ROW8 = [LENS["k1"], LENS["k2"], LENS["p1"], LENS["p2"], 0, 0, 0, 0]


def _ball_poses():
    from cnc_amd.datasets import SyntheticBallDataset
    p = SyntheticBallDataset._poses(N, torch.Generator().manual_seed(77)).numpy()          # [n, 3, 4], OpenGL axes
    return np.concatenate([p, np.tile(np.asarray([[[0, 0, 0, 1]]], np.float32), (N, 1, 1))], 1).astype(np.float32)


@pytest.fixture(scope="module")
def capture(tmp_path_factory):
    """(root, images [n, H, W, 4] uint8, poses): the ball through the lens, and the same files without coefficients."""
    from cnc_amd.datasets import SyntheticBallDataset
    root = str(tmp_path_factory.mktemp("captures"))
    poses = _ball_poses()
    table = T.camera_table(np.tile(np.asarray([[26.0, 26.0, 12.0, 9.0]], np.float32), (N, 1)), poses,
                           np.tile(np.asarray([ROW8], np.float32), (N, 1)))
    px, py = T.frame_pixels(W, H)
    shader = SyntheticBallDataset.__new__(SyntheticBallDataset)
    images = np.zeros((N, H, W, 4), np.uint8)
    for i in range(N):
        o, d = T.camera_rays(table, T.OPENCV, True, np.full(W * H, i), px, py)
        rgb, alpha = shader._shade(torch.from_numpy(o).float(), torch.from_numpy(d).float())
        images[i] = (torch.cat([rgb, alpha], -1) * 255).round().to(torch.uint8).numpy().reshape(H, W, 4)
    assert 0.1 < (images[..., 3] > 0).mean() < 0.9                                     # the ball is in view, with rim
    for scene, meta in (("ball_lens", dict(INTR, **LENS)), ("ball_plain", INTR)):
        write_capture(root, scene, n=N, W=W, H=H, meta=dict(meta, aabb=[-1.5] * 3 + [1.5] * 3), images=images)
        # write_capture draws poses of its own: put the ball's in
        import json
        path = os.path.join(root, scene, "transforms.json")
        doc = json.load(open(path))
        for fr, pose in zip(doc["frames"], poses):
            fr["transform_matrix"] = pose.tolist()
        json.dump(doc, open(path, "w"))
    return root, images, poses, table


def _bound(golden_err):
    return VIEWDIR_BOUND + 4 * golden_err


@pytest.fixture(scope="module")
def ref_err():
    return float(np.load(os.path.join(HERE, "golden", "cameras.npz"))["ref_err"])


def test_views_and_batches_match_the_twin_and_the_files(cuda, capture, ref_err):
    from cnc_amd.datasets import TransformsLoader
    root, images, poses, table = capture
    test = TransformsLoader("ball_lens", root, "test", device=cuda)
    train = TransformsLoader("ball_lens", root, "train", num_rays=4099, color_bkgd_aug="random", device=cuda)
    assert (len(train), len(test)) == (7, 2) and test.camera_model == "OPENCV" and test.cameras.is_cuda
    held = [0, 8]
    px, py = T.frame_pixels(W, H)
    for i, frame in enumerate(held):
        out = test[i]
        o, d = T.camera_rays(table, T.OPENCV, True, np.full(W * H, frame), px, py)
        assert out["rays"].origins.shape == (H, W, 3) and out["pixels"].shape == (H, W, 3)
        assert np.array_equal(out["rays"].origins.cpu().numpy().reshape(-1, 3), o.astype(np.float32))
        assert np.abs(out["rays"].viewdirs.cpu().numpy().reshape(-1, 3) - d).max() <= _bound(ref_err)
        assert np.abs(out["pixels"].cpu().numpy().reshape(-1, 3)
                      - T.blend(images[frame].reshape(-1, 4), [1.0, 1.0, 1.0])).max() <= 2.0 ** -23
    kept = [i for i in range(N) if i % 8]
    train.seed_sampling(9)
    batch = train[0]
    train.seed_sampling(9)
    ids, x, y, _ = train._pixels_to_sample(0, cuda)
    bkgd = train._background(cuda)
    ids, x, y = ids.cpu().numpy(), x.cpu().numpy(), y.cpu().numpy()
    assert torch.equal(bkgd, batch["color_bkgd"]) and batch["pixels"].shape == (4099, 3)
    o, d = T.camera_rays(table[kept], T.OPENCV, True, ids, x, y)
    assert np.array_equal(batch["rays"].origins.cpu().numpy(), o.astype(np.float32))
    assert np.abs(batch["rays"].viewdirs.cpu().numpy() - d).max() <= _bound(ref_err)
    assert np.abs(batch["pixels"].cpu().numpy() - T.blend(images[kept][ids, y, x], bkgd.cpu().numpy())).max() <= 2.0 ** -23
    # the same seed gives the same batch twice
    train.seed_sampling(9)
    again = train[0]
    for a, b in ((again["pixels"], batch["pixels"]), (again["rays"].viewdirs, batch["rays"].viewdirs),
                 (again["rays"].origins, batch["rays"].origins), (again["color_bkgd"], batch["color_bkgd"])):
        assert torch.equal(a, b)
    # the device loader and the host loader (torch restatement) see the same capture
    host = TransformsLoader("ball_lens", root, "test")
    assert np.abs(host[1]["rays"].viewdirs.numpy() - test[1]["rays"].viewdirs.cpu().numpy()).max() <= 2 * _bound(ref_err)


def test_the_lens_is_really_applied(cuda, capture):
    from cnc_amd.datasets import TransformsLoader
    root = capture[0]
    lens = TransformsLoader("ball_lens", root, "test", device=cuda)
    plain = TransformsLoader("ball_plain", root, "test", device=cuda)
    assert plain.camera_model == "PINHOLE" and lens.camera_model == "OPENCV"
    a, b = lens[0]["rays"], plain[0]["rays"]
    assert torch.equal(a.origins, b.origins)
    assert float((a.viewdirs - b.viewdirs).abs().max()) > 1e-3


def test_trainer_runs_on_the_capture(cuda, capture, tmp_path):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    from cnc_amd.trainer import Trainer
    root = capture[0]
    train = TransformsLoader("ball_lens", root, "train", num_rays=512, color_bkgd_aug="random", device=cuda)
    test = TransformsLoader("ball_lens", root, "test", device=cuda)
    torch.manual_seed(1234)
    tr = Trainer(_cfg(tmp_path, seed=3, aabb=tuple(train.aabb.tolist())), device=cuda, dataset=LoaderDataset(train, test))
    stats = [tr.train_step(s) for s in range(20)]
    torch.cuda.synchronize()
    taken = [s for s in stats if s is not None]
    assert taken and all(math.isfinite(s["mse"]) and math.isfinite(s["bpp"]) for s in taken)
    Pgs, est_MB, coded_MB, prefix = tr.encode()
    assert coded_MB > 0 and math.isfinite(est_MB)
    e = tr.field.mlp_base
    tables = (e.encoding_xyz, e.encoding_xy, e.encoding_xz, e.encoding_yz)
    orig = [torch.where(t.params.data >= 0, 1.0, -1.0) for t in tables]
    tr.decode_into_field(Pgs, prefix)
    for t, o in zip(tables, orig):                        # as tests/test_gpu_trainer.py checks the round trip
        dec = t.params.data
        assert torch.all(dec.abs() == 1)
        uncoded = (dec == 1).all(dim=1)                   # never-written rows keep the init value
        assert torch.equal(dec[~uncoded], o[~uncoded])
