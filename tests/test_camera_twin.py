"""CPU: the camera twin (tests/camera_twin.py) against the reference's numbers (tests/golden/cameras.npz), the torch
restatements of cnc_amd/nerfacc/cameras.py, `TransformsLoader` on captures written into tmp_path, and the driver's
dataset choice."""
import json
import os
import re

import numpy as np
import pytest
import torch

import camera_twin as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ULP = 2.0 ** -24
# viewdirs of the pinhole chain against float64, per component of a unit vector, first order: three roundings per
# camera-space component ((px - cx) + 0.5) / fx, six per rotated component (three products, two adds, and the inherited
# one) weighted by at most sqrt(3) over the three terms, and the normalisation (squares, sum, sqrt, division)
VIEWDIR_BOUND = 24 * ULP


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "cameras.npz"))


def test_twin_matches_the_reference_numbers(golden):
    g = golden
    eps, iters = float(g["eps"]), int(g["iters"])
    assert float(g["ref_err"]) == max(float(g[f"ref_err_{i}"]) for i in range(int(g["n_sets"])))
    assert float(g["ref_err"]) <= 4.5 * ULP                    # the reference's float32 twin on well-conditioned inputs
    for i in range(int(g["n_sets"])):
        uv, p = g[f"uv_{i}"], g[f"params_{i}"]
        want = T.undistort_newton(uv, p, eps, iters, np.float64)
        # the float64 twin is the inverse: back through the forward model it lands on the float32 input it was given
        assert np.abs(T.distort(want, p.astype(np.float64)) - uv).max() < 1e-12
        # the golden's error figure is reproduced from its own arrays
        assert np.abs(g[f"undist_{i}"].astype(np.float64) - want).max() == float(g[f"ref_err_{i}"])
        # the float32 mode, early exit and another operation order, stays within the reference's own error of float64
        info = {}
        mine = T.undistort_newton(uv, p, eps, iters, np.float32, info)
        assert mine.dtype == np.float32 and info["rounds"].max() < iters and not info["det_stop"].any()
        assert np.abs(mine.astype(np.float64) - want).max() <= float(g["ref_err"])
        # forward model: float64 twin against the reference's float32 output, one float32 rounding chain apart
        fwd = T.distort(g["ideal"].astype(np.float32), p, np.float64)
        assert np.abs(fwd - g[f"dist_{i}"]).max() <= 8 * ULP
    for i in range(int(g["n_fish"])):
        k = g[f"fish_params_{i}"].astype(np.float64)
        assert np.abs(T.distort_fisheye(g["fish_ideal"], k) - g[f"fish_dist_{i}"]).max() < 1e-14
        info = {}
        back = T.undistort_fisheye(g[f"fish_uv_{i}"], g[f"fish_params_{i}"], eps, iters, np.float64, info)
        assert info["converged"].all() and info["rounds"].max() <= 3
        assert np.abs(back - g["fish_ideal"]).max() < 4e-7       # the float32 rounding of uv, amplified by 1 / cos^2
    back = T.undistort_fixed_point(g["prism_uv"], g["prism_params"], 40, np.float64)
    assert np.abs(back - g["ideal"]).max() < 4e-7


def test_round_trip_through_the_torch_restatements(golden):
    from cnc_amd.nerfacc import cameras
    g = golden
    for i in range(int(g["n_sets"])):
        uv, p = torch.from_numpy(g[f"uv_{i}"]), torch.from_numpy(g[f"params_{i}"])
        und = cameras._opencv_lens_undistortion(uv, p, 1e-6, 10)
        assert und.dtype == torch.float32 and und.shape == uv.shape
        want = T.undistort_newton(g[f"uv_{i}"], g[f"params_{i}"], 1e-6, 10, np.float64)
        assert np.abs(und.numpy().astype(np.float64) - want).max() <= 2 * float(g["ref_err"])
        assert (cameras._opencv_lens_distortion(und, p) - uv).abs().max() <= 8 * ULP
        assert np.abs(cameras._opencv_lens_distortion(torch.from_numpy(g["ideal"]), p.double()).numpy()
                      - T.distort(g["ideal"], g[f"params_{i}"].astype(np.float64))).max() < 1e-14
    for i in range(int(g["n_fish"])):
        uv, k = torch.from_numpy(g[f"fish_uv_{i}"]), torch.from_numpy(g[f"fish_params_{i}"])
        und = cameras.opencv_lens_undistortion_fisheye(uv, k)          # host tensors: the restatement
        want = T.undistort_fisheye(g[f"fish_uv_{i}"], g[f"fish_params_{i}"], 1e-6, 10, np.float64)
        assert und.dtype == torch.float32 and np.abs(und.numpy() - want).max() <= 16 * ULP
        assert (cameras._opencv_lens_distortion_fisheye(und, k) - uv).abs().max() <= 16 * ULP
    # a row that cannot converge keeps its input; the centre maps to the centre
    far = torch.tensor([[1.2, -0.7], [0.0, 0.0]])
    out = cameras._opencv_lens_undistortion_fisheye(far, torch.tensor([0.05, -0.01, 0.002, -3e-4]), 1e-6, 1)
    assert torch.equal(out, far)


@pytest.mark.parametrize("n", [0, 1, 2, 4, 8])
def test_padding_of_short_coefficient_rows(golden, n):
    from cnc_amd.nerfacc import cameras
    full = torch.tensor([0.12, -0.05, 5e-4, -3e-4, 0.01, 0.05, -0.02, 0.004])
    uv = torch.from_numpy(golden["uv_3"][:257]).reshape(257, 1, 2).expand(257, 3, 2)
    got = cameras.opencv_lens_undistortion(uv, full[:n])
    if n == 0:
        assert got is uv
        return
    padded = torch.cat([full[:n], torch.zeros(8 - n)])
    assert got.shape == uv.shape and torch.equal(got, cameras._opencv_lens_undistortion(uv, padded))
    assert torch.equal(got, cameras.opencv_lens_undistortion(uv, padded.expand(257, 3, 8)))
    want = T.undistort_newton(uv.numpy(), padded.numpy(), 1e-6, 10, np.float64)
    assert np.abs(got.numpy() - want).max() <= 2 * float(golden["ref_err"])
    with pytest.raises(AssertionError):
        cameras.opencv_lens_undistortion(uv, full[:3])


def test_the_pinhole_torch_chain_stays_inside_the_viewdir_bound():
    """The bound the GPU test holds cnc_camera_rays to (24 x 2^-24 per component) is met by the float32 chain of
    `_PosedImages.__getitem__` itself against the float64 twin, on random cameras and pixels."""
    from cnc_amd.datasets import _PosedImages
    rng = np.random.default_rng(3)
    worst = 0.0
    for opengl in (True, False):
        for trial in range(8):
            poses = _poses(rng, 5)
            fx, fy, cx, cy = rng.uniform(300, 1400), rng.uniform(300, 1400), rng.uniform(200, 600), rng.uniform(200, 600)
            W, H, n = 800, 780, 4099
            ld = _PosedImages.__new__(_PosedImages)
            ld.OPENGL_CAMERA, ld.training, ld.num_rays, ld.batch_over_images = opengl, True, n, True
            ld.color_bkgd_aug, ld.WIDTH, ld.HEIGHT = "white", W, H
            ld.images = torch.zeros(5, H, W, 4, dtype=torch.uint8)
            ld.camtoworlds = torch.from_numpy(poses)
            ld.K = torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float32)
            gen = torch.Generator().manual_seed(trial)
            ld._gen = gen
            state = gen.get_state()
            rays = ld[0]["rays"]
            gen.set_state(state)
            ids, x, y, _ = ld._pixels_to_sample(0, torch.device("cpu"))
            table = T.camera_table(np.tile(ld.K.numpy()[[0, 1, 0, 1], [0, 1, 2, 2]], (5, 1)), poses)
            o, d = T.camera_rays(table, T.PINHOLE, opengl, ids.numpy(), x.numpy(), y.numpy())
            assert np.array_equal(rays.origins.numpy(), o.astype(np.float32))
            worst = max(worst, float(np.abs(rays.viewdirs.numpy().astype(np.float64) - d).max()))
    assert worst <= VIEWDIR_BOUND, worst / ULP


def _poses(rng, n, radius=4.0):
    """Camera-to-world [n, 4, 4] float32: cameras on a sphere looking at the origin (OpenGL axes), slightly rolled."""
    out = np.zeros((n, 4, 4), np.float32)
    for i in range(n):
        eye = rng.normal(size=3)
        eye *= radius / np.linalg.norm(eye)
        fwd = -eye / np.linalg.norm(eye)
        up = rng.normal(size=3)
        right = np.cross(fwd, up)
        right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        out[i, :3, 0], out[i, :3, 1], out[i, :3, 2], out[i, :3, 3], out[i, 3, 3] = right, up, -fwd, eye, 1.0
    return out


def write_capture(root, scene, *, n=9, W=24, H=18, meta=None, per_frame=None, split_files=False, alpha=True, ext=".png",
                  with_ext=False, seed=0, images=None):
    """A capture under root/scene: n frames of seeded noise (or `images` [n, H, W, 3|4] uint8), transforms.json or
    transforms_{train,test}.json (frames 0, 8, .. as test).  -> (images, poses)."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    d = os.path.join(root, scene)
    os.makedirs(os.path.join(d, "images"), exist_ok=True)
    poses = _poses(rng, n)
    if images is None:
        images = rng.integers(0, 256, (n, H, W, 4 if alpha else 3), dtype=np.uint8)
    frames = []
    for i in range(n):
        name = f"images/frame_{i:03d}"
        Image.fromarray(images[i]).save(os.path.join(d, name + ext))
        fr = {"file_path": name + (ext if with_ext else ""), "transform_matrix": poses[i].tolist()}
        fr.update((per_frame or {}).get(i, {}))
        frames.append(fr)
    meta = dict(meta or {})
    if split_files:
        for split, keep in (("train", lambda i: i % 8 != 0), ("test", lambda i: i % 8 == 0)):
            with open(os.path.join(d, f"transforms_{split}.json"), "w") as fp:
                json.dump(dict(meta, frames=[f for i, f in enumerate(frames) if keep(i)]), fp)
    else:
        with open(os.path.join(d, "transforms.json"), "w") as fp:
            json.dump(dict(meta, frames=frames), fp)
    return images, poses


OPENCV_META = {"fl_x": 30.0, "fl_y": 31.0, "cx": 12.5, "cy": 8.5, "w": 24, "h": 18, "k1": -0.28, "k2": 0.07, "p1": 2e-4,
               "p2": -1e-4}


def _check_view(loader, i, images, poses, intr, model, lens, bound):
    out = loader[i]
    H, W = images.shape[1:3]
    px, py = T.frame_pixels(W, H)
    table = T.camera_table(np.asarray([intr], np.float32), poses[i:i + 1], np.asarray([lens], np.float32))
    o, d = T.camera_rays(table, model, True, np.zeros(W * H, int), px, py)
    assert out["rays"].origins.shape == (H, W, 3) and out["pixels"].shape == (H, W, 3)
    assert np.array_equal(out["rays"].origins.numpy().reshape(-1, 3), o.astype(np.float32))
    assert np.abs(out["rays"].viewdirs.numpy().reshape(-1, 3) - d).max() <= bound
    rgba = images[i].reshape(-1, images.shape[-1])
    if rgba.shape[1] == 3:
        rgba = np.concatenate([rgba, np.full((rgba.shape[0], 1), 255, np.uint8)], 1)
    assert np.abs(out["pixels"].numpy().reshape(-1, 3) - T.blend(rgba, [1.0, 1.0, 1.0])).max() <= 2 * ULP
    assert torch.equal(out["color_bkgd"], torch.ones(3))


def test_transforms_loader_models_layouts_and_hold_out(tmp_path, golden):
    from cnc_amd.datasets import LoaderDataset, TransformsLoader
    root = str(tmp_path)
    lens_bound = VIEWDIR_BOUND + 4 * float(golden["ref_err"])
    # one file, OPENCV implied by the coefficients, global intrinsics, 17 frames: 0, 8, 16 are held out
    images, poses = write_capture(root, "lens", n=17, meta=dict(OPENCV_META, aabb=[-1, -1.5, -2, 1, 1.5, 2]))
    train = TransformsLoader("lens", root, "train", num_rays=64)
    test = TransformsLoader("lens", root, "test")
    assert (len(train), len(test)) == (14, 3) and train.camera_model == test.camera_model == "OPENCV"
    assert train.training and not test.training and (train.HEIGHT, train.WIDTH) == (18, 24)
    assert train.aabb.tolist() == [-1, -1.5, -2, 1, 1.5, 2] and train.scene_bbox.shape == (2, 3)
    assert np.array_equal(test.camtoworlds.numpy(), poses[[0, 8, 16]])
    assert np.array_equal(train.camtoworlds.numpy(), poses[[i for i in range(17) if i % 8]])
    assert train.cameras.shape == (14, 24) and train.cameras[0, 16:].tolist() == pytest.approx([-0.28, 0.07, 2e-4, -1e-4, 0, 0, 0, 0])
    _check_view(test, 1, images[[0, 8, 16]], poses[[0, 8, 16]], [30.0, 31.0, 12.5, 8.5], T.OPENCV,
                [-0.28, 0.07, 2e-4, -1e-4, 0, 0, 0, 0], lens_bound)
    # a training batch: the base class's draws, the rays of those pixels, the files' colours
    train.seed_sampling(5)
    batch = train[0]
    train.seed_sampling(5)
    ids, x, y, _ = train._pixels_to_sample(0, torch.device("cpu"))
    assert batch["pixels"].shape == (64, 3) and batch["rays"].viewdirs.shape == (64, 3)
    o, d = T.camera_rays(train.cameras.numpy(), T.OPENCV, True, ids.numpy(), x.numpy(), y.numpy())
    assert np.array_equal(batch["rays"].origins.numpy(), o.astype(np.float32))
    assert np.abs(batch["rays"].viewdirs.numpy() - d).max() <= lens_bound
    rgba = images[[i for i in range(17) if i % 8]][ids.numpy(), y.numpy(), x.numpy()]
    assert np.abs(batch["pixels"].numpy() - T.blend(rgba, [1.0, 1.0, 1.0])).max() <= 2 * ULP
    train.seed_sampling(5)
    again = train[0]
    assert torch.equal(again["pixels"], batch["pixels"]) and torch.equal(again["rays"].viewdirs, batch["rays"].viewdirs)
    ds = LoaderDataset(train, test)
    assert len(ds) == 3 and ds.view(4)["pixels"].shape == (18, 24, 3) and ds.fetch()["pixels"].shape == (64, 3)
    # two files, PINHOLE from camera_angle_x, RGB images without alpha (opaque), file_path with its extension
    images, poses = write_capture(root, "pin", n=9, meta={"camera_angle_x": 0.7}, split_files=True, alpha=False, ext=".jpg",
                                  with_ext=True)
    test = TransformsLoader("pin", root, "test")
    train = TransformsLoader("pin", root, "train", num_rays=8)
    assert (len(train), len(test)) == (7, 2) and test.camera_model == "PINHOLE" and test.aabb is None
    focal = 0.5 * 24 / np.tan(0.35)
    assert float(test.K[0, 0]) == pytest.approx(focal) and float(test.K[1, 2]) == 9.0
    shown = np.asarray(test.images[:, :, :, :3])           # JPEG is lossy: compare with what the loader decoded
    assert bool((test.images[..., 3] == 255).all())
    _check_view(test, 1, shown[:, :, :, :3], poses[[0, 8]], [focal, focal, 12.0, 9.0], T.PINHOLE, [0] * 8, VIEWDIR_BOUND)
    # fisheye named by the file, per-frame intrinsics and coefficients over global ones
    per = {8: {"fl_x": 20.0, "fl_y": 21.0, "cx": 11.0, "cy": 9.5, "k1": 0.05, "k2": -0.01, "k3": 0.002, "k4": -3e-4}}
    meta = {"camera_model": "OPENCV_FISHEYE", "fl_x": 25.0, "cx": 12.0, "cy": 9.0, "k1": -0.02, "k2": 0.003, "k3": -5e-4, "k4": 1e-4}
    images, poses = write_capture(root, "fish", n=9, meta=meta, per_frame=per)
    test = TransformsLoader("fish", root, "test")
    assert test.camera_model == "OPENCV_FISHEYE" and test.cameras[0, :4].tolist() == [25.0, 25.0, 12.0, 9.0]
    fish_bound = VIEWDIR_BOUND + 32 * ULP
    _check_view(test, 0, images[[0, 8]], poses[[0, 8]], [25.0, 25.0, 12.0, 9.0], T.FISHEYE, [-0.02, 0.003, -5e-4, 1e-4], fish_bound)
    _check_view(test, 1, images[[0, 8]], poses[[0, 8]], [20.0, 21.0, 11.0, 9.5], T.FISHEYE, [0.05, -0.01, 0.002, -3e-4], fish_bound)


def test_transforms_loader_refuses_what_it_cannot_read(tmp_path):
    from PIL import Image
    from cnc_amd.datasets import TransformsLoader
    root = str(tmp_path)
    write_capture(root, "sizes", n=9, meta=OPENCV_META)
    odd = os.path.join(root, "sizes", "images", "frame_003.png")
    Image.fromarray(np.zeros((18, 25, 4), np.uint8)).save(odd)
    with pytest.raises(ValueError, match=re.escape(odd)):
        TransformsLoader("sizes", root, "train", num_rays=8)
    write_capture(root, "mixed", n=9, meta=OPENCV_META, per_frame={2: {"camera_model": "PINHOLE"}})
    with pytest.raises(ValueError, match="one camera_model per capture"):
        TransformsLoader("mixed", root, "train", num_rays=8)
    write_capture(root, "k4", n=9, meta=dict(OPENCV_META, camera_model="OPENCV", k4=0.1))
    with pytest.raises(ValueError, match="no k4"):
        TransformsLoader("k4", root, "train", num_rays=8)
    write_capture(root, "nofocal", n=9, meta={"w": 24})
    with pytest.raises(ValueError, match="neither fl_x nor camera_angle_x"):
        TransformsLoader("nofocal", root, "test")
    write_capture(root, "gone", n=9, meta=OPENCV_META)
    os.remove(os.path.join(root, "gone", "images", "frame_008.png"))
    with pytest.raises(FileNotFoundError, match="frame_008"):
        TransformsLoader("gone", root, "test")


def test_driver_picks_the_capture_and_its_box(tmp_path):
    from cnc_amd.train import build_parser, make_config_and_data
    root = str(tmp_path)
    write_capture(root, "desk", n=9, meta=dict(OPENCV_META, aabb=[-1, -1, -1, 1, 1, 2]))
    write_capture(root, "shelf", n=9, meta=OPENCV_META)
    cpu = torch.device("cpu")
    # auto-detected: a free scene name with a transforms*.json under it
    kind, cfg, ds = make_config_and_data(build_parser().parse_args(["--data_root", root, "--scene", "desk"]), cpu)
    assert kind == "transforms" and cfg.scene == "desk" and cfg.aabb == (-1.0, -1.0, -1.0, 1.0, 1.0, 2.0)
    assert type(ds.train).__name__ == "TransformsLoader" and len(ds) == 2 and cfg.test_views == 2
    # --aabb over the file's box
    args = build_parser().parse_args(["--data_root", root, "--scene", "desk", "--dataset", "transforms",
                                      "--aabb", "-2", "-2", "-2", "2", "2", "2"])
    assert make_config_and_data(args, cpu)[1].aabb == (-2.0, -2.0, -2.0, 2.0, 2.0, 2.0)
    # neither: the default box
    from cnc_amd.trainer import TrainConfig
    args = build_parser().parse_args(["--data_root", root, "--scene", "shelf"])
    assert make_config_and_data(args, cpu)[1].aabb == TrainConfig().aabb
    # the named scenes parse as before; a free name without a capture behind it is refused at the command line
    a = build_parser().parse_args(["--scene", "lego", "--data_root", root])
    assert a.scene == "lego" and make_config_and_data(a, cpu)[0] == "procedural"
    assert build_parser().parse_args([]).scene == "chair"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--data_root", root, "--scene", "nothing_here"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--data_root", root, "--scene", "desk", "--dataset", "tanks"])


def test_new_signatures_are_declared_in_the_header():
    from cnc_amd import _lib
    src = open(os.path.join(ROOT, "include", "cnc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("cnc_lens_undistort", "cnc_lens_undistort_fisheye", "cnc_camera_rays"):
        assert name in _lib.SIGNATURES
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert decl, f"{name} is not declared in include/cnc_hip.h"
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name])
    for const in ("CNC_CAMERA_ROW", "CNC_CAMERA_PINHOLE", "CNC_CAMERA_OPENCV", "CNC_CAMERA_FISHEYE"):
        m = re.search(r"#define\s+" + const + r"\s+(\d+)", src)
        assert m and int(m.group(1)) == getattr(_lib, const)


def test_dropin_name_resolves():
    import cnc_amd
    cnc_amd.install_dropins()
    from nerfacc.cameras import opencv_lens_undistortion, opencv_lens_undistortion_fisheye  # noqa: F401
    import nerfacc
    from cnc_amd.nerfacc import cameras
    assert opencv_lens_undistortion is cameras.opencv_lens_undistortion
    assert "opencv_lens_undistortion" not in nerfacc.__all__
    for name in ("_opencv_lens_distortion", "_opencv_lens_distortion_fisheye", "_opencv_lens_undistortion"):
        assert callable(getattr(cameras, name))
