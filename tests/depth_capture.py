"""A 3-frame capture with measured depth, written with PIL and NumPy, for the depth loader tests (CPU and GPU): small RGBA
PNGs, frame 0 with a 16-bit PNG depth (counts), frame 1 with a `.npy` float depth (scene units, with a zero, a NaN and a
negative in it), frame 2 without depth.  (A pinhole ray never passes 90 degrees from the optical axis: `c <= 0` is exercised
through the C ABI in tests/test_gpu_depth_fetch.py.)"""
import json
import os

import numpy as np

H, W = 5, 7
SCENE = "cap"


def _pose(az, el, dist=4.0):
    eye = dist * np.array([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    m = np.eye(4)
    m[:3, :3] = np.stack([right, up, -fwd], axis=-1)           # OpenGL: the camera looks down -z
    m[:3, 3] = eye
    return m


def write(root, scale_key="depth_unit_scale_factor", scale=0.002, euclidean=None, depth_shape=(H, W), with_depth=True):
    """-> (planes float32 [3, H, W] in scene units as the loader must read them, the meta dict).  `scale_key` None: no scale
    key in the file (the default, 0.001, applies)."""
    from PIL import Image
    rng = np.random.default_rng(7)
    scene = os.path.join(str(root), SCENE)
    os.makedirs(scene, exist_ok=True)
    frames = []
    for k in range(3):
        rgba = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        Image.fromarray(rgba).save(os.path.join(scene, f"f{k}.png"))
        frames.append({"file_path": f"f{k}", "transform_matrix": _pose(0.7 * k + 0.2, 0.3 - 0.2 * k).tolist()})
    counts = rng.integers(1000, 3000, depth_shape).astype(np.uint16)
    counts[0, 0] = 0                                            # a pixel without a measurement
    metres = rng.uniform(2.0, 6.0, depth_shape).astype(np.float32)
    metres[1, 2], metres[2, 3], metres[3, 4] = 0.0, np.nan, -1.5
    if with_depth:
        Image.fromarray(counts).save(os.path.join(scene, "d0.png"))
        np.save(os.path.join(scene, "d1.npy"), metres)
        frames[0]["depth_file_path"], frames[1]["depth_file_path"] = "d0.png", "d1.npy"
    meta = {"fl_x": 9.0, "fl_y": 9.5, "cx": 3.4, "cy": 2.6, "w": W, "h": H, "frames": frames}
    if scale_key is not None:
        meta[scale_key] = scale
    if euclidean is not None:
        meta["is_euclidean_depth"] = euclidean
    for name in ("transforms_train.json", "transforms_test.json"):
        with open(os.path.join(scene, name), "w") as fp:
            json.dump(meta, fp)
    planes = np.zeros((3,) + tuple(depth_shape), np.float32)
    planes[0] = counts.astype(np.float32) * np.float32(0.001 if scale_key is None else scale)
    planes[1] = metres
    return planes, meta


def loader(root, device, num_rays=64, seed=5, **kw):
    from cnc_amd.datasets import TransformsLoader
    ld = TransformsLoader(SCENE, str(root), "train", num_rays=num_rays, device=device, **kw)
    ld.seed_sampling(seed)
    return ld
