"""Scene loaders for the CNC drivers: `SubjectLoader` (NeRF-synthetic: `transforms_{split}.json`
+ RGBA PNGs) and `SubjectLoader_Tanks` (Tanks&Temples in the NSVF layout: `intrinsics.txt`, `bbox.txt`,
`pose/*.txt`, `rgb/*.png`, split by file-name prefix); and, an extension, `TransformsLoader` (a capture in the
instant-ngp / nerfstudio `transforms.json` layout, with OpenCV lens distortion: rays from one HIP launch).

Interface of the reference's loaders (examples/datasets/nerf_synthetic.py:53-239, tanks.py:62-259): same
constructor arguments, `len()`, `loader[i]` -> {"pixels", "rays", "color_bkgd"}, `update_num_rays`, the
attributes the drivers read (`images`, `camtoworlds`, `K`, `HEIGHT`, `WIDTH`, `training`, and for T&T the scene
box and step size).  Images are read with PIL (imageio / cv2 are not available offline) and kept on the device as
uint8; rays are generated on the device.  No dataset ships with this repository: without a `data_root` the
trainer uses the procedural scene below (`SyntheticBallDataset`); `LoaderDataset` puts a pair of loaders behind the
three calls the Trainer makes.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from .render import Rays

_BKGD = {"white": 1.0, "black": 0.0}


def _rgba(path) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as img:
        return np.asarray(img.convert("RGBA"), dtype=np.uint8)


def _read_blender_split(scene_dir: str, split: str):
    """(images uint8 [n,H,W,4], camera-to-world [n,4,4], focal length in pixels) of one split."""
    with open(os.path.join(scene_dir, f"transforms_{split}.json")) as fp:
        meta = json.load(fp)
    frames = meta["frames"]
    images = np.stack([_rgba(os.path.join(scene_dir, fr["file_path"] + ".png")) for fr in frames])
    poses = np.asarray([fr["transform_matrix"] for fr in frames], dtype=np.float32)
    focal = 0.5 * images.shape[2] / np.tan(0.5 * float(meta["camera_angle_x"]))
    return images, poses, focal


class _PosedImages(torch.utils.data.Dataset):
    """Posed RGBA images on the device + pinhole ray generation.  Subclasses fill `images` (uint8 [n,H,W,4]),
    `camtoworlds` (float [n,3|4,4]) and `K` (3x3) and say whether the camera looks down -z (OpenGL) or +z."""

    OPENGL_CAMERA = True
    TRAIN_SPLITS = ("train", "trainval")

    def _configure(self, split, color_bkgd_aug, num_rays, near, far, batch_over_images):
        if color_bkgd_aug not in ("white", "black", "random"):
            raise AssertionError(color_bkgd_aug)
        self.split, self.num_rays, self.color_bkgd_aug = split, num_rays, color_bkgd_aug
        self.near = self.NEAR if near is None else near
        self.far = self.FAR if far is None else far
        self.batch_over_images = batch_over_images
        self.training = num_rays is not None and split in self.TRAIN_SPLITS

    def __len__(self):
        return self.images.shape[0]

    def update_num_rays(self, num_rays):
        self.num_rays = num_rays

    def seed_sampling(self, seed: int):
        """(extension) draw training images / pixels / random backgrounds from a generator of this loader's own
        instead of the global one — one seed per data-parallel rank."""
        self._gen = torch.Generator(device=self.images.device).manual_seed(int(seed))

    def _pixels_to_sample(self, index, dev):
        """(image ids, x, y, output shape): `num_rays` random pixels when training, else every pixel of image
        `index` in row-major order."""
        if self.training:
            n = self.num_rays
            g = getattr(self, "_gen", None)
            ids = (torch.randint(0, len(self), (n,), device=dev, generator=g) if self.batch_over_images
                   else torch.full((n,), index, device=dev))
            return (ids, torch.randint(0, self.WIDTH, (n,), device=dev, generator=g),
                    torch.randint(0, self.HEIGHT, (n,), device=dev, generator=g), (n,))
        cols, rows = torch.meshgrid(torch.arange(self.WIDTH, device=dev), torch.arange(self.HEIGHT, device=dev),
                                    indexing="xy")
        return torch.tensor([index], device=dev), cols.reshape(-1), rows.reshape(-1), (self.HEIGHT, self.WIDTH)

    def _background(self, dev):
        if self.training and self.color_bkgd_aug == "random":
            return torch.rand(3, device=dev, generator=getattr(self, "_gen", None))
        level = _BKGD.get(self.color_bkgd_aug, 1.0) if self.training else 1.0     # evaluation is always on white
        return torch.full((3,), level, device=dev)

    @torch.no_grad()
    def __getitem__(self, index):
        dev = self.images.device
        ids, x, y, shape = self._pixels_to_sample(index, dev)
        rgba = self.images[ids, y, x].to(torch.float32) / 255.0
        pose = self.camtoworlds[ids]
        # pixel centre -> camera-space direction; OpenGL cameras have y up and look down -z
        flip = -1.0 if self.OPENGL_CAMERA else 1.0
        cam = torch.stack([(x - self.K[0, 2] + 0.5) / self.K[0, 0],
                           (y - self.K[1, 2] + 0.5) / self.K[1, 1] * flip,
                           torch.full(x.shape, flip, dtype=torch.float32, device=dev)], dim=-1)
        world = torch.einsum("nk,njk->nj", cam, pose[:, :3, :3].expand(cam.shape[0], 3, 3))
        dirs = world / world.norm(dim=-1, keepdim=True)
        origins = pose[:, :3, 3].expand_as(dirs)
        colour, alpha = rgba[:, :3], rgba[:, 3:]
        bkgd = self._background(dev)
        return {"pixels": (colour * alpha + bkgd * (1.0 - alpha)).reshape(*shape, 3),
                "rays": Rays(origins=origins.reshape(*shape, 3), viewdirs=dirs.reshape(*shape, 3)),
                "color_bkgd": bkgd}


class SubjectLoader(_PosedImages):
    """One NeRF-synthetic scene."""

    SPLITS = ["train", "val", "trainval", "test"]
    SUBJECT_IDS = ["chair", "drums", "ficus", "hotdog", "lego", "materials", "mic", "ship"]
    NEAR, FAR = 2.0, 6.0
    OPENGL_CAMERA = True

    def __init__(self, subject_id: str, root_fp: str, split: str, color_bkgd_aug: str = "white",
                 num_rays: int = None, near: float = None, far: float = None,
                 batch_over_images: bool = True, device: torch.device = torch.device("cpu")):
        super().__init__()
        if split not in self.SPLITS:
            raise AssertionError(split)
        self._configure(split, color_bkgd_aug, num_rays, near, far, batch_over_images)
        scene_dir = os.path.join(root_fp, subject_id)
        parts = [_read_blender_split(scene_dir, s) for s in (("train", "val") if split == "trainval" else (split,))]
        images = np.concatenate([p[0] for p in parts])
        poses = np.concatenate([p[1] for p in parts])
        self.focal = parts[0][2]
        self.HEIGHT, self.WIDTH = images.shape[1:3]
        self.images = torch.from_numpy(images).to(device)
        self.camtoworlds = torch.from_numpy(poses).to(device)
        self.K = torch.tensor([[self.focal, 0.0, self.WIDTH / 2.0], [0.0, self.focal, self.HEIGHT / 2.0],
                               [0.0, 0.0, 1.0]], dtype=torch.float32, device=device)


class SubjectLoader_Tanks(_PosedImages):
    """One Tanks&Temples scene (NSVF layout; file names starting with 0_ are training views, 1_ test views).
    OpenCV camera convention.  `aabb` = the bounding box of bbox.txt scaled by 1.2 and `render_step_size` =
    4e-3 if the box's voxel size is >= 0.15 else 1e-3 (tanks.py:135-137)."""

    SPLITS = ["train", "test"]
    SUBJECT_IDS = ["Barn", "Caterpillar", "Family", "Ignatius", "Truck"]
    NEAR, FAR = 0.01, 6.0
    OPENGL_CAMERA = False
    TRAIN_SPLITS = ("train",)

    def __init__(self, subject_id: str, root_fp: str, split: str, color_bkgd_aug: str = "white",
                 num_rays: int = None, near: float = None, far: float = None,
                 batch_over_images: bool = True, device: torch.device = torch.device("cpu")):
        super().__init__()
        if split not in self.SPLITS:
            raise AssertionError(split)
        self._configure(split, color_bkgd_aug, num_rays, near, far, batch_over_images)
        scene_dir = os.path.join(root_fp, subject_id)
        tag = "0_" if split == "train" else "1_"
        names = sorted(f for f in os.listdir(os.path.join(scene_dir, "rgb")) if f.startswith(tag))
        images = np.stack([_rgba(os.path.join(scene_dir, "rgb", f)) for f in names])
        poses = np.stack([np.loadtxt(os.path.join(scene_dir, "pose", os.path.splitext(f)[0] + ".txt"), dtype=np.float32)
                          for f in names])
        intrinsics = np.loadtxt(os.path.join(scene_dir, "intrinsics.txt"), dtype=np.float32)[:3, :3]
        box = np.loadtxt(os.path.join(scene_dir, "bbox.txt"), dtype=np.float32)
        self.aabb = torch.tensor(box[:6] * 1.2, dtype=torch.float32, device=device)
        self.scene_bbox = self.aabb.view(2, 3)
        self.render_step_size = 4e-3 if float(box[-1]) >= 0.15 else 1e-3
        self.HEIGHT, self.WIDTH = images.shape[1:3]
        self.focal = float(intrinsics[0, 0])
        self.images = torch.from_numpy(images).to(device)
        self.camtoworlds = torch.from_numpy(poses).to(device)
        self.K = torch.from_numpy(intrinsics).to(device)


_LENS_KEYS = ("k1", "k2", "k3", "k4", "p1", "p2")
_IMAGE_SUFFIXES = ("", ".png", ".jpg", ".jpeg", ".PNG", ".JPG", ".JPEG")


class TransformsLoader(_PosedImages):
    """A capture of one's own in the instant-ngp / nerfstudio layout: `<root>/<scene>/transforms_{train,test}.json` when
    present, else `transforms.json` with every 8th frame held out for `test`.

    Keys: `fl_x fl_y cx cy w h k1 k2 k3 k4 p1 p2` at the top level, each overridable per frame; `camera_model` in
    {PINHOLE, OPENCV, OPENCV_FISHEYE} (absent: OPENCV if any coefficient is non-zero, else PINHOLE); `camera_angle_x` when
    there is no `fl_x`; `frames[].file_path` (looked up with and without an extension) and `frames[].transform_matrix`
    (camera-to-world, OpenGL convention); an optional top-level `aabb` (six numbers) exposed as `.aabb` / `.scene_bbox`.
    OPENCV reads k1 k2 p1 p2 k3 (rational-radial + tangential), OPENCV_FISHEYE k1..k4.  All images must have one size; an
    image without alpha is opaque.  Measured depth, read only under `with_depth`: `frames[].depth_file_path` (a 16-bit PNG or
    a `.npy` float array of the images' size), the top-level `depth_unit_scale_factor` (nerfstudio; default 0.001) or
    `integer_depth_scale` (instant-ngp) that takes an integer file to scene units, and `is_euclidean_depth` (default false:
    z-depth along the optical axis, converted to the distance along each ray by cnc_depth_fetch).

    The cameras go into one table on the device (backends/camera_backend.py); a training batch is the base class's three
    `randint` draws, the background, and ONE launch of cnc_camera_rays with the pixel fetch; a view is one launch in its
    full-frame form.  On a host device the torch restatement runs instead."""

    SPLITS = ["train", "test"]
    NEAR, FAR = 0.0, 1e10
    OPENGL_CAMERA = True
    TRAIN_SPLITS = ("train",)
    HOLD_OUT = 8
    # set (on the instance) by pose refinement: a training batch also holds "camera_ids" i64 [num_rays], the row of
    # `cameras` every ray was drawn from (cnc_amd.poses).  Off: the batch dict is what it always was
    with_camera_ids = False
    # set (on the instance) by error-map sampling: an `ErrorMapSampler` (cnc_amd.error_map) whose `draw`, with this loader's
    # generator, takes the place of the three `randint` draws of a training batch; the batch then also holds "camera_ids",
    # "pixel_xy" = (px, py) and "ray_weight" f32 [num_rays].  None: the draws and the batch dict are what they always were
    sampler = None
    # set (on the instance) by depth supervision, before the first draw: a training batch also holds "depth" f32 [num_rays],
    # the measured distance ALONG each ray in scene units, 0 = no measurement (`depth_planes`: the frames'
    # `depth_file_path`, read at the first use).  Off: nothing is read and the batch dict is what it always was
    with_depth = False

    def __init__(self, subject_id: str, root_fp: str, split: str, color_bkgd_aug: str = "white",
                 num_rays: int = None, near: float = None, far: float = None,
                 batch_over_images: bool = True, device: torch.device = torch.device("cpu"),
                 eps: float = 1e-6, iters: int = 10):
        super().__init__()
        if split not in self.SPLITS:
            raise AssertionError(split)
        self._configure(split, color_bkgd_aug, num_rays, near, far, batch_over_images)
        from .backends import camera_backend
        self.eps, self.iters = float(eps), int(iters)
        scene_dir = os.path.join(root_fp, subject_id)
        per_split = os.path.join(scene_dir, f"transforms_{split}.json")
        path = per_split if os.path.exists(per_split) else os.path.join(scene_dir, "transforms.json")
        with open(path) as fp:
            meta = json.load(fp)
        frames = list(meta["frames"])
        # where this split's cameras come from: the file, and each camera's index in its `frames` (cnc_amd.poses writes
        # refined poses back there)
        self.transforms_path, self.frame_ids = path, list(range(len(frames)))
        if path != per_split:
            self.frame_ids = [i for i in self.frame_ids if (i % self.HOLD_OUT == 0) == (split == "test")]
            frames = [frames[i] for i in self.frame_ids]
        if not frames:
            raise ValueError(f"{path}: no frames for split '{split}'")
        images, rows, lens, models = [], [], [], set()
        for fr in frames:
            file = self._find_image(scene_dir, fr["file_path"])
            img = _rgba(file)
            if images and img.shape != images[0].shape:
                raise ValueError(f"{file}: image is {img.shape[1]} x {img.shape[0]}, the images before it are "
                                 f"{images[0].shape[1]} x {images[0].shape[0]} (one size per capture)")
            images.append(img)
            get = lambda k, default=None: fr.get(k, meta.get(k, default))
            h, w = img.shape[:2]
            fw = float(get("w", w))
            if get("fl_x") is not None:
                fx = float(get("fl_x"))
            elif get("camera_angle_x") is not None:
                fx = 0.5 * fw / math.tan(0.5 * float(get("camera_angle_x")))
            else:
                raise ValueError(f"{path}: neither fl_x nor camera_angle_x")
            fy = float(get("fl_y", fx))
            rows.append([fx, fy, float(get("cx", fw / 2.0)), float(get("cy", float(get("h", h)) / 2.0))])
            k = {name: float(get(name, 0.0)) for name in _LENS_KEYS}
            model = get("camera_model")
            if model is None:
                model = "OPENCV" if any(v != 0.0 for v in k.values()) else "PINHOLE"
            if model not in camera_backend.MODELS:
                raise ValueError(f"{path}: camera_model {model!r} is not one of {sorted(camera_backend.MODELS)}")
            if model == "OPENCV" and k["k4"] != 0.0:
                raise ValueError(f"{path}: the OPENCV model has no k4 (OPENCV_FISHEYE does)")
            if model == "OPENCV_FISHEYE" and (k["p1"] != 0.0 or k["p2"] != 0.0):
                raise ValueError(f"{path}: the OPENCV_FISHEYE model has no tangential coefficients")
            models.add(model)
            lens.append([k["k1"], k["k2"], k["k3"], k["k4"]] if model == "OPENCV_FISHEYE"
                        else [k["k1"], k["k2"], k["p1"], k["p2"], k["k3"]] if model == "OPENCV" else [])
        if len(models) != 1:
            raise ValueError(f"{path}: one camera_model per capture, not {sorted(models)}")
        self.camera_model = models.pop()
        self.model = camera_backend.MODELS[self.camera_model]
        self.HEIGHT, self.WIDTH = images[0].shape[:2]
        # measured depth (read by `depth_planes`, and only when asked for): a file per frame or None, the factor that takes an
        # integer file's counts to scene units, and whether the values are distances along the ray or along the optical axis
        self._scene_dir, self._depth_planes = scene_dir, None
        self.depth_files = [fr.get("depth_file_path") for fr in frames]
        if meta.get("depth_unit_scale_factor") is not None:
            self.depth_scale = float(meta["depth_unit_scale_factor"])
        else:
            self.depth_scale = float(meta.get("integer_depth_scale", 0.001))
        self.is_euclidean_depth = bool(meta.get("is_euclidean_depth", False))
        self.images = torch.from_numpy(np.stack(images)).to(device)
        poses = np.asarray([fr["transform_matrix"] for fr in frames], dtype=np.float32)
        self.camtoworlds = torch.from_numpy(poses).to(device)
        self.intrinsics = torch.tensor(rows, dtype=torch.float32, device=device)
        self.lens = torch.tensor(lens, dtype=torch.float32, device=device).reshape(len(frames), len(lens[0]))
        self.cameras = camera_backend.camera_table(self.intrinsics, self.camtoworlds, self.lens)
        fx, fy, cx, cy = rows[0]
        self.focal = fx
        self.K = torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float32, device=device)
        if meta.get("aabb") is not None:
            box = np.asarray(meta["aabb"], dtype=np.float32).reshape(-1)
            if box.shape[0] != 6:
                raise ValueError(f"{path}: aabb must hold six numbers")
            self.aabb = torch.tensor(box, dtype=torch.float32, device=device)
            self.scene_bbox = self.aabb.view(2, 3)
        else:
            self.aabb = None

    @staticmethod
    def _find_image(scene_dir, file_path):
        for suffix in _IMAGE_SUFFIXES:
            file = os.path.join(scene_dir, file_path + suffix)
            if os.path.isfile(file):
                return file
        raise FileNotFoundError(f"{os.path.join(scene_dir, file_path)}: no such image (with or without an extension)")

    def depth_planes(self):
        """float32 [n_cams, H, W] on the images' device: every frame's `depth_file_path` in scene units, read once — a
        16-bit PNG (or any integer image / array: times `depth_scale`) or a `.npy` float array (as it is); an all-zero plane,
        no measurement, for a frame without one.  ValueError: a file of another size than the images, or no file at all."""
        if self._depth_planes is not None:
            return self._depth_planes
        if not any(self.depth_files):
            raise ValueError(f"{self.transforms_path}: depth was asked for, but no frame of split '{self.split}' has a "
                             "depth_file_path")
        planes = np.zeros((len(self.depth_files), self.HEIGHT, self.WIDTH), np.float32)
        for k, name in enumerate(self.depth_files):
            if not name:
                continue
            file = os.path.join(self._scene_dir, name)
            if file.endswith(".npy"):
                raw = np.load(file)
            else:
                from PIL import Image
                with Image.open(file) as img:
                    raw = np.asarray(img)
            if raw.shape != (self.HEIGHT, self.WIDTH):
                raise ValueError(f"{file}: depth is {' x '.join(str(s) for s in raw.shape[::-1])}, the images are "
                                 f"{self.WIDTH} x {self.HEIGHT}")
            integer = np.issubdtype(raw.dtype, np.integer)
            planes[k] = raw.astype(np.float32) * np.float32(self.depth_scale) if integer else raw.astype(np.float32)
        self._depth_planes = torch.from_numpy(planes).to(self.images.device)
        return self._depth_planes

    def _fetch_depth(self, ids, x, y, dirs):
        from .backends import camera_backend
        planes = self.depth_planes()
        fetch = camera_backend.depth_fetch if planes.is_cuda else camera_backend.depth_fetch_torch
        return fetch(planes, self.cameras, self.OPENGL_CAMERA, self.is_euclidean_depth, ids.expand(x.shape[0]).contiguous(),
                     x, y, dirs)

    @torch.no_grad()
    def __getitem__(self, index):
        from .backends import camera_backend
        dev = self.images.device
        weight = None
        if self.sampler is not None and self.training:
            ids, x, y, weight = self.sampler.draw(self.num_rays, getattr(self, "_gen", None))
            shape = (self.num_rays,)
        elif self.training or not dev.type == "cuda":
            ids, x, y, shape = self._pixels_to_sample(index, dev)
        else:
            ids, shape = None, (self.HEIGHT, self.WIDTH)
        bkgd = self._background(dev)
        if dev.type != "cuda":
            o, d, pix = camera_backend.camera_rays_torch(self.cameras, self.model, self.OPENGL_CAMERA, ids.expand(x.shape[0]),
                                                         x, y, self.images, bkgd, self.eps, self.iters)
        elif ids is not None:
            o, d, pix = camera_backend.camera_rays(self.cameras, self.model, self.OPENGL_CAMERA, ids, x, y, images=self.images,
                                                   bkgd=bkgd, eps=self.eps, iters=self.iters)
        else:
            o, d, pix = camera_backend.camera_rays(self.cameras, self.model, self.OPENGL_CAMERA, cam0=int(index),
                                                   width=self.WIDTH, height=self.HEIGHT, images=self.images, bkgd=bkgd,
                                                   eps=self.eps, iters=self.iters)
        out = {"pixels": pix.reshape(*shape, 3),
               "rays": Rays(origins=o.reshape(*shape, 3), viewdirs=d.reshape(*shape, 3)),
               "color_bkgd": bkgd}
        if self.with_camera_ids and self.training:
            out["camera_ids"] = ids
        if weight is not None:
            out["camera_ids"], out["pixel_xy"], out["ray_weight"] = ids, (x, y), weight
        if self.with_depth and self.training:
            out["depth"] = self._fetch_depth(ids, x, y, d)          # one launch behind the rays', on the same stream
        return out


class SyntheticBallDataset:
    """Procedural scene: an opaque textured ball of radius 0.8 in front of a white background,
    seen from cameras on a sphere of radius 4 (focal as nerf_synthetic, camera_angle_x=0.6911).
    `fetch(num_rays)` returns random training pixels like SubjectLoader.fetch_data in training mode
    (nerf_synthetic.py:164-239); `view(i)` returns a whole test image."""

    RADIUS = 0.8
    has_alpha = True         # pixels a ray misses the ball with are transparent, blended with the batch's colour (`fetch`)
    # set (on the instance) by depth supervision: `fetch()` also returns "depth" f32 [n], the analytic distance along each ray
    # to the ball, 0 where it misses.  Off: the batch dict and the draws are what they always were (no draw is added either way)
    with_depth = False

    def __init__(self, image_size=200, n_train_views=100, device="cuda", seed=0):
        self.H = self.W = image_size
        self.focal = 0.5 * image_size / math.tan(0.5 * 0.6911)
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device).manual_seed(seed)
        g = torch.Generator().manual_seed(1234)
        self.train_c2w = self._poses(n_train_views, g).to(self.device)
        self.test_c2w = self._poses(16, torch.Generator().manual_seed(4321)).to(self.device)
        self.num_rays = 1024

    @staticmethod
    def _poses(n, g):
        az = torch.rand(n, generator=g) * 2 * math.pi
        el = (torch.rand(n, generator=g) - 0.3) * 1.2
        eye = 4.0 * torch.stack([torch.cos(el) * torch.cos(az), torch.cos(el) * torch.sin(az), torch.sin(el)], -1)
        fwd = -eye / eye.norm(dim=-1, keepdim=True)
        up0 = torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)
        right = torch.linalg.cross(fwd, up0)
        right = right / right.norm(dim=-1, keepdim=True)
        up = torch.linalg.cross(right, fwd)
        return torch.cat([torch.stack([right, up, -fwd], dim=-1), eye[..., None]], dim=-1)   # [n,3,4]

    def update_num_rays(self, n):
        self.num_rays = int(n)

    def _rays(self, c2w, x, y):
        cam = torch.stack([(x - self.W / 2 + 0.5) / self.focal, -(y - self.H / 2 + 0.5) / self.focal,
                           -torch.ones_like(x)], dim=-1)
        d = (cam[:, None, :] * c2w[:, :3, :3]).sum(-1)
        d = d / torch.linalg.norm(d, dim=-1, keepdim=True)
        o = c2w[:, :3, 3].expand_as(d)
        return o.contiguous(), d.contiguous()

    def _shade(self, o, d):
        """Ground-truth pixel colour and alpha: first hit of the ball."""
        b = (o * d).sum(-1)
        c = (o * o).sum(-1) - self.RADIUS ** 2
        disc = b * b - c
        hit = disc > 0
        t = -b - torch.sqrt(disc.clamp_min(0))
        p = o + d * t[:, None]
        n = p / self.RADIUS
        if getattr(self, "_shade_consts", None) is None or self._shade_consts[0].device != p.device:
            self._shade_consts = (torch.tensor([0.0, 2.0, 4.0], device=p.device),
                                  torch.tensor([0.3, 0.5, 0.8], device=p.device))
        phase, light = self._shade_consts
        tex = 0.5 + 0.5 * torch.sin(p * 9.0 + phase)
        lam = (0.35 + 0.65 * (n * light).sum(-1).clamp(0, 1))[:, None]
        rgb = (tex * lam).clamp(0, 1)
        return rgb, hit.float()[:, None]

    def _train_images(self):
        """The training views as RGBA images in device memory, as SubjectLoader holds its images
        (nerf_synthetic.py:133-146): the analytic shading evaluated once per pixel instead of once per fetched ray."""
        if getattr(self, "_images", None) is None:
            ys, xs = torch.meshgrid(torch.arange(self.H, device=self.device),
                                    torch.arange(self.W, device=self.device), indexing="ij")
            x, y = xs.reshape(-1).float(), ys.reshape(-1).float()
            views = []
            for c2w in self.train_c2w:
                o, d = self._rays(c2w[None].expand(x.shape[0], 3, 4), x, y)
                views.append(torch.cat(self._shade(o, d), dim=-1).view(self.H, self.W, 4))
            self._images = torch.stack(views)
        return self._images

    def _train_depth(self):
        """The training views' exact depth [n, H, W], computed once: the distance along each pixel's ray to the first hit
        of the ball (Euclidean depth), 0 — no measurement — where the ray misses it."""
        if getattr(self, "_depth", None) is None:
            ys, xs = torch.meshgrid(torch.arange(self.H, device=self.device),
                                    torch.arange(self.W, device=self.device), indexing="ij")
            x, y = xs.reshape(-1).float(), ys.reshape(-1).float()
            views = []
            for c2w in self.train_c2w:
                o, d = self._rays(c2w[None].expand(x.shape[0], 3, 4), x, y)
                b = (o * d).sum(-1)
                disc = b * b - ((o * o).sum(-1) - self.RADIUS ** 2)
                t = -b - torch.sqrt(disc.clamp_min(0))
                views.append(torch.where(disc > 0, t, torch.zeros_like(t)).view(self.H, self.W))
            self._depth = torch.stack(views)
        return self._depth

    def fetch(self, num_rays=None):
        n = self.num_rays if num_rays is None else num_rays
        img = torch.randint(0, self.train_c2w.shape[0], (n,), device=self.device, generator=self.gen)
        xi = torch.randint(0, self.W, (n,), device=self.device, generator=self.gen)
        yi = torch.randint(0, self.H, (n,), device=self.device, generator=self.gen)
        o, d = self._rays(self.train_c2w[img], xi.float(), yi.float())
        rgba = self._train_images()[img, yi, xi]            # the same numbers as shading the fetched rays
        rgb, alpha = rgba[:, :3], rgba[:, 3:]
        bkgd = torch.rand(3, device=self.device, generator=self.gen)     # random bkgd in training
        out = {"rays": Rays(o, d), "pixels": rgb * alpha + bkgd * (1 - alpha), "color_bkgd": bkgd}
        if self.with_depth:
            out["depth"] = self._train_depth()[img, yi, xi]
        return out

    def view(self, i):
        ys, xs = torch.meshgrid(torch.arange(self.H, device=self.device),
                                torch.arange(self.W, device=self.device), indexing="ij")
        x, y = xs.reshape(-1).float(), ys.reshape(-1).float()
        c2w = self.test_c2w[i % self.test_c2w.shape[0]][None].expand(x.shape[0], 3, 4)
        o, d = self._rays(c2w, x, y)
        rgb, alpha = self._shade(o, d)
        bkgd = torch.ones(3, device=self.device)
        return {"rays": Rays(o.view(self.H, self.W, 3), d.view(self.H, self.W, 3)),
                "pixels": (rgb * alpha + bkgd * (1 - alpha)).view(self.H, self.W, 3), "color_bkgd": bkgd}


class LoaderDataset:
    """`SubjectLoader` / `SubjectLoader_Tanks` behind the three calls the Trainer makes:
    `fetch()` = one training batch as the reference draws it (`train_dataset[randint(len)]`,
    train_CNC_nerf_synthetic.py:305-306), `view(i)` = test image i, `update_num_rays`."""

    def __init__(self, train_loader, test_loader):
        self.train, self.test = train_loader, test_loader
        self._gen = None

    def seed_sampling(self, seed: int):
        """Per-rank stream for the image index drawn here and for the loader's pixel draws (data parallelism:
        without it every rank would render the same batch and the all-reduce would average N copies of one
        gradient)."""
        self._gen = torch.Generator().manual_seed(int(seed))
        self.train.seed_sampling(int(seed) + 1)

    def update_num_rays(self, n):
        self.train.update_num_rays(int(n))

    def fetch(self):
        return self.train[int(torch.randint(0, len(self.train), (1,), generator=self._gen).item())]

    def view(self, i):
        return self.test[i % len(self.test)]

    def __len__(self):
        return len(self.test)
