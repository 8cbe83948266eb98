"""CPU: measured depth in the loaders — `TransformsLoader` over a 3-frame capture written into tmp_path (a 16-bit PNG, a
`.npy` array, a frame without depth): the scale keys, `is_euclidean_depth`, the z -> t conversion of the torch path against
the float64 twin, the errors, and that nothing moves without `with_depth`; `SyntheticBallDataset`'s analytic depth."""
import numpy as np
import pytest
import torch

import depth_capture as C
import depth_twin as T

CPU = torch.device("cpu")


def _draws(n, seed=5):
    """The three draws of a training batch from the loader's generator, in its order."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 3, (n,), generator=g)
    return ids, torch.randint(0, C.W, (n,), generator=g), torch.randint(0, C.H, (n,), generator=g)


@pytest.mark.parametrize("key,scale", [("depth_unit_scale_factor", 0.002), ("integer_depth_scale", 0.0005), (None, None)])
def test_planes_and_scale_keys(tmp_path, key, scale):
    planes, _ = C.write(tmp_path, scale_key=key, scale=scale)
    ld = C.loader(tmp_path, CPU)
    assert ld._depth_planes is None                      # nothing is read before it is asked for
    got = ld.depth_planes()
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, C.H, C.W)
    assert np.array_equal(got.numpy(), planes, equal_nan=True)
    assert ld.depth_scale == (0.001 if key is None else scale) and ld.is_euclidean_depth is False
    assert not got[2].any()                              # the frame without a depth file: no measurement anywhere
    assert got[0, 0, 0] == 0 and torch.isnan(got[1, 2, 3])


@pytest.mark.parametrize("euclidean", [None, False, True])
def test_batch_depth_against_the_twin(tmp_path, euclidean):
    planes, _ = C.write(tmp_path, euclidean=euclidean)
    ld = C.loader(tmp_path, CPU, num_rays=256)
    ld.with_depth = True
    batch = ld[0]
    assert set(batch) == {"pixels", "rays", "color_bkgd", "depth"}
    depth = batch["depth"]
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (256,)
    ids, px, py = _draws(256)
    dirs = batch["rays"].viewdirs.numpy()
    want, c, z = T.fetch64(planes, ld.cameras.numpy(), True, bool(euclidean), ids.numpy(), px.numpy(), py.numpy(), dirs)
    tol = T.fetch_bound(ld.cameras.numpy(), bool(euclidean), ids.numpy(), dirs, want, c)
    assert np.all(c > 1e-3)                              # pinhole rays: well inside the half space in front of the camera
    got = depth.numpy().astype(np.float64)
    assert np.all(np.abs(got - want) <= tol), T.ratio(got, want, tol)
    none = ~(np.isfinite(z) & (z > 0))
    assert none.any() and (ids.numpy() == 2).any() and not got[none].any() and (got[~none] > 0).all()
    if euclidean:
        assert np.array_equal(got[~none], z[~none])
    else:
        assert np.all(got[~none] >= z[~none])            # the distance along the ray is never shorter than the z-depth


def test_without_with_depth_nothing_changes(tmp_path):
    C.write(tmp_path)
    plain, deep = C.loader(tmp_path, CPU), C.loader(tmp_path, CPU)
    deep.with_depth = True
    for _ in range(3):
        a, b = plain[0], deep[0]
        assert set(a) == {"pixels", "rays", "color_bkgd"} and set(b) == set(a) | {"depth"}
        assert torch.equal(a["pixels"], b["pixels"]) and torch.equal(a["color_bkgd"], b["color_bkgd"])
        assert torch.equal(a["rays"].origins, b["rays"].origins) and torch.equal(a["rays"].viewdirs, b["rays"].viewdirs)
    assert plain._depth_planes is None
    # the draws are the base class's three, from the loader's own generator: the pixels are the images' at those indices
    ids, px, py = _draws(64)
    rgba = plain.images[ids, py, px].float() / 255.0
    first = C.loader(tmp_path, CPU)[0]
    assert torch.allclose(first["pixels"], rgba[:, :3] * rgba[:, 3:] + (1.0 - rgba[:, 3:]), atol=1e-6)
    # evaluation views never carry depth
    view = C.loader(tmp_path, CPU, num_rays=None)
    view.with_depth = True
    assert "depth" not in view[0]


def test_errors(tmp_path):
    C.write(tmp_path / "a", depth_shape=(C.H + 1, C.W))
    ld = C.loader(tmp_path / "a", CPU)
    with pytest.raises(ValueError, match="d0.png"):
        ld.depth_planes()
    C.write(tmp_path / "b", with_depth=False)
    ld = C.loader(tmp_path / "b", CPU)
    ld.with_depth = True
    with pytest.raises(ValueError, match="depth_file_path"):
        ld[0]


def test_trainer_refuses_a_dataset_without_depth(tmp_path):
    """Construction on the CPU device: a capture without depth files, and a dataset of another kind."""
    from cnc_amd.datasets import LoaderDataset
    from cnc_amd.trainer import TrainConfig, Trainer
    C.write(tmp_path, with_depth=False)
    small = dict(lmbda=2e-3, Pg_level=5, Pg_level_2D=3, log2_hashmap_size=12, log2_hashmap_size_2D=9, sample_num=3000,
                 n_features=2, n_neurons=32, resolutions_list=(10, 14, 18, 26, 34), resolutions_list_2D=(18, 34, 66),
                 grid_resolution=16, image_size=16, out_dir=str(tmp_path / "bits"))
    data = LoaderDataset(C.loader(tmp_path, CPU), C.loader(tmp_path, CPU, num_rays=None))
    with pytest.raises(ValueError, match="depth_file_path"):
        Trainer(TrainConfig(depth_weight=1.0, **small), device="cpu", dataset=data)

    class Other:
        def update_num_rays(self, n):
            pass

    with pytest.raises(ValueError, match="measured depth"):
        Trainer(TrainConfig(depth_weight=1.0, **small), device="cpu", dataset=Other())
    tr = Trainer(TrainConfig(depth_weight=0.0, depth_spread=-3.0, **small), device="cpu", dataset=data)      # off: inert
    assert tr._depth_weight == 0.0 and data.train.with_depth is False


def test_synthetic_ball_depth_is_the_analytic_distance():
    from cnc_amd.datasets import SyntheticBallDataset
    plain = SyntheticBallDataset(image_size=24, n_train_views=5, device="cpu", seed=9)
    deep = SyntheticBallDataset(image_size=24, n_train_views=5, device="cpu", seed=9)
    deep.with_depth = True
    hits = 0
    for _ in range(3):
        a, b = plain.fetch(500), deep.fetch(500)
        assert set(a) == {"rays", "pixels", "color_bkgd"} and set(b) == set(a) | {"depth"}
        assert torch.equal(a["pixels"], b["pixels"]) and torch.equal(a["color_bkgd"], b["color_bkgd"])
        assert torch.equal(a["rays"].origins, b["rays"].origins) and torch.equal(a["rays"].viewdirs, b["rays"].viewdirs)
        o, d = b["rays"].origins.double(), b["rays"].viewdirs.double()
        bb = (o * d).sum(-1)
        disc = bb * bb - ((o * o).sum(-1) - SyntheticBallDataset.RADIUS ** 2)
        want = torch.where(disc > 0, -bb - disc.clamp_min(0).sqrt(), torch.zeros_like(bb))
        # (a grazing ray may fall on either side in float32, and sqrt(disc) magnifies disc's 2e-6 of rounding by 1 / (2 sqrt(disc)))
        sure = disc.abs() > 1e-2
        assert torch.allclose(b["depth"].double()[sure], want[sure], atol=1e-4)
        assert b["depth"].dtype == torch.float32 and tuple(b["depth"].shape) == (500,)
        hits += int((b["depth"] > 0).sum())
        assert bool((b["depth"][sure & (disc <= 0)] == 0).all())
    assert hits > 20
