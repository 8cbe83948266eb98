"""CPU: error-map pixel sampling — the NumPy twin of the kernels (tests/errmap_twin.py) against the
sampling law as an exact identity, the sampler against its own CDF without statistics, the edge cases, the package's torch
restatement for host tensors against the twin's bits, and the loader with the option off against its own draws."""
import numpy as np
import pytest
import torch

import errmap_twin as T
from cnc_amd import error_map as EM
from cnc_amd.backends import errmap_backend as K

SHAPES = [(1, 7, 13, 1), (3, 7, 13, 4), (2, 33, 65, 16), (5, 16, 16, 64)]          # (n_cams, H, W, G)


def _bits(a):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _same_bits(a, b):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _map(shape, seed):
    n_cams, _, _, G = shape
    return np.random.default_rng(seed).uniform(1e-4, 1.0, (n_cams, G, G)).astype(np.float32) ** 3


def test_unbiasedness_is_an_exact_identity():
    """3 cameras of 13 x 7 pixels, G = 4, a random map, every pixel enumerated, float64."""
    assert (EM.RESOLUTION, EM.UNIFORM_FLOOR, EM.DECAY, EM.REFRESH_EVERY) == (16, 0.5, 0.9, 16)
    n_cams, H, W, G, u = 3, 7, 13, 4, EM.UNIFORM_FLOOR
    rng = np.random.default_rng(0)
    m = rng.uniform(0.0, 1.0, (n_cams, G, G)) ** 4
    prob, cdf = T.cdf(m, n_cams, H, W, G, u, np.float64)
    a = T.areas(n_cams, H, W, G)
    assert a.sum() == n_cams * H * W and len(set(a.tolist())) > 1                   # cells of different pixel counts
    cells = T.pixel_cells(n_cams, H, W, G)
    p_pix = prob[cells] / a[cells]
    w = (1.0 / (n_cams * H * W)) / p_pix
    assert abs(p_pix.sum() - 1.0) <= 1e-12 and abs(prob.sum() - 1.0) <= 1e-12
    assert w.max() <= 1.0 / u + 1e-12
    for _ in range(4):
        f = rng.normal(size=cells.shape) * 10.0 ** rng.uniform(-3, 3)
        assert abs((p_pix * w * f).sum() - f.mean()) <= 1e-12 * max(1.0, np.abs(f).max())
    assert cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sampler_follows_its_cdf_without_statistics(shape, dtype):
    """Stratified randoms (k + 0.5) / n: every cell's count within 1 of n p(cell); every pixel inside its cell."""
    n_cams, H, W, G = shape
    m = _map(shape, 1)
    prob, cdf = T.cdf(m, n_cams, H, W, G, 0.5, dtype)
    assert prob.dtype == dtype and cdf.dtype == dtype
    n = 4096
    rng = np.random.default_rng(2)
    rand = np.stack([(np.arange(n) + 0.5) / n, rng.uniform(size=n), rng.uniform(size=n)], axis=1).astype(dtype)
    rand[:5, 1:] = [[0.0, 0.0], [np.nextafter(dtype(1), dtype(0))] * 2, [0.0, np.nextafter(dtype(1), dtype(0))], [0.5, 0.0],
                    [np.nextafter(dtype(1), dtype(0)), 0.5]]
    ids, px, py, w = T.sample(rand, cdf, prob, n_cams, H, W, G, dtype)
    cell = T.keys(ids, px, py, n_cams, H, W, G).astype(np.int64)
    assert np.all((ids >= 0) & (ids < n_cams) & (px >= 0) & (px < W) & (py >= 0) & (py < H))
    expect = np.minimum(np.searchsorted(cdf, rand[:, 0], side="right"), cdf.shape[0] - 1)
    assert np.array_equal(cell, expect)                                   # the pixel lies in the cell the CDF selected
    counts = np.bincount(cell, minlength=prob.shape[0])
    step = np.diff(np.concatenate([[0.0], cdf.astype(np.float64)]))
    assert np.all(np.abs(counts - n * step) <= 1.0 + 1e-9)                 # against the CDF's own steps: exact
    slack = 1e-9 if dtype == np.float64 else n * prob.shape[0] * 2.0 ** -24
    assert np.all(np.abs(counts - n * prob.astype(np.float64)) <= 1.0 + slack)
    a = T.areas(n_cams, H, W, G)
    assert np.all(counts[a == 0] == 0)
    # the weight is (1 / N_pix) / p(pixel), at most 1 / u
    want = (1.0 / (n_cams * H * W)) / (prob.astype(np.float64)[cell] / a[cell])
    assert np.allclose(w, want, rtol=1e-6 if dtype == np.float32 else 1e-14)
    assert w.max() <= 2.0 * (1 + 1e-6)


def test_edge_cases():
    f32 = np.float32
    # G = 1: one cell per camera, p = the camera's share whatever the map holds per camera ... times its mass
    prob, cdf = T.cdf(np.asarray([[[2.0]], [[6.0]]], f32), 2, 5, 3, 1, 0.5)
    assert np.allclose(prob, [0.5 * 0.25 + 0.25, 0.5 * 0.75 + 0.25]) and cdf[-1] == 1.0
    # G larger than H: empty cells have probability exactly 0, repeat their predecessor in the CDF and are never drawn
    n_cams, H, W, G = 2, 7, 13, 16
    a = T.areas(n_cams, H, W, G)
    assert (a == 0).sum() > 0 and a.sum() == n_cams * H * W and a[-1] == 1 and a[0] == 0
    m = _map((n_cams, H, W, G), 3)
    for dtype in (np.float32, np.float64):
        prob, cdf = T.cdf(m, n_cams, H, W, G, 0.5, dtype)
        assert np.all(prob[a == 0] == 0) and np.all(prob[a > 0] > 0)
        prev = np.concatenate([[dtype(0)], cdf[:-1]])
        assert np.all(cdf[a == 0] == prev[a == 0]) and cdf[-1] == 1 and np.all(np.diff(cdf) >= 0)
        n = 5000
        rand = np.random.default_rng(4).uniform(size=(n, 3)).astype(dtype)
        rand[0], rand[1] = 0.0, np.nextafter(dtype(1), dtype(0))
        ids, px, py, w = T.sample(rand, cdf, prob, n_cams, H, W, G, dtype)
        cell = T.keys(ids, px, py, n_cams, H, W, G)
        assert np.all(a[cell] > 0) and np.all(np.isfinite(w)) and np.all(w > 0)
        assert np.all((px >= 0) & (px < W) & (py >= 0) & (py < H))
    # a map whose last cells are empty: H = 3, G = 4 has edges 0 0 1 2 3, fine; W = 2, G = 3 has edges 0 0 1 2.  An image
    # whose LAST cell is empty does not exist (the last edge is the size), but everything from the last cell with pixels on is 1
    prob, cdf = T.cdf(np.ones((1, 3, 3), f32), 1, 2, 2, 3, 0.5)
    assert cdf[-1] == 1.0 and prob[-1] > 0
    # a zero map, a NaN map, an infinite map: uniform
    for bad in (0.0, np.nan, np.inf, -1.0):
        for dtype in (np.float32, np.float64):
            prob, cdf = T.cdf(np.full((3, 4, 4), bad), 3, 7, 13, 4, 0.5, dtype)
            assert np.array_equal(prob, (T.areas(3, 7, 13, 4).astype(dtype) / dtype(3 * 7 * 13)))
            assert cdf[-1] == 1 and np.all(np.diff(cdf) >= 0)
    # one NaN entry among good ones counts as 0
    m = np.ones((1, 2, 2), f32)
    m[0, 0, 0] = np.nan
    prob, _ = T.cdf(m, 1, 4, 4, 2, 0.5, np.float64)
    assert np.allclose(prob, [0.125, 0.5 / 3 + 0.125, 0.5 / 3 + 0.125, 0.5 / 3 + 0.125])
    # one hot cell: it gets 1 - u on top of its uniform share, every weight stays <= 1 / u
    m = np.zeros((3, 4, 4), f32)
    m[1, 2, 3] = 0.25
    prob, cdf = T.cdf(m, 3, 7, 13, 4, 0.5, np.float64)
    a = T.areas(3, 7, 13, 4)
    hot = (1 * 4 + 2) * 4 + 3
    uniform = 0.5 * a / a.sum()
    assert abs(prob[hot] - (0.5 + uniform[hot])) <= 1e-15 and np.allclose(np.delete(prob, hot), np.delete(uniform, hot))


def test_update_and_loss_float32_against_float64():
    rng = np.random.default_rng(5)
    shape = (3, 7, 13, 4)
    n = 4097
    ids, px, py = rng.integers(0, 3, n), rng.integers(0, 13, n), rng.integers(0, 7, n)
    keys = T.keys(ids, px, py, *shape)
    err = (rng.uniform(size=n) ** 2).astype(np.float32)
    err[7] = np.nan
    err[11] = np.inf
    m = _map(shape, 6)
    m32, m64 = T.update(m, keys, err, 0.9), T.update(m, keys, err, 0.9, np.float64)
    assert m32.dtype == np.float32 and np.all(np.isfinite(m32))
    assert np.all(np.abs(m32 - m64) <= (n + 8) * 2.0 ** -24 * np.maximum(m64, 1e-30) + 1e-12)
    few = T.update(m, keys[:5], err[:5], 0.9)                       # five rays: every other cell keeps its bits
    untouched = np.ones(m.size, bool)
    untouched[keys[:5]] = False
    assert np.array_equal(_bits(few.reshape(-1)[untouched]), _bits(m.reshape(-1)[untouched]))
    assert not np.array_equal(few, m)
    # the loss: all weights 1 is the mse within the float32 summation bound; the backward is its gradient
    rgb, pix = rng.uniform(size=(n, 3)).astype(np.float32), rng.uniform(size=(n, 3)).astype(np.float32)
    w = rng.uniform(0.1, 2.0, n).astype(np.float32)
    l32, e32 = T.loss_forward(rgb, pix, w)
    l64, e64 = T.loss_forward(rgb, pix, w, np.float64)
    terms = (w.astype(np.float64)[:, None] * (rgb.astype(np.float64) - pix) ** 2).sum() / (3 * n)
    assert abs(float(l32) - l64) <= (3 * n + 8) * 2.0 ** -24 * terms
    assert np.allclose(e32, e64, rtol=1e-6, atol=0)
    one = np.ones(n, np.float32)
    mse = float(torch.nn.functional.mse_loss(torch.from_numpy(rgb), torch.from_numpy(pix)))
    l1 = float(T.loss_forward(rgb, pix, one)[0])
    assert abs(l1 - mse) <= (3 * n + 8) * 2.0 ** -23 * mse
    x = torch.from_numpy(rgb.astype(np.float64)).requires_grad_(True)
    ((torch.from_numpy(w.astype(np.float64))[:, None] * (x - torch.from_numpy(pix.astype(np.float64))) ** 2).sum()
     / (3 * n) * 1024.0).backward()
    assert np.allclose(T.loss_backward(1024.0, rgb, pix, w), x.grad.numpy(), rtol=1e-5, atol=1e-12)


@pytest.mark.parametrize("shape", SHAPES + [(2, 7, 13, 16)])
def test_host_restatement_equals_the_twin(shape):
    """Integers exactly, floats bit for bit in float32 mode."""
    n_cams, H, W, G = shape
    rng = np.random.default_rng(7)
    m = _map(shape, 8)
    for mm in (m, np.zeros_like(m), np.full_like(m, np.nan)):
        prob, cdf = T.cdf(mm, n_cams, H, W, G, 0.5)
        prob_t, cdf_t = K.cdf_torch(torch.from_numpy(mm), H, W, 0.5)
        assert _same_bits(prob_t, prob) and _same_bits(cdf_t, cdf)
    prob, cdf = T.cdf(m, n_cams, H, W, G, 0.5)
    n = 1000
    rand = rng.uniform(size=(n, 3)).astype(np.float32)
    rand[0], rand[1], rand[2] = 0.0, np.nextafter(np.float32(1), np.float32(0)), np.nan
    got = K.sample_torch(torch.from_numpy(rand), torch.from_numpy(cdf), torch.from_numpy(prob), n_cams, H, W, G)
    want = T.sample(rand, cdf, prob, n_cams, H, W, G)
    for g, w_ in zip(got, want):
        assert _same_bits(g, w_)
    ids, px, py = want[:3]
    ids[3], px[4], py[5] = -7, 10 ** 9, -1                          # clamped for the access
    keys = T.keys(ids, px, py, n_cams, H, W, G)
    assert _same_bits(K.keys_torch(torch.from_numpy(ids), torch.from_numpy(px), torch.from_numpy(py), n_cams, H, W, G), keys)
    err = (rng.uniform(size=n) ** 2).astype(np.float32)
    err[9] = np.nan
    mt = torch.from_numpy(m.copy())
    K.update_torch(mt, torch.from_numpy(keys), torch.from_numpy(err), 0.9)
    assert _same_bits(mt, T.update(m, keys, err, 0.9))
    for k in (1, 255, 257, 1000):
        rgb, pix = rng.uniform(size=(k, 3)).astype(np.float32), rng.uniform(size=(k, 3)).astype(np.float32)
        w = rng.uniform(0.1, 2.0, k).astype(np.float32)
        loss_t, err_t = K.loss_forward_torch(torch.from_numpy(rgb), torch.from_numpy(pix), torch.from_numpy(w))
        loss, e = T.loss_forward(rgb, pix, w)
        assert _same_bits(loss_t, np.float32(loss)) and _same_bits(err_t, e)
        g = K.loss_backward_torch(torch.tensor(1024.0), torch.from_numpy(rgb), torch.from_numpy(pix), torch.from_numpy(w))
        assert _same_bits(g, T.loss_backward(1024.0, rgb, pix, w))


def test_sampler_object_on_a_host_device():
    s = EM.ErrorMapSampler(3, 7, 13, resolution=4, refresh_every=8, device="cpu")
    assert s.effective_fraction() == pytest.approx(1.0, abs=1e-6)                     # a constant map: the uniform draw
    g = torch.Generator().manual_seed(3)
    ids, px, py, w = s.draw(500, g)
    assert ids.dtype == px.dtype == py.dtype == torch.int64 and w.dtype == torch.float32
    assert torch.allclose(w, torch.ones_like(w), rtol=1e-6)
    before = s.map.clone()
    err = torch.rand(500, generator=g) ** 2
    err[0] = float("nan")
    s.observe(ids, px, py, err)
    assert bool(torch.isfinite(s.map).all()) and not torch.equal(s.map, before)
    cdf = s.cdf.clone()
    state = s.state_dict()                                          # the distribution lags the map: both are state
    s.refresh()
    assert not torch.equal(s.cdf, cdf) and 0.0 < s.effective_fraction() < 1.0
    ids2, _, _, w2 = s.draw(500, torch.Generator().manual_seed(9))
    assert float(w2.max()) <= 2.0 * (1 + 1e-6) and float(w2.min()) > 0
    s2 = EM.ErrorMapSampler(3, 7, 13, resolution=4, device="cpu")
    s2.load_state_dict(state)
    assert torch.equal(s2.cdf, cdf) and torch.equal(s2.map, state["map"]) and s2.refresh_every == 8
    a = s2.draw(64, torch.Generator().manual_seed(1))
    s.load_state_dict(state)
    b = s.draw(64, torch.Generator().manual_seed(1))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        EM.ErrorMapSampler(3, 7, 13, resolution=65, device="cpu")
    with pytest.raises(ValueError):
        EM.ErrorMapSampler(3, 7, 13, uniform_floor=0.0, device="cpu")
    with pytest.raises(ValueError):
        s2.load_state_dict(EM.ErrorMapSampler(2, 7, 13, resolution=4, device="cpu").state_dict())
    # the weighted loss of host tensors is differentiable and equals the mse at weight 1
    rgb = torch.rand(300, 3, requires_grad=True)
    pix = torch.rand(300, 3)
    loss, e = EM.weighted_mse(rgb, pix, torch.ones(300))
    loss.backward()
    ref = torch.nn.functional.mse_loss(rgb.detach(), pix)
    assert abs(float(loss.detach()) - float(ref)) <= 908 * 2.0 ** -23 * float(ref) and not e.requires_grad
    assert torch.allclose(rgb.grad, 2.0 * (rgb.detach() - pix) / 900.0, rtol=1e-5, atol=1e-9)
    assert torch.allclose(e.mean(), ref, rtol=1e-5)


def test_loader_is_unchanged_when_off(tmp_path):
    """With the option off a TransformsLoader's training batch is `_pixels_to_sample` + `camera_rays_torch`, key for key and
    tensor for tensor; with a sampler set the same loader hands out the sampler's pixels and their weights."""
    from test_camera_twin import write_capture
    from cnc_amd.backends import camera_backend
    from cnc_amd.datasets import TransformsLoader
    root = str(tmp_path)
    meta = {"fl_x": 30.0, "fl_y": 31.0, "cx": 6.5, "cy": 3.5, "w": 13, "h": 7, "aabb": [-1.0] * 3 + [1.0] * 3}
    write_capture(root, "tiny", n=9, W=13, H=7, meta=meta)

    def loader():
        ld = TransformsLoader("tiny", root, "train", num_rays=37, color_bkgd_aug="random")
        ld.seed_sampling(5)
        return ld
    ld, ref = loader(), loader()
    assert ld.sampler is None and TransformsLoader.sampler is None
    for _ in range(2):
        batch = ld[0]
        assert set(batch) == {"pixels", "rays", "color_bkgd"}
        dev = ref.images.device
        ids, x, y, shape = ref._pixels_to_sample(0, dev)
        bkgd = ref._background(dev)
        o, d, pix = camera_backend.camera_rays_torch(ref.cameras, ref.model, ref.OPENGL_CAMERA, ids, x, y, ref.images, bkgd,
                                                     ref.eps, ref.iters)
        assert shape == (37,)
        assert torch.equal(batch["pixels"], pix) and torch.equal(batch["color_bkgd"], bkgd)
        assert torch.equal(batch["rays"].origins, o) and torch.equal(batch["rays"].viewdirs, d)
    # on: the sampler's draw from the loader's generator, one rand [n, 3]
    ld.sampler = EM.ErrorMapSampler(len(ld), ld.HEIGHT, ld.WIDTH, resolution=4, device="cpu")
    batch = ld[0]
    assert set(batch) == {"pixels", "rays", "color_bkgd", "camera_ids", "pixel_xy", "ray_weight"}
    ids, x, y, w = ld.sampler.draw(37, ref._gen)                          # (the twin loader's generator: the same state)
    px, py = batch["pixel_xy"]
    assert torch.equal(batch["camera_ids"], ids) and torch.equal(px, x) and torch.equal(py, y)
    assert torch.equal(batch["ray_weight"], w) and tuple(batch["pixels"].shape) == (37, 3)
    rgba = ld.images[ids, y, x].float() / 255.0
    assert torch.allclose(batch["pixels"], rgba[:, :3] * rgba[:, 3:] + batch["color_bkgd"] * (1 - rgba[:, 3:]))
    ld.training = False                                                   # a view is never drawn from the sampler
    assert set(ld[0]) == {"pixels", "rays", "color_bkgd"}
