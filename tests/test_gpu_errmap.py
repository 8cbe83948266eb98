"""GPU: the error-map kernels (csrc/error_map.hip) through the C ABI against tests/errmap_twin.py — every
operand in a sentinel-filled allocation (tests/guarded.py) — and the option in the Trainer on a capture the test writes:
the procedural ball, 5 views of 32 x 32 pixels, 4 of them training views.

The float32 twin follows the order of operations include/cnc_hip.h states, so the comparisons are of bits, the CDF's
included; the loss is also held to float64 within the bound of its summation length."""
import builtins
import os
import sys

import numpy as np
import pytest
import torch

import errmap_twin as T
import test_gpu_reproducible_step as R
from guarded import Guarded, same_bits
from test_gpu_guarded_trainer import SHAPE

pytestmark = pytest.mark.gpu
NS = [1, 63, 64, 65, 4097]
SHAPES = [(1, 7, 13, 1), (3, 7, 13, 4), (2, 33, 65, 16), (5, 16, 16, 64)]          # (n_cams, H, W, G)
ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))


def _lib(cuda):
    from cnc_amd import _lib as L
    return L.lib(), L.stream(cuda), L.check


def _map(shape, seed):
    n_cams, _, _, G = shape
    return np.random.default_rng(seed).uniform(1e-4, 1.0, (n_cams, G, G)).astype(np.float32) ** 3


def _all_intact(*bufs):
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs)


# ---------------------------------------------------------------------------------------------------------------- sample
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_sample_equals_the_twin(cuda, shape, n):
    n_cams, H, W, G = shape
    lib, s, check = _lib(cuda)
    prob, cdf = T.cdf(_map(shape, n), n_cams, H, W, G, 0.5)
    rand = np.random.default_rng(n + G).uniform(size=(n, 3)).astype(np.float32)
    rand[0] = 0.0                                              # exactly 0, and the last float below 1
    if n > 1:
        rand[1] = ONE_BELOW
        rand[n // 2] = [ONE_BELOW, 0.0, ONE_BELOW]
    want = T.sample(rand, cdf, prob, n_cams, H, W, G)
    g_rand, g_cdf, g_prob = Guarded(rand, cuda), Guarded(cdf, cuda), Guarded(prob, cuda)
    outs = [Guarded.empty((n,), np.int64, cuda) for _ in range(3)] + [Guarded.empty((n,), np.float32, cuda)]
    check(lib.cnc_errmap_sample(g_rand.ptr, g_cdf.ptr, g_prob.ptr, n, n_cams, H, W, G, *[o.ptr for o in outs], s), "sample")
    _all_intact(g_rand, g_cdf, g_prob, *outs)
    for o, w, name in zip(outs, want, ("cam_ids", "px", "py", "weight")):
        assert same_bits(o.get(), w), name
    ids, px, py = (o.get() for o in outs[:3])
    assert np.all((ids >= 0) & (ids < n_cams) & (px >= 0) & (px < W) & (py >= 0) & (py < H))
    assert float(outs[3].get().max()) <= 2.0 * (1 + 1e-6)


def test_sample_stays_inside_whatever_the_randoms_hold(cuda):
    """NaN, infinities, negatives and values >= 1: every output still lies in its range, nothing around a buffer is
    touched, and the integers equal the twin's (which clamps as the header says)."""
    shape = n_cams, H, W, G = (2, 7, 13, 16)                   # G > H: with empty cells
    lib, s, check = _lib(cuda)
    prob, cdf = T.cdf(_map(shape, 1), n_cams, H, W, G, 0.5)
    bad = np.asarray([np.nan, np.inf, -np.inf, -1.0, 1.0, 2.0, 1e30, -0.0], np.float32)
    rand = np.stack([np.repeat(bad, 64), np.tile(np.repeat(bad, 8), 8), np.tile(bad, 64)], axis=1)
    n = rand.shape[0]
    g_rand, g_cdf, g_prob = Guarded(rand, cuda), Guarded(cdf, cuda), Guarded(prob, cuda)
    outs = [Guarded.empty((n,), np.int64, cuda) for _ in range(3)] + [Guarded.empty((n,), np.float32, cuda)]
    check(lib.cnc_errmap_sample(g_rand.ptr, g_cdf.ptr, g_prob.ptr, n, n_cams, H, W, G, *[o.ptr for o in outs], s), "sample")
    _all_intact(g_rand, g_cdf, g_prob, *outs)
    ids, px, py, w = (o.get() for o in outs)
    assert np.all((ids >= 0) & (ids < n_cams) & (px >= 0) & (px < W) & (py >= 0) & (py < H)) and np.all(np.isfinite(w))
    want = T.sample(rand, cdf, prob, n_cams, H, W, G)
    for got, w_, name in zip((ids, px, py, w), want, ("cam_ids", "px", "py", "weight")):
        assert same_bits(got, w_), name


# ---------------------------------------------------------------------------------------------------------------- update
def _layout(kind, shape, rng):
    """(cam_ids, px, py) of the named ray layout."""
    n_cams, H, W, G = shape
    if kind == "one_cell":                                     # 4097 rays in one cell: a group longer than a block
        n = 4097
        k, gy, gx = n_cams - 1, G - 1, G - 1                    # (the last cell of an axis is never empty)
        ex, ey = T.cell_edges(W, G), T.cell_edges(H, G)
        assert ex[gx + 1] > ex[gx] and ey[gy + 1] > ey[gy]
        return (np.full(n, k), rng.integers(ex[gx], ex[gx + 1], n), rng.integers(ey[gy], ey[gy + 1], n))
    cells = np.unique(T.pixel_cells(n_cams, H, W, G).reshape(-1), return_index=True)
    first = cells[1]                                           # one pixel of every cell that has any
    if kind == "own_cell":
        pick = first
    else:                                                      # "sparse": a third of the cells, several rays in some
        pick = np.concatenate([first[::3], first[::9], first[::9]])
    pick = rng.permutation(pick)
    k, rem = pick // (H * W), pick % (H * W)
    return k, rem % W, rem // W


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind", ["one_cell", "own_cell", "sparse"])
def test_update_equals_the_twin(cuda, shape, kind):
    n_cams, H, W, G = shape
    lib, s, check = _lib(cuda)
    rng = np.random.default_rng(G + len(kind))
    ids, px, py = (np.ascontiguousarray(a, np.int64) for a in _layout(kind, shape, rng))
    n = ids.shape[0]
    err = (rng.uniform(size=n) ** 2).astype(np.float32)
    if n > 2:
        err[n // 2], err[n - 1] = np.nan, np.inf               # ignored on the device
    keys = T.keys(ids, px, py, n_cams, H, W, G)
    touched = np.zeros(n_cams * G * G, bool)
    touched[keys[np.isfinite(err)]] = True
    m0 = _map(shape, 3)
    flat = m0.reshape(-1)
    rest = np.nonzero(~touched)[0]                             # bit patterns an untouched cell must keep
    flat[rest[::3]] = -0.0
    flat.view(np.uint32)[rest[1::3]] = 0x7FC12345
    g_ids, g_px, g_py, g_err = Guarded(ids, cuda), Guarded(px, cuda), Guarded(py, cuda), Guarded(err, cuda)
    g_keys = Guarded.empty((n,), np.int32, cuda)
    check(lib.cnc_errmap_keys(g_ids.ptr, g_px.ptr, g_py.ptr, n, n_cams, H, W, G, g_keys.ptr, s), "keys")
    _all_intact(g_ids, g_px, g_py, g_keys)
    assert same_bits(g_keys.get(), keys)
    # the grouping as the package makes it: a stable sort and the segment bounds
    sorted_keys, order = torch.sort(g_keys.tensor(), stable=True)
    offsets = torch.searchsorted(sorted_keys, torch.arange(m0.size + 1, dtype=torch.int32, device=cuda))
    g_order, g_off = Guarded.like(order), Guarded.like(offsets.contiguous())
    g_map = Guarded(m0, cuda).out()
    check(lib.cnc_errmap_update(g_order.ptr, g_off.ptr, g_err.ptr, n, n_cams, G, 0.9, g_map.ptr, s), "update")
    _all_intact(g_order, g_off, g_err, g_map)
    got, want = g_map.get(), T.update(m0, keys, err, 0.9)
    assert same_bits(got, want)
    assert touched.any() and (kind == "own_cell" or m0.size == 1 or not touched.all())
    assert same_bits(got.reshape(-1)[~touched].view(np.uint32), m0.reshape(-1)[~touched].view(np.uint32))
    changed = got.reshape(-1).view(np.uint32) != m0.reshape(-1).view(np.uint32)
    assert not np.any(changed & ~touched) and changed.any()
    # an observation that holds nothing finite changes nothing; neither does one of no rays
    g_nan = Guarded(np.full(n, np.nan, np.float32), cuda)
    check(lib.cnc_errmap_update(g_order.ptr, g_off.ptr, g_nan.ptr, n, n_cams, G, 0.9, g_map.ptr, s), "update")
    check(lib.cnc_errmap_update(g_order.ptr, g_off.ptr, g_err.ptr, 0, n_cams, G, 0.9, g_map.ptr, s), "update")
    _all_intact(g_map, g_nan)
    assert same_bits(g_map.get(), want)


# ------------------------------------------------------------------------------------------------------------------- cdf
@pytest.mark.parametrize("shape", SHAPES + [(2, 7, 13, 16), (100, 20, 30, 16)])
def test_cdf_equals_the_twin(cuda, shape):
    n_cams, H, W, G = shape
    lib, s, check = _lib(cuda)
    hot = np.zeros((n_cams, G, G), np.float32)
    hot[-1, G // 2, -1] = 0.25
    mixed = _map(shape, 5)
    mixed.reshape(-1)[::3] = [np.nan, -1.0, 0.0][G % 3]
    for name, m in (("random", _map(shape, 4)), ("zero", np.zeros((n_cams, G, G), np.float32)),
                    ("nan", np.full((n_cams, G, G), np.nan, np.float32)), ("hot", hot), ("mixed", mixed)):
        for u in (0.5, 0.125):
            g_map = Guarded(m, cuda)
            g_prob, g_cdf = (Guarded.empty((m.size,), np.float32, cuda) for _ in range(2))
            check(lib.cnc_errmap_cdf(g_map.ptr, n_cams, H, W, G, u, g_prob.ptr, g_cdf.ptr, s), "cdf")
            _all_intact(g_map, g_prob, g_cdf)
            prob, cdf = T.cdf(m, n_cams, H, W, G, u)
            assert same_bits(g_prob.get(), prob), (name, u)
            assert same_bits(g_cdf.get(), cdf), (name, u)
            got = g_cdf.get()
            assert got[-1] == np.float32(1.0) and np.all(np.diff(got) >= 0), (name, u)
            cdf64 = T.cdf(m, n_cams, H, W, G, u, np.float64)[1]
            assert np.all(np.abs(got - cdf64) <= m.size * 2.0 ** -24), (name, u)
            if name in ("zero", "nan"):
                assert same_bits(g_prob.get(), T.areas(n_cams, H, W, G).astype(np.float32) / np.float32(n_cams * H * W))


# ------------------------------------------------------------------------------------------------------------------ loss
@pytest.mark.parametrize("n", NS + [70001])
def test_loss_forward_and_backward(cuda, n):
    lib, s, check = _lib(cuda)
    rng = np.random.default_rng(n)
    rgb, pix = rng.uniform(size=(n, 3)).astype(np.float32), rng.uniform(size=(n, 3)).astype(np.float32)
    w = rng.uniform(0.05, 2.0, n).astype(np.float32)
    g_rgb, g_pix, g_w = Guarded(rgb, cuda), Guarded(pix, cuda), Guarded(w, cuda)
    nbytes = int(lib.cnc_errmap_loss_workspace(n))
    assert nbytes == 4 * ((n + 255) // 256)
    runs = []
    for _ in range(2):
        ws = Guarded.empty((nbytes // 4,), np.float32, cuda).scratch()
        loss, err = Guarded.empty((1,), np.float32, cuda), Guarded.empty((n,), np.float32, cuda)
        check(lib.cnc_errmap_loss_forward(g_rgb.ptr, g_pix.ptr, g_w.ptr, n, ws.ptr, nbytes, loss.ptr, err.ptr, s), "loss")
        _all_intact(g_rgb, g_pix, g_w, ws, loss, err)
        runs.append((loss.get(), err.get()))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])       # two calls, the same bits
    got, e = float(runs[0][0][0]), runs[0][1]
    l64, e64 = T.loss_forward(rgb, pix, w, np.float64)
    terms = (w.astype(np.float64)[:, None] * (rgb.astype(np.float64) - pix) ** 2).sum() / (3 * n)
    print(f"errmap loss n={n}: |kernel - float64| = {abs(got - l64):.3e}, bound {(3 * n + 8) * 2.0 ** -24 * terms:.3e}")
    assert abs(got - l64) <= (3 * n + 8) * 2.0 ** -24 * terms
    l32, e32 = T.loss_forward(rgb, pix, w)
    assert same_bits(runs[0][0], np.asarray([l32], np.float32)) and same_bits(e, e32)
    assert np.allclose(e, e64, rtol=1e-6, atol=0)
    # all weights 1: F.mse_loss within the summation bound of both sums
    g_one = Guarded(np.ones(n, np.float32), cuda)
    ws = Guarded.empty((nbytes // 4,), np.float32, cuda).scratch()
    loss, err = Guarded.empty((1,), np.float32, cuda), Guarded.empty((n,), np.float32, cuda)
    check(lib.cnc_errmap_loss_forward(g_rgb.ptr, g_pix.ptr, g_one.ptr, n, ws.ptr, nbytes, loss.ptr, err.ptr, s), "loss")
    mse = float(torch.nn.functional.mse_loss(g_rgb.tensor(), g_pix.tensor()))
    assert abs(float(loss.get()[0]) - mse) <= (3 * n + 8) * 2.0 ** -23 * mse
    # backward: the twin's bits
    g = Guarded(np.asarray([1024.0], np.float32), cuda)
    g_out = Guarded.empty((n, 3), np.float32, cuda)
    check(lib.cnc_errmap_loss_backward(g.ptr, g_rgb.ptr, g_pix.ptr, g_w.ptr, n, g_out.ptr, s), "loss backward")
    _all_intact(g, g_rgb, g_pix, g_w, g_out)
    assert same_bits(g_out.get(), T.loss_backward(1024.0, rgb, pix, w))


def test_entries_refuse_what_they_cannot_take(cuda):
    lib, s, _ = _lib(cuda)
    buf = Guarded(np.zeros(64, np.float32), cuda)
    i64 = Guarded(np.zeros(8, np.int64), cuda)
    assert lib.cnc_errmap_cdf(buf.ptr, 1, 4, 4, 65, 0.5, buf.ptr, buf.ptr, s) != 0               # G > 64
    assert lib.cnc_errmap_cdf(buf.ptr, 1, 4, 4, 0, 0.5, buf.ptr, buf.ptr, s) != 0
    assert lib.cnc_errmap_cdf(buf.ptr, 1, 4, 4, 2, 1.5, buf.ptr, buf.ptr, s) != 0                # the floor outside [0, 1]
    assert lib.cnc_errmap_cdf(None, 1, 4, 4, 2, 0.5, buf.ptr, buf.ptr, s) != 0
    assert lib.cnc_errmap_sample(buf.ptr, buf.ptr, buf.ptr, 4, 200, 4, 4, 64, i64.ptr, i64.ptr, i64.ptr, buf.ptr, s) != 0
    assert lib.cnc_errmap_sample(buf.ptr + 2, buf.ptr, buf.ptr, 4, 1, 4, 4, 2, i64.ptr, i64.ptr, i64.ptr, buf.ptr, s) != 0
    assert lib.cnc_errmap_loss_forward(buf.ptr, buf.ptr, buf.ptr, 8, buf.ptr, 0, buf.ptr, buf.ptr, s) != 0   # no workspace
    assert lib.cnc_errmap_loss_forward(buf.ptr, buf.ptr, buf.ptr, 0, buf.ptr, 4, buf.ptr, buf.ptr, s) != 0
    assert lib.cnc_errmap_sample(buf.ptr, buf.ptr, buf.ptr, 0, 1, 4, 4, 2, None, None, None, None, s) == 0   # no rays: nothing
    torch.cuda.synchronize()
    assert buf.intact() and i64.intact() and not buf.get().any()
    from cnc_amd.backends import errmap_backend as K
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        K.loss_forward(torch.rand(4, 3), torch.rand(4, 3), torch.ones(4))


def test_sampler_object_and_autograd_on_the_gpu(cuda):
    """The package's path: ErrorMapSampler on the device equals the one on the host bit for bit, and the weighted loss
    back-propagates through the kernel."""
    from cnc_amd import error_map as EM
    dev_s = EM.ErrorMapSampler(3, 7, 13, resolution=4, refresh_every=8, device=cuda)
    host_s = EM.ErrorMapSampler(3, 7, 13, resolution=4, refresh_every=8, device="cpu")
    assert same_bits(dev_s.cdf, host_s.cdf) and same_bits(dev_s.prob, host_s.prob)
    rng = np.random.default_rng(0)
    for rounds in range(3):
        ids, px, py = rng.integers(0, 3, 300), rng.integers(0, 13, 300), rng.integers(0, 7, 300)
        err = (rng.uniform(size=300) ** 2).astype(np.float32)
        err[5] = np.nan
        for sm, dev in ((dev_s, cuda), (host_s, "cpu")):
            sm.observe(*(torch.from_numpy(a).to(dev) for a in (ids, px, py, err)))
            sm.refresh()
        assert same_bits(dev_s.map, host_s.map) and same_bits(dev_s.cdf, host_s.cdf) and same_bits(dev_s.prob, host_s.prob)
    assert dev_s.effective_fraction() == pytest.approx(host_s.effective_fraction(), rel=1e-12)
    a = dev_s.draw(1000, torch.Generator(device=cuda).manual_seed(4))
    b = dev_s.draw(1000, torch.Generator(device=cuda).manual_seed(4))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[0].dtype == torch.int64 and a[3].dtype == torch.float32
    rgb = torch.rand(1000, 3, device=cuda, requires_grad=True)
    pix = torch.rand(1000, 3, device=cuda)
    loss, e = EM.weighted_mse(rgb, pix, a[3])
    (loss * 1024.0).backward()
    want = T.loss_backward(1024.0, rgb.detach().cpu().numpy(), pix.cpu().numpy(), a[3].cpu().numpy())
    assert same_bits(rgb.grad, want) and not e.requires_grad


# --------------------------------------------------------------------------------------------------------------- Trainer
VIEWS, SIDE, FOCAL = 5, 32, 40.0


@pytest.fixture(scope="module")
def tiny_capture(tmp_path_factory):
    """root of a capture `tiny_ball`: the procedural ball from 5 pinhole cameras (OpenGL axes) at 32 x 32 pixels with alpha,
    frames 1..4 the training views."""
    import json
    from cnc_amd.datasets import SyntheticBallDataset
    from test_camera_twin import write_capture
    root = str(tmp_path_factory.mktemp("errmap_capture"))
    c2w = SyntheticBallDataset._poses(VIEWS, torch.Generator().manual_seed(77))           # [n, 3, 4]
    ys, xs = torch.meshgrid(torch.arange(SIDE), torch.arange(SIDE), indexing="ij")
    x, y = xs.reshape(-1).float(), ys.reshape(-1).float()
    cam = torch.stack([(x - SIDE / 2 + 0.5) / FOCAL, -(y - SIDE / 2 + 0.5) / FOCAL, -torch.ones_like(x)], dim=-1)
    shader = SyntheticBallDataset.__new__(SyntheticBallDataset)
    images = np.zeros((VIEWS, SIDE, SIDE, 4), np.uint8)
    for i in range(VIEWS):
        d = (cam[:, None, :] * c2w[i, :3, :3][None]).sum(-1)
        d = d / d.norm(dim=-1, keepdim=True)
        rgb, alpha = shader._shade(c2w[i, :3, 3].expand_as(d).contiguous(), d.contiguous())
        images[i] = (torch.cat([rgb, alpha], -1) * 255).round().to(torch.uint8).numpy().reshape(SIDE, SIDE, 4)
    assert 0.05 < (images[..., 3] > 0).mean() < 0.6                                   # the ball fills part of each frame
    meta = {"fl_x": FOCAL, "fl_y": FOCAL, "cx": SIDE / 2, "cy": SIDE / 2, "w": SIDE, "h": SIDE, "aabb": [-1.5] * 3 + [1.5] * 3}
    write_capture(root, "tiny_ball", n=VIEWS, W=SIDE, H=SIDE, meta=meta, images=images)
    path = os.path.join(root, "tiny_ball", "transforms.json")
    doc = json.load(open(path))
    for fr, pose in zip(doc["frames"], c2w):
        fr["transform_matrix"] = torch.cat([pose, torch.tensor([[0.0, 0.0, 0.0, 1.0]])]).tolist()
    json.dump(doc, open(path, "w"))
    return root


def _trainer(cuda, tmp_path, root, **kw):
    from test_gpu_pose_trainer import _trainer as make
    return make(cuda, tmp_path, root, scene="tiny_ball", **kw)


ON = dict(error_map=True, error_map_resolution=8, error_map_refresh_every=8)
STEPS = 24


def _record(tr):
    """Every batch the Trainer's dataset hands out, as host copies of what the sampler drew."""
    seen = []
    fetch = tr.dataset.fetch

    def recording():
        d = fetch()
        seen.append(d)
        return d
    tr.dataset.fetch = recording
    return seen


def _drawn(seen):
    torch.cuda.synchronize()
    return [tuple(t.cpu() for t in (d["camera_ids"], *d["pixel_xy"], d["ray_weight"])) for d in seen]


def test_option_runs_and_the_map_learns(cuda, tiny_capture, tmp_path, monkeypatch):
    monkeypatch.delenv("CNC_ERROR_MAP", raising=False)
    tr = _trainer(cuda, tmp_path, tiny_capture, **ON)
    em = tr.error_map
    assert em is not None and tr.dataset.train.sampler is em and len(tr.dataset.train) == 4
    assert (em.n_cams, em.height, em.width, em.resolution, em.refresh_every) == (4, SIDE, SIDE, 8, 8)
    assert (em.uniform_floor, em.decay) == (0.5, 0.9)
    start_map, start_cdf = em.map.clone(), em.cdf.clone()
    assert em.effective_fraction() == pytest.approx(1.0, abs=1e-6)
    seen = _record(tr)
    lines = []
    tr.cfg.log_every = 8
    tr.train(steps=STEPS - 1, log=lines.append)
    torch.cuda.synchronize()
    assert all(set(d) >= {"camera_ids", "pixel_xy", "ray_weight"} for d in seen) and len(seen) >= STEPS
    assert not torch.equal(em.map, start_map) and not torch.equal(em.cdf, start_cdf)
    assert bool(torch.isfinite(em.map).all()) and float(em.cdf[-1]) == 1.0 and bool((em.cdf.diff() >= 0).all())
    assert 0.0 < em.effective_fraction() < 1.0
    assert all(float(w.max()) <= 2.0 * (1 + 1e-6) and float(w.min()) > 0 for *_, w in _drawn(seen))
    assert lines and all(" | errmap_cover=" in ln for ln in lines)
    # the environment variable switches it on as well; what cannot work raises
    monkeypatch.setenv("CNC_ERROR_MAP", "1")
    assert _trainer(cuda, tmp_path / "env", tiny_capture).error_map is not None
    from cnc_amd.trainer import Trainer
    with pytest.raises(ValueError, match="TransformsLoader"):
        Trainer(R._cfg(tmp_path / "ball", seed=3, **SHAPE), device=cuda)                # the synthetic dataset
    monkeypatch.delenv("CNC_ERROR_MAP")
    plain = _trainer(cuda, tmp_path / "dp", tiny_capture)
    plain.dp, plain.world = True, 2
    with pytest.raises(ValueError, match="data-parallel"):
        plain.enable_error_map_sampling()
    plain.dp, plain.world = False, 1
    with pytest.raises(ValueError, match="1..64"):
        plain.enable_error_map_sampling(resolution=65)
    assert plain.error_map is None and plain.dataset.train.sampler is None


def test_reproducible_runs_give_the_same_batches_and_map(cuda, tiny_capture, tmp_path):
    """Two runs from one seed in the reproducible mode: every batch, the map, the distribution and the field bit for bit;
    and a step with a NaN batch under the guarded step leaves the map finite."""
    runs = []
    for k in range(2):
        tr = _trainer(cuda, tmp_path / str(k), tiny_capture, reproducible=True, guarded_step=True, **ON)
        seen = _record(tr)
        for s in range(STEPS):
            if s == 11:                                         # a poisoned batch: the step is skipped, the map ignores it
                from test_gpu_guarded_trainer import _nan_batch
                tr._next_data = _nan_batch(tr)
            tr.train_step(s, want_stats=False)
        torch.cuda.synchronize()
        assert tr.step_guard.stats()["skipped"] == 1
        assert bool(torch.isfinite(tr.error_map.map).all())
        runs.append((_drawn(seen), tr.error_map.map.clone(), tr.error_map.cdf.clone(), R._state(tr)))
    (b0, m0, c0, s0), (b1, m1, c1, s1) = runs
    assert len(b0) == len(b1) and all(all(torch.equal(x, y) for x, y in zip(p, q)) for p, q in zip(b0, b1))
    assert same_bits(m0, m1) and same_bits(c0, c1)
    assert all(R._bits(s0[k]).equal(R._bits(s1[k])) for k in s0)


def test_both_schedules_draw_the_same_batches(cuda, tiny_capture, tmp_path):
    """The order of events: the batch of step s + 1 is drawn from the CDF rebuilt at the end of step s where (s + 1) % 8 == 0,
    whether `_prefetch` draws it on the look-ahead stream during step s's backward or `fetch()` draws it at the top of step
    s + 1.  The threaded schedule's gradients differ in their last bits from run to run, so here the error that reaches the
    map is replaced by a function of the pixel alone: the sequence of batches then depends on the order of events only."""
    def run(sub, prefetch, **kw):
        tr = _trainer(cuda, tmp_path / sub, tiny_capture, target_sample_batch_size=0, **ON, **kw)
        tr.prefetch = prefetch
        em = tr.error_map
        observe = em.observe
        em.observe = lambda ids, px, py, err: observe(ids, px, py, ((ids * 7 + px * 3 + py) % 11).float() / 11.0 + 0.01)
        seen = _record(tr)
        for s in range(STEPS):
            assert tr.train_step(s, want_stats=False) is not None
        torch.cuda.synchronize()
        return tr, _drawn(seen), em.map.clone(), em.cdf.clone()
    tr_a, b_a, m_a, c_a = run("ahead", True)
    assert tr_a.ctx_thread and tr_a.ahead_stream is not None                              # the look-ahead draw was in use
    tr_b, b_b, m_b, c_b = run("top", False)
    tr_c, b_c, m_c, c_c = run("plain", True, reproducible=True)
    assert len(b_a) >= STEPS and len(b_b) >= STEPS
    for other, m, c in ((b_b, m_b, c_b), (b_c, m_c, c_c)):
        assert all(all(torch.equal(x, y) for x, y in zip(p, q)) for p, q in zip(b_a[:STEPS], other[:STEPS]))
        assert same_bits(m_a, m) and same_bits(c_a, c)
    assert not torch.equal(b_a[0][3], b_a[STEPS - 1][3])                                  # the weights moved with the map


def test_off_is_bit_equal_to_a_run_that_cannot_import_the_module(cuda, tiny_capture, tmp_path, monkeypatch):
    """Option off, reproducible mode, 24 steps: once with `cnc_amd.error_map` impossible to import, once as usual — the same
    parameters and optimizer state bit for bit, the same batch keys, and no field more in the log."""
    monkeypatch.delenv("CNC_ERROR_MAP", raising=False)

    def run(sub):
        tr = _trainer(cuda, tmp_path / sub, tiny_capture, reproducible=True)
        assert tr.error_map is None and tr.dataset.train.sampler is None
        seen = _record(tr)
        lines = []
        tr.cfg.log_every = 8
        tr.train(steps=STEPS - 1, log=lines.append)
        torch.cuda.synchronize()
        assert all(set(d) == {"pixels", "rays", "color_bkgd"} for d in seen)
        assert lines and not any("errmap" in ln for ln in lines)
        return R._state(tr)
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k in ("cnc_amd.error_map", "cnc_amd.backends.errmap_backend")}
    real_import = builtins.__import__

    def refusing(name, globals=None, locals=None, fromlist=(), level=0):
        full = name if level == 0 else f"{(globals or {}).get('__package__', '')}.{name}".strip(".")
        wanted = [full] + [f"{full}.{f}" for f in (fromlist or ())]
        if any(w.endswith(("error_map", "errmap_backend")) for w in wanted):
            raise ImportError(f"{full}: not in this run")
        return real_import(name, globals, locals, fromlist, level)
    monkeypatch.setattr(builtins, "__import__", refusing)
    try:
        without = run("without")
        assert "cnc_amd.error_map" not in sys.modules and "cnc_amd.backends.errmap_backend" not in sys.modules
    finally:
        monkeypatch.setattr(builtins, "__import__", real_import)
        sys.modules.update(saved)
    import cnc_amd.error_map  # noqa: F401
    usual = run("usual")
    assert set(without) == set(usual) and all(R._bits(without[k]).equal(R._bits(usual[k])) for k in usual)
