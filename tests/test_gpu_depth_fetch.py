"""GPU: cnc_depth_fetch (cnc_amd/csrc/depth_loss.hip) through the C ABI between sentinel-filled guards on a 3-camera, 5 x 7
capture — both camera conventions, Euclidean and z-depth, planes with 0, NaN and negatives, one camera turned so that some
rays lie at or past 90 degrees from its axis — against the float64 twin within the bound derived there; and a
`TransformsLoader` on the GPU against the torch path."""
import numpy as np
import pytest
import torch

import depth_capture as C
import depth_twin as T
from guarded import Guarded

pytestmark = pytest.mark.gpu
f32, i64 = np.float32, np.int64
H, W, CAMS = 5, 7, 3


def _inputs(rng):
    """Camera rows with rotations about y by 0.2, 1.3 and 2.2 rad (the third looks away from the rays below), planes with
    holes, every pixel of every camera, and unit directions in a cone around +z."""
    cams = np.zeros((CAMS, 24), f32)
    cams[:, :4] = [9.0, 9.5, 3.4, 2.6]
    for k, a in enumerate((0.2, 1.3, 2.2)):
        rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        cams[k, 4:16] = np.concatenate([rot, rng.uniform(-1, 1, (3, 1))], axis=1).reshape(-1).astype(f32)
    planes = rng.uniform(0.5, 6.0, (CAMS, H, W)).astype(f32)
    planes[0, 0, 0], planes[1, 2, 3], planes[2, 4, 6], planes[0, 3, 1] = 0.0, np.nan, -2.0, np.inf
    ids, py, px = (a.reshape(-1).astype(i64) for a in np.meshgrid(np.arange(CAMS), np.arange(H), np.arange(W), indexing="ij"))
    d = np.stack([rng.uniform(-0.6, 0.6, ids.size), rng.uniform(-0.6, 0.6, ids.size), np.ones(ids.size)], -1)
    dirs = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    return cams, planes, ids, px, py, dirs


@pytest.mark.parametrize("opengl", [False, True])
@pytest.mark.parametrize("euclidean", [False, True])
def test_depth_fetch_through_the_c_abi(cuda, opengl, euclidean):
    """Largest error / bound measured on the MI355X: 0.27 for z-depth (1 / c up to 25.7), 0 for Euclidean depth (a copy)."""
    from cnc_amd import _lib
    rng = np.random.default_rng(3)
    cams, planes, ids, px, py, dirs = _inputs(rng)
    if opengl:
        dirs = -dirs              # an OpenGL camera looks down -z: the same rays in front of it
    n = ids.size
    gp, gc, gd = Guarded(planes, cuda), Guarded(cams, cuda), Guarded(dirs, cuda)
    gi, gx, gy = (Guarded(a, cuda) for a in (ids, px, py))
    out = Guarded.empty((n,), f32, cuda)
    L = _lib.lib()
    _lib.check(L.cnc_depth_fetch(gp.ptr, gc.ptr, CAMS, H, W, int(opengl), int(euclidean), gi.ptr, gx.ptr, gy.ptr, gd.ptr, n,
                                 out.ptr, _lib.stream(cuda)), "depth_fetch")
    torch.cuda.synchronize()
    for g in (gp, gc, gd, gi, gx, gy, out):
        assert g.intact()
    got = out.get()
    want, c, z = T.fetch64(planes, cams, opengl, euclidean, ids, px, py, dirs)
    tol = T.fetch_bound(cams, euclidean, ids, dirs, want, c)
    assert np.all(np.abs(c) > 1e-3)                       # no ray so close to 90 degrees that float32 could see another sign
    none = ~(np.isfinite(z) & (z > 0) & (c > 0))
    assert not got[none].view(np.uint32).any()            # exactly +0
    assert np.isnan(z).any() and (z == 0).any() and (z < 0).any() and np.isinf(z).any()
    if not euclidean:
        assert (c <= 0).sum() >= 5 and (c[ids == 2] <= 0).any() and (c[ids == 0] > 0).all()
    err = np.abs(got.astype(np.float64) - want)
    print(f"largest error / bound: {T.ratio(got, want, tol):.3g}; largest 1 / c: {1.0 / c[c > 0].min():.3g}")
    assert np.all(err <= tol)
    if euclidean:
        assert np.array_equal(got[~none], z[~none].astype(f32))
    # out-of-range indices are clamped for the loads: nothing outside the planes or the table is touched, nothing faults
    wild = Guarded(np.array([-5, 99, 1], i64), cuda)
    wx, wy = Guarded(np.array([-1, 3, 70], i64), cuda), Guarded(np.array([9, -2, 2], i64), cuda)
    out3 = Guarded.empty((3,), f32, cuda)
    _lib.check(L.cnc_depth_fetch(gp.ptr, gc.ptr, CAMS, H, W, int(opengl), 1, wild.ptr, wx.ptr, wy.ptr, gd.ptr, 3, out3.ptr,
                                 _lib.stream(cuda)), "depth_fetch")
    torch.cuda.synchronize()
    assert out3.intact()
    clamped = planes[[0, 2, 1], [4, 0, 2], [0, 3, 6]]
    assert np.array_equal(out3.get(), np.where(np.isfinite(clamped) & (clamped > 0), clamped, 0).astype(f32))


def test_c_abi_refuses_missing_buffers(cuda):
    from cnc_amd import _lib
    x = torch.zeros(64, device=cuda)
    i = torch.zeros(4, dtype=torch.int64, device=cuda)
    L, st, p, q = _lib.lib(), _lib.stream(cuda), x.data_ptr(), i.data_ptr()
    assert L.cnc_depth_fetch(p, None, 1, 2, 2, 0, 0, q, q, q, p, 4, p, st) != 0          # z-depth needs the camera table
    assert L.cnc_depth_fetch(p, p, 1, 2, 2, 0, 0, q, q, q, None, 4, p, st) != 0          # ... and the directions
    assert L.cnc_depth_fetch(p, p, 0, 2, 2, 0, 1, q, q, q, p, 4, p, st) != 0
    assert L.cnc_depth_fetch(p, None, 1, 2, 2, 0, 1, q, q, q, None, 4, p, st) == 0       # Euclidean depth reads neither
    torch.cuda.synchronize()


@pytest.mark.parametrize("euclidean", [False, True])
def test_loader_on_the_gpu_equals_the_torch_path(cuda, tmp_path, euclidean):
    planes, _ = C.write(tmp_path, euclidean=euclidean)
    host, dev = C.loader(tmp_path, torch.device("cpu"), num_rays=256), C.loader(tmp_path, cuda, num_rays=256)
    host.with_depth = dev.with_depth = True
    batch = dev[0]
    assert set(batch) == {"pixels", "rays", "color_bkgd", "depth"} and batch["depth"].is_cuda
    assert dev.depth_planes().is_cuda and np.array_equal(dev.depth_planes().cpu().numpy(), planes, equal_nan=True)
    # the device generator's draws are its own: fetch the same list on both paths
    g = torch.Generator(device=cuda).manual_seed(5)
    ids = torch.randint(0, 3, (256,), device=cuda, generator=g)
    px = torch.randint(0, C.W, (256,), device=cuda, generator=g)
    py = torch.randint(0, C.H, (256,), device=cuda, generator=g)
    got = batch["depth"].cpu().numpy().astype(np.float64)
    dirs = batch["rays"].viewdirs
    via_torch = host._fetch_depth(ids.cpu(), px.cpu(), py.cpu(), dirs.cpu()).numpy().astype(np.float64)
    want, c, z = T.fetch64(planes, dev.cameras.cpu().numpy(), True, euclidean, ids.cpu().numpy(), px.cpu().numpy(),
                           py.cpu().numpy(), dirs.cpu().numpy())
    tol = T.fetch_bound(dev.cameras.cpu().numpy(), euclidean, ids.cpu().numpy(), dirs.cpu().numpy(), want, c)
    assert np.all(np.abs(got - want) <= tol) and np.all(np.abs(via_torch - want) <= tol)
    assert np.all(np.abs(got - via_torch) <= 2 * tol)
    none = ~(np.isfinite(z) & (z > 0))
    assert none.any() and not got[none].any() and (got[~none] > 0).all()
