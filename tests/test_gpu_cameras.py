"""GPU: the camera kernels (csrc/camera.hip) against the float64 twin (tests/camera_twin.py) on the golden's inputs
(tests/golden/cameras.npz), through the C ABI with every device buffer guarded (tests/guarded.py), and the mirrors
`nerfacc.cuda.opencv_lens_undistortion*` / `nerfacc.cameras` through the drop-in names.

Bounds.  Layouts 5 and 8: 4 x `ref_err`, the reference's own float32 twin against float64 on these inputs (the margin
covers the kernel's early exit and another operation order).  Layout 12 and the fisheye have no float32 reference twin:
4 x the error of the twin's float32 mode against float64 on the same inputs (the margin covers the device tan / sqrt).
cnc_camera_rays: origins bit-equal to the pose column; every viewdirs component within 24 x 2^-24 of the twin (first
order on a unit vector: three roundings per camera-space component, six per rotated component weighted by at most
sqrt(3), and the normalisation — tests/test_camera_twin.py confirms that the float32 torch chain of the existing loaders
meets it), plus the undistortion bound for the distorted models; pixels within 2^-23 of the torch expression."""
import os

import numpy as np
import pytest
import torch

import camera_twin as T
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ULP = 2.0 ** -24
VIEWDIR_BOUND = 24 * ULP
SIZES = [1, 63, 64, 65, 257, 4099]          # one point per lane, 256 per block, no grid-stride loop: 4099 = 16 blocks + 3
EPS, ITERS = 1e-6, 10
FISH = [[-0.02, 0.003, -5e-4, 1e-4], [0.05, -0.01, 0.002, -3e-4]]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "cameras.npz"))


@pytest.fixture(scope="module")
def L(cuda):
    from cnc_amd import _lib
    return _lib.lib()


def take(a, n):
    """The first n points of a golden array; past its 4096 it starts over (4099 is there for the launch shape)."""
    return a[np.arange(n) % a.shape[0]]


def _stream(dev):
    from cnc_amd import _lib
    return _lib.stream(dev)


def undistort(L, dev, uv, params, layout, shared, eps=EPS, iters=ITERS):
    """cnc_lens_undistort / _fisheye (layout 4) on guarded buffers.  params: one row, used as it is (shared) or
    repeated per point."""
    uv = np.ascontiguousarray(uv, np.float32)
    n = uv.shape[0]
    rows = np.asarray(params, np.float32).reshape(1, -1)
    rows = rows if shared else (np.repeat(rows, n, 0) if rows.shape[0] == 1 else rows)
    g_uv, g_p = Guarded(uv, dev), Guarded(rows, dev)
    g_out = Guarded.empty((n, 2), np.float32, dev)
    snaps = g_uv.snapshot(), g_p.snapshot()
    stride = 0 if shared else rows.shape[1]
    if layout == 4:
        rc = L.cnc_lens_undistort_fisheye(g_uv.ptr, g_p.ptr, stride, eps, iters, g_out.ptr, n, _stream(dev))
    else:
        rc = L.cnc_lens_undistort(g_uv.ptr, g_p.ptr, stride, layout, eps, iters, g_out.ptr, n, _stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert g_out.intact() and g_uv.unchanged_since(snaps[0]) and g_p.unchanged_since(snaps[1])
    return g_out.get()


@pytest.mark.parametrize("n", SIZES)
def test_newton_layouts_against_the_float64_twin(cuda, L, golden, n):
    bound = 4 * float(golden["ref_err"])
    for i in range(int(golden["n_sets"])):
        uv, p8 = take(golden[f"uv_{i}"], n), golden[f"params_{i}"]
        want = T.undistort_newton(uv, p8, EPS, ITERS, np.float64)
        got = undistort(L, cuda, uv, p8, 8, shared=True)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"layout 8 set {i} n {n}: {err:.3e} (bound {bound:.3e})")
        assert np.isfinite(got).all() and err <= bound
        assert same_bits(got, undistort(L, cuda, uv, p8, 8, shared=False))          # shared row == the row per point
        if not p8[5:].any():                                                         # k4 k5 k6 zero: layout 5 says the same
            got5 = undistort(L, cuda, uv, p8[:5], 5, shared=True)
            assert same_bits(got5, got) and same_bits(got5, undistort(L, cuda, uv, p8[:5], 5, shared=False))


def test_kernel_and_float32_twin_agree_bit_for_bit(cuda, L, golden):
    """Contraction off, correctly rounded division: NumPy float32 in the kernel's operation order is the kernel."""
    for i in range(int(golden["n_sets"])):
        uv, p8 = golden[f"uv_{i}"], golden[f"params_{i}"]
        assert same_bits(undistort(L, cuda, uv, p8, 8, shared=True), T.undistort_newton(uv, p8, EPS, ITERS, np.float32))
    uv, p12 = golden["prism_uv"], golden["prism_params"]
    assert same_bits(undistort(L, cuda, uv, p12, 12, shared=True), T.undistort_fixed_point(uv, p12, ITERS, np.float32))


@pytest.mark.parametrize("n", SIZES)
def test_thin_prism_layout_against_the_float64_twin(cuda, L, golden, n):
    uv, p12 = take(golden["prism_uv"], n), golden["prism_params"]
    want = T.undistort_fixed_point(uv, p12, ITERS, np.float64)
    bound = 4 * np.abs(T.undistort_fixed_point(uv, p12, ITERS, np.float32).astype(np.float64) - want).max()
    got = undistort(L, cuda, uv, p12, 12, shared=True)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"layout 12 n {n}: {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all() and err <= bound
    assert same_bits(got, undistort(L, cuda, uv, p12, 12, shared=False))


@pytest.mark.parametrize("n", SIZES)
def test_fisheye_against_the_float64_twin(cuda, L, golden, n):
    for i in range(int(golden["n_fish"])):
        uv, k = take(golden[f"fish_uv_{i}"], n), golden[f"fish_params_{i}"]
        assert np.array_equal(k, np.asarray(FISH[i], np.float32))
        want = T.undistort_fisheye(uv, k, EPS, ITERS, np.float64)
        bound = 4 * np.abs(T.undistort_fisheye(uv, k, EPS, ITERS, np.float32).astype(np.float64) - want).max()
        got = undistort(L, cuda, uv, k, 4, shared=True)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"fisheye set {i} n {n}: {err:.3e} (bound {bound:.3e})")
        assert np.isfinite(got).all() and err <= bound
        assert same_bits(got, undistort(L, cuda, uv, k, 4, shared=False))


def test_mirror_shapes_broadcasts_and_refusals(cuda, golden):
    from cnc_amd.backends import nerfacc_cuda as nc
    from cnc_amd.nerfacc import cameras
    H, W = 5, 13
    uv = torch.from_numpy(golden["uv_3"][:H * W]).to(cuda).reshape(H, W, 2)
    p = torch.from_numpy(golden["params_3"]).to(cuda)
    a = cameras.opencv_lens_undistortion(uv, p)
    b = cameras.opencv_lens_undistortion(uv, p.reshape(1, 1, 8))
    c = cameras.opencv_lens_undistortion(uv, p.expand(H, W, 8).contiguous())
    assert a.shape == (H, W, 2) and same_bits(a, b) and same_bits(a, c)
    want = T.undistort_newton(golden["uv_3"][:H * W], golden["params_3"], EPS, ITERS, np.float32).reshape(H, W, 2)
    assert same_bits(a, want)
    # a row per image row, broadcast over the columns: not one shared row, so it is packed
    d = cameras.opencv_lens_undistortion(uv, p.reshape(1, 1, 8).repeat(H, 1, 1))
    assert same_bits(a, d)
    k = torch.tensor(FISH[1], device=cuda)
    fuv = torch.from_numpy(golden["fish_uv_1"][:H * W]).to(cuda).reshape(H, W, 2)
    fa = cameras.opencv_lens_undistortion_fisheye(fuv, k)
    assert fa.shape == (H, W, 2) and same_bits(fa, cameras.opencv_lens_undistortion_fisheye(fuv, k.expand(H, W, 4).contiguous()))
    # n = 0
    empty = torch.empty(0, 2, device=cuda)
    assert cameras.opencv_lens_undistortion(empty, p).shape == (0, 2)
    assert cameras.opencv_lens_undistortion_fisheye(empty, k).shape == (0, 2)
    assert cameras.opencv_lens_undistortion(uv, p[:0]) is uv
    # the extension's host checks
    wide = torch.rand(10, 4, device=cuda)
    with pytest.raises(RuntimeError, match="uv must be contiguous"):
        nc.opencv_lens_undistortion(wide[:, :2], p.expand(10, 8), EPS, ITERS)
    with pytest.raises(RuntimeError, match="params must be contiguous"):
        nc.opencv_lens_undistortion(wide[:, :2].contiguous(), torch.rand(10, 16, device=cuda)[:, :8], EPS, ITERS)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        nc.opencv_lens_undistortion(wide[:, :2].contiguous().cpu(), p.expand(10, 8), EPS, ITERS)
    with pytest.raises(RuntimeError, match="same number of dimensions"):
        nc.opencv_lens_undistortion(uv, p, EPS, ITERS)
    with pytest.raises(RuntimeError, match="params must have shape"):
        nc.opencv_lens_undistortion(uv, p[:4].expand(H, W, 4), EPS, ITERS)
    with pytest.raises(RuntimeError, match="params must have shape"):
        nc.opencv_lens_undistortion_fisheye(uv, p.expand(H, W, 8), EPS, ITERS)
    with pytest.raises(RuntimeError, match="float32"):
        nc.opencv_lens_undistortion(uv.double(), p.double().expand(H, W, 8), EPS, ITERS)


def test_argument_checks_return_the_negative_codes(cuda, L):
    s = _stream(cuda)
    buf = Guarded(np.zeros((64, 24), np.float32), cuda)
    out = Guarded.empty((64, 3), np.float32, cuda)
    ids = Guarded(np.zeros(64, np.int64), cuda)
    assert L.cnc_lens_undistort(None, None, 0, 8, EPS, ITERS, None, 0, s) == 0                    # n == 0: a no-op
    assert L.cnc_lens_undistort_fisheye(None, None, 0, EPS, ITERS, None, 0, s) == 0
    assert L.cnc_camera_rays(None, 0, 9, 1, None, None, None, 0, 0, 0, 0, EPS, ITERS, None, None, None, None, None, s) == 0
    assert L.cnc_lens_undistort(None, buf.ptr, 0, 8, EPS, ITERS, out.ptr, 4, s) == -1
    assert L.cnc_lens_undistort(buf.ptr, None, 0, 8, EPS, ITERS, out.ptr, 4, s) == -1
    assert L.cnc_lens_undistort(buf.ptr, buf.ptr, 0, 8, EPS, ITERS, None, 4, s) == -1
    for layout in (0, 4, 7, 9, 13):
        assert L.cnc_lens_undistort(buf.ptr, buf.ptr, 0, layout, EPS, ITERS, out.ptr, 4, s) == -1
    assert L.cnc_lens_undistort(buf.ptr, buf.ptr, 5, 8, EPS, ITERS, out.ptr, 4, s) == -1           # rows shorter than the layout
    assert L.cnc_lens_undistort(buf.ptr + 4, buf.ptr, 0, 8, EPS, ITERS, out.ptr, 4, s) == -1        # uv off its 8-byte alignment
    assert L.cnc_lens_undistort_fisheye(buf.ptr, None, 0, EPS, ITERS, out.ptr, 4, s) == -1
    assert L.cnc_lens_undistort_fisheye(buf.ptr, buf.ptr, 3, EPS, ITERS, out.ptr, 4, s) == -1
    rays = lambda cams, n_cams, model, cam_ids, px, py, o, d: L.cnc_camera_rays(
        cams, n_cams, model, 1, cam_ids, px, py, 0, 8, 8, 64, EPS, ITERS, None, None, o, d, None, s)
    assert rays(buf.ptr, 64, 0, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == 0
    assert rays(None, 64, 0, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, 0, 0, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, -3, 0, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, 64, 3, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, 64, -1, ids.ptr, ids.ptr, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, 64, 0, ids.ptr, None, ids.ptr, out.ptr, out.ptr) == -1
    assert rays(buf.ptr, 64, 0, ids.ptr, ids.ptr, ids.ptr, None, out.ptr) == -1
    assert rays(buf.ptr, 64, 0, ids.ptr, ids.ptr, ids.ptr, out.ptr, None) == -1
    assert rays(buf.ptr, 64, 0, None, None, None, out.ptr, out.ptr) == 0                          # full frame: 8 x 8 == 64
    frame = lambda cam0, w, h, n: L.cnc_camera_rays(buf.ptr, 64, 0, 1, None, None, None, cam0, w, h, n, EPS, ITERS, None, None,
                                                    out.ptr, out.ptr, None, s)
    assert frame(64, 8, 8, 64) == -1 and frame(-1, 8, 8, 64) == -1 and frame(0, 8, 7, 64) == -1 and frame(0, 0, 8, 64) == -1
    # a pixel fetch needs the background and the output
    assert L.cnc_camera_rays(buf.ptr, 64, 0, 1, ids.ptr, ids.ptr, ids.ptr, 0, 8, 8, 64, EPS, ITERS, buf.ptr, None, out.ptr,
                             out.ptr, out.ptr, s) == -1
    torch.cuda.synchronize()
    assert out.intact() and buf.intact() and ids.intact()


def test_edge_behaviour_is_the_twins(cuda, L):
    third = np.float32(-1.0 / 3.0)
    k = np.zeros(8, np.float32)
    k[0] = third
    # (1, 0): 1 + 3 k1 r^2 = 0 — the Jacobian is singular AT THE START, the twin stops on |det| < eps before any update
    # and the start comes back.  (2/3, 0) is that point's image: Newton from there is regular and must agree all the same.
    uv = np.asarray([[1.0, 0.0], [2.0 / 3.0, 0.0], [0.0, 1.0], [-1.0, 0.0]], np.float32)
    info = {}
    want = T.undistort_newton(uv, k, EPS, ITERS, np.float32, info)
    assert info["det_stop"][[0, 2, 3]].all() and (info["rounds"][[0, 2, 3]] == 0).all() and not info["det_stop"][1]
    assert same_bits(want[[0, 2, 3]], uv[[0, 2, 3]])
    for shared in (True, False):
        got = undistort(L, cuda, uv, k, 8, shared)
        assert np.isfinite(got).all() and same_bits(got, want)
        assert same_bits(undistort(L, cuda, uv, k[:5], 5, shared), want)
    # fisheye: the centre, beyond pi / 2 (clipped), and a row that cannot converge in one round
    kf = np.asarray(FISH[1], np.float32)
    uv = np.asarray([[0.0, 0.0], [3.0, 4.0], [-2.0, 0.5], [1e-7, -1e-7], [1.2, -0.7]], np.float32)
    info = {}
    want = T.undistort_fisheye(uv, kf, EPS, ITERS, np.float32, info)
    assert info["converged"].all() and not want[0].any() and not want[3].any()          # theta_d <= eps: scale 0
    clipped = T.undistort_fisheye(np.asarray([[0.6, 0.8]], np.float32) * np.float32(np.pi / 2), kf, EPS, ITERS, np.float32)
    assert np.allclose(want[1] / 5.0, clipped[0] / np.float32(np.pi / 2), rtol=1e-5)          # |uv| = 5 solved as |uv| = pi / 2
    got = undistort(L, cuda, uv, kf, 4, shared=True)
    assert np.isfinite(got).all() and same_bits(got, want) and same_bits(got, undistort(L, cuda, uv, kf, 4, shared=False))
    info = {}
    want1 = T.undistort_fisheye(uv, kf, EPS, 1, np.float32, info)
    assert not info["converged"][[1, 2, 4]].any() and same_bits(want1[[1, 2, 4]], uv[[1, 2, 4]])
    assert same_bits(undistort(L, cuda, uv, kf, 4, shared=True, iters=1), want1)
    # layout 12: the inverse radial factor (1 + k4 r + ..) / (1 + k1 r + ..) is negative at r = 1 for k1 = -2
    p12 = np.zeros(12, np.float32)
    p12[0] = -2.0
    uv = np.asarray([[1.0, 0.0], [0.1, 0.1], [0.6, -0.8]], np.float32)
    want = T.undistort_fixed_point(uv, p12, ITERS, np.float32)
    assert same_bits(want[[0, 2]], uv[[0, 2]]) and not same_bits(want[1], uv[1])
    got = undistort(L, cuda, uv, p12, 12, shared=True)
    assert np.isfinite(got).all() and same_bits(got, want)


# ---------------------------------------------------------------------------------------------- cnc_camera_rays
W, H = 65, 49


def _cameras():
    """Three cameras with different intrinsics, poses and coefficients (rows: opencv layout 8 | fisheye k1..k4)."""
    from test_camera_twin import _poses
    rng = np.random.default_rng(11)
    poses = _poses(rng, 3)
    intr = np.asarray([[61.0, 63.5, 32.25, 24.5], [70.0, 68.0, 30.0, 26.0], [55.5, 55.5, 33.5, 23.75]], np.float32)
    opencv = np.asarray([[-0.28, 0.07, 2e-4, -1e-4, 0, 0, 0, 0], [0.12, -0.05, 5e-4, -3e-4, 0.01, 0.05, -0.02, 0.004],
                         [-0.15, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    fish = np.asarray([FISH[0], FISH[1], [0.0, 0.0, 0.0, 0.0]], np.float32)
    return {T.PINHOLE: T.camera_table(intr, poses), T.OPENCV: T.camera_table(intr, poses, opencv),
            T.FISHEYE: T.camera_table(intr, poses, fish)}


def _undistortion_bound(table, model, ids, px, py, golden):
    """The undistortion kernels' bound on this call's own (u, v)."""
    if model == T.PINHOLE:
        return 0.0
    if model == T.OPENCV:
        return 4 * float(golden["ref_err"])
    row = table[ids]
    uv = np.stack([((px.astype(np.float32) - row[:, 2]) + np.float32(0.5)) / row[:, 0],
                   ((py.astype(np.float32) - row[:, 3]) + np.float32(0.5)) / row[:, 1]], -1)
    a = T.undistort_fisheye(uv, row[:, 16:20], EPS, ITERS, np.float32).astype(np.float64)
    return 4 * np.abs(a - T.undistort_fisheye(uv, row[:, 16:20], EPS, ITERS, np.float64)).max()


def rays(L, dev, table, model, opengl, ids=None, px=None, py=None, cam0=0, width=0, height=0, images=None, bkgd=None):
    n = len(ids) if ids is not None else width * height
    g_t = Guarded(table, dev)
    g_ids, g_x, g_y = (None if a is None else Guarded(np.asarray(a, np.int64), dev) for a in (ids, px, py))
    g_img = None if images is None else Guarded(images, dev)
    g_bk = None if bkgd is None else Guarded(np.asarray(bkgd, np.float32), dev)
    o, d = Guarded.empty((n, 3), np.float32, dev), Guarded.empty((n, 3), np.float32, dev)
    pix = Guarded.empty((n, 3), np.float32, dev) if images is not None else None
    ins = [g for g in (g_t, g_ids, g_x, g_y, g_img, g_bk) if g is not None]
    snaps = [g.snapshot() for g in ins]
    p = lambda g: None if g is None else g.ptr
    rc = L.cnc_camera_rays(g_t.ptr, table.shape[0], model, int(opengl), p(g_ids), p(g_x), p(g_y), cam0, width, height, n,
                           EPS, ITERS, p(g_img), p(g_bk), o.ptr, d.ptr, p(pix), _stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert o.intact() and d.intact() and (pix is None or pix.intact())                 # every output inside its allocation
    assert all(g.unchanged_since(s) for g, s in zip(ins, snaps))
    return o.get(), d.get(), (None if pix is None else pix.get())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("model", [T.PINHOLE, T.OPENCV, T.FISHEYE])
def test_rays_of_a_pixel_list(cuda, L, golden, model, n):
    table = _cameras()[model]
    rng = np.random.default_rng(100 + n)
    ids, px, py = rng.integers(0, 3, n), rng.integers(0, W, n), rng.integers(0, H, n)
    images = rng.integers(0, 256, (3, H, W, 4), dtype=np.uint8)
    bkgd = rng.uniform(0, 1, 3).astype(np.float32)
    bound = VIEWDIR_BOUND + _undistortion_bound(table, model, ids, px, py, golden)
    for opengl in (True, False):
        o, d, pix = rays(L, cuda, table, model, opengl, ids, px, py, width=W, height=H, images=images, bkgd=bkgd)
        want_o, want_d = T.camera_rays(table, model, opengl, ids, px, py, EPS, ITERS, np.float64)
        assert same_bits(o, table[ids][:, [7, 11, 15]])                             # the pose's translation column
        err = np.abs(d.astype(np.float64) - want_d).max()
        print(f"rays model {model} opengl {opengl} n {n}: {err / ULP:.2f} x 2^-24 (bound {bound / ULP:.2f})")
        assert np.isfinite(d).all() and err <= bound
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1).max() <= 4 * ULP
        dev_img, t = torch.from_numpy(images).to(cuda), lambda a: torch.from_numpy(np.asarray(a)).to(cuda)
        rgba = dev_img[t(ids), t(py), t(px)].to(torch.float32) / 255.0
        torch_pixels = rgba[:, :3] * rgba[:, 3:] + t(bkgd) * (1.0 - rgba[:, 3:])
        assert np.abs(pix - torch_pixels.cpu().numpy()).max() <= 2.0 ** -23
        # without the fetch: the same rays, and no pixels are touched
        o2, d2, none = rays(L, cuda, table, model, opengl, ids, px, py)
        assert same_bits(o2, o) and same_bits(d2, d) and none is None


@pytest.mark.parametrize("size", [(7, 5), (65, 3)])
@pytest.mark.parametrize("model", [T.PINHOLE, T.OPENCV, T.FISHEYE])
def test_rays_of_a_full_frame(cuda, L, golden, model, size):
    """Width no multiple of a wave: a row-major slip would show."""
    w, h = size
    table = _cameras()[model].copy()
    table[:, 2], table[:, 3] = w / 2.0 + 0.25, h / 2.0 - 0.25
    table[:, :2] *= w / 65.0 if w < 65 else 1.0
    rng = np.random.default_rng(7 * w + h)
    images = rng.integers(0, 256, (3, h, w, 4), dtype=np.uint8)
    bkgd = np.ones(3, np.float32)
    px, py = T.frame_pixels(w, h)
    for cam0 in (0, 2):
        ids = np.full(w * h, cam0)
        bound = VIEWDIR_BOUND + _undistortion_bound(table, model, ids, px, py, golden)
        for opengl in (True, False):
            o, d, pix = rays(L, cuda, table, model, opengl, cam0=cam0, width=w, height=h, images=images, bkgd=bkgd)
            want_o, want_d = T.camera_rays(table, model, opengl, ids, px, py, EPS, ITERS, np.float64)
            assert same_bits(o, want_o.astype(np.float32))
            assert np.abs(d.astype(np.float64) - want_d).max() <= bound
            assert np.abs(pix - T.blend(images[cam0].reshape(-1, 4), bkgd)).max() <= 2.0 ** -23
            # the list form on the same pixels gives the same bits
            o2, d2, pix2 = rays(L, cuda, table, model, opengl, ids, px, py, width=w, height=h, images=images, bkgd=bkgd)
            assert same_bits(o, o2) and same_bits(d, d2) and same_bits(pix, pix2)


def test_rays_are_the_float32_twins_bits(cuda, L):
    """Pinhole and OpenCV models: NumPy float32 in the kernel's operation order gives the kernel's bits."""
    rng = np.random.default_rng(5)
    n = 4099
    ids, px, py = rng.integers(0, 3, n), rng.integers(0, W, n), rng.integers(0, H, n)
    for model in (T.PINHOLE, T.OPENCV):
        table = _cameras()[model]
        for opengl in (True, False):
            o, d, _ = rays(L, cuda, table, model, opengl, ids, px, py)
            want_o, want_d = T.camera_rays(table, model, opengl, ids, px, py, EPS, ITERS, np.float32)
            assert same_bits(o, want_o) and same_bits(d, want_d)


def test_dropin_cameras_on_device_tensors(cuda, golden):
    """`from nerfacc.cameras import opencv_lens_undistortion` after install_dropins(): the backend's values."""
    import cnc_amd
    cnc_amd.install_dropins()
    from nerfacc.cameras import opencv_lens_undistortion, opencv_lens_undistortion_fisheye
    from cnc_amd.backends import nerfacc_cuda as nc
    host_uv = take(golden["uv_2"], 4099)
    uv = torch.from_numpy(host_uv).to(cuda)
    for n_coeffs in (1, 2, 4, 8):
        p = torch.from_numpy(golden["params_3"][:n_coeffs].copy()).to(cuda)
        padded = torch.cat([p, torch.zeros(8 - n_coeffs, device=cuda)])
        got = opencv_lens_undistortion(uv, p)
        assert same_bits(got, nc.opencv_lens_undistortion(uv, padded.expand(4099, 8).contiguous(), EPS, ITERS))
        assert same_bits(got, T.undistort_newton(host_uv, padded.cpu().numpy(), EPS, ITERS, np.float32))
    k = torch.tensor(FISH[0], device=cuda)
    fuv = torch.from_numpy(take(golden["fish_uv_0"], 4099)).to(cuda)
    assert same_bits(opencv_lens_undistortion_fisheye(fuv, k), nc.opencv_lens_undistortion_fisheye(fuv, k.expand(4099, 4), EPS, ITERS))
