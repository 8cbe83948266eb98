"""GPU: the exposure-compensation kernels (csrc/exposure.hip) through the C ABI, every operand inside a
sentinel-filled allocation (tests/guarded.py), against the NumPy twin tests/exposure_twin.py: the gain table within one
float32 step (a double exp may differ in its last bit between libraries), everything else bit for bit given the
kernel's own table, the camera gradient also within the twin's derived bound of float64 — and the autograd.Function
against float64 autograd of the definition, and the argument checks."""
import numpy as np
import pytest
import torch

import exposure_twin as T
from guarded import FILL, Guarded, holds_fill, same_bits

pytestmark = pytest.mark.gpu
FORMS = [("none", True), ("b3", True), ("b3", False), ("bn", True), ("bn", False)]


@pytest.fixture(scope="module")
def libs(cuda):
    from cnc_amd import _lib
    return _lib, _lib.lib(), cuda


def _gains(libs, e):
    _lib, L, dev = libs
    C = e.shape[0]
    ge, gg = Guarded(e, dev), Guarded.empty((C, 3), np.float32, dev)
    _lib.check(L.cnc_exposure_gains(ge.ptr, C, gg.ptr, _lib.stream(dev)), "exposure_gains")
    torch.cuda.synchronize()
    assert ge.intact() and gg.intact() and same_bits(ge.get(), e)
    return gg.get()


def _bkgd(kind, b3, bn):
    return None if kind == "none" else b3 if kind == "b3" else bn


def _forward(libs, c, a, b, ids, g, gain_background):
    _lib, L, dev = libs
    n, C = c.shape[0], g.shape[0]
    ins = [Guarded(x, dev) for x in (c, a, ids, g)] + ([Guarded(b, dev)] if b is not None else [])
    gc, ga, gi, gg = ins[:4]
    out = Guarded.empty((n, 3), np.float32, dev)
    _lib.check(L.cnc_exposure_forward(gc.ptr, ga.ptr, ins[4].ptr if b is not None else None, int(b is not None and b.ndim == 2),
                                      int(gain_background), gi.ptr, gg.ptr, C, n, out.ptr, _lib.stream(dev)), "exposure_forward")
    torch.cuda.synchronize()
    assert all(x.intact() for x in ins) and out.intact()
    return out.get()


def _backward(libs, gp, c, a, b, ids, g, gain_background):
    """-> (g_rgb, g_opacity | None, G_eff, G) as the kernel left them."""
    _lib, L, dev = libs
    n, C = c.shape[0], g.shape[0]
    ins = [Guarded(x, dev) for x in (gp, c, a, ids, g)] + ([Guarded(b, dev)] if b is not None else [])
    ggp, gc, ga, gi, gg = ins[:5]
    nbytes = int(L.cnc_exposure_backward_workspace(n, C))
    assert nbytes == 4 * (((n + 255) // 256) * C * 3 + C * 3)
    ws = Guarded.empty((max(nbytes // 4, 1),), np.float32, dev)
    outs = {"g_rgb": Guarded.empty((n, 3), np.float32, dev), "g_opacity": Guarded.empty((n,), np.float32, dev),
            "G_eff": Guarded.empty((C, 3), np.float32, dev), "G": Guarded.empty((C, 3), np.float32, dev)}
    _lib.check(L.cnc_exposure_backward(ggp.ptr, gc.ptr, ga.ptr, ins[5].ptr if b is not None else None,
                                       int(b is not None and b.ndim == 2), int(gain_background), gi.ptr, gg.ptr, C, n, ws.ptr,
                                       nbytes, outs["g_rgb"].ptr, outs["g_opacity"].ptr, outs["G_eff"].ptr, outs["G"].ptr,
                                       _lib.stream(dev)), "exposure_backward")
    torch.cuda.synchronize()
    assert all(x.intact() for x in ins) and ws.intact() and all(x.intact() for x in outs.values())
    g_op = outs["g_opacity"].get()
    if b is None:                                   # not written without a background
        assert holds_fill(g_op, FILL)
        g_op = None
    return outs["g_rgb"].get(), g_op, outs["G_eff"].get(), outs["G"].get()


# ----------------------------------------------------------------------------------------------------------- gain table
@pytest.mark.parametrize("C", [1, 2, 7, 64, 65, 300])
def test_gain_table(libs, C):
    e = T.cases(1, C, seed=C)[0]
    got = _gains(libs, e)
    assert np.all(T.ulp_distance(got, T.gains(e)) <= 1), T.ulp_distance(got, T.gains(e)).max()
    for const in T.CONSTANTS:                       # e = 0 and e constant over the cameras: exactly 1
        assert same_bits(_gains(libs, np.full((C, 3), const, np.float32)), np.ones((C, 3), np.float32)), const


# ------------------------------------------------------------------------------------------ forward and the ray gradients
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_forward_and_ray_gradients_are_the_twins(libs, n):
    C = 7
    e, c, a, b3, bn, ids, gp = T.cases(n, C, seed=100 + n, ids="outside")
    g = _gains(libs, e)
    for kind, gain_background in FORMS:
        b = _bkgd(kind, b3, bn)
        what = (n, kind, gain_background)
        assert same_bits(_forward(libs, c, a, b, ids, g, gain_background), T.forward(c, a, b, ids, g, gain_background)), what
        g_rgb, g_op, G_eff, G = _backward(libs, gp, c, a, b, ids, g, gain_background)
        if n == 0:                                  # the ray outputs are not touched; the cameras get +0
            assert not G_eff.view(np.uint32).any() and not G.view(np.uint32).any()
            continue
        w_rgb, w_op, w_eff, w_G = T.backward(gp, c, a, b, ids, g, gain_background)
        assert same_bits(g_rgb, w_rgb), what
        assert (g_op is None and w_op is None) or same_bits(g_op, w_op), what
        assert same_bits(G_eff, w_eff) and same_bits(G, w_G), what


@pytest.fixture(scope="module")
def training_size(libs):
    """n = 37,000 rays of C = 100 cameras: the inputs, the kernel's table and the twin's float64 results, made once."""
    e, c, a, b3, bn, ids, gp = T.cases(37000, 100, seed=9)
    return e, c, a, b3, bn, ids, gp, _gains(libs, e)


@pytest.mark.parametrize("kind,gain_background", [("b3", True), ("bn", False)])
def test_training_size(libs, training_size, kind, gain_background):
    e, c, a, b3, bn, ids, gp, g = training_size
    b = _bkgd(kind, b3, bn)
    assert same_bits(_forward(libs, c, a, b, ids, g, gain_background), T.forward(c, a, b, ids, g, gain_background))
    got = _backward(libs, gp, c, a, b, ids, g, gain_background)
    want = T.backward(gp, c, a, b, ids, g, gain_background)
    for x, y, name in zip(got, want, ("g_rgb", "g_opacity", "G_eff", "G")):
        assert same_bits(x, y), name
    w64 = T.backward(gp, c, a, b, ids, g, gain_background, np.float64)
    b_eff, b_G = T.camera_bounds(gp, c, a, b, ids, g, gain_background)
    assert np.all(np.abs(got[2] - w64[2]) <= b_eff) and np.all(np.abs(got[3] - w64[3]) <= b_G)


# ---------------------------------------------------------------------------------------------------- the camera gradient
@pytest.mark.parametrize("C", [5, 64, 65, 300])
@pytest.mark.parametrize("pattern", ["one", "per_chunk", "random", "sparse", "outside"])
def test_camera_gradient_in_its_fixed_order(libs, C, pattern):
    n = 1500                                        # six chunks, the last one short
    e, c, a, b3, bn, ids, gp = T.cases(n, C, seed=C, ids=pattern)
    g = _gains(libs, e)
    for b, gain_background in ((bn, True), (b3, False)):
        first = _backward(libs, gp, c, a, b, ids, g, gain_background)
        again = _backward(libs, gp, c, a, b, ids, g, gain_background)
        want = T.backward(gp, c, a, b, ids, g, gain_background)
        assert same_bits(first[2], want[2]) and same_bits(first[3], want[3])
        assert same_bits(first[2], again[2]) and same_bits(first[3], again[3])           # two runs: equal bits
        w64 = T.backward(gp, c, a, b, ids, g, gain_background, np.float64)
        b_eff, b_G = T.camera_bounds(gp, c, a, b, ids, g, gain_background)
        assert np.all(np.abs(first[2] - w64[2]) <= b_eff) and np.all(np.abs(first[3] - w64[3]) <= b_G)
        unseen = np.setdiff1d(np.arange(C), T.clamp_ids(ids, C))
        if pattern in ("one", "sparse") or (pattern == "per_chunk" and C > 6):
            assert unseen.size
        assert not first[2][unseen].view(np.uint32).any()      # a camera without rays: the bits of +0


# ------------------------------------------------------------------------------------------------- autograd and validation
def _definition(e, c, a, b, ids, gain_background):
    C = e.shape[0]
    g = torch.exp(e - e.sum(dim=0) / C)[ids.clamp(0, C - 1)]
    if b is None:
        return g * c
    behind = (1.0 - a)[:, None] * b
    return g * (c + behind) if gain_background else g * c + behind


@pytest.mark.parametrize("kind,gain_background", FORMS)
def test_autograd_function_against_float64(cuda, kind, gain_background):
    from cnc_amd.exposure import ExposureCompensation
    n, C = 700, 9
    e, c, a, b3, bn, ids, gp = T.cases(n, C, seed=21, ids="outside")
    b = _bkgd(kind, b3, bn)
    ex = ExposureCompensation(C, cuda)
    with torch.no_grad():
        ex.log_gain.copy_(torch.from_numpy(e))
    tc = torch.tensor(c, device=cuda, requires_grad=True)
    ta = torch.tensor(a, device=cuda, requires_grad=True)
    tid = torch.from_numpy(ids).to(cuda)
    p = ex(tc, tid, opacity=ta[:, None], bkgd=None if b is None else torch.from_numpy(b).to(cuda), gain_background=gain_background)
    assert p.shape == tc.shape
    p.backward(torch.from_numpy(gp).to(cuda))
    de, dc, da = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (e, c, a))
    q = _definition(de, dc, da, None if b is None else torch.tensor(b, dtype=torch.float64), torch.from_numpy(ids), gain_background)
    q.backward(torch.tensor(gp, dtype=torch.float64))
    g = ex.gains().cpu().numpy()
    assert np.all(np.abs(g - T.gains(e, np.float64)) <= T.gains_bound(e))
    # the table's own error reaches every output once: (1 + rel) on top of the bounds given the table
    rel = float((T.gains_bound(e) / T.gains(e, np.float64)).max()) * 1.01
    pb = T.forward_bound(c, a, b, ids, g, gain_background) + rel * np.abs(q.detach().numpy())
    assert np.all(np.abs(p.detach().cpu().numpy() - q.detach().numpy()) <= pb)
    b_rgb, b_op, _ = T.ray_bounds(gp, c, a, b, ids, g, gain_background)
    assert np.all(np.abs(tc.grad.cpu().numpy() - dc.grad.numpy()) <= b_rgb + rel * np.abs(dc.grad.numpy()))
    if b is None:
        assert ta.grad is None and da.grad is None
    else:
        assert np.all(np.abs(ta.grad.cpu().numpy() - da.grad.numpy()) <= b_op + rel * np.abs(da.grad.numpy()) + 1e-12)
    _, b_G = T.camera_bounds(gp, c, a, b, ids, g, gain_background)
    absq = T.fold(np.abs(T.backward_rays(gp, c, a, b, ids, g, gain_background, np.float64)[2]), ids, C, np.float64)
    slack = rel * (absq + absq.mean(axis=0))
    assert np.all(np.abs(ex.log_gain.grad.cpu().numpy() - de.grad.numpy()) <= b_G + slack)
    # what the Trainer's Adam descends along: the same before the centring's transpose
    eff = ex.effective_grad.cpu().numpy()
    assert np.allclose(eff - eff.mean(axis=0), ex.log_gain.grad.cpu().numpy(), rtol=1e-4, atol=1e-5)


def test_arguments_are_checked(cuda):
    from cnc_amd.backends import exposure_backend as K
    n, C = 10, 3
    rgb = torch.rand(n, 3, device=cuda)
    ids = torch.zeros(n, dtype=torch.int64, device=cuda)
    gains = K.exposure_gains(torch.zeros(C, 3, device=cuda))
    op, b3 = torch.rand(n, device=cuda), torch.rand(3, device=cuda)
    assert K.exposure_forward(rgb, ids, gains, op, b3).shape == (n, 3)
    bad = [dict(rgb=rgb.double()), dict(rgb=rgb[:, :2].contiguous()), dict(rgb=torch.rand(3, n, device=cuda).t()),
           dict(rgb=rgb.cpu()), dict(ids=ids.int()), dict(ids=ids[:5]), dict(ids=ids.cpu()), dict(gains=gains.double()),
           dict(gains=gains[:, :2].contiguous()), dict(gains=gains.cpu()), dict(op=op.double()), dict(op=op[:, None]),
           dict(op=torch.rand(2 * n, device=cuda)[::2]), dict(op=op.cpu()), dict(op=None), dict(b=b3.double()),
           dict(b=torch.rand(4, device=cuda)), dict(b=torch.rand(n + 1, 3, device=cuda)), dict(b=b3.cpu())]
    for kw in bad:
        args = dict(rgb=rgb, ids=ids, gains=gains, op=op, b=b3)
        args.update(kw)
        with pytest.raises(RuntimeError):
            K.exposure_forward(args["rgb"], args["ids"], args["gains"], args["op"], args["b"])
        with pytest.raises(RuntimeError):
            K.exposure_backward(torch.ones(n, 3, device=cuda), args["rgb"], args["ids"], args["gains"], args["op"], args["b"])
    for g_out in (torch.ones(n, 3, device=cuda).double(), torch.ones(n, 2, device=cuda), torch.ones(n, 3)):
        with pytest.raises(RuntimeError):
            K.exposure_backward(g_out, rgb, ids, gains, op, b3)
    for e in (torch.zeros(C, 3, device=cuda).double(), torch.zeros(C, 2, device=cuda), torch.zeros(3, C, device=cuda).t(),
              torch.zeros(C, 3)):
        with pytest.raises(RuntimeError):
            K.exposure_gains(e)


def test_the_c_abi_refuses_and_ignores(libs):
    _lib, L, dev = libs
    s = _lib.stream(dev)
    assert L.cnc_exposure_gains(None, 0, None, s) == 0 and L.cnc_exposure_gains(None, 3, None, s) != 0
    assert L.cnc_exposure_gains(None, -1, None, s) != 0
    assert L.cnc_exposure_forward(None, None, None, 0, 1, None, None, 3, 0, None, s) == 0
    assert L.cnc_exposure_forward(None, None, None, 0, 1, None, None, 0, 5, None, s) == 0
    assert L.cnc_exposure_forward(None, None, None, 0, 1, None, None, 3, 5, None, s) != 0
    assert L.cnc_exposure_forward(None, None, None, 0, 1, None, None, 3, -1, None, s) != 0
    assert L.cnc_exposure_backward(None, None, None, None, 0, 1, None, None, 0, 5, None, 0, None, None, None, None, s) == 0
    assert L.cnc_exposure_backward(None, None, None, None, 0, 1, None, None, 3, 5, None, 0, None, None, None, None, s) != 0
    assert L.cnc_exposure_backward_workspace(0, 3) == 36 and L.cnc_exposure_backward_workspace(5, 0) == 0
    # a background without the opacity, and a workspace one byte short
    t = torch.zeros(5, 3, device=dev)
    ids = torch.zeros(5, dtype=torch.int64, device=dev)
    g = torch.ones(3, 3, device=dev)
    out = torch.zeros(5, 3, device=dev)
    assert L.cnc_exposure_forward(t.data_ptr(), None, t.data_ptr(), 0, 1, ids.data_ptr(), g.data_ptr(), 3, 5, out.data_ptr(), s) != 0
    need = int(L.cnc_exposure_backward_workspace(5, 3))
    ws = torch.zeros(need // 4, device=dev)
    G = torch.zeros(3, 3, device=dev)
    assert L.cnc_exposure_backward(t.data_ptr(), t.data_ptr(), None, None, 0, 1, ids.data_ptr(), g.data_ptr(), 3, 5,
                                   ws.data_ptr(), need - 1, out.data_ptr(), None, None, G.data_ptr(), s) != 0
    assert L.cnc_exposure_backward(t.data_ptr(), t.data_ptr(), None, None, 0, 1, ids.data_ptr(), g.data_ptr(), 3, 5,
                                   ws.data_ptr(), need, out.data_ptr(), None, None, G.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert not bool(G.any()) and bool(torch.isfinite(out).all())
