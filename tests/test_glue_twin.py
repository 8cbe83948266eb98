"""tests/glue_twin.py (the float32 twins tests/test_gpu_field_glue.py holds the field's glue kernels to) checked without
a GPU: the harmonics against their float64 closed forms on unit vectors under a derived bound, and bit for bit against
field.SHEncoding; the selector, the STE expressions and the ReLU mask against the reference's op chains in torch.

The harmonics' bound is a running error analysis of the twin's own operation sequence: every quantity is carried as
(value in float64, bound e on |float32 value - float64 value|), with u = 2^-24 and
    a + b : e = e_a + e_b + u |a + b|            a * b : e = |a| e_b + |b| e_a + e_a e_b + u |a b|
(a float32 constant c differs from its decimal by at most u |c|; * 2 and / 2 are exact), then multiplied by 1 + 2^-20
for the second-order terms the |.| of the float64 values leave out."""
import numpy as np
import pytest
import torch

import glue_twin as G

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


class _E:
    """A float64 value with a bound on the float32 computation's distance from it."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, f64)
        self.e = np.zeros_like(self.v) if e is None else e

    @staticmethod
    def const(c):
        return _E(np.float64(c), np.float64(U * abs(c)))

    def __add__(self, o):
        v = self.v + o.v
        return _E(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        v = self.v - o.v
        return _E(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        v = self.v * o.v
        return _E(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + U * np.abs(v))

    def __neg__(self):
        return _E(-self.v, self.e)


def _sh16_bounds(dirs):
    """The twin's operation sequence over _E: (float64 values, bounds), [N, 16] each."""
    d = np.asarray(dirs, f64)
    one = _E(np.float64(1.0))
    comp = []
    for a in range(3):
        t = _E(d[:, a]) + one                       # (d + 1): one rounding; / 2 and * 2 are exact
        comp.append(t - one)
    x, y, z = comp
    c = [_E.const(float(k)) for k in (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997,
                                      0.31539156525251999, 0.54627421529603959, 0.59004358992664352, 2.8906114426405538,
                                      0.45704579946446572, 0.3731763325901154, 1.4453057213202769)]
    c0, c1, c2, c3, c3b, c4, c5, c6, c7, c8, c9 = c
    three, five = _E(np.float64(3.0)), _E(np.float64(5.0))
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    full = _E(np.full(d.shape[0], c0.v), np.full(d.shape[0], c0.e))
    o = [full, (-c1) * y, c1 * z, (-c1) * x, c2 * xy, (-c2) * yz, c3 * zz - c3b, (-c2) * xz,
         c4 * xx - c4 * yy, (c5 * y) * (((-three) * xx) + yy), (c6 * xy) * z, (c7 * y) * (one - five * zz),
         (c8 * z) * (five * zz - three), (c7 * x) * (one - five * zz), (c9 * z) * (xx - yy), (c5 * x) * ((-xx) + three * yy)]
    return np.stack([t.v for t in o], 1), np.stack([t.e for t in o], 1) * (1.0 + 2.0 ** -20)


def _dirs(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(f32)
    return np.concatenate([d, axes])


def test_harmonics_against_the_float64_closed_form_on_unit_vectors(capsys):
    d = _dirs(20000, 0)
    got = G.sh16(d)
    ref = G.sh16_float64(d.astype(f64))
    v, bound = _sh16_bounds(d)
    assert np.allclose(v, ref, rtol=0, atol=1e-14)          # the analysis walks the same polynomials
    err = np.abs(got.astype(f64) - ref)
    r = float((err / (bound + 1e-14)).max())
    with capsys.disabled():
        print(f"\nglue twin, harmonics: largest |twin - float64| / bound {r:.3g}; largest bound {bound.max() / U:.3g} u")
    assert r <= 1.0
    assert bound.max() <= 64 * U                              # a rounding bound: a few u per operation, values <= 3


def test_harmonics_are_orthonormal_on_the_sphere():
    """The closed forms the twin is held to are the real spherical harmonics: 4 pi times their Gram matrix over the sphere
    is the identity, here by Monte Carlo over 2^18 uniform directions (standard error ~ 1 / 512 per entry times the
    harmonics' 4th moments, below 2: 0.02 leaves 5 sigma)."""
    rng = np.random.default_rng(1)
    d = rng.normal(size=(1 << 18, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y = G.sh16_float64(d)
    gram = 4.0 * np.pi * (Y.T @ Y) / d.shape[0]
    assert np.abs(gram - np.eye(16)).max() <= 0.02


@pytest.mark.parametrize("fp16", [False, True])
def test_harmonics_equal_the_module(fp16):
    from cnc_amd.field import SHEncoding
    d = np.concatenate([_dirs(5000, 2), np.zeros((1, 3), f32), (np.random.default_rng(3).normal(size=(500, 3)) * 2).astype(f32)])
    d01 = (torch.tensor(d) + 1.0) / 2.0
    want = SHEncoding(fp16_round=fp16)(d01).numpy()
    got = G.sh16(d, fp16)
    assert got.dtype == want.dtype == f32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if fp16:
        assert np.array_equal(got, got.astype(np.float16).astype(f32)) and not np.array_equal(got, G.sh16(d, False))


def test_prepare_and_selector_equal_the_op_chain():
    aabb = np.array([-1.5, -1.0, -0.5, 1.5, 2.0, 0.75], f32)
    rng = np.random.default_rng(4)
    pos = rng.uniform(-2, 2.5, size=(4000, 3)).astype(f32)
    pos[0] = aabb[:3]
    pos[1] = aabb[3:]
    pos[2] = np.nextafter(aabb[:3], aabb[3:])
    pos[3] = [np.nan, 0, 0]
    x, sel = G.prepare(pos, aabb)
    t, a = torch.tensor(pos), torch.tensor(aabb)
    tx = (t - a[:3]) / (a[3:] - a[:3])
    ts = ((tx > 0) & (tx < 1)).all(-1)
    assert np.array_equal(x.view(np.uint32), tx.numpy().view(np.uint32)) and np.array_equal(sel, ts.numpy().astype(np.uint8))
    assert sel[:4].tolist() == [0, 0, 1, 0] and 0.05 < sel.mean() < 0.9


def _specials():
    one = f32(1)
    return np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, f32(2)), np.nextafter(one, f32(0)), np.nextafter(-one, f32(-2)),
                     np.nextafter(-one, f32(0)), np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.3, -0.7, 5.0], f32)


def test_ste_and_relu_expressions_equal_the_op_chains():
    x = _specials()
    t = torch.tensor(x)
    c = torch.clamp(t, -1, 1)
    fwd = (c >= 0) * 1.0 + (c < 0) * -1.0
    assert np.array_equal(G.ste_forward(x).view(np.uint32), fwd.float().numpy().view(np.uint32))
    g = np.linspace(-2, 2, x.size).astype(f32)
    bwd = torch.tensor(g) * ((t >= -1) & (t <= 1))
    assert np.array_equal(G.ste_backward(x, g).view(np.uint32), bwd.numpy().view(np.uint32))
    # y > 0 ? g : 0.  aten::threshold_backward is `y <= 0 ? 0 : g` and lets g through where y is NaN; a ReLU output is
    # never NaN unless the step is already lost, and the kernel's documented expression is the one held here
    relu = torch.where(t > 0, torch.tensor(g), torch.zeros(()))
    assert np.array_equal(G.relu_backward(g, x).view(np.uint32), relu.numpy().view(np.uint32))
    lib = torch.ops.aten.threshold_backward(torch.tensor(g), t, 0.0).numpy()
    ok = ~np.isnan(x)
    assert np.array_equal(G.relu_backward(g, x)[ok].view(np.uint32), lib[ok].view(np.uint32))


def test_sinusoid_layout_and_arguments():
    x = np.array([[0.25, -0.0, 1.0], [0.1, 0.7, 1.2]], f32)
    freqs = (2.0 ** np.arange(3)).astype(f32)
    out, exact = G.sinusoid(x, freqs, 24)
    assert exact.tolist() == [True] * 3 + [False] * 18 + [True] * 3
    assert np.array_equal(out[:, :3], x.astype(f64)) and np.all(out[:, 21:] == 0)
    arg = G.sinusoid_arguments(x, freqs)
    assert arg.dtype == f32 and arg[1, 2, 1] == f32(0.7) * f32(4)
    assert out[1, 3 + 6 * 2 + 1] == np.sin(f64(arg[1, 2, 1])) and out[1, 3 + 6 * 2 + 3 + 1] == np.cos(f64(arg[1, 2, 1]))
