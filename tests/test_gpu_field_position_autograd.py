"""GPU: `field(x.requires_grad_(), d)` — the fused training path's position gradient through autograd
(`_FieldTrain.backward` -> cnc_field_position_grad), on two small models of tests/field_lattice.py.

Reference: the analytic float64 gradient with the view directions held fixed.  The first layer's input rows come from
the CPU oracle's encoder (`field_lattice.reference_features`), both networks run forward and backward in float64 NumPy
(the arithmetic of tests/test_gpu_field_chain.py's `_float64_field`, here also handing out the gradient of the
raw-coordinate and sinusoid columns), and (dX, dS) go through the float64 twin of the kernel (tests/pose_twin.py, held to
central differences by tests/test_pose_twin.py).  Bound: 3e-4 of the tensor's largest entry, the lattice's bound for
table gradients; samples within KINK_MARGIN of a ReLU kink carry no loss weight, as in tests/test_gpu_field_lattice.py.
Rows outside the box are exactly zero on both sides (the kernel's contract: selector 0 -> 0).

Measured on the MI355X: 3.4e-7 (f2_h64_5x3d_5x2d) and 9.8e-7 (f8_h160_5x3d_3x2d) of the largest entry."""
import numpy as np
import pytest
import torch

import field_lattice as fl
import pose_twin as P
from test_gpu_field_chain import _sh4_f64
from test_gpu_field_fused import AABB, _field, _inputs
from test_gpu_field_lattice import KINK_MARGIN, _near_a_kink

pytestmark = pytest.mark.gpu
MODELS = ["f2_h64_5x3d_5x2d", "f8_h160_5x3d_3x2d"]
N = 1021
_CASES = {}


def _input_gradients64(f, feats, xu, dirs, wr, wd):
    """(dX [N, n_enc], dS [N, 63]) of sum(rgb * wr) + sum(density * wd) in float64: ngp.py:506-566 forward and backward on
    the given first-layer input rows, down to the gradient of the rows themselves."""
    mb, mh = f.mlp_base.network, f.mlp_head
    W1, b1, W2, b2, W3, b3, W4, b4, W5, b5 = (t.detach().cpu().numpy().astype(np.float64) for t in
                                              (mb[0].weight, mb[0].bias, mb[2].weight, mb[2].bias, mh[0].weight, mh[0].bias,
                                               mh[2].weight, mh[2].bias, mh[4].weight, mh[4].bias))
    X = feats[:, :W1.shape[1]].astype(np.float64)
    sel = np.all((xu > 0) & (xu < 1), axis=1).astype(np.float64)
    h1 = np.maximum(X @ W1.T + b1, 0.0)
    o2 = h1 @ W2.T + b2
    raw = o2[:, 0]
    d32 = ((dirs.astype(np.float32) + np.float32(1.0)) / np.float32(2.0)) * np.float32(2.0) - np.float32(1.0)
    hin = np.concatenate([_sh4_f64(d32.astype(np.float64)), o2[:, 1:]], axis=1)
    h3 = np.maximum(hin @ W3.T + b3, 0.0)
    h4 = np.maximum(h3 @ W4.T + b4, 0.0)
    rgb = 1.0 / (1.0 + np.exp(-(h4 @ W5.T + b5)))
    g5 = wr * rgb * (1.0 - rgb)
    g4 = (g5 @ W5) * (h4 > 0)
    g3 = (g4 @ W4) * (h3 > 0)
    ghin = g3 @ W3
    g2 = np.concatenate([(wd[:, 0] * sel * np.exp(np.minimum(raw - 1.0, 15.0)))[:, None], ghin[:, 16:]], axis=1)
    g1 = (g2 @ W2) * (h1 > 0)
    gX = g1 @ W1
    n_enc = sum(e.n_output_dims for e in f.mlp_base._encoders())
    return gX[:, :n_enc], gX[:, n_enc:n_enc + 63]


class _Case:
    def __init__(self, cuda, oracle, name):
        e = fl.BY_NAME[name]
        seed = 300 + MODELS.index(name)
        f = self.f = _field(cuda, fl.kwargs_of(e), seed=seed, sh_fp16_round=False)
        x, d = _inputs(cuda, N, seed=seed + 1)
        on_edges = torch.from_numpy(fl.boundary_points(e)).to(cuda)
        x[8:8 + on_edges.shape[0]] = on_edges
        self.x, self.d = x, d
        xu = ((x - f.aabb[:3]) / (f.aabb[3:] - f.aabb[:3])).cpu().numpy().astype(np.float32)
        self.sel = np.all((xu > 0) & (xu < 1), axis=1)
        params = fl.field_params(f)
        ref = fl.reference_features(params, xu, oracle)
        g = torch.Generator(device=cuda).manual_seed(9)
        scale = torch.exp(torch.randn(N, 1, device=cuda, generator=g) * 3.0 - 6.0)
        wr = torch.randn(N, 3, device=cuda, generator=g) * scale
        wd = torch.randn(N, 1, device=cuda, generator=g) * scale * 0.1
        near = _near_a_kink(f, ref, d.cpu().numpy())
        assert KINK_MARGIN == 1e-5 and float(near.mean()) < 0.05
        keep = torch.from_numpy(~near).to(cuda)[:, None]
        self.wr, self.wd = wr * keep, wd * keep
        dX, dS = _input_gradients64(f, ref, xu, d.cpu().numpy(), self.wr.cpu().numpy().astype(np.float64),
                                    self.wd.cpu().numpy().astype(np.float64))
        self.want, _ = P.position_grad(params, AABB, x.cpu().numpy(), self.sel.astype(np.uint8), dX, dS)


def _case(cuda, oracle, name):
    if name not in _CASES:
        _CASES[name] = _Case(cuda, oracle, name)
    c = _CASES[name]
    f = c.f
    f.fused_field, f.fused_field_precision, f.fused_field_waves = True, "f16x3", 0
    f.fused_chain = f.fused_train = True
    f._chain_supported = None
    return c


def _backward(c, x):
    f = c.f
    for p in f.parameters():
        p.grad = None
    rgb, den = f(x, c.d)
    ((rgb * c.wr).sum() + (den * c.wd).sum()).backward()
    return {n: p.grad.clone() for n, p in f.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("name", MODELS)
def test_position_gradient_against_the_analytic_float64_gradient(cuda, oracle, name):
    c = _case(cuda, oracle, name)
    x = c.x.clone().requires_grad_(True)
    grads = _backward(c, x)
    assert c.f._field_fused and c.f._field_fused._train_calls, "the fused training forward did not run"
    assert len(grads) == 14 and x.grad is not None and x.grad.shape == x.shape
    got = x.grad.cpu().numpy().astype(np.float64)
    assert np.all(got[~c.sel] == 0) and np.all(c.want[~c.sel] == 0) and 0.05 < (~c.sel).mean() < 0.95
    big = float(np.abs(c.want).max())
    err = float(np.abs(got - c.want).max())
    print(f"POSITION AUTOGRAD {name}: |error| {err:.3e} = {err / big:.3e} of the largest entry {big:.3e}")
    assert big > 0 and err <= 3e-4 * big, (name, err, big)
    assert not c.f.check_range_guard()


@pytest.mark.parametrize("name", MODELS)
def test_parameter_gradients_do_not_depend_on_whether_positions_require_grad(cuda, oracle, name):
    """Bit for bit, in the reproducible mode (the tables' default scatter adds with float atomics, whose order differs from
    run to run whatever the positions do)."""
    from cnc_amd import _repro
    c = _case(cuda, oracle, name)
    with _repro.reproducible(True):
        plain = _backward(c, c.x)
        x = c.x.clone().requires_grad_(True)
        with_x = _backward(c, x)
        again = _backward(c, c.x.clone().requires_grad_(True))
    assert set(plain) == set(with_x) and len(plain) == 14 and x.grad is not None
    for k in plain:
        assert torch.equal(plain[k], with_x[k]), k
        assert torch.equal(with_x[k], again[k]), k


def test_paths_without_position_gradients_raise(cuda, oracle):
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    c = _case(cuda, oracle, MODELS[0])
    f = c.f
    x = c.x[:64].clone().requires_grad_(True)
    d = c.d[:64]
    with pytest.raises(ValueError, match="view direction"):
        f(x, d.clone().requires_grad_(True))
    f.fused_train = False                                   # what the range guard's fallback leaves: the library forward
    with pytest.raises(RuntimeError, match="position gradients"):
        f(x, d)
    f.fused_train, f.fused_chain = True, False
    with pytest.raises(RuntimeError, match="position gradients"):
        f(x, d)
    f.fused_chain = True
    with torch.no_grad():
        f(x, d)                                             # no gradient wanted: nothing to refuse
    unb = NGPRadianceField_mygrid_2D3D(aabb=AABB, unbounded=True, **fl.kwargs_of(fl.BY_NAME[MODELS[0]])).to(cuda)
    with pytest.raises(ValueError, match="bounded"):
        unb(x, d)
    # a shape the gradient chain is not built for (196 encoder columns): raises as well
    e = next(v for v in fl.LATTICE if v.kind == "chain")
    wide = _field(cuda, fl.kwargs_of(e), seed=1)
    with pytest.raises(RuntimeError, match="position gradients"):
        wide(x, d)
    rgb, den = wide(x.detach(), d)                          # ... and without the request it runs as before
    assert rgb.shape == (64, 3)
