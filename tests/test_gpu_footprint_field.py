"""Footprint of the field kernels: every result depends on the caller's buffers alone.  Inputs lie in guarded allocations
(tests/guarded.py) whose surroundings — and the pad columns of a matrix with ld > the columns in use — hold 0x00, 0xA5
and 0xFF in turn.

  * cnc_field_weight_grads (field_wgrad.hip): G and A are read through buffer resources of N * ld * 4 bytes; rows past N
    read "beyond the records", columns [nO, roundup4(nO)) of G and the pad columns of A "are readable (zero or not: they
    are dropped)".  Here those columns hold the fill — at the two shapes of that test they are column 3 of G_4 (the
    colour gradient, 3 of 4) and the last 5 columns of A_0 (K0 of ldf); ld2 and ldh have no pad there — and dW is the same
    bits under every fill and within
    `test_weight_gradient_kernel_against_float64`'s bound of the float64 product.
  * cnc_field_fused_forward through `FusedFieldForward` (bounded and contracted) on guarded [N, 3] positions and
    directions (12-byte rows): the same bits under every fill; within test_gpu_field_fused.py's bound of the chain
    (bounded), the bits of the bounded field on the twin's coordinates (contracted, test_gpu_field_unbounded.py).
  * cnc_field_backward_chain through `_FieldChain` with guarded upstream gradients: the encoders' tables are summed with
    atomics, so each fill on its own is finite and within test_gpu_field_chain.py's bound of the layer-by-layer path.

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import FILLS, Guarded, moved_with_fill, same_bits, under_fills
from test_gpu_field_chain import CHAIN_REL, WGRAD_REL, wgrad_case, wgrad_reference
from test_gpu_field_fused import CONFIGS, FUSED_TOL, _close, _field, _inputs

pytestmark = pytest.mark.gpu
f32 = np.float32
MODELS = ["f2_toy", "f4_h64"]
_FIELDS = {}


def _model(cuda, cfg):
    if cfg not in _FIELDS:
        _FIELDS[cfg] = _field(cuda, CONFIGS[cfg], seed=3)
    f = _FIELDS[cfg]
    f.fused_field, f.fused_train, f.fused_chain, f._chain_supported = True, False, True, None
    f.zero_grad(set_to_none=True)
    return f


# ----------------------------------------------------------------------------------------------------------------------
# cnc_field_weight_grads
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_workgroups", [0, 7])
@pytest.mark.parametrize("n", [1, 63, 129])
@pytest.mark.parametrize("shape", ["f8_full", "h64"])
def test_weight_grads_drop_the_pad_columns(cuda, shape, n, n_workgroups):
    from cnc_amd import _lib
    Gs, As, n_out, n_in, gmax, geo = wgrad_case(cuda, shape, n)
    # the columns the product uses: G's [0, n_out); A's [0, n_in) and, for head.0, the raw-density slot in front of geo
    used_a = [n_in[l] + (1 if l == 2 else 0) for l in range(5)]
    hG = [G[:, :o].cpu().numpy() for G, o in zip(Gs, n_out)]
    hA = [A[:, :u].cpu().numpy() for A, u in zip(As, used_a)]
    ldG, ldA = [G.shape[1] for G in Gs], [A.shape[1] for A in As]
    # which matrices carry pad columns at these shapes: G_4 (3 of 4 columns) and A_0 (K0 of ldf: 251 / 256, 91 / 96).  ld2 =
    # roundup4(1 + geo) and ldh equal the columns in use (80 / 16 and 96 / 32): G_1 and A_2 have no pad to poison
    assert [ld - o for ld, o in zip(ldG, n_out)] == [0, 0, 0, 0, 1]
    assert [ld - u for ld, u in zip(ldA, used_a)] == [5, 0, 0, 0, 0]
    probe = _lib.FieldWGrad()
    probe.N, probe.n_workgroups = n, n_workgroups
    for l in range(5):
        probe.ldG[l], probe.n_out[l], probe.ldA[l], probe.n_in[l] = ldG[l], n_out[l], ldA[l], n_in[l]
    nbytes = ctypes.c_uint64(0)
    _lib.check(_lib.lib().cnc_field_weight_grads_workspace(ctypes.byref(probe), ctypes.byref(nbytes)), "workspace")

    def build(fill):
        b = {"gmax": Guarded(gmax.cpu().numpy(), cuda, fill=fill),
             "ws": Guarded.empty((nbytes.value,), np.uint8, cuda, fill=fill).scratch()}
        for l in range(5):
            b[f"G{l}"] = Guarded.window(hG[l], ldG[l], 0, cuda, fill)
            b[f"A{l}"] = Guarded.window(hA[l], ldA[l], 0, cuda, fill)
            # dW_0 as a column window of a wider matrix, the others dense
            b[f"dW{l}"] = (Guarded.empty_window(n_out[l], n_in[l], n_in[l] + 5, 2, f32, cuda, fill) if l == 0 else
                           Guarded.empty((n_out[l], n_in[l]), f32, cuda, fill=fill))
        return b

    def run(b):
        d = _lib.FieldWGrad()
        d.N, d.head_gap_col, d.g_max, d.n_workgroups = n, 16, b["gmax"].ptr, n_workgroups
        for l in range(5):
            d.G[l], d.ldG[l], d.n_out[l] = b[f"G{l}"].ptr, ldG[l], n_out[l]
            d.A[l], d.ldA[l], d.n_in[l] = b[f"A{l}"].ptr, ldA[l], n_in[l]
            d.dW[l], d.ld_dW[l] = b[f"dW{l}"].ptr, n_in[l] + 5 if l == 0 else n_in[l]
        d.workspace, d.workspace_bytes = b["ws"].ptr, nbytes.value
        _lib.check(_lib.lib().cnc_field_weight_grads(ctypes.byref(d), _lib.stream(cuda)), "field_weight_grads")

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    for l in range(5):
        got = torch.from_numpy(res[FILLS[0]][f"dW{l}"]).to(cuda)
        ref = wgrad_reference(Gs, As, n_out, n_in, geo, l)
        err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
        assert bool(torch.isfinite(got).all()) and err <= WGRAD_REL * scale, (l, err, scale)


# ----------------------------------------------------------------------------------------------------------------------
# cnc_field_fused_forward
# ----------------------------------------------------------------------------------------------------------------------
def _forward_under_fills(cuda, f, x, d):
    """rgb / density (colour kernel) / density (density-only kernel) of guarded positions and directions, per fill."""
    N = x.shape[0]

    def build(fill):
        return {"x": Guarded(x, cuda, fill=fill), "d": Guarded(d, cuda, fill=fill),
                "rgb": Guarded.empty((N, 3), f32, cuda, fill=fill), "sig": Guarded.empty((N, 1), f32, cuda, fill=fill),
                "den": Guarded.empty((N, 1), f32, cuda, fill=fill)}

    def run(b):
        with torch.no_grad():
            rgb, sig = f(b["x"].tensor(), b["d"].tensor())
            den = f.query_density(b["x"].tensor())
        assert f._field_fused, "the fused kernel did not run"
        b["rgb"].tensor().copy_(rgb), b["sig"].tensor().copy_(sig), b["den"].tensor().copy_(den)

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    return {k: torch.from_numpy(v).to(cuda) for k, v in res[FILLS[0]].items()}


@pytest.mark.parametrize("precision", list(FUSED_TOL))
@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("cfg", MODELS)
def test_fused_forward_bounded(cuda, cfg, n, precision):
    f = _model(cuda, cfg)
    f.fused_field_precision = precision
    x, d = _inputs(cuda, n, seed=n)
    got = _forward_under_fills(cuda, f, x.cpu().numpy(), d.cpu().numpy())
    with torch.no_grad():
        f.fused_field = False
        rgb0, sig0 = f(x, d)
        den0 = f.query_density(x)
        f.fused_field = True
    tol = FUSED_TOL[precision]
    _close(got["den"], den0, tol, "density (density-only kernel)")
    _close(got["sig"], sig0, tol, "density (colour kernel)")
    _close(got["rgb"], rgb0, tol, "rgb")
    assert torch.equal(got["den"] == 0, den0 == 0) and torch.equal(got["sig"] == 0, sig0 == 0)
    f.fused_field_precision = "f16x3"


@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("model", ["f2", "f4"])
def test_fused_forward_contracted(cuda, model, n):
    import test_gpu_field_unbounded as TU
    U, V = TU._pair(cuda, model)
    x, xc, d, _ = TU._inputs(cuda, n, seed=200 + n)
    got = _forward_under_fills(cuda, U, x.cpu().numpy(), d.cpu().numpy())
    with torch.no_grad():
        rgb_v, sig_v = V(xc, d)
        den_v = V.query_density(xc)
    assert V._field_fused
    TU._equal(got["rgb"], rgb_v, "rgb"); TU._equal(got["sig"], sig_v, "density (colour kernel)")
    TU._equal(got["den"], den_v, "density")
    assert bool((got["den"] > 0).all()) and bool(torch.isfinite(got["rgb"]).all())


# ----------------------------------------------------------------------------------------------------------------------
# cnc_field_backward_chain
# ----------------------------------------------------------------------------------------------------------------------
def _backward(f, x, d, wr, wd, chain):
    f.fused_chain, f.fused_train, f._chain_supported = chain, False, None
    f.zero_grad(set_to_none=True)
    rgb, den = f(x, d)
    torch.autograd.backward([rgb, den], [wr, wd])
    return rgb.detach(), den.detach(), {k: p.grad.clone() for k, p in f.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("n", [1, 31, 33])
@pytest.mark.parametrize("cfg", MODELS)
def test_backward_chain_with_guarded_gradients(cuda, cfg, n):
    f = _model(cuda, cfg)
    x, d = _inputs(cuda, n, seed=n + 1)
    g = torch.Generator(device=cuda).manual_seed(3)
    scale = torch.exp(torch.randn(n, 1, device=cuda, generator=g) * 3.0 - 6.0)
    wr = torch.randn(n, 3, device=cuda, generator=g) * scale
    wd = torch.randn(n, 1, device=cuda, generator=g) * scale * 0.1
    rgb0, den0, g0 = _backward(f, x, d, wr, wd, chain=False)
    host = {"x": x, "d": d, "wr": wr, "wd": wd}
    host = {k: v.cpu().numpy() for k, v in host.items()}
    grads = {}

    def build(fill):
        b = {k: Guarded(v, cuda, fill=fill) for k, v in host.items()}
        b["rgb"], b["den"] = Guarded.empty((n, 3), f32, cuda, fill=fill), Guarded.empty((n, 1), f32, cuda, fill=fill)
        return b

    def run(b):
        rgb, den, grads[b["x"].fill] = _backward(f, *(b[k].tensor() for k in ("x", "d", "wr", "wd")), chain=True)
        assert f._chain_supported, "the chain did not run"
        b["rgb"].tensor().copy_(rgb), b["den"].tensor().copy_(den)

    res = under_fills(build, run)
    assert moved_with_fill(res) == []                                   # the forward values: no atomics
    assert same_bits(res[FILLS[0]]["rgb"], rgb0.cpu().numpy()) and same_bits(res[FILLS[0]]["den"], den0.cpu().numpy())
    for fill in FILLS:
        g1 = grads[fill]
        assert set(g1) == set(g0) and len(g0) == 14
        for name in g0:
            a, b = g1[name].double(), g0[name].double()
            scale_ = float(b.abs().max())
            assert bool(torch.isfinite(a).all()), (fill, name)
            assert float((a - b).abs().max()) <= CHAIN_REL * max(scale_, 1e-30), (fill, name, float((a - b).abs().max()), scale_)
    f.zero_grad(set_to_none=True)
