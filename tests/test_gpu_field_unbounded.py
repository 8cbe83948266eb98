"""An UNBOUNDED radiance field (`unbounded=True`: contract_to_unisphere, ngp.py:337-361,515-516) on the project's
kernels: cnc_field_prepare_contracted and cnc_field_fused_forward with CNC_FIELD_CONTRACT (include/cnc_hip.h).

The contraction is a per-sample map of the position in front of everything else, so the tests are built on two facts:
  1. the coordinates the kernels compute equal the NumPy twin's (tests/contract_twin.py) BIT FOR BIT — the glue entry
     point and the saving form's xyz / xy / xz / yz / selector;
  2. everything downstream is the bounded kernel: an unbounded field U on positions x returns the bits a bounded field V
     with the box [0, 1]^3 and U's parameters returns on twin(x) — (c - 0) / (1 - 0) = c exactly, so V's kernels see the
     same coordinates.  No tolerance: a mismatch is a bug in where the contraction sits, not rounding.
Against the torch op chain (`fused_unbounded=False`, the route an unbounded field took before) and against the
reference's own numbers (tests/golden/field_unbounded_toy.npz) the project's usual bounds apply: 1e-4 of the tensor's
scale, 2e-5 for the fp16 three-product forward (tests/test_gpu_field_fused.py), 2e-4 for gradients against the
reference (tests/test_gpu_field_golden.py).

Positions: the shared seeded set of contract_twin.points (uniform in 1.2 x an asymmetric box, normal x 10 extents, normal
x 1e4, the exact cases, interleaved so that every 32-sample tile mixes contracted and uncontracted rows).  On it the twin
selects every row (asserted), so selector 0 is exercised by the saving form's rows of padding only (asserted too)."""
import os

import numpy as np
import pytest
import torch

import contract_twin as T
from guarded import Guarded
from test_gpu_field_fused import _close
from test_gpu_field_golden import FIELD_CASES, close, fill_state

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32, u32 = np.float32, np.uint32
MODELS = dict(FIELD_CASES,          # f8 (H 160), f2 (H 64) + an F = 4 model
              f4=dict(n_features_per_level=4, n_neurons=64, resolutions_list=(6, 9, 14, 20, 26), log2_hashmap_size=10,
                      resolutions_list_2D=(10, 18, 34), log2_hashmap_size_2D=9))
N_ROWS = [1, 31, 32, 33, 4101]
UNIT = [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]
_FIELDS = {}


def _pair(cuda, model):
    """(U, V): the unbounded field in the asymmetric box, and a bounded field in [0, 1]^3 with U's parameters (every
    state-dict key except `aabb`).  Built once per model; tests restore the switches they touch."""
    if model not in _FIELDS:
        from cnc_amd.field import NGPRadianceField_mygrid_2D3D
        torch.manual_seed(7)
        U = NGPRadianceField_mygrid_2D3D(aabb=torch.from_numpy(T.BOX.copy()), unbounded=True, **MODELS[model])
        sd = fill_state(U.state_dict(), seed=19)
        sd["mlp_base.network.2.bias"][0] = 1.5          # densities of order one
        U.load_state_dict(sd, strict=True)
        V = NGPRadianceField_mygrid_2D3D(aabb=UNIT, **MODELS[model])
        missing = V.load_state_dict({k: v for k, v in U.state_dict().items() if k != "aabb"}, strict=False)
        assert list(missing.missing_keys) == ["aabb"] and not missing.unexpected_keys
        _FIELDS[model] = (U.to(cuda), V.to(cuda))
    U, V = _FIELDS[model]
    for f in (U, V):
        f.fused_field_precision, f.fused_field_waves, f.fused_unbounded = "f16x3", 0, True
        f.fused_field, f.fused_train = True, True
        f.zero_grad(set_to_none=True)
    assert U.unbounded and not V.unbounded
    return U, V


def _inputs(cuda, n, seed):
    """(positions, their contracted twins, directions) on the device + the twin's selector (NumPy)."""
    p = T.points(n, seed=seed)
    xc, sel = T.contract(p)
    assert sel.all() and float(xc.min()) > 0.0 and float(xc.max()) < 1.0        # the set leaves no coordinate outside (0, 1)
    rng = np.random.default_rng([seed, n, 1])
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    return torch.from_numpy(p).to(cuda), torch.from_numpy(xc).to(cuda), torch.from_numpy(d).to(cuda), sel


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    ok = got.view(np.uint8) == want.view(np.uint8) if got.dtype == np.uint8 else got.view(u32) == want.view(u32)
    if not ok.all():
        i = np.unravel_index(int(np.argmin(ok)), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} differ, first at {i}: got {got[i]!r} want {want[i]!r}")


def _equal(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        bad = (a != b)
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} differ, largest |diff| {float((a.double() - b.double()).abs().max()):.3g}")


# ------------------------------------------------------------------------------------------------------------------
# 1. the coordinates, bit for bit
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", N_ROWS)
def test_prepare_contracted_equals_the_twin(cuda, N):
    from cnc_amd import _lib
    pos = T.points(N, seed=N)
    want_x, want_s = T.contract(pos)
    P, A = Guarded(pos, cuda), Guarded(T.BOX, cuda)
    X, S = Guarded.empty((N, 3), f32, cuda), Guarded.empty((N,), np.uint8, cuda)
    rc = _lib.lib().cnc_field_prepare_contracted(P.ptr, A.ptr, N, X.ptr, S.ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    _same_bits(X.get(), want_x, "x_unit")
    _same_bits(S.get(), want_s, "selector")
    assert want_s.all()
    assert all(b.intact() for b in (P, A, X, S)) and np.array_equal(P.get().view(u32), pos.view(u32))
    # the bounded entry point is the expression it was: (p - min) / (max - min)
    X0, S0 = Guarded.empty((N, 3), f32, cuda), Guarded.empty((N,), np.uint8, cuda)
    assert _lib.lib().cnc_field_prepare(P.ptr, A.ptr, N, X0.ptr, S0.ptr, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    u = (pos - T.BOX[:3]) / (T.BOX[3:] - T.BOX[:3])
    _same_bits(X0.get(), u, "x_unit (bounded)")
    _same_bits(S0.get(), ((u > 0) & (u < 1)).all(1).astype(np.uint8), "selector (bounded)")
    assert X0.intact() and S0.intact()


@pytest.mark.parametrize("N", N_ROWS)
@pytest.mark.parametrize("model", list(MODELS))
def test_saving_form_keeps_the_contracted_coordinates(cuda, model, N):
    """n_live = N, rows = N + 27: xyz / xy / xz / yz / selector of the live rows equal the twin's, the 27 rows of padding
    are a point outside the box (selector 0) — and the route's own glue kernel writes the same bits."""
    U, _ = _pair(cuda, model)
    x, xc, d, sel = _inputs(cuda, N, seed=100 + N)
    with torch.no_grad():
        assert U._fused_forward(x) is not None                      # creates the evaluator
    rgb, density, kept = U._field_fused.save_forward(x, d, N + 27)
    torch.cuda.synchronize()
    want = xc.cpu().numpy()
    assert kept["xyz"].shape == (N + 27, 3) and kept["selector"].shape == (N + 27,)
    _same_bits(kept["xyz"][:N].cpu().numpy(), want, "save.xyz")
    _same_bits(kept["xy"][:N].cpu().numpy(), want[:, [0, 1]], "save.xy")
    _same_bits(kept["xz"][:N].cpu().numpy(), want[:, [0, 2]], "save.xz")
    _same_bits(kept["yz"][:N].cpu().numpy(), want[:, [1, 2]], "save.yz")
    _same_bits(kept["selector"][:N].cpu().numpy(), sel, "save.selector")
    assert sel.all() and not kept["selector"][N:].any()             # selector 0: the rows of padding, and only they
    assert float(density[N:].abs().max()) == 0.0 and bool((density[:N] > 0).all())
    assert bool(torch.isfinite(rgb).all())
    x_unit, selector, _ = U._prepare(x)
    _same_bits(x_unit.cpu().numpy(), want, "_prepare: x_unit")
    _same_bits(selector[:N].cpu().numpy(), sel, "_prepare: selector")


# ------------------------------------------------------------------------------------------------------------------
# 2. everything downstream is the bounded kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["f16x3-waves3", "f16x3-waves4", "f32"])
@pytest.mark.parametrize("N", N_ROWS)
@pytest.mark.parametrize("model", list(MODELS))
def test_unbounded_equals_bounded_on_the_twin(cuda, model, N, form):
    U, V = _pair(cuda, model)
    x, xc, d, _ = _inputs(cuda, N, seed=200 + N)
    for f in (U, V):
        f.fused_field_precision = form.split("-")[0]
        f.fused_field_waves = int(form[-1]) if form.startswith("f16x3") else 0
    with torch.no_grad():
        rgb_u, sig_u = U(x, d)
        den_u = U.query_density(x)
        rgb_v, sig_v = V(xc, d)
        den_v = V.query_density(xc)
    assert U._field_fused and V._field_fused, "the fused evaluator did not run"
    if form.startswith("f16x3"):
        assert not U._field_fused.range_guard_fired() and not V._field_fused.range_guard_fired()
    _equal(rgb_u, rgb_v, "rgb"); _equal(sig_u, sig_v, "density (colour kernel)"); _equal(den_u, den_v, "density")
    assert bool((den_u > 0).all()) and bool(torch.isfinite(rgb_u).all())


@pytest.mark.parametrize("N", [33, 4101])
@pytest.mark.parametrize("model", list(MODELS))
def test_debug_features_and_device_row_count(cuda, model, N):
    """The `debug_features` form (the first layer's input rows as the kernel computed them: features of the contracted
    position, the contracted coordinates themselves, their sinusoids) and the `n_rows_dev` form."""
    U, V = _pair(cuda, model)
    x, xc, d, _ = _inputs(cuda, N, seed=300 + N)
    K0 = U.mlp_base.network[0].in_features
    ld = (K0 + 31) // 32 * 32
    with torch.no_grad():
        U.query_density(x), V.query_density(xc)
        fu, fv = (torch.full((N, ld), -7.0, device=cuda) for _ in range(2))
        du = U._field_fused(x, debug_features=fu)
        dv = V._field_fused(xc, debug_features=fv)
        _equal(du, dv, "density (debug form)"); _equal(fu, fv, "feature rows")
        n_enc = sum(e.n_output_dims for e in U.mlp_base._encoders())
        _equal(fu[:, n_enc:n_enc + 3], xc, "the raw-coordinate columns hold the contracted position")
        count = N - 7
        n_dev = torch.tensor([count], dtype=torch.int64, device=cuda)
        for dirs in (None, d):
            got = U._field_fused(x, dirs, n_rows_dev=n_dev)
            ref = V._field_fused(xc, dirs, n_rows_dev=n_dev)
            for a, b in zip(got if dirs is not None else (got,), ref if dirs is not None else (ref,)):
                _equal(a[:count], b[:count], "n_rows_dev form")


# ------------------------------------------------------------------------------------------------------------------
# 3. the gradient pass
# ------------------------------------------------------------------------------------------------------------------
def _grads(f, x, d, g1, g2):
    f.zero_grad(set_to_none=True)
    rgb, density = f(x, d)
    ((rgb * g1).sum() + (density * g2).sum()).backward()
    mb, mh = f.mlp_base, f.mlp_head
    out = {"xyz": mb.encoding_xyz.params.grad, "xy": mb.encoding_xy.params.grad, "xz": mb.encoding_xz.params.grad,
           "yz": mb.encoding_yz.params.grad}
    for name, l in (("base.0", mb.network[0]), ("base.2", mb.network[2]), ("head.0", mh[0]), ("head.2", mh[2]), ("head.4", mh[4])):
        out[name + ".weight"], out[name + ".bias"] = l.weight.grad, l.bias.grad
    assert all(v is not None for v in out.values()) and len(out) == 14
    return rgb.detach(), density.detach(), {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("N", [4101, 33])
@pytest.mark.parametrize("model", list(MODELS))
def test_gradient_pass_equals_bounded_on_the_twin(cuda, model, N):
    import cnc_amd
    U, V = _pair(cuda, model)
    x, xc, d, _ = _inputs(cuda, N, seed=400 + N)
    g = torch.Generator(device=cuda).manual_seed(N)
    g1, g2 = torch.randn(N, 3, device=cuda, generator=g), torch.randn(N, 1, device=cuda, generator=g)
    with cnc_amd.reproducible(True):
        with torch.no_grad():
            U.query_density(x[:1]), V.query_density(xc[:1])
        for f in (U, V):
            f._field_fused._train_calls = False
        rgb_u, den_u, gu = _grads(U, x, d, g1, g2)
        assert U._field_fused._train_calls, "the saving fused forward was not taken"
        rgb_v, den_v, gv = _grads(V, xc, d, g1, g2)
        assert V._field_fused._train_calls
    _equal(rgb_u, rgb_v, "rgb"); _equal(den_u, den_v, "density")
    for k in gu:
        _equal(gu[k], gv[k], "grad " + k)
        assert float(gu[k].abs().max()) > 0.0, k
    assert not U.check_range_guard() and U.fused_train, "the fused training route was left"


@pytest.mark.parametrize("model", ["f8", "f2"])
def test_chain_route_equals_bounded_on_the_twin(cuda, model):
    """`fused_train=False` (also where a tripped range guard sends the gradient pass): cnc_field_prepare_contracted, the
    encoders' launches, library GEMMs forward, the gradient chain kernel backward (`_FieldChain`).  Same kernels on the
    same coordinates as the bounded field's, so the same bits, under the reproducible mode's fixed summation orders."""
    import cnc_amd
    U, V = _pair(cuda, model)
    N = 4101
    x, xc, d, _ = _inputs(cuda, N, seed=450)
    g = torch.Generator(device=cuda).manual_seed(45)
    g1, g2 = torch.randn(N, 3, device=cuda, generator=g), torch.randn(N, 1, device=cuda, generator=g)
    with cnc_amd.reproducible(True):
        with torch.no_grad():
            U.query_density(x[:1]), V.query_density(xc[:1])
        for f in (U, V):
            f.fused_train = False
            f._field_fused._train_calls = False
        rgb_u, den_u, gu = _grads(U, x, d, g1, g2)
        rgb_v, den_v, gv = _grads(V, xc, d, g1, g2)
        assert U._chain_supported and not U._field_fused._train_calls and not V._field_fused._train_calls
        with torch.no_grad():
            for f in (U, V):
                f.fused_field = False                  # gradient-free calls on the chain as well: _prepare + library GEMMs
            _equal(U.query_density(x), V.query_density(xc), "density (chain, no gradients)")
            du, fu = U.query_density(x, return_feat=True)
            dv, fv = V.query_density(xc, return_feat=True)
            _equal(du, dv, "density (return_feat)"); _equal(fu, fv, "geo features")
    _equal(rgb_u, rgb_v, "rgb"); _equal(den_u, den_v, "density")
    for k in gu:
        _equal(gu[k], gv[k], "grad " + k)
    assert bool((den_u > 0).all())


# ------------------------------------------------------------------------------------------------------------------
# 4. the range guard's fallback contracts too
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["f8", "f2"])
def test_range_guard_fallback(cuda, model):
    """As test_fp16_range_guard[weight beyond fp16]: one weight with |2^8 w| > 65504 — every call is recomputed by the
    exact-fp32 kernel enqueued behind the fp16 launch, which must apply the contraction as well."""
    U, V = _pair(cuda, model)
    x, xc, d, _ = _inputs(cuda, 4101, seed=500)
    w = U.mlp_base.network[0].weight
    keep = float(w[3, 5])
    try:
        with torch.no_grad():
            for f in (U, V):
                f.mlp_base.network[0].weight[3, 5] = 300.0
            rgb_u, sig_u = U(x, d)
            fired_rgb = U._field_fused.range_guard_fired()
            den_u = U.query_density(x)
            fired_den = U._field_fused.range_guard_fired()
            rgb_v, sig_v = V(xc, d)
            den_v = V.query_density(xc)
        assert fired_rgb and fired_den and V._field_fused.range_guard_fired()
        _equal(rgb_u, rgb_v, "rgb"); _equal(sig_u, sig_v, "density (colour kernel)"); _equal(den_u, den_v, "density")
        assert bool(torch.isfinite(rgb_u).all()) and bool(torch.isfinite(den_u).all())
    finally:
        with torch.no_grad():
            for f in (U, V):
                f.mlp_base.network[0].weight[3, 5] = keep
    with torch.no_grad():
        U.query_density(x)
    assert not U._field_fused.range_guard_fired()


# ------------------------------------------------------------------------------------------------------------------
# 5. against the op chain (the route an unbounded field took before)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", list(MODELS))
def test_against_the_op_chain(cuda, model):
    """`fused_unbounded=False` — the contraction as torch ops, one launch per encoder, library GEMMs, autograd — against
    the fused route: forward at 2e-5 of the tensor's scale, every gradient at 1e-4.  The gradient bound presumes that both
    routes see the SAME coordinates, which `contract_to_unisphere` provides by spelling its norm in the kernels' order:
    a gradient of a ReLU network is not continuous in them (a coordinate 2 ulp away, times the sinusoids' 2^9, flips a
    first-layer unit that is within rounding of zero, and the tables' gradients of f8 then move by 0.6-1 % of scale —
    measured on an MI355X with `torch.linalg.norm` in that function; forward 2.6e-6 of scale either way)."""
    U, _ = _pair(cuda, model)
    N = 4101
    x, _, d, _ = _inputs(cuda, N, seed=600)
    g = torch.Generator(device=cuda).manual_seed(6)
    g1, g2 = torch.randn(N, 3, device=cuda, generator=g), torch.randn(N, 1, device=cuda, generator=g)
    out = {}
    for fused in (False, True):
        U.fused_unbounded = fused
        with torch.no_grad():
            assert (U._fused_forward(x) is not None) == fused and U._glue_ok(x) == fused
            rgb, sig = U(x, d)
            den = U.query_density(x)
        out[fused] = (rgb, sig, den) + _grads(U, x, d, g1, g2)
    U.fused_unbounded = True
    (rgb0, sig0, den0, trgb0, tden0, gr0), (rgb1, sig1, den1, trgb1, tden1, gr1) = out[False], out[True]
    for a, b, what in ((rgb1, rgb0, "rgb"), (sig1, sig0, "density (colour kernel)"), (den1, den0, "density")):
        print(what, "max |diff| / scale: %.3g" % (float((a.double() - b.double()).abs().max()) / float(b.abs().max())))
        _close(a, b, 2e-5, what)
    _close(trgb1, trgb0, 1e-4, "rgb (gradient pass)"); _close(tden1, tden0, 1e-4, "density (gradient pass)")
    for k in gr0:
        print("grad", k, "max |diff| / scale: %.3g" % (float((gr1[k].double() - gr0[k].double()).abs().max()) / float(gr0[k].abs().max())))
        _close(gr1[k], gr0[k], 1e-4, "grad " + k)


# ------------------------------------------------------------------------------------------------------------------
# 6. against the reference's numbers
# ------------------------------------------------------------------------------------------------------------------
def _golden_inputs(g):
    """make_golden_unbounded.inputs: positions, directions, rgb weights, density weights from the stored seeds."""
    n = int(g["n"])
    pos = T.points(n, seed=int(g["point_seed"]))
    rng = np.random.default_rng(int(g["input_seed"]))
    dirs = rng.normal(size=(n, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)).astype(f32)
    return pos, dirs, rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 1)).astype(f32)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "op_chain"])
@pytest.mark.parametrize("sh", ["sh_half", "sh_float"])
@pytest.mark.parametrize("case", ["f8", "f2"])
def test_unbounded_field_matches_reference(cuda, case, sh, fused):
    """The reference's class with `unbounded=True`, run on CPU through the oracle stand-ins
    (tests/golden/make_golden_unbounded.py), under both conventions of the direction encoding's output precision."""
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    g = np.load(os.path.join(GOLD, "field_unbounded_toy.npz"))
    tag = "sh16" if sh == "sh_half" else "sh32"
    assert np.array_equal(g["aabb"], T.BOX)
    f = NGPRadianceField_mygrid_2D3D(aabb=torch.from_numpy(T.BOX.copy()), unbounded=True, ste_binary=True, ste_multistep=False,
                                     add_noise=False, Q=10, **({} if sh == "sh_half" else {"sh_fp16_round": False}),
                                     **FIELD_CASES[case])
    sd = f.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"{case}_keys"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in g[f"{case}_shapes"]]
    f.load_state_dict(fill_state(sd, seed=int(g["state_seed"])), strict=True)
    f = f.to(cuda)
    f.fused_unbounded = fused
    pos, dirs, w_rgb, w_sig = _golden_inputs(g)
    x, v = torch.from_numpy(pos).to(cuda), torch.from_numpy(dirs).to(cuda)
    p = f"{tag}_{case}"
    for grad_mode in (False, True):
        with torch.set_grad_enabled(grad_mode):
            density = f.query_density(x)
            rgb, sigma = f(x, v)
        close(density, g[f"{p}_density"], 1e-4, "density")
        close(rgb, g[f"{p}_rgb"], 1e-4, "rgb")
        close(sigma, g[f"{p}_sigma"], 1e-4, "sigma")
    assert bool(f._field_fused) == fused
    loss = (rgb * torch.from_numpy(w_rgb).to(cuda)).sum() + (sigma * torch.from_numpy(w_sig).to(cuda)).sum()
    assert abs(loss.item() - float(g[f"{p}_loss"])) <= 1e-4 * max(abs(float(g[f"{p}_loss"])), 1.0)
    f.zero_grad()
    loss.backward()
    checked = 0
    for k, q in f.named_parameters():
        if f"{p}_grad_{k}" in g.files:          # the half-precision run stores the head's gradients only
            close(q.grad, g[f"{p}_grad_{k}"], 2e-4, "grad " + k)     # that file's own bound for gradients (outputs: 1e-4)
            checked += 1
    assert checked == (14 if tag == "sh32" else 6)
    other = "sh32" if tag == "sh16" else "sh16"
    want = g[f"{other}_{case}_grad_mlp_head.0.weight"]
    err = np.abs(f.mlp_head[0].weight.grad.cpu().numpy() - want).max()
    assert err > 2e-3 * np.abs(want).max(), "the half / float harmonics are indistinguishable: the golden pins nothing"


# ------------------------------------------------------------------------------------------------------------------
# 7. end to end: a proposal-network render of an unbounded scene
# ------------------------------------------------------------------------------------------------------------------
def test_propnet_render_runs_on_the_fused_evaluator(cuda, monkeypatch):
    from cnc_amd.field import FusedFieldForward
    from cnc_amd.nerfacc import PropNetEstimator
    from cnc_amd.render import Rays, render_image_with_propnet
    U, _ = _pair(cuda, "f2")
    rng = np.random.default_rng(71)
    centre = (T.BOX[:3] + T.BOX[3:]) / 2
    o = (centre + rng.uniform(-0.3, 0.3, size=(64, 3))).astype(f32)
    d = rng.normal(size=(64, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    rays = Rays(torch.from_numpy(o).to(cuda), torch.from_numpy(d).to(cuda))
    calls = []
    orig = FusedFieldForward.__call__

    def counting(self, *a, **k):
        calls.append(a[0].shape[0])
        return orig(self, *a, **k)
    monkeypatch.setattr(FusedFieldForward, "__call__", counting)
    est = PropNetEstimator().to(cuda)
    U.eval(); est.eval()
    out = {}
    for fused in (False, True):
        U.fused_unbounded = fused
        before = len(calls)
        with torch.no_grad():
            rgb, opacity, depth, _ = render_image_with_propnet(U, [U.query_density], est, rays, num_samples=16,
                                                               num_samples_per_prop=[32], near_plane=0.05, far_plane=60.0,
                                                               sampling_type="lindisp", opaque_bkgd=True)
        out[fused] = (rgb, opacity, depth)
        assert (len(calls) > before) == fused, "the fused evaluator must serve the fused route, and only it"
    U.fused_unbounded = True
    U.train()
    assert calls[-2:] == [64 * 32, 64 * 16]             # the proposal level's densities, then the field's samples
    for a, b, what in zip(out[True], out[False], ("rgb", "opacity", "depth")):
        print(what, "max |diff| / scale: %.3g" % (float((a.double() - b.double()).abs().max()) / float(b.abs().max())))
        assert bool(torch.isfinite(a).all())
        _close(a, b, 1e-4, what)
    # (the proposal level starts from a uniform CDF in disparity over [0.05, 60]: its 32 samples per ray reach far beyond
    # the box, so both the contracted and the uncontracted branch were taken)
