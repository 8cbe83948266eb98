"""The fused field kernels — cnc_field_fused_forward in its two-wave fp16x3 form, its exact-fp32 form and its saving form,
cnc_field_backward_chain and cnc_field_weight_grads — over the lattice of models `FusedFieldForward.supported` and
`_chain_ok` admit (tests/field_lattice.py: every residue of the tail's start in a 32-column chunk per F, every kind of
16-column window, 4 to 64 units, K0 up to 575, dense / hashed / mixed tables, 1 to 12 column blocks of the chain with and
without a partial one), each against references that share no code with the package:

  * the first layer's input rows, as the two-wave kernel dumps them and as the saving form stores them, against
    `reference_features`: the encoder columns BIT-EQUAL to oracle.grid_encode_forward on the binarised tables, the raw
    coordinates equal, the sinusoids within 1e-6 (v_sin / v_cos behind a two-term reduction: 3e-7), the padding exactly 0;
  * density and rgb of every forward form against a float64 NumPy evaluation of both MLPs on those reference rows, at
    north_star's 1e-4 of the tensor's scale (the fp16 forms also within the existing 2e-5 of the library op chain);
  * the ten MLP gradients against the float64 backward under the three-part criterion of
    test_gpu_field_chain.py::test_gradient_pass_against_float64_at_full_size, and the FOUR TABLES' gradients against
    oracle.grid_encode_backward (float64 accumulators, the STE mask) fed the float64 dX sliced per encoder, each within
    3e-4 of the table's largest entry.

2081 samples per composition (65 tiles and a one-row tile): box faces, points outside, the centre, points on cell
boundaries of the coarsest and the finest levels.  The three compositions outside the kernels' shapes (67 units; F = 8 at
H = 64; 196 encoder columns) must take the library path without raising and meet the same bounds there."""
import numpy as np
import pytest
import torch

import field_lattice as fl
from test_gpu_field_chain import _float64_field, _grads, _sh4_f64
from test_gpu_field_fused import _close, _field, _inputs

pytestmark = pytest.mark.gpu
N = 2081
FORWARD = fl.FUSED + [n for n in fl.FALLBACKS if fl.BY_NAME[n].kind == "chain"]      # 196 columns: the forward is fused
MLP = {"W1": "mlp_base.network.0.weight", "b1": "mlp_base.network.0.bias", "W2": "mlp_base.network.2.weight",
       "b2": "mlp_base.network.2.bias", "W3": "mlp_head.0.weight", "b3": "mlp_head.0.bias", "W4": "mlp_head.2.weight",
       "b4": "mlp_head.2.bias", "W5": "mlp_head.4.weight", "b5": "mlp_head.4.bias"}
TABLES = ["mlp_base.encoding_xyz.params", "mlp_base.encoding_xy.params", "mlp_base.encoding_xz.params",
          "mlp_base.encoding_yz.params"]
_CASES = {}
KINK_MARGIN = 1e-5


def _near_a_kink(f, feats, dirs):
    """bool [N]: the sample has a hidden unit (of the three ReLU layers) whose float64 pre-activation z lies within
    KINK_MARGIN of its own sum of |terms| of zero.  There the ReLU's mask — and with it a whole term of the gradient —
    is decided by the forward's rounding (three-product fp16: 5e-7 per term, fp32 accumulation: 6e-8 per term and step;
    1e-5 leaves a factor of 20 for what the layers in front add), not by the arithmetic under test: either mask is the
    gradient of a forward that is exact to that rounding.  Computed from the float64 reference alone."""
    mb, mh = f.mlp_base.network, f.mlp_head
    W1, b1, W2, b2, W3, b3, W4, b4 = (t.detach().cpu().numpy().astype(np.float64) for t in
                                      (mb[0].weight, mb[0].bias, mb[2].weight, mb[2].bias, mh[0].weight, mh[0].bias,
                                       mh[2].weight, mh[2].bias))
    near = np.zeros(feats.shape[0], bool)

    def layer(a, W, b):
        z = a @ W.T + b
        near[:] |= (np.abs(z) <= KINK_MARGIN * (np.abs(a) @ np.abs(W).T + np.abs(b))).any(axis=1)
        return np.maximum(z, 0.0)
    h1 = layer(feats[:, :W1.shape[1]].astype(np.float64), W1, b1)
    o2 = h1 @ W2.T + b2
    d32 = ((dirs.astype(np.float32) + np.float32(1.0)) / np.float32(2.0)) * np.float32(2.0) - np.float32(1.0)
    h3 = layer(np.concatenate([_sh4_f64(d32.astype(np.float64)), o2[:, 1:]], axis=1), W3, b3)
    layer(h3, W4, b4)
    return near


class _Case:
    """One composition: the model, its 2081 samples, and every reference — computed once, left unchanged."""

    def __init__(self, cuda, oracle, name):
        self.name, self.e = name, fl.BY_NAME[name]
        seed = 100 + [x.name for x in fl.LATTICE].index(name)
        f = self.f = _field(cuda, fl.kwargs_of(self.e), seed=seed, sh_fp16_round=False)   # (the half-rounded SH has its own golden)
        x, d = _inputs(cuda, N, seed=seed + 1)
        on_edges = torch.from_numpy(fl.boundary_points(self.e)).to(cuda)
        x[8:8 + on_edges.shape[0]] = on_edges
        self.x, self.d = x, d
        self.xu_dev = (x - f.aabb[:3]) / (f.aabb[3:] - f.aabb[:3])
        self.xu = self.xu_dev.cpu().numpy().astype(np.float32)
        self.sel = np.all((self.xu > 0) & (self.xu < 1), axis=1)
        self.params = fl.field_params(f)
        self.k0, self.n_enc, self.ld = fl.k0_of(self.e), fl.n_enc_of(self.e), fl.roundup32(fl.k0_of(self.e))
        assert f.mlp_base.network[0].in_features == self.k0
        self.ref = fl.reference_features(self.params, self.xu, oracle)
        assert self.ref.shape == (N, self.ld)
        # gradients of very different sizes from sample to sample, as a rendering loss produces them (weights w_i T_i)
        g = torch.Generator(device=cuda).manual_seed(9)
        scale = torch.exp(torch.randn(N, 1, device=cuda, generator=g) * 3.0 - 6.0)
        self.wr = torch.randn(N, 3, device=cuda, generator=g) * scale
        self.wd = torch.randn(N, 1, device=cuda, generator=g) * scale * 0.1
        # ... none to the few samples that sit on a ReLU's kink (`_near_a_kink`): their rows run through every kernel as
        # rows of zero gradient
        self.near_kink = _near_a_kink(f, self.ref, d.cpu().numpy())
        assert float(self.near_kink.mean()) < 0.05, float(self.near_kink.mean())
        keep = torch.from_numpy(~self.near_kink).to(cuda)[:, None]
        self.wr, self.wd = self.wr * keep, self.wd * keep
        self.rgb64, self.den64, self.G64, self.A64, self.dX64 = _float64_field(
            f, self.ref, self.xu, d.cpu().numpy(), self.wr.cpu().numpy().astype(np.float64),
            self.wd.cpu().numpy().astype(np.float64), want_dx=True)
        self._tables64, self._chain_out, self._oracle = None, None, oracle
        # densities on both sides: some samples outside the box (exactly zero), most inside (positive)
        assert 0.05 < float((self.den64 > 0).mean()) < 0.95 and np.array_equal(self.den64 > 0, self.sel)

    def tables64(self):
        if self._tables64 is None:
            self._tables64 = fl.table_gradients64(self.params, self.xu, self.dX64, self._oracle)
        return self._tables64

    def op_chain(self):
        """(rgb, density of the colour call, density) of the library op chain: encoder launches, GEMMs, glue kernels."""
        if self._chain_out is None:
            f = self.f
            with torch.no_grad():
                f.fused_field = False
                rgb, sig = f(self.x, self.d)
                den = f.query_density(self.x)
                f.fused_field = True
            self._chain_out = (rgb, sig, den)
        return self._chain_out


def _case(cuda, oracle, name):
    if name not in _CASES:
        _CASES[name] = _Case(cuda, oracle, name)
    c = _CASES[name]
    f = c.f
    f.fused_field, f.fused_field_precision, f.fused_field_waves = True, "f16x3", 0
    f.fused_chain = f.fused_train = True
    return c


def _check_rows(got, c, what):
    """First-layer input rows [N, roundup32(K0)] against the reference's."""
    ref, n_enc, k0 = c.ref, c.n_enc, c.k0
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not np.isnan(got).any(), (what, "columns never written:", sorted(set(np.nonzero(np.isnan(got))[1].tolist())))
    got = got.astype(np.float64)
    bad = np.nonzero((got[:, :n_enc] != ref[:, :n_enc]).any(axis=0))[0]
    assert bad.size == 0, (what, "encoder columns that differ from the oracle's:", bad.tolist(),
                           float(np.abs(got[:, :n_enc] - ref[:, :n_enc]).max()))
    assert float(np.abs(ref[:, :n_enc]).max()) > 0.5
    assert np.array_equal(got[:, n_enc:n_enc + 3], ref[:, n_enc:n_enc + 3]), (what, "raw coordinates")
    err = np.abs(got[:, n_enc + 3:k0] - ref[:, n_enc + 3:k0]).max(axis=0)
    assert float(err.max()) < 1e-6, (what, "sinusoid columns off:", (n_enc + 3 + np.nonzero(err >= 1e-6)[0]).tolist(), float(err.max()))
    assert np.all(got[:, k0:] == 0), (what, "padding")


def _check_outputs(rgb, den, c, what, chain_tol=None):
    """rgb [N, 3] / density [N, 1] (either may be None) against float64 at 1e-4 of the tensor's scale; `chain_tol`: and
    against the library op chain; the selector pattern exact."""
    ref_rgb, ref_sig, ref_den = c.op_chain() if chain_tol is not None else (None, None, None)
    if den is not None:
        got = den.cpu().numpy().reshape(-1).astype(np.float64)
        err, scale = float(np.abs(got - c.den64).max()), float(c.den64.max())
        print(f"LATTICE {c.name} {what}: density |error| {err:.3e} of scale {scale:.3e}")
        assert err <= 1e-4 * scale, (c.name, what, "density", err, scale)
        assert np.array_equal(got == 0, ~c.sel), (c.name, what, "selector pattern")
        if chain_tol is not None:
            _close(den.reshape(-1, 1), ref_den if rgb is None else ref_sig, chain_tol, f"{c.name} {what}: density against the op chain")
    if rgb is not None:
        err = float(np.abs(rgb.cpu().numpy().astype(np.float64) - c.rgb64).max())
        print(f"LATTICE {c.name} {what}: rgb |error| {err:.3e}")
        assert err <= 1e-4, (c.name, what, "rgb", err)
        if chain_tol is not None:
            _close(rgb, ref_rgb, chain_tol, f"{c.name} {what}: rgb against the op chain")


def _gradient_errors(grads, c):
    """Per MLP tensor (max |error| / largest entry, max |error| / (sum |terms| + 1 % of the largest entry), max relative
    error of the entries that are no cancellations, their count, entries): the figures of
    test_gradient_pass_against_float64_at_full_size.  Per table: max |error| / largest entry."""
    worst = {}
    for k, name in MLP.items():
        got = grads[name].cpu().numpy().astype(np.float64)
        want = c.G64[k][:, :got.shape[1]] if got.ndim == 2 else c.G64[k]
        assert got.shape == want.shape, (k, got.shape, want.shape)
        big = float(np.abs(want).max())
        scale_ = c.A64[k][:, :got.shape[1]] if got.ndim == 2 else c.A64[k]
        ratio = np.abs(got - want) / (scale_ + 1e-2 * big)
        m = (np.abs(want) >= 1e-5 * big) & (np.abs(want) >= 1e-2 * scale_)
        rel = np.abs(got - want)[m] / np.abs(want)[m]
        worst[k] = (float(np.abs(got - want).max()) / big, float(ratio.max()), float(rel.max()) if m.any() else 0.0,
                    int(m.sum()), int(m.size))
    tables = {}
    for name, want in zip(TABLES, c.tables64()):
        got = grads[name].cpu().numpy().astype(np.float64)
        assert got.shape == want.shape, (name, got.shape, want.shape)
        big = float(np.abs(want).max())
        assert big > 0, name
        tables[name] = float(np.abs(got - want).max()) / big
    return worst, tables


def _check_gradients(grads, c, what):
    assert set(grads) == set(MLP.values()) | set(TABLES), sorted(grads)
    worst, tables = _gradient_errors(grads, c)
    print(f"LATTICE {c.name} {what}: MLP gradients {worst}")
    print(f"LATTICE {c.name} {what}: table gradients {tables}")
    for k, w in worst.items():
        assert w[0] <= 3e-4 and w[1] <= 1e-4 and w[2] <= 3e-3, (c.name, what, k, w)
    for name, err in tables.items():
        assert err <= 3e-4, (c.name, what, name, err)


@pytest.mark.parametrize("name", FORWARD)
def test_first_layer_input_rows_against_the_oracle(cuda, oracle, name):
    """What the two-wave density kernel dumps (`debug_features`) and what the saving form keeps (`kept["feat"]`): both the
    reference's rows.  The dump goes into a NaN-filled buffer one chunk wider than the row: written everywhere up to
    roundup32(K0), untouched behind it."""
    c = _case(cuda, oracle, name)
    f = c.f
    dump = torch.full((N, c.ld + 32), float("nan"), device=cuda)
    with torch.no_grad():
        f.query_density(c.x[:8])                                         # builds the evaluator
        assert f._field_fused, "the fused kernel did not run"
        f._field_fused(c.x, debug_features=dump)
        assert not f._field_fused.range_guard_fired()
        _, _, kept = f._field_fused.save_forward(c.x, c.d, N)
    dump = dump.cpu().numpy()
    assert np.isnan(dump[:, c.ld:]).all(), "the dump wrote behind roundup32(K0)"
    _check_rows(dump[:, :c.ld], c, "debug_features")
    assert kept["feat"].shape == (N, c.ld)
    _check_rows(kept["feat"].cpu().numpy(), c, "save_forward")
    assert torch.equal(kept["xyz"], c.xu_dev) and np.array_equal(kept["selector"].cpu().numpy().astype(bool), c.sel)


@pytest.mark.parametrize("name", FORWARD)
def test_density_and_rgb_of_every_forward_form_against_float64(cuda, oracle, name):
    c = _case(cuda, oracle, name)
    f = c.f
    with torch.no_grad():
        for waves in (4, 3):                                             # the two register budgets of the density kernel
            f.fused_field_waves = waves
            den = f.query_density(c.x)
            assert f._field_fused and not f._field_fused.range_guard_fired()
            _check_outputs(None, den, c, f"f16x3 density, {waves} waves", chain_tol=2e-5)
        f.fused_field_waves = 0
        rgb, den = f(c.x, c.d)
        assert not f._field_fused.range_guard_fired()
        _check_outputs(rgb, den, c, "f16x3 colour", chain_tol=2e-5)
        f.fused_field_precision = "f32"
        den = f.query_density(c.x)
        _check_outputs(None, den, c, "f32 density")
        rgb, den = f(c.x, c.d)
        _check_outputs(rgb, den, c, "f32 colour")
        f.fused_field_precision = "f16x3"
        rgb, den, _ = f._field_fused.save_forward(c.x, c.d, N)
        _check_outputs(rgb, den, c, "saving forward")
        # ... within the existing bound of the op chain (test_fused_training_forward_and_its_gradients)
        ref_rgb, ref_sig, _ = c.op_chain()
        assert float((rgb - ref_rgb).abs().max()) <= 2e-5
        assert float((den - ref_sig).abs().max()) <= 2e-5 * max(1.0, float(ref_sig.abs().max()))
        assert not f._field_fused.range_guard_fired()


@pytest.mark.parametrize("train", [False, True], ids=["chain", "fused_training_forward"])
@pytest.mark.parametrize("name", fl.CHAIN)
def test_gradient_pass_against_float64_and_the_oracle(cuda, oracle, name, train):
    """cnc_field_backward_chain + cnc_field_weight_grads behind the library forward (`chain`) and behind the saving fused
    forward (`fused_training_forward`): rgb / density at 1e-4; every MLP gradient entry within 3e-4 of its tensor's largest,
    within 1e-4 of its own sum of |terms| (+ 1 % of the largest), the entries that are no cancellations relatively exact to
    3e-3; every table's gradient within 3e-4 of its largest entry of the oracle's float64 scatter of the float64 dX.

    Measured over the 74 cases (and the six of the fallbacks): at most 2.0e-6 of a tensor's largest entry, 1.1e-5 of an
    entry's sum of |terms|, 1.9e-3 relative on the entries that are no cancellations, 9.3e-7 of a table's largest entry.
    With the loss weights of the samples on a ReLU's kink left in (`_near_a_kink`: about two rows in a hundred) two cases
    missed a bound by one flipped unit of one heavy sample: f4_h160_4x3d_2x2d behind the library forward, head.2's weight
    at 1.31e-4 of its sum of |terms| — the layer-by-layer library path measured the same 1.31e-4 there — and
    f8_h160_9x3d_1x2d behind the fused training forward, head.0's weight at 4.4e-3 of its largest entry (unit 154 of
    head.0 on the second-heaviest sample: float64 pre-activation 1.9e-8, the kernel's 0)."""
    c = _case(cuda, oracle, name)
    f = c.f
    if f._field_fused:
        f._field_fused._train_calls = False                              # (an earlier test's saving forward set it)
    rgb, den, grads = _grads(f, c.x, c.d, c.wr, c.wd, chain=True, train=train)
    assert f._chain_supported, "the chain did not run"
    if train:
        assert f._field_fused and f._field_fused._train_calls, "the fused training forward did not run"
    what = "fused training forward + chain" if train else "library forward + chain"
    _check_outputs(rgb, den, c, what)
    _check_gradients(grads, c, what)
    if train:
        assert not f.check_range_guard()


@pytest.mark.parametrize("name", fl.FALLBACKS)
def test_fallbacks_do_not_raise_and_meet_the_bounds(cuda, oracle, name):
    """67 units and (F = 8, H = 64): no fused kernel, forward or backward; 196 encoder columns: the fused forward, the
    layer-by-layer gradient pass.  Nothing raises, and the library path meets the float64 bounds."""
    c = _case(cuda, oracle, name)
    f, kind = c.f, c.e.kind
    with torch.no_grad():
        rgb, sig = f(c.x, c.d)
        den = f.query_density(c.x)
    if kind == "chain":
        assert f._field_fused
    else:
        assert f._field_fused is False
    _check_outputs(rgb, sig, c, "gradient-free colour call")
    _check_outputs(None, den, c, "gradient-free density call")
    if f._field_fused:
        f._field_fused._train_calls = False                              # (an earlier test's saving forward set it)
    for train in (False, True):
        rgb, den, grads = _grads(f, c.x, c.d, c.wr, c.wd, chain=True, train=train)
        assert f._chain_supported is False
        assert not getattr(f._field_fused, "_train_calls", False)
        _check_outputs(rgb, den, c, f"library gradient pass (train={train})")
        _check_gradients(grads, c, f"library gradient pass (train={train})")
