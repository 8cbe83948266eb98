"""The lattice of tests/field_lattice.py covers what tests/test_gpu_field_lattice.py claims for it, its reference is pinned
by a second twin, and `FusedFieldForward.supported` gives the verdict the lattice expects — all on the host."""
import numpy as np
import pytest
import torch

import field_lattice as fl
import np_twins

AABB = [-1.5] * 3 + [1.5] * 3


def _entries(F=None, H=None, kind="fused"):
    return [e for e in fl.LATTICE if e.kind == kind and F in (None, e.F) and H in (None, e.H)]


def test_every_entry_is_a_model_of_the_ladders():
    for e in fl.LATTICE:
        kw = fl.kwargs_of(e)
        assert kw["resolutions_list"] == fl.LADDER_3D[:e.L3] and len(kw["resolutions_list"]) == e.L3
        assert kw["resolutions_list_2D"] == fl.LADDER_2D[:e.L2] and len(kw["resolutions_list_2D"]) == e.L2
        assert fl.units_of(e) == e.L3 + 3 * e.L2 and fl.k0_of(e) == e.F * fl.units_of(e) + 63
    # only the 67-unit fallback reaches past the sixteen 3-D resolutions
    assert [e.name for e in fl.LATTICE if e.L3 > 16] == [e.name for e in fl.LATTICE if e.kind == "units"]


def test_tables_are_dense_hashed_or_both_as_named():
    for e in fl.LATTICE:
        kw = fl.kwargs_of(e)
        d3 = [R ** 3 <= 2 ** kw["log2_hashmap_size"] for R in kw["resolutions_list"]]
        d2 = [R ** 2 <= 2 ** kw["log2_hashmap_size_2D"] for R in kw["resolutions_list_2D"]]
        if e.tables == "dense":
            assert all(d3) and all(d2), e.name
        elif e.tables == "hashed":
            assert not any(d3) and not any(d2), e.name
        else:
            assert d3[0] and d2[0] and (kw["log2_hashmap_size"], kw["log2_hashmap_size_2D"]) == (10, 9)
    assert any(e.tables == "dense" for e in _entries()) and any(e.tables == "hashed" for e in _entries())
    # "mixed" really mixes somewhere: a composition with dense and hashed levels in the 3-D grid AND in the planes
    assert any(e.tables == "mixed" and e.L3 > 4 and e.L2 > 5 for e in _entries())


@pytest.mark.parametrize("F", [2, 4, 8])
def test_sweep_reaches_every_residue_of_the_tail_start(F):
    """U = F units mod 32 (the chunk): every multiple of F, at H = 160; and an odd L3 and an odd L2 among them."""
    es = _entries(F, 160)
    assert {fl.n_enc_of(e) % 32 for e in es} == set(range(0, 32, F))
    assert any(e.L3 % 2 == 1 for e in es) and any(e.L3 % 2 == 0 for e in es)
    assert any(e.L2 % 2 == 1 for e in es) and {e.L2 for e in es} >= {1, 2, 3, 5}
    if F == 2:        # U mod 8 in {2, 6}: a sin / cos pair three columns apart straddles 8-column windows differently
        assert {fl.n_enc_of(e) % 8 for e in es} == {0, 2, 4, 6}
    assert all(fl.straddling_pairs(e, 8) > 0 and fl.straddling_pairs(e, 16) > 0 for e in es)


@pytest.mark.parametrize("F", [2, 4])
def test_reduced_sweep_at_64_neurons(F):
    es = _entries(F, 64)
    assert len({fl.n_enc_of(e) % 32 for e in es if e.tables == "mixed"}) >= 4
    assert all(fl.forward_fused(e) for e in es)


@pytest.mark.parametrize("F", [2, 4, 8])
def test_every_window_kind_runs_per_feature_count(F):
    seen = set()
    for e in _entries(F, 160):
        seen |= fl.window_kinds(e)
    assert seen == {"3d", "plane", "planes", "tail", "mixed"}, (F, seen)


def test_window_kinds_on_known_rows():
    # F = 8, 12 + 3 x 4 levels: every boundary on a multiple of 16 columns — what the suite ran before
    e = fl.Entry("x", 8, 160, 12, 4, "mixed", "fused")
    assert fl.window_kinds(e) == {"3d", "plane", "tail"}
    # F = 8, 3 + 3 x 2: halves [0,1] 3-D, [2,3] 3-D + xy, [4,5] xy + xz, [6,7] xz + yz, [8, tail]
    e = fl.Entry("x", 8, 160, 3, 2, "mixed", "fused")
    assert fl.window_kinds(e) == {"3d", "mixed", "planes", "tail"}


def test_extremes_are_in_the_lattice():
    es = _entries()
    for F in (2, 4, 8):
        assert any((e.F, e.L3, e.L2) == (F, 1, 1) for e in es)
    assert any(e.F == 8 and fl.units_of(e) == 64 and fl.k0_of(e) == 575 for e in es)
    assert any(e.F == 2 and fl.units_of(e) == 64 for e in es)
    assert any(e.F == 8 and fl.units_of(e) == 40 and fl.k0_of(e) == 383 for e in es)
    assert max(fl.units_of(e) for e in es) == fl.MAX_UNITS
    chain = [fl.BY_NAME[n] for n in fl.CHAIN]
    assert {8, 12, 100, 112, 184, 188, 192} <= {fl.n_enc_of(e) for e in chain}
    blocks = {fl.chain_blocks(e) for e in chain}
    assert {(1, False), (1, True), (7, False), (7, True), (12, False), (12, True)} <= blocks, blocks
    assert any(fl.n_enc_of(e) % 16 == 4 for e in chain)                # a 4-column partial block
    assert {11} <= {b for b, _ in blocks}
    # the fallbacks
    kinds = {e.kind: e for e in fl.LATTICE if e.kind != "fused"}
    assert fl.units_of(kinds["units"]) == 67 and (kinds["units"].L3, kinds["units"].L2) == (19, 16)
    assert (kinds["shape"].F, kinds["shape"].H) == (8, 64)
    assert fl.n_enc_of(kinds["chain"]) == 196 and fl.forward_fused(kinds["chain"]) and not fl.chain_capable(kinds["chain"])


@pytest.fixture(scope="module")
def host_fields():
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    out = {}

    def get(name):
        if name not in out:
            torch.manual_seed(1)
            f = NGPRadianceField_mygrid_2D3D(aabb=AABB, **fl.kwargs_of(fl.BY_NAME[name]))
            with torch.no_grad():
                for e in f.mlp_base._encoders():
                    e.params.uniform_(-1, 1)
            out[name] = f
        return out[name]
    return get


@pytest.mark.parametrize("name", [e.name for e in fl.LATTICE])
def test_supported_gives_the_expected_verdict(host_fields, name):
    from cnc_amd.field import FusedFieldForward
    e = fl.BY_NAME[name]
    f = host_fields(name)
    assert f.mlp_base.network[0].in_features == fl.k0_of(e)
    assert sum(enc.n_levels for enc in f.mlp_base._encoders()) == fl.units_of(e)
    want = e.kind in ("fused", "chain")
    assert fl.forward_fused(e) == want
    assert bool(FusedFieldForward.supported(f)) == want, name
    assert fl.chain_capable(e) == (name in fl.CHAIN)
    # the chain's own conditions (`_chain_ok`, evaluated there only with a device tensor in hand), restated
    n_enc = sum(enc.n_output_dims for enc in f.mlp_base._encoders())
    assert n_enc == fl.n_enc_of(e)
    assert fl.chain_capable(e) == (want and n_enc % 4 == 0 and n_enc <= 192
                                   and (1 + f.geo_feat_dim + 31) // 32 * 32 <= e.H
                                   and 1 + f.geo_feat_dim <= (80 if e.H == 160 else 64))


def test_more_than_64_units_is_refused_on_the_host():
    """The two-wave kernels keep 64 unit records in LDS and the C entry returns CNC_ERR_UNSUPPORTED above that: the
    host must not send such a model there."""
    from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
    mk = lambda L3, L2: NGPRadianceField_mygrid_2D3D(aabb=AABB, **fl.composition(2, 160, L3, L2))
    assert FusedFieldForward.MAX_UNITS == fl.MAX_UNITS
    assert FusedFieldForward.supported(mk(16, 16))                      # 64
    assert not FusedFieldForward.supported(mk(17, 16))                  # 65
    assert not FusedFieldForward.supported(mk(19, 16))                  # 67


@pytest.mark.parametrize("name", ["f2_h160_3x3d_2x2d", "f8_h160_5x3d_3x2d", "f2_h64_4x3d_2x2d_hashed"])
def test_reference_features_against_the_second_twin(oracle, host_fields, name):
    """oracle.grid_encode_forward on the binarised tables (what `reference_features` is built from) equals
    np_twins.grid_encode_forward with its own STE, encoder by encoder and bit for bit; the rest of the row is the
    coordinates, NumPy's sinusoids and zeros."""
    e = fl.BY_NAME[name]
    params = fl.field_params(host_fields(name))
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.03, 1.03, size=(257, 3)).astype(np.float32)          # a few points outside the unit cube
    x[:32] = (fl.boundary_points(e) + 1.5) / 3.0
    x[32] = (0.0, 0.5, 1.0)
    ref = fl.reference_features(params, x, oracle)
    n_enc, k0 = fl.n_enc_of(e), fl.k0_of(e)
    assert ref.shape == (257, fl.roundup32(k0)) and ref.dtype == np.float64
    twin = fl.encoder_columns(params, x, lambda xx, s, o, r: np_twins.grid_encode_forward(
        xx, np.where(s >= 0, np.float32(0.25), np.float32(-3.0)), o, r, ste_binary=True))
    assert twin.shape == (257, n_enc)
    assert np.array_equal(ref[:, :n_enc], twin.astype(np.float64))
    assert float(np.abs(twin).max()) > 0.5 and np.all(np.abs(twin) <= 1.0 + 1e-6)
    assert np.array_equal(ref[:, n_enc:n_enc + 3], x.astype(np.float64))
    for k in range(10):
        arg = (x * np.float32(2.0 ** k)).astype(np.float64)
        assert np.array_equal(ref[:, n_enc + 3 + 6 * k:n_enc + 6 + 6 * k], np.sin(arg))
        assert np.array_equal(ref[:, n_enc + 6 + 6 * k:n_enc + 9 + 6 * k], np.cos(arg))
    assert np.all(ref[:, k0:] == 0) and ref.shape[1] - k0 < 32
    # the encoders really are four different ones on four coordinate pairs: swapping a pair changes the columns
    swapped = fl.reference_features(params, x[:, [0, 2, 1]], oracle)
    assert not np.array_equal(swapped[:, e.F * e.L3:n_enc], ref[:, e.F * e.L3:n_enc])


def test_table_gradients64_is_the_adjoint_of_the_encoder(oracle, host_fields):
    """<dX, features(table)> differentiated with respect to the (binarised) table: the oracle's backward on dX sliced per
    encoder is the transpose of its forward — sum(dX * features) == sum(grad * signs) per table."""
    name = "f2_h160_3x3d_2x2d"
    e = fl.BY_NAME[name]
    params = fl.field_params(host_fields(name))
    rng = np.random.default_rng(3)
    x = rng.uniform(0.0, 1.0, size=(300, 3)).astype(np.float32)
    dX = rng.standard_normal((300, fl.n_enc_of(e)))
    grads = fl.table_gradients64(params, x, dX, oracle)
    feats = fl.reference_features(params, x, oracle)
    col = 0
    for (table, offs, res), g in zip(params["encoders"], grads):
        w = len(res) * e.F
        signs = np.where(table >= 0, 1.0, -1.0)
        lhs = float((dX[:, col:col + w].astype(np.float32).astype(np.float64) * feats[:, col:col + w]).sum())
        rhs = float((g * signs).sum())
        terms = float(np.abs(dX[:, col:col + w] * feats[:, col:col + w]).sum())
        assert abs(lhs - rhs) <= 1e-6 * terms, (col, lhs, rhs, terms)        # float32 features and products: 6e-8 per term
        assert g.shape == table.shape and np.abs(g).max() > 0
        col += w
