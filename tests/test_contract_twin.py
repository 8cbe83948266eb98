"""CPU: the NumPy twin of the unbounded field's contraction (tests/contract_twin.py) against the torch restatement of
the reference's `contract_to_unisphere` (cnc_amd.field, ngp.py:337-361), the twin's exact cases, and the host-side
routing of an unbounded field (`FusedFieldForward.shapes_ok` / `supported`, the `fused_unbounded` switch).

The twin is what the device code is held to bit for bit (tests/test_gpu_field_unbounded.py); torch's chain on the CPU
is not (its vectorised sqrt and reciprocal are not correctly rounded), hence a bound and not equality here."""
import numpy as np
import torch

import contract_twin as T

f32 = np.float32


def test_twin_against_the_torch_restatement():
    """The restatement spells its norm in the twin's order, so what is left between the two is torch's own CPU
    arithmetic.  Bound: 2.4e-7, twice the 1.19e-7 (2 ulp at 0.5..1) measured.  Measured on 60 000 points of the shared
    set: max |diff| 1.19e-7, 99.5 % of the rows bit-equal (torch's vectorised CPU sqrt and reciprocal are not correctly
    rounded in under 1 % of the elements); against float64 both are 9.59e-8 off at most (printed with pytest -s)."""
    from cnc_amd.field import contract_to_unisphere
    p = T.points(60000, seed=1)
    x, sel = T.contract(p)
    want = contract_to_unisphere(torch.from_numpy(p), torch.from_numpy(T.BOX)).numpy()
    diff = np.abs(x.astype(np.float64) - want.astype(np.float64))
    p64, lo, hi = p.astype(np.float64), T.BOX[:3].astype(np.float64), T.BOX[3:].astype(np.float64)
    c = (p64 - lo) / (hi - lo) * 2 - 1
    mag = np.linalg.norm(c, axis=1, keepdims=True)
    with np.errstate(all="ignore"):                                        # mag == 0 at the box centre: not selected below
        ref = np.where(mag > 1, (2 - 1 / mag) * (c / mag), c) / 4 + 0.5
    print("twin vs torch: max |diff| %.3g, rows bit-equal %.1f %%; vs float64: twin %.3g, torch %.3g" % (
        diff.max(), 100.0 * (x.view(np.uint32) == want.view(np.uint32)).all(1).mean(),
        np.abs(x - ref).max(), np.abs(want - ref).max()))
    assert diff.max() <= 2.4e-7
    assert np.array_equal(sel.astype(bool), ((want > 0) & (want < 1)).all(1))
    # ... and against the reference's own spelling (ngp.py:337-361, `torch.linalg.norm`), which shares no line with the
    # twin: same bound (measured 1.19e-7, 92.6 % of the rows bit-equal)
    t, box = torch.from_numpy(p), torch.from_numpy(T.BOX)
    c32 = (t - box[:3]) / (box[3:] - box[:3]) * 2 - 1
    m32 = torch.linalg.norm(c32, ord=2, dim=-1, keepdim=True)
    far = m32.squeeze(-1) > 1
    c32[far] = (2 - 1 / m32[far]) * (c32[far] / m32[far])
    ref32 = (c32 / 4 + 0.5).numpy()
    print("twin vs linalg.norm spelling: max |diff| %.3g" % np.abs(x.astype(np.float64) - ref32).max())
    assert np.abs(x.astype(np.float64) - ref32).max() <= 2.4e-7


def test_twin_exact_cases():
    x, sel = T.contract(T.exact_cases())
    assert np.array_equal(x[0], np.array([0.5, 0.5, 0.5], f32))                  # the box centre
    assert np.array_equal(x[1], np.array([0.75, 0.5, 0.5], f32))                 # mag == 1 exactly: NOT contracted
    assert x[2, 0] < f32(1) and x[2, 0] > f32(0.999) and x[2, 1] == f32(0.5) and x[2, 2] == f32(0.5)     # p_x = 1e6
    assert sel.tolist() == [1, 1, 1]
    # u = (2, .5, .5): c = (3, 0, 0), mag = 3 exactly -> k = 2 - 1/3 on the x axis
    p = T.exact_cases()[1:2].copy()
    p[0, 0] = f32(4.5)
    x1, _ = T.contract(p)
    assert np.array_equal(x1[0], np.array([(f32(2) - f32(1) / f32(3)) / f32(4) + f32(0.5), 0.5, 0.5], f32))


def test_point_set_mixes_every_tile_and_selects_every_row():
    """What the GPU tests rely on: every 32-sample tile holds contracted and uncontracted rows, and the twin leaves no
    coordinate <= 0 or >= 1 on this set (600 000 points) — selector 0 is exercised by the saving form's rows of padding
    only."""
    p = T.points(600000, seed=2)
    x, sel = T.contract(p)
    assert sel.all() and float(x.min()) > 0.0 and float(x.max()) < 1.0
    lo, hi = T.BOX[:3], T.BOX[3:]
    c = (p - lo) / (hi - lo) * f32(2) - f32(1)
    far = (np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) > 1).reshape(-1, 32)
    assert far.any(1).all() and (~far).any(1).all()
    for n in (1, 31, 32, 33, 4101):
        assert T.points(n).shape == (n, 3) and T.points(n).dtype == f32
        assert np.array_equal(T.points(n)[:min(n, 3)], T.exact_cases()[:min(n, 3)])


BASE = dict(aabb=[-1.5] * 3 + [1.5] * 3, resolutions_list=(6, 9, 14), log2_hashmap_size=8,
            resolutions_list_2D=(10, 18), log2_hashmap_size_2D=8)


def test_unbounded_field_keeps_the_shape_table():
    """`shapes_ok` is the shape table without the box: True for the unbounded models whose bounded twins the kernels
    take (while `supported`, the bounded table, still says False), and equal to `supported` for every bounded case of
    tests/test_host_logic.py::test_fused_field_shape_table_on_cpu."""
    from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
    for kw in (dict(n_features_per_level=8, n_neurons=160), dict(n_features_per_level=2, n_neurons=64)):
        f = NGPRadianceField_mygrid_2D3D(**BASE, **kw, unbounded=True)
        assert FusedFieldForward.shapes_ok(f) and not FusedFieldForward.supported(f)
        assert f._chain_supported is None
    bounded = [dict(n_features_per_level=8, n_neurons=160), dict(n_features_per_level=4, n_neurons=160),
               dict(n_features_per_level=2, n_neurons=64), dict(n_features_per_level=4, n_neurons=64),
               dict(n_features_per_level=8, n_neurons=64), dict(n_features_per_level=2, n_neurons=128),
               dict(n_features_per_level=1, n_neurons=64), dict(n_features_per_level=8, n_neurons=160, fused_ste=False)]
    want = [True, True, True, True, False, False, False, False]
    for kw, ok in zip(bounded, want):
        f = NGPRadianceField_mygrid_2D3D(**BASE, **kw)
        assert FusedFieldForward.shapes_ok(f) == FusedFieldForward.supported(f) == ok, kw
    # a shape outside the table stays outside it when the field is unbounded
    assert not FusedFieldForward.shapes_ok(NGPRadianceField_mygrid_2D3D(**BASE, n_features_per_level=8, n_neurons=64, unbounded=True))


def test_fused_unbounded_switch(monkeypatch):
    """`fused_unbounded` (default on; CNC_FUSED_UNBOUNDED=0 read at construction) only bears on unbounded fields; host
    tensors never reach a kernel."""
    from cnc_amd import _lib
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D
    assert _lib.CNC_FIELD_CONTRACT == 16 and "cnc_field_prepare_contracted" in _lib.SIGNATURES
    kw = dict(n_features_per_level=2, n_neurons=64)
    f = NGPRadianceField_mygrid_2D3D(**BASE, **kw, unbounded=True)
    assert f.fused_unbounded is True
    monkeypatch.setenv("CNC_FUSED_UNBOUNDED", "0")
    g = NGPRadianceField_mygrid_2D3D(**BASE, **kw, unbounded=True)
    assert g.fused_unbounded is False
    monkeypatch.delenv("CNC_FUSED_UNBOUNDED")
    x = torch.from_numpy(T.points(64, seed=3))
    with torch.no_grad():
        assert f._fused_forward(x) is None and not f._glue_ok(x)           # host tensors: no kernel either way
