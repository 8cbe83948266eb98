"""GPU: cnc_field_position_grad (cnc_amd/csrc/field_position_grad.hip) against its float64 twin
(tests/pose_twin.py, itself held to central differences by tests/test_pose_twin.py), through the C ABI.

Models: the smallest of tests/field_lattice.py with both a dense and a hashed 3-D level and planes, at F = 2, 4 and 8
(the kernel's three instances), and the all-hashed one (hashed planes too). N in {1, 63, 64, 65, 257}: one lane quad, a block less one / exactly / plus
one sample (64 samples per block), several blocks.  The points cycle through: uniform in the box, cell faces of the
coarsest and finest levels (`field_lattice.boundary_points`: floor() at its edge — twin and kernel take the cell from
the same float32 operations, so they stand on the same side), the border ring (a coordinate in the outermost cell,
where the normaliser's derivative matters), the box faces and points outside the box (selector 0: the row must be
exactly +0), and an inside point whose selector byte is 0.  The box is not a cube (per-axis scale).

Bound: |got - want| <= 1e-4 x the entry's sum of |terms| (the bound tests/test_gpu_field_lattice.py applies to MLP gradient
entries); an entry without terms must be exactly 0.  Every buffer lies inside a sentinel-filled allocation
(tests/guarded.py); dX and the selector have more rows than N, dX and dS wider rows than the kernel reads, all poisoned.

Measured on the MI355X: the largest |got - want| / sum |terms| over all cases is 1.23e-7 (f2_h64_5x3d_5x2d, N = 257);
at F = 4, 1.01e-7 (f4_h64_6x3d_1x2d, N = 65), 1.0e-3 of the bound."""
import ctypes

import numpy as np
import pytest
import torch

import field_lattice as fl
import pose_twin as P
from guarded import Guarded, same_bits, under_fills, moved_with_fill

pytestmark = pytest.mark.gpu
f32 = np.float32
# (the kernel is instantiated for F in {2, 4, 8}: the last entry is the F = 4 instance, dense and hashed 3-D levels again)
MODELS = ["f2_h64_5x3d_5x2d", "f8_h160_5x3d_3x2d", "f2_h64_4x3d_2x2d_hashed", "f4_h64_6x3d_1x2d"]
SIZES = [1, 63, 64, 65, 257]
AABB = [-1.5, -1.0, -2.0, 1.5, 2.0, 1.0]
_MODELS = {}


def _model(cuda, name):
    """(field, its evaluator, the twin's model dict) — built once per composition."""
    if name not in _MODELS:
        from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
        e = fl.BY_NAME[name]
        torch.manual_seed(40 + MODELS.index(name))
        f = NGPRadianceField_mygrid_2D3D(aabb=AABB, **fl.kwargs_of(e)).to(cuda)
        with torch.no_grad():
            for enc in f.mlp_base._encoders():
                enc.params.uniform_(-1, 1)
        assert FusedFieldForward.shapes_ok(f)
        _MODELS[name] = (f, FusedFieldForward(f), fl.field_params(f), e)
    return _MODELS[name]


def _levels_are_mixed(e, params):
    table, offs, res = params["encoders"][0]
    dense = [int(r) ** 3 <= int(offs[l + 1] - offs[l]) for l, r in enumerate(res)]
    return any(dense) and not all(dense)


def _points(e, n, seed):
    """World positions [n, 3] cycling through the kinds of the module docstring, and the selector bytes."""
    rng = np.random.default_rng(seed)
    lo, ext = np.asarray(AABB[:3]), np.asarray(AABB[3:]) - np.asarray(AABB[:3])
    faces = (fl.boundary_points(e, aabb_min=0.0, aabb_ext=1.0).astype(np.float64)) * ext + lo      # unit cube -> this box
    pts, sel = [], []
    for i in range(n):
        kind = i % 6
        u = rng.uniform(0.02, 0.98, size=3)
        if kind == 1:
            p = faces[(i // 6) % len(faces)]
        else:
            if kind == 2:                                   # the border ring: the outermost cell of an axis, either end
                a = (i // 6) % 3
                u[a] = rng.uniform(0.002, 0.04) if (i // 18) % 2 == 0 else rng.uniform(0.96, 0.998)
            elif kind == 3:                                 # outside, or on a box face
                a = (i // 6) % 3
                u[a] = (-0.2, 1.3, 0.0, 1.0)[(i // 18) % 4]
            p = u * ext + lo
        pts.append(p)
        sel.append(0 if kind == 5 and (i // 6) % 2 == 0 else 1)
    world = np.asarray(pts).astype(f32)
    inside = P.unit_position(world, AABB)[1]
    return world, (np.asarray(sel, np.uint8) * inside).astype(np.uint8)


def _call(ff, cuda, bufs, n, ld_x, ld_s):
    from cnc_amd import _lib
    st, keep, _ = ff._descriptor(cuda, True)
    rc = _lib.lib().cnc_field_position_grad(ctypes.byref(st), bufs["pos"].ptr, bufs["sel"].ptr, bufs["dX"].ptr, ld_x,
                                            bufs["dS"].ptr, ld_s, n, bufs["g"].ptr, _lib.stream(cuda))
    torch.cuda.synchronize()
    return rc, keep


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_kernel_against_the_twin(cuda, name, n):
    f, ff, params, e = _model(cuda, name)
    if "hashed" not in name:
        assert _levels_are_mixed(e, params), "the 3-D grid must hold a dense and a hashed level"
    F, n_enc = e.F, fl.n_enc_of(e)
    world, sel = _points(e, n, seed=7 * n + MODELS.index(name))
    rng = np.random.default_rng(n)
    extra = 3                                               # rows of padding behind the N samples (the bucketed row count)
    ld_x, ld_s = (n_enc + 8) // 4 * 4, 64
    scale = np.exp(rng.normal(size=(n + extra, 1)) * 2.0 - 3.0)                   # gradients of very different sizes
    dX = (rng.normal(size=(n + extra, n_enc)) * scale).astype(f32)
    dS = (rng.normal(size=(n + extra, 63)) * scale * 0.1).astype(f32)
    selp = np.concatenate([sel, np.zeros(extra, np.uint8)])

    def build(fill):
        return dict(pos=Guarded(world, cuda, fill=fill), sel=Guarded(selp, cuda, fill=fill),
                    dX=Guarded.window(dX, ld_x, 0, cuda, fill=fill), dS=Guarded.window(dS, ld_s, 0, cuda, fill=fill),
                    g=Guarded.empty((n, 3), f32, cuda, fill=fill))

    def run(bufs):
        rc, _ = _call(ff, cuda, bufs, n, ld_x, ld_s)
        assert rc == 0

    res = under_fills(build, run)
    assert moved_with_fill(res) == [], "the result depends on bytes outside the kernel's inputs"
    got = res[0xA5]["g"]
    again = under_fills(build, run, fills=(0xA5,))[0xA5]["g"]
    assert same_bits(got, again), "two runs differ"
    want, mag = P.position_grad(params, AABB, world, sel, dX[:n].astype(np.float64), dS[:n].astype(np.float64))
    dead = sel == 0
    assert np.all(got[dead] == 0) and not np.signbit(got[dead]).any(), "a deselected row is not +0"
    err = np.abs(got.astype(np.float64) - want)
    live = mag > 0
    assert np.all(err[~live] == 0)
    worst = float((err[live] / mag[live]).max()) if live.any() else 0.0
    print(f"POSITION GRAD {name} n={n}: max |got - want| / sum|terms| = {worst:.3e}, live rows {int((~dead).sum())}")
    assert np.all(err <= 1e-4 * mag), (name, n, worst)
    if n >= 63:
        assert dead.sum() >= 5 and (~dead).sum() >= 40 and np.abs(want[~dead]).min() > 0
        x_unit = P.unit_position(world, AABB)[0]
        assert P.touches_border_ring(params, x_unit[~dead]).sum() >= 5
        assert (P.face_distance(params, x_unit[~dead]) < 1e-4).sum() >= 3, "no point on a cell face"


def test_arguments_are_checked(cuda):
    from cnc_amd import _lib
    f, ff, params, e = _model(cuda, MODELS[0])
    n, n_enc = 8, fl.n_enc_of(e)
    world, sel = _points(e, n, seed=1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    pos, selt = t(world), t(sel)
    dX, dS, g = torch.zeros(n, n_enc, device=cuda), torch.zeros(n, 64, device=cuda), torch.full((n, 3), 7.0, device=cuda)
    L = _lib.lib()

    def call(st, ld_x=n_enc, ld_s=64, dx=dX):
        return L.cnc_field_position_grad(ctypes.byref(st), pos.data_ptr(), selt.data_ptr(), dx.data_ptr(), ld_x, dS.data_ptr(),
                                         ld_s, n, g.data_ptr(), _lib.stream(cuda))
    st, keep, _ = ff._descriptor(cuda, True)
    assert call(st) == 0
    assert call(st, ld_x=n_enc - 4) == -1 and call(st, ld_x=n_enc + 1) == -1 and call(st, ld_s=62) == -1
    assert call(st, dx=dX.view(-1)[1:]) == -1                                   # not 16-byte aligned
    st.flags |= _lib.CNC_FIELD_CONTRACT
    assert call(st) == -2                                                       # bounded fields only
    torch.cuda.synchronize()


def test_unbounded_field_raises(cuda):
    from cnc_amd.field import FusedFieldForward, NGPRadianceField_mygrid_2D3D
    e = fl.BY_NAME[MODELS[0]]
    f = NGPRadianceField_mygrid_2D3D(aabb=AABB, unbounded=True, **fl.kwargs_of(e)).to(cuda)
    ff = FusedFieldForward(f)
    z = torch.zeros(4, 64, device=cuda)
    with pytest.raises(ValueError, match="bounded"):
        ff.position_grad(torch.zeros(4, 3, device=cuda), torch.ones(4, dtype=torch.uint8, device=cuda), z, z)
