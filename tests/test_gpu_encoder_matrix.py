"""The hash-grid encoder over the whole surface the C ABI accepts, against the CPU oracle.

D in {1, 2, 3} x F in {1, 2, 4, 8, 16, 32}, STE on and off, every backward route that applies to a shape (the run /
per-point kernels, the finest-first merge kernel, the cell-merging kernel with and without its x-neighbour carry, the
binned and the overlapped entries), at the resolutions where kernels go wrong:
  * tiny     R = 2, 3, 4: at R = 2 every corner is a border corner (output 0, no gradient), R = 3 / 4 have one / two
             interior vertices per axis;
  * boundary a dense level with R^D == T (no padding rows), one just above (hashed), a dense level whose R^D is not a
             multiple of 8 (padding rows that must stay 0);
  * production the trainer's 3-D and 2-D resolution lists on small tables (dense and hashed levels collide heavily);
  * large    R = 65535 ... 100003 (and 2^20 + 3 in 1-D): cell coordinates that do not fit 16 bits, with points placed
             in the top cells along every axis.
Every level of R > 2^16 has a table of 2^17 rows (np_twins.make_grid_wide), so that a row computed from coordinates
cut to 16 bits is another row on every axis; the constructed points check that they are.
Forward, dy_dx and the input backward are bit-exact; the embedding gradient lies within the float32 summation bound of
the oracle's float64 sums (tests/test_gpu_encoder.py `_check_bwd`) and rows nobody touches are exactly 0."""
import numpy as np
import pytest
import torch

import np_twins as tw
from conftest import ball_occupancy
from test_gpu_binned_backward import _bwd_binned
from test_gpu_encoder import _bwd_gpu, _check_bwd, _fwd_gpu, _points

pytestmark = pytest.mark.gpu

LARGE = [65535, 65536, 65537, 65538, 100003]
# (resolutions, log2 T) per class and dimension
CLASSES = {
    "tiny": {1: ([2, 3, 4], 12), 2: ([2, 3, 4], 12), 3: ([2, 3, 4], 12)},
    # T = 4096: 1001 / 63^2 / 15^3 dense with padding rows, 4096 / 64^2 / 16^3 exactly T, 4097 / 65^2 / 17^3 hashed
    "boundary": {1: ([1001, 4096, 4097], 12), 2: ([63, 64, 65], 12), 3: ([15, 16, 17], 12)},
    "production": {1: ([130, 258, 514, 1026], 10), 2: ([130, 258, 514, 1026], 15),
                   3: ([18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514], 14)},
    # (the levels of R > 2^16 get 2^17 rows: make_grid_wide)
    "large": {1: (LARGE + [(1 << 20) + 3], 12), 2: (LARGE, 12), 3: (LARGE, 12)},
}
# one grid per dimension with a level of every class, for the (D, F) matrix
MIXED = {1: ([2, 3, 1001, 4096, 4097, 65538, (1 << 20) + 3], 12),
         2: ([2, 3, 63, 64, 65, 130, 65538], 12),
         3: ([2, 3, 15, 16, 17, 33, 65538], 12)}
FS = [1, 2, 4, 8, 16, 32]


def _cells_route(D, F):
    return D in (2, 3) and F in (2, 4, 8)


def _routes(D, F):
    """Backward routes of the plain entry for a shape: the dispatcher's default (run kernel, or the per-point kernel when
    2^D F > 64), the finest-first order (the merge kernel for D = 3, F = 8), the cell-merging kernel (+ carry)."""
    r = ["default", "interleave"]
    return r + (["cells", "cells+carry"] if _cells_route(D, F) else [])


def _edge_points(D, res, offs, rng, per=6):
    """Points in the top cells of every level of `res` whose coordinates reach 2^16 - 1: the cells 65535, 65536,
    R - 3 and R - 2 along each axis in turn (the other axes anywhere), checked to land where they are meant to — and,
    for the cells 65536, that their level's table tells the cell from the one a 16-bit key would name."""
    pts = []
    for l, R in enumerate(res):
        if R < 65537:
            continue
        for d in range(D):
            for gd in sorted({65535, 65536, R - 3, R - 2}):
                if not 1 <= gd <= R - 2:
                    continue
                cells = rng.integers(1, R - 2, size=(per, D))
                cells[:, d] = gd
                if gd == 65536:
                    assert tw.cut_coordinate_moves_rows(cells, d, int(offs[l + 1] - offs[l]), R)
                pts.append(tw.points_in_cells(cells, R, rng))
        pts.append(tw.points_in_cells(np.full((per, D), R - 2), R, rng))      # top cell on all axes at once
    return np.concatenate(pts) if pts else np.zeros((0, D), np.float32)


def _inputs(D, res, offs, N, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([_points(N, D, seed), _edge_points(D, res, offs, rng)]).astype(np.float32)
    # shuffled, so that the constructed points share blocks with random ones (the edge cases of `_points` stay first)
    tail = x[16:]
    x[16:] = tail[rng.permutation(tail.shape[0])]
    return x


def _oracle_bwd(oracle, g, x, emb, offs, res, **kw):
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, res, want_acc64=True, **kw)
    _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, res, want_acc64=True, **kw)
    return want32, acc64, abs64


def _bwd_route(dev, g, x, emb, offs, res, route, vxl=None, mli=None, ste=False, vbits=False):
    if route != "interleave":
        return _bwd_gpu(dev, g, x, emb, offs, res, vxl=vxl, mli=mli, ste=ste, vbits=vbits,
                        route="runs" if route == "default" else route)
    from cnc_amd.backends import gridencoder_backend as be
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)
    L, N, F = g.shape
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=dev)
    Rb = 128 if vxl is None else vxl.shape[-1]
    be.grid_encode_backward(t(g), t(x), t(emb), t(offs), t(res), ge, N, x.shape[1], F, L, 0, Rb, None, None,
                            t(vxl), t(mli), ste_binary=ste, interleave_levels=True)
    torch.cuda.synchronize()
    return ge.cpu().numpy()


def _check_route(cuda, oracle, g, x, emb, offs, res, route, **kw):
    want32, acc64, abs64 = _oracle_bwd(oracle, g, x, emb, offs, res, binary_vxl=kw.get("vxl"),
                                       min_level_id=kw.get("mli"), ste_binary=kw.get("ste", False))
    got = _bwd_route(cuda, g, x, emb, offs, res, route, **kw)
    _check_bwd(got, want32, acc64, abs64, n_terms_max=x.shape[0] << x.shape[1])
    return got, abs64


def _forward_checks(cuda, oracle, x, emb, offs, resl, ste):
    """fp32 forward, sign-plane forward (STE), dy_dx and the input backward: all bit-exact."""
    from cnc_amd.backends import gridencoder_backend as be
    N, D = x.shape
    F, L = emb.shape[1], len(resl)
    t = lambda a: torch.as_tensor(a, device=cuda)
    want = oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=ste)
    assert np.array_equal(_fwd_gpu(cuda, x, emb, offs, resl, L, ste=ste), want)
    if ste:
        bits = be.pack_sign_bits(t(emb))
        out = torch.full((L, N, F), 7.0, device=cuda)
        be.grid_encode_forward_bits(t(x), bits, t(offs), t(resl), out, N, D, F, L, 128)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
    out = torch.empty((L, N, F), device=cuda)
    dy = torch.full((N, L, D, F), 7.0, device=cuda)
    be.grid_encode_forward(t(x), t(emb), t(offs), t(resl), out, N, D, F, L, 0, 128, 0.0, dy, None, None,
                           ste_binary=ste)
    torch.cuda.synchronize()
    want_dy = oracle.grid_dy_dx(x, emb, offs, resl, ste_binary=ste)
    assert np.array_equal(dy.cpu().numpy(), want_dy)
    assert np.array_equal(out.cpu().numpy(), want)
    g = np.random.default_rng(N + F).normal(size=(L, N, F)).astype(np.float32)
    ge, gi = torch.zeros(emb.shape, device=cuda), torch.full((N, D), 3.0, device=cuda)
    be.grid_encode_backward(t(g), t(x), t(emb), t(offs), t(resl), ge, N, D, F, L, 0, 128, dy, gi, None, None,
                            ste_binary=ste)
    torch.cuda.synchronize()
    assert np.array_equal(gi.cpu().numpy(), oracle.input_backward(g, want_dy))
    return want


# ---------------------------------------------------------------------------------------------------------------------
# the (D, F) matrix on one grid per dimension that holds every class of level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ste", [False, True], ids=["fp32", "ste"])
@pytest.mark.parametrize("F", FS)
@pytest.mark.parametrize("D", [1, 2, 3])
def test_matrix_forward_bits_and_dy_dx(cuda, oracle, D, F, ste):
    res, log2T = MIXED[D]
    offs, resl, emb = tw.make_grid_wide(res, log2T, D, F, seed=100 + 10 * D + F)
    x = _inputs(D, res, offs, 1500, seed=D * 100 + F)
    want = _forward_checks(cuda, oracle, x, emb, offs, resl, ste)
    assert np.all(want[0] == 0)                                  # R = 2: every corner is a border corner


MATRIX_BWD = [pytest.param(D, F, route, id=f"D{D}-F{F}-{route}") for D in (1, 2, 3) for F in FS for route in _routes(D, F)]


@pytest.mark.parametrize("ste", [False, True], ids=["fp32", "ste"])
@pytest.mark.parametrize("D,F,route", MATRIX_BWD)
def test_matrix_backward(cuda, oracle, D, F, route, ste):
    res, log2T = MIXED[D]
    offs, resl, emb = tw.make_grid_wide(res, log2T, D, F, seed=200 + 10 * D + F)
    x = _inputs(D, res, offs, 2000, seed=D * 1000 + F)
    g = np.random.default_rng(7 + F).normal(size=(len(res), x.shape[0], F)).astype(np.float32)
    got, abs64 = _check_route(cuda, oracle, g, x, emb, offs, resl, route, ste=ste)
    assert np.all(got[offs[0]:offs[1]] == 0)                     # R = 2: no corner is ever valid
    assert np.abs(got[offs[-2]:offs[-1]]).sum() > 0              # the large level did receive gradient
    if ste:
        assert np.all(got[np.abs(emb) > 1] == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the resolution classes, one grid each, on the shapes whose kernels differ
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 8), (3, 2), (2, 16), (2, 4), (1, 32), (1, 4)]      # 2^D F == 64 (rows rebuilt from the cell) and < 64
CLASS_BWD = [pytest.param(cls, D, F, route, id=f"{cls}-D{D}-F{F}-{route}")
             for cls in CLASSES for D, F in SHAPES for route in _routes(D, F)]


def _class_case(cls, D, F, seed):
    res, log2T = CLASSES[cls][D]
    offs, resl, emb = tw.make_grid_wide(res, log2T, D, F, seed=seed)
    x = _inputs(D, res, offs, 3000 if cls != "production" else 2000, seed=seed + 1)
    return res, offs, resl, emb, x


def _padding_rows(res, offs, D):
    """(first, last) table rows of every dense level that lie past its R^D vertices."""
    return [(int(offs[l]) + R ** D, int(offs[l + 1])) for l, R in enumerate(res) if R ** D < offs[l + 1] - offs[l]]


@pytest.mark.parametrize("cls", list(CLASSES))
@pytest.mark.parametrize("D,F", SHAPES)
def test_class_forward_bits_and_dy_dx(cuda, oracle, cls, D, F):
    res, offs, resl, emb, x = _class_case(cls, D, F, seed=300 + 10 * D + F)
    for ste in (False, True):
        want = _forward_checks(cuda, oracle, x, emb, offs, resl, ste)
        if cls == "tiny":
            assert np.all(want[0] == 0) and np.any(want[1] != 0)


@pytest.mark.parametrize("ste", [False, True], ids=["fp32", "ste"])
@pytest.mark.parametrize("cls,D,F,route", CLASS_BWD)
def test_class_backward(cuda, oracle, cls, D, F, route, ste):
    res, offs, resl, emb, x = _class_case(cls, D, F, seed=400 + 10 * D + F)
    g = np.random.default_rng(401).normal(size=(len(res), x.shape[0], F)).astype(np.float32)
    got, abs64 = _check_route(cuda, oracle, g, x, emb, offs, resl, route, ste=ste)
    if cls == "tiny":
        assert np.all(got[offs[0]:offs[1]] == 0)
    if cls == "boundary":
        pads = _padding_rows(res, offs, D)
        assert pads and all(np.all(got[a:b] == 0) for a, b in pads)
        exact = [l for l, R in enumerate(res) if R ** D == offs[l + 1] - offs[l]]
        assert exact                                             # a level with R^D == T and no padding
    if cls == "large":
        for l in range(len(res)):
            assert np.abs(got[offs[l]:offs[l + 1]]).sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# occupancy mask and per-point level windows (the cell-merging kernel's calls), with large levels in the windows
# ---------------------------------------------------------------------------------------------------------------------
MASKED = {1: ([6, 70, 1001, 65536, 65538, 100003], 10, 4), 2: ([10, 34, 66, 65536, 65538, 100003], 10, 8),
          3: ([6, 14, 31, 65536, 65538, 100003], 10, 8)}
MASK_CASES = [pytest.param(D, mode, vbits, route, id=f"D{D}-{mode}-{'vbits' if vbits else 'scan'}-{route}")
              for D in (1, 2, 3) for mode in ("mask", "levels", "mask+levels")
              for vbits in ((False, True) if "mask" in mode else (False,))
              for route in (["default", "cells", "cells+carry"] if D > 1 else ["default", "interleave"])]


@pytest.mark.parametrize("D,mode,vbits,route", MASK_CASES)
def test_masked_and_per_point_levels(cuda, oracle, D, mode, vbits, route):
    res, log2T, F = MASKED[D]
    offs, resl, emb = tw.make_grid_wide(res, log2T, D, F, seed=500 + D)
    emb[::7] *= 3.0                                              # parameters outside [-1, 1]: the STE mask is live
    x = _inputs(D, res, offs, 2500, seed=501 + D)
    rng = np.random.default_rng(502)
    vxl = ball_occupancy(16 if D == 3 else 32, D, radius=0.45) if "mask" in mode else None
    mli = None
    L = len(res)
    if "levels" in mode:
        L = 3
        mli = rng.integers(0, len(res) - L + 1, size=x.shape[0]).astype(np.int32)
        mli[: x.shape[0] // 3] = len(res) - L                    # a third on the three finest levels (all large)
    kw = dict(binary_vxl=vxl, min_level_id=mli, ste_binary=True)
    want = oracle.grid_encode_forward(x, emb, offs, resl, n_levels_calc=L, **kw)
    assert np.array_equal(_fwd_gpu(cuda, x, emb, offs, resl, L, vxl=vxl, mli=mli, ste=True, vbits=vbits), want)
    g = rng.normal(size=(L, x.shape[0], F)).astype(np.float32)
    g[:, rng.random(x.shape[0]) < 0.1] = 0                       # points without gradient
    got, abs64 = _check_route(cuda, oracle, g, x, emb, offs, resl, route, vxl=vxl, mli=mli, ste=True, vbits=vbits)
    assert np.all(got[np.abs(emb) > 1] == 0)
    assert np.abs(got[offs[-2]:offs[-1]]).sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# adversarial layouts for keys that pack a cell into 16 bits per axis
# ---------------------------------------------------------------------------------------------------------------------
def _key16(cell):
    """The cell key as the 16-bit packing forms it: x | y << 16 | z << 32, with each coordinate OR-ed in unmasked."""
    k = 0
    for gd in reversed([int(c) for c in cell]):
        k = (k << 16) | gd
    return k


def _pair_points(D, R, first, second, n, seed, at=(100, 300, 612, 1000, 1500)):
    """n random points with the constructed pairs (first[i], second[i]) placed consecutively at the offsets `at`, none
    straddling a 256-point block."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.02, 0.98, size=(n, D)).astype(np.float32)
    pa, pb = tw.points_in_cells(first, R, rng), tw.points_in_cells(second, R, rng)
    for i, p in enumerate(at):
        assert p % 256 != 255
        x[p], x[p + 1] = pa[i], pb[i]
    return x


ALIAS = [pytest.param(D, F, route, id=f"D{D}-F{F}-{route}")
         for D, F in [(3, 8), (3, 2), (2, 16), (2, 4), (2, 8)] for route in _routes(D, F)]


@pytest.mark.parametrize("D,F,route", ALIAS)
def test_key_alias_pair(cuda, oracle, D, F, route):
    """Cells (65536, y) and (0, y | 1), y even, next to each other in one block: the same key once the x coordinate
    overflows into the y field.  A kernel that merges them sends both points' gradient to one cell's rows — the kernels
    that keep the head point's rows (2^D F < 64) do too, which a single point would not show."""
    R = 65538
    res = [17, R]
    offs, resl, emb = tw.make_grid_wide(res, 12, D, F, seed=600 + D * 10 + F)
    rng = np.random.default_rng(601)
    n = 5
    first = rng.integers(1, R - 2, size=(n, D))
    first[:, 0] = 65536
    first[:, 1] = (first[:, 1] // 2) * 2
    second = first.copy()
    second[:, 0] = 0
    second[:, 1] |= 1
    for a, b in zip(first, second):
        assert _key16(a) == _key16(b) and tuple(a) != tuple(b)
    assert tw.cut_coordinate_moves_rows(first, 0, int(offs[2] - offs[1]), R)
    x = _pair_points(D, R, first, second, 2048, seed=602)
    g = rng.normal(size=(len(res), x.shape[0], F)).astype(np.float32)
    _check_route(cuda, oracle, g, x, emb, offs, resl, route)


@pytest.mark.parametrize("R", [65537, 65538])
@pytest.mark.parametrize("D,F", [(3, 8), (2, 4), (2, 8)])
def test_carry_wrap_pair(cuda, oracle, D, F, R):
    """Cells (65535, y) and (0, y + 1) in one block: the cell kernel's x-neighbour probe (key + 1) carries from x into y
    and finds the second cell as the first one's right-hand neighbour.  At R = 65537 the upper x corners of x = 65535
    are border vertices (x + 1 = R - 1), so nothing is shared; at 65538 they are live."""
    res = [17, R]
    offs, resl, emb = tw.make_grid_wide(res, 12, D, F, seed=700 + D * 10 + F)
    rng = np.random.default_rng(701)
    n = 5
    first = rng.integers(1, R - 3, size=(n, D))
    first[:, 0] = 65535
    second = first.copy()
    second[:, 0] = 0
    second[:, 1] += 1
    for a, b in zip(first, second):
        assert _key16(a) + 1 == _key16(b)
    x = _pair_points(D, R, first, second, 2048, seed=702)
    g = rng.normal(size=(len(res), x.shape[0], F)).astype(np.float32)
    _check_route(cuda, oracle, g, x, emb, offs, resl, "cells+carry")


# ---------------------------------------------------------------------------------------------------------------------
# binned and overlapped entries with large levels (D = 3)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["binned_large", "coarse_large"])
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("ste", [False, True], ids=["fp32", "ste"])
def test_binned_entry_with_large_levels(cuda, oracle, F, case, ste):
    """n_binned = 2 finest levels through the bin / owner passes, the rest through the finest-first atomic call (the
    merge kernel at F = 8): a binned level of R = 100003 / 65538, or a coarse level of R = 65538."""
    res = [6, 31, 65538, 100003] if case == "binned_large" else [6, 65538, 31, 44]
    offs, resl, emb = tw.make_grid_wide(res, 12, 3, F, seed=800 + F)
    x = _inputs(3, res, offs, 6000, seed=801)
    g = np.random.default_rng(802).normal(size=(len(res), x.shape[0], F)).astype(np.float32)
    want32, acc64, abs64 = _oracle_bwd(oracle, g, x, emb, offs, resl, ste_binary=ste)
    level_rows = int(np.diff(offs)[-2:].max())                  # 2^17 rows for the R > 2^16 levels
    got = _bwd_binned(cuda, g, x, emb, offs, resl, 2, level_rows, ste=ste)
    _check_bwd(got, want32, acc64, abs64, n_terms_max=x.shape[0] * 8)


def test_overlapped_entry_with_a_large_coarse_level(cuda, oracle):
    """cnc_grid_encode_backward_overlapped straight through the C ABI, N >= 2^16 (the overlapped path proper): the coarse
    levels, one of them R = 65538, on the merge kernel next to the binned R = 100003 level on a side stream."""
    import ctypes as C

    from cnc_amd import _lib
    F, res = 8, [18, 65538, 44, 100003]
    offs, resl, emb = tw.make_grid_wide(res, 12, 3, F, seed=900)
    x = _inputs(3, res, offs, (1 << 16) + 77, seed=901)
    N, L = x.shape[0], len(res)
    g = np.random.default_rng(902).normal(size=(L, N, F)).astype(np.float32)
    want32, acc64, abs64 = _oracle_bwd(oracle, g, x, emb, offs, resl, ste_binary=True)
    lib = _lib.lib()
    t = lambda a: torch.as_tensor(a, device=cuda)
    gd, xd, ed, od, rd = t(g), t(x), t(emb), t(offs), t(resl)
    p = lambda a: C.c_void_p(a.data_ptr())
    plan = C.c_void_p()
    assert lib.cnc_backward_plan_create(C.byref(plan)) == 0 and plan.value
    level_rows = int(offs[-1] - offs[-2])
    assert level_rows == 1 << 17
    nbytes = int(lib.cnc_grid_encode_backward_overlapped_workspace(N, 1, level_rows))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=cuda)
    rc = lib.cnc_grid_encode_backward_overlapped(plan, p(gd), p(xd), p(ed), p(od), p(rd), p(ge), N, 3, F, L,
                                                 _lib.CNC_FLAG_STE_BINARY, None, 0, 0, 1, level_rows, p(ws), nbytes,
                                                 _lib.stream(cuda))
    torch.cuda.synchronize()
    assert lib.cnc_backward_plan_destroy(plan) == 0
    assert rc == 0
    _check_bwd(ge.cpu().numpy(), want32, acc64, abs64, n_terms_max=N * 8)
