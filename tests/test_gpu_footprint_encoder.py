"""Footprint of the hash-grid encoder (cnc_amd/csrc/grid_encode*.hip): every result depends on the call's buffers alone.
Points ([N, 3]: 12-byte rows), tables, sign planes, level tables (`offsets` of exactly L + 1 entries), gradients, masks,
summed-volume tables and vertex bit planes lie in guarded allocations (tests/guarded.py) whose surroundings hold 0x00,
0xA5 and 0xFF in turn.

  * forward (fp32 and STE), the sign-plane forward with and without the paired word gathers (encoder_common.hpp argues
    that the aligned word "never leaves the level's plane": here the plane ends where the poison begins, down to one word
    per level, and once more four bytes off its alignment) and cnc_grid_vertex_bits: the same bits under every fill, and
    the oracle's bits;
  * the ordered backward: the same bits under every fill, and the serial oracle's bits;
  * the atomic routes (default, binned, overlapped, cell-merging on a masked call): under each fill on its own, finite
    and within the float64-shadow bound of tests/test_gpu_encoder.py `_check_bwd`;
  * every backward route twice: the gradient as a contiguous [L, N, F] tensor, and read in place (grad_ld / grad_col)
    from a column window of a wider [N, ld] matrix whose other columns hold the fill.

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import numpy as np
import pytest
import torch

from conftest import ball_occupancy, make_grid
from guarded import FILLS, Guarded, moved_with_fill, same_bits, under_fills
from test_gpu_binned_backward import RES as RES_BINNED
from test_gpu_encoder import RES2, RES3, _check_bwd, _points
from test_gpu_forward_pair_gather import RES as RES_PAIR, _cell_points, _table

pytestmark = pytest.mark.gpu
f32, i32 = np.float32, np.int32
_ORACLE = {}


def _be():
    from cnc_amd.backends import gridencoder_backend as be
    return be


def _once(key, fn):
    """An oracle result, computed once and shared (never modified)."""
    if key not in _ORACLE:
        _ORACLE[key] = fn()
    return _ORACLE[key]


def _grid_bufs(x, emb, offs, resl, cuda, fill):
    assert offs.shape == (len(resl) + 1,) and offs.dtype == i32 and resl.dtype == i32
    return {"x": Guarded(x, cuda, fill=fill), "emb": Guarded(emb, cuda, fill=fill), "offs": Guarded(offs, cuda, fill=fill),
            "res": Guarded(resl, cuda, fill=fill)}


# ----------------------------------------------------------------------------------------------------------------------
# cnc_grid_encode_forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 65])
@pytest.mark.parametrize("ste", [False, True], ids=["fp32", "ste"])
@pytest.mark.parametrize("F", [2, 8])
@pytest.mark.parametrize("D", [2, 3])
def test_forward(cuda, oracle, D, F, ste, N):
    res = RES3 if D == 3 else RES2
    L = len(res)
    offs, resl, emb = make_grid(res, 10, D, F, seed=F)
    x = _points(65, D, seed=D * 10 + F)[:N] if N > 1 else _points(65, D, seed=D * 10 + F)[20:21]
    want = _once(("fwd", D, F, ste, N), lambda: oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=ste))

    def build(fill):
        return dict(_grid_bufs(x, emb, offs, resl, cuda, fill), out=Guarded.empty((L, N, F), f32, cuda, fill=fill))

    def run(b):
        _be().grid_encode_forward(b["x"].tensor(), b["emb"].tensor(), b["offs"].tensor(), b["res"].tensor(),
                                  b["out"].tensor(), N, D, F, L, 0, 128, 0.0, None, None, None, ste_binary=ste)

    res_ = under_fills(build, run)
    assert moved_with_fill(res_) == []
    assert same_bits(res_[FILLS[0]]["out"], want)


# ----------------------------------------------------------------------------------------------------------------------
# cnc_grid_encode_forward_bits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4])
@pytest.mark.parametrize("lut", [0, 1])
@pytest.mark.parametrize("pair", [0, 2])
@pytest.mark.parametrize("log2_rows", [3, 10])
def test_forward_bits(cuda, oracle, monkeypatch, log2_rows, pair, lut, shift):
    D, F = 3, 8
    res = RES_PAIR[log2_rows]
    L = len(res)
    offs, resl, emb = _table(res, log2_rows, D, F, seed=300 + log2_rows + D)
    x = _cell_points(res, D, seed=11 * log2_rows + D)[-257:]                  # cells of the finest levels, g % 8 == 7 among them
    N = x.shape[0]
    want = _once(("bits", log2_rows), lambda: oracle.grid_encode_forward(x, emb, offs, resl, ste_binary=True))
    plane = _be().pack_sign_bits(torch.as_tensor(emb, device=cuda)).cpu().numpy()
    assert plane.shape == (int(offs[-1]) * F // 8,) and (log2_rows != 3 or plane.size == 8 * L)      # one word per level
    monkeypatch.setenv("CNC_FWD_PAIR", str(pair))
    monkeypatch.setenv("CNC_FWD_LUT", str(lut))

    def build(fill):
        b = _grid_bufs(x, emb, offs, resl, cuda, fill)
        del b["emb"]
        return dict(b, bits=Guarded(plane, cuda, shift, fill), out=Guarded.empty((L, N, F), f32, cuda, fill=fill))

    def run(b):
        assert b["bits"].tensor().data_ptr() % 16 == shift
        _be().grid_encode_forward_bits(b["x"].tensor(), b["bits"].tensor(), b["offs"].tensor(), b["res"].tensor(),
                                       b["out"].tensor(), N, D, F, L, 128)

    res_ = under_fills(build, run)
    assert moved_with_fill(res_) == []
    assert same_bits(res_[FILLS[0]]["out"], want)


# ----------------------------------------------------------------------------------------------------------------------
# cnc_grid_vertex_bits, and the plane in one masked forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [14, 31])
def test_vertex_bits_plane_and_a_masked_forward(cuda, oracle, R):
    from cnc_amd import _lib
    D, F, Rb, N = 3, 8, 16, 65
    assert R ** D % 64 != 0
    n_words = int(_lib.lib().cnc_grid_vertex_bits_words(D, R))
    assert n_words == (R ** D + 63) // 64 * 2
    offs, resl, emb = make_grid([R], 10, D, F, seed=R)
    vxl = ball_occupancy(Rb, D)
    sat = _be().occupancy_sat(torch.as_tensor(vxl)).numpy()
    x = _points(N, D, seed=R)
    want = _once(("vbits", R), lambda: oracle.grid_encode_forward(x, emb, offs, resl, binary_vxl=vxl, ste_binary=True))
    assert np.any(want != 0) and np.any(np.all(want[0] == 0, axis=1))

    def build(fill):
        return dict(_grid_bufs(x, emb, offs, resl, cuda, fill), vxl=Guarded(vxl, cuda, fill=fill), sat=Guarded(sat, cuda, fill=fill),
                    vb_offs=Guarded(np.zeros(1, i32), cuda, fill=fill), words=Guarded.empty((n_words,), i32, cuda, fill=fill),
                    out=Guarded.empty((1, N, F), f32, cuda, fill=fill))

    def run(b):
        _lib.check(_lib.lib().cnc_grid_vertex_bits(b["sat"].ptr, D, Rb, R, b["words"].ptr, _lib.stream(cuda)), "grid_vertex_bits")
        _be().grid_encode_forward(b["x"].tensor(), b["emb"].tensor(), b["offs"].tensor(), b["res"].tensor(), b["out"].tensor(),
                                  N, D, F, 1, 0, Rb, 0.0, None, b["vxl"].tensor(), None, ste_binary=True,
                                  occ_sat=b["sat"].tensor(), vertex_bits=(b["words"].tensor(), b["vb_offs"].tensor()))

    res_ = under_fills(build, run)
    assert moved_with_fill(res_) == []                    # the plane too: its last word's bits past R^D are the kernel's
    assert same_bits(res_[FILLS[0]]["out"], want)
    words = res_[FILLS[0]]["words"].view(np.uint32)
    flags = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert flags.size == 32 * n_words and flags[:R ** D].any() and not flags[R ** D:].any()      # nothing set past the last vertex
    # the same plane as the wrapper builds it
    ref_words, _ = _be().occupancy_vertex_bits(torch.as_tensor(vxl, device=cuda), torch.as_tensor(sat, device=cuda), [R])
    assert same_bits(words, ref_words.cpu().numpy().view(np.uint32)[:n_words])


# ----------------------------------------------------------------------------------------------------------------------
# backward routes
# ----------------------------------------------------------------------------------------------------------------------
def _bwd_case(oracle, F, N, masked):
    D = 3
    offs, resl, emb = make_grid(RES_BINNED, 10, D, F, seed=41)
    emb[::7] *= 3.0                                             # parameters outside [-1, 1]: the STE mask is live
    x = _points(257, D, seed=42)[:N] if N > 1 else _points(257, D, seed=42)[20:21]
    g = np.random.default_rng(43).normal(size=(len(RES_BINNED), N, F)).astype(f32)
    vxl = ball_occupancy(16, D, radius=0.45) if masked else None
    ste = masked

    def refs():
        kw = dict(binary_vxl=vxl, ste_binary=ste)
        want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, resl, want_acc64=True, **kw)
        _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, resl, want_acc64=True, **kw)
        serial = oracle.grid_encode_backward(g, x, emb, offs, resl, threads=1, **kw)
        return want32, acc64, abs64, serial
    return offs, resl, emb, x, g, vxl, ste, _once(("bwd", F, N, masked), refs)


BWD = [pytest.param(F, N, route, layout, id=f"F{F}-N{N}-{route}-{layout}")
       for F, Ns in ((8, (1, 65, 257)), (2, (65,))) for N in Ns
       for route in ("default", "binned", "overlapped", "ordered", "cells_masked", "ordered_masked")
       for layout in ("level_major", "point_major")]


@pytest.mark.parametrize("F,N,route,layout", BWD)
def test_backward_routes(cuda, oracle, F, N, route, layout):
    """`level_major`: the gradient as a contiguous [L, N, F] tensor.  `point_major`: read in place from columns
    [4, 4 + L F) of an [N, L F + 8] matrix (grad_ld / grad_col, the layout of tests/test_gpu_binned_backward.py) whose
    other columns hold the fill: a route that reads into the gap between two gradient rows sees poison."""
    from cnc_amd import _lib
    D, L = 3, len(RES_BINNED)
    masked = route.endswith("_masked")
    offs, resl, emb, x, g, vxl, ste, (want32, acc64, abs64, serial) = _bwd_case(oracle, F, N, masked)
    n_binned, level_rows = 3, 1024
    ws_bytes = int(_lib.lib().cnc_grid_encode_backward_binned_workspace(N, n_binned, level_rows))
    ld, col = (L * F + 8, 4) if layout == "point_major" else (0, 0)
    g_rows = np.ascontiguousarray(g.transpose(1, 0, 2).reshape(N, L * F))

    def build(fill):
        b = dict(_grid_bufs(x, emb, offs, resl, cuda, fill),
                 g=Guarded.window(g_rows, ld, col, cuda, fill) if ld else Guarded(g, cuda, fill=fill),
                 ge=Guarded(np.zeros(emb.shape, f32), cuda, fill=fill).out(),
                 vxl=Guarded(vxl, cuda, fill=fill) if masked else None)
        if route == "binned":                                 # the C ABI, as tests/test_gpu_binned_backward.py calls it
            b["ws"] = Guarded.empty((max(ws_bytes, 4),), np.uint8, cuda, fill=fill).scratch()
        return b

    def run(b):
        t = {k: v.tensor() for k, v in b.items()}
        g_all = b["g"].whole()                                # the [N, ld] matrix, gap columns included, or [L, N, F]
        assert g_all.is_contiguous() and g_all.data_ptr() == b["g"].ptr - 4 * col
        args = (g_all, t["x"], t["emb"], t["offs"], t["res"], t["ge"], N, D, F, L, 0, 16 if masked else 128, None, None,
                t.get("vxl"), None)
        kw = dict(grad_ld=ld, grad_col=col)
        if route == "binned":
            _lib.check(_lib.lib().cnc_grid_encode_backward_binned(
                g_all.data_ptr(), b["x"].ptr, b["emb"].ptr, b["offs"].ptr, b["res"].ptr, b["ge"].ptr, N, D, F, L, 0, None, ld, col,
                n_binned, level_rows, b["ws"].ptr, ws_bytes, _lib.stream(cuda)), "binned")
        elif route == "overlapped":
            # (CNC_BWD_OVERLAP=0 would send this call to the binned entry: the route named in the id must be the one that ran)
            assert _be()._OVERLAP_ENABLED, "the overlapped entry is switched off in this environment"
            _be().grid_encode_backward(*args, ordered=False, binned=(n_binned, level_rows), overlap_streams=True, **kw)
        elif route.startswith("ordered"):
            before = _be().ROUTE_CALLS["ordered"]
            _be().grid_encode_backward(*args, ste_binary=ste, ordered=True, **kw)
            assert _be().ROUTE_CALLS["ordered"] == before + 1
        else:
            _be().grid_encode_backward(*args, ste_binary=ste, ordered=False, cell_merge=route == "cells_masked", **kw)

    res_ = under_fills(build, run)
    if route.startswith("ordered"):
        assert moved_with_fill(res_) == []
        assert same_bits(res_[FILLS[0]]["ge"], serial)
    for fill in FILLS:
        got = res_[fill]["ge"]
        assert np.isfinite(got).all(), fill
        _check_bwd(got, want32, acc64, abs64, n_terms_max=N * 8)
        if ste:
            assert np.all(got[np.abs(emb) > 1] == 0)
    assert np.count_nonzero(serial) > 0
