"""Footprint of the aligner kernels (cnc_amd/csrc/aligner.hip and the segment reductions' backward in ctx_head.hip): every
result depends on the call's buffers alone.  int16 points (6-byte rows at D = 3), bool occupancy grids, int64 counts,
prefix sums, orders and resolution lists of exactly the stated length and float32 rows lie in guarded allocations
(tests/guarded.py) whose surroundings hold 0x00, 0xA5 and 0xFF in turn.  None of these kernels sums with atomics: every
output is the same bits under every fill, and equals the reference of the family's own tests — the CPU oracle bit for
bit (query_mask, align_and_pack), float64 sums at those tests' tolerances (the segment reductions).

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import numpy as np
import pytest
import torch

from conftest import ball_occupancy
from guarded import FILLS, Guarded, moved_with_fill, same_bits, under_fills
from test_gpu_context import SEGMENT_ATOL
from test_gpu_ctx_head import SEGMENT_BWD_TOL

pytestmark = pytest.mark.gpu
f32, i16, i32, i64 = np.float32, np.int16, np.int32, np.int64


def _pa():
    from cnc_amd.backends import pack_and_align as pa
    return pa


def _ragged(seed, n=37):
    """Counts with empty slots, a slot longer than a block, and their prefix sums (n + 1 entries)."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 9, size=n).astype(i64)
    cnt[::5] = 0
    cnt[3] = 288                                             # the reference's max collision count
    return rng, cnt, np.concatenate([[0], np.cumsum(cnt)]).astype(i64)


@pytest.mark.parametrize("qlist", [False, True], ids=["scalar", "qlist"])
@pytest.mark.parametrize("D,Rb", [(3, 12), (2, 32)])
def test_query_mask(cuda, oracle, D, Rb, qlist):
    N, R = 65, 59
    vxl = ball_occupancy(Rb, D, seed=R)
    rng = np.random.default_rng(R + Rb)
    rl = np.array([18, 24, 33, 44, 59], i64)[rng.integers(0, 5, size=N)] if qlist else None
    pts = (rng.uniform(size=(N, D)) * (rl[:, None] if qlist else R)).astype(i16)
    pts[:2] = [[0] * D, [(int(rl[1]) if qlist else R) - 1] * D]               # ring vertices
    want_m, want_o = oracle.query_mask(pts, vxl, resolution_list=rl) if qlist else oracle.query_mask(pts, vxl, resolution=R)

    def build(fill):
        return {"pts": Guarded(pts, cuda, fill=fill), "vxl": Guarded(vxl, cuda, fill=fill),
                "rl": Guarded(rl, cuda, fill=fill) if qlist else None,
                "mask": Guarded(np.zeros(N, i16), cuda, fill=fill).out(), "ov": Guarded(np.zeros(N, i32), cuda, fill=fill).out()}

    def run(b):
        if qlist:
            _pa().query_mask_3D_qlist(b["pts"].tensor(), b["vxl"].tensor(), b["mask"].tensor(), b["ov"].tensor(), b["rl"].tensor(), N)
        else:
            _pa().query_mask_3D(b["pts"].tensor(), b["vxl"].tensor(), b["mask"].tensor(), b["ov"].tensor(), R, N)

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    assert np.array_equal(res[FILLS[0]]["mask"], want_m) and np.array_equal(res[FILLS[0]]["ov"], want_o)
    assert want_m.max() == 1 and want_m.min() == 0


@pytest.mark.parametrize("F", [1, 8])
def test_align_and_pack(cuda, oracle, F):
    rng, cnt, cumsum = _ragged(F)
    N, M, T = cnt.shape[0], int(cnt.max()), int(cnt.sum())
    feat = rng.normal(size=(T, F)).astype(f32)
    dpk = rng.normal(size=(N, M, F)).astype(f32)
    want = oracle.align_and_pack_forward(feat, cnt, V=-7.0)
    want_b = oracle.align_and_pack_backward(dpk, cnt, T)

    def build(fill):
        return {"feat": Guarded(feat, cuda, fill=fill), "cnt": Guarded(cnt, cuda, fill=fill), "cum": Guarded(cumsum, cuda, fill=fill),
                "dpk": Guarded(dpk, cuda, fill=fill), "packed": Guarded.empty((N, M, F), f32, cuda, fill=fill),
                "d_feat": Guarded.empty((T, F), f32, cuda, fill=fill)}

    def run(b):
        t = {k: v.tensor() for k, v in b.items()}
        b["packed"].tensor().copy_(_pa().align_and_pack_forward(t["feat"], t["cnt"], t["cum"], N, M, F, -7.0, 3))
        b["d_feat"].tensor().copy_(_pa().align_and_pack_backward(t["dpk"], t["feat"], t["cnt"], t["cum"], N, M, F, T, 3))

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    assert same_bits(res[FILLS[0]]["packed"], want) and same_bits(res[FILLS[0]]["d_feat"], want_b)


def _segment_refs(v, w, cnt, mode, go):
    """float64: the reduction per slot and the gradient of sum(out * go) w.r.t. the values (ragged-row order)."""
    n = cnt.shape[0]
    slot = np.repeat(np.arange(n), cnt)
    w64 = np.ones(v.shape[0]) if w is None else w.astype(np.float64)
    num = np.zeros((n, v.shape[1]))
    np.add.at(num, slot, v.astype(np.float64) * w64[:, None])
    wsum = np.zeros(n)
    np.add.at(wsum, slot, w64)
    den = {0: np.ones(n), 1: wsum, 2: cnt.astype(np.float64)}[mode]
    nz = cnt > 0
    out = np.zeros_like(num)
    out[nz] = num[nz] / den[nz][:, None]
    scale = w64 / den[slot] if mode != 2 else 1.0 / den[slot]
    return out, nz, go.astype(np.float64)[slot] * scale[:, None], wsum.astype(f32)


@pytest.mark.parametrize("gathered", [False, True], ids=["plain", "gathered"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("F", [1, 8])
def test_segment_weighted_sum_and_its_backward(cuda, F, mode, gathered):
    """cnc_segment_weighted_sum{,_gathered}{,_backward} through the C ABI (the wrappers reach the gathered entries only).
    Empty slots: the forward's value there is the kernel's own (compared across fills, not with the reference)."""
    from cnc_amd import _lib
    L, st = _lib.lib(), _lib.stream(cuda)
    rng, cnt, cumsum = _ragged(10 * F + mode)
    n, T = cnt.shape[0], int(cnt.sum())
    v = rng.normal(size=(T, F)).astype(f32)
    w = None if mode == 2 else (rng.uniform(size=T) + 0.1).astype(f32)
    go = rng.normal(size=(n, F)).astype(f32)
    order = rng.permutation(T).astype(i64)
    inv = np.empty_like(order)
    inv[order] = np.arange(T)
    out64, nz, gv64, wsum = _segment_refs(v, w, cnt, mode, go)
    stored = v[inv] if gathered else v                       # stored[order[r]] = ragged row r

    def build(fill):
        return {"v": Guarded(stored, cuda, fill=fill), "w": None if w is None else Guarded(w, cuda, fill=fill),
                "cum": Guarded(cumsum, cuda, fill=fill), "order": Guarded(order, cuda, fill=fill) if gathered else None,
                "go": Guarded(go, cuda, fill=fill), "wsum": Guarded(wsum, cuda, fill=fill) if mode == 1 else None,
                "out": Guarded.empty((n, F), f32, cuda, fill=fill), "gv": Guarded.empty((T, F), f32, cuda, fill=fill)}

    def run(b):
        p = lambda k: b[k].ptr if k in b else None
        if gathered:
            _lib.check(L.cnc_segment_weighted_sum_gathered(p("v"), p("order"), p("w"), p("cum"), p("out"), n, F, mode, st), "fwd")
            _lib.check(L.cnc_segment_weighted_sum_gathered_backward(p("go"), p("order"), p("cum"), p("w"), p("wsum"), n, T, F, mode,
                                                                    p("gv"), st), "bwd")
        else:
            _lib.check(L.cnc_segment_weighted_sum(p("v"), p("w"), p("cum"), p("out"), n, F, mode, st), "fwd")
            _lib.check(L.cnc_segment_weighted_sum_backward(p("go"), p("cum"), p("w"), p("wsum"), n, T, F, mode, p("gv"), st), "bwd")

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    out, gv = res[FILLS[0]]["out"], res[FILLS[0]]["gv"]
    assert np.isfinite(out[nz]).all() and np.allclose(out[nz].astype(np.float64), out64[nz], rtol=0, atol=SEGMENT_ATOL[mode])
    gv = gv[order] if gathered else gv                        # the gradient of ragged row t is stored at order[t]
    assert np.isfinite(gv).all()                              # every row written: the 0xFF run's bits are these
    assert torch.allclose(torch.from_numpy(gv).double(), torch.from_numpy(gv64), **SEGMENT_BWD_TOL)
