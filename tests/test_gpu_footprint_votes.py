"""Footprint of the vote kernels (cnc_amd/csrc/cnt_votes.hip and the atomic cnc_cnt_np_embed pair): every result depends
on the call's buffers alone.  The int16 vertex list (6-byte rows), the bool occupancy grid (Rb = 6: rows of 6 bytes, not
a multiple of the 16-byte loads), tables, counts and gradients lie in guarded allocations (tests/guarded.py) whose
surroundings hold 0x00, 0xA5 and 0xFF in turn; what a `VotePlan` allocates for itself stays as it is.

Counts are integers (exact in fp32, atomics or not) and the planned kernels sum without atomics: the same bits under
every fill, the oracle's counts, gradients within the float64-shadow bound of tests/test_gpu_encoder.py.  The atomic
backward is held to that bound under each fill on its own.

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import numpy as np
import pytest
import torch

from guarded import FILLS, Guarded, moved_with_fill, same_bits, under_fills
from test_gpu_context_matrix import FRACTION_U, U, _vertex_set
from test_gpu_encoder import vote_backward_bound

pytestmark = pytest.mark.gpu
f32, i16 = np.float32, np.int16
RB, T_UP, LOG2T = 6, 2, 10                         # R = 14: 14^3 vertices hashed into 2^10 rows
R, HS, S = RB * T_UP + 2, 2 ** LOG2T, RB * T_UP
_CASE = {}


def _be():
    from cnc_amd.backends import gridencoder_backend as be
    return be


def _case(oracle, F):
    """Occupancy touching the box faces, its vertex list, a table with "no" votes that are not -1, and the oracle's counts
    and float64 gradients per plane: computed once per F."""
    if F not in _CASE:
        rng = np.random.default_rng(F)
        occ = rng.uniform(size=(RB, RB, RB)) < 0.15
        occ[0, 0, :] = True
        occ[-1, :, -1] = True
        pts = _vertex_set(torch.as_tensor(occ), T_UP).numpy()
        emb = np.where(rng.uniform(size=(HS, F)) < 0.5, 1.0, -1.0).astype(f32)
        emb[::5] *= 0.5
        want = [oracle.cnt_np_embed(pts, emb, R, HS, axis) for axis in range(3)]
        sums = [(w.sum(-1, keepdims=True) + 1e-6).astype(f32) for w in want]
        grads = [rng.normal(size=w.shape).astype(f32) for w in want]
        acc, absacc = [], []
        for axis in range(3):
            acc.append(oracle.cnt_np_embed_backward(pts, emb, sums[axis], grads[axis], R, HS, axis, want_acc64=True)[1])
            absacc.append(oracle.cnt_np_embed_backward(pts, emb, sums[axis], np.abs(grads[axis]), R, HS, axis, want_acc64=True)[1])
        gos = [(np.float32(1.0) / s * g).astype(f32) for s, g in zip(sums, grads)]        # grad / sum, as the planned entries take it
        _CASE[F] = dict(occ=occ, pts=pts, emb=emb, want=want, sums=sums, grads=grads, acc=acc, absacc=absacc, gos=gos)
    return _CASE[F]


def _within(got, acc, absacc):
    return np.isfinite(got).all() and np.all(np.abs(got.astype(np.float64) - acc) <= vote_backward_bound(absacc))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("F", [2, 8])
def test_atomic_votes(cuda, oracle, F, axis):
    c = _case(oracle, F)
    N = c["pts"].shape[0]

    def build(fill):
        return {"pts": Guarded(c["pts"], cuda, fill=fill), "emb": Guarded(c["emb"], cuda, fill=fill),
                "s": Guarded(c["sums"][axis], cuda, fill=fill), "g": Guarded(c["grads"][axis], cuda, fill=fill),
                "out": Guarded(np.zeros((S, S, F, 2), f32), cuda, fill=fill).out(),
                "ge": Guarded(np.zeros((HS, F), f32), cuda, fill=fill).out()}

    def run(b):
        t = {k: v.tensor() for k, v in b.items()}
        _be().cnt_np_embed(t["pts"], t["emb"], t["out"], N, R, F, HS, axis)
        _be().cnt_np_embed_backward(t["pts"], t["emb"], t["s"], t["g"], t["ge"], N, R, F, HS, axis)

    res = under_fills(build, run)
    for fill in FILLS:
        assert same_bits(res[fill]["out"], c["want"][axis])               # integer counts: exact in any order
        assert _within(res[fill]["ge"], c["acc"][axis], c["absacc"][axis]), fill


@pytest.mark.parametrize("form", ["list", "occupancy"])
@pytest.mark.parametrize("F", [2, 8])
def test_planned_votes(cuda, oracle, F, form):
    """cnc_cnt_np_plan3 (the list) or cnc_vote_plan_count / _fill (the occupancy) build the plan from a guarded input;
    cnc_cnt_vote_masks + cnc_cnt_np_embed_planned_masked, cnc_cnt_np_embed_planned (through the C ABI: the wrapper takes
    the masked entry), cnc_cnt_np_embed_planned_backward and _backward3{,_xyz} consume it."""
    from cnc_amd import _lib
    c = _case(oracle, F)
    rows = min(HS, R ** 3)
    emb = c["emb"][:rows].copy()

    def build(fill):
        b = {"src": Guarded(c["pts"] if form == "list" else c["occ"], cuda, fill=fill), "emb": Guarded(emb, cuda, fill=fill),
             "ge3": Guarded.empty((rows, F), f32, cuda, fill=fill)}
        for axis in range(3):
            b[f"gos{axis}"] = Guarded(c["gos"][axis], cuda, fill=fill)
            b[f"out{axis}"] = Guarded.empty((S, S, F, 2), f32, cuda, fill=fill)
            b[f"plain{axis}"] = Guarded.empty((S, S, F, 2), f32, cuda, fill=fill)
            b[f"ge{axis}"] = Guarded(np.zeros((rows, F), f32), cuda, fill=fill).out()
        return b

    def run(b):
        be = _be()
        plan = be.VotePlan(b["src"].tensor(), R, HS) if form == "list" else be.VotePlan.from_occupancy(b["src"].tensor(), T_UP, R, HS)
        assert (plan.xyz_by_row is None) == (form == "list")
        e = b["emb"].tensor()
        for axis in range(3):
            be.cnt_np_embed_planned(plan, e, b[f"out{axis}"].tensor(), F, axis)
            _lib.check(_lib.lib().cnc_cnt_np_embed_planned(plan.rows_by_pixel[axis].data_ptr(), plan.pixel_seg[axis].data_ptr(),
                                                           b["emb"].ptr, b[f"plain{axis}"].ptr, plan.n_pixels, F, _lib.stream(cuda)),
                       "cnt_np_embed_planned")
            be.cnt_np_embed_planned_backward(plan, e, b[f"gos{axis}"].tensor(), b[f"ge{axis}"].tensor(), F, axis)
        be.cnt_np_embed_planned_backward3(plan, e, [b[f"gos{axis}"].tensor() for axis in range(3)], b["ge3"].tensor(), F)

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    r = res[FILLS[0]]
    for axis in range(3):
        assert same_bits(r[f"out{axis}"], c["want"][axis]) and same_bits(r[f"plain{axis}"], c["want"][axis])
        assert _within(r[f"ge{axis}"], c["acc"][axis][:rows], c["absacc"][axis][:rows])
        assert np.all(c["acc"][axis][rows:] == 0)
    assert _within(r["ge3"], sum(c["acc"])[:rows], sum(c["absacc"])[:rows]) and np.abs(r["ge3"]).max() > 0


@pytest.mark.parametrize("F", [2, 8])
def test_vote_fraction_tables(cuda, oracle, F):
    """cnc_vote_fraction_table{,_backward} on guarded buffers, against the float64 restatement and the bounds of
    tests/test_gpu_context_matrix.py::test_vote_fraction_tables."""
    from cnc_amd import _lib
    L, st = _lib.lib(), _lib.stream(cuda)
    c = _case(oracle, F)
    cnt = c["want"][1]
    g = np.random.default_rng(3).normal(size=((S + 2) * (S + 2), F)).astype(f32)

    def build(fill):
        return {"cnt": Guarded(cnt, cuda, fill=fill), "g": Guarded(g, cuda, fill=fill),
                "table": Guarded.empty(((S + 2) * (S + 2), F), f32, cuda, fill=fill), "sums": Guarded.empty((S, S, F), f32, cuda, fill=fill),
                "gos": Guarded.empty((S, S, F, 2), f32, cuda, fill=fill)}

    def run(b):
        _lib.check(L.cnc_vote_fraction_table(b["cnt"].ptr, S, F, b["table"].ptr, b["sums"].ptr, st), "vote_fraction_table")
        _lib.check(L.cnc_vote_fraction_table_backward(b["g"].ptr, b["sums"].ptr, S, F, b["gos"].ptr, st), "vote_fraction_table_backward")

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    r = res[FILLS[0]]
    c64 = cnt.astype(np.float64)
    den = c64[..., 0] + c64[..., 1] + 1e-6
    ref = c64[..., 0] / den
    tab = r["table"].reshape(S + 2, S + 2, F)
    assert not tab[0].any() and not tab[-1].any() and not tab[:, 0].any() and not tab[:, -1].any()
    assert np.all(np.abs(tab[1:-1, 1:-1] - ref) <= FRACTION_U["table"] * U * np.abs(ref))
    assert np.all(np.abs(r["sums"] - den) <= FRACTION_U["sums"] * U * den)
    want = g.reshape(S + 2, S + 2, F)[1:-1, 1:-1].astype(np.float64) / r["sums"].astype(np.float64)
    assert np.all(np.abs(r["gos"][..., 0] - want) <= FRACTION_U["grad"] * U * np.abs(want)) and not r["gos"][..., 1].any()
