"""Footprint of the fused MLP forward (cnc_amd/csrc/mlp.hip, `cnc_mlp_forward` and `cnc_mlp_forward32`): the result
depends on the [N, K0] input alone.  X lies in a guarded allocation (tests/guarded.py) whose surroundings — and, for
a column window, the gap between its rows — hold 0x00, 0xA5 and 0xFF in turn; the outputs must be the same bits each
time and within `test_fused_mlp_forward_matches_torch`'s bound of its float64 chain.

`load_a`'s vector path reads K0p floats of a row (into the gap, or into the next row) and zeroes the columns >= K0
afterwards; the last row takes guarded scalar loads.  If the zeroing went missing, the 0xFF run turns NaN: the packed
weights are zero there, and 0 * NaN is NaN.  An outside read whose value is discarded is NOT caught here: this pins the
value-level contract, not memory safety."""
import numpy as np
import pytest
import torch

from guarded import FILLS, Guarded, holds_fill, moved_with_fill, same_bits, under_fills
from test_gpu_mlp import REL, chain64, make_seq

pytestmark = pytest.mark.gpu
f32 = np.float32

DIMS = [(95, 160, 160, 3), (25, 32, 32, 8), (255, 160, 80)]
# name -> (ld, col, shift) from K0 and K0p.  contig: ldx = K0 (odd: scalar loads); tight: the vector path, a row's read
# ends where the row ends; gap: the vector path with 16 floats of poison behind every row; unaligned: the layout of the
# existing test's strided case (K0 = 25: ldx = 34, scalar; K0 = 95, 255: ldx % 4 == 0 and the window 16 bytes in, so the
# vector path with poison on both sides); gap_shift4: `gap` four bytes off, the other side of the a_vec gate
LAYOUTS = {
    "contig": lambda K0, K0p: (K0, 0, 0),
    "tight": lambda K0, K0p: (K0p, 0, 0),
    "gap": lambda K0, K0p: (K0p + 16, 0, 0),
    "unaligned": lambda K0, K0p: (K0 + 9, 4, 0),
    "gap_shift4": lambda K0, K0p: (K0p + 16, 0, 4),
}
_MODELS = {}


def _supported32(dims):
    """cnc_mlp_forward32 has the radiance field's two shapes only."""
    return dims[1] == 160 and ((len(dims) == 3 and dims[2] <= 96) or (len(dims) == 4 and dims[2] == 160 and dims[3] <= 32))


def _model(dims, dev):
    """One network per shape, its float32 and float64 results on a fixed 33-row input: computed once, never changed."""
    if dims not in _MODELS:
        from cnc_amd.mlp import FusedMLPForward
        torch.manual_seed(len(dims) * 1000 + dims[0])
        seq = make_seq(dims, dev)
        x = torch.randn(33, dims[0], generator=torch.Generator().manual_seed(dims[0]))
        with torch.no_grad():
            want = seq(x.to(dev))
        ref = chain64(seq, x.to(dev))
        _MODELS[dims] = (seq, {16: FusedMLPForward(seq), 32: FusedMLPForward(seq, rows_per_wave=32)}, x.numpy(), want, ref)
    return _MODELS[dims]


CASES = [(d, r) for d in DIMS for r in (16, 32) if r == 16 or _supported32(d)]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("N", [1, 17, 33])
@pytest.mark.parametrize("dims,rows", CASES)
def test_forward_depends_on_its_input_alone(cuda, dims, rows, N, layout):
    seq, fused, x, want, ref = _model(dims, cuda)
    K0, n_out = dims[0], dims[-1]
    K0p = (K0 + 7) // 8 * 8 if rows == 32 else (K0 + 15) // 16 * 16
    ld, col, shift = LAYOUTS[layout](K0, K0p)

    def build(fill):
        X = Guarded(x[:N], cuda, shift, fill) if ld == K0 else Guarded.window(x[:N], ld, col, cuda, fill, shift)
        return {"x": X, "y": Guarded.empty((N, n_out), f32, cuda, fill=fill)}

    def run(b):
        xt = b["x"].tensor()
        assert xt.stride(0) == ld and xt.data_ptr() == b["x"].ptr and xt.data_ptr() % 16 == (4 * col + shift) % 16
        b["y"].tensor().copy_(fused[rows](xt))

    res = under_fills(build, run)
    assert moved_with_fill(res) == [], "the result moves with the bytes around X"
    got = torch.from_numpy(res[FILLS[0]]["y"]).to(cuda)
    scale = want[:N].abs().max().clamp_min(1.0)
    assert bool(torch.isfinite(got).all())
    assert (got - want[:N]).abs().max() <= REL * scale
    assert (got.double() - ref[:N]).abs().max() <= REL * scale


@pytest.mark.parametrize("N", [1, 17, 33])
@pytest.mark.parametrize("dims,rows", CASES)
def test_output_window_through_the_abi(cuda, dims, rows, N):
    """The C ABI with Y as columns [3, 3 + n_out) of an [N + 2, n_out + 7] buffer and X as the `gap` window: the columns
    around Y's and the rows >= N keep the fill, the result is the wrapper's, bit for bit, under every fill."""
    from cnc_amd import _lib
    seq, fused, x, want, ref = _model(dims, cuda)
    K0, n_out = dims[0], dims[-1]
    K0p = (K0 + 7) // 8 * 8 if rows == 32 else (K0 + 15) // 16 * 16
    ldy = n_out + 7
    packed = fused[rows]._pack()
    (w1, b1, h1), (w2, b2, h2) = packed[0], packed[1]
    w3, b3, h3 = packed[2] if len(packed) == 3 else (None, None, 0)
    fn = _lib.lib().cnc_mlp_forward32 if rows == 32 else _lib.lib().cnc_mlp_forward

    def build(fill):
        return {"x": Guarded.window(x[:N], K0p + 16, 0, cuda, fill),
                "y": Guarded.empty_window(N + 2, n_out, ldy, 3, f32, cuda, fill)}

    def run(b):
        _lib.check(fn(b["x"].ptr, N, K0p + 16, K0, w1.data_ptr(), b1.data_ptr(), h1, w2.data_ptr(), b2.data_ptr(), h2,
                      _lib.ptr(w3), _lib.ptr(b3), h3, b["y"].ptr, ldy, n_out, _lib.stream(cuda)), "mlp_forward")

    res = under_fills(build, run)           # (intact() covers the columns left and right of the window)
    for fill in FILLS:
        assert holds_fill(res[fill]["y"][N:], fill), "rows >= N were written"
        res[fill]["y"] = res[fill]["y"][:N]
    assert moved_with_fill(res) == []
    assert same_bits(res[FILLS[0]]["y"], fused[rows](torch.from_numpy(x[:N]).to(cuda)).cpu().numpy())
