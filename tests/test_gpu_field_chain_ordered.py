"""The ordered form of the field chain's bias sums (cnc_field_backward_chain_ordered, cnc_amd/csrc/field_bwd.hip).  The gradient pass
of `_FieldChain` runs once per route; inside it the chain kernel's descriptor is taken and the kernel called again on
sentinel-guarded outputs and scratch — the plain form and the ordered one, the latter eight times under fresh allocations,
two streams and a busy side stream.  Bias gradients against the layer-by-layer path with the bound of
tests/test_gpu_field_chain.py; every other output bit-equal to the plain call; nothing written outside the stated sizes."""
import ctypes

import numpy as np
import pytest
import torch

from guarded import Guarded
from test_gpu_field_chain import _grads
from test_gpu_field_fused import CONFIGS, _field, _inputs

pytestmark = pytest.mark.gpu

OUTS = ("G5", "G4", "G3", "G2", "G1", "dX")


def _again(L, st, dev, ordered, shapes, stream_of=None):
    """The captured call once more: outputs, bias sums (zeroed) + g_max and scratch in guarded buffers of their own."""
    from cnc_amd import _lib
    d = _lib.FieldBwd.from_buffer_copy(st)
    bufs = {k: Guarded.empty(shapes[k], np.float32, dev) for k in OUTS}
    for k in OUTS:
        setattr(d, k, bufs[k].ptr)
    H = d.n_neurons
    bufs["bsum"] = Guarded(np.zeros(3 * H + 84 + 8, np.float32), dev)
    d.bias_grads, d.g_max = bufs["bsum"].ptr, bufs["bsum"].ptr + (3 * H + 84) * 4
    if ordered:
        n = int(L.cnc_field_backward_chain_ordered_workspace(ctypes.byref(d)))
        assert n == min((d.N + 31) // 32, 2048) * (3 * H + 84) * 4
        bufs["ws"] = Guarded.empty((n,), np.uint8, dev)
        _lib.check(L._ordered_chain(ctypes.byref(d), bufs["ws"].ptr, n, _lib.stream(dev)), "field_backward_chain_ordered")
    else:
        _lib.check(L._plain_chain(ctypes.byref(d), _lib.stream(dev)), "field_backward_chain")
    return bufs


# k_field_bwd_chain<NT, true>: the grid is min(tiles of 32 rows, what is resident at once, kOrderedMaxSlots = 2048) and a
# workgroup walks `tile += gridDim.x`, adding every tile's column sums into its one slot.  4133 rows are 130 tiles, one
# each; 32 * 2048 + 33 = 65569 rows are 2050 tiles, more than either cap on any device: workgroups 0 and 1 at least
# take a second tile, the last tile has one row
@pytest.mark.parametrize("n", [4133, 31, 32 * 2048 + 33])
@pytest.mark.parametrize("cfg", ["f2_toy", "f8_full"])          # (F = 2, H = 64) and (F = 8, H = 160)
def test_ordered_bias_sums(cuda, cfg, n, monkeypatch):
    import cnc_amd
    from cnc_amd import _lib, _repro
    f = _field(cuda, CONFIGS[cfg], seed=8)
    x, d = _inputs(cuda, n, seed=n + 1)
    g = torch.Generator(device=cuda).manual_seed(3)
    scale = torch.exp(torch.randn(n, 1, device=cuda, generator=g) * 3.0 - 6.0)
    wr = torch.randn(n, 3, device=cuda, generator=g) * scale
    wd = torch.randn(n, 1, device=cuda, generator=g) * scale * 0.1
    with cnc_amd.reproducible(False):
        _, _, g0 = _grads(f, x, d, wr, wd, chain=False)
    L = _lib.lib()
    side, streams = torch.cuda.Stream(cuda), [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    m = torch.randn(2048, 2048, device=cuda)
    seen = {}

    def spy(st_ref, workspace, workspace_bytes, stream):
        st = st_ref._obj
        rc = L._ordered_chain(st_ref, workspace, workspace_bytes, stream)
        if rc == 0 and "plain" not in seen:
            Np, H = st.N, st.n_neurons
            shapes = {"G5": (Np, 4), "G4": (Np, H), "G3": (Np, H), "G2": (Np, st.ld_g2), "G1": (Np, H), "dX": (Np, st.ld_x)}
            torch.cuda.synchronize()
            seen["plain"] = _again(L, st, cuda, False, shapes)
            runs = []
            for rep in range(8):
                if rep >= 4:
                    with torch.cuda.stream(side):
                        for _ in range(6):
                            m @ m
                with torch.cuda.stream(streams[rep % 2]):
                    runs.append(_again(L, st, cuda, True, shapes))
            torch.cuda.synchronize()
            seen["ordered"] = runs
        return rc

    L._plain_chain, L._ordered_chain = L.cnc_field_backward_chain, L.cnc_field_backward_chain_ordered
    monkeypatch.setattr(L, "cnc_field_backward_chain_ordered", spy)
    try:
        before = dict(_repro.ROUTE_CALLS)
        with cnc_amd.reproducible(True):
            _, _, g1 = _grads(f, x, d, wr, wd, chain=True)
        assert f._chain_supported, "the chain did not run"
        assert _repro.ROUTE_CALLS["field_ordered"] == before["field_ordered"] + 1
        assert _repro.ROUTE_CALLS["field_default"] == before["field_default"]
        assert "ordered" in seen, "the ordered entry did not run"
        with cnc_amd.reproducible(False):
            _grads(f, x, d, wr, wd, chain=True)
        assert _repro.ROUTE_CALLS["field_default"] == before["field_default"] + 1
    finally:
        monkeypatch.undo()
        del L._plain_chain, L._ordered_chain
    # bias gradients (and, while at it, everything else) against the layer-by-layer path: the bound of the plain chain
    assert set(g0) == set(g1) and len(g0) == 14
    for name in g0:
        a, b = g1[name].double(), g0[name].double()
        scale_ = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-5 * max(scale_, 1e-30), (name, float((a - b).abs().max()), scale_)
    assert sum(name.endswith("bias") for name in g0) == 5
    # every other output of the chain: bit-equal to the plain call; g_max too; sentinels intact; scratch fully written
    plain, runs = seen["plain"], seen["ordered"]
    for bufs in [plain] + runs:
        assert all(b.intact() for b in bufs.values())
    H = CONFIGS[cfg]["n_neurons"]
    nb = 3 * H + 84
    for r in runs:
        for k in OUTS:
            assert torch.equal(r[k].tensor().view(torch.int32), plain[k].tensor().view(torch.int32)), k
        assert np.array_equal(r["bsum"].get()[nb:].view(np.uint32), plain["bsum"].get()[nb:].view(np.uint32))
        ws = r["ws"].get().view(np.uint32).reshape(-1, nb)
        tiles = (n + 31) // 32                                              # (of the rows given; the call may pad them)
        if ws.shape[0] < 2048:
            assert (ws != 0xA5A5A5A5).all()                                 # every slot of the scratch is written
        else:
            # the scratch is sized for 2048 workgroups on every device, the grid is what is resident of them: one whole
            # slot per workgroup launched, the slots behind them untouched, and fewer workgroups than tiles
            k = int((ws != 0xA5A5A5A5).all(axis=1).sum())
            assert 256 <= k < tiles and (ws[:k] != 0xA5A5A5A5).all() and (ws[k:] == 0xA5A5A5A5).all(), k
        # eight perturbed repeats: the same bits
        assert np.array_equal(r["bsum"].get().view(np.uint32), runs[0]["bsum"].get().view(np.uint32))
    # ... and the ordered sums are the plain ones up to the order of a few hundred fp32 additions
    a, b = runs[0]["bsum"].get()[:nb].astype(np.float64), plain["bsum"].get()[:nb].astype(np.float64)
    assert np.abs(a - b).max() <= 2e-5 * max(np.abs(b).max(), 1e-30)
