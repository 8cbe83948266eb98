"""The ordered encoder backward without a GPU: its definition, pinned independently of the C oracle, and the mode
resolution of the mirror with the library call stubbed out."""
import itertools

import numpy as np
import pytest
import torch

import np_twins
from conftest import make_grid

f32 = np.float32


def _contract(grad, x, emb, offs, res, ste):
    """The contract of cnc_grid_encode_backward_ordered (include/cnc_hip.h) as a plain loop: per element one fp32
    accumulator, level slot, then point, then corner; every term two rounded multiplies and one rounded add.  Corners,
    weights w[c] * wn_re and validity from the NumPy twin (written from the reference's CUDA source, not the oracle)."""
    acc = np.zeros_like(emb)
    F = emb.shape[1]
    for k in range(len(res)):
        o0, hs = int(offs[k]), int(offs[k + 1] - offs[k])
        rows, t, valid, _ = np_twins.grid_corners(x, int(res[k]), hs)
        assert t.dtype == np.float32
        for b in range(x.shape[0]):
            for c in range(rows.shape[1]):
                if not valid[b, c]:
                    continue
                row = o0 + int(rows[b, c])
                for ch in range(F):
                    if ste and not (f32(-1) <= emb[row, ch] <= f32(1)):
                        continue
                    term = f32(t[b, c] * grad[k, b, ch])       # numpy float32 scalars: one rounded multiply
                    acc[row, ch] = f32(acc[row, ch] + term)    # one rounded add, never an fma
    return acc


@pytest.mark.parametrize("ste", [False, True])
def test_contract_loop_equals_serial_oracle(oracle, ste):
    offs, res, emb = make_grid([3, 6], 12, 2, 2, seed=5)
    rng = np.random.default_rng(6)
    x = rng.uniform(-0.02, 1.02, size=(200, 2)).astype(np.float32)
    x[:3] = 0.0
    x[3:6] = 1.0
    x[6:30] = x[30]                                            # duplicates: one row's sum gets many equal-row terms
    g = rng.normal(size=(2, 200, 2)).astype(np.float32)
    want = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=ste, threads=1)
    got = _contract(g, x, emb, offs, res, ste)
    assert np.count_nonzero(want) > 20
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the definition discriminates: the same terms in another point order give other bits somewhere
    perm = rng.permutation(200)
    other = oracle.grid_encode_backward(g[:, perm], x[perm], emb, offs, res, ste_binary=ste, threads=1)
    assert not np.array_equal(other, want)


class _StubLib:
    """Stands in for libcnc_hip.so: records which backward entry the mirror takes."""

    def __init__(self):
        self.calls = []

    def cnc_grid_encode_backward_ordered_workspace(self, N, D, rows_total):
        return 64

    def cnc_grid_encode_backward_ordered(self, *a):
        self.calls.append("ordered")
        return 0

    def cnc_grid_encode_backward(self, *a):
        self.calls.append("default")
        return 0


@pytest.fixture
def stubbed(monkeypatch):
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    stub = _StubLib()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(be, "_common_checks", lambda named: None)     # (they ask for CUDA tensors)
    monkeypatch.setattr(be, "stream", lambda device=None: 0)
    monkeypatch.setattr(be, "_workspace", lambda device, nbytes, which=0: torch.empty(nbytes, dtype=torch.uint8))
    monkeypatch.setattr(be, "_ORDERED_MODE", None)
    monkeypatch.delenv("CNC_ORDERED_BACKWARD", raising=False)
    return be, stub


def _call(be, ordered):
    z = torch.zeros(8, 2)
    i = torch.zeros(2, dtype=torch.int32)
    be.grid_encode_backward(z, z, z, i, i, z, 8, 2, 2, 1, 0, 128, ordered=ordered)


@pytest.mark.parametrize("explicit,mode,env,switch",
                         list(itertools.product([None, True, False], [None, True, False], [None, "1", "0"], [False, True])))
def test_mode_resolution(stubbed, monkeypatch, explicit, mode, env, switch):
    """explicit argument, then the process-wide mode, then CNC_ORDERED_BACKWARD=1, then torch's deterministic switch."""
    import cnc_amd
    be, stub = stubbed
    if env is not None:
        monkeypatch.setenv("CNC_ORDERED_BACKWARD", env)
    if explicit is not None:
        want = explicit
    elif mode is not None:
        want = mode
    else:
        want = env == "1" or switch
    was = torch.are_deterministic_algorithms_enabled()
    before = dict(be.ROUTE_CALLS)
    try:
        torch.use_deterministic_algorithms(switch)
        if mode is None:
            _call(be, explicit)
        else:
            with cnc_amd.ordered_backward(mode):
                _call(be, explicit)
            assert be._ORDERED_MODE is None                    # the context manager restores what it found
    finally:
        torch.use_deterministic_algorithms(was)
    assert stub.calls == ["ordered" if want else "default"]
    assert be.ROUTE_CALLS["ordered"] - before["ordered"] == int(want)
    assert be.ROUTE_CALLS["default"] - before["default"] == int(not want)


def test_mode_setter_and_nesting(stubbed):
    import cnc_amd
    be, stub = stubbed
    assert cnc_amd.ordered_backward is be.ordered_backward
    cnc_amd.ordered_backward(True)                             # plain setter
    assert be.ordered_backward_enabled()
    with cnc_amd.ordered_backward(False):
        assert not be.ordered_backward_enabled()
        with cnc_amd.ordered_backward():
            assert be.ordered_backward_enabled()
        assert not be.ordered_backward_enabled()
    assert be.ordered_backward_enabled()
    cnc_amd.ordered_backward(None)                             # back to "not set"
    assert not be.ordered_backward_enabled()


def test_module_override_reaches_the_backward(stubbed, monkeypatch):
    """GridEncoder(ordered_backward=...) is captured in the forward and handed to the backward as `ordered=`."""
    from cnc_amd import gridencoder
    be, stub = stubbed
    seen = []
    monkeypatch.setattr(be, "grid_encode_forward", lambda *a, **k: a[4].zero_())
    monkeypatch.setattr(be, "grid_encode_backward", lambda *a, **k: seen.append(k.get("ordered", "missing")))
    for flag in (True, False, None):
        enc = gridencoder.GridEncoder(num_dim=2, n_features=2, resolutions_list=(4, 8), log2_hashmap_size=8,
                                      ordered_backward=flag)
        out = enc(torch.rand(5, 2))
        out.sum().backward()
    assert seen == [True, False, None]
