"""tests/guarded.py itself, on the CPU with stand-in "kernels" written in torch: an over-read whose value reaches the
output moves with the fill (or turns NaN) and `under_fills` + `same_bits` report it, a write past an output fails
`intact()` under every fill, a correct kernel passes, and every supported type round-trips."""
import numpy as np
import pytest
import torch

from guarded import FILL, FILLS, PAD, Guarded, holds_fill, moved_with_fill, same_bits, sentinel, under_fills

CPU = torch.device("cpu")
f32 = np.float32
DTYPES = [np.float32, np.float64, np.int16, np.int32, np.uint32, np.int64, np.uint8, np.bool_]


def _flat(g, dtype):
    """The whole allocation of `g` as elements of `dtype`, and the index of the buffer's first element in it: what a
    kernel holding `g.ptr` can reach."""
    item = torch.empty((), dtype=dtype).element_size()
    assert g.lo % item == 0
    n = g.alloc.numel() // item * item
    return g.alloc[:n].view(dtype), g.lo // item


def _row_sums(x, y, n, k, ld, over=0, spill=0):
    """y[i] = sum of x[i, :k + over] for rows of stride ld; `over` > 0 reads past each row, `spill` > 0 writes that
    many elements past y."""
    a, x0 = _flat(x, torch.float32)
    b, y0 = _flat(y, torch.float32)
    x0 += 0 if x.win is None else x.win[0]
    for i in range(n + spill):
        b[y0 + i] = a[x0 + i * ld:x0 + i * ld + k + over].sum() if i < n else 1.0


def test_fills_and_sentinels():
    assert FILLS == (0x00, 0xA5, 0xFF) and FILL == 0xA5
    assert sentinel(np.float32, 0x00) == 0 and np.isnan(sentinel(np.float32, 0xFF)) and np.isnan(sentinel(np.float64, 0xFF))
    assert -1e-15 < sentinel(np.float32) < 0 and sentinel(np.float32) == sentinel(np.float32, 0xA5)
    for dt in (np.int16, np.int32, np.int64):                      # no fill is a large positive count
        assert all(sentinel(dt, f) <= 0 for f in FILLS) and sentinel(dt, 0xFF) == -1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fill", FILLS)
def test_every_type_round_trips(dtype, fill):
    rng = np.random.default_rng(3)
    host = (rng.integers(0, 2, (5, 7)).astype(dtype) if dtype is np.bool_ else
            (rng.standard_normal((5, 7)) * 100).astype(dtype))
    g = Guarded(host, CPU, fill=fill)
    assert g.intact() and g.fill == fill and g.role == "in"
    assert same_bits(g.get(), host) and g.get().dtype == np.dtype(dtype)
    t = g.tensor()
    assert tuple(t.shape) == (5, 7) and t.data_ptr() == g.ptr and t.element_size() == np.dtype(dtype).itemsize
    assert same_bits(t.numpy().view(dtype) if dtype is np.uint32 else t.numpy(), host)
    e = Guarded.empty((3, 4), dtype, CPU, fill=fill)
    assert e.role == "out" and e.intact() and holds_fill(e.get(), fill)
    if dtype is not np.bool_:
        assert same_bits(e.get(), np.full((3, 4), sentinel(dtype, fill)))
    w = Guarded.window(host, 11, 3, CPU, fill)
    assert w.intact() and same_bits(w.get(), host) and w.tensor().stride() == (11, 1)
    assert w.ptr == w.alloc.data_ptr() + w.lo + 3 * np.dtype(dtype).itemsize == w.tensor().data_ptr()
    full = w.full()
    assert holds_fill(full[:, :3], fill) and holds_fill(full[:, 10:], fill) and same_bits(full[:, 3:10], host)
    like = Guarded.like(g.tensor(), fill=fill)
    assert same_bits(like.get().view(dtype), host) and like.intact()     # (a tensor of uint32 data is int32)


def test_defaults_are_what_they_were():
    g = Guarded(np.arange(6, dtype=f32), CPU)
    assert g.fill == FILL and g.lo == PAD and g.alloc.numel() == 2 * PAD + 24 + 256
    assert int(g.alloc[0]) == FILL and int(g.alloc[-1]) == FILL
    s = Guarded(np.arange(6, dtype=f32), CPU, 4)                   # shift stays the third positional argument
    assert s.lo == PAD + 4 and s.ptr % 16 == (s.alloc.data_ptr() + 4) % 16 and same_bits(s.get(), g.get())
    with pytest.raises(TypeError):
        Guarded(np.zeros(3, np.float16), CPU)
    with pytest.raises(ValueError):
        Guarded.window(np.zeros((2, 5), f32), 8, 4, CPU)


def test_shift_moves_a_window_off_its_alignment():
    w = Guarded.window(np.ones((3, 4), f32), 8, 0, CPU, 0xFF, shift=4)
    assert (w.ptr - w.alloc.data_ptr()) % 16 == 4 and w.intact() and same_bits(w.get(), np.ones((3, 4), f32))


def test_intact_sees_a_write_into_a_windows_gap_and_behind_a_buffer():
    for fill in FILLS:
        w = Guarded.window(np.ones((3, 4), f32), 8, 2, CPU, fill)
        assert tuple(w.whole().shape) == (3, 8) and w.whole().is_contiguous() and w.whole().data_ptr() == w.ptr - 2 * 4
        w.whole()[1, 6] = 5.0
        assert not w.intact()
        w = Guarded.window(np.ones((3, 4), f32), 8, 2, CPU, fill)
        w.whole()[2, 1] = 5.0
        assert not w.intact()
        for at in (-1, 0):                                         # the byte before, the byte behind
            g = Guarded(np.ones(4, f32), CPU, fill=fill)
            g.alloc[g.lo + (at if at else g.nbytes)] = 1
            assert not g.intact()


def test_same_bits_counts_nan_payloads_and_signed_zero():
    a = np.array([0.0, np.nan, 1.0], f32)
    assert same_bits(a, a.copy()) and same_bits(torch.from_numpy(a), a)
    assert not same_bits(a, np.array([-0.0, np.nan, 1.0], f32))
    b = a.copy()
    b.view(np.uint32)[1] ^= 1                                      # another NaN
    assert np.isnan(b[1]) and not same_bits(a, b)
    assert not same_bits(a, a.astype(np.float64)) and not same_bits(a, a[:2])
    assert not same_bits(np.zeros(2, np.int32), np.zeros(2, np.uint32))


def _build(n, k, ld, col):
    rng = np.random.default_rng(0)
    host = rng.standard_normal((n, k)).astype(f32)

    def build(fill):
        x = Guarded(host, CPU, fill=fill) if ld == k else Guarded.window(host, ld, col, CPU, fill)
        return {"x": x, "y": Guarded.empty((n,), f32, CPU, fill=fill), "none": None}
    return host, build


@pytest.mark.parametrize("ld,col", [(5, 0), (9, 0), (9, 2)])
def test_a_correct_kernel_passes(ld, col):
    host, build = _build(4, 5, ld, col)
    res = under_fills(build, lambda b: _row_sums(b["x"], b["y"], 4, 5, ld))
    assert set(res) == set(FILLS) and all(set(r) == {"y"} for r in res.values())
    assert moved_with_fill(res) == []
    assert np.allclose(res[0xFF]["y"], host.sum(1), rtol=0, atol=1e-6)


def test_one_element_past_the_input_is_reported():
    """Contiguous rows: only the LAST row's extra element lies outside the buffer.  Under 0x00 the sums are right (the
    bug hides, as on a fresh allocation); the other fills show it."""
    host, build = _build(4, 5, 5, 0)
    want = host.sum(1)
    want[:3] += host[1:, 0]
    res = under_fills(build, lambda b: _row_sums(b["x"], b["y"], 4, 5, 5, over=1))
    assert np.allclose(res[0x00]["y"], want, atol=1e-6)
    assert moved_with_fill(res) == ["y"]
    assert np.isnan(res[0xFF]["y"][3]) and not np.isnan(res[0xFF]["y"][:3]).any()


@pytest.mark.parametrize("col", [0, 2])
def test_a_windows_gap_column_is_reported(col):
    host, build = _build(4, 5, 9, col)
    res = under_fills(build, lambda b: _row_sums(b["x"], b["y"], 4, 5, 9, over=1))
    assert np.allclose(res[0x00]["y"], host.sum(1), atol=1e-6)
    assert moved_with_fill(res) == ["y"] and np.isnan(res[0xFF]["y"]).all()


@pytest.mark.parametrize("fill", FILLS)
def test_one_element_past_the_output_fails_intact(fill):
    _, build = _build(4, 5, 5, 0)
    with pytest.raises(AssertionError, match="around 'y'"):
        under_fills(build, lambda b: _row_sums(b["x"], b["y"], 4, 5, 5, spill=1), fills=(fill,))


@pytest.mark.parametrize("fill", FILLS)
def test_a_modified_input_is_reported(fill):
    _, build = _build(4, 5, 9, 2)

    def run(b):
        _row_sums(b["x"], b["y"], 4, 5, 9)
        b["x"].tensor()[0, 0] += 1.0
    with pytest.raises(AssertionError, match="input 'x' was modified"):
        under_fills(build, run, fills=(fill,))


def test_buffers_entered_during_the_call_are_held_to_the_same_rules():
    """A helper that builds its operands itself enters them into `bufs` while the call is made: under_fills snapshots such
    an input when it is entered, checks its surroundings, returns such an output, and refuses another fill or a name twice."""
    host = np.arange(5, dtype=f32)

    def run(b, over=0, touch=False, fill=None):
        b["x"] = Guarded(host, CPU, fill=b.fill if fill is None else fill)
        b["y"] = Guarded.empty((1,), f32, CPU, fill=b.fill)
        _row_sums(b["x"], b["y"], 1, 5, 5, over=over)
        if touch:
            b["x"].tensor()[0] = 9.0

    res = under_fills(lambda fill: {}, run)
    assert moved_with_fill(res) == [] and float(res[0xFF]["y"][0]) == 10.0
    assert moved_with_fill(under_fills(lambda fill: {}, lambda b: run(b, over=1))) == ["y"]
    with pytest.raises(AssertionError, match="input 'x' was modified"):
        under_fills(lambda fill: {}, lambda b: run(b, touch=True), fills=(0xA5,))
    with pytest.raises(AssertionError, match="not built with fill"):
        under_fills(lambda fill: {}, lambda b: run(b, fill=0x00), fills=(0xFF,))
    with pytest.raises(AssertionError, match="two buffers named"):
        under_fills(lambda fill: {"x": Guarded(host, CPU, fill=fill)}, run, fills=(0x00,))


def test_roles():
    acc = Guarded(np.zeros(3, f32), CPU, fill=0xFF).out()
    ws = Guarded.empty((16,), np.uint8, CPU, fill=0xFF).scratch()
    x = Guarded(np.ones(3, f32), CPU, fill=0xFF)

    def run(b):
        b["acc"].tensor().add_(b["x"].tensor())
        b["ws"].tensor().zero_()
    res = under_fills(lambda fill: {"acc": acc, "ws": ws, "x": x}, run, fills=(0xFF,))
    assert set(res[0xFF]) == {"acc"} and same_bits(res[0xFF]["acc"], np.ones(3, f32))
    with pytest.raises(AssertionError, match="not built with fill"):
        under_fills(lambda fill: {"x": Guarded(np.ones(3, f32), CPU)}, lambda b: None, fills=(0x00,))
