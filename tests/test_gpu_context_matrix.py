"""The context-model kernels at the sizes the training step runs (configs[2]: 12 3-D levels at T = 2^19, planes of 4 levels
at T = 2^17, F = 8, sample_num = 150,000, Rb = 128) against references written here: float64 torch that calls no project
kernel, or the CPU oracle.  The launch code switches paths above fixed sizes (cnc_amd/csrc/ctx_head.hip `launch_mlp`,
`cnc_bernoulli_bits_partials`, `k_level_sums`' 2048-row blocks); every case sits on one side of such a size.

Sums over many rows are held to |got - G| <= c 2^-24 A, where A is the same sum over the magnitudes of the terms, so
the bound grows with N as the rounding error does; per-row values keep the bounds of tests/test_gpu_ctx_head.py."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import ball_occupancy, make_grid

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # unit roundoff of float32
# Reductions over N rows.  Each fp32 addition of a reduction rounds once, by at most U times the partial sum it
# produces, and a partial sum is bounded by the A of the rows it holds.  The deepest chains at N = 640k: k_ctx_mlp_bwd<1>
# 16 MFMA steps x 5 batches per wave, then 64 blocks' atomics per replica (partial sums ~A / 16) and the 16-replica
# sum; k_ctx_head3_bwd 4 steps x 14 tiles per wave, 4 waves, 48 atomics per replica, the replica sum: worst case
# (every rounding at its maximum, all of one sign) 65-95 U A.  Round-to-nearest errors are unbiased and independent,
# so the realised error is of the order of the square root of that depth (~10 U A): c = 64 leaves a wide margin for
# them, while one lost or doubled row of the sparse case moves its sum by ~A / 3300 = 80x the bound
# (test_heads_sparse_gradient_sees_every_tile).
C_SUM = 64

N_ROWS = [1, 15, 16, 17,
          49152, 49153 + 14,       # k_ctx_head3_*: above 3072 tiles a wave walks a contiguous range (tail tile inside it)
          131072, 131073,          # k_ctx_mlp_bwd<1,F>: above 1024 batches a block sums several before its atomics
          524288, 524289,          # k_ctx_mlp_fwd<1,F>: above 2048 blocks of 256 rows, grid-stride
          640_003]                 # the training step's ~0.64 M rows, not a multiple of 16


_RATIOS = {}                       # largest |got - ref| / bound per group, printed when the module ends (pytest -s)


def _note(group, r):
    _RATIOS[group] = max(_RATIOS.get(group, 0.0), float(r))


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nlargest |got - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_RATIOS.items())))


def _lib():
    from cnc_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------------
# 1. Context heads (cnc_ctx_mlp_forward / _backward)
# ------------------------------------------------------------------------------------------------------------------
def _head_weights(NL, C_in, F, gen, dev):
    shapes = [(F, C_in), (F,)] if NL == 1 else [(32, C_in), (32,), (32, 32), (32,), (F, 32), (F,)]
    return [torch.randn(s, generator=gen, device=dev) * 0.4 for s in shapes]


def _pre_activations(x, ws):
    w = [t.double() for t in ws]
    a1 = x @ w[0].T + w[1]
    m1 = x.abs() @ w[0].T.abs() + w[1].abs()
    h1 = torch.where(a1 > 0, a1, 0.01 * a1)
    a2 = h1 @ w[2].T + w[3]
    m2 = torch.where(a1 > 0, 1.0, 0.01) * m1 @ w[2].T.abs() + w[3].abs()
    return a1, m1, a2, m2


def _avoid_kinks(x_of, redraw, ws, C_in, rounds=6):
    """NL = 3: rows whose pre-activations lie within the float32 error bound of LeakyReLU's kink may take the other branch
    in the kernel (a factor 100 in that unit's gradient).  Such rows get fresh inputs until none is left, so both
    precisions differentiate the same function.  Bounds: a1 = W1 x + b1 carries <= (C + 1) U m1, a2 <= (C + 34) U m2."""
    for _ in range(rounds):
        x = x_of()
        a1, m1, a2, m2 = _pre_activations(x, ws)
        bad = ((a1.abs() <= 2 * (C_in + 1) * U * m1).any(1)) | ((a2.abs() <= 2 * (C_in + 34) * U * m2).any(1))
        if not bool(bad.any()):
            return
        redraw(bad)
    raise AssertionError("could not move the rows off the LeakyReLU kinks")


def _ref_head(x, ws, go):
    """float64 forward and backward, written out (Linear; or Linear-LeakyReLU(0.01)-Linear-LeakyReLU-Linear), with the
    magnitudes the rounding errors scale with: y, d x, |d x| (per-term magnitude of each input gradient), and per
    parameter the gradient G and A = the same sum over the magnitudes of its terms.  For NL = 3 the magnitudes follow
    the float32 chain itself (|W3|^T |d_out| ... and |W1| |x| + |b1| ...): the gradients at the hidden layers carry
    errors relative to those, not to their own (possibly cancelled) values."""
    w = [t.detach().double() for t in ws]
    go = go.double()
    if len(w) == 2:
        W1, b1 = w
        y = x @ W1.T + b1
        return y, go @ W1, go.abs() @ W1.abs(), [go.T @ x, go.sum(0)], [go.abs().T @ x.abs(), go.abs().sum(0)]
    W1, b1, W2, b2, W3, b3 = w
    a1 = x @ W1.T + b1
    s1 = torch.where(a1 > 0, 1.0, 0.01)
    h1 = a1 * s1
    a2 = h1 @ W2.T + b2
    s2 = torch.where(a2 > 0, 1.0, 0.01)
    h2 = a2 * s2
    y = h2 @ W3.T + b3
    d2 = (go @ W3) * s2
    d1 = (d2 @ W2) * s1
    mh1 = (x.abs() @ W1.abs().T + b1.abs()) * s1
    mh2 = (mh1 @ W2.abs().T + b2.abs()) * s2
    e2 = (go.abs() @ W3.abs()) * s2
    e1 = (e2 @ W2.abs()) * s1
    G = [d1.T @ x, d1.sum(0), d2.T @ h1, d2.sum(0), go.T @ h2, go.sum(0)]
    A = [e1.T @ x.abs(), e1.sum(0), e2.T @ mh1, e2.sum(0), go.abs().T @ mh2, go.abs().sum(0)]
    return y, d1 @ W1, e1 @ W1.abs(), G, A


def _check_sum(got, G, A, what, group="heads"):
    err = (got.double() - G).abs()
    bound = C_SUM * U * A + 1e-30
    r = float((err / bound).max())
    _note(group, r)
    assert r <= 1.0, (what, r)


def _check_rows(got, ref, what):
    assert torch.allclose(got.double(), ref, rtol=2e-5, atol=2e-5), (what, float((got.double() - ref).abs().max()))


def _inputs(N, Ca, Cb, gen, dev):
    a = torch.randn(N, Ca, generator=gen, device=dev)
    b = torch.randn(N, Cb, generator=gen, device=dev) if Cb else None
    return a, b


@pytest.mark.parametrize("N", N_ROWS)
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("NL", [1, 3])
def test_heads_rows(cuda, NL, F, N):
    """C = 33 = 24 + 8 + Pg (the widest row the training step builds: three context levels, the dimension-wise
    features, Pg; the third 16-column block of the three-layer head) through the autograd path."""
    from cnc_amd.backends.context_backend import ContextMLP
    gen = torch.Generator(device=cuda).manual_seed(1000 * NL + 10 * F + N % 997)
    Ca, Cb = 24, 8
    C_in = Ca + Cb + 1
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a, b = _inputs(N, Ca, Cb, gen, cuda)
    pg = torch.rand((), generator=gen, device=cuda)
    x_of = lambda: torch.cat([a.double(), b.double(), pg.double().expand(N, 1)], 1)
    if NL == 3:
        def redraw(bad):
            a[bad] = torch.randn(int(bad.sum()), Ca, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    go = torch.randn(N, F, generator=gen, device=cuda)
    y64, dx, adx, G, A = _ref_head(x_of(), ws, go)
    dpg, apg = dx[:, -1].sum(), adx[:, -1].sum()
    leaves = [w.clone().requires_grad_() for w in ws]
    ad, bd, pgd = a.clone().requires_grad_(), b.clone().requires_grad_(), pg.clone().requires_grad_()
    full = leaves + [None] * (6 - len(leaves))
    y = ContextMLP.apply(ad, bd, pgd, *full, None)
    (y * go).sum().backward()
    _check_rows(y, y64, "out")
    _check_rows(ad.grad, dx[:, :Ca], "grad_a")
    _check_rows(bd.grad, dx[:, Ca:Ca + Cb], "grad_b")
    for k, (p, g_ref, a_ref) in enumerate(zip(leaves, G, A)):
        _check_sum(p.grad, g_ref, a_ref, f"param {k}")
    _check_sum(pgd.grad, dpg, apg, "pg")


def _abi_heads(NL, F, ws, a, lda, Ca, b, ldb, Cb, pg, pg_index, N, go, ga, ldga, gb, ldgb, g_pg, reps=16):
    """Forward and backward straight through the C ABI: `out` starts as NaN (every row must be written); the caller's
    grad_a / grad_b buffers are NaN too.  Returns out and the replica-summed weight gradients."""
    L = _lib()
    lib, st = L.lib(), L.stream(a.device)
    out = torch.full((N, F), float("nan"), device=a.device)
    w6 = [w.contiguous() for w in ws] + [None] * (6 - len(ws))
    L.check(lib.cnc_ctx_mlp_forward(a.data_ptr(), lda, Ca, L.ptr(b), ldb, Cb, L.ptr(pg), L.ptr(pg_index), N, NL, F,
                                    *[L.ptr(w) for w in w6], out.data_ptr(), st), "ctx_mlp_forward")
    total = sum(w.numel() for w in ws)
    copies = torch.zeros((reps, total), device=a.device)
    firsts, o = [], 0
    for w in ws:
        firsts.append(copies[0, o:o + w.numel()])
        o += w.numel()
    firsts += [None] * (6 - len(firsts))
    L.check(lib.cnc_ctx_mlp_backward(a.data_ptr(), lda, Ca, L.ptr(b), ldb, Cb, L.ptr(pg), L.ptr(pg_index), N, NL, F,
                                     *[L.ptr(w) for w in w6], go.data_ptr(), ga.data_ptr(), L.ptr(gb), L.ptr(g_pg),
                                     *[L.ptr(f) for f in firsts], reps, total, ldga, ldgb, st), "ctx_mlp_backward")
    flat, gws, o = copies.sum(0), [], 0
    for w in ws:
        gws.append(flat[o:o + w.numel()].view_as(w))
        o += w.numel()
    return out, gws


def _offset_view(n, floats_past, dev, fill=None):
    """A float32 vector of n elements whose first element sits `floats_past` floats past a 16-byte boundary."""
    buf = torch.empty(n + 8, device=dev) if fill is None else torch.full((n + 8,), fill, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf[floats_past:floats_past + n]


# (Ca, lda, col0, Cb, in_b offset, pg, a offset, grad_a pitch)
WIDTHS = {
    "c33": (24, 24, 0, 8, 0, True, 0, 24),
    "c40": (24, 24, 0, 15, 0, True, 0, 24),          # kMaxC: the three-layer head's third column block, 8 columns of it
    "c40_nopg": (32, 32, 0, 8, 0, False, 0, 32),
    "odd_ca": (25, 25, 0, 8, 0, True, 0, 25),          # Ca % 4 != 0: the scalar fetch
    "strided": (20, 36, 8, 8, 0, True, 0, 28),         # lda > Ca, a column window (c0 = 8), padded grad_a pitch
    "misaligned": (24, 24, 0, 8, 3, True, 1, 24),      # in_a 4 bytes, in_b 12 bytes past a 16-byte boundary
}


@pytest.mark.parametrize("N", [17, 49153 + 14, 131073, 640_003])
@pytest.mark.parametrize("F", [1, 8])
@pytest.mark.parametrize("layout", list(WIDTHS))
@pytest.mark.parametrize("NL", [1, 3])
def test_heads_widths_and_layouts_through_the_abi(cuda, NL, layout, F, N):
    Ca, lda, c0, Cb, b_off, with_pg, a_off, ldga = WIDTHS[layout]
    gen = torch.Generator(device=cuda).manual_seed(100 * NL + 10 * list(WIDTHS).index(layout) + F + N)
    C_in = Ca + Cb + int(with_pg)
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a_mat = _offset_view(N * lda, a_off, cuda).view(N, lda)
    a_mat.copy_(torch.randn(N, lda, generator=gen, device=cuda))
    a = a_mat[:, c0:c0 + Ca]
    b = _offset_view(N * Cb, b_off, cuda).view(N, Cb)
    b.copy_(torch.randn(N, Cb, generator=gen, device=cuda))
    pg = torch.rand(1, generator=gen, device=cuda) if with_pg else None
    if layout == "misaligned":
        assert a.data_ptr() % 16 == 4 and b.data_ptr() % 16 == 12
    x_of = lambda: torch.cat([a.double(), b.double()] + ([pg.double().expand(N, 1)] if with_pg else []), 1)
    if NL == 3:
        def redraw(bad):
            a_mat[bad] = torch.randn(int(bad.sum()), lda, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    go = torch.randn(N, F, generator=gen, device=cuda)
    ga = torch.full((N, ldga), float("nan"), device=cuda)
    gb = _offset_view(N * Cb, b_off, cuda, fill=float("nan")).view(N, Cb)
    g_pg = torch.zeros(1, device=cuda) if with_pg else None
    out, gws = _abi_heads(NL, F, ws, a, lda, Ca, b, Cb, Cb, pg, None, N, go, ga, ldga, gb, Cb, g_pg)
    assert torch.isfinite(out).all() and torch.isfinite(ga[:, :Ca]).all() and torch.isfinite(gb).all()
    assert torch.isnan(ga[:, Ca:]).all()                      # nothing written past the window
    y64, dx, adx, G, A = _ref_head(x_of(), ws, go)
    _check_rows(out, y64, "out")
    _check_rows(ga[:, :Ca], dx[:, :Ca], "grad_a")
    _check_rows(gb, dx[:, Ca:Ca + Cb], "grad_b")
    for k, (g, g_ref, a_ref) in enumerate(zip(gws, G, A)):
        _check_sum(g, g_ref, a_ref, f"param {k}")
    if with_pg:
        _check_sum(g_pg[0], dx[:, -1].sum(), adx[:, -1].sum(), "pg")


@pytest.mark.parametrize("NL", [1, 3])
def test_heads_refuse_a_row_wider_than_kmaxc(cuda, NL):
    from cnc_amd.backends.context_backend import ContextMLP
    gen = torch.Generator(device=cuda).manual_seed(41)
    ws = _head_weights(NL, 41, 8, gen, cuda)
    a = torch.randn(64, 32, device=cuda)
    b = torch.randn(64, 8, device=cuda)
    with pytest.raises(RuntimeError, match="ctx_mlp_forward"):
        ContextMLP.apply(a, b, torch.rand((), device=cuda), *(ws + [None] * (6 - len(ws))), None)


def _pg_runs(N, T, gen, dev):
    """pg_index: sorted runs whose ends fall on both sides of 16-row tile, 64-row wave, 128-row batch and 224-row wave
    range boundaries (head3 at 640k rows: 14 tiles per wave), then a scrambled tail."""
    lengths = [1, 15, 17, 63, 65, 127, 129, 223, 225, 2047, 2049, 4096 + 16]
    idx = torch.empty(N, dtype=torch.int64)
    at, k = 0, 0
    tail = N - 5000
    while at < tail:
        n = min(lengths[k % len(lengths)], tail - at)
        idx[at:at + n] = (k * 5) % T
        at += n
        k += 1
    idx[tail:] = torch.randint(0, T, (N - tail,))
    return idx.to(dev)


@pytest.mark.parametrize("NL", [1, 3])
def test_heads_pg_table_runs(cuda, NL):
    N, Ca, Cb, F, T = 640_003, 24, 8, 8, 12
    gen = torch.Generator(device=cuda).manual_seed(77 + NL)
    torch.manual_seed(5)
    C_in = Ca + Cb + 1
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a, b = _inputs(N, Ca, Cb, gen, cuda)
    idx = _pg_runs(N, T, gen, cuda)
    pg = torch.rand(T, generator=gen, device=cuda)
    x_of = lambda: torch.cat([a.double(), b.double(), pg.double()[idx][:, None]], 1)
    if NL == 3:
        def redraw(bad):
            a[bad] = torch.randn(int(bad.sum()), Ca, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    go = torch.randn(N, F, generator=gen, device=cuda)
    ga = torch.full((N, Ca), float("nan"), device=cuda)
    gb = torch.full((N, Cb), float("nan"), device=cuda)
    g_pg = torch.zeros(T, device=cuda)
    out, gws = _abi_heads(NL, F, ws, a, Ca, Ca, b, Cb, Cb, pg, idx, N, go, ga, Ca, gb, Cb, g_pg)
    y64, dx, adx, G, A = _ref_head(x_of(), ws, go)
    _check_rows(out, y64, "out")
    _check_rows(ga, dx[:, :Ca], "grad_a")
    _check_rows(gb, dx[:, Ca:Ca + Cb], "grad_b")
    for k, (g, g_ref, a_ref) in enumerate(zip(gws, G, A)):
        _check_sum(g, g_ref, a_ref, f"param {k}")
    G_pg = torch.zeros(T, dtype=torch.float64, device=cuda).index_add_(0, idx, dx[:, -1])
    A_pg = torch.zeros(T, dtype=torch.float64, device=cuda).index_add_(0, idx, adx[:, -1])
    _check_sum(g_pg, G_pg, A_pg, "pg table")


def _sparse_rows(N, dev):
    """~0.5 % of the rows, on tile / wave / batch / block-range boundaries and at the tail."""
    picks = set()
    for step in (16, 64, 128, 224, 256, 2048):
        for base in range(0, N, step * 37):
            for d in (-1, 0, 1):
                if 0 <= base + d < N:
                    picks.add(base + d)
    picks.update(range(N - 20, N))
    picks.update(range(0, 20))
    return torch.tensor(sorted(picks), dtype=torch.int64, device=dev)


@pytest.mark.parametrize("NL", [1, 3])
def test_heads_sparse_gradient_sees_every_tile(cuda, NL):
    """grad_out is zero except on ~0.5 % of the rows: a dense sum over 640k rows would hide one lost or doubled tile under
    its bound; here ~3,300 rows carry A, so each is ~3e-4 A against a bound of 64 U A = 3.8e-6 A."""
    N, Ca, Cb, F = 640_003, 24, 8, 8
    gen = torch.Generator(device=cuda).manual_seed(300 + NL)
    C_in = Ca + Cb + 1
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a, b = _inputs(N, Ca, Cb, gen, cuda)
    pg = torch.rand(1, generator=gen, device=cuda)
    x_of = lambda: torch.cat([a.double(), b.double(), pg.double().expand(N, 1)], 1)
    if NL == 3:
        def redraw(bad):
            a[bad] = torch.randn(int(bad.sum()), Ca, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    rows = _sparse_rows(N, cuda)
    assert 0.005 * N < rows.numel() < 0.02 * N
    go = torch.zeros(N, F, device=cuda)
    go[rows] = torch.rand(rows.numel(), F, generator=gen, device=cuda) + 0.5      # one sign: no cancellation
    ga = torch.full((N, Ca), float("nan"), device=cuda)
    gb = torch.full((N, Cb), float("nan"), device=cuda)
    g_pg = torch.zeros(1, device=cuda)
    out, gws = _abi_heads(NL, F, ws, a, Ca, Ca, b, Cb, Cb, pg, None, N, go, ga, Ca, gb, Cb, g_pg)
    y64, dx, adx, G, A = _ref_head(x_of(), ws, go)
    _check_rows(ga, dx[:, :Ca], "grad_a")
    assert float(ga[go.abs().sum(1) == 0].abs().max()) == 0.0
    for k, (g, g_ref, a_ref) in enumerate(zip(gws, G, A)):
        _check_sum(g, g_ref, a_ref, f"param {k}")
    _check_sum(g_pg[0], dx[:, -1].sum(), adx[:, -1].sum(), "pg")


def test_context_heads_segments(cuda):
    """ContextHeads: row ranges of ONE matrix with lda > Ca, column offsets c0 (one not a multiple of 4), an empty
    segment, a Pg entry per segment; two segments above 131,072 rows."""
    from cnc_amd.backends.context_backend import ContextHeads
    gen = torch.Generator(device=cuda).manual_seed(99)
    lda, Cb, F = 24, 8, 8
    segs = [(0, 70001, 0, 16, 0), (70001, 70001, 4, 8, 1), (70001, 210000, 8, 16, 2), (210000, 380017, 3, 21, 3)]
    N = segs[-1][1]
    in_a = torch.randn(N, lda, generator=gen, device=cuda)
    in_b = torch.randn(N, Cb, generator=gen, device=cuda)
    pg = torch.rand(4, generator=gen, device=cuda)
    wb = []
    for (_, _, _, Ca, _) in segs:
        W, bias = _head_weights(1, Ca + Cb + 1, F, gen, cuda)
        wb += [W.requires_grad_(), bias.requires_grad_()]
    go = torch.randn(N, F, generator=gen, device=cuda)
    ad, bd, pgd = in_a.clone().requires_grad_(), in_b.clone().requires_grad_(), pg.clone().requires_grad_()
    y = ContextHeads.apply(ad, bd, pgd, tuple(segs), *wb)
    (y * go).sum().backward()
    ga_ref = torch.zeros(N, lda, dtype=torch.float64, device=cuda)
    gb_ref = torch.zeros(N, Cb, dtype=torch.float64, device=cuda)
    G_pg = torch.zeros(4, dtype=torch.float64, device=cuda)
    A_pg = torch.zeros(4, dtype=torch.float64, device=cuda)
    for i, (r0, r1, c0, Ca, pi) in enumerate(segs):
        if r1 == r0:
            assert float(wb[2 * i].grad.abs().max()) == 0.0 and float(wb[2 * i + 1].grad.abs().max()) == 0.0
            continue
        x = torch.cat([in_a[r0:r1, c0:c0 + Ca].double(), in_b[r0:r1].double(), pg[pi].double().expand(r1 - r0, 1)], 1)
        y64, dx, adx, G, A = _ref_head(x, wb[2 * i:2 * i + 2], go[r0:r1])
        _check_rows(y[r0:r1], y64, f"out seg {i}")
        ga_ref[r0:r1, c0:c0 + Ca] = dx[:, :Ca]
        gb_ref[r0:r1] = dx[:, Ca:Ca + Cb]
        G_pg[pi] += dx[:, -1].sum()
        A_pg[pi] += adx[:, -1].sum()
        for k in range(2):
            _check_sum(wb[2 * i + k].grad, G[k], A[k], f"seg {i} param {k}")
    _check_rows(ad.grad, ga_ref, "grad_a")
    _check_rows(bd.grad, gb_ref, "grad_b")
    _check_sum(pgd.grad, G_pg, A_pg, "pg")


@pytest.mark.parametrize("NL", [1, 3])
def test_heads_in_a_gradient_sink(cuda, NL):
    """The training step's route: weight gradients into the sink's 16 replicas at the sink's stride."""
    from cnc_amd import _gradsink
    from cnc_amd.backends.context_backend import ContextMLP
    N, Ca, Cb, F = 640_003, 24, 8, 8
    gen = torch.Generator(device=cuda).manual_seed(500 + NL)
    C_in = Ca + Cb + 1
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a, b = _inputs(N, Ca, Cb, gen, cuda)
    pg = torch.rand((), generator=gen, device=cuda)
    x_of = lambda: torch.cat([a.double(), b.double(), pg.double().expand(N, 1)], 1)
    if NL == 3:
        def redraw(bad):
            a[bad] = torch.randn(int(bad.sum()), Ca, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    go = torch.randn(N, F, generator=gen, device=cuda)
    _, _, _, G, A = _ref_head(x_of(), ws, go)
    other = torch.nn.Parameter(torch.zeros(37, device=cuda))           # a parameter of another head: a non-zero offset
    got = {}
    for use_sink in (False, True):
        leaves = [torch.nn.Parameter(w.clone()) for w in ws]
        sink = _gradsink.GradSink([], [other] + leaves) if use_sink else None
        if sink is not None:
            sink.zero()
        with _gradsink.activate(sink):
            y = ContextMLP.apply(a, b, pg, *(leaves + [None] * (6 - len(leaves))), None)
        (y * go).sum().backward()
        if sink is not None:
            assert all(p.grad is None for p in leaves)
            sink.flush()
        got[use_sink] = [p.grad.clone() for p in leaves]
    for k in range(len(ws)):
        _check_sum(got[True][k], G[k], A[k], f"sink param {k}")
        _check_sum(got[True][k], got[False][k].double(), A[k], f"sink vs plain param {k}")


# ------------------------------------------------------------------------------------------------------------------
# 2. Bernoulli rate (cnc_bernoulli_bits_forward / _backward, cnc_rows_scatter)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rows", [False, True])
@pytest.mark.parametrize("S,F", [(32768, 8), (32769, 8), (150_000, 1), (150_000, 2), (150_000, 4), (150_000, 8)])
def test_bernoulli_rate(cuda, S, F, with_rows):
    """S F = 262,144 is the last size without the grid-stride (1,024 partials); 150,000 x F is the training step's."""
    from cnc_amd.backends import context_backend as K
    gen = torch.Generator(device=cuda).manual_seed(S + F + 7 * with_rows)
    T = 2 ** 19
    pmin = torch.tensor(1e-6, dtype=torch.float32)
    pmax = (1.0 - pmin).to(torch.float32)                           # 1.0f - 1e-6f, as the kernel rounds it
    table = torch.where(torch.rand(T if with_rows else S, F, generator=gen, device=cuda) > 0.4, 1.0, -1.0)
    rows = torch.randperm(T, generator=gen, device=cuda)[:S] if with_rows else None
    mean = torch.rand(S, F, generator=gen, device=cuda) * 1.2 - 0.1
    flat = mean.view(-1)
    for k, v in enumerate([1e-7, float(pmin), float(pmax), 1.0 - 1e-7, 1.0, 0.0, 0.5, 1e-6 * 0.999]):
        flat[k::97] = v
    x = (table[rows] if with_rows else table).double()
    m = mean.double()
    p32 = mean.clamp(float(pmin), float(pmax))
    p = p32.double()
    q = (1.0 - p32).double()                                       # 1.0f - p is rounded in float32 by the kernel too
    pos, neg = (1 + x) / 2, (1 - x) / 2
    terms = -torch.log2(p) * pos - torch.log2(q) * neg
    ref = terms.sum()
    td, md = table.clone().requires_grad_(), mean.clone().requires_grad_()
    got = K.bernoulli_bits(td, rows, md)
    g32 = torch.tensor(0.37, dtype=torch.float32)
    (got * float(g32)).backward()
    # all terms are >= 0: A = the total itself; the kernel's log2f adds a few U per term to the reduction's depth
    ratio_total = abs(float(got.detach()) - float(ref)) / (C_SUM * U * float(ref))
    _note("bernoulli total", ratio_total)
    assert ratio_total <= 1.0
    gs = float(g32)
    inside = (m >= float(pmin)) & (m <= float(pmax))
    gm_ref = torch.where(inside, gs * (-pos / p + neg / q) / np.log(2.0), torch.zeros_like(m))
    # one division, the rounded 1 / ln 2, two products: <= 4 U relative
    _note("bernoulli grad_mean", ((md.grad.double() - gm_ref).abs() / (8 * U * gm_ref.abs() + 1e-300)).max())
    assert float(((md.grad.double() - gm_ref).abs() - 8 * U * gm_ref.abs()).max()) <= 0.0
    assert bool((md.grad[~inside] == 0).all())
    gx_ref = gs * 0.5 * (-torch.log2(p) + torch.log2(q))
    gx_bound = 8 * U * gs * 0.5 * (torch.log2(p).abs() + torch.log2(q).abs()) + 1e-30
    if with_rows:
        off = torch.ones(T, dtype=torch.bool, device=cuda)
        off[rows] = False
        assert bool((td.grad[off] == 0).all())                     # exactly zero off the coded rows
        gx = td.grad[rows]
    else:
        gx = td.grad
    _note("bernoulli grad_table", ((gx.double() - gx_ref).abs() / gx_bound).max())
    assert float(((gx.double() - gx_ref).abs() - gx_bound).max()) <= 0.0
    again = K.bernoulli_bits(table, rows, mean)
    assert float(again) == float(got.detach())                     # the partials make the total deterministic


def test_rows_scatter_writes_only_its_rows(cuda):
    L = _lib()
    gen = torch.Generator(device=cuda).manual_seed(8)
    T, S, F = 2 ** 19, 150_000, 8
    rows = torch.randperm(T, generator=gen, device=cuda)[:S]
    vals = torch.randn(S, F, generator=gen, device=cuda)
    table = torch.full((T, F), float("nan"), device=cuda)
    L.check(L.lib().cnc_rows_scatter(vals.data_ptr(), rows.data_ptr(), table.data_ptr(), S, F, L.stream(cuda)), "rows_scatter")
    assert torch.equal(table[rows], vals)
    off = torch.ones(T, dtype=torch.bool, device=cuda)
    off[rows] = False
    assert bool(torch.isnan(table[off]).all())


# ------------------------------------------------------------------------------------------------------------------
# 3. Level statistics (cnc_level_stats_forward / _backward)
# ------------------------------------------------------------------------------------------------------------------
def _layout(name):
    from cnc_amd import synthetic
    if name == "3d":
        offs = make_grid(synthetic.RES_3D_REF, 19, 3, 1)[0]
        return offs, {9: 0.0, 10: 1.0, 11: 0.5}          # levels 6-11 hold 2^19 rows each
    if name == "2d":
        offs = make_grid(synthetic.RES_2D_REF, 17, 2, 1)[0]
        return offs, {0: 0.0, 2: 1.0, 3: 0.5}
    sizes = [1, 3, 2047, 2049, 7, 4096, 1, 5000, 8, 2048, 13, 100, 2050, 1, 1, 777] * 2       # kMaxLevels = 32
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), {1: 0.0, 3: 1.0, 5: 0.5, 30: 0.0}


def _level_offsets_arg(offs):
    arr = (C.c_int64 * len(offs))(*[int(o) for o in offs])
    return arr, C.cast(arr, C.c_void_p)


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
@pytest.mark.parametrize("layout", ["3d", "2d", "32"])
def test_level_stats(cuda, layout, F, misaligned):
    """Rows before the first level and past the last belong to no level; levels with Pg = 0, 1 and exactly 1/2 (where
    the (pos dA + neg dB) term of the backward cancels); a table view 4 bytes past a 16-byte boundary (scalar path)."""
    from cnc_amd.context import _zero_order_bits
    L = _lib()
    lib, st = L.lib(), L.stream(cuda)
    gen = torch.Generator(device=cuda).manual_seed(F * 3 + misaligned + len(layout))
    base, special = _layout(layout)
    lead, tail = 5, 11
    offs = np.asarray(base, np.int64) + lead
    n_lv = len(offs) - 1
    rows = int(offs[-1]) + tail
    table = _offset_view(rows * F, 1 if misaligned else 0, cuda).view(rows, F)
    assert (table.data_ptr() % 16 == 4) == misaligned
    probs = torch.rand(n_lv, generator=gen, device=cuda)
    table.copy_(torch.where(torch.rand(rows, F, generator=gen, device=cuda) < 0.5, 1.0, -1.0))
    for l in range(n_lv):
        lv = table[int(offs[l]):int(offs[l + 1])]
        if l in special and special[l] == 0.5:
            n = lv.numel()
            assert n % 2 == 0
            v = torch.full((n,), -1.0, device=cuda)
            v[torch.randperm(n, generator=gen, device=cuda)[:n // 2]] = 1.0
            lv.copy_(v.view_as(lv))
        elif l in special:
            lv.fill_(1.0 if special[l] == 1.0 else -1.0)
        else:
            lv.copy_(torch.where(torch.rand(lv.shape, generator=gen, device=cuda) < probs[l], 1.0, -1.0))
    if layout == "3d":
        assert int(offs[12] - offs[11]) * F == 2 ** 19 * F
    arr, offs_p = _level_offsets_arg(offs)
    sums = torch.full((n_lv,), float("nan"), dtype=torch.float64, device=cuda)
    Pg = torch.full((n_lv,), float("nan"), device=cuda)
    bits = torch.full((n_lv,), float("nan"), device=cuda)
    L.check(lib.cnc_level_stats_forward(table.data_ptr(), offs_p, n_lv, F, sums.data_ptr(), Pg.data_ptr(), bits.data_ptr(), st),
            "level_stats_forward")
    s_ref = torch.stack([table[int(offs[l]):int(offs[l + 1])].double().sum() for l in range(n_lv)])
    assert torch.equal(sums, s_ref)                              # sums of +-1 are integer counts: exact
    # float64 autograd of the formula (cnc_amd.context._zero_order_bits)
    gP = torch.randn(n_lv, generator=gen, device=cuda)
    gB = torch.randn(n_lv, generator=gen, device=cuda)
    s64 = s_ref.clone().requires_grad_()
    ttl = torch.as_tensor(np.diff(offs) * F, dtype=torch.float64, device=cuda)
    pos, neg = (ttl + s64) / 2, (ttl - s64) / 2
    Pg64 = pos / ttl
    bits64 = _zero_order_bits(pos, neg, Pg64)
    ((Pg64 * gP.double()).sum() + (bits64 * gB.double()).sum()).backward()
    ds = s64.grad
    for l, v in special.items():
        assert float(Pg[l]) == v
    assert float(((Pg.double() - Pg64.detach()).abs() - 2 * U * Pg64.detach()).max()) <= 0.0
    lA = -torch.log2(Pg64.detach().clamp_min(1e-9))
    lB = -torch.log2((1 - Pg64.detach()).clamp_min(1e-9))
    pos_, neg_ = pos.detach(), neg.detach()
    # Pg and 1 - Pg are rounded once each: -log2 of them is off by <= U / ln 2 absolute, times pos / neg; plus log2f
    bits_bound = 8 * U * (pos_ * lA + neg_ * lB + ttl)
    _note("level bits", ((bits.double() - bits64.detach()).abs() / bits_bound).max())
    assert float(((bits.double() - bits64.detach()).abs() - bits_bound).max()) <= 0.0
    assert float(bits[[l for l, v in special.items() if v != 0.5]].abs().max()) == 0.0
    g = _offset_view(rows * F, 1 if misaligned else 0, cuda, fill=float("nan")).view(rows, F)
    L.check(lib.cnc_level_stats_backward(sums.data_ptr(), offs_p, n_lv, F, gP.data_ptr(), gB.data_ptr(), rows, g.data_ptr(), st),
            "level_stats_backward")
    assert torch.isfinite(g).all()
    assert float(g[:lead].abs().max()) == 0.0 and float(g[int(offs[-1]):].abs().max()) == 0.0
    # d bits / d s = (A - B) / 2 + (pos dA + neg dB) / (2 ttl): the second term is 0 in exact arithmetic and a few U
    # after rounding (pos / Pg and neg / (1 - Pg) are ~ttl each)
    d_bound = 8 * U * (gP.double().abs() * 0.5 / ttl + gB.double().abs() * (0.5 * (lA + lB) + 1.0 / np.log(2.0))) + 1e-30
    lvl = torch.repeat_interleave(torch.arange(n_lv, device=cuda), torch.as_tensor(np.diff(offs), device=cuda))
    inner = g[int(offs[0]):int(offs[-1])].double()
    err = (inner - ds[lvl][:, None]).abs()
    _note("level grad", (err / d_bound[lvl][:, None]).max())
    assert float((err - d_bound[lvl][:, None]).max()) <= 0.0
    for l in [l for l, v in special.items() if v == 0.5]:
        # Pg = 1/2: A = B = 1 and pos dA = -neg dB exactly, so the rows get g_Pg dPg/ds alone, bit for bit
        lv = g[int(offs[l]):int(offs[l + 1])]
        dp = torch.tensor(0.5, device=cuda) / ttl[l].float()
        assert bool((lv == gP[l] * dp).all()), l


def test_level_stats_refuses_33_levels(cuda):
    L = _lib()
    offs = np.arange(34, dtype=np.int64) * 16
    arr, offs_p = _level_offsets_arg(offs)
    table = torch.ones(int(offs[-1]), 8, device=cuda)
    sums = torch.zeros(33, dtype=torch.float64, device=cuda)
    Pg, bits = torch.zeros(33, device=cuda), torch.zeros(33, device=cuda)
    rc = L.lib().cnc_level_stats_forward(table.data_ptr(), offs_p, 33, 8, sums.data_ptr(), Pg.data_ptr(), bits.data_ptr(),
                                         L.stream(cuda))
    assert rc != 0
    g = torch.zeros_like(table)
    rc = L.lib().cnc_level_stats_backward(sums.data_ptr(), offs_p, 33, 8, Pg.data_ptr(), bits.data_ptr(), table.shape[0],
                                          g.data_ptr(), L.stream(cuda))
    assert rc != 0


# ------------------------------------------------------------------------------------------------------------------
# 4. Votes at the training size (R = 514: Rb = 128, t = 4, T = 2^19)
# ------------------------------------------------------------------------------------------------------------------
def _vertex_set(occ, t):
    """The vertex list get_idx_coords2 builds (the construction of
    test_vote_plan_from_the_occupancy_grid_equals_the_plan_from_the_vertex_list)."""
    m = occ
    for axis in range(3):
        up = m.repeat_interleave(t, dim=axis)
        n = up.shape[axis]
        shape = list(up.shape)
        shape[axis] = n + 2
        out = torch.zeros(shape, dtype=torch.bool, device=occ.device)
        for sft in range(3):
            out.narrow(axis, sft, n).logical_or_(up)
        m = out
    return torch.nonzero(m).to(torch.int16).contiguous()


def _vote_setup(cuda, Rb, t, log2T):
    from cnc_amd.backends import gridencoder_backend as be
    occ = torch.as_tensor(ball_occupancy(Rb), device=cuda)
    occ[0, :, Rb // 3] = True                                    # cells on the box faces: vertices cnt_np_embed skips
    occ[-1, Rb // 2, :] = True
    occ[:, 0, -1] = True
    R, hs = Rb * t + 2, 2 ** log2T
    verts = _vertex_set(occ, t)
    plans = {"list": be.VotePlan(verts, R, hs), "occupancy": be.VotePlan.from_occupancy(occ, t, R, hs)}
    assert plans["list"].xyz_by_row is None and plans["occupancy"].xyz_by_row is not None
    return dict(R=R, hs=hs, pts=verts.cpu().numpy(), plans=plans)


@pytest.fixture(scope="module")
def votes_full(cuda, oracle):
    return _vote_setup(cuda, 128, 4, 19)


def _check_votes(cuda, oracle, setup, F, seed):
    from cnc_amd.backends import gridencoder_backend as be
    R, hs, pts = setup["R"], setup["hs"], setup["pts"]
    S = R - 2
    rows = min(hs, R ** 3)
    rng = np.random.default_rng(seed)
    emb = np.where(rng.uniform(size=(rows, F)) < 0.5, 1.0, -1.0).astype(np.float32)
    emb[::5] *= 0.5                                              # not +-1: 0.5 is a "no" vote (> 0.9 test)
    gs = [rng.normal(size=(S, S, F, 2)).astype(np.float32) for _ in range(3)]
    ones = np.ones((S, S, F, 1), np.float32)
    with ThreadPoolExecutor(9) as pool:                         # ctypes releases the GIL: the oracle calls run side by side
        fwd = [pool.submit(oracle.cnt_np_embed, pts, emb, R, hs, axis) for axis in range(3)]
        bwd = [pool.submit(oracle.cnt_np_embed_backward, pts, emb, ones, g, R, hs, axis, True) for axis, g in enumerate(gs)]
        bwd_abs = [pool.submit(oracle.cnt_np_embed_backward, pts, emb, ones, np.abs(g), R, hs, axis, True)
                   for axis, g in enumerate(gs)]
        want = [f.result() for f in fwd]
        acc = sum(f.result()[1] for f in bwd)
        absacc = sum(f.result()[1] for f in bwd_abs)
    t = lambda a: torch.as_tensor(a, device=cuda)
    emb_d = t(emb)
    gs_d = [t(g) for g in gs]
    bound = 64 * np.finfo(np.float32).eps * np.abs(absacc) + 1e-30
    for name, plan in setup["plans"].items():
        for axis in range(3):
            out = torch.full((S, S, F, 2), -7.0, device=cuda)
            be.cnt_np_embed_planned(plan, emb_d, out, F, axis)
            assert np.array_equal(out.cpu().numpy(), want[axis]), (name, axis)
        ge = torch.full((rows, F), float("nan"), device=cuda)
        be.cnt_np_embed_planned_backward3(plan, emb_d, gs_d, ge, F)
        err = np.abs(ge.cpu().numpy().astype(np.float64) - acc)
        _note("votes backward", (err / bound).max())
        assert np.all(err <= bound), (name, float((err / bound).max()))
    assert float(np.abs(acc).max()) > 0
    return want


@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_votes_at_training_size(cuda, oracle, votes_full, F):
    """Both plans' masked counts equal the oracle's on all three planes; the three-plane backward (pixel route for the
    list plan, packed-vertex route for the occupancy plan) lies within the oracle's float64-shadow bound."""
    assert votes_full["pts"].shape[0] > 10 ** 7
    _check_votes(cuda, oracle, votes_full, F, seed=F)


def test_votes_dense_level(cuda, oracle):
    """R^3 <= T: the finest level is dense (row = x + y R + z R^2)."""
    setup = _vote_setup(cuda, 16, 4, 19)
    assert setup["R"] ** 3 <= setup["hs"]
    _check_votes(cuda, oracle, setup, 8, seed=11)


# cnc_vote_fraction_table{,_backward} against float64, in units of U relative to the value: one division and one sum
FRACTION_U = {"table": 4, "sums": 2, "grad": 3}


def test_vote_fraction_tables(cuda, oracle, votes_full):
    """cnc_vote_fraction_table{,_backward} (the kernels of `_vote_tables3`) against a float64 restatement:
    c0 / ((c0 + c1) + 1e-6) on the inner pixels and a ring of zeros; back, [(1 / sum) g, 0]."""
    L = _lib()
    lib, st = L.lib(), L.stream(cuda)
    F, R, hs = 8, votes_full["R"], votes_full["hs"]
    S = R - 2
    rng = np.random.default_rng(3)
    emb = np.where(rng.uniform(size=(hs, F)) < 0.5, 1.0, -1.0).astype(np.float32)
    cnt = torch.as_tensor(oracle.cnt_np_embed(votes_full["pts"], emb, R, hs, 1), device=cuda)
    table = torch.full((R * R, F), float("nan"), device=cuda)
    sums = torch.full((S, S, F), float("nan"), device=cuda)
    L.check(lib.cnc_vote_fraction_table(cnt.data_ptr(), S, F, table.data_ptr(), sums.data_ptr(), st), "vote_fraction_table")
    c = cnt.double()
    den = c[..., 0] + c[..., 1] + 1e-6
    ref = c[..., 0] / den
    tab = table.view(R, R, F)
    assert float(tab[0].abs().max()) == 0 and float(tab[-1].abs().max()) == 0
    assert float(tab[:, 0].abs().max()) == 0 and float(tab[:, -1].abs().max()) == 0
    inner = tab[1:-1, 1:-1].double()
    assert float(((inner - ref).abs() - FRACTION_U["table"] * U * ref.abs()).max()) <= 0.0
    assert float(((sums.double() - den).abs() - FRACTION_U["sums"] * U * den).max()) <= 0.0
    assert float(ref.max()) > 0.5 and float(ref.min()) == 0.0
    g = torch.randn(R * R, F, device=cuda)
    gos = torch.full((S, S, F, 2), float("nan"), device=cuda)
    L.check(lib.cnc_vote_fraction_table_backward(g.data_ptr(), sums.data_ptr(), S, F, gos.data_ptr(), st),
            "vote_fraction_table_backward")
    g_in = g.view(R, R, F)[1:-1, 1:-1].double()
    want = g_in / sums.double()
    assert float(((gos[..., 0].double() - want).abs() - FRACTION_U["grad"] * U * want.abs()).max()) <= 0.0
    assert float(gos[..., 1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------
# 5. Gathers at full size, and the whole pass at configs[2]
# ------------------------------------------------------------------------------------------------------------------
def test_window_gather_at_the_window_limit(cuda):
    """cnc_ctx_window_gather over kMaxWin = 16 windows (int16 vertices up to 513, configs[2]-sized slot windows) equals
    the tensor expressions it replaces bit for bit: copies, and (x - 0.5) / (R - 2) rounded once."""
    from cnc_amd import synthetic
    from cnc_amd.backends import context_backend as K
    gen = torch.Generator(device=cuda).manual_seed(16)
    res = (synthetic.RES_3D_REF + synthetic.RES_3D_REF)[:16]
    levels, want = [], {k: [] for k in ("pts", "pts_n", "lvl", "res", "cnt", "rows")}
    row0 = 0
    for w, R in enumerate(res):
        V = 150_000 // 12 + 37 * w
        P = 3 * V + w
        pos = torch.randint(0, R, (P, 3), generator=gen, device=cuda).to(torch.int16)
        pos[w] = R - 1
        cnt = torch.randint(0, 7, (V,), generator=gen, device=cuda)
        val = torch.randint(0, 2 ** 19, (V,), generator=gen, device=cuda)
        levels.append(dict(pos=pos, cnt=cnt, val=val, level=w % 12, res=R, row0=row0))
        want["pts"].append(pos)
        want["pts_n"].append((pos - 0.5) / torch.tensor([R - 2], device=cuda))
        want["lvl"].append(torch.full((P,), w % 12, dtype=torch.int64, device=cuda))
        want["res"].append(torch.full((P,), R, dtype=torch.int64, device=cuda))
        want["cnt"].append(cnt)
        want["rows"].append(val + row0)
        row0 += 2 ** 19
    assert int(max(res)) == 514
    got = K.window_gather(levels, cuda)
    for g, k in zip(got, ("pts", "pts_n", "lvl", "res", "cnt", "rows")):
        w = torch.cat(want[k])
        assert g.dtype == w.dtype and torch.equal(g, w), k


def test_compact_masked_at_full_size(cuda):
    from cnc_amd.backends import context_backend as K
    gen = torch.Generator(device=cuda).manual_seed(17)
    N, L = 750_001, 3
    pts_n = torch.rand(N, 3, generator=gen, device=cuda) * 2 - 0.5
    level_ids = torch.randint(3, 12, (N,), generator=gen, device=cuda)
    overlap = torch.randint(-2, 9, (N,), generator=gen, device=cuda).to(torch.int32)
    idx = torch.nonzero(torch.rand(N, generator=gen, device=cuda) < 0.6).squeeze(1)
    pts_m, lvl_m, min_l, ow = K.compact_masked(idx, pts_n, level_ids, overlap, L)
    assert torch.equal(pts_m, pts_n[idx]) and torch.equal(lvl_m, level_ids[idx])
    assert torch.equal(min_l, (level_ids[idx] - L).to(torch.int32))
    assert torch.equal(ow, torch.clamp(overlap[idx], min=1).to(torch.float32))
    _, _, _, none = K.compact_masked(idx, pts_n, level_ids, None, L)
    assert none is None


@pytest.mark.parametrize("axis", ["xy", "xz", "yz"])
def test_plane_ring_vertices_of_the_projected_ball(cuda, axis):
    """Every occupied cell of a 128^2 projection of the training step's occupancy, at the plane levels R = 514 (T = 4)
    and 1026 (T = 8), hashed into 2^17 rows."""
    from cnc_amd.backends import context_backend as K
    from cnc_amd.context import CNC_context_models, get_grid_index
    from cnc_amd.synthetic import ball_binaries
    plane = CNC_context_models._project(ball_binaries(128, radius=1.0, device=cuda), axis).clone()
    plane[-1, ::3] = True                    # cells on the border: vertices up to R - 1
    plane[::5, 0] = True
    cells = torch.nonzero(plane).contiguous()
    assert cells.shape[0] > 5000
    for R, T in ((514, 4), (1026, 8)):
        hs = 2 ** 17
        rows, pts = K.plane_ring_vertices(cells, T, R, hs)
        ar = torch.arange(T + 2, device=cuda)
        ring = torch.stack(torch.meshgrid(ar, ar, indexing="ij"), dim=-1).view(1, T + 2, T + 2, 2)
        v = (cells.view(-1, 1, 1, 2) * T + ring).view(-1, 2)
        assert int(v.max()) == R - 1 and int(v.min()) == 0
        assert torch.equal(rows.long(), get_grid_index(hs, R, v))
        assert torch.equal(pts, (v - 0.5) / float(R - 2))


def _configs2_model(cuda, F=8, seed=5, **kw):
    from cnc_amd import synthetic
    from cnc_amd.context import CNC_context_models
    from cnc_amd.gridencoder import GridEncoder
    torch.manual_seed(seed)
    m = CNC_context_models(num_dim=3, resolutions_list=synthetic.RES_3D_REF, resolutions_list_2D=synthetic.RES_2D_REF,
                           log2_hashmap_size=19, log2_hashmap_size_2D=17, n_features=F, sample_num=150000,
                           max_context_layer_num=3, ste_binary=True, Pg_level=12, Pg_level_2D=4, Rb=128,
                           step_update=16, skip_levels_3D=[0, 1, 2], skip_levels_2D=[0], device=cuda, **kw)
    encs = [GridEncoder(3, F, synthetic.RES_3D_REF, 19, ste_binary=True).to(cuda)] + \
           [GridEncoder(2, F, synthetic.RES_2D_REF, 17, ste_binary=True).to(cuda) for _ in range(3)]
    with torch.no_grad():
        for e in encs:       # spatially smooth signs, as test_full_size_encode_decode_roundtrip sets them
            e.params.copy_(torch.sin(torch.arange(e.params.shape[0], device=cuda).float()[:, None] * 0.01
                                     + torch.arange(F, device=cuda).float()) + 0.3 * torch.randn_like(e.params))
    return m, encs


def _configs2_pass(m, encs, binaries, seed=77):
    torch.manual_seed(seed)
    for p in [q for e in encs for q in e.parameters()] + list(m.parameters()):
        p.grad = None
    bpp, _ = m.forward_binary_vxl_mixPg_3D2D(*encs, binaries, step=0)
    bpp.backward()
    return float(bpp.detach()), [e.params.grad.clone() for e in encs], [p.grad.clone() for p in m.parameters()
                                                                         if p.grad is not None]


@pytest.fixture(scope="module")
def configs2_fused_and_chain(cuda):
    """The whole configs[2] training pass with the fused heads off and on; the rows handed to each Bernoulli rate call are
    checked to be distinct on the way (cnc_rows_scatter stores, it does not add)."""
    from cnc_amd.synthetic import ball_binaries
    binaries = ball_binaries(128, radius=1.0, device=cuda)
    outs = []
    for fused in (False, True):
        m, encs = _configs2_model(cuda, fused_heads=fused)
        seen = []
        bits = m._bits

        def spy(table_q, rows, mean, bits=bits, seen=seen):
            seen.append(int(rows.numel()))
            assert torch.unique(rows).numel() == rows.numel(), "rows of one rate call repeat"
            return bits(table_q, rows, mean)
        m._bits = spy
        outs.append(_configs2_pass(m, encs, binaries) + (seen,))
    return outs


def _toy_bound_check(a, b, what, note=True):
    scale = max(float(a.abs().max()), 1e-12)
    # the toy test's bound, unchanged: the two passes add the same float32 terms in different orders (GEMM reductions
    # against LDS tiles and atomics), so they differ by <= depth x eps x sum|terms| each
    if note:
        _note("configs2 fused vs chain", float((a - b).abs().max()) / (3e-3 * scale))
    assert float((a - b).abs().max()) <= 3e-3 * scale, what


def test_configs2_fused_heads_equal_the_op_chain(configs2_fused_and_chain):
    """The configs[2] counterpart of test_context_pass_fused_heads_equals_op_chain: same rate (1e-5 relative), same
    gradients for the 3-D table and every context-model weight, distinct rows in every rate call."""
    (b0, ge0, gp0, seen0), (b1, ge1, gp1, seen1) = configs2_fused_and_chain
    assert len(seen0) >= 4 and len(seen1) >= 2 and min(seen0 + seen1) > 0
    assert abs(b0 - b1) <= 1e-5 * abs(b0)
    assert len(gp0) == len(gp1) > 0
    _toy_bound_check(ge0[0], ge1[0], "3-D table")
    for k, (a, b) in enumerate(zip(gp0, gp1)):
        _toy_bound_check(a, b, f"context-model parameter {k}")


def test_configs2_fused_heads_plane_gradients_equal_the_op_chain(cuda):
    """The plane tables' gradients of the same comparison.  The rate's gradient in a predicted P(+1) = p is
    -1 / (p ln 2) (+1 entries): where an untrained 2-D head predicts p near the 1e-6 clamp, the float32 rounding of
    the head's dot product (~C U sum|w x| ~ 1e-7 absolute, different in the two routes) is a relative change of
    ~1e-7 / p in that row's gradient — tenths at p ~ 1e-6 — and those rows carry the plane tables' largest entries.
    Nothing but conditioning: with the untrained heads the routes differ by ~1 % there (measured), and with the
    predictions held inside [0.2, 0.8] (weights x 0.05, bias 0.5: |w x| <= 33 x 0.0087), where 1 / p stays below 8,
    they agree within the toy test's bound."""
    from cnc_amd.synthetic import ball_binaries
    binaries = ball_binaries(128, radius=1.0, device=cuda)
    outs = []
    for fused in (False, True):
        m, encs = _configs2_model(cuda, fused_heads=fused)
        with torch.no_grad():
            for head in m.context_model_2D:
                lin = [x for x in head if isinstance(x, torch.nn.Linear)] if isinstance(head, torch.nn.Sequential) else [head]
                lin[0].weight.mul_(0.05)
                lin[0].bias.fill_(0.5)
        outs.append(_configs2_pass(m, encs, binaries))
    (b0, ge0, gp0), (b1, ge1, gp1) = outs
    assert abs(b0 - b1) <= 1e-5 * abs(b0)
    for k in (1, 2, 3):
        assert float(ge1[k].abs().max()) > 0
        _toy_bound_check(ge0[k], ge1[k], f"plane table {k}")
    for k, (a, b) in enumerate(zip(gp0, gp1)):
        _toy_bound_check(a, b, f"context-model parameter {k}")


def test_configs2_planned_votes_equal_atomic_votes(cuda):
    """The configs[2] counterpart of test_planned_votes_equal_atomic_votes: the vote plans (R = 514, T = 2^19) against
    the atomic cnt_np_embed kernels in the whole pass — the same rate bit for bit (integer counts), the same gradients."""
    from cnc_amd.synthetic import ball_binaries
    binaries = ball_binaries(128, radius=1.0, device=cuda)
    m, encs = _configs2_model(cuda)
    res = {}
    for planned in (True, False):
        m.planned_votes = planned
        bpp, ge, gp = _configs2_pass(m, encs, binaries)
        assert (m.vote_plan is not None) == planned
        res[planned] = (bpp, ge[0], ge[1], gp[0])
    assert res[True][0] == res[False][0]
    for a, b in zip(res[True][1:], res[False][1:]):
        assert float(b.abs().max()) > 0
        assert (a - b).abs().max() <= 1e-5 * b.abs().max()
