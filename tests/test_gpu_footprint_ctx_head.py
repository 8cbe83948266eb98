"""Footprint of the context heads (cnc_amd/csrc/ctx_head.hip: cnc_ctx_mlp_forward, cnc_ctx_mlp_backward,
cnc_ctx_mlp_backward_ordered) through the C ABI: every buffer of a call — inputs, weights, the Pg table and its
int64 index of exactly N entries, gradients, scratch — lies in a guarded allocation (tests/guarded.py) whose
surroundings, and the gap columns of in_a / in_b / grad_a / grad_b where lda > Ca or ldb > Cb, hold 0x00, 0xA5 and 0xFF
in turn.  `for_each_input` and `head3_fetch4` take 16-byte loads when `seg_vec_ok` / `veca` / `vecb` allow it: the
`_shift4` layout puts the same windows four bytes off, on the other side of that gate.

The forward and the ordered backward are the same bits under every fill; the plain backward sums its parameter
gradients with atomics and is held, under each fill separately, by `_check_rows` / `_check_sum` of
tests/test_gpu_context_matrix.py against its float64 reference.

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import numpy as np
import pytest
import torch

from guarded import FILLS, Guarded, moved_with_fill, same_bits, under_fills
from test_gpu_context_matrix import WIDTHS, _avoid_kinks, _check_rows, _check_sum, _head_weights, _ref_head

pytestmark = pytest.mark.gpu
f32 = np.float32
T = 4            # entries of the Pg table (the last belongs to no row)

# name -> (Ca, lda, c0, Cb, ldb, pg table, shift)
_odd, _str, _c33 = WIDTHS["odd_ca"], WIDTHS["strided"], WIDTHS["c33"]
LAYOUTS = {
    "odd_ca": (_odd[0], _odd[1], _odd[2], _odd[3], _odd[3], False, 0),             # Ca % 4 != 0: the scalar fetch
    "windows": (_str[0], _str[1], _str[2], _str[3], _str[3] + 4, False, 0),        # lda > Ca and ldb > Cb, 16-byte loads
    "windows_shift4": (_str[0], _str[1], _str[2], _str[3], _str[3] + 4, False, 4),   # the same, scalar
    "pg_index": (_c33[0], _c33[1], _c33[2], _c33[3], _c33[3], True, 0),            # packed rows, Pg through an index
}


def _case(cuda, NL, layout, F, N):
    Ca, lda, c0, Cb, ldb, table, shift = LAYOUTS[layout]
    gen = torch.Generator(device=cuda).manual_seed(100 * NL + 10 * list(LAYOUTS).index(layout) + F + N)
    C_in = Ca + Cb + 1
    ws = _head_weights(NL, C_in, F, gen, cuda)
    a = torch.randn(N, Ca, generator=gen, device=cuda)
    b = torch.randn(N, Cb, generator=gen, device=cuda)
    pg = torch.rand(T if table else 1, generator=gen, device=cuda)
    idx = (torch.arange(N, device=cuda) * 3 // N) if table else None           # three runs; entry T - 1 is unused
    x_of = lambda: torch.cat([a.double(), b.double(), (pg.double()[idx] if table else pg.double().expand(N))[:, None]], 1)
    if NL == 3:
        def redraw(bad):
            a[bad] = torch.randn(int(bad.sum()), Ca, generator=gen, device=cuda)
        _avoid_kinks(x_of, redraw, ws, C_in)
    go = torch.randn(N, F, generator=gen, device=cuda)
    y64, dx, adx, G, A = _ref_head(x_of(), ws, go)
    if table:
        G_pg = torch.zeros(T, dtype=torch.float64, device=cuda).index_add_(0, idx, dx[:, -1])
        A_pg = torch.zeros(T, dtype=torch.float64, device=cuda).index_add_(0, idx, adx[:, -1])
    else:
        G_pg, A_pg = dx[:, -1].sum().reshape(1), adx[:, -1].sum().reshape(1)
    host = dict(a=a, b=b, pg=pg, go=go, **{f"w{k}": w for k, w in enumerate(ws)})
    host = {k: v.cpu().numpy() for k, v in host.items()}
    if table:
        host["idx"] = idx.cpu().numpy().astype(np.int64)
    return host, len(ws), (y64, dx, G, A, G_pg, A_pg)


def _inputs(host, n_w, layout, N, cuda, fill):
    Ca, lda, c0, Cb, ldb, table, shift = LAYOUTS[layout]
    b = {"a": Guarded.window(host["a"], lda, c0, cuda, fill, shift), "b": Guarded.window(host["b"], ldb, 0, cuda, fill, shift),
         "pg": Guarded(host["pg"], cuda, fill=fill), "go": Guarded(host["go"], cuda, fill=fill),
         "idx": Guarded(host["idx"], cuda, fill=fill) if table else None}
    assert b["a"].ptr % 16 == (4 * c0 + shift) % 16 and b["b"].ptr % 16 == shift
    for k in range(n_w):
        b[f"w{k}"] = Guarded(host[f"w{k}"], cuda, fill=fill)
    return b


def _head_args(b, layout, n_w):
    Ca, lda, c0, Cb, ldb, table, shift = LAYOUTS[layout]
    head = (b["a"].ptr, lda, Ca, b["b"].ptr, ldb, Cb, b["pg"].ptr, b["idx"].ptr if table else None)
    return head, [b[f"w{k}"].ptr for k in range(n_w)] + [None] * (6 - n_w)


def _grad_outputs(host, n_w, layout, N, cuda, fill):
    Ca, lda, c0, Cb, ldb, table, shift = LAYOUTS[layout]
    o = {"g_a": Guarded.empty_window(N, Ca, lda, c0, f32, cuda, fill, shift),
         "g_b": Guarded.empty_window(N, Cb, ldb, 0, f32, cuda, fill, shift),
         "g_pg": Guarded(np.zeros(host["pg"].shape, f32), cuda, fill=fill).out()}            # accumulated: start at zero
    for k in range(n_w):
        o[f"gw{k}"] = Guarded(np.zeros(host[f"w{k}"].shape, f32), cuda, fill=fill).out()
    return o


@pytest.mark.parametrize("N", [1, 17, 257])
@pytest.mark.parametrize("F", [1, 8])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("NL", [1, 3])
def test_heads_depend_on_their_buffers_alone(cuda, NL, layout, F, N):
    from cnc_amd import _lib
    L, st = _lib.lib(), _lib.stream(cuda)
    Ca, lda, c0, Cb, ldb, table, shift = LAYOUTS[layout]
    host, n_w, (y64, dx, G, A, G_pg, A_pg) = _case(cuda, NL, layout, F, N)
    dev = lambda a: torch.from_numpy(a).to(cuda)

    # forward
    def build(fill):
        return dict(_inputs(host, n_w, layout, N, cuda, fill), out=Guarded.empty((N, F), f32, cuda, fill=fill))

    def run(b):
        head, w6 = _head_args(b, layout, n_w)
        _lib.check(L.cnc_ctx_mlp_forward(*head, N, NL, F, *w6, b["out"].ptr, st), "ctx_mlp_forward")

    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    _check_rows(dev(res[FILLS[0]]["out"]), y64, "out")

    # backward: plain (atomics into one replica) and ordered
    ws_bytes = int(L.cnc_ctx_mlp_backward_ordered_workspace(N, NL, F, Ca + Cb + 1, T if table else 1))

    def build_bwd(fill, ordered):
        b = dict(_inputs(host, n_w, layout, N, cuda, fill), **_grad_outputs(host, n_w, layout, N, cuda, fill))
        if ordered:
            b["ws"] = Guarded.empty((ws_bytes,), np.uint8, cuda, fill=fill).scratch()
        return b

    def run_bwd(b, ordered):
        head, w6 = _head_args(b, layout, n_w)
        tail = (*w6, b["go"].ptr, b["g_a"].ptr, b["g_b"].ptr, b["g_pg"].ptr,
                *([b[f"gw{k}"].ptr for k in range(n_w)] + [None] * (6 - n_w)))
        if ordered:
            rc = L.cnc_ctx_mlp_backward_ordered(*head, T, N, NL, F, *tail, lda, ldb, b["ws"].ptr, ws_bytes, st)
        else:
            rc = L.cnc_ctx_mlp_backward(*head, N, NL, F, *tail, 1, 0, lda, ldb, st)
        _lib.check(rc, "ctx_mlp_backward")

    def check(r, what):
        for k, v in r.items():
            assert np.isfinite(v).all(), (what, k)
        _check_rows(dev(r["g_a"]), dx[:, :Ca], f"{what}: grad_a")
        _check_rows(dev(r["g_b"]), dx[:, Ca:Ca + Cb], f"{what}: grad_b")
        for k in range(n_w):
            _check_sum(dev(r[f"gw{k}"]), G[k], A[k], f"{what}: param {k}")
        _check_sum(dev(r["g_pg"]), G_pg, A_pg, f"{what}: pg")

    plain = under_fills(lambda fill: build_bwd(fill, False), lambda b: run_bwd(b, False))
    for fill in FILLS:
        check(plain[fill], f"plain, fill {fill:#x}")
    ordered = under_fills(lambda fill: build_bwd(fill, True), lambda b: run_bwd(b, True))
    assert moved_with_fill(ordered) == []
    check(ordered[FILLS[0]], "ordered")
    # the per-row gradients hold no reduction: the plain entry's are the ordered entry's bits, under every fill
    for fill in FILLS:
        assert same_bits(plain[fill]["g_a"], ordered[fill]["g_a"]) and same_bits(plain[fill]["g_b"], ordered[fill]["g_b"])
