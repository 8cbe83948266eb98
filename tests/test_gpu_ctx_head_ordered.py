"""The ordered form of the context heads' backward (cnc_ctx_mlp_backward_ordered, cnc_amd/csrc/ctx_head.hip): the sums of
the plain entry in an order that depends on N, the shapes and the build only.  Through the C ABI on sentinel-guarded
buffers: against the float64 nn.Sequential with the bounds tests/test_gpu_ctx_head.py applies to the plain route (the same
terms are summed), grad_a / grad_b bit-equal to the plain entry, accumulation as documented (dst = fl(dst + s)), eight
repeats bit-identical under fresh allocations, two streams and a busy side stream, nothing written outside the stated
sizes; and through autograd: the route counters."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from guarded import Guarded

pytestmark = pytest.mark.gpu

# name -> (n_layers, Ca, Cb, F, window): the three-layer head 25 -> 32 -> 32 -> 8; single Linears with C = 9, 17, 33 at
# F = 8 and one at F = 2.  window = (lda, c0): in_a / grad_a are a column window of a wider matrix (pitched rows, the
# ContextHeads layout); None: packed.
HEADS = {"h3_c25": (3, 24, 0, 8, None), "l1_c9": (1, 8, 0, 8, (24, 8)), "l1_c17": (1, 8, 8, 8, None),
         "l1_c33": (1, 24, 8, 8, None), "l1_c17_f2": (1, 8, 8, 2, None)}
T = 4            # entries of the Pg table (the last one belongs to no row)


def _levels(N):
    """pg_index over three levels: one boundary inside a wave's rows, one on a wave boundary (64 rows of a wave of the
    single-Linear kernel, 16 of the three-layer one: both divide the second boundary, neither the first)."""
    b1, b2 = (6437, 12800) if N > 12800 else (30, 48 if N <= 64 else 64)
    r = torch.arange(N)
    return (r >= b1).long() + (r >= b2).long()


_CASES = {}


def _case(cuda, head, N, table):
    """Inputs on the device and the float64 gradients, computed once per (head, N, Pg form)."""
    key = (head, N, table)
    if key in _CASES:
        return _CASES[key]
    n_layers, Ca, Cb, F, window = HEADS[head]
    g = torch.Generator(device="cpu").manual_seed(N + 7 * Ca + F + int(table))
    C = Ca + Cb + 1
    if n_layers == 1:
        seq = nn.Sequential(nn.Linear(C, F))
    else:
        seq = nn.Sequential(nn.Linear(C, 32), nn.LeakyReLU(), nn.Linear(32, 32), nn.LeakyReLU(), nn.Linear(32, F))
    with torch.no_grad():
        for p in seq.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.4)
    lda, c0 = window if window else (Ca, 0)
    a_full = torch.randn(N, lda, generator=g)
    b = torch.randn(N, Cb, generator=g) if Cb else None
    pg = torch.rand(T if table else 1, generator=g)
    idx = _levels(N) if table else None
    go = torch.randn(N, F, generator=g)
    ref = seq.double()
    a64 = a_full[:, c0:c0 + Ca].double().requires_grad_()
    b64 = None if b is None else b.double().requires_grad_()
    pg64 = pg.double().requires_grad_()
    cols = [a64] + ([b64] if b is not None else []) + [pg64[idx][:, None] if table else pg64.reshape(1, 1).repeat(N, 1)]
    (ref(torch.cat(cols, dim=-1)) * go.double()).sum().backward()
    lin = [m for m in ref if isinstance(m, nn.Linear)]
    ws = []
    for m in lin:
        ws += [m.weight, m.bias]
    c = dict(n_layers=n_layers, Ca=Ca, Cb=Cb, F=F, lda=lda, c0=c0, N=N, table=table,
             a=a_full.to(cuda), b=None if b is None else b.to(cuda), pg=pg.to(cuda), idx=None if idx is None else idx.to(cuda),
             go=go.to(cuda), ws=[w.detach().float().to(cuda).contiguous() for w in ws] + [None] * (6 - len(ws)),
             ref_a=a64.grad, ref_b=None if b is None else b64.grad, ref_pg=pg64.grad, ref_w=[w.grad for w in ws])
    _CASES[key] = c
    return c


class _Out:
    """Guarded outputs (and scratch) of one call; `fill`: what the accumulated destinations hold before it."""

    def __init__(self, c, dev, fill=0.0, ws_bytes=0):
        N = c["N"]
        self.g_a = Guarded.empty((N, c["lda"]), np.float32, dev)
        self.g_b = Guarded.empty((N, c["Cb"]), np.float32, dev) if c["Cb"] else None
        self.g_pg = Guarded(np.full(c["pg"].numel(), fill, np.float32), dev)
        self.gw = [None if w is None else Guarded(np.full(tuple(w.shape), fill, np.float32), dev) for w in c["ws"]]
        self.ws = Guarded.empty((ws_bytes,), np.uint8, dev) if ws_bytes else None

    def all(self):
        return [x for x in [self.g_a, self.g_b, self.g_pg, self.ws] + self.gw if x is not None]

    def results(self):
        return [x.tensor().clone() for x in [self.g_a, self.g_b, self.g_pg] + self.gw if x is not None]


def _ws_bytes(c):
    from cnc_amd import _lib
    return int(_lib.lib().cnc_ctx_mlp_backward_ordered_workspace(c["N"], c["n_layers"], c["F"], c["Ca"] + c["Cb"] + 1,
                                                                T if c["table"] else 1))


def _run(c, dev, ordered, fill=0.0):
    from cnc_amd import _lib
    from cnc_amd._lib import ptr
    L = _lib.lib()
    o = _Out(c, dev, fill, _ws_bytes(c) if ordered else 0)
    head = (c["a"].data_ptr() + 4 * c["c0"], c["lda"], c["Ca"], ptr(c["b"]), c["Cb"], c["Cb"], c["pg"].data_ptr(), ptr(c["idx"]))
    tail = (*[ptr(w) for w in c["ws"]], c["go"].data_ptr(), o.g_a.ptr + 4 * c["c0"], None if o.g_b is None else o.g_b.ptr,
            o.g_pg.ptr, *[None if w is None else w.ptr for w in o.gw])
    if ordered:
        rc = L.cnc_ctx_mlp_backward_ordered(*head, T, c["N"], c["n_layers"], c["F"], *tail, c["lda"], c["Cb"], o.ws.ptr,
                                            o.ws.nbytes, _lib.stream(dev))
    else:
        rc = L.cnc_ctx_mlp_backward(*head, c["N"], c["n_layers"], c["F"], *tail, 1, 0, c["lda"], c["Cb"], _lib.stream(dev))
    _lib.check(rc, "ctx_mlp_backward")
    return o


@pytest.mark.parametrize("table", [False, True], ids=["scalar_pg", "pg_index"])
@pytest.mark.parametrize("N", [20011, 1, 64, 65])
@pytest.mark.parametrize("head", list(HEADS))
def test_ordered_backward_values_and_bounds(cuda, head, N, table):
    c = _case(cuda, head, N, table)
    o = _run(c, cuda, True)
    p = _run(c, cuda, False)
    torch.cuda.synchronize()
    for x in o.all() + p.all():
        assert x.intact()
    Ca, c0 = c["Ca"], c["c0"]
    ga = o.g_a.get()
    # the window's columns are written, nothing else of the pitched matrix is
    rest = np.delete(ga, np.s_[c0:c0 + Ca], axis=1).view(np.uint8)
    assert (rest == 0xA5).all()
    # per-row outputs: bit-equal to the plain entry
    assert np.array_equal(ga[:, c0:c0 + Ca].view(np.uint32), p.g_a.get()[:, c0:c0 + Ca].view(np.uint32))
    if c["Cb"]:
        assert np.array_equal(o.g_b.get().view(np.uint32), p.g_b.get().view(np.uint32))
    # against float64: the bounds of tests/test_gpu_ctx_head.py
    tol = dict(rtol=2e-5, atol=2e-5)
    assert torch.allclose(torch.from_numpy(ga[:, c0:c0 + Ca]).double(), c["ref_a"], **tol)
    if c["Cb"]:
        assert torch.allclose(torch.from_numpy(o.g_b.get()).double(), c["ref_b"], **tol)
    gpg = torch.from_numpy(o.g_pg.get()).double()
    if table:
        assert torch.allclose(gpg, c["ref_pg"], rtol=1e-4, atol=1e-3)
        assert float(gpg[T - 1]) == 0.0
    else:
        assert abs(float(gpg) - float(c["ref_pg"])) <= 1e-4 * max(1.0, abs(float(c["ref_pg"])))
    got_w = [w for w in o.gw if w is not None]
    assert len(got_w) == len(c["ref_w"])
    for w, q in zip(got_w, c["ref_w"]):
        scale = max(1.0, float(q.abs().max()))
        assert float((torch.from_numpy(w.get()).double() - q).abs().max()) <= 3e-5 * scale
    # accumulation: dst = fl(dst + s), s = the call's sum in its fixed order — one rounded add per element
    k = _run(c, cuda, True, fill=0.75)
    torch.cuda.synchronize()
    for zero, filled in zip([o.g_pg] + got_w, [k.g_pg] + [w for w in k.gw if w is not None]):
        want = (np.float32(0.75) + zero.get()).astype(np.float32)
        assert np.array_equal(want.view(np.uint32), filled.get().view(np.uint32))


@pytest.mark.parametrize("table", [False, True], ids=["scalar_pg", "pg_index"])
@pytest.mark.parametrize("N", [20011, 65])
@pytest.mark.parametrize("head", list(HEADS))
def test_ordered_backward_repeats_are_bit_identical(cuda, head, N, table):
    """Eight calls — fresh outputs and scratch each time, alternating between two streams, a side stream busy with large
    matmuls — give the same bits."""
    c = _case(cuda, head, N, table)
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    side = torch.cuda.Stream(cuda)
    m = torch.randn(2048, 2048, device=cuda)
    torch.cuda.synchronize()
    runs = []
    for rep in range(8):
        if rep >= 4:
            with torch.cuda.stream(side):
                for _ in range(6):
                    m @ m
        with torch.cuda.stream(streams[rep % 2]):
            runs.append(_run(c, cuda, True))
    torch.cuda.synchronize()
    first = runs[0].results()
    for r in runs:
        assert all(x.intact() for x in r.all())
        for x, y in zip(first, r.results()):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_route_counters_follow_the_mode(cuda):
    import cnc_amd
    from cnc_amd import _repro
    from cnc_amd.backends import context_backend as K
    torch.manual_seed(3)
    seq = nn.Sequential(nn.Linear(25, 32), nn.LeakyReLU(), nn.Linear(32, 32), nn.LeakyReLU(), nn.Linear(32, 8)).to(cuda)
    heads = [nn.Linear(17, 8).to(cuda) for _ in range(2)]
    a, b = torch.randn(3000, 24, device=cuda), torch.randn(3000, 8, device=cuda)
    pg = torch.rand(2, device=cuda)
    grads = {}
    for mode in (False, True):
        before = dict(_repro.ROUTE_CALLS)
        for p in list(seq.parameters()) + [q for h in heads for q in h.parameters()]:
            p.grad = None
        with cnc_amd.reproducible(mode):
            assert cnc_amd.reproducible_enabled() is mode
            ad, pgd = a.clone().requires_grad_(), pg.clone().requires_grad_()
            y = K.context_mlp(seq, ad, None, pgd[:1])
            z = K.context_heads(heads, ad, b, pgd, [(0, 1000, 0, 8, 0), (1000, 3000, 16, 8, 1)])
            (y.square().sum() + z.square().sum()).backward()
        calls = {k: _repro.ROUTE_CALLS[k] - before[k] for k in before}
        assert calls["ctx_ordered" if mode else "ctx_default"] == 3 and calls["ctx_default" if mode else "ctx_ordered"] == 0
        grads[mode] = [ad.grad, pgd.grad] + [p.grad for p in seq.parameters()] + [q.grad for h in heads for q in h.parameters()]
    assert torch.equal(grads[False][0], grads[True][0])               # the per-row gradient: no reduction in it
    for x, y in zip(grads[False][1:], grads[True][1:]):
        assert float((x - y).abs().max()) <= 3e-5 * max(1.0, float(x.abs().max()))
