"""The per-ray render kernels (cnc_amd/csrc/volrend.hip, cnc_amd/csrc/scan.hip) at the sizes a training step and an
evaluation frame run, against the float64 twin (tests/render_twin.py), per entry:

    |got - ref64| <= K 2^-24 A + tiny

with A the entry's magnitude sum and K the number of float32 roundings on the longest path to it.  The counts are
derived in tests/render_twin.py from the structure of the kernels (tile tree, lane-strided per-ray sums, the two
roundings of sigma * (t1 - t0)) and doubled (ROUND); expf is allowed twice the 0.86 ulp measured on the device over
[0, 104] (`E_EXP`, `test_expf_figure`).  tests/test_render_twin.py shows on the CPU that a correct float32
implementation meets every one of these bounds on these layouts.

Layouts (render_twin.pair_counts / ragged_counts / training_counts): every length of 0, 1, 2, 31..33, 63..65, 255..257,
1023..1025, 4097 as the lower and as the upper ray of a wave next to a partner of length 0, 1 and greater; 1, 2, 7, 8,
9, 4095, 4096, 4097 rays; 2^18 samples over 6000 rays with a marched batch's long tail; 2^22 samples of the bench frame.
`starts` with gaps wherever a kernel takes both starts and counts.  Buffers handed to the C ABI start as NaN (0xFF for
masks, -1 for indices): an element a kernel should have written and did not fails, and so does one it wrote and should
not have.  All inputs are finite."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import render_twin as T
from test_render_twin import GRADS, LAYOUTS, scan_inputs

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
ACC, FIN = 1, 2                                    # CNC_VOLREND_ACCUMULATE, CNC_VOLREND_FINALIZE
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nlargest |got - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_RATIOS.items())))


def _within(group, got, ref, bound, what=""):
    got = np.asarray(got, f64)
    assert np.isfinite(got).all(), (group, what, "unwritten or non-finite entries")
    ratio = np.abs(got - ref) / bound
    r = float(ratio.max()) if ratio.size else 0.0
    _RATIOS[group] = max(_RATIOS.get(group, 0.0), r)
    assert r <= 1.0, (group, what, r, int(np.argmax(ratio)))


def _api():
    from cnc_amd import _lib as L
    return L.lib(), L.stream


class Dev:
    """A layout and its value buffers on the device."""

    def __init__(self, cuda, lay, v=None):
        self.cuda, self.lay, self.n = cuda, lay, max(lay.size, 1)
        self.starts, self.counts = self.t(lay.starts), self.t(lay.counts)
        if v is not None:
            self.t0, self.t1, self.sig, self.rgb, self.prefix = (self.buf(a) for a in (v.t0, v.t1, v.sig, v.rgb, v.prefix))
            self.op_in, self.bk = self.t(v.op_in), self.t(v.bk)

    def t(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), device=self.cuda)

    def buf(self, a):
        """A per-sample buffer (at least one element, so that it has an address)."""
        a = np.asarray(a)
        if a.shape[0] == 0:
            a = np.zeros((1,) + a.shape[1:], a.dtype)
        return self.t(a)

    def nan(self, *shape):
        return torch.full(shape or (self.n,), float("nan"), device=self.cuda)

    def live(self, buf):
        """The live view of a result buffer that started as NaN; what no ray addresses must still be NaN."""
        a = buf.cpu().numpy()
        rest = np.ones(a.shape[0], bool)
        rest[self.lay.at] = False
        assert np.isnan(a[rest]).all(), "an element between the rays was written"
        return a[self.lay.at]


def _p(t):
    """Device address of a tensor THE CALLER HOLDS: the address of a temporary is free again before the kernel runs."""
    return None if t is None else t.data_ptr()


def _forward(d, *, rgbs=True, opacity_in=None, prefix=False, bkgd=False, samples=True, flags=0, into=None):
    """cnc_volrend_forward on NaN buffers (or `into` = (colors, opacity, depth) when accumulating)."""
    lib, stream = _api()
    R = d.lay.R
    W, Tr, Al = (d.nan(), d.nan(), d.nan()) if samples else (None, None, None)
    col, op, dep = into if into is not None else (d.nan(R, 3) if rgbs else None, d.nan(R), d.nan(R))
    rc = lib.cnc_volrend_forward(_p(d.starts), _p(d.counts), _p(d.t0), _p(d.t1), _p(d.sig), _p(d.rgb) if rgbs else None,
                                 _p(opacity_in), _p(d.prefix) if prefix else None, _p(d.bk) if bkgd else None,
                                 _p(W), _p(Tr), _p(Al), _p(col), _p(op), _p(dep), R, flags, stream(d.cuda))
    torch.cuda.synchronize()
    return rc, NS(W=W, Tr=Tr, Al=Al, col=col, op=op, dep=dep)


# ------------------------------------------------------------------------------------------------------------------
# expf
# ------------------------------------------------------------------------------------------------------------------
def test_expf_figure(cuda):
    """expf of the device library alone, through cnc_ray_transmittance on one-sample rays (sigma = x, dt = 1: the
    kernel's sum is x exactly): within the figure render_twin.E_EXP is twice of, over the arguments the tests use."""
    from cnc_amd.backends import volrend_backend as K
    rng = np.random.default_rng(0)
    x = np.concatenate([np.linspace(0, 104, 2_000_001), 10 ** rng.uniform(-8, 2.02, 1_000_000),
                        rng.uniform(0, 20, 1_000_000)]).astype(f32)
    n = len(x)
    got = K.ray_transmittance(torch.arange(n, device=cuda), torch.ones(n, dtype=torch.int64, device=cuda),
                              torch.zeros(n, device=cuda), torch.ones(n, device=cuda),
                              torch.as_tensor(x, device=cuda)).cpu().numpy().astype(f64)
    ref = np.exp(-x.astype(f64))
    normal = ref >= T.TINY
    ulps = np.abs(got - ref)[normal] / np.spacing(ref[normal].astype(f32)).astype(f64)
    print(f"\nexpf: largest error {ulps.max():.4f} ulp over [0, 104]")
    assert ulps.max() <= T.EXPF_ULP_MEASURED
    assert np.abs(got - ref)[~normal].max() <= T.TINY


# ------------------------------------------------------------------------------------------------------------------
# volrend_forward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("prefix", ["neither", "opacity_in", "prefix_trans", "both"])
def test_forward_matrix(cuda, name, prefix):
    """{per-sample outputs wanted or not} x {rgbs or none} x {plain, FINALIZE, FINALIZE + background, ACCUMULATE}, and
    ACCUMULATE with opacity_in the very buffer it accumulates into."""
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    d = Dev(cuda, lay, v)
    oi, pt = prefix in ("opacity_in", "both"), prefix in ("prefix_trans", "both")
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in if oi else None, v.prefix if pt else None, v.bk)
    b = T.forward_bounds(f)
    f0 = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in if oi else None, v.prefix if pt else None)
    b0 = T.forward_bounds(f0)
    rng = np.random.default_rng(5)
    base = NS(col=rng.normal(size=(lay.R, 3)).astype(f32), op=rng.uniform(size=lay.R).astype(f32),
              dep=rng.normal(size=lay.R).astype(f32) * 10)
    for samples in (True, False):
        for rgbs in (True, False):
            for mode in ("plain", "finalize", "finalize_bkgd", "accumulate"):
                what = (samples, rgbs, mode)
                into = (d.t(base.col) if rgbs else None, d.t(base.op), d.t(base.dep)) if mode == "accumulate" else None
                rc, o = _forward(d, rgbs=rgbs, opacity_in=d.op_in if oi else None, prefix=pt, bkgd=mode == "finalize_bkgd",
                                 samples=samples, flags={"accumulate": ACC, "plain": 0}.get(mode, FIN), into=into)
                assert rc == 0, what
                if samples:
                    _within("fwd alpha", d.live(o.Al), f.alpha, b.eA, what)
                    _within("fwd trans", d.live(o.Tr), f.trans, b.eT, what)
                    _within("fwd weights", d.live(o.W), f.w, b.eW, what)
                op, dep = o.op.cpu().numpy(), o.dep.cpu().numpy()
                col = o.col.cpu().numpy() if rgbs else None
                if mode == "accumulate":
                    _within("fwd opacity", op, base.op + f.op, T.accumulate_bound(b.e_op, base.op, f.op), what)
                    _within("fwd depth", dep, base.dep + f.dsum, T.accumulate_bound(b.e_dsum, base.dep, f.A_dsum), what)
                    if rgbs:
                        _within("fwd colour", col, base.col + f.col, T.accumulate_bound(b.e_col, base.col, f.A_col), what)
                    continue
                _within("fwd opacity", op, f.op, b.e_op, what)
                assert np.all(op[lay.counts == 0] == 0)                  # rays without samples are written too
                if mode == "plain":
                    _within("fwd depth", dep, f.dsum, b.e_dsum, what)
                    if rgbs:
                        _within("fwd colour", col, f.col, b.e_col, what)
                else:
                    _within("fwd depth", dep, f.depth, b.e_depth, what)
                    if rgbs:
                        fc, bc = (f, b) if mode == "finalize_bkgd" else (f0, b0)
                        _within("fwd colour", col, fc.col_f, bc.e_col_f, what)
    if oi:                                         # the iterative render's call: opacity_in IS the accumulator
        acc = (d.t(base.col), d.t(v.op_in), d.t(base.dep))
        rc, o = _forward(d, opacity_in=acc[1], prefix=pt, flags=ACC, into=acc)
        assert rc == 0
        _within("fwd weights", d.live(o.W), f.w, b.eW, "aliased")
        _within("fwd opacity", o.op.cpu().numpy(), v.op_in + f.op, T.accumulate_bound(b.e_op, v.op_in, f.op), "aliased")
        _within("fwd colour", o.col.cpu().numpy(), base.col + f.col, T.accumulate_bound(b.e_col, base.col, f.A_col), "aliased")


def test_refusals_leave_the_buffers_alone(cuda):
    """ACCUMULATE | FINALIZE, colours without rgbs, a FINALIZE backward without opacity or depth, null required
    pointers: an error code, and not one element written."""
    lib, stream = _api()
    lay = LAYOUTS["rays9"]()
    v = T.make_values(lay, 3)
    d = Dev(cuda, lay, v)
    R = lay.R
    s = stream(cuda)
    outs = [d.nan(), d.nan(), d.nan(), d.nan(R, 3), d.nan(R), d.nan(R)]
    W, Tr, Al, col, op, dep = outs
    ok = [_p(d.starts), _p(d.counts), _p(d.t0), _p(d.t1), _p(d.sig), _p(d.rgb), None, None, None] + [_p(t) for t in outs]
    bad = [("both flags", ok, ACC | FIN), ("colours without rgbs", ok[:5] + [None] + ok[6:], 0)]
    bad += [(f"null argument {i}", ok[:i] + [None] + ok[i + 1:], 0) for i in range(5)]
    for what, args, flags in bad:
        assert lib.cnc_volrend_forward(*args, R, flags, s) != 0, what
    gs, grgb = d.nan(), d.nan(d.n, 3)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb)
    w, tr, al = (d.buf(lay.spread(getattr(f, k).astype(f32), 0)) for k in ("w", "trans", "alpha"))
    g = T.make_grads(lay, 4)
    go, gc = d.t(g.opacity), d.t(g.colors)
    op_, dep_ = d.t(f.op.astype(f32)), d.t(f.depth.astype(f32))
    okb = [_p(d.starts), _p(d.counts), _p(d.t0), _p(d.t1), _p(d.rgb), _p(w), _p(tr), _p(al), _p(op_), _p(dep_), None, _p(gc), _p(go), None, None, None, None, _p(gs), _p(grgb)]
    badb = [("finalize without opacity", okb[:8] + [None] + okb[9:], FIN), ("finalize without depth", okb[:9] + [None] + okb[10:], FIN),
            ("colour gradients without rgbs", okb[:4] + [None] + okb[5:], 0)]
    badb += [(f"null argument {i}", okb[:i] + [None] + okb[i + 1:], 0) for i in (0, 1, 2, 3, 5, 6, 7)]
    for what, args, flags in badb:
        assert lib.cnc_volrend_backward(*args, R, flags, s) != 0, what
    torch.cuda.synchronize()
    for t in outs + [gs, grgb]:
        assert bool(torch.isnan(t).all())
    assert lib.cnc_volrend_backward(*okb, R, 0, s) == 0 and lib.cnc_volrend_forward(*ok, R, 0, s) == 0     # the calls were sound
    torch.cuda.synchronize()
    assert not bool(torch.isnan(op).any()) and not bool(torch.isnan(gs[d.t(lay.at)]).any())


# ------------------------------------------------------------------------------------------------------------------
# rounds equal the whole
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pairs", "training"])
@pytest.mark.parametrize("rounds", [2, 3, 5])
def test_rounds_equal_the_whole(cuda, name, rounds):
    """Every ray split into `rounds` depth rounds, rendered with ACCUMULATE and opacity_in aliasing the accumulated
    opacity, against the twin of each round (given the float32 opacity the round started from) and against the ray
    rendered whole, kernel and twin.  The prefix of a round is 1 - opacity: a difference at the scale of 1, known to
    the accumulated opacity's ABSOLUTE bound E whatever is left of the ray, so against the whole ray a later round's
    weight is held to its own bound plus alpha exp(-before) E."""
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 41)
    d = Dev(cuda, lay, v)
    whole = T.forward(lay, v.t0, v.t1, v.sig, v.rgb)
    rc, ow = _forward(d)
    assert rc == 0
    R = lay.R
    acc = (torch.zeros(R, 3, device=cuda), torch.zeros(R, device=cuda), torch.zeros(R, device=cuda))
    W, Tr = d.nan(), d.nan()
    lib, stream = _api()
    E = np.zeros(R)                                # absolute bound of the accumulated opacity against the whole ray's
    e_col, e_dsum = np.zeros((R, 3)), np.zeros(R)
    w_whole_kernel = d.live(ow.W)
    for j in range(rounds):
        lo, hi = lay.counts * j // rounds, lay.counts * (j + 1) // rounds
        sub = T.Layout(lay.starts + lo, hi - lo, size=lay.size)
        op_before = acc[1].cpu().numpy()
        prev = [a.cpu().numpy().astype(f64) for a in acc]
        sub_starts, sub_counts = d.t(sub.starts), d.t(sub.counts)
        rc = lib.cnc_volrend_forward(_p(sub_starts), _p(sub_counts), _p(d.t0), _p(d.t1), _p(d.sig), _p(d.rgb),
                                     _p(acc[1]), None, None, _p(W), _p(Tr), None, _p(acc[0]), _p(acc[1]), _p(acc[2]), R, ACC,
                                     stream(cuda))
        torch.cuda.synchronize()
        assert rc == 0
        f = T.forward(sub, v.t0, v.t1, v.sig, v.rgb, opacity_in=op_before)
        b = T.forward_bounds(f)
        w, tr = W.cpu().numpy()[sub.at], Tr.cpu().numpy()[sub.at]
        _within("rounds, weights of a round", w, f.w, b.eW, j)
        _within("rounds, trans of a round", tr, f.trans, b.eT, j)
        _within("rounds, opacity of a round", acc[1].cpu().numpy(), prev[1] + f.op, T.accumulate_bound(b.e_op, prev[1], f.op), j)
        # against the whole ray
        at_whole = np.repeat(lay.first + lo, sub.counts) + sub.k
        extra = np.exp(-f.before) * (E + T.ROUND * T.U)[sub.ri]          # and the rounding of 1 - opacity
        e_w = b.eW + f.alpha * extra
        _within("rounds, weights against the whole ray", w, whole.w[at_whole], e_w, j)
        _within("rounds, trans against the whole ray", tr, whole.trans[at_whole], b.eT + extra, j)
        both = e_w + T.forward_bounds(whole).eW[at_whole]
        _within("rounds, kernel against kernel", w, w_whole_kernel[at_whole].astype(f64), both, j)
        more = sub.ray_sum(f.alpha * extra)
        E = E + b.e_op + more + T.ROUND * T.U * (np.abs(prev[1]) + f.op)
        e_col = e_col + b.e_col + sub.ray_sum((f.alpha * extra)[:, None] * np.abs(f.rgb)) + T.ROUND * T.U * (np.abs(prev[0]) + f.A_col)
        e_dsum = e_dsum + b.e_dsum + sub.ray_sum(f.alpha * extra * np.abs(f.tmid)) + T.ROUND * T.U * (np.abs(prev[2]) + f.A_dsum)
    assert not bool(torch.isnan(W[d.t(lay.at)]).any())                   # the rounds cover every sample
    _within("rounds, opacity against the whole ray", acc[1].cpu().numpy(), whole.op, E)
    _within("rounds, colour against the whole ray", acc[0].cpu().numpy(), whole.col, e_col)
    _within("rounds, depth against the whole ray", acc[2].cpu().numpy(), whole.dsum, e_dsum)


# ------------------------------------------------------------------------------------------------------------------
# volrend_backward
# ------------------------------------------------------------------------------------------------------------------
def _backward(d, f32in, g, which, *, rgbs=True, finalize=False, bkgd=False, want_rgbs=True):
    lib, stream = _api()
    gs = d.nan()
    grgb = d.nan(d.n, 3) if (want_rgbs and rgbs) else None
    has = lambda k: getattr(g, k) if k in which else None
    rc = lib.cnc_volrend_backward(
        _p(d.starts), _p(d.counts), _p(d.t0), _p(d.t1), _p(d.rgb) if rgbs else None, _p(f32in.w), _p(f32in.tr), _p(f32in.al),
        _p(f32in.op), _p(f32in.dep), _p(d.bk) if bkgd else None, _p(has("colors")), _p(has("opacity")), _p(has("depth")),
        _p(has("weights")), _p(has("trans")), _p(has("alphas")), _p(gs), _p(grgb), d.lay.R, FIN if finalize else 0,
        stream(d.cuda))
    torch.cuda.synchronize()
    return rc, gs, grgb


@pytest.mark.parametrize("name", ["pairs", "pairs_packed", "training", "rays1", "rays7", "rays8", "rays9", "rays4097"])
@pytest.mark.parametrize("prefix", [False, True])
def test_backward_matrix(cuda, name, prefix):
    """Each gradient input alone and all together, with and without FINALIZE, with and without background, rgbs none,
    want_grad_rgbs off, behind forwards that used opacity_in and prefix_trans; under FINALIZE with a depth gradient,
    rays whose opacity is below, at and above eps32.  The kernel is handed the twin's weights, transmittance, alphas,
    opacity and depth rounded to float32, so its bound holds one rounding for each of them."""
    lay = LAYOUTS[name]()
    v, gr = T.make_values(lay, 21), T.make_grads(lay, 22)
    d = Dev(cuda, lay, v)
    g = NS(**{k: d.buf(getattr(gr, k)) for k in GRADS})
    nonempty = np.flatnonzero(lay.counts > 0)
    for bkgd in (False, True):
        f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in if prefix else None, v.prefix if prefix else None,
                      v.bk if bkgd else None)
        op32, dep32 = f.op.astype(f32), f.depth.astype(f32)
        eps = f32(T.EPS32)
        for r, o in zip(nonempty[:3], (eps / f32(2), eps, eps * f32(2))):
            op32[r] = o
        e = T.rounded_inputs_bounds(f)
        fin = NS(w=d.buf(lay.spread(f.w.astype(f32), 1e30)), tr=d.buf(lay.spread(f.trans.astype(f32), 1e30)),
                 al=d.buf(lay.spread(f.alpha.astype(f32), 1e30)), op=d.t(op32), dep=d.t(dep32))
        for finalize in (False, True):
            if bkgd and not finalize:
                continue                           # the background enters the backward under FINALIZE only
            cases = [([k], True, True) for k in GRADS] + [(GRADS, True, True), (GRADS, True, False)]
            cases += [([k for k in GRADS if k != "colors"], False, False), (["depth"], False, False)]
            for which, rgbs, want_rgbs in cases:
                what = (which, rgbs, want_rgbs, finalize, bkgd)
                rc, gs, grgb = _backward(d, fin, g, which, rgbs=rgbs, finalize=finalize, bkgd=bkgd, want_rgbs=want_rgbs)
                assert rc == 0, what
                kw = {"grad_" + k: getattr(gr, k) for k in which}
                fr = f if rgbs else NS(**{**f.__dict__, "rgb": None})
                b = T.backward(fr, finalize=finalize, opacity=op32, depth=dep32, **kw)
                eb = T.backward_bounds(b, e)
                _within("bwd grad_sigmas", d.live(gs), b.g_sigmas, eb.e_sigmas, what)
                if grgb is not None and "colors" in which:
                    _within("bwd grad_rgbs", d.live(grgb), b.g_rgbs, eb.e_rgbs, what)
                elif grgb is not None:
                    assert np.all(d.live(grgb) == 0), what


# ------------------------------------------------------------------------------------------------------------------
# the autograd layer
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["ray_indices", "packed_info"])
def test_rendering_autograd_at_training_size(cuda, route):
    """nerfacc.rendering forward and backward (kernel behind kernel) on the training-size layout against the twin; the
    backward's bound carries the forward's.  Rays whose float64 opacity lies within its bound of eps32 may take the
    other branch of the clamp and are left out of the gradient comparison (alpha is known to ~2^-24 absolutely, so an
    opacity of that order is not known at all)."""
    import cnc_amd.nerfacc as n
    gaps = route == "packed_info"
    lay = T.make_layout(T.training_counts(), gaps, 9)
    v, gr = T.make_values(lay, 51), T.make_grads(lay, 52)
    d = Dev(cuda, lay, v)
    sg, rg = d.sig.clone().requires_grad_(), d.rgb.clone().requires_grad_()
    ri = d.t(lay.spread(lay.ri, 0))
    kw = dict(packed_info=torch.stack([d.starts, d.counts], 1)) if gaps else {}
    col, op, dep, extras = n.rendering(d.t0, d.t1, ri, n_rays=lay.R, rgb_sigma_fn=lambda a, b, c: (rg, sg, None),
                                       render_bkgd=d.bk, **kw)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, render_bkgd=v.bk)
    fb = T.forward_bounds(f)
    _within("autograd colour", col.detach().cpu().numpy(), f.col_f, fb.e_col_f)
    _within("autograd opacity", op.detach().cpu().numpy()[:, 0], f.op, fb.e_op)
    _within("autograd depth", dep.detach().cpu().numpy()[:, 0], f.depth, fb.e_depth)
    at = d.t(lay.at)
    loss = (col * d.t(gr.colors)).sum() + (op * d.t(gr.opacity)).sum() + (dep * d.t(gr.depth)).sum() \
        + (extras["weights"][at] * d.t(gr.weights)[at]).sum()
    loss.backward()
    b = T.backward(f, gr.colors, gr.opacity, gr.depth, gr.weights, finalize=True)
    eb = T.backward_bounds(b, fb)
    sure = (np.abs(f.op - T.EPS32) > fb.e_op)[lay.ri]
    assert sure.mean() > 0.7
    _within("autograd grad_sigmas", sg.grad.cpu().numpy()[lay.at][sure], b.g_sigmas[sure], eb.e_sigmas[sure])
    _within("autograd grad_rgbs", rg.grad.cpu().numpy()[lay.at], b.g_rgbs, eb.e_rgbs)


def test_render_weight_from_density_autograd_at_training_size(cuda):
    """render_weight_from_density with prefix_trans, gradients through weights, trans and alphas at once."""
    import cnc_amd.nerfacc as n
    lay = T.make_layout(T.training_counts(), False)
    v, gr = T.make_values(lay, 61), T.make_grads(lay, 62)
    d = Dev(cuda, lay, v)
    sg = d.sig.clone().requires_grad_()
    w, tr, al = n.render_weight_from_density(d.t0, d.t1, sg, ray_indices=d.t(lay.ri), n_rays=lay.R, prefix_trans=d.prefix)
    f = T.forward(lay, v.t0, v.t1, v.sig, prefix_trans=v.prefix)
    fb = T.forward_bounds(f)
    _within("autograd weights", w.detach().cpu().numpy(), f.w, fb.eW)
    ((w * d.t(gr.weights)).sum() + (tr * d.t(gr.trans)).sum() + (al * d.t(gr.alphas)).sum()).backward()
    b = T.backward(f, grad_weights=gr.weights, grad_trans=gr.trans, grad_alphas=gr.alphas)
    _within("autograd grad_sigmas", sg.grad.cpu().numpy(), b.g_sigmas, T.backward_bounds(b, fb).e_sigmas)


def test_rendering_without_samples(cuda):
    import cnc_amd.nerfacc as n
    z = torch.zeros(0, device=cuda)
    bk = torch.tensor([0.2, 0.4, 0.9], device=cuda)
    col, op, dep, _ = n.rendering(z, z, torch.zeros(0, dtype=torch.int64, device=cuda), n_rays=5,
                                  rgb_sigma_fn=lambda a, b, c: None, render_bkgd=bk)
    assert torch.equal(col, bk.expand(5, 3)) and torch.equal(op, torch.zeros(5, 1, device=cuda))
    assert torch.equal(dep, torch.zeros(5, 1, device=cuda))


# ------------------------------------------------------------------------------------------------------------------
# visibility, compaction, windows, edges, per-ray transmittance, pack_bounds
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("from_alpha", [False, True])
def test_visibility_and_compaction(cuda, name, from_alpha):
    """Masks equal the twin's outside the samples whose float64 transmittance (alpha) lies within its bound of the
    threshold; those are at most 0.1 % of the case.  `kept` and the compaction are exact functions of the mask."""
    lib, stream = _api()
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    d = Dev(cuda, lay, v)
    f = T.forward(lay, v.t0, v.t1, v.sig)
    values = d.buf(lay.spread(f.alpha.astype(f32), 1e30)) if from_alpha else d.sig
    for eps in (1e-2, 1e-4):
        for thre, cap in ((0.0, None), (0.02, None), (0.02, 0.015), (0.01, 0.5)):
            mask = torch.full((d.n,), 255, dtype=torch.uint8, device=cuda)
            kept = torch.full((lay.R,), -1, dtype=torch.int64, device=cuda)
            cap_t = None if cap is None else torch.tensor([cap], device=cuda)
            rc = lib.cnc_render_visibility(_p(d.starts), _p(d.counts), _p(d.t0), _p(d.t1), _p(values), int(from_alpha), eps, thre,
                                           _p(cap_t), _p(mask), _p(kept), lay.R, stream(cuda))
            torch.cuda.synchronize()
            assert rc == 0
            m = mask.cpu().numpy()
            rest = np.ones(d.n, bool)
            rest[lay.at] = False
            assert np.all(m[rest] == 255) and np.all(m[lay.at] <= 1)
            got = m[lay.at].astype(bool)
            eff = thre if cap is None else float(min(f32(thre), f32(cap)))
            want, unsure = T.visibility_from_alpha(lay, lay.spread(f.alpha.astype(f32)), eps, eff) if from_alpha \
                else T.visibility_from_density(f, eps, eff)
            assert np.array_equal(got[~unsure], want[~unsure]), (eps, thre, cap)
            assert unsure.sum() <= 1e-3 * max(lay.S, 1000), (unsure.sum(), lay.S)
            assert np.array_equal(kept.cpu().numpy(), np.bincount(lay.ri[got], minlength=lay.R))
    # compaction by the last mask
    ri, a, b_, ns, k = T.compact(lay, got, v.t0, v.t1)
    total = int(k.sum())
    o_s, o_e = d.nan(max(total, 1)), d.nan(max(total, 1))
    o_r = torch.full((max(total, 1),), -1, dtype=torch.int64, device=cuda)
    ns_ = d.t(ns)
    rc = lib.cnc_compact_samples(_p(d.starts), _p(d.counts), _p(ns_), _p(mask), _p(d.t0), _p(d.t1), _p(o_s), _p(o_e), _p(o_r),
                                 lay.R, stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(o_r.cpu().numpy()[:total], ri) and np.array_equal(o_s.cpu().numpy()[:total], a)
    assert np.array_equal(o_e.cpu().numpy()[:total], b_)
    from cnc_amd.backends import volrend_backend as K
    r2, a2, b2, ns2, k2 = K.compact_samples(d.starts, d.counts, mask, kept, d.t0, d.t1)
    assert np.array_equal(r2.cpu().numpy(), ri) and np.array_equal(a2.cpu().numpy(), a) and np.array_equal(ns2.cpu().numpy(), ns)


@pytest.mark.parametrize("name", ["pairs", "rays9", "training"])
def test_window_samples_against_indexing(cuda, name):
    """cnc_ray_window_samples against plain indexing: windows of length 0, 1, 33, the whole ray, first > 0."""
    lib, stream = _api()
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    d = Dev(cuda, lay, v)
    rng = np.random.default_rng(3)
    kind = np.arange(lay.R) % 5
    n = lay.counts
    cnt = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0 * n, np.minimum(n, 1), np.minimum(n, 33), n], n // 2)
    first = np.where(kind == 3, 0, rng.integers(0, 1 << 30, size=lay.R) % (n - cnt + 1))
    assert (first > 0).any()
    win = T.Layout(lay.starts + first, cnt, size=lay.size)
    total = max(win.S, 1)
    o_s, o_e = d.nan(total), d.nan(total)
    o_r, o_i = (torch.full((total,), -1, dtype=torch.int64, device=cuda) for _ in range(2))
    first_, cnt_, out_ = d.t(first), d.t(cnt), d.t(win.first)
    assert first_.dtype == cnt_.dtype == out_.dtype == torch.int64 and bool((first_ + cnt_ <= d.counts).all())
    rc = lib.cnc_ray_window_samples(_p(d.starts), _p(first_), _p(cnt_), _p(out_), _p(d.t0), _p(d.t1), _p(o_s),
                                    _p(o_e), _p(o_r), _p(o_i), lay.R, stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    S = win.S
    assert np.array_equal(o_i.cpu().numpy()[:S], win.at) and np.array_equal(o_r.cpu().numpy()[:S], win.ri)
    assert np.array_equal(o_s.cpu().numpy()[:S], v.t0[win.at]) and np.array_equal(o_e.cpu().numpy()[:S], v.t1[win.at])
    from cnc_amd.backends import volrend_backend as K
    r2, a2, b2, i2 = K.window_samples(d.starts, first_, cnt_, d.t0, d.t1, S)
    assert np.array_equal(i2.cpu().numpy(), win.at) and np.array_equal(a2.cpu().numpy(), v.t0[win.at])


@pytest.mark.parametrize("over_allocated", [False, True])
def test_samples_from_hand_built_edges(cuda, over_allocated):
    """Edge lists written by hand: runs of touching samples (inner edges are both a right and a left edge), lone
    samples, edges that belong to no sample, rays without edges, rays longer than two tiles."""
    from cnc_amd.backends import volrend_backend as K
    rng = np.random.default_rng(8)
    rays = []
    for r in range(300):
        runs = [] if r % 7 == 0 else list(rng.integers(1, 40 if r % 5 else 90, size=rng.integers(1, 5)))
        t, vals, left, right = 0.5, [], [], []
        for run in runs:
            if rng.uniform() < 0.3:                                      # an edge of no sample
                vals.append(t), left.append(0), right.append(0)
                t += 0.25
            for k in range(run + 1):
                vals.append(t), left.append(int(k < run)), right.append(int(k > 0))
                t += 0.125
            t += 1.0
        rays.append((vals, left, right))
    n_edges = np.asarray([len(r[0]) for r in rays], i64)
    n_samples = np.asarray([sum(r[1]) for r in rays], i64)
    iv = T.make_layout(n_edges, over_allocated, 2)
    cat = lambda i, dt: iv.spread(np.asarray([x for r in rays for x in r[i]], dt), 1)      # gaps: stray left AND right edges
    vals, left, right = cat(0, f32), cat(1, np.uint8), cat(2, np.uint8)
    tt = lambda a: torch.as_tensor(a, device=cuda)
    spec = NS(chunk_starts=tt(np.cumsum(n_edges) - n_edges), chunk_cnts=tt(n_edges), vals=tt(vals), is_left=tt(left).bool(),
              is_right=tt(right).bool())
    if over_allocated:
        spec.alloc_starts = tt(iv.starts)
    for total in (None, int(n_samples.sum())):
        ri, a, b, starts = K.samples_from_intervals(spec, tt(n_samples), total)
        lv, ll, lr = iv.live(vals), iv.live(left).astype(bool), iv.live(right).astype(bool)
        assert np.array_equal(a.cpu().numpy(), lv[ll]) and np.array_equal(b.cpu().numpy(), lv[lr])
        assert np.array_equal(ri.cpu().numpy(), np.repeat(np.arange(300), n_samples))
        assert np.array_equal(starts.cpu().numpy(), np.cumsum(n_samples) - n_samples)
    assert n_edges.max() > 64 and (n_edges == 0).any() and np.all(b.cpu().numpy() > a.cpu().numpy())


@pytest.mark.parametrize("name", ["pairs", "training"])
def test_ray_transmittance_and_window_next(cuda, name):
    """cnc_ray_transmittance against the twin under its bound, and the front-to-back sampler's step
    (cnc_ray_window_next) against the decisions the twin's transmittance gives; a ray whose transmittance lies within
    the bound of the threshold may go either way and is left out from then on (at most 0.1 % of the rays + 1)."""
    from cnc_amd.backends import volrend_backend as K
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    d = Dev(cuda, lay, v)
    ref, e = T.ray_transmittance(lay, v.t0, v.t1, v.sig)
    _within("ray_transmittance", K.ray_transmittance(d.starts, d.counts, d.t0, d.t1, d.sig).cpu().numpy(), ref, e)
    thr = 1e-2 * (1 - 1e-3)
    done, take = torch.zeros_like(d.counts), torch.full_like(d.counts, -7)
    done_ref, alive = np.zeros(lay.R, i64), lay.counts > 0
    sure = np.ones(lay.R, bool)
    for i, w in enumerate((4, 100, 700, None)):
        K.ray_window_next(d.starts, d.counts, d.t0, d.t1, d.sig, done, take, w, thr, first=i == 0)
        left = lay.counts - done_ref
        take_ref = np.where(alive, left if w is None else np.minimum(left, w), 0)
        assert np.array_equal(done.cpu().numpy()[sure], done_ref[sure]) and np.array_equal(take.cpu().numpy()[sure], take_ref[sure]), i
        done_ref = done_ref + take_ref
        sub = T.Layout(lay.starts, done_ref, size=lay.size)
        tr, e = T.ray_transmittance(sub, v.t0, v.t1, v.sig)
        done_ = d.t(done_ref)
        _within("ray_transmittance", K.ray_transmittance(d.starts, done_, d.t0, d.t1, d.sig).cpu().numpy(), tr, e)
        sure &= np.abs(tr - float(f32(thr))) > e
        alive = (tr >= float(f32(thr))) & (done_ref < lay.counts)
    assert (~sure).sum() <= 1e-3 * lay.R + 1 and (take_ref > 0).any() and (~alive & (done_ref < lay.counts)).any()


def test_pack_bounds_beyond_the_last_ray(cuda):
    from cnc_amd.backends import volrend_backend as K
    lay = LAYOUTS["pairs_packed"]()
    starts, counts = K.pack_bounds(torch.as_tensor(lay.ri, device=cuda), lay.R + 5)
    assert np.array_equal(counts.cpu().numpy(), np.concatenate([lay.counts, np.zeros(5, i64)]))
    assert np.array_equal(starts.cpu().numpy(), np.concatenate([lay.starts, np.full(5, lay.S)]))


# ------------------------------------------------------------------------------------------------------------------
# scans
# ------------------------------------------------------------------------------------------------------------------
def _scan(d, fn, x, *more, tail=()):
    lib, stream = _api()
    out = d.nan()
    ins = [d.buf(d.lay.spread(a, 1e30)) for a in (x,) + more]           # (held until the kernel has run)
    rc = getattr(lib, fn)(_p(d.starts), _p(d.counts), *[_p(t) for t in ins], _p(out), d.lay.R, d.n, *tail, stream(d.cuda))
    torch.cuda.synchronize()
    assert rc == 0, fn
    return d.live(out)


@pytest.mark.parametrize("name", ["pairs", "training", "rays4097"])
def test_scans_bit_equal_and_within_the_twin(cuda, oracle, name):
    """Sums (inclusive / exclusive x forward / reverse x normalised or not) and products on the long layouts, starts
    with gaps: bit-equal to the oracle, within the derived bound of the twin; the product backward with inputs 0,
    1e-12, 1e-10 (its clamp) and 1."""
    lay = LAYOUTS[name]()
    d = Dev(cuda, lay)
    pos, signed, near1 = scan_inputs(lay, 31)
    for excl in (False, True):
        fn = "cnc_exclusive_sum" if excl else "cnc_inclusive_sum"
        for rev in (False, True):
            for norm in (False, True):
                for x in (pos,) if norm else (pos, signed):
                    got = _scan(d, fn, x, tail=(int(norm), int(rev)))
                    assert np.array_equal(got, oracle.segmented_scan(x, lay.first, lay.counts, excl, reverse=rev, normalize=norm))
                    ref, e = T.segmented_sum(x, lay, excl, rev, norm)
                    _within("scan sums", got, ref, e, (excl, rev, norm))
        kind = "exclusive" if excl else "inclusive"
        got = _scan(d, f"cnc_{kind}_prod_forward", near1)
        assert np.array_equal(got, oracle.segmented_scan(near1, lay.first, lay.counts, excl, prod=True))
        ref, e = T.segmented_prod(near1, lay, excl)
        _within("scan products", got, ref, e, excl)
        x = near1.copy()
        x[::5], x[1::5], x[2::5], x[3::5] = 0.0, 1e-12, 1e-10, 1.0
        out = oracle.segmented_scan(x, lay.first, lay.counts, excl, prod=True)
        got = _scan(d, f"cnc_{kind}_prod_backward", x, out, signed)
        assert np.array_equal(got, oracle.prod_backward(x, out, signed, lay.first, lay.counts, excl))
        ref, e = T.prod_backward(x, out, signed, lay, excl)
        _within("scan product backward", got, ref, e, excl)


def test_scans_without_edges(cuda):
    """n_edges == 0: success, nothing read, nothing written."""
    lib, stream = _api()
    lay = LAYOUTS["rays9"]()
    d = Dev(cuda, lay)
    out, x = d.nan(), d.nan()
    s = stream(cuda)
    a = (_p(d.starts), _p(d.counts), _p(x))
    assert lib.cnc_inclusive_sum(*a, _p(out), lay.R, 0, 0, 0, s) == 0 and lib.cnc_exclusive_sum(*a, _p(out), lay.R, 0, 1, 0, s) == 0
    assert lib.cnc_inclusive_prod_forward(*a, _p(out), lay.R, 0, s) == 0 and lib.cnc_exclusive_prod_forward(*a, _p(out), lay.R, 0, s) == 0
    assert lib.cnc_inclusive_prod_backward(*a, None, None, _p(out), lay.R, 0, s) == 0
    assert lib.cnc_exclusive_prod_backward(*a, None, None, _p(out), lay.R, 0, s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    from cnc_amd.backends import nerfacc_cuda as nc
    z = torch.zeros(0, device=cuda)
    assert nc.inclusive_sum(d.starts * 0, d.counts * 0, z, False, False).shape == (0,)
    assert nc.exclusive_prod_backward(d.starts * 0, d.counts * 0, z, z, z).shape == (0,)


# ------------------------------------------------------------------------------------------------------------------
# a slice of the bench frame
# ------------------------------------------------------------------------------------------------------------------
def test_bench_frame_slice(cuda):
    """2^22 samples of the bench's 800 x 800 frame as the marcher lays them out (rays from the middle of the image, up
    to about a thousand samples each): forward, finalised forward and the backward behind it, once."""
    import bench
    from cnc_amd.backends import nerfacc_cuda as C
    from cnc_amd.backends import volrend_backend as K
    w = bench.build_workload(cuda, 0)
    t_lo, t_hi, hit = C.ray_aabb_intersect(w["rays_o"], w["rays_d"], w["aabbs"], -float("inf"), float("inf"), float("inf"))
    ri, ts, te, starts, counts, _ = C.march_samples(w["rays_o"], w["rays_d"], None, w["binaries"], w["aabbs"],
                                                     torch.cat([t_lo, t_hi], -1), w["t_order"], hit, w["near"], w["far"],
                                                     bench.STEP_SIZE, 0.0)
    counts_np, starts_np = counts.cpu().numpy(), starts.cpu().numpy()
    r0 = len(counts_np) // 2
    r1 = r0 + int(np.searchsorted(np.cumsum(counts_np[r0:]), 1 << 22)) + 1
    a, z = int(starts_np[r0]), int(starts_np[r1 - 1] + counts_np[r1 - 1])
    lay = T.Layout(starts_np[r0:r1] - a, counts_np[r0:r1], size=z - a)
    print(f"\nframe slice: {lay.R} rays, {lay.S} samples, longest ray {lay.counts.max()}")
    assert lay.S >= 1 << 22 and lay.counts.max() > 64
    del ri
    rng = np.random.default_rng(71)
    scale = rng.choice([1.0, 3.0, 30.0, 80.0, 300.0], size=lay.R)
    v = NS(t0=ts[a:z].cpu().numpy(), t1=te[a:z].cpu().numpy(), sig=(rng.uniform(size=lay.size) ** 4 * scale[lay.ri]).astype(f32),
           rgb=rng.uniform(size=(lay.size, 3)).astype(f32), prefix=np.zeros(1, f32), op_in=np.zeros(1, f32),
           bk=np.asarray([0.2, 0.4, 0.9], f32))
    del ts, te
    torch.cuda.empty_cache()
    gr = T.make_grads(lay, 72)
    d = Dev(cuda, lay, v)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, render_bkgd=v.bk)
    fb = T.forward_bounds(f)
    rc, o = _forward(d, bkgd=True, flags=FIN)
    assert rc == 0
    _within("frame weights", d.live(o.W), f.w, fb.eW)
    _within("frame trans", d.live(o.Tr), f.trans, fb.eT)
    _within("frame colour", o.col.cpu().numpy(), f.col_f, fb.e_col_f)
    _within("frame depth", o.dep.cpu().numpy(), f.depth, fb.e_depth)
    g = NS(**{k: d.buf(getattr(gr, k)) for k in GRADS})
    rc, gs, grgb = _backward(d, NS(w=o.W, tr=o.Tr, al=o.Al, op=o.op, dep=o.dep), g, GRADS, finalize=True, bkgd=True)
    assert rc == 0
    b = T.backward(f, gr.colors, gr.opacity, gr.depth, gr.weights, gr.trans, gr.alphas, finalize=True)
    eb = T.backward_bounds(b, fb)
    sure = (np.abs(f.op - T.EPS32) > fb.e_op)[lay.ri]
    assert sure.mean() > 0.99
    _within("frame grad_sigmas", d.live(gs)[sure], b.g_sigmas[sure], eb.e_sigmas[sure])
    _within("frame grad_rgbs", d.live(grgb), b.g_rgbs, eb.e_rgbs)
