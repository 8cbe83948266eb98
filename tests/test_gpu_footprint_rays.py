"""Footprint of the per-ray kernels (cnc_amd/csrc/volrend.hip, scan.hip, pdf.hip and the ray-window helpers): every
result depends on the samples the rays own alone.  The layouts are render_twin's `rays9` and `pairs` — starts that are not
the running sum of the counts, so there are holes before, between and behind the rays — and here the holes of every
per-sample input, and the bytes around every buffer (int64 starts / counts of exactly n_rays entries included), hold
0x00, 0xA5 and 0xFF in turn (tests/guarded.py).  The holes of every per-sample output must still hold the fill.

None of these kernels sums with atomics: what a ray owns of every output is the same bits under every fill, and is held
to the reference and bound of the family's own tests (tests/test_gpu_render_matrix.py: the float64 twin's derived bounds,
the CPU oracle bit for bit for the scans; tests/test_gpu_pdf.py: the twin bit for bit).

An outside read whose value is discarded is NOT caught here: this pins the value-level contract, not memory safety."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import pdf_twin as PT
import render_twin as T
from guarded import FILLS, Guarded, holds_fill, same_bits, under_fills
from test_gpu_pdf import BIG, _bits_equal, _rows
from test_gpu_render_matrix import FIN, Dev, _backward, _forward, _scan, _within
from test_render_twin import GRADS, LAYOUTS, scan_inputs

pytestmark = pytest.mark.gpu
f32, i64 = np.float32, np.int64
NAMES = ["rays9", "pairs"]


class GDev(Dev):
    """test_gpu_render_matrix.Dev with every buffer guarded, so that its helpers (`_forward`, `_backward`, `_scan`), which
    build their operands themselves, run on guarded buffers: inputs through `t` / `buf` (the holes of a per-sample
    buffer poisoned), outputs through `nan` / `out` (born holding the fill), `inout` for what a call updates in place.

    Every buffer is entered into `bufs`, the dict of the running `under_fills`, the moment it is made, and `under_fills`
    enforces what it enforces everywhere: the bytes around every buffer intact, every input byte-identical to what it
    held when it was entered.  What this class adds is `live`: the holes of a per-sample OUTPUT still hold the fill."""

    def __init__(self, cuda, lay, v, bufs):
        self.fill, self.bufs = bufs.fill, bufs
        self.holes = np.ones(max(lay.size, 1), bool)
        self.holes[lay.at] = False
        super().__init__(cuda, lay, v)

    def _keep(self, g, kind):
        self.bufs[f"{kind}{len(self.bufs)}"] = g
        return g.tensor()

    def t(self, a):
        return self._keep(Guarded(np.ascontiguousarray(a), self.cuda, fill=self.fill), "in")

    def inout(self, a):
        """A buffer the call reads and updates in place."""
        return self._keep(Guarded(np.ascontiguousarray(a), self.cuda, fill=self.fill).out(), "inout")

    def buf(self, a):
        a = np.ascontiguousarray(a).copy()
        if a.shape[0] == 0:
            a = np.zeros((1,) + a.shape[1:], a.dtype)
        if a.shape[0] == self.holes.shape[0]:
            a.reshape(a.shape[0], -1).view(np.uint8)[self.holes] = self.fill
        return self.t(a)

    def nan(self, *shape):
        return self.out(shape or (self.n,), f32)

    def out(self, shape, dtype):
        return self._keep(Guarded.empty(shape, dtype, self.cuda, fill=self.fill), "out")

    def live(self, buf):
        a = buf.cpu().numpy()
        assert holds_fill(a[self.holes[:a.shape[0]]], self.fill), "an element between the rays was written"
        return a[self.lay.at]


def _under_fills(cuda, lay, v, call):
    """`call(d)` -> {name: host array: what the rays own of an output} on a GDev, under every fill.  -> the results of
    the first fill, after checking that every fill gives the same bits.  (The buffers are compared through `call`'s
    results and not through `under_fills`' own: a per-sample output's holes hold the fill, which differs by design.)"""
    per_fill = {}

    def run(bufs):
        per_fill[bufs.fill] = call(GDev(cuda, lay, v, bufs))

    under_fills(lambda fill: {}, run)
    first = per_fill[FILLS[0]]
    for fill in FILLS[1:]:
        assert set(per_fill[fill]) == set(first)
        for k in first:
            assert same_bits(per_fill[fill][k], first[k]), f"'{k}' moves with the fill ({fill:#x})"
    return first


@pytest.mark.parametrize("name", NAMES)
def test_volrend_forward(cuda, name):
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in, v.prefix, v.bk)
    b = T.forward_bounds(f)

    def call(d):
        rc, o = _forward(d, opacity_in=d.op_in, prefix=True, bkgd=True, flags=FIN)
        assert rc == 0
        return dict(Al=d.live(o.Al), Tr=d.live(o.Tr), W=d.live(o.W), col=o.col.cpu().numpy(), op=o.op.cpu().numpy(),
                    dep=o.dep.cpu().numpy())

    r = _under_fills(cuda, lay, v, call)
    _within("fwd alpha", r["Al"], f.alpha, b.eA)
    _within("fwd trans", r["Tr"], f.trans, b.eT)
    _within("fwd weights", r["W"], f.w, b.eW)
    _within("fwd opacity", r["op"], f.op, b.e_op)
    _within("fwd depth", r["dep"], f.depth, b.e_depth)
    _within("fwd colour", r["col"], f.col_f, b.e_col_f)
    assert np.all(r["op"][lay.counts == 0] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_volrend_backward(cuda, name):
    """test_backward_matrix's case with every gradient input, FINALIZE and a background, behind a forward that used
    opacity_in and prefix_trans."""
    lay = LAYOUTS[name]()
    v, gr = T.make_values(lay, 21), T.make_grads(lay, 22)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in, v.prefix, v.bk)
    op32, dep32 = f.op.astype(f32), f.depth.astype(f32)
    eps = f32(T.EPS32)
    for r_, o in zip(np.flatnonzero(lay.counts > 0)[:3], (eps / f32(2), eps, eps * f32(2))):
        op32[r_] = o
    e = T.rounded_inputs_bounds(f)
    bt = T.backward(f, finalize=True, opacity=op32, depth=dep32, **{"grad_" + k: getattr(gr, k) for k in GRADS})
    eb = T.backward_bounds(bt, e)

    def call(d):
        g = NS(**{k: d.buf(getattr(gr, k)) for k in GRADS})
        fin = NS(w=d.buf(lay.spread(f.w.astype(f32), 1e30)), tr=d.buf(lay.spread(f.trans.astype(f32), 1e30)),
                 al=d.buf(lay.spread(f.alpha.astype(f32), 1e30)), op=d.t(op32), dep=d.t(dep32))
        rc, gs, grgb = _backward(d, fin, g, GRADS, finalize=True, bkgd=True)
        assert rc == 0
        return dict(gs=d.live(gs), grgb=d.live(grgb))

    r = _under_fills(cuda, lay, v, call)
    _within("bwd grad_sigmas", r["gs"], bt.g_sigmas, eb.e_sigmas)
    _within("bwd grad_rgbs", r["grgb"], bt.g_rgbs, eb.e_rgbs)


@pytest.mark.parametrize("from_alpha", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_visibility_and_compaction(cuda, name, from_alpha):
    from cnc_amd import _lib
    lib = _lib.lib()
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    f = T.forward(lay, v.t0, v.t1, v.sig)
    eps, thre, cap = 1e-2, 0.02, 0.015
    eff = float(min(f32(thre), f32(cap)))
    want, unsure = T.visibility_from_alpha(lay, lay.spread(f.alpha.astype(f32)), eps, eff) if from_alpha \
        else T.visibility_from_density(f, eps, eff)

    def call(d):
        values = d.buf(lay.spread(f.alpha.astype(f32), 1e30)) if from_alpha else d.sig
        mask, kept, cap_t = d.out((d.n,), np.uint8), d.out((lay.R,), i64), d.t(np.array([cap], f32))
        assert lib.cnc_render_visibility(d.starts.data_ptr(), d.counts.data_ptr(), d.t0.data_ptr(), d.t1.data_ptr(),
                                         values.data_ptr(), int(from_alpha), eps, thre, cap_t.data_ptr(), mask.data_ptr(),
                                         kept.data_ptr(), lay.R, _lib.stream(cuda)) == 0
        torch.cuda.synchronize()
        got = d.live(mask)
        ri, a, b_, ns, k = T.compact(lay, got.astype(bool), v.t0, v.t1)
        total = max(int(k.sum()), 1)
        o_s, o_e, o_r, ns_ = d.nan(total), d.nan(total), d.out((total,), i64), d.t(ns)
        assert lib.cnc_compact_samples(d.starts.data_ptr(), d.counts.data_ptr(), ns_.data_ptr(), mask.data_ptr(), d.t0.data_ptr(),
                                       d.t1.data_ptr(), o_s.data_ptr(), o_e.data_ptr(), o_r.data_ptr(), lay.R, _lib.stream(cuda)) == 0
        torch.cuda.synchronize()
        n = int(k.sum())
        assert np.array_equal(o_r.cpu().numpy()[:n], ri) and np.array_equal(o_s.cpu().numpy()[:n], a)
        assert np.array_equal(o_e.cpu().numpy()[:n], b_)
        return dict(mask=got, kept=kept.cpu().numpy())

    r = _under_fills(cuda, lay, v, call)
    got = r["mask"].astype(bool)
    assert np.all(r["mask"] <= 1) and np.array_equal(got[~unsure], want[~unsure])
    assert unsure.sum() <= 1e-3 * max(lay.S, 1000)
    assert np.array_equal(r["kept"], np.bincount(lay.ri[got], minlength=lay.R))


@pytest.mark.parametrize("name", NAMES)
def test_window_helpers(cuda, name):
    """cnc_ray_window_samples, cnc_ray_window_positions + cnc_scatter_counted, cnc_ray_transmittance, cnc_ray_window_next,
    cnc_pack_bounds: exact against plain indexing, the transmittance within the twin's bound."""
    from cnc_amd import _lib
    from cnc_amd.backends import nerfacc_cuda as C
    from cnc_amd.backends import volrend_backend as K
    lib = _lib.lib()
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    rng = np.random.default_rng(3)
    kind = np.arange(lay.R) % 5
    n = lay.counts
    cnt = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0 * n, np.minimum(n, 1), np.minimum(n, 33), n], n // 2)
    first = np.where(kind == 3, 0, rng.integers(0, 1 << 30, size=lay.R) % (n - cnt + 1))
    win = T.Layout(lay.starts + first, cnt, size=lay.size)
    S = win.S
    rays_o = rng.normal(size=(lay.R, 3)).astype(f32)
    rays_d = rng.normal(size=(lay.R, 3)).astype(f32)
    values = rng.uniform(size=S + 7).astype(f32)
    tr_ref, tr_e = T.ray_transmittance(lay, v.t0, v.t1, v.sig)
    packed = T.make_layout(lay.counts, False)

    def call(d):
        first_, cnt_, out_, ends_ = d.t(first), d.t(cnt), d.t(win.first), d.t(np.cumsum(cnt))
        o_s, o_e, o_r, o_i = d.nan(max(S, 1)), d.nan(max(S, 1)), d.out((max(S, 1),), i64), d.out((max(S, 1),), i64)
        assert lib.cnc_ray_window_samples(d.starts.data_ptr(), first_.data_ptr(), cnt_.data_ptr(), out_.data_ptr(), d.t0.data_ptr(),
                                          d.t1.data_ptr(), o_s.data_ptr(), o_e.data_ptr(), o_r.data_ptr(), o_i.data_ptr(), lay.R,
                                          _lib.stream(cuda)) == 0
        o_, d_ = d.t(rays_o), d.t(rays_d)
        pos, src = K.window_positions(d.starts, first_, cnt_, ends_, d.t0, d.t1, o_, d_, S + 7)
        want_pos, _ = C.sample_positions(o_, d_, o_r[:S], o_s[:S], o_e[:S], want_dirs=True)
        assert torch.equal(pos[:S], want_pos)
        scattered = d.nan()
        K.scatter_counted(scattered, torch.cat([src[:S], src.new_zeros(7)]), d.t(values), d.t(np.array([S], i64)))
        tr = K.ray_transmittance(d.starts, d.counts, d.t0, d.t1, d.sig)
        done, take = d.inout(np.zeros(lay.R, i64)), d.inout(np.full(lay.R, -7, i64))
        K.ray_window_next(d.starts, d.counts, d.t0, d.t1, d.sig, done, take, 4, 1e-2 * (1 - 1e-3), first=True)
        b_starts, b_counts = K.pack_bounds(d.t(packed.ri), lay.R + 5)
        torch.cuda.synchronize()
        sc = scattered.cpu().numpy()
        rest = np.ones(sc.shape[0], bool)
        rest[win.at] = False
        assert holds_fill(sc[rest], d.fill), "scatter_counted wrote where no source index points"
        return dict(o_i=o_i.cpu().numpy()[:S], o_r=o_r.cpu().numpy()[:S], o_s=o_s.cpu().numpy()[:S], o_e=o_e.cpu().numpy()[:S],
                    src=src.cpu().numpy()[:S], sc=sc[win.at], tr=tr.cpu().numpy(), done=done.cpu().numpy(), take=take.cpu().numpy(),
                    b_starts=b_starts.cpu().numpy(), b_counts=b_counts.cpu().numpy())

    r = _under_fills(cuda, lay, v, call)
    assert np.array_equal(r["o_i"], win.at) and np.array_equal(r["o_r"], win.ri) and np.array_equal(r["src"], win.at)
    assert np.array_equal(r["o_s"], v.t0[win.at]) and np.array_equal(r["o_e"], v.t1[win.at])
    assert np.array_equal(r["sc"], values[:S])
    _within("ray_transmittance", r["tr"], tr_ref, tr_e)
    assert np.array_equal(r["done"], np.zeros(lay.R, i64)) and np.array_equal(r["take"], np.minimum(lay.counts, 4))
    assert np.array_equal(r["b_counts"], np.concatenate([lay.counts, np.zeros(5, i64)]))
    assert np.array_equal(r["b_starts"], np.concatenate([packed.starts, np.full(5, lay.S)]))


@pytest.mark.parametrize("name", NAMES)
def test_scans(cuda, oracle, name):
    """cnc_{inclusive,exclusive}_sum (reverse, normalised) and cnc_{inclusive,exclusive}_prod_{forward,backward}: the
    oracle's bits."""
    lay = LAYOUTS[name]()
    pos, signed, near1 = scan_inputs(lay, 31)
    x = near1.copy()
    x[::5], x[1::5], x[2::5], x[3::5] = 0.0, 1e-12, 1e-10, 1.0
    want = {}
    for excl in (False, True):
        kind = "exclusive" if excl else "inclusive"
        want[f"{kind}_sum"] = oracle.segmented_scan(signed, lay.first, lay.counts, excl)
        want[f"{kind}_sum_rev_norm"] = oracle.segmented_scan(pos, lay.first, lay.counts, excl, reverse=True, normalize=True)
        want[f"{kind}_prod"] = oracle.segmented_scan(near1, lay.first, lay.counts, excl, prod=True)
        out = oracle.segmented_scan(x, lay.first, lay.counts, excl, prod=True)
        want[f"{kind}_prod_bwd"] = oracle.prod_backward(x, out, signed, lay.first, lay.counts, excl)
        want[f"_{kind}_out"] = out

    def call(d):
        r = {}
        for excl in (False, True):
            kind = "exclusive" if excl else "inclusive"
            r[f"{kind}_sum"] = _scan(d, f"cnc_{kind}_sum", signed, tail=(0, 0))
            r[f"{kind}_sum_rev_norm"] = _scan(d, f"cnc_{kind}_sum", pos, tail=(1, 1))
            r[f"{kind}_prod"] = _scan(d, f"cnc_{kind}_prod_forward", near1)
            r[f"{kind}_prod_bwd"] = _scan(d, f"cnc_{kind}_prod_backward", x, want[f"_{kind}_out"], signed)
        return r

    r = _under_fills(cuda, lay, None, call)
    for k, got in r.items():
        assert np.array_equal(got, want[k]), k
    ref, e = T.segmented_sum(signed, lay, False, False, False)
    _within("scan sums", r["inclusive_sum"], ref, e)


def _pdf_rows(ptr_of, vals, starts=None, cnts=None, ray_indices=None, is_left=None, is_right=None, n_rays=0, per_ray=-1, n=0):
    from cnc_amd import _lib
    p = lambda g: None if g is None else ptr_of(g)
    return _lib.PdfRows(_lib.RaySegments(p(vals), p(starts), p(cnts), p(ray_indices), p(is_left), p(is_right), None), n_rays, per_ray, n)


@pytest.mark.parametrize("E", [3, 65, BIG])
def test_importance_sampling_batched(cuda, E):
    from cnc_amd import _lib
    rng = np.random.default_rng(E)
    R, n = 9, 33
    vals, cdfs, starts, cnts = _rows(rng, [E] * R, nan_every=7)
    s, e = PT.importance_sampling_batched(vals, cdfs, starts, cnts, n)

    def build(fill):
        return {"vals": Guarded(vals, cuda, fill=fill), "cdfs": Guarded(cdfs, cuda, fill=fill),
                "s": Guarded.empty((R, n), f32, cuda, fill=fill), "e": Guarded.empty((R, n + 1), f32, cuda, fill=fill)}

    def run(b):
        ptr = lambda g: g.ptr
        seg = _pdf_rows(ptr, b["vals"], n_rays=R, per_ray=E, n=R * E)
        smp, itv = _pdf_rows(ptr, b["s"], n_rays=R, per_ray=n, n=R * n), _pdf_rows(ptr, b["e"], n_rays=R, per_ray=n + 1, n=R * (n + 1))
        _lib.check(_lib.lib().cnc_importance_sampling(ctypes.byref(seg), b["cdfs"].ptr, None, ctypes.byref(smp), ctypes.byref(itv),
                                                      _lib.stream(cuda)), "importance_sampling")

    res = under_fills(build, run)
    for fill in FILLS:            # (a NaN's payload is not specified: test_gpu_pdf.py's comparison, under every fill)
        assert _bits_equal(res[fill]["s"], s) and _bits_equal(res[fill]["e"], e), fill


def test_importance_sampling_packed_and_searchsorted(cuda):
    from cnc_amd import _lib
    from cnc_amd.nerfacc import RayIntervals, searchsorted
    rng = np.random.default_rng(11)
    R = 29
    counts = rng.choice([0, 1, 2, 65, BIG], R)
    vals, cdfs, starts, cnts = _rows(rng, counts)
    n = rng.choice([0, 1, 2, 65, 257], R).astype(i64)
    want = PT.importance_sampling(vals, cdfs, starts, cnts, n)
    S, Ee = len(want["samples"]), len(want["edges"])
    q = rng.uniform(-1, 11, (R, 7)).astype(f32)
    q[:, 0] = np.nan
    wl, wr = PT.searchsorted(vals, starts, cnts, q, np.repeat(np.arange(R), 7), local=True)

    def build(fill):
        G = lambda a: Guarded(np.ascontiguousarray(a), cuda, fill=fill)
        E = lambda shape, dt: Guarded.empty(shape, dt, cuda, fill=fill)
        return {"vals": G(vals), "cdfs": G(cdfs), "starts": G(starts), "cnts": G(cnts), "s_starts": G(want["sample_starts"]), "s_cnts": G(n),
                "e_starts": G(want["edge_starts"]), "e_cnts": G(want["edge_cnts"]), "q": G(q), "info": G(np.stack([starts, cnts], -1)),
                "sv": E((S,), f32), "sri": E((S,), i64), "ev": E((Ee,), f32), "eri": E((Ee,), i64), "el": E((Ee,), np.uint8),
                "er": E((Ee,), np.uint8), "left": E(q.shape, i64), "right": E(q.shape, i64)}

    def run(b):
        ptr = lambda g: g.ptr
        seg = _pdf_rows(ptr, b["vals"], b["starts"], b["cnts"], n_rays=R, n=len(vals))
        smp = _pdf_rows(ptr, b["sv"], b["s_starts"], b["s_cnts"], b["sri"], n_rays=R, n=S)
        itv = _pdf_rows(ptr, b["ev"], b["e_starts"], b["e_cnts"], b["eri"], b["el"], b["er"], n_rays=R, n=Ee)
        _lib.check(_lib.lib().cnc_importance_sampling(ctypes.byref(seg), b["cdfs"].ptr, None, ctypes.byref(smp), ctypes.byref(itv),
                                                      _lib.stream(cuda)), "importance_sampling")
        left, right = searchsorted(RayIntervals(vals=b["vals"].tensor(), packed_info=b["info"].tensor()), RayIntervals(vals=b["q"].tensor()))
        b["left"].tensor().copy_(left), b["right"].tensor().copy_(right)

    res = under_fills(build, run)
    for fill in FILLS:
        r = res[fill]
        assert _bits_equal(r["sv"], want["samples"]) and _bits_equal(r["ev"], want["edges"]), fill
        assert np.array_equal(r["sri"], want["sample_rays"]) and np.array_equal(r["eri"], want["edge_rays"])
        assert np.array_equal(r["el"].astype(bool), want["is_left"]) and np.array_equal(r["er"].astype(bool), want["is_right"])
        assert np.array_equal(r["left"].reshape(-1), wl) and np.array_equal(r["right"].reshape(-1), wr)
