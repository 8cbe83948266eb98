"""tests/render_twin.py (the float64 twin of the per-ray render kernels and the bounds a float32 implementation is
held to) checked without a GPU: against float64 torch autograd of the reference's op chain, against the reference's own
functions (tests/golden/render.npz), and — the proof that the bounds of tests/test_gpu_render_matrix.py can be met —
the float32 CPU oracle under those very bounds on those very layouts."""
import os

import numpy as np
import pytest
import torch

import render_twin as T
from test_gpu_volrend import _chain64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32
_RATIOS = {}


def _note(group, err, bound):
    r = float((err / bound).max()) if err.size else 0.0
    _RATIOS[group] = max(_RATIOS.get(group, 0.0), r)
    return r


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nfloat32 oracle, largest |got - ref| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_RATIOS.items())))


def _within(group, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    r = _note(group, err, bound)
    assert r <= 1.0, (group, r, int(np.argmax(err / bound)))


LAYOUTS = {"pairs": lambda: T.make_layout(T.pair_counts(), True, 1),
           "pairs_packed": lambda: T.make_layout(T.pair_counts(), False),
           "training": lambda: T.make_layout(T.training_counts(), False),
           **{f"rays{n}": (lambda n=n: T.make_layout(T.ragged_counts(n, n), True, n)) for n in T.RAY_COUNTS}}


# ------------------------------------------------------------------------------------------------------------------
# (a) float64 autograd of the op chain
# ------------------------------------------------------------------------------------------------------------------
GRADS = ["colors", "opacity", "depth", "weights", "trans", "alphas"]


@pytest.mark.parametrize("finalize", [False, True])
@pytest.mark.parametrize("prefix", [False, True])
def test_twin_against_float64_autograd(prefix, finalize):
    lay = T.make_layout(np.concatenate([T.ragged_counts(290, 4), [300, 0, 1, 64, 65, 0, 2, 33, 700, 5]]), True, 3)
    v, gr = T.make_values(lay, 11), T.make_grads(lay, 12)
    pt = None
    if prefix:                                     # both prefixes at once; autograd sees their product
        pt = torch.tensor((1.0 - v.op_in.astype(np.float64))[lay.ri] * lay.live(v.prefix).astype(np.float64))
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in if prefix else None, v.prefix if prefix else None, v.bk)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    for which in [[g] for g in GRADS] + [GRADS]:
        s64 = t64(lay.live(v.sig)).requires_grad_()
        r64 = t64(lay.live(v.rgb)).requires_grad_()
        col, op, dep, w, tr, al = _chain64(t64(lay.live(v.t0)), t64(lay.live(v.t1)), s64, r64, lay.first, lay.counts,
                                           t64(v.bk), prefix=pt, finalize=finalize, expm1=True)
        per_ray = {"colors": col, "opacity": op, "depth": dep}
        per_sample = {"weights": w, "trans": tr, "alphas": al}
        loss = sum((per_ray[k] * t64(getattr(gr, k))).sum() for k in which if k in per_ray) \
            + sum((per_sample[k] * t64(lay.live(getattr(gr, k)))).sum() for k in which if k in per_sample)
        loss.backward()
        b = T.backward(f, finalize=finalize, **{"grad_" + k: getattr(gr, k) for k in which})
        # two float64 evaluations of the same sums.  torch differentiates expm1 as (result + 1): exp(-tau) to 2^-53
        # ABSOLUTELY, which the first term of the gradient inherits; autograd also underflows earlier
        tol = 1e-10 * b.A_sigmas + 2.0 ** -51 * b.A_own * np.abs(f.dt) + 1e-150
        assert np.all(np.abs(b.g_sigmas - s64.grad.numpy()) <= tol), which
        assert np.all(b.A_sigmas >= np.abs(b.g_sigmas) * (1 - 1e-12))
        if "colors" in which:
            assert np.allclose(b.g_rgbs, r64.grad.numpy(), rtol=1e-12, atol=1e-150)
    # forward values of the same chain
    ref = {"w": w, "trans": tr, "alpha": al, "op": op[:, 0], "col_f" if finalize else "col": col,
           "depth" if finalize else "dsum": dep[:, 0]}
    for k, r in ref.items():
        assert np.allclose(getattr(f, k), r.detach().numpy(), rtol=1e-11, atol=1e-150), k


# ------------------------------------------------------------------------------------------------------------------
# (b) the reference's own functions
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "prefix"])
def test_twin_against_reference_golden(case):
    """The tolerances are those tests/test_oracle_pins.py holds the oracle to on the same file (the reference's batched
    branch sums 45 terms with torch.cumsum in float32)."""
    g = np.load(os.path.join(GOLD, "render.npz"))
    R, M = g["sigmas"].shape
    lay = T.Layout(np.arange(R) * M, np.full(R, M))
    flat = lambda a: np.ascontiguousarray(a.reshape(R * M, *a.shape[2:]))
    f = T.forward(lay, flat(g["t_starts"]), flat(g["t_ends"]), flat(g["sigmas"]), flat(g["rgbs"]),
                  prefix_trans=flat(g["prefix"]) if case == "prefix" else None, render_bkgd=g["bkgd"])
    assert np.allclose(f.alpha, flat(g[f"{case}_alphas"]), rtol=2e-6, atol=2.5e-7)
    assert np.allclose(f.trans, flat(g[f"{case}_trans"]), rtol=3e-5, atol=1e-9)
    assert np.allclose(f.w, flat(g[f"{case}_weights"]), rtol=3e-5, atol=2.5e-7)
    assert np.allclose(f.col, g[f"{case}_colors"], rtol=1e-5, atol=1e-7)
    assert np.allclose(f.op, g[f"{case}_opacity"][:, 0], rtol=1e-5, atol=1e-7)
    assert np.allclose(f.dsum, g[f"{case}_depth_sum"][:, 0], rtol=1e-5, atol=1e-7)
    assert np.allclose(f.col_f, g[f"{case}_colors_bkgd"], rtol=1e-5, atol=1e-6)
    assert np.allclose(f.depth, g[f"{case}_depth"][:, 0], rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------------------------
# (c) a float32 implementation meets the bounds
# ------------------------------------------------------------------------------------------------------------------
def _ray_sums32(lay, terms):
    """Per-ray float32 sums in the kernels' order: lane j adds elements j, j + 32, ... one after the other, then five
    butterfly additions across the 32 lanes."""
    out = np.zeros(lay.R, f32)
    for rays, W in lay.groups():
        tiles = -(-W // 32)
        k = np.arange(tiles * 32)[None, :]
        on = k < lay.counts[rays][:, None]
        v = np.where(on, terms[np.where(on, lay.first[rays][:, None] + k, 0)], f32(0)).reshape(len(rays), tiles, 32)
        acc = np.zeros((len(rays), 32), f32)
        for t in range(tiles):
            acc = acc + v[:, t]
        for d in (16, 8, 4, 2, 1):
            acc = acc + acc[:, np.arange(32) ^ d]
        out[rays] = acc[:, 0]
    return out


def _forward32(oracle, lay, v, with_op_in, with_prefix):
    t0, t1, sig, rgb = (lay.live(a) for a in (v.t0, v.t1, v.sig, v.rgb))
    w, tr, al = oracle.render_weight_from_density(t0, t1, sig, lay.first, lay.counts)
    if with_op_in:
        tr = tr * (f32(1) - v.op_in)[lay.ri]
    if with_prefix:
        tr = tr * lay.live(v.prefix)
    w = tr * al
    mid = (t0 + t1) / f32(2)
    col = np.stack([_ray_sums32(lay, w * rgb[:, c]) for c in range(3)], 1)
    return w, tr, al, col, _ray_sums32(lay, w), _ray_sums32(lay, w * mid)


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("prefix", ["none", "opacity_in", "both"])
def test_float32_forward_meets_the_bounds(oracle, name, prefix):
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    oi, pt = prefix != "none", prefix == "both"
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in if oi else None, v.prefix if pt else None, v.bk)
    b = T.forward_bounds(f)
    w, tr, al, col, op, dsum = _forward32(oracle, lay, v, oi, pt)
    if lay.S > 10000:                                                   # underflow and saturation are inside the case
        assert tr.min() == 0 and al.max() == 1
    _within("alpha", al, f.alpha, b.eA)
    _within("trans", tr, f.trans, b.eT)
    _within("weights", w, f.w, b.eW)
    _within("opacity", op, f.op, b.e_op)
    _within("colour", col, f.col, b.e_col)
    _within("depth sum", dsum, f.dsum, b.e_dsum)
    eps = f32(T.EPS32)
    _within("depth", dsum / np.maximum(op, eps), f.depth, b.e_depth)
    _within("colour + bkgd", col + v.bk[None, :] * (f32(1) - op)[:, None], f.col_f, b.e_col_f)
    small = f.op[lay.counts > 0]
    assert lay.S < 10000 or ((small < T.EPS32).any() and (small > T.EPS32).any())


def _backward32(oracle, lay, v, gr, w, tr, al, op, dep, finalize, which):
    """The gradient formula operation by operation in float32, the suffix sum through the oracle's tile tree."""
    R, S = lay.R, lay.S
    has = lambda k: k in which
    gc = gr.colors if has("colors") else np.zeros((R, 3), f32)
    go = gr.opacity[:, 0] if has("opacity") else np.zeros(R, f32)
    gd = gr.depth[:, 0] if has("depth") else np.zeros(R, f32)
    if finalize:
        eps = f32(T.EPS32)
        go = go - (gc[:, 0] * v.bk[0] + gc[:, 1] * v.bk[1] + gc[:, 2] * v.bk[2])
        den = np.maximum(op, eps)
        go = np.where(op > eps, go - gd * dep / den, go)
        gd = gd / den
    t0, t1, rgb = lay.live(v.t0), lay.live(v.t1), lay.live(v.rgb)
    ri = lay.ri
    g = go[ri] + gd[ri] * ((t0 + t1) / f32(2))
    g = g + (gc[ri, 0] * rgb[:, 0] + gc[ri, 1] * rgb[:, 1] + gc[ri, 2] * rgb[:, 2])
    if has("weights"):
        g = g + lay.live(gr.weights)
    carry = g * w
    if has("trans"):
        carry = carry + lay.live(gr.trans) * tr
    after = oracle.segmented_scan(carry, lay.first, lay.counts, exclusive=True, reverse=True)
    own = g * tr
    if has("alphas"):
        own = own + lay.live(gr.alphas)
    return (own * (f32(1) - al) - after) * (t1 - t0), w[:, None] * gc[ri]


@pytest.mark.parametrize("name", ["pairs", "training", "rays9"])
@pytest.mark.parametrize("finalize", [False, True])
def test_float32_backward_meets_the_bounds(oracle, name, finalize):
    lay = LAYOUTS[name]()
    v, gr = T.make_values(lay, 21), T.make_grads(lay, 22)
    f = T.forward(lay, v.t0, v.t1, v.sig, v.rgb, v.op_in, v.prefix, v.bk)
    fb = T.forward_bounds(f)
    w, tr, al, col, op, dsum = _forward32(oracle, lay, v, True, True)
    dep = dsum / np.maximum(op, f32(T.EPS32))
    sure = np.abs(f.op - T.EPS32) > fb.e_op                       # rays whose clamp branch is the same in both precisions
    # (alpha is known to ~U absolutely, so a float32 opacity of the order of eps is not: such rays are left out here;
    # tests/test_gpu_render_matrix.py hands the backward kernel opacities below, at and above eps directly)
    assert sure.mean() > 0.8
    for which in [[g] for g in GRADS] + [GRADS]:
        b = T.backward(f, finalize=finalize, **{"grad_" + k: getattr(gr, k) for k in which})
        e = T.backward_bounds(b, fb)
        gs, grgb = _backward32(oracle, lay, v, gr, w, tr, al, op, dep, finalize, which)
        keep = sure[lay.ri]
        _within("grad_sigmas", gs[keep], b.g_sigmas[keep], e.e_sigmas[keep])
        if "colors" in which:
            _within("grad_rgbs", grgb, b.g_rgbs, e.e_rgbs)


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("alpha_thre", [0.0, 0.02])
def test_float32_visibility_within_the_ambiguous_set(oracle, name, alpha_thre):
    """Masks may differ from the twin only where the float64 value lies within the bound of a threshold, and that set
    is at most 0.1 % of the case's samples."""
    lay = LAYOUTS[name]()
    v = T.make_values(lay, 21)
    f = T.forward(lay, v.t0, v.t1, v.sig)
    w, tr, al = oracle.render_weight_from_density(lay.live(v.t0), lay.live(v.t1), lay.live(v.sig), lay.first, lay.counts)
    for eps in (1e-2, 1e-4):
        want, unsure = T.visibility_from_density(f, eps, alpha_thre)
        got = oracle.render_visibility(tr, al, eps, alpha_thre)
        assert np.array_equal(got[~unsure], want[~unsure])
        assert unsure.sum() <= 1e-3 * max(lay.S, 1000), (unsure.sum(), lay.S)
        tr_a = oracle.segmented_scan(f32(1) - al, lay.first, lay.counts, exclusive=True, prod=True)
        want, unsure = T.visibility_from_alpha(lay, lay.spread(al), eps, alpha_thre)
        got = oracle.render_visibility(tr_a, al, eps, alpha_thre)
        assert np.array_equal(got[~unsure], want[~unsure])
        assert unsure.sum() <= 1e-3 * max(lay.S, 1000), (unsure.sum(), lay.S)
        if lay.S > 1000:
            assert want.any() and not want.all()
    m = want
    ri, a, b_, ns, kept = T.compact(lay, m, v.t0, v.t1)
    assert kept.sum() == m.sum() == len(ri) and np.all(np.diff(ri) >= 0) and np.array_equal(ns, np.cumsum(kept) - kept)


def scan_inputs(lay, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.01, 1.0, size=lay.S) * 10.0 ** rng.uniform(-3, 3, size=lay.R)[lay.ri]
    return x.astype(f32), rng.normal(size=lay.S).astype(f32), rng.uniform(0.9, 1.1, size=lay.S).astype(f32)


@pytest.mark.parametrize("name", ["pairs", "training", "rays4097"])
def test_float32_scans_meet_the_bounds(oracle, name):
    lay = LAYOUTS[name]()
    pos, signed, near1 = scan_inputs(lay, 31)
    for excl in (False, True):
        for rev in (False, True):
            for norm in (False, True):
                for x in (pos,) if norm else (pos, signed):
                    got = oracle.segmented_scan(x, lay.first, lay.counts, excl, reverse=rev, normalize=norm)
                    ref, e = T.segmented_sum(x, lay, excl, rev, norm)
                    _within("sums", got, ref, e)
        got = oracle.segmented_scan(near1, lay.first, lay.counts, excl, prod=True)
        ref, e = T.segmented_prod(near1, lay, excl)
        _within("products", got, ref, e)
        x = near1.copy()
        x[::5], x[1::5], x[2::5] = 0.0, 1e-12, 1e-10               # at and below the backward's clamp
        x[3::5] = 1.0
        out = oracle.segmented_scan(x, lay.first, lay.counts, excl, prod=True)
        got = oracle.prod_backward(x, out, signed, lay.first, lay.counts, excl)
        ref, e = T.prod_backward(x, out, signed, lay, excl)
        assert np.isfinite(got).all()
        _within("product backward", got, ref, e)
