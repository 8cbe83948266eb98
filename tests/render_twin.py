"""float64 NumPy twin of the per-ray render kernels (cnc_amd/csrc/volrend.hip, cnc_amd/csrc/scan.hip), written from
the formulas (the reference's op chain, nerfacc/volrend.py, and the gradient formula in the header comment of
`k_volrend_bwd`), vectorised over rays, and the error bounds a float32 implementation of them is held to.

Every ray is (start, count) into 1-D buffers; `starts` need not be the running sum of `counts`.  Per-sample results are
returned in LIVE order (ray by ray, the samples the layout addresses): `x[lay.at]` is the live view of a buffer `x`.

Next to every output stands its magnitude sum A: the same expression with every term replaced by its absolute value.
A float32 evaluation errs by (number of roundings on the longest path to the entry) * 2^-24 * A; the `*_bounds`
functions below count those roundings from the structure of the kernels (never from their output):

  K_sum(i) = 10 + ceil(i / 32)    running sum at element i of a ray: a 32-element tile tree has at most 5 up-sweep and
                                  5 down-sweep additions on the path to any element, and the total of every earlier
                                  tile enters element 0 of the next one with one addition;
  2                               the summands sigma * (t1 - t0): one difference, one product;
  5 + ceil(n / 32)                a per-ray sum of n terms: lane-strided partial sums, then 5 butterfly additions;
  E_EXP                           ulps of expf, measured on the MI355X (see E_EXP).

exp() turns the absolute error of its argument into a relative one, so transmittance is held RELATIVE to
expm1(K 2^-24 sum(tau)); alpha = 1 - exp(-tau) rounds at the scale of 1 and is held absolutely.  ROUND (2) multiplies
every count: a rounder, larger K than the bare worst case, as tests/test_gpu_context_matrix.py uses."""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np

f64, i64 = np.float64, np.int64
U = 2.0 ** -24                                   # unit roundoff of float32
EPS32 = float(np.finfo(np.float32).eps)          # the clamp of depth / opacity
TINY = float(np.finfo(np.float32).tiny)          # smallest normal float32: results below it may be flushed
# expf of the ROCm device library, measured alone on an MI355X against float64 (cnc_ray_transmittance on one-sample
# rays with sigma = x, dt = 1, so that the kernel's sum is x exactly): 12 M arguments, 6 M evenly spaced over
# [0, 104] and 6 M drawn log-uniformly over [1e-8, 104] and uniformly over [0, 1] and [0, 20] (the tests' optical
# depths; results down to the smallest normal float32): largest error 0.857 ulp of the float32 result (at x = 5.2854;
# subnormal results within 1.2e-7 of the smallest normal).  Twice the figure 0.86 is allowed;
# tests/test_gpu_render_matrix.py::test_expf_figure measures it again.
EXPF_ULP_MEASURED = 0.86
E_EXP = 2 * EXPF_ULP_MEASURED
ROUND = 2.0


def ksum(i):
    return 10.0 + np.ceil(np.asarray(i, f64) / 32.0)


def kray(n):
    return 5.0 + np.ceil(np.asarray(n, f64) / 32.0)


class Layout:
    """Rays as (start, count) into buffers of `size` elements."""

    def __init__(self, starts, counts, size=None):
        self.starts, self.counts = np.asarray(starts, i64), np.asarray(counts, i64)
        self.R = len(self.counts)
        self.S = int(self.counts.sum())
        self.size = int(size) if size is not None else int((self.starts + self.counts).max(initial=0))
        self.first = np.cumsum(self.counts) - self.counts          # start of the ray in live order
        self.ri = np.repeat(np.arange(self.R, dtype=i64), self.counts)
        self.k = np.arange(self.S, dtype=i64) - np.repeat(self.first, self.counts)     # index inside the ray
        self.n = np.repeat(self.counts, self.counts)
        self.at = np.repeat(self.starts, self.counts) + self.k      # position in the buffers
        self._groups = None

    def groups(self, budget=1 << 22):
        """Rays of similar length, to be scanned as rows of one padded 2-D array of at most `budget` elements."""
        if self._groups is None:
            order = np.argsort(self.counts, kind="stable")
            order = order[self.counts[order] > 0]
            width = self.counts[order]
            self._groups, i = [], 0
            while i < len(order):
                j = i + 1
                while j < len(order) and (j + 1 - i) * int(width[j]) <= budget:
                    j += 1
                self._groups.append((order[i:j], int(width[j - 1])))
                i = j
        return self._groups

    def live(self, buf):
        return None if buf is None else np.asarray(buf)[self.at]

    def spread(self, x, fill=np.nan):
        out = np.full((self.size,) + x.shape[1:], fill, x.dtype)
        out[self.at] = x
        return out

    def ray_sum(self, x):
        x = np.asarray(x, f64)
        if x.ndim == 1:
            return np.bincount(self.ri, weights=x, minlength=self.R)
        return np.stack([np.bincount(self.ri, weights=x[:, c], minlength=self.R) for c in range(x.shape[1])], 1)


def seg_scan(x, lay, exclusive=False, reverse=False, prod=False):
    """Running sum (product) of live-ordered `x` inside every ray, each ray on its own (no global running total whose
    rounding would leak from ray to ray); `reverse` runs from the ray's last element to its first."""
    x = np.asarray(x, f64)
    out = np.empty_like(x)
    ident = 1.0 if prod else 0.0
    for rays, W in lay.groups():
        n = lay.counts[rays][:, None]
        k = np.arange(W, dtype=i64)[None, :]
        on = k < n
        src = np.where(on, lay.first[rays][:, None] + (n - 1 - k if reverse else k), 0)
        v = np.where(on, x[src], ident)
        c = np.cumprod(v, 1) if prod else np.cumsum(v, 1)
        if exclusive:
            c = np.concatenate([np.full((len(rays), 1), ident), c[:, :-1]], 1)
        out[src[on]] = c[on]
    return out


# ------------------------------------------------------------------------------------------------------------------
# scans (scan.hip)
# ------------------------------------------------------------------------------------------------------------------
def _from_end(lay, reverse):
    return lay.n - 1 - lay.k if reverse else lay.k


def segmented_sum(x, lay, exclusive=False, reverse=False, normalize=False):
    """(sum, bound).  Normalised: divided by max(the ray's total, 1e-10)."""
    x = np.asarray(x, f64)
    s, A = seg_scan(x, lay, exclusive, reverse), seg_scan(np.abs(x), lay, exclusive, reverse)
    e = ROUND * ksum(_from_end(lay, reverse)) * U * A
    if normalize:
        tot, A_tot = lay.ray_sum(x)[lay.ri], lay.ray_sum(np.abs(x))[lay.ri]
        den = np.maximum(tot, 1e-10)
        e_tot = ROUND * ksum(lay.n - 1) * U * A_tot
        s, e = s / den, (e + np.abs(s) * e_tot / den + ROUND * U * np.abs(s)) / den
    return s, e + TINY


def segmented_prod(x, lay, exclusive=False):
    """(product, bound).  Every multiplication rounds the WHOLE product relatively, so element i carries one rounding
    per factor and per tile carry: K_prod(i) = i + ceil(i / 32) + 1."""
    p = seg_scan(x, lay, exclusive, prod=True)
    return p, ROUND * (lay.k + np.ceil(lay.k / 32.0) + 1) * U * np.abs(p) + TINY


def prod_backward(inputs, outputs, grad_outputs, lay, exclusive):
    """grad_inputs_k = (sum over the outputs that contain input k of grad_i * output_i) / max(input_k, 1e-10), with
    the `outputs` it is given (scan.cu:199-210).  (grad, bound)."""
    x, o, g = (np.asarray(a, f64) for a in (inputs, outputs, grad_outputs))
    s, A = seg_scan(g * o, lay, exclusive, reverse=True), seg_scan(np.abs(g * o), lay, exclusive, reverse=True)
    den = np.maximum(x, 1e-10)
    # one rounding per product grad * output, the running sum, the division
    return s / den, (ROUND * (ksum(lay.n - 1 - lay.k) + 1) * U * A + ROUND * U * np.abs(s)) / den + TINY


# ------------------------------------------------------------------------------------------------------------------
# volume rendering, forward
# ------------------------------------------------------------------------------------------------------------------
def forward(lay, t_starts, t_ends, sigmas, rgbs=None, opacity_in=None, prefix_trans=None, render_bkgd=None):
    """alpha, transmittance, weight per live sample; colour / opacity / depth sums per ray with their magnitude sums
    (A_*); the finalised forms depth = dsum / max(opacity, eps32), colour + bkgd (1 - opacity)."""
    t0, t1, sig = (lay.live(a).astype(f64) for a in (t_starts, t_ends, sigmas))
    f = NS(lay=lay, t0=t0, t1=t1, dt=t1 - t0, tmid=(t0 + t1) / 2.0)
    f.tau = sig * f.dt
    f.before = seg_scan(f.tau, lay, exclusive=True)
    f.alpha = -np.expm1(-f.tau)
    f.surv = np.exp(-f.tau)                        # 1 - alpha without the cancellation
    f.n_prefix = 0
    P = np.ones(lay.S)
    if opacity_in is not None:
        P = P * (1.0 - np.asarray(opacity_in, f64).reshape(-1))[lay.ri]
        f.n_prefix += 2                            # 1 - opacity_in, and the product
    if prefix_trans is not None:
        P = P * lay.live(prefix_trans).astype(f64)
        f.n_prefix += 1
    f.prefix = P
    f.trans = np.exp(-f.before) * P
    f.w = f.trans * f.alpha
    f.rgb = None if rgbs is None else lay.live(rgbs).astype(f64)
    f.op = lay.ray_sum(f.w)
    f.dsum, f.A_dsum = lay.ray_sum(f.w * f.tmid), lay.ray_sum(np.abs(f.w * f.tmid))
    f.den = np.maximum(f.op, EPS32)
    f.depth = f.dsum / f.den
    f.bk = None if render_bkgd is None else np.asarray(render_bkgd, f64).reshape(3)
    if f.rgb is not None:
        f.col, f.A_col = lay.ray_sum(f.w[:, None] * f.rgb), lay.ray_sum(np.abs(f.w[:, None] * f.rgb))
        f.col_f = f.col if f.bk is None else f.col + f.bk[None, :] * (1.0 - f.op)[:, None]
    return f


def forward_bounds(f):
    """Bounds of a float32 forward against `f`: eT, eA, eW per sample; e_op, e_dsum, e_col (plain sums), e_depth,
    e_col_f (finalised) per ray.

    tau32 = fl(sigma * fl(t1 - t0)) is off by 2 U relative, the running sum before element i by K_sum(i) U more, both
    relative to the sum itself (the terms are non-negative), so exp(-before) is off by expm1((K_sum + 2) U before)
    relative, plus E_EXP ulps (<= 2 E_EXP U), plus one rounding per prefix operation.
    alpha: e32 = expf(-tau32) is off by e (2 U tau) <= 0.74 U (x e^-x <= 1/e) plus E_EXP ulps of a number below 1
    (<= E_EXP U), then fl(1 - e32) rounds by U alpha.  weight = fl(T alpha)."""
    lay = f.lay
    b = forward_bounds_samples(f)
    b.eW = f.alpha * b.eT + f.trans * b.eA + ROUND * U * f.w + TINY
    kr = ROUND * kray(lay.counts) * U
    b.e_op = lay.ray_sum(b.eW) + kr * f.op + TINY
    # tmid = fl(fl(t0 + t1) / 2): one rounding (the halving is exact); one more for the product
    b.e_dsum = lay.ray_sum(b.eW * np.abs(f.tmid) + ROUND * 2 * U * np.abs(f.w * f.tmid)) + kr * f.A_dsum + TINY
    maybe_above = f.op > EPS32 - b.e_op                            # max(o, eps) is 1-Lipschitz in o
    b.e_depth = b.e_dsum / f.den + np.where(maybe_above, np.abs(f.dsum) * b.e_op / f.den ** 2, 0.0) \
        + ROUND * U * np.abs(f.depth) + TINY
    if f.rgb is not None:
        b.e_col = lay.ray_sum(b.eW[:, None] * np.abs(f.rgb) + ROUND * U * np.abs(f.w[:, None] * f.rgb)) \
            + kr[:, None] * f.A_col + TINY
        b.e_col_f = b.e_col
        if f.bk is not None:                                       # fl(1 - o), the product, the sum
            b.e_col_f = b.e_col + np.abs(f.bk)[None, :] * b.e_op[:, None] + ROUND * U * (
                3 * np.abs(f.bk)[None, :] * np.abs(1.0 - f.op)[:, None] + f.A_col)
    return b


def accumulate_bound(e_sum, base, A_sum):
    """out = fl(base + sum): the sum's own bound and one rounding of the result."""
    return e_sum + ROUND * U * (np.abs(base) + A_sum)


def rounded_inputs_bounds(f):
    """The bounds of per-sample / per-ray values that are the twin's own, rounded once to float32."""
    return NS(eW=U * f.w + TINY, eT=U * f.trans + TINY, eA=U * f.alpha + TINY, e_op=U * f.op + TINY,
              e_depth=U * np.abs(f.depth) + TINY)


# ------------------------------------------------------------------------------------------------------------------
# volume rendering, backward
# ------------------------------------------------------------------------------------------------------------------
def backward(f, grad_colors=None, grad_opacity=None, grad_depth=None, grad_weights=None, grad_trans=None,
             grad_alphas=None, finalize=False, opacity=None, depth=None):
    """dL/dsigma and dL/drgb in closed form.  With T_i = P_i exp(-sum_{j<i} tau_j), alpha_i = 1 - exp(-tau_i),
    w_i = T_i alpha_i and L a function of (w, T, alpha):  d alpha_k / d tau_k = exp(-tau_k),  d T_i / d tau_k = -T_i
    for i > k, nothing else depends on tau_k, so

        dL/dtau_k = (g_k T_k + gA_k) exp(-tau_k) - sum_{i>k} (g_i alpha_i + gT_i) T_i,     dL/dsigma_k = dt_k dL/dtau_k

    with g_i = dL/dw_i = grad_weights_i + gO + gD tmid_i + gC . rgb_i the total gradient of weight i.  Finalised
    outputs are depth = dsum / max(o, eps) and colour + bkgd (1 - o), which pull the per-ray gradients back to
    gO - gC . bkgd - [o > eps] gD depth / max(o, eps) and gD / max(o, eps).  `opacity` / `depth` replace the forward's
    own where a caller hands other values to the kernel."""
    lay = f.lay
    z = np.zeros(lay.R)
    go = z if grad_opacity is None else np.asarray(grad_opacity, f64).reshape(-1)
    gd = z if grad_depth is None else np.asarray(grad_depth, f64).reshape(-1)
    gc = None if grad_colors is None else np.asarray(grad_colors, f64).reshape(-1, 3)
    b = NS(f=f, finalize=finalize, gc=gc)
    b.A_go, b.A_gd = np.abs(go), np.abs(gd)
    if finalize:
        o = f.op if opacity is None else np.asarray(opacity, f64).reshape(-1)
        dep = f.depth if depth is None else np.asarray(depth, f64).reshape(-1)
        den = np.maximum(o, EPS32)
        b.o, b.dep, b.den, b.gd_in = o, dep, den, gd
        pull = np.where(o > EPS32, gd * dep / den, 0.0)
        go, b.A_go = go - pull, b.A_go + np.abs(pull)
        if gc is not None and f.bk is not None:
            go, b.A_go = go - gc @ f.bk, b.A_go + np.abs(gc) @ np.abs(f.bk)
        gd = gd / den
        b.A_gd = np.abs(gd)
    b.go, b.gd = go, gd
    g = go[lay.ri] + gd[lay.ri] * f.tmid
    A_g = b.A_go[lay.ri] + b.A_gd[lay.ri] * np.abs(f.tmid)
    if gc is not None and f.rgb is not None:
        g, A_g = g + (gc[lay.ri] * f.rgb).sum(1), A_g + (np.abs(gc[lay.ri]) * np.abs(f.rgb)).sum(1)
    if grad_weights is not None:
        gw = lay.live(grad_weights).astype(f64)
        g, A_g = g + gw, A_g + np.abs(gw)
    gT = np.zeros(lay.S) if grad_trans is None else lay.live(grad_trans).astype(f64)
    gA = np.zeros(lay.S) if grad_alphas is None else lay.live(grad_alphas).astype(f64)
    b.g, b.A_g, b.gT, b.gA = g, A_g, gT, gA
    b.carry, b.A_carry = (g * f.alpha + gT) * f.trans, (A_g * f.alpha + np.abs(gT)) * f.trans
    b.after = seg_scan(b.carry, lay, exclusive=True, reverse=True)
    b.A_after = seg_scan(b.A_carry, lay, exclusive=True, reverse=True)
    b.own, b.A_own = g * f.trans + gA, A_g * f.trans + np.abs(gA)
    b.g_sigmas = (b.own * f.surv - b.after) * f.dt
    b.A_sigmas = (b.A_own * f.surv + b.A_after) * np.abs(f.dt)
    b.g_rgbs = None if gc is None else f.w[:, None] * gc[lay.ri]
    return b


def backward_bounds(b, e):
    """Bounds (e_sigmas, e_rgbs) of a float32 backward that is handed weights, transmittance, alphas (and, finalised,
    opacity and depth) which are themselves off by e.eW, e.eT, e.eA (e.e_op, e.e_depth).  Counts, per entry:

      pull-back:  gO' has at most 8 operations (3 products and 2 additions for gC . bkgd, its subtraction; product,
                  quotient and subtraction for gD depth / den); gD' one quotient.  The handed opacity and depth enter
                  through gD (e_depth / den + |depth| e_op / den^2).
      g_i:        at most 10 (tmid: 1; gD tmid: 2; gC . rgb: 3 + 3; grad_weights: 1), on the magnitude sum A_g.
      carry_i:    g_i w_i + gT_i T_i: 3 roundings, plus |g| eW + |gT| eT from the handed values.
      after_k:    the running sum over the samples behind k: K_sum(n - 1 - k) on sum |carry|, plus their own errors.
      own_k:      g T + gA: 2 roundings, |g| eT.
      1 - alpha:  the kernel has the float32 alpha, not tau: fl(1 - alpha32) is off from exp(-tau) by eA ABSOLUTELY
                  (and U (1 - alpha) for its rounding) however small exp(-tau) is: behind an opaque sample the first
                  term of the gradient is known only to |own| eA dt.  This is the precision of the stored alpha, the
                  counterpart of alpha's own absolute bound.
      result:     the product with fl(1 - alpha), the subtraction, t1 - t0 and the product with it: 5 on A_sigmas."""
    f, lay = b.f, b.f.lay
    tm = np.abs(f.tmid)
    e_go, e_gd = ROUND * 8 * U * b.A_go, np.zeros(lay.R)
    if b.finalize:
        above = b.o > EPS32
        e_go = e_go + np.where(above, np.abs(b.gd_in) * (e.e_depth / b.den + np.abs(b.dep) * e.e_op / b.den ** 2), 0.0)
        e_gd = ROUND * U * b.A_gd + np.where(above, np.abs(b.gd_in) * e.e_op / b.den ** 2, 0.0)
    e_g = e_go[lay.ri] + e_gd[lay.ri] * tm + ROUND * 10 * U * b.A_g
    e_carry = e_g * f.w + np.abs(b.g) * e.eW + np.abs(b.gT) * e.eT + ROUND * 3 * U * b.A_carry
    e_after = seg_scan(e_carry, lay, exclusive=True, reverse=True) + ROUND * ksum(lay.n - 1 - lay.k) * U * b.A_after
    e_own = e_g * f.trans + np.abs(b.g) * e.eT + ROUND * 2 * U * b.A_own
    e_sig = np.abs(f.dt) * (e_own * f.surv + b.A_own * (e.eA + ROUND * U * f.surv) + e_after) + ROUND * 5 * U * b.A_sigmas
    e_rgb = None
    if b.g_rgbs is not None:
        agc = np.abs(b.gc[lay.ri])
        e_rgb = e.eW[:, None] * agc + ROUND * U * f.w[:, None] * agc + TINY
    return NS(e_sigmas=e_sig + TINY, e_rgbs=e_rgb)


# ------------------------------------------------------------------------------------------------------------------
# visibility, compaction, per-ray transmittance
# ------------------------------------------------------------------------------------------------------------------
def _mask(trans, eT, alpha, eA, early_stop_eps, alpha_thre):
    eps, thre = float(np.float32(early_stop_eps)), float(np.float32(alpha_thre))
    vis, unsure = trans >= eps, np.abs(trans - eps) <= eT
    if thre > 0:
        vis, unsure = vis & (alpha >= thre), unsure | (np.abs(alpha - thre) <= eA)
    return vis, unsure


def visibility_from_density(f, early_stop_eps, alpha_thre=0.0):
    """(mask, unsure): visible = T >= early_stop_eps (and alpha >= alpha_thre when that is positive), without prefix;
    `unsure` marks the samples whose float64 value lies within the forward bound of a threshold."""
    bare = NS(**{**f.__dict__, "trans": np.exp(-f.before), "n_prefix": 0})
    bare.w = bare.trans * f.alpha
    e = forward_bounds_samples(bare)
    return _mask(bare.trans, e.eT, f.alpha, e.eA, early_stop_eps, alpha_thre)


def forward_bounds_samples(f):
    lay = f.lay
    # (a transmittance that has underflowed to 0 keeps a bound of 0 + TINY: the argument is capped before expm1)
    relT = np.expm1(np.minimum(ROUND * (ksum(lay.k) + 2) * U * f.before, 60.0)) + ROUND * (2 * E_EXP + f.n_prefix) * U
    return NS(eT=f.trans * relT + TINY, eA=ROUND * ((1 + E_EXP) * U + U * f.alpha))


def visibility_from_alpha(lay, alphas, early_stop_eps, alpha_thre=0.0):
    """T = exclusive product of fl(1 - alpha): the k factors before element k each round once, and so does every
    multiplication (see `segmented_prod`).  The alphas are the input: compared exactly with the threshold."""
    a = lay.live(alphas).astype(f64)
    T = seg_scan(1.0 - a, lay, exclusive=True, prod=True)
    eT = ROUND * (2 * lay.k + np.ceil(lay.k / 32.0) + 1) * U * np.abs(T) + TINY
    return _mask(T, eT, a, np.zeros_like(a), early_stop_eps, alpha_thre)


def compact(lay, mask_live, t_starts, t_ends):
    """Stable compaction: (ray_indices, t_starts, t_ends, new_starts, kept)."""
    m = np.asarray(mask_live, bool)
    kept = np.bincount(lay.ri[m], minlength=lay.R).astype(i64)
    return lay.ri[m], lay.live(t_starts)[m], lay.live(t_ends)[m], np.cumsum(kept) - kept, kept


def ray_transmittance(lay, t_starts, t_ends, sigmas):
    """exp(-sum of sigma dt over the ray's samples) per ray, and its bound: a per-ray sum of n products."""
    tau = lay.live(sigmas).astype(f64) * (lay.live(t_ends).astype(f64) - lay.live(t_starts).astype(f64))
    s = lay.ray_sum(tau)
    T = np.exp(-s)
    return T, T * (np.expm1(np.minimum(ROUND * (kray(lay.counts) + 2) * U * s, 60.0)) + ROUND * 2 * E_EXP * U) + TINY


# ------------------------------------------------------------------------------------------------------------------
# the case matrix shared by tests/test_render_twin.py (float32 oracle) and tests/test_gpu_render_matrix.py (kernels)
# ------------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
RAY_COUNTS = [1, 2, 7, 8, 9, 4095, 4096, 4097]       # one block holds 8 rays, one wave 2


def pair_counts():
    """Every length once as the lower (even) and once as the upper (odd) ray of a 64-lane wave, next to a partner of
    length 0, of length 1 and of a greater length: 192 rays."""
    out = []
    for i, n in enumerate(LENGTHS):
        for partner in (0, 1, LENGTHS[i + 1] if i + 1 < len(LENGTHS) else 4129):
            out += [n, partner, partner, n]
    return np.asarray(out, i64)


def ragged_counts(n_rays, seed):
    """`n_rays` rays of mixed lengths; the last ray is long, so an odd count leaves a live lower half next to a dead
    upper half for several tiles."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 70, size=n_rays)
    c[rng.uniform(size=n_rays) < 0.2] = 0
    c[-1] = 77
    return c.astype(i64)


def training_counts(seed=5, total=1 << 18, n_rays=6000):
    """2^18 samples over 6000 rays with the long tail of a marched batch: a third of the rays miss the occupied cells,
    most cross a few dozen samples, a few cross several hundred."""
    rng = np.random.default_rng(seed)
    c = np.minimum(rng.lognormal(np.log(40.0), 1.0, size=n_rays), 1500.0)
    c[rng.uniform(size=n_rays) < 0.33] = 0
    c = np.floor(c * (total / c.sum())).astype(i64)
    c[np.argmax(c)] += total - int(c.sum())
    assert int(c.sum()) == total and c.min() >= 0
    return c


def make_layout(counts, gaps, seed=0):
    """`gaps`: starts that are not the running sum of counts (unused elements before, between and behind the rays)."""
    counts = np.asarray(counts, i64)
    starts = np.cumsum(counts) - counts
    if not gaps:
        return Layout(starts, counts)
    g = np.random.default_rng(seed).integers(0, 6, size=len(counts) + 1)
    starts = starts + np.cumsum(g[:-1])
    return Layout(starts, counts, size=int((starts + counts).max(initial=0) + g[-1] + 1))


def make_values(lay, seed):
    """Buffers (float32) for a layout.  dt in [1e-3, 2e-2] with 3 % exact zeros, t from 0.05 up to 1e3; sigma = u^4
    times a per-ray scale from 1e-5 (opacity around float32's eps) to 1e4 (alpha exactly 1, transmittance underflowing
    part-way down the ray), a tenth of them 0, runs of 40 zeros on every third ray, some exactly 1e4.  Elements no ray
    addresses hold large finite values that would wreck any sum that read them."""
    rng = np.random.default_rng(seed)
    S = lay.S
    dt = rng.uniform(1e-3, 2e-2, size=S)
    step = seg_scan(dt * rng.uniform(1.0, 2.0, size=S), lay)
    origin = rng.choice([0.05, 2.0, 2.0, 900.0], size=lay.R)
    t0 = (origin[lay.ri] + step).astype(np.float32)
    t1 = (t0 + dt.astype(np.float32)).astype(np.float32)
    t1 = np.where(rng.uniform(size=S) < 0.03, t0, t1)
    scale = rng.choice([1e-5, 3e-5, 1.0, 3.0, 30.0, 80.0, 300.0, 1e4], size=lay.R)
    sig = rng.uniform(size=S) ** 4 * scale[lay.ri]
    sig[rng.uniform(size=S) < 0.1] = 0
    sig[(lay.ri % 3 == 0) & ((lay.k // 40) % 5 == 3)] = 0
    sig[(scale[lay.ri] == 1e4) & (rng.uniform(size=S) < 0.05)] = 1e4
    v = NS(t0=lay.spread(t0, 0.0), t1=lay.spread(t1, 1e4), sig=lay.spread(sig.astype(np.float32), 1e30),
           rgb=lay.spread(rng.uniform(size=(S, 3)).astype(np.float32), 1e30))
    op_in = rng.uniform(0, 0.9, size=lay.R)
    op_in[::7], op_in[3::7], op_in[5::11] = 0.0, 1.0 - 2.0 ** -20, 1.0
    v.op_in = op_in.astype(np.float32)
    v.prefix = lay.spread(rng.uniform(size=S).astype(np.float32), 1e30)
    v.bk = np.asarray([0.2, 0.4, 0.9], np.float32)
    return v


def make_grads(lay, seed):
    """Incoming gradients whose size varies over six decades from ray to ray."""
    rng = np.random.default_rng(seed)
    s = 10.0 ** rng.uniform(-3, 3, size=lay.R)
    per = lambda: lay.spread((rng.normal(size=lay.S) * s[lay.ri]).astype(np.float32), 1e30)
    return NS(colors=(rng.normal(size=(lay.R, 3)) * s[:, None]).astype(np.float32),
              opacity=(rng.normal(size=(lay.R, 1)) * s[:, None]).astype(np.float32),
              depth=(rng.normal(size=(lay.R, 1)) * s[:, None]).astype(np.float32),
              weights=per(), trans=per(), alphas=per())
