"""NumPy twin of depth supervision (cnc_amd/csrc/depth_loss.hip, cnc_amd/nerfacc/losses.py), one ray at
a time, and of the depth fetch:

  * `direct64`: the DEFINITION, e = m - D, L = (sum w e)^2 + spread sum w e^2 and dL/dw = 2 (sum w e) e + spread e^2,
    evaluated in float64 from the float32 inputs — the reference of every test;
  * `kernel32`: the kernels' arithmetic, every operation rounded to float32, in their summation order (a butterfly over each
    tile of 32, the tiles' sums added one after the other);
  * `prefix32`: what the kernels do NOT compute, sum w m - D sum w — kept to show what the offset case is for;
  * `bound(...)`: the absolute tolerances between `direct64` and the float32 forms, derived below from the summation order
    and NOT from what any implementation is observed to do;
  * `fetch64` / `fetch_bound`: the depth fetch's z -> t conversion and its tolerance.

The bound.  u = 2^-24.  Per sample, a_i = (|t0_i - D| + |t1_i - D|) / 2: this is |e_i| for every interval that does not
straddle the target and at most max(|e_i|, width_i / 2) for one that does.  A1 = sum w_i a_i, A2 = sum w_i a_i^2 (the
sums "sum w |e|" and "sum w e^2" with that reading of |e|), T = ceil(S / 32) tiles.
  e:   fl(t0 - D), fl(t1 - D) and their sum are three roundings of quantities of size <= 2 a_i: |e^ - e| <= 2 u a_i (the
       halving is exact).  w e one more: <= 3 u w a;  (w e) e: 3 + 2 + 1 = 6 u w a^2.
  sum: a product passes through the 5 additions of its tile's butterfly and at most T additions of the carry:
       (T + 5) u per term.  So |S1^ - S1| <= (T + 8) u A1 and |S2^ - S2| <= (T + 11) u A2 to first order; with
       gamma_n = n u / (1 - n u) <= (n + 1) u the higher orders are covered by b1 = (T + 9) u A1, b2 = (T + 12) u A2.
  L = fl(fl(S1 S1) + fl(spread S2)):   |L^ - L| <= 2 |S1| b1 + b1^2 + spread b2 + 2 u (S1^2 + spread S2)
       (b1^2 matters: where the expected depth is right, S1 is ~0 and the first-order term vanishes).
  g_i = fl(gl fl(fl(fl(2 S1) e) + fl(spread fl(e e)))):   the error of S1 enters as 2 a_i b1; e's own error and the four
       products and one sum add at most 5 u on 2 |S1| a_i and 8 u on spread a_i^2:
       |g^_i - g_i| <= |gl| (2 a_i b1 + 9 u (2 |S1| a_i + spread a_i^2)).
"""
import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24


def valid_target(D):
    return bool(np.isfinite(D) and D > 0)


def direct64(w, t0, t1, D, spread=1.0):
    """(loss, dloss/dw, S1, S2) of one ray from the definition, float64; no measurement or no samples: zeros."""
    w, t0, t1 = (np.asarray(x, f32).astype(f64) for x in (w, t0, t1))
    if not valid_target(D) or w.size == 0:
        return 0.0, np.zeros(w.size, f64), 0.0, 0.0
    e = 0.5 * (t0 + t1) - f64(f32(D))
    s1, s2 = float(np.sum(w * e)), float(np.sum(w * e * e))
    return s1 * s1 + spread * s2, 2.0 * s1 * e + spread * e * e, s1, s2


def _terms32(w, t0, t1, D):
    w, t0, t1, D = np.asarray(w, f32), np.asarray(t0, f32), np.asarray(t1, f32), f32(D)
    e = f32(0.5) * ((t0 - D) + (t1 - D))
    a = w * e
    return e, a, a * e


def _butterfly(v):
    """half_wave_sum over one tile of 32 float32 values: lane 0's result."""
    v = np.asarray(v, f32).copy()
    for d in (16, 8, 4, 2, 1):
        v = v + v[np.arange(32) ^ d]
    return v[0]


def _tiled_sum(x):
    total = f32(0.0)
    for lo in range(0, x.size, 32):
        tile = np.zeros(32, f32)
        tile[:min(32, x.size - lo)] = x[lo:lo + 32]
        total = total + _butterfly(tile)
    return total


def _finish32(e, s1, s2, spread, upstream):
    spread, up = f32(spread), f32(upstream)
    loss = s1 * s1 + spread * s2
    return loss, up * ((f32(2.0) * s1) * e + spread * (e * e)), s1


def kernel32(w, t0, t1, D, spread=1.0, upstream=1.0):
    """(loss, upstream * dloss/dw, S1) as the kernels compute them, float32."""
    n = np.asarray(w).size
    if not valid_target(D):
        return f32(0.0), np.zeros(n, f32), f32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        e, a, b = _terms32(w, t0, t1, D)
        return _finish32(e, _tiled_sum(a), _tiled_sum(b), spread, upstream)


def prefix32(w, t0, t1, D):
    """S1 in the prefix form sum w m - D sum w, serial float32 sums: two sums of the size of D subtracted."""
    w, t0, t1, D = np.asarray(w, f32), np.asarray(t0, f32), np.asarray(t1, f32), f32(D)
    m = f32(0.5) * (t0 + t1)
    M = W = f32(0.0)
    for i in range(w.size):
        M, W = M + w[i] * m[i], W + w[i]
    return M - D * W


def moments(w, t0, t1, D):
    """(a, A1, A2) of the module docstring, float64."""
    w, t0, t1 = (np.asarray(x, f32).astype(f64) for x in (w, t0, t1))
    D = f64(f32(D))
    a = 0.5 * (np.abs(t0 - D) + np.abs(t1 - D))
    return a, float(np.sum(np.abs(w) * a)), float(np.sum(np.abs(w) * a * a))


def bound(S, w, t0, t1, D, spread=1.0, upstream=1.0):
    """(tolerance of S1, tolerance of the loss, tolerance of every upstream * dloss/dw_i), absolute — see the module
    docstring.  A ray without a measurement or without samples: zeros, the results must be exact."""
    if not valid_target(D) or S == 0:
        return 0.0, 0.0, np.zeros(S, f64)
    T = (S + 31) // 32
    a, A1, A2 = moments(w, t0, t1, D)
    _, _, s1, s2 = direct64(w, t0, t1, D, spread)
    b1, b2 = (T + 9) * U * A1, (T + 12) * U * A2
    b_loss = 2.0 * abs(s1) * b1 + b1 * b1 + spread * b2 + 2.0 * U * (s1 * s1 + spread * s2)
    b_grad = abs(float(upstream)) * (2.0 * a * b1 + 9.0 * U * (2.0 * abs(s1) * a + spread * a * a))
    return b1, b_loss, b_grad


def ratio(got, want, tol):
    """Largest |got - want| / tol (0 where both the error and the tolerance are 0, inf where only the tolerance is)."""
    got, want, tol = (np.atleast_1d(np.asarray(x, f64)) for x in (got, want, tol))
    if got.size == 0:
        return 0.0
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return float(np.max(r))


def offset_case(seed, S=64):
    """A thin surface far from the origin: D ~ 4096, S samples of width 1e-3 within +-0.05 of it, w = u^2 / (1.3 sum u^2)."""
    rng = np.random.default_rng(seed)
    D = f32(4096.0 + rng.uniform(-0.25, 0.25))
    mid = np.sort(f64(D) + rng.uniform(-0.05, 0.05, S))
    t0, t1 = (mid - 0.5e-3).astype(f32), (mid + 0.5e-3).astype(f32)
    u = rng.uniform(0, 1, S) ** 2
    return (u / (1.3 * u.sum())).astype(f32), t0, t1, D


# ---------------------------------------------------------------------------------------------------- the depth fetch
def fetch64(planes, cams, opengl, euclidean, cam_ids, px, py, dirs):
    """(t, c, z) float64 of the depth fetch from its float32 inputs: t = 0 where there is no measurement."""
    z = np.asarray(planes, f32)[cam_ids, py, px].astype(f64)
    if euclidean:
        c = np.ones_like(z)
    else:
        col = np.asarray(cams, f32)[cam_ids][:, [6, 10, 14]].astype(f64)
        c = np.sum(np.asarray(dirs, f32).astype(f64) * col, axis=-1) * (-1.0 if opengl else 1.0)
    ok = np.isfinite(z) & (z > 0) & (c > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ok, z / c, 0.0)
    return t, c, z


def fetch_bound(cams, euclidean, cam_ids, dirs, t, c):
    """Tolerance of t = z / c in float32.  The dot product: three products and two additions, (d0 r0 + d1 r1) + d2 r2 —
    |c^ - c| <= 3 u sum_k |d_k r_k| = 3 u P (each product one rounding, passing through at most two additions; gamma_3 <= 4 u
    covers the higher orders: 4 u P).  The division: t^ = z / c^ (1 + delta), so |t^ - t| <= |t| (|c^ - c| / c + u) to first
    order = |t| (4 u P / c + u): it grows with 1 / c.  One more u P / c for the second order of a c^ close to 0.  Euclidean
    depth is copied: exact."""
    if euclidean:
        return np.zeros_like(t)
    col = np.asarray(cams, f32)[cam_ids][:, [6, 10, 14]].astype(f64)
    P = np.sum(np.abs(np.asarray(dirs, f32).astype(f64) * col), axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 0, np.abs(t) * (5.0 * U * P / c + U), 0.0)
