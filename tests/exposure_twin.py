"""NumPy twin of csrc/exposure.hip: the arithmetic include/cnc_hip.h spells out for the exposure-compensation entry points,
restated operation by operation in float32 (`gains`, `forward`, `backward_rays`, `fold`, `centre`, and `backward` = the
last three), with the float64 definition beside it (`dtype=np.float64`: the same functions with sums in any order), and
the error bounds between the two, derived from the operation counts.

Bounds.  u = 2^-24, the unit round-off of float32; gamma(k) = k u / (1 - k u) bounds k roundings in a row.  A sequential
sum of m terms makes m - 1 roundings on its first term and fewer on the others, so its error is at most
gamma(m - 1) sum |terms|.

  gains       mean: gamma(C - 1) sum|e| / C <= gamma(C - 1) E with E = max |e|, one more rounding for the division, one for
              e - mean (|e - mean| <= 2 E): the effective log-gain is off by at most d = gamma(C + 3) E.  exp in double is
              exact to far below u, its rounding to float adds u:  |g32 - g64| <= g64 (expm1(d) + u (1 + expm1(d))).
  forward     (given equal gains) t = 1 - a, t b, c + t b, g (...): four roundings on the way to every term at most:
              |p32 - p64| <= gamma(4) M,  M = |g| (|c| + |t| |b|)   [whole pixel]   or   |g c| + |t b|   [foreground only]
  g_rgb       one rounding: u |g gp|
  g_opacity   g gp (whole pixel only), the product with b, two additions: gamma(4) sum_ch |u_ch b_ch|
  q           x: three roundings at most; g x; gp (...): gamma(5) |gp| |g| (|c| + |t| |b|)
  G_eff[k]    the rays of camera k in a chunk: at most 255 additions behind a term; the chunks: n_chunks - 1 more; the
              terms' own gamma(5):   gamma(255 + n_chunks + 5) sum_{r of k} |q_r|  =: B_k
  G[k]        mean of G_eff: its terms' B_j, gamma(C - 1) sum_j |G_eff_j| / C for the sum, one rounding for the division,
              one for the subtraction:   B_k + mean_j B_j + gamma(C + 1) (|G_eff_k| + mean_j |G_eff_j|)
"""
import numpy as np

CHUNK = 256
U = 2.0 ** -24
F32 = np.float32
CONSTANTS = (0.0, 0.25, -1.5)         # log-gains whose every multiple up to 2^20 is a float32 number


def gamma(k):
    return k * U / (1.0 - k * U)


def clamp_ids(ids, C):
    return np.clip(np.asarray(ids, np.int64), 0, C - 1)


def _ordered_column_sum(a):
    """s = 0; s = s + a[k] for k in order, per column, in a's dtype."""
    s = np.zeros(a.shape[1:], a.dtype)
    for row in a:
        s = s + row
    return s


def gains(e, dtype=F32):
    e = np.asarray(e, dtype)
    C = e.shape[0]
    if dtype == F32:
        mean = _ordered_column_sum(e) / F32(C)
        return np.exp((e - mean).astype(np.float64)).astype(F32)
    return np.exp(e - e.mean(axis=0))


def _behind(a, b, dtype):
    """t = 1 - a and the rounded product t b, [n, 3]."""
    t = (dtype(1.0) - np.asarray(a, dtype))[:, None]
    return t, t * np.asarray(b, dtype).reshape(-1, 3)


def forward(c, a, b, ids, g, gain_background=True, dtype=F32):
    """c [n, 3], a [n] | None, b [3] | [n, 3] | None, g [C, 3] -> p [n, 3]."""
    c, g = np.asarray(c, dtype), np.asarray(g, dtype)
    gr = g[clamp_ids(ids, g.shape[0])]
    if b is None:
        return gr * c
    _, tb = _behind(a, b, dtype)
    return gr * (c + tb) if gain_background else gr * c + tb


def backward_rays(gp, c, a, b, ids, g, gain_background=True, dtype=F32):
    """-> (g_rgb [n, 3], g_opacity [n] | None, q [n, 3])."""
    gp, c, g = np.asarray(gp, dtype), np.asarray(c, dtype), np.asarray(g, dtype)
    gr = g[clamp_ids(ids, g.shape[0])]
    gc = gr * gp
    if b is None:
        return gc, None, gp * (gr * c)
    bb = np.broadcast_to(np.asarray(b, dtype).reshape(-1, 3), c.shape)
    if gain_background:
        _, tb = _behind(a, b, dtype)
        x, u = c + tb, gc
    else:
        x, u = c, gp
    g_opacity = -((u[:, 0] * bb[:, 0] + u[:, 1] * bb[:, 1]) + u[:, 2] * bb[:, 2])
    return gc, g_opacity, gp * (gr * x)


def fold(q, ids, C, dtype=F32):
    """G_eff [C, 3]: chunks of 256 consecutive rays, a camera's rays in ray order from +0, the chunks in order from +0."""
    q = np.asarray(q, dtype)
    k = clamp_ids(ids, C)
    if dtype != F32:
        G = np.zeros((C, 3), dtype)
        np.add.at(G, k, q)
        return G
    n = q.shape[0]
    n_chunks = (n + CHUNK - 1) // CHUNK
    part = np.zeros((n_chunks, C, 3), F32)
    for j in range(min(CHUNK, n)):                 # the j-th ray of every chunk: one camera per chunk, so no collisions
        r = np.arange(j, n, CHUNK)
        ch = np.arange(r.shape[0])
        part[ch, k[r]] = part[ch, k[r]] + q[r]
    return _ordered_column_sum(part)


def centre(G_eff, dtype=F32):
    G_eff = np.asarray(G_eff, dtype)
    if dtype == F32:
        return G_eff - _ordered_column_sum(G_eff) / F32(G_eff.shape[0])
    return G_eff - G_eff.mean(axis=0)


def backward(gp, c, a, b, ids, g, gain_background=True, dtype=F32):
    """-> (g_rgb, g_opacity | None, G_eff, G)."""
    g_rgb, g_opacity, q = backward_rays(gp, c, a, b, ids, g, gain_background, dtype)
    G_eff = fold(q, ids, np.asarray(g).shape[0], dtype)
    return g_rgb, g_opacity, G_eff, centre(G_eff, dtype)


# ------------------------------------------------------------------------------------------------ the bounds (float64)
def gains_bound(e):
    e = np.asarray(e, np.float64)
    C = e.shape[0]
    d = gamma(C + 3) * np.abs(e).max(initial=0.0)
    return gains(e, np.float64) * (np.expm1(d) + U * (1.0 + np.expm1(d)))


def _magnitudes(c, a, b, ids, g):
    """|g|, |c| + |t| |b| per ray and channel."""
    c, g = np.abs(np.asarray(c, np.float64)), np.abs(np.asarray(g, np.float64))
    gr = g[clamp_ids(ids, g.shape[0])]
    if b is None:
        return gr, c, np.zeros_like(c)
    t, _ = _behind(a, b, np.float64)
    return gr, c, np.abs(t) * np.abs(np.asarray(b, np.float64).reshape(-1, 3))


def forward_bound(c, a, b, ids, g, gain_background=True):
    gr, cc, tb = _magnitudes(c, a, b, ids, g)
    return gamma(4) * (gr * (cc + tb) if gain_background else gr * cc + tb)


def ray_bounds(gp, c, a, b, ids, g, gain_background=True):
    """-> bounds of (g_rgb, g_opacity | None, q)."""
    gp = np.abs(np.asarray(gp, np.float64))
    gr, cc, tb = _magnitudes(c, a, b, ids, g)
    b_q = gamma(5) * gp * gr * (cc + (tb if gain_background else 0.0))
    if b is None:
        return U * gr * gp, None, b_q
    bb = np.abs(np.broadcast_to(np.asarray(b, np.float64).reshape(-1, 3), cc.shape))
    u = gr * gp if gain_background else gp
    return U * gr * gp, gamma(4) * (u * bb).sum(axis=1), b_q


def camera_bounds(gp, c, a, b, ids, g, gain_background=True):
    """-> bounds of (G_eff, G), [C, 3] each."""
    C = np.asarray(g).shape[0]
    _, _, q = backward_rays(gp, c, a, b, ids, g, gain_background, np.float64)
    n_chunks = (q.shape[0] + CHUNK - 1) // CHUNK
    B = gamma(255 + n_chunks + 5) * fold(np.abs(q), ids, C, np.float64)
    G_eff = np.abs(fold(q, ids, C, np.float64))
    return B, B + B.mean(axis=0) + gamma(C + 1) * (G_eff + G_eff.mean(axis=0))


def ulp_distance(a, b):
    """Distance in float32 steps between two float32 arrays of one sign (gains are positive)."""
    a, b = np.ascontiguousarray(a, F32).view(np.int32), np.ascontiguousarray(b, F32).view(np.int32)
    return np.abs(a.astype(np.int64) - b.astype(np.int64))


def cases(n, C, seed, ids="random"):
    """One set of inputs: (e [C, 3], c [n, 3], a [n], b3 [3], bn [n, 3], ids [n], gp [n, 3]) as float32 / int64."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-0.5, 0.5, (C, 3)).astype(F32)
    c = rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    a = rng.uniform(0.0, 1.0, n).astype(F32)
    a[rng.uniform(size=n) < 0.2] = 1.0
    b3 = rng.uniform(0.0, 1.0, 3).astype(F32)
    bn = rng.uniform(0.0, 1.0, (n, 3)).astype(F32)
    gp = rng.normal(0.0, 1.0, (n, 3)).astype(F32)
    if ids == "random":
        k = rng.integers(0, C, n)
    elif ids == "one":                              # all rays on one camera
        k = np.full(n, C // 2)
    elif ids == "per_chunk":                        # one image per chunk
        k = (np.arange(n) // CHUNK) % C
    elif ids == "sparse":                           # only every third camera receives rays
        k = (rng.integers(0, max(C // 3, 1), n) * 3) % C
    elif ids == "outside":                          # ids below 0 and at or above C
        k = rng.integers(-3, C + 3, n)
    else:
        raise ValueError(ids)
    return e, c, a, b3, bn, k.astype(np.int64), gp
