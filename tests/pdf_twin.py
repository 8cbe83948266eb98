"""NumPy twin of the proposal-sampling kernels (cnc_amd/csrc/pdf.hip; semantics in include/cnc_hip.h at
cnc_importance_sampling / cnc_searchsorted), written from that specification and vectorised over all outputs.

Arithmetic: float32 operation by operation.  `fmaf` rounds once: the float64 product of two float32 is exact, the
sum with c is rounded to odd in float64 (two-sum error, then the neighbour with an odd last bit when inexact), and
rounding that to float32 is the correctly rounded fused result (53 >= 24 + 2 bits), ties included.

Layouts are given in the flattened form: every ray's segment is (start, count) into a 1-D array; a batched row of
E edges is (r * E, E).
"""
from __future__ import annotations

import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
HALF = f32(0.5)


def fmaf(a, b, c):
    """a * b + c rounded once to float32."""
    a, b, c = (np.asarray(x, f32) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(f64) * b.astype(f64)
        cc = c.astype(f64)
        s = p + cc
        bb = s - p
        err = (p - (s - bb)) + (cc - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(i64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def upper_bound(data, lo, hi, u):
    """First index in [lo, hi) with data[index] > u, per element; `!(v > u)` sends NaN to the right."""
    lo, hi, u = np.broadcast_arrays(np.asarray(lo, i64), np.asarray(hi, i64), np.asarray(u))
    lo, hi = lo.copy(), hi.copy()
    data = np.asarray(data)
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = lo + ((hi - lo) >> 1)
        mv = data[np.where(act, mid, 0)]
        with np.errstate(invalid="ignore"):
            right = mv > u
        lo = np.where(act & ~right, mid + 1, lo)
        hi = np.where(act & right, mid, hi)


def importance_sampling(vals, cdfs, seg_starts, seg_cnts, n_per_ray, jitter=None):
    """Resample every ray.  vals / cdfs: 1-D float32; seg_starts / seg_cnts: the input segment of each ray;
    n_per_ray: the number of samples of each ray; jitter: None or float32 [n_rays].
    Returns a dict: samples (1-D, ray after ray), sample_starts, edges (1-D: n + 1 per ray with n > 0),
    edge_starts, edge_cnts, sample_rays, edge_rays, is_left, is_right."""
    vals, cdfs = np.asarray(vals, f32).reshape(-1), np.asarray(cdfs, f32).reshape(-1)
    seg_starts, seg_cnts = np.asarray(seg_starts, i64), np.asarray(seg_cnts, i64)
    n = np.asarray(n_per_ray, i64)
    n_rays = n.shape[0]
    ecnt = (n + 1) * (n > 0)
    s_start = np.cumsum(n) - n
    e_start = np.cumsum(ecnt) - ecnt
    S, E = int(n.sum()), int(ecnt.sum())
    ray = np.repeat(np.arange(n_rays, dtype=i64), n)
    sid = np.arange(S, dtype=i64) - s_start[ray]
    nr = n[ray]
    base, ne = seg_starts[ray], seg_cnts[ray]
    last = base + ne - 1
    ok = ne > 0
    sb, sl = np.where(ok, base, 0), np.where(ok, last, 0)
    with np.errstate(all="ignore"):
        u_floor, u_ceil = cdfs[sb] if cdfs.size else np.zeros(S, f32), cdfs[sl] if cdfs.size else np.zeros(S, f32)
        u_step = (u_ceil - u_floor) / nr.astype(f32)
        bias = np.full(S, HALF, f32) if jitter is None else np.asarray(jitter, f32)[ray]
        u = fmaf(sid.astype(f32) + bias, u_step, u_floor)
        p = upper_bound(cdfs, sb, np.where(ok, last, sb), u)
        p0 = np.clip(p - 1, sb, sl)
        p1 = np.clip(p, sb, sl)
        c0, c1 = cdfs[p0] if cdfs.size else u, cdfs[p1] if cdfs.size else u
        v0, v1 = vals[p0] if vals.size else u, vals[p1] if vals.size else u
        t = np.where(c1 - c0 < f32(1e-10), (v0 + v1) * HALF, fmaf(u - c0, (v1 - v0) / (c1 - c0), v0))
        t = np.where(ok, t, f32(np.nan)).astype(f32)

        edges = np.empty(E, f32)
        t_min = np.where(ok, vals[sb] if vals.size else 0, np.nan).astype(f32)
        t_max = np.where(ok, vals[sl] if vals.size else 0, np.nan).astype(f32)
        pos = e_start[ray] + sid
        prev = np.concatenate([[f32(0)], t[:-1]]).astype(f32) if S else t
        nxt = np.concatenate([t[1:], [f32(0)]]).astype(f32) if S else t
        first = sid == 0
        e_first = np.where(nr == 1, t_min, np.fmax(t - (nxt - t) * HALF, t_min))
        edges[pos] = np.where(first, e_first, (t + prev) * HALF)
        lastm = sid == nr - 1
        e_last = np.where(nr == 1, t_max, np.fmin(t + (t - prev) * HALF, t_max))
        edges[pos[lastm] + 1] = e_last[lastm]
        edges = np.where(np.repeat(seg_cnts > 0, ecnt), edges, f32(np.nan)).astype(f32)
    edge_rays = np.repeat(np.arange(n_rays, dtype=i64), ecnt)
    k = np.arange(E, dtype=i64) - e_start[edge_rays]
    return dict(samples=t, sample_starts=s_start, sample_rays=ray, edges=edges, edge_starts=e_start,
                edge_cnts=ecnt, edge_rays=edge_rays, is_left=k < ecnt[edge_rays] - 1, is_right=k > 0)


def importance_sampling_batched(vals, cdfs, seg_starts, seg_cnts, n, jitter=None):
    """Batched outputs of an int n: (samples [n_rays, n], edges [n_rays, n + 1]).  n == 0: the one edge of a
    ray is vals[start] (NaN for an empty segment)."""
    n_rays = len(seg_cnts)
    if n == 0:
        vals = np.asarray(vals, f32).reshape(-1)
        st, ct = np.asarray(seg_starts, i64), np.asarray(seg_cnts, i64)
        e = np.where(ct > 0, vals[np.where(ct > 0, st, 0)] if vals.size else 0, np.nan).astype(f32)
        return np.zeros((n_rays, 0), f32), e.reshape(n_rays, 1)
    r = importance_sampling(vals, cdfs, seg_starts, seg_cnts, np.full(n_rays, n, i64), jitter)
    return r["samples"].reshape(n_rays, n), r["edges"].reshape(n_rays, n + 1)


def searchsorted(key_vals, key_starts, key_cnts, q_vals, q_rays, local):
    """(ids_left, ids_right) of every query value q_vals[i] in the key segment of ray q_rays[i]; `local` subtracts
    the segment start (a batched query).  A ray outside [0, n_key_rays) gives -1 for both."""
    key_vals = np.asarray(key_vals, f32).reshape(-1)
    key_starts, key_cnts = np.asarray(key_starts, i64), np.asarray(key_cnts, i64)
    q_vals, q_rays = np.asarray(q_vals, f32).reshape(-1), np.asarray(q_rays, i64).reshape(-1)
    bad = (q_rays < 0) | (q_rays >= len(key_starts))
    rr = np.where(bad, 0, q_rays)
    base = key_starts[rr] if len(key_starts) else np.zeros_like(rr)
    last = base + (key_cnts[rr] if len(key_cnts) else 0) - 1
    p = upper_bound(key_vals, base, np.maximum(last, base), q_vals)
    left = np.maximum(np.minimum(p - 1, last), base)
    right = np.maximum(np.minimum(p, last), base)
    if local:
        left, right = left - base, right - base
    return np.where(bad, -1, left), np.where(bad, -1, right)


def query_rays_from_starts(chunk_starts, n_entries):
    """The reference's ray of a flattened query entry without ray_indices: the last chunk whose start is <= it."""
    return upper_bound(np.asarray(chunk_starts, i64), np.zeros(n_entries, i64),
                       np.full(n_entries, len(chunk_starts), i64), np.arange(n_entries, dtype=i64)) - 1
