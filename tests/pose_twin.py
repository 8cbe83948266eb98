"""NumPy twins of the pose-refinement kernels (cnc_amd/csrc/field_position_grad.hip, cnc_amd/csrc/pose.hip) — test
infrastructure, no GPU needed.

Position gradient (`position_grad`): float64 arithmetic on the cell index and the fraction the kernel forms — those two
come from the forward's own float32 operations (`cell_and_fraction`: p = x (R - 2), rounded; + 0.5, rounded; floor; p -
floor) — so that twin and kernel differentiate the SAME function and differ by the rounding of the sums alone.  Next to
each gradient entry the twin returns the entry's sum of |terms|, the scale of that rounding.  `forward64` is the function
itself (the first layer's input row contracted with (dX, dS)) at a displaced point, in float64 with the same cells and
base fractions: what the central differences of tests/test_pose_twin.py are taken of.

Pose kernels: `rodrigues`, `pose_apply`, `ray_pose_q`, `pose_fold`, `ray_pose_grad`, each in a float32 mode that restates
the kernels operation by operation (include/cnc_hip.h lists the order; NumPy's float32 array operations are the IEEE
single operations, and nothing fuses) and in a float64 mode with the same order.

A model is the dict of field_lattice.field_params: {"encoders": [(table, offsets, resolutions)] * 4 in the order
xyz | xy | xz | yz, "F", "freqs"}."""
from __future__ import annotations

import numpy as np

import np_twins as T

f32, f64 = np.float32, np.float64
PLANE_DIMS = ((0, 1, 2), (0, 1), (0, 2), (1, 2))
POSE_CHUNK = 256                     # kPoseChunk, csrc/pose.hip
SERIES_BELOW = 2.0 ** -24            # theta^2 under which the Rodrigues coefficients are their series
CAMERA_ROW = 24


# ---------------------------------------------------------------------------------------------------------------------
# position gradient
# ---------------------------------------------------------------------------------------------------------------------
def unit_position(pos_world, aabb):
    """(x_unit float32 [N, 3], strictly-inside flags): field_unit_position of csrc/field_common.hpp, bounded form."""
    aabb = np.asarray(aabb, f32)
    ext = (aabb[3:] - aabb[:3]).astype(f32)
    x = ((np.asarray(pos_world, f32) - aabb[:3]).astype(f32) / ext).astype(f32)
    return x, np.all((x > 0) & (x < 1), axis=1)


def cell_and_fraction(x, R):
    """Corners::setup's float32 operations: (cell int64 [N, D], fraction float32 [N, D])."""
    p = (np.asarray(x, f32) * f32(R - 2)).astype(f32)
    p = (p + f32(0.5)).astype(f32)
    fl = np.floor(p)
    return fl.astype(np.int64), (p - fl).astype(f32)


def _corners(cell, t, R, hs):
    """Per corner i of every point: rows [N, C], weights w [N, C] float64, validity [N, C] (no border-ring coordinate),
    and dw [N, C, D]: the derivative of w_i with respect to the fraction along each axis."""
    N, D = cell.shape
    C = 1 << D
    t = np.asarray(t, f64)
    rows, w, valid, dw = np.zeros((N, C), np.uint32), np.ones((N, C)), np.ones((N, C), bool), np.ones((N, C, D))
    for i in range(C):
        q = np.empty((N, D), np.uint32)
        for d in range(D):
            bit = (i >> d) & 1
            fac = t[:, d] if bit else 1.0 - t[:, d]
            w[:, i] *= fac
            for a in range(D):
                dw[:, i, a] *= (1.0 if bit else -1.0) if a == d else fac
            q[:, d] = np.minimum(cell[:, d] + bit, R - 1)
        valid[:, i] = ~np.any((q == 0) | (q == R - 1), axis=1)
        rows[:, i] = T.grid_index(q, hs, R)
    return rows, w, valid, dw


def _unit_terms(x, table, off, hs, R, g_cols, shift=None):
    """One (encoder, level) unit at float32 points x [N, D] with gradient columns g_cols [N, F] (float64):
    (value sum_c g_c y_c [N], gradient with respect to the unit's coordinates [N, D], its sum of |terms| [N, D]).
    `shift` [N, D] (unit-cube units, float64) displaces the points inside their cells: the fraction becomes
    t + shift (R - 2) with t the float32 fraction of the base point."""
    cell, t = cell_and_fraction(x, R)
    t = t.astype(f64)
    if shift is not None:
        t = t + np.asarray(shift, f64) * (R - 2)
    rows, w, valid, dw = _corners(cell, t, R, hs)
    signs = np.where(np.asarray(table)[off:off + hs] >= 0, 1.0, -1.0)
    e = signs[rows]                                                   # [N, C, F]
    wv = np.where(valid, w, 0.0)
    wn = wv.sum(axis=1)
    empty = wn == 0
    wn = np.where(empty, 1e-9, wn)
    y = np.einsum("nc,ncf->nf", wv, e) / wn[:, None]                  # [N, F]
    value = np.einsum("nf,nf->n", g_cols, y)
    # d y_c / d x_a = (R - 2) sum_V d_a w_i (e_ic - y_c) / wn
    dev = e - y[:, None, :]                                           # [N, C, F]
    term = (R - 2) * dw[:, :, :, None] * dev[:, :, None, :] * g_cols[:, None, None, :] / wn[:, None, None, None]
    term = np.where(valid[:, :, None, None] & ~empty[:, None, None, None], term, 0.0)        # [N, C, D, F]
    return value, term.sum(axis=(1, 3)), np.abs(term).sum(axis=(1, 3))


def _walk(model, x_unit, dX, dS, shift):
    """(value [N], gradient in unit-cube units [N, 3], sum of |terms| [N, 3]) of the row contracted with (dX, dS)."""
    x_unit = np.asarray(x_unit, f32)
    N, F = x_unit.shape[0], model["F"]
    dX = np.asarray(dX, f64)
    value, g, mag = np.zeros(N), np.zeros((N, 3)), np.zeros((N, 3))
    col = 0
    for (table, offs, res), dims in zip(model["encoders"], PLANE_DIMS):
        dims = list(dims)
        for l in range(len(res)):
            hs = int(offs[l + 1] - offs[l])
            v, gu, mu = _unit_terms(x_unit[:, dims], table, int(offs[l]), hs, int(res[l]), dX[:, col:col + F],
                                    None if shift is None else shift[:, dims])
            value += v
            g[:, dims] += gu
            mag[:, dims] += mu
            col += F
    assert col == dX.shape[1], "dX: one block of F columns per (encoder, level) unit"
    if dS is not None:
        dS = np.asarray(dS, f64)
        xs = x_unit.astype(f64) + (0.0 if shift is None else shift)
        value += np.einsum("na,na->n", dS[:, :3], xs)
        g += dS[:, :3]
        mag += np.abs(dS[:, :3])
        for k, fr in enumerate(np.asarray(model["freqs"], f32)):
            # the argument as the forward forms it: the float32 product x f (a displaced point adds shift f to it)
            arg = (x_unit * fr).astype(f32).astype(f64) + (0.0 if shift is None else shift * f64(fr))
            ds_sin, ds_cos = dS[:, 3 + 6 * k:6 + 6 * k], dS[:, 6 + 6 * k:9 + 6 * k]
            value += np.einsum("na,na->n", ds_sin, np.sin(arg)) + np.einsum("na,na->n", ds_cos, np.cos(arg))
            a, b = f64(fr) * np.cos(arg) * ds_sin, -f64(fr) * np.sin(arg) * ds_cos
            g += a + b
            mag += np.abs(a) + np.abs(b)
    return value, g, mag


def position_grad(model, aabb, pos_world, selector, dX, dS):
    """(g_x [N, 3] float64 in world units, the entries' sums of |terms|) — cnc_field_position_grad.  Rows whose selector
    is 0 or whose position is not strictly inside the box are zero."""
    x_unit, inside = unit_position(pos_world, aabb)
    live = inside & (np.asarray(selector) != 0)
    aabb = np.asarray(aabb, f32)
    ext = (aabb[3:] - aabb[:3]).astype(f32).astype(f64)
    N = x_unit.shape[0]
    g, mag = np.zeros((N, 3)), np.zeros((N, 3))
    if live.any():
        _, gl, ml = _walk(model, x_unit[live], np.asarray(dX)[live], None if dS is None else np.asarray(dS)[live], None)
        g[live], mag[live] = gl / ext, ml / ext
    return g, mag


def forward64(model, x_unit, dX, dS, shift):
    """sum_c dX_c feature_c + sum dS tail at x_unit + shift (unit-cube units), the cells and base fractions of x_unit."""
    return _walk(model, x_unit, dX, dS, np.asarray(shift, f64))[0]


def features64(model, x_unit):
    """The encoder columns [N, F units] in float64 from the float32 cell and fraction (no displacement): what
    `forward64` contracts, for comparison with the float32 encoder forward."""
    x_unit = np.asarray(x_unit, f32)
    N, F = x_unit.shape[0], model["F"]
    cols = []
    for (table, offs, res), dims in zip(model["encoders"], PLANE_DIMS):
        for l in range(len(res)):
            hs = int(offs[l + 1] - offs[l])
            for c in range(F):
                g = np.zeros((N, F))
                g[:, c] = 1.0
                cols.append(_unit_terms(x_unit[:, list(dims)], table, int(offs[l]), hs, int(res[l]), g)[0])
    return np.stack(cols, axis=1)


def face_distance(model, x_unit):
    """Per point, the smallest distance (in cell units) of any coordinate from a cell face on any level."""
    x_unit = np.asarray(x_unit, f32)
    d = np.full(x_unit.shape[0], np.inf)
    for (_, _, res), dims in zip(model["encoders"], PLANE_DIMS):
        for R in res:
            _, t = cell_and_fraction(x_unit[:, list(dims)], int(R))
            d = np.minimum(d, np.minimum(t, 1 - t).min(axis=1))
    return d


def touches_border_ring(model, x_unit):
    """Per point: some level's cell has a corner on the border ring (coordinate 0 or R - 1)."""
    x_unit = np.asarray(x_unit, f32)
    hit = np.zeros(x_unit.shape[0], bool)
    for (_, _, res), dims in zip(model["encoders"], PLANE_DIMS):
        for R in res:
            cell, _ = cell_and_fraction(x_unit[:, list(dims)], int(R))
            hit |= np.any((cell == 0) | (cell + 1 == int(R) - 1), axis=1)
    return hit


# ---------------------------------------------------------------------------------------------------------------------
# pose kernels
# ---------------------------------------------------------------------------------------------------------------------
def rodrigues_coefficients(t2, dtype=f64, branch=None):
    """(A, B) of exp(w) = I + A [w]x + B [w]x^2 for theta^2 = t2 (array of `dtype`).  float32 mode: the kernel's
    operations — the series under 2^-24, otherwise double from sqrt((double)t2), rounded to float once.  `branch`
    ("series" / "closed") forces one of them for every element."""
    t2 = np.asarray(t2, dtype)
    series = t2 < dtype(SERIES_BELOW) if branch is None else np.full(t2.shape, branch == "series")
    one, half = dtype(1), dtype(0.5)
    As = one - t2 / dtype(6)
    Bs = half - t2 / dtype(24)
    with np.errstate(invalid="ignore", divide="ignore"):
        th = np.sqrt(t2.astype(f64))
        h = 0.5 * th
        sh = np.sin(h) / h
        Ac = (np.sin(th) / th).astype(dtype)
        Bc = (0.5 * (sh * sh)).astype(dtype)
    return np.where(series, As, Ac).astype(dtype), np.where(series, Bs, Bc).astype(dtype)


def rodrigues(w, dtype=f64):
    """exp(w) [n, 3, 3] of w [n, 3], in the kernel's operation order (w = 0 rows are the identity)."""
    w = np.asarray(w, dtype).reshape(-1, 3)
    t2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    A, B = rodrigues_coefficients(t2, dtype)
    E = np.empty((w.shape[0], 3, 3), dtype)
    for i in range(3):
        for j in range(3):
            if i == j:
                k = np.zeros_like(t2)
                s = w[:, i] * w[:, j] - t2
            else:
                third = w[:, 3 - i - j]
                k = -third if (j - i + 3) % 3 == 1 else third
                s = w[:, i] * w[:, j]
            E[:, i, j] = (dtype(1 if i == j else 0) + A * k) + B * s
    E[t2 == 0] = np.eye(3, dtype=dtype)
    return E


def pose_apply(cams, delta, dtype=f32):
    """cnc_camera_pose_apply: cams [C, 24], delta [C, 6] = (omega, tau) -> the rewritten table."""
    cams = np.asarray(cams, dtype)
    delta = np.asarray(delta, dtype).reshape(-1, 6)
    out = cams.copy()
    w, tau = delta[:, :3], delta[:, 3:]
    t2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    E = rodrigues(w, dtype)
    R0 = cams[:, 4:16].reshape(-1, 3, 4)[:, :, :3]
    R1 = np.empty_like(R0)
    for i in range(3):
        for j in range(3):
            R1[:, i, j] = (E[:, i, 0] * R0[:, 0, j] + E[:, i, 1] * R0[:, 1, j]) + E[:, i, 2] * R0[:, 2, j]
    rows = out[:, 4:16].reshape(-1, 3, 4)                       # a copy: written back below
    rot = t2 != 0
    rows[rot, :, :3] = R1[rot]
    t0 = rows[:, :, 3]
    rows[:, :, 3] = np.where(tau != 0, t0 + tau, t0)
    out[:, 4:16] = rows.reshape(-1, 12)
    return out


def ray_pose_q(g_x, t_starts, t_ends, starts, counts, dirs, dtype=f32):
    """Stage 1: q [n_rays, 6] = (d x g_d, g_o), the sums over a ray's samples in sample order from +0."""
    g_x = np.asarray(g_x, dtype).reshape(-1, 3)
    t0, t1, d = np.asarray(t_starts, dtype), np.asarray(t_ends, dtype), np.asarray(dirs, dtype).reshape(-1, 3)
    n_rays, n = d.shape[0], g_x.shape[0]
    q = np.zeros((n_rays, 6), dtype)
    for r in range(n_rays):
        go, gd = np.zeros(3, dtype), np.zeros(3, dtype)
        s0, c = int(starts[r]), int(counts[r])
        if s0 < 0 or c < 0 or s0 > n:
            s0 = c = 0
        for s in range(s0, min(s0 + c, n)):
            m = (t0[s] + t1[s]) * dtype(0.5)
            go = go + g_x[s]
            gd = gd + m * g_x[s]
        q[r, 0] = d[r, 1] * gd[2] - d[r, 2] * gd[1]
        q[r, 1] = d[r, 2] * gd[0] - d[r, 0] * gd[2]
        q[r, 2] = d[r, 0] * gd[1] - d[r, 1] * gd[0]
        q[r, 3:] = go
    return q


def pose_fold(q, cam_ids, n_cams, dtype=f32):
    """Stage 2: per chunk of 256 consecutive rays and camera, the chunk's rows in ray order from +0; the chunks' sums in
    chunk order from +0."""
    q = np.asarray(q, dtype)
    ids = np.clip(np.asarray(cam_ids, np.int64), 0, n_cams - 1)
    G = np.zeros((n_cams, 6), dtype)
    for k0 in range(0, q.shape[0], POSE_CHUNK):
        part = np.zeros((n_cams, 6), dtype)
        for r in range(k0, min(k0 + POSE_CHUNK, q.shape[0])):
            part[ids[r]] = part[ids[r]] + q[r]
        G = G + part
    return G


def ray_pose_grad(g_x, t_starts, t_ends, starts, counts, dirs, cam_ids, n_cams, dtype=f32):
    """cnc_ray_pose_grad: G [n_cams, 6]."""
    return pose_fold(ray_pose_q(g_x, t_starts, t_ends, starts, counts, dirs, dtype), cam_ids, n_cams, dtype)
