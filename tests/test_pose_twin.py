"""CPU checks of the pose-refinement twins (tests/pose_twin.py): the twins the GPU tests hold the kernels to are
themselves held to finite differences and to the algebra they restate.

Position gradient.  `pose_twin.position_grad` against float64 central differences, h = 1e-6 unit-cube units, of the
function it differentiates: the first layer's input row contracted with fixed (dX, dS) (`pose_twin.forward64`, whose
encoder columns are first held to the existing float32 NumPy encoder forward, np_twins.grid_encode_forward).  The cell
and the base fraction are the float32 ones on both sides, so what is left is the differences' own error: truncation
(h (R - 2))^2 times a third-derivative factor of order 10 — 6.6e-8 x 10 at the finest level used, R = 258 — and float64
cancellation 2.2e-16 / 2e-6 per unit of |value|.  Bound: 1e-6 of the entry's sum of |terms| + 1e-9 of sum |dX| + |dS|.
Every point is at least 1e-3 cell units from every cell face on every level (h (R - 2) <= 2.6e-4 keeps both displaced
points in the cell); the points are used as drawn — nothing is filtered, and the test asserts the distance for all.

Pose.  The fold's G against central differences of the loss under a left perturbation exp(phi) exp(omega) R0 at
omega = 0 and |omega| = 0.3; exp(omega) orthonormal; the series and the closed branch of the coefficients at the switch;
zero delta is the identity on the table's bits."""
import numpy as np
import pytest

import np_twins as T
import pose_twin as P
from conftest import make_grid

f32, f64 = np.float32, np.float64
RES_3D, LOG2_3D = (5, 8, 14, 24), 10            # 125 and 512 rows dense, the other two hashed into 2^10
RES_2D, LOG2_2D = (6, 18, 66, 258), 9           # 36 and 324 rows dense, the other two hashed into 2^9
AABB = np.asarray([-1.5, -1.0, -2.0, 1.5, 2.0, 1.0], f32)
H = 1e-6


def make_model(F, seed=3):
    encs = []
    for k, (res, log2, D) in enumerate([(RES_3D, LOG2_3D, 3)] + [(RES_2D, LOG2_2D, 2)] * 3):
        offs, r, emb = make_grid(res, log2, D, F, seed=seed + k)
        encs.append((emb, offs, r))
    return dict(encoders=encs, F=F, freqs=(2.0 ** np.arange(10)).astype(f32))


def n_units():
    return len(RES_3D) + 3 * len(RES_2D)


def draw_points(seed, n_free=48, n_ring=16):
    """Unit-cube points: uniform ones, and ones whose first / last coordinate lies in the outermost cell of the coarse
    levels (x < 0.5 / (R - 2) puts the cell at 0: its lower corners are on the border ring)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.02, 0.98, size=(n_free + n_ring, 3))
    x[n_free:n_free + n_ring // 2, 0] = rng.uniform(0.004, 0.09, size=n_ring // 2)
    x[n_free + n_ring // 2:, 2] = rng.uniform(0.91, 0.996, size=n_ring - n_ring // 2)
    return x.astype(f32)


@pytest.fixture(scope="module", params=[2, 8], ids=["F2", "F8"])
def case(request):
    F = request.param
    model = make_model(F)
    # world positions, and the unit-cube points the kernel's own map makes of them: the points every check uses
    world = (draw_points(seed=16).astype(f64) * (AABB[3:] - AABB[:3]).astype(f64) + AABB[:3]).astype(f32)
    x, inside = P.unit_position(world, AABB)
    assert inside.all()
    rng = np.random.default_rng(5)
    dX = rng.normal(size=(x.shape[0], n_units() * F))
    dS = rng.normal(size=(x.shape[0], 63)) * 0.1
    return model, x, dX, dS, world


def test_points_are_used_as_drawn_and_cover_the_border_ring(case):
    model, x, _, _, _ = case
    assert x.shape[0] == 64, "no point was dropped"
    assert P.face_distance(model, x).min() >= 1e-3
    ring = P.touches_border_ring(model, x)
    assert ring.sum() >= 16 and (~ring).sum() >= 1
    # ... and on a level where the ring matters: cell 0 of the coarsest 3-D level
    cell, _ = P.cell_and_fraction(x, RES_3D[0])
    assert np.any(cell == 0) and np.any(cell == RES_3D[0] - 2)


def test_forward64_is_the_float32_encoder_forward(case):
    model, x, _, _, _ = case
    got = P.features64(model, x)
    col = 0
    for (table, offs, res), dims in zip(model["encoders"], P.PLANE_DIMS):
        want = T.grid_encode_forward(np.ascontiguousarray(x[:, list(dims)]), table, offs, res, ste_binary=True)   # [L, N, F]
        want = np.transpose(want, (1, 0, 2)).reshape(x.shape[0], -1)
        # the float32 forward rounds 2^D products, a running sum, a division and 2^D fmas: a few 2^-24 of |y| <= 1
        assert np.abs(got[:, col:col + want.shape[1]] - want).max() <= 32 * 2.0 ** -24
        col += want.shape[1]
    assert col == got.shape[1]


def test_position_gradient_against_central_differences(case):
    model, x_unit, dX, dS, world = case
    assert P.face_distance(model, x_unit).min() >= 1e-3
    g, mag = P.position_grad(model, AABB, world, np.ones(len(world), np.uint8), dX, dS)
    ext = (AABB[3:] - AABB[:3]).astype(f64)
    worst = 0.0
    for a in range(3):
        sh = np.zeros((len(world), 3))
        sh[:, a] = H
        fd = (P.forward64(model, x_unit, dX, dS, sh) - P.forward64(model, x_unit, dX, dS, -sh)) / (2 * H) / ext[a]
        bound = 1e-6 * mag[:, a] + 1e-9 * (np.abs(dX).sum(axis=1) + np.abs(dS).sum(axis=1)) / ext[a]
        err = np.abs(fd - g[:, a])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (a, float((err / bound).max()))
    assert np.abs(g).min() > 0
    print(f"position gradient against central differences: worst error / bound = {worst:.3g}")


def test_renormalisation_term_matters_in_border_cells(case):
    """The plain trilinear derivative (the normaliser held fixed) is NOT the gradient in a cell with border-ring corners:
    along an axis whose lower corners are invalid the feature does not depend on the coordinate at all."""
    model, _, _, _, _ = case
    F = model["F"]
    table, offs, res = model["encoders"][0]
    R, hs = int(res[0]), int(offs[1] - offs[0])
    x = np.asarray([[0.05, 0.4, 0.6]], f32)                  # cell 0 along x at R = 5
    assert P.cell_and_fraction(x, R)[0][0, 0] == 0
    g = np.ones((1, F))
    _, grad, _ = P._unit_terms(x, table, int(offs[0]), hs, R, g)
    assert grad[0, 0] == pytest.approx(0.0, abs=1e-12)
    sh = np.asarray([[H, 0, 0]])
    v1 = P._unit_terms(x, table, int(offs[0]), hs, R, g, sh)[0]
    v0 = P._unit_terms(x, table, int(offs[0]), hs, R, g, -sh)[0]
    assert abs(v1 - v0) <= 1e-12


def test_rows_outside_the_box_or_deselected_are_zero(case):
    model, _, dX, dS, world = case
    world = world.copy()
    world[0, 1] = 2.5
    world[1, 2] = AABB[2]                                    # on the box face: x_unit = 0, not strictly inside
    sel = np.ones(len(world), np.uint8)
    sel[2] = 0
    g, mag = P.position_grad(model, AABB, world, sel, dX, dS)
    assert np.all(g[:3] == 0) and np.all(mag[:3] == 0) and np.all(g[3:] != 0)


# ---------------------------------------------------------------------------------------------------------------------
# pose
# ---------------------------------------------------------------------------------------------------------------------
def _table(rng, C):
    """A camera table with random rotations (QR of a normal matrix, det +1) and translations."""
    cams = np.zeros((C, P.CAMERA_ROW), f64)
    cams[:, :4] = [400.0, 410.0, 63.5, 47.5]
    for c in range(C):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        cams[c, 4:16] = np.concatenate([q, rng.normal(size=(3, 1))], axis=1).reshape(-1)
    cams[:, 16:] = rng.normal(size=(C, 8)) * 0.01
    return cams


def _expm(w):
    """exp([w]x) by its power series in float64: an independent reference for `rodrigues`."""
    K = np.asarray([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)
    E, term = np.eye(3), np.eye(3)
    for n in range(1, 40):
        term = term @ K / n
        E = E + term
    return E


def test_rodrigues_is_the_matrix_exponential():
    rng = np.random.default_rng(2)
    w = rng.normal(size=(32, 3))
    w *= (rng.uniform(0, 3.1, size=32) / np.linalg.norm(w, axis=1))[:, None]
    w[0] *= 1e-5 / np.linalg.norm(w[0])                      # the series branch
    E = P.rodrigues(w, f64)
    for k in range(32):
        assert np.abs(E[k] - _expm(w[k])).max() <= 1e-14
    E32 = P.rodrigues(w.astype(f32), f32)
    assert E32.dtype == f32
    # float32 mode: three rounded operations per entry on terms of magnitude <= 1 + |sin| + (1 - cos) <= 4
    assert np.abs(E32 - P.rodrigues(w.astype(f32), f64)).max() <= 3 * 2.0 ** -24 * 4


def test_exp_is_orthonormal_to_a_few_ulp():
    rng = np.random.default_rng(4)
    w = rng.normal(size=(256, 3))
    w *= (rng.uniform(0, 3.1, size=256) / np.linalg.norm(w, axis=1))[:, None]
    E = P.rodrigues(w.astype(f32), f32).astype(f64)
    # an entry carries at most 3 roundings of terms summing to <= 3 in magnitude (|dE| <= 9 x 2^-24); (E E^T)_ij then moves by
    # at most 2 sum_k |E_ik| |dE_jk| <= 2 sqrt(3) 9 x 2^-24 = 16 ulp of 1
    dev = np.abs(np.einsum("nij,nkj->nik", E, E) - np.eye(3)).max()
    assert dev <= 16 * 2.0 ** -23
    assert np.abs(np.linalg.det(E) - 1).max() <= 16 * 2.0 ** -23
    E64 = P.rodrigues(w, f64)
    assert np.abs(np.einsum("nij,nkj->nik", E64, E64) - np.eye(3)).max() <= 16 * 2.0 ** -52
    print(f"orthonormality of the float32 exp: {dev / 2.0 ** -23:.2f} ulp")


def test_series_and_closed_branch_agree_at_the_switch():
    for dtype, ulp in ((f32, 2.0 ** -23), (f64, 2.0 ** -52)):
        t2 = np.asarray([P.SERIES_BELOW, np.nextafter(dtype(P.SERIES_BELOW), dtype(0))], dtype)
        As, Bs = P.rodrigues_coefficients(t2, dtype, branch="series")
        Ac, Bc = P.rodrigues_coefficients(t2, dtype, branch="closed")
        # the series' first dropped terms are t2^2 / 120 and t2^2 / 720 = 3e-17 and 5e-18: under half an ulp of either format
        assert np.abs(As - Ac).max() <= ulp and np.abs(Bs - Bc).max() <= ulp
    # the default picks the series strictly below the switch, the closed form at it
    A, _ = P.rodrigues_coefficients(np.asarray([0.0], f32), f32)
    assert A[0] == 1.0


def test_zero_delta_keeps_the_table_bit_for_bit():
    rng = np.random.default_rng(6)
    cams = _table(rng, 5).astype(f32)
    cams[1, 5] = -0.0
    cams[2, 7] = -0.0                                        # a translation component of -0
    out = P.pose_apply(cams, np.zeros((5, 6), f32), f32)
    assert out.tobytes() == cams.tobytes()
    d = np.zeros((5, 6), f32)
    d[3, 4] = 0.25                                           # a translation alone leaves the rotation's bits
    out = P.pose_apply(cams, d, f32)
    assert out[3, 11] == cams[3, 11] + f32(0.25)
    keep = np.ones(cams.shape, bool)
    keep[3, 11] = False
    assert out[keep].tobytes() == cams[keep].tobytes()


@pytest.mark.parametrize("omega", [0.0, 0.3])
def test_tangent_pose_gradient_against_central_differences(omega):
    """L(phi, tau') = sum_s g_s . (t + tau' + m_s exp(phi) d) for the rays of each camera, d drawn with the table
    exp(omega) R0: G[c] must be dL / d(phi, tau') at 0 — the left-perturbation gradient, at omega = 0 and away from it."""
    rng = np.random.default_rng(8)
    C, n_rays = 3, 300
    base = _table(rng, C)
    delta = np.zeros((C, 6))
    if omega:
        w = rng.normal(size=(C, 3))
        delta[:, :3] = w * (omega / np.linalg.norm(w, axis=1))[:, None]
        delta[:, 3:] = rng.normal(size=(C, 3)) * 0.05
    cams = P.pose_apply(base, delta, f64)
    R = cams[:, 4:16].reshape(C, 3, 4)[:, :, :3]
    if omega:
        assert np.abs(R - np.einsum("cij,cjk->cik", np.stack([_expm(w) for w in delta[:, :3]]),
                                    base[:, 4:16].reshape(C, 3, 4)[:, :, :3])).max() <= 1e-14
    ids = rng.integers(0, C, size=n_rays)
    cvec = np.concatenate([rng.uniform(-0.3, 0.3, size=(n_rays, 2)), -np.ones((n_rays, 1))], axis=1)
    d = np.einsum("rij,rj->ri", R[ids], cvec)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    counts = rng.integers(0, 9, size=n_rays)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    n = int(counts.sum())
    t0 = rng.uniform(0.5, 4.0, size=n)
    t1 = t0 + rng.uniform(0.01, 0.1, size=n)
    g_x = rng.normal(size=(n, 3))
    G = P.ray_pose_grad(g_x, t0, t1, starts, counts, d, ids, C, f64)
    ray_of = np.repeat(np.arange(n_rays), counts)
    m = (t0 + t1) * 0.5

    def loss(c, phi, tau):
        E = _expm(phi)
        sel = ids[ray_of] == c
        x = (cams[c, 4:16].reshape(3, 4)[:, 3] + tau)[None, :] + m[sel, None] * (d[ray_of[sel]] @ E.T)
        return float((g_x[sel] * x).sum())

    h = 1e-5
    scale = np.abs(g_x).sum() * 4.0
    for c in range(C):
        for a in range(6):
            e = np.zeros(6)
            e[a] = h
            fd = (loss(c, e[:3], e[3:]) - loss(c, -e[:3], -e[3:])) / (2 * h)
            # exp(phi) d is phi x d + O(phi^2) with an odd remainder: the central difference's error is h^2 / 6 |m g|
            assert abs(fd - G[c, a]) <= (h * h + 1e-10) * scale, (c, a, fd, G[c, a])


def test_fold_order_and_cameras_without_rays():
    rng = np.random.default_rng(9)
    n_rays, C = 1000, 7
    q = rng.normal(size=(n_rays, 6)).astype(f32)
    ids = rng.integers(0, C - 1, size=n_rays)                # camera C - 1 has no rays
    G = P.pose_fold(q, ids, C, f32)
    assert G.dtype == f32 and np.all(G[C - 1] == 0) and not np.signbit(G[C - 1]).any()
    G64 = P.pose_fold(q, ids, C, f64)
    for c in range(C):
        assert np.allclose(G64[c], q[ids == c].astype(f64).sum(axis=0), rtol=0, atol=1e-12)
    # n - 1 float32 additions of terms summing to at most sum |q|
    bound = np.stack([np.abs(q[ids == c]).sum(axis=0) for c in range(C)]) * n_rays * 2.0 ** -24
    assert np.all(np.abs(G - G64) <= bound)
    # out-of-range ids are clamped into the table
    assert np.array_equal(P.pose_fold(q, ids - 3, C, f32), P.pose_fold(q, np.clip(ids - 3, 0, C - 1), C, f32))
