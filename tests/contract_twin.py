"""NumPy float32 twin of the unbounded field's map of the position (include/cnc_hip.h, cnc_field_prepare_contracted /
CNC_FIELD_CONTRACT; the device function is field_unit_position, cnc_amd/csrc/field_common.hpp), written op by op in the
header's order, and the point set the unbounded field's tests share.

Every operation below is one IEEE float32 operation (NumPy keeps float32 when both operands are float32; np.sqrt and
the division are correctly rounded), none fused — the library is built with contraction off."""
import numpy as np

f32 = np.float32
BOX = np.array([-1.5, -1.0, -2.0, 1.5, 2.0, 1.0], f32)        # asymmetric on purpose: every axis has its own min and extent


def contract(p, aabb=BOX):
    """(x [N, 3] float32, selector [N] uint8) of world positions p [N, 3]."""
    p, aabb = np.ascontiguousarray(p, f32), np.asarray(aabb, f32)
    lo, hi = aabb[:3], aabb[3:]
    with np.errstate(all="ignore"):
        u = (p - lo) / (hi - lo)
        c = u * f32(2) - f32(1)
        s = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        mag = np.sqrt(s)
        k = f32(2) - f32(1) / mag
        far = k[:, None] * (c / mag[:, None])
        c = np.where((mag > f32(1))[:, None], far, c)
        x = c / f32(4) + f32(0.5)
    assert x.dtype == f32 and mag.dtype == f32 and k.dtype == f32
    sel = ((x > f32(0)) & (x < f32(1))).all(axis=1)
    return x, sel.astype(np.uint8)


def exact_cases(aabb=BOX):
    """[3, 3]: the box centre (-> 0.5 on every axis); u = (1, .5, .5), i.e. mag == 1 exactly: not contracted (-> 0.75 on
    x); p_x = 1e6 (-> just below 1 on x)."""
    aabb = np.asarray(aabb, f32)
    lo, hi = aabb[:3], aabb[3:]
    centre = (lo + (hi - lo) * f32(0.5)).astype(f32)
    on_sphere = centre.copy()
    on_sphere[0] = hi[0]
    far = centre.copy()
    far[0] = f32(1e6)
    return np.stack([centre, on_sphere, far]).astype(f32)


def points(n, seed=0, aabb=BOX):
    """n seeded world positions [n, 3] float32.  Three families interleaved row by row — uniform in 1.2 x the box
    (a third of them inside the unit ball: uncontracted), normal x 10 box extents, normal x 1e4 (contracted) — so that a
    32-sample tile mixes contracted and uncontracted rows; to make that hold for EVERY tile, row 5 of each tile is drawn
    uniformly inside 0.99 of the unit ball (chance alone leaves 2 % of the tiles without an uncontracted row).  Rows
    0..2 (as far as n reaches) are `exact_cases`."""
    aabb = np.asarray(aabb, f32)
    lo, hi = aabb[:3].astype(np.float64), aabb[3:].astype(np.float64)
    centre, ext = (lo + hi) / 2, hi - lo
    rng = np.random.default_rng([seed, n])
    uni = centre + ext * rng.uniform(-0.6, 0.6, size=(n, 3))
    mid = centre + 10.0 * ext * rng.standard_normal((n, 3))
    far = 1.0e4 * rng.standard_normal((n, 3))
    d = rng.standard_normal((n, 3))
    ball = centre + ext / 2 * (0.99 * rng.uniform(size=(n, 1)) ** (1.0 / 3.0)) * d / np.linalg.norm(d, axis=1, keepdims=True)
    kind = (np.arange(n) % 3)[:, None]
    p = np.where(kind == 0, uni, np.where(kind == 1, mid, far))
    p = np.where((np.arange(n) % 32 == 5)[:, None], ball, p).astype(f32)
    ex = exact_cases(aabb)
    k = min(n, len(ex))
    p[:k] = ex[:k]
    return p
