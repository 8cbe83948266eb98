"""NumPy twin of csrc/camera.hip: OpenCV's camera models forward, the three undistortion solvers with the kernel's
control flow, and pixel -> ray.

Every function takes `dtype`: float64 (the reference the GPU tests measure against) or float32 — the same formulas in
the kernels' operation order, evaluated by NumPy in float32: a second float32 evaluation that is not the kernel.  With
contraction off and correctly rounded division / sqrt on the device, the float32 mode agrees with the kernels bit for
bit on everything but the fisheye's tan (both sides round a double tan to float; the libraries may differ in the last
double bit).  Points are vectorised; a point that has stopped is frozen with `np.where`, which is what `break` does to a
lane."""
import numpy as np

HALF_PI_F32 = np.float32(np.pi / 2)


def _cols(a, dtype):
    a = np.asarray(a, dtype=dtype)
    return [a[..., k] for k in range(a.shape[-1])]


def distort(xy, params, dtype=np.float64):
    """Ideal (x, y) -> distorted; params (..., 8) = k1 k2 p1 p2 k3 k4 k5 k6."""
    k1, k2, p1, p2, k3, k4, k5, k6 = _cols(params, dtype)
    x, y = _cols(xy, dtype)
    r = x * x + y * y
    q = (1 + r * (k1 + r * (k2 + r * k3))) / (1 + r * (k4 + r * (k5 + r * k6)))
    txy = 2 * x * y
    return np.stack([x * q + (p1 * txy + p2 * (r + 2 * x * x)), y * q + (p2 * txy + p1 * (r + 2 * y * y))], -1).astype(dtype)


def distort12(xy, params, dtype=np.float64):
    """The same with thin-prism terms; params (..., 12) = k1..k6 p1 p2 s1..s4."""
    k1, k2, k3, k4, k5, k6, p1, p2, s1, s2, s3, s4 = _cols(params, dtype)
    x, y = _cols(xy, dtype)
    r = x * x + y * y
    q = (1 + r * (k1 + r * (k2 + r * k3))) / (1 + r * (k4 + r * (k5 + r * k6)))
    txy = 2 * x * y
    return np.stack([x * q + p1 * txy + p2 * (r + 2 * x * x) + s1 * r + s2 * r * r,
                     y * q + p2 * txy + p1 * (r + 2 * y * y) + s3 * r + s4 * r * r], -1).astype(dtype)


def distort_fisheye(xy, params, dtype=np.float64):
    k1, k2, k3, k4 = _cols(params, dtype)
    xy = np.asarray(xy, dtype=dtype)
    r = np.sqrt((xy * xy).sum(-1))
    t = np.arctan(r)
    t2 = t * t
    td = t * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    return (xy * (td / np.maximum(r, 1e-30))[..., None]).astype(dtype)


def undistort_newton(uv, params, eps=1e-6, iters=10, dtype=np.float64, info=None):
    """Layouts 5 and 8 (params (..., 8) = k1 k2 p1 p2 k3 k4 k5 k6; layout 5 = the last three zero).  `info`, a dict,
    receives `rounds` (Newton updates applied per point) and `det_stop` (stopped on |det| < eps)."""
    k1, k2, p1, p2, k3, k4, k5, k6 = _cols(params, dtype)
    u, v = _cols(uv, dtype)
    eps = dtype(eps)
    x, y = u.copy(), v.copy()
    live = np.ones(np.broadcast(u, k1).shape, bool)
    x, y = np.broadcast_to(x, live.shape).copy(), np.broadcast_to(y, live.shape).copy()
    rounds, det_stop = np.zeros(live.shape, int), np.zeros(live.shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            r = x * x + y * y
            A = 1 + r * (k1 + r * (k2 + r * k3))
            B = 1 + r * (k4 + r * (k5 + r * k6))
            q = A / B
            txy = 2 * x * y
            gx = (x * q + (p1 * txy + p2 * (r + 2 * x * x))) - u
            gy = (y * q + (p2 * txy + p1 * (r + 2 * y * y))) - v
            Ar = k1 + r * (2 * k2 + r * (3 * k3))
            Br = k4 + r * (2 * k5 + r * (3 * k6))
            qr = (Ar * B - A * Br) / (B * B)
            qx = 2 * x * qr
            qy = 2 * y * qr
            j00 = (q + x * qx) + 2 * (p1 * y + 3 * p2 * x)
            j01 = x * qy + 2 * (p1 * x + p2 * y)
            j10 = y * qx + 2 * (p2 * y + p1 * x)
            j11 = (q + y * qy) + 2 * (p2 * x + 3 * p1 * y)
            det = j00 * j11 - j01 * j10
            singular = live & (np.abs(det) < eps)
            det_stop |= singular
            live = live & ~singular
            sx = (j01 * gy - j11 * gx) / det
            sy = (j10 * gx - j00 * gy) / det
            x = np.where(live, x + sx, x)
            y = np.where(live, y + sy, y)
            rounds += live
            live = live & ~((np.abs(sx) < eps) & (np.abs(sy) < eps))
    if info is not None:
        info.update(rounds=rounds, det_stop=det_stop)
    return np.stack([x, y], -1).astype(dtype)


def undistort_fixed_point(uv, params, iters=10, dtype=np.float64):
    """Layout 12 (k1..k6 p1 p2 s1..s4): OpenCV's iteration; a negative inverse radial factor returns the input."""
    c = _cols(params, dtype)
    u, v = _cols(uv, dtype)
    shape = np.broadcast(u, c[0]).shape
    x, y = np.broadcast_to(u, shape).copy(), np.broadcast_to(v, shape).copy()
    failed = np.zeros(shape, bool)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            r = x * x + y * y
            inv = (1 + ((c[5] * r + c[4]) * r + c[3]) * r) / (1 + ((c[2] * r + c[1]) * r + c[0]) * r)
            failed |= ~failed & (inv < 0)
            txy = 2 * x * y
            dx = ((c[6] * txy + c[7] * (r + 2 * x * x)) + c[8] * r) + c[9] * r * r
            dy = ((c[6] * (r + 2 * y * y) + c[7] * txy) + c[10] * r) + c[11] * r * r
            x = np.where(failed, x, (u - dx) * inv)
            y = np.where(failed, y, (v - dy) * inv)
    return np.stack([np.where(failed, u, x), np.where(failed, v, y)], -1).astype(dtype)


def undistort_fisheye(uv, params, eps=1e-6, iters=10, dtype=np.float64, info=None):
    """theta_d = min(|uv|, pi/2); Newton on theta with the update in float64 whatever `dtype` (the kernel's), theta kept
    in `dtype`; tan in float64, rounded to `dtype` once.  Not converged, or theta negative: the input comes back."""
    k1, k2, k3, k4 = _cols(params, np.float64)
    u, v = _cols(uv, dtype)
    eps_t = dtype(eps)
    td = np.sqrt(u * u + v * v)
    td = np.where(td > dtype(HALF_PI_F32), dtype(HALF_PI_F32), td).astype(dtype)
    shape = np.broadcast(td, k1).shape
    td = np.broadcast_to(td, shape)
    theta = td.copy()
    small = ~(td > eps_t)
    live = ~small
    converged = small.copy()
    rounds = np.zeros(shape, int)
    with np.errstate(all="ignore"):
        for _ in range(int(iters)):
            t = theta.astype(np.float64)
            t2 = t * t
            t4 = t2 * t2
            t6 = t4 * t2
            t8 = t4 * t4
            a, b, c, d = k1 * t2, k2 * t4, k3 * t6, k4 * t8
            fix = (t * ((((1.0 + a) + b) + c) + d) - td.astype(np.float64)) / ((((1.0 + 3.0 * a) + 5.0 * b) + 7.0 * c) + 9.0 * d)
            theta = np.where(live, (t - fix).astype(dtype), theta)
            rounds += live
            done = live & (np.abs(fix) < np.float64(eps_t))
            converged |= done
            live = live & ~done
        scale = np.where(small, dtype(0), np.tan(theta.astype(np.float64)).astype(dtype) / np.where(small, dtype(1), td))
    keep = converged & ~(theta < 0)
    if info is not None:
        info.update(rounds=rounds, converged=converged)
    return np.stack([np.where(keep, u * scale, u), np.where(keep, v * scale, v)], -1).astype(dtype)


PINHOLE, OPENCV, FISHEYE = 0, 1, 2


def camera_rays(cams, model, opengl, cam_ids, px, py, eps=1e-6, iters=10, dtype=np.float64):
    """cnc_camera_rays: cams (n_cams, 24) = fx fy cx cy | [R | t] rows | 8 coefficients -> (origins, viewdirs)."""
    row = np.asarray(cams, dtype=dtype)[np.asarray(cam_ids)]
    fx, fy, cx, cy = (row[:, k] for k in range(4))
    u = ((np.asarray(px).astype(dtype) - cx) + dtype(0.5)) / fx
    v = ((np.asarray(py).astype(dtype) - cy) + dtype(0.5)) / fy
    uv = np.stack([u, v], -1)
    if model == OPENCV:
        uv = undistort_newton(uv, row[:, 16:24], eps, iters, dtype)
    elif model == FISHEYE:
        uv = undistort_fisheye(uv, row[:, 16:20], eps, iters, dtype)
    flip = dtype(-1.0 if opengl else 1.0)
    c0, c1, c2 = uv[:, 0], uv[:, 1] * flip, flip
    R = row[:, 4:16].reshape(-1, 3, 4)
    w = [(R[:, j, 0] * c0 + R[:, j, 1] * c1) + R[:, j, 2] * c2 for j in range(3)]
    length = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    return R[:, :, 3].astype(dtype), np.stack([w[0] / length, w[1] / length, w[2] / length], -1).astype(dtype)


def frame_pixels(width, height):
    """(px, py) of the full-frame form: row-major."""
    i = np.arange(width * height)
    return i % width, i // width


def blend(rgba_u8, bkgd, dtype=np.float64):
    """pixels = rgb / 255 * (a / 255) + bkgd * (1 - a / 255), the loaders' expression."""
    rgba = np.asarray(rgba_u8).astype(dtype) / dtype(255)
    alpha = rgba[:, 3:]
    return (rgba[:, :3] * alpha + np.asarray(bkgd, dtype)[None] * (dtype(1) - alpha)).astype(dtype)


def camera_table(intrinsics, camtoworlds, lens=None):
    intrinsics = np.asarray(intrinsics, np.float32)
    t = np.zeros((intrinsics.shape[0], 24), np.float32)
    t[:, :4] = intrinsics
    t[:, 4:16] = np.asarray(camtoworlds, np.float32)[:, :3, :4].reshape(-1, 12)
    if lens is not None:
        lens = np.asarray(lens, np.float32)
        t[:, 16:16 + lens.shape[1]] = lens
    return t
