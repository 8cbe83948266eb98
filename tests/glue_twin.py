"""float32 NumPy twins of the field's glue kernels and the two streaming kernels (cnc_amd/csrc/field_glue.hip), written
from include/cnc_hip.h and the kernels' header document, operation for operation: every intermediate is a float32 array,
every operator one correctly rounded float32 operation, nothing fused (NumPy never fuses two ufuncs; the library is built
with contraction off).  What the kernels compute with +, -, *, /, comparisons and the half round trip is therefore
predicted bit for bit; `expf` and `sincosf` are the only library functions, and for those the twins return the exact
float32 ARGUMENT, whose float64 function the tests take as reference (tests/test_gpu_field_glue.py)."""
import numpy as np

f32, f64 = np.float32, np.float64

SH_C = [f32(c) for c in (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997,
                         0.31539156525251999, 0.54627421529603959, 0.59004358992664352, 2.8906114426405538,
                         0.45704579946446572, 0.3731763325901154, 1.4453057213202769)]


def prepare(pos, aabb):
    """x_unit = (pos - lo) / (hi - lo); selector = all(0 < x_unit < 1), strict (NaN: 0)."""
    pos, aabb = np.asarray(pos, f32), np.asarray(aabb, f32)
    with np.errstate(all="ignore"):
        x = (pos - aabb[None, :3]) / (aabb[None, 3:] - aabb[None, :3])
        sel = ((x > f32(0)) & (x < f32(1))).all(axis=1).astype(np.uint8)
    return x, sel


def direction(dirs):
    """((d + 1) / 2) * 2 - 1: what the reference and the encoding do to a view direction between them."""
    d = np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        return ((d + f32(1)) / f32(2)) * f32(2) - f32(1)


def sh16(dirs, fp16=False):
    """The sixteen real spherical harmonics up to degree 4 of direction(dirs), in the association of the kernel's
    `sh4_quad` (a product `c * a * b` is `(c * a) * b`)."""
    d = direction(dirs)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c3b, c4, c5, c6, c7, c8, c9 = SH_C
    one, three, five = f32(1), f32(3), f32(5)
    with np.errstate(all="ignore"):
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        o = [np.full_like(x, c0), -c1 * y, c1 * z, -c1 * x,
             c2 * xy, -c2 * yz, c3 * zz - c3b, -c2 * xz,
             c4 * xx - c4 * yy, (c5 * y) * ((-three * xx) + yy), (c6 * xy) * z, (c7 * y) * (one - five * zz),
             (c8 * z) * (five * zz - three), (c7 * x) * (one - five * zz), (c9 * z) * (xx - yy),
             (c5 * x) * ((-xx) + three * yy)]
        out = np.stack(o, axis=1).astype(f32)
        if fp16:
            out = out.astype(np.float16).astype(f32)
    assert out.dtype == f32
    return out


def sh16_float64(d):
    """The closed forms in float64 of a direction d in [-1, 1]^3 (no (d + 1) / 2 detour), written as polynomials in their
    textbook shape rather than in the kernel's association."""
    d = np.asarray(d, f64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([
        np.full_like(x, 0.28209479177387814),
        -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
        0.94617469575755997 * z * z - 0.31539156525251999, -1.0925484305920792 * x * z,
        0.54627421529603959 * (x * x - y * y),
        0.59004358992664352 * (y * y * y - 3.0 * x * x * y),
        2.8906114426405538 * x * y * z,
        0.45704579946446572 * (y - 5.0 * y * z * z),
        0.3731763325901154 * (5.0 * z * z * z - 3.0 * z),
        0.45704579946446572 * (x - 5.0 * x * z * z),
        1.4453057213202769 * (z * x * x - z * y * y),
        0.59004358992664352 * (3.0 * x * y * y - x * x * x)], axis=1)


def sinusoid_arguments(x, freqs):
    """[N, n_freqs, 3] float32 products x * f_k: the arguments the kernel hands to sincosf."""
    x, freqs = np.asarray(x, f32), np.asarray(freqs, f32)
    return (x[:, None, :] * freqs[None, :, None]).astype(f32)


def sinusoid(x, freqs, width):
    """[N, width] float64: [x | sin(f_0 x) (3) | cos(f_0 x) (3) | ... | zeros], the sines and cosines those of the
    float32 arguments in float64; and the mask of the columns that must be met exactly."""
    x = np.asarray(x, f32)
    N, nf = x.shape[0], len(freqs)
    out = np.zeros((N, width), f64)
    exact = np.ones(width, bool)
    out[:, :3] = x
    arg = sinusoid_arguments(x, freqs).astype(f64)
    for k in range(nf):
        out[:, 3 + 6 * k:6 + 6 * k] = np.sin(arg[:, k])
        out[:, 6 + 6 * k:9 + 6 * k] = np.cos(arg[:, k])
        exact[3 + 6 * k:9 + 6 * k] = False
    return out, exact


def density_argument(base0):
    """float32 b - 1: the argument of the density's expf."""
    with np.errstate(all="ignore"):
        return np.asarray(base0, f32) - f32(1)


def head_input(base, geo, dirs, ld_head, fp16):
    """[N, ld_head] float32 = [sh16 | base[:, 1:1 + geo] | zeros]."""
    base = np.asarray(base, f32)
    out = np.zeros((base.shape[0], ld_head), f32)
    out[:, :16] = sh16(dirs, fp16)
    out[:, 16:16 + geo] = base[:, 1:1 + geo]
    return out


def ste_forward(x):
    """(c >= 0) * 1 + (c < 0) * -1 of c = clamp(x, -1, 1) (NaN: 0)."""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        c = np.clip(x, f32(-1), f32(1))
        return (c >= 0).astype(f32) * f32(1) + (c < 0).astype(f32) * f32(-1)


def ste_backward(x, g):
    x, g = np.asarray(x, f32), np.asarray(g, f32)
    with np.errstate(invalid="ignore"):
        return g * ((x >= f32(-1)) & (x <= f32(1))).astype(f32)


def relu_backward(go, y):
    go, y = np.asarray(go, f32), np.asarray(y, f32)
    with np.errstate(invalid="ignore"):
        return np.where(y > 0, go, f32(0))
