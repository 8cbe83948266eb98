"""NumPy twin of cnc_table_adam (cnc_amd/csrc/table_adam.hip), written from the arithmetic include/cnc_hip.h and the
kernel's header document: every operation in IEEE double or float exactly where the kernel has it, every `(float)` an
explicit rounding.  The library is built with contraction off, double `sqrt` and `/` are correctly rounded, so the twin
predicts every bit of p, m, v, of the sign plane and of the clip counter (tests/test_gpu_table_adam_matrix.py).

    g   = ((g0 + g1) + g2) + g3                       float; over the pieces that cover the element, in slot order; the
                                                      first covering piece is copied; nothing covers it: 0
    g   = (float)((double)g + (double)p * wd)         only when wd != 0
    m   = (float)((double)m + (1 - b1) * (double)(g - m))                    g - m in float
    v   = (float)(b2 * (double)v + ((1 - b2) * (double)g) * (double)g)
    p   = (float)((double)p - ((lr / (1 - b1^t)) * (double)m) / (sqrt((double)v) / sqrt(1 - b2^t) + eps))

The bound `error_bound` holds such a float32-state update to the same update carried out in float64 throughout.
With u = 2^-24 (one unit roundoff per `(float)`, one for the float `g - m`, one for the decay's rounding of g), hats
for the twin's values, stars for the float64 ones, and e_p, e_m, e_v the bounds on |p^ - p*|, |m^ - m*|, |v^ - v*|
going in (all zero when both start from the same float32 state):

    e_g  = wd e_p + u |g^|                            (0 when wd = 0: g is then the same float in both)
    e_m' = (1 - a) e_m + a e_g + a u |g^ - m^| + u |m^'|                     a = 1 - b1
    e_v' = b2 e_v + (1 - b2) e_g (2 |g^| + e_g) + u |v^'|
    D^   = sqrt(v^') / c + eps,   D_lo = sqrt(max(v^' - e_v', 0)) / c + eps <= D*,     c = sqrt(1 - b2^t)
    e_D  = e_v' / (c (sqrt(v^') + sqrt(max(v^' - e_v', 0))))                 (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b))
    e_p' = e_p + L (e_m' / D^ + (|m^'| + e_m') e_D / (D^ D_lo)) + u |p^'|    L = lr / (1 - b1^t)

Every term is a magnitude of an operand, none the ulp of a result: m' = (1 - a) m + a g cancels when m and g have
mixed magnitudes and signs, and its error stays a u |g|.  The float64 side's own roundings (2^-53 of the same
magnitudes, a few per expression) are 2^-29 of the terms above; the whole bound is multiplied by 1 + 2^-20 for them
and for the second-order products of u left out."""
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20

Piece = Optional[Tuple[np.ndarray, int, int]]            # (values [hi - lo], lo, hi) in elements, or None = slot absent


class Step(NamedTuple):
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    bits: Optional[np.ndarray]                           # uint8 [n / 8] when n % 8 == 0, else None
    clipped: int
    g: np.ndarray                                        # the gradient after the decay (float32)
    gm: np.ndarray                                       # the float g - m (for the tests' zero-or-normal check)


def grad_sum(pieces: Sequence[Piece], n: int) -> np.ndarray:
    g = np.zeros(n, f32)
    covered = np.zeros(n, bool)
    for pc in pieces:
        if pc is None:
            continue
        q, lo, hi = pc
        q = np.asarray(q, f32).reshape(-1)[:hi - lo]
        assert 0 <= lo <= hi <= n and q.size == hi - lo
        with np.errstate(all="ignore"):
            g[lo:hi] = np.where(covered[lo:hi], g[lo:hi] + q, q)          # a copy keeps -0.0 and a NaN's bits
        covered[lo:hi] = True
    return g


def scalars(lr, b1, b2, step):
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) as the launcher computes them (the C library's pow)."""
    return float(lr) / (1.0 - math.pow(b1, step)), math.sqrt(1.0 - math.pow(b2, step))


def sign_plane(p: np.ndarray):
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        bits = np.packbits(p >= 0, bitorder="little") if p.size % 8 == 0 else None
        clipped = int(np.count_nonzero(~((p >= -1) & (p <= 1))))
    return bits, clipped


def adam_step(p, m, v, pieces, n, lr, b1, b2, eps, wd, step) -> Step:
    p, m, v = (np.asarray(t, f32).reshape(-1) for t in (p, m, v))
    assert p.size == m.size == v.size == n
    L, c = scalars(lr, b1, b2, step)
    a, omb2 = 1.0 - b1, 1.0 - b2
    g = grad_sum(pieces, n)
    with np.errstate(all="ignore"):
        if wd != 0.0:
            g = (g.astype(f64) + p.astype(f64) * f64(wd)).astype(f32)
        gm = g - m                                                        # float32
        m1 = (m.astype(f64) + f64(a) * gm.astype(f64)).astype(f32)
        g64 = g.astype(f64)
        v1 = (f64(b2) * v.astype(f64) + (f64(omb2) * g64) * g64).astype(f32)
        denom = np.sqrt(v1.astype(f64)) / f64(c) + f64(eps)
        p1 = (p.astype(f64) - (f64(L) * m1.astype(f64)) / denom).astype(f32)
    bits, clipped = sign_plane(p1)
    return Step(p1, m1, v1, bits, clipped, g, gm)


def adam_step_flushing(p, m, v, pieces, n, lr, b1, b2, eps, wd, step) -> Step:
    """The same with float32 subnormals flushed to (signed) zero wherever a float is produced or read — what a device
    in flush mode would compute.  Only tests/test_gpu_table_adam_matrix.py's denormal case may fall back on it, and a
    fall-back is a finding."""
    def ftz(x):
        x = np.asarray(x, f32).copy()
        tiny = (np.abs(x) < np.finfo(f32).tiny) & (x != 0)
        x[tiny] = np.copysign(f32(0), x[tiny])
        return x
    p, m, v = (ftz(np.asarray(t, f32).reshape(-1)) for t in (p, m, v))
    L, c = scalars(lr, b1, b2, step)
    g = ftz(grad_sum([None if pc is None else (ftz(pc[0]), pc[1], pc[2]) for pc in pieces], n))
    with np.errstate(all="ignore"):
        if wd != 0.0:
            g = ftz((g.astype(f64) + p.astype(f64) * f64(wd)).astype(f32))
        gm = ftz(g - m)
        m1 = ftz((m.astype(f64) + f64(1.0 - b1) * gm.astype(f64)).astype(f32))
        g64 = g.astype(f64)
        v1 = ftz((f64(b2) * v.astype(f64) + (f64(1.0 - b2) * g64) * g64).astype(f32))
        denom = np.sqrt(v1.astype(f64)) / f64(c) + f64(eps)
        p1 = ftz((p.astype(f64) - (f64(L) * m1.astype(f64)) / denom).astype(f32))
    bits, clipped = sign_plane(p1)
    return Step(p1, m1, v1, bits, clipped, g, gm)


def float64_step(p, m, v, g, lr, b1, b2, eps, wd, step):
    """The update in float64 throughout (g: the summed gradient before the decay)."""
    p, m, v, g = (np.asarray(t, f64) for t in (p, m, v, g))
    L, c = scalars(lr, b1, b2, step)
    g = g + wd * p
    m1 = m + (1.0 - b1) * (g - m)
    v1 = b2 * v + (1.0 - b2) * g * g
    p1 = p - L * m1 / (np.sqrt(v1) / c + eps)
    return p1, m1, v1


def error_bound(before: Step, after: Step, lr, b1, b2, eps, wd, step, e_p=0.0, e_m=0.0, e_v=0.0):
    """(e_p', e_m', e_v') of the module docstring for the twin's step before -> after; `before` supplies the float32 m
    the step started from (its .m), `after` the step's g, g - m, m', v', p'."""
    L, c = scalars(lr, b1, b2, step)
    a = 1.0 - b1
    g, gm = np.abs(after.g.astype(f64)), np.abs(after.gm.astype(f64))
    m1, v1, p1 = np.abs(after.m.astype(f64)), after.v.astype(f64), np.abs(after.p.astype(f64))
    e_g = (wd * e_p + U * g) if wd != 0.0 else 0.0 * g
    e_m1 = (1.0 - a) * e_m + a * e_g + a * U * gm + U * m1
    e_v1 = b2 * e_v + (1.0 - b2) * e_g * (2.0 * g + e_g) + U * v1
    lo = np.sqrt(np.maximum(v1 - e_v1, 0.0))
    D, D_lo = np.sqrt(v1) / c + eps, lo / c + eps
    with np.errstate(invalid="ignore", divide="ignore"):
        e_D = np.where(e_v1 > 0, e_v1 / (c * (np.sqrt(v1) + lo)), 0.0)
    e_p1 = e_p + L * (e_m1 / D + (m1 + e_m1) * e_D / (D * D_lo)) + U * p1
    return e_p1 * SLACK, e_m1 * SLACK, e_v1 * SLACK
