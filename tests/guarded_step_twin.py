"""NumPy twin of the guarded step's device side (cnc_amd/csrc/step_verdict.hip, cnc_table_adam_guarded in table_adam.hip),
written from include/cnc_hip.h: the non-finite test on the bits, the range guard's predicate, the seal with its running
products b^t — one IEEE double multiplication a step, so the twin predicts every bit, which a library pow would not allow —
and a guarded Adam step built on tests/adam_twin.adam_step.

    scan   acc |= NONFINITE    when any scanned float32 has (bits & 0x7f800000) == 0x7f800000
           acc |= RANGE_GUARD  when guard[0] != 0 and guard[0] >= seen, or any of guard[1..5] == pack_id
    seal   skip = acc; acc = 0; found_inf = 1.0 if skip else 0.0
           skip:  skipped += 1; reasons_seen |= skip; nothing else moves
           go:    b1_pow *= b1; b2_pow *= b2; lr_over_bc1 = lr / (1 - b1_pow); bc2_sqrt = sqrt(1 - b2_pow);
                  one_minus_b1 = 1 - b1; b2; one_minus_b2 = 1 - b2; eps; wd; the clip counters = 0
    adam   skip:  every input as it was
           go:    adam_twin.adam_step with (lr_over_bc1, bc2_sqrt) in place of the launcher's pow-based pair
"""
import copy
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

import adam_twin

NONFINITE, RANGE_GUARD = 1, 2
f32 = np.float32


def nonfinite(x) -> bool:
    """True when any float32 of `x` is +-inf or a NaN of any payload: all eight exponent bits set."""
    bits = np.ascontiguousarray(np.asarray(x, f32)).reshape(-1).view(np.uint32)
    return bool(((bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)).any())


def guard_fired(words, seen: int, pack_id: int) -> bool:
    """`check_range_guard`'s predicate (cnc_amd/field.py) on the first six guard words, as unsigned 32-bit values."""
    w = [int(x) & 0xFFFFFFFF for x in words[:6]]
    return (w[0] != 0 and w[0] >= (seen & 0xFFFFFFFF)) or any(x == (pack_id & 0xFFFFFFFF) for x in w[1:6])


@dataclass
class Verdict:
    """cnc_step_verdict_t."""
    acc: int = 0
    skip: int = 0
    skipped: int = 0
    reasons_seen: int = 0
    b1_pow: float = 1.0
    b2_pow: float = 1.0
    lr_over_bc1: float = 0.0
    one_minus_b1: float = 0.0
    b2: float = 0.0
    one_minus_b2: float = 0.0
    bc2_sqrt: float = 0.0
    eps: float = 0.0
    wd: float = 0.0

    def doubles(self) -> List[float]:
        """The nine doubles in the struct's order (for a bit comparison with the device's)."""
        return [self.b1_pow, self.b2_pow, self.lr_over_bc1, self.one_minus_b1, self.b2, self.one_minus_b2, self.bc2_sqrt,
                self.eps, self.wd]


def seeded(b1: float, b2: float, t0: int) -> Verdict:
    """The buffer as the host leaves it for an optimizer that has taken t0 updates: zero but for pow(b, t0)."""
    return Verdict(b1_pow=math.pow(b1, t0), b2_pow=math.pow(b2, t0))


def scan(v: Verdict, tensors=(), guard=None, seen=0, pack_id=0):
    """-> (the verdict after the scan, what `poison` receives or None without a guard)."""
    v = copy.copy(v)
    if any(t is not None and np.size(t) and nonfinite(t) for t in tensors):
        v.acc |= NONFINITE
    poison = None
    if guard is not None:
        fired = guard_fired(guard, seen, pack_id)
        if fired:
            v.acc |= RANGE_GUARD
        poison = f32(np.inf) if fired else f32(0.0)
    return v, poison


def seal(v: Verdict, lr, b1, b2, eps, wd, clip_counters=()):
    """-> (the sealed verdict, found_inf as a float32, the clip counters afterwards)."""
    v = copy.copy(v)
    v.skip, v.acc = v.acc, 0
    counters = [int(c) for c in clip_counters]
    if v.skip:
        v.skipped += 1
        v.reasons_seen |= v.skip
        return v, f32(1.0), counters
    f64 = np.float64
    v.b1_pow = float(f64(v.b1_pow) * f64(b1))
    v.b2_pow = float(f64(v.b2_pow) * f64(b2))
    v.lr_over_bc1 = float(f64(lr) / (f64(1.0) - f64(v.b1_pow)))
    v.one_minus_b1 = float(f64(1.0) - f64(b1))
    v.b2 = float(b2)
    v.one_minus_b2 = float(f64(1.0) - f64(b2))
    v.bc2_sqrt = float(np.sqrt(f64(1.0) - f64(v.b2_pow)))
    v.eps, v.wd = float(eps), float(wd)
    return v, f32(0.0), [0] * len(counters)


def adam_step_with_scalars(p, m, v, pieces, n, lr_over_bc1, bc2_sqrt, b1, b2, eps, wd) -> adam_twin.Step:
    """adam_twin.adam_step with the two step-dependent factors given instead of computed from pow(b, step)."""
    saved = adam_twin.scalars
    adam_twin.scalars = lambda lr, b1_, b2_, step: (float(lr_over_bc1), float(bc2_sqrt))
    try:
        return adam_twin.adam_step(p, m, v, pieces, n, 0.0, b1, b2, eps, wd, 0)
    finally:
        adam_twin.scalars = saved


def guarded_adam_step(verdict: Verdict, p, m, v, pieces, n, b1, b2) -> Optional[adam_twin.Step]:
    """cnc_table_adam_guarded on a sealed verdict: None on skip (nothing moves), the updated state on go.  b1, b2: the betas
    the verdict was sealed with (1 - b1 and 1 - b2 are formed from them as the seal forms them)."""
    if verdict.skip:
        return None
    assert verdict.one_minus_b1 == 1.0 - b1 and verdict.b2 == b2 and verdict.one_minus_b2 == 1.0 - b2
    return adam_step_with_scalars(p, m, v, pieces, n, verdict.lr_over_bc1, verdict.bc2_sqrt, b1, b2, verdict.eps, verdict.wd)
