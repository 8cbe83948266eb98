"""CPU-only: the NumPy twin of the guarded step (tests/guarded_step_twin.py) against what include/cnc_hip.h promises —
the non-finite test on the bits, the range guard's predicate against `check_range_guard`'s expression, the seal's two
outcomes, the running products' distance from b ** t, and the guarded Adam step against tests/adam_twin.adam_step."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import adam_twin as T
import guarded_step_twin as G

f32, u32 = np.float32, np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(*words):
    return np.array(words, u32).view(f32)


def test_nonfinite_is_all_exponent_bits_set():
    bad = _bits(0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fa5a5a5, 0xffffffff)
    for x in bad:
        assert G.nonfinite(np.array([0.0, x, 1.0], f32))
    fine = np.concatenate([_bits(0x7f7fffff, 0xff7fffff, 0x00000001, 0x807fffff, 0x80000000, 0x00800000, 0x7f000000),
                           np.array([0.0, 1.0, -3.4e38, 1e-45], f32)])
    assert not G.nonfinite(fine)
    assert not G.nonfinite(np.zeros(0, f32))
    for x in bad:                                        # the same answer as numpy's own test, value by value
        assert not np.isfinite(x)
    assert np.isfinite(fine).all()


def test_guard_predicate_is_the_hosts():
    """Every combination of the three clauses against the expression in cnc_amd/field.py (`check_range_guard`)."""
    rng = np.random.default_rng(1)
    for _ in range(2000):
        seen, pack = int(rng.integers(1, 50)), int(rng.integers(1, 6))
        w = [int(rng.integers(0, 60)) if rng.random() < 0.7 else 0] + [int(rng.integers(0, 8)) for _ in range(5)] + [pack, pack]
        want = bool(w[0] != 0 and w[0] >= seen or any(x == pack for x in w[1:6]))
        assert G.guard_fired(w, seen, pack) == want
    assert not G.guard_fired([6, 0, 0, 0, 0, 0], 7, 3)                   # a stamp older than `seen`
    assert G.guard_fired([7, 0, 0, 0, 0, 0], 7, 3)
    assert not G.guard_fired([0, 0, 0, 0, 0, 0, 3, 3], 0, 3)             # words behind the sixth are not the guard's
    assert G.guard_fired([0, 0, 0, 0, 0, 3], 9, 3) and G.guard_fired([0, 3, 0, 0, 0, 0], 9, 3)


def test_scan_accumulates_and_poison():
    v = G.seeded(0.9, 0.999, 0)
    v1, poison = G.scan(v, [np.ones(5, f32), None, np.zeros(0, f32)])
    assert v1.acc == 0 and poison is None
    v2, _ = G.scan(v1, [np.array([1.0, np.nan], f32)])
    v3, poison = G.scan(v2, [np.ones(3, f32)], guard=[9, 0, 0, 0, 0, 0], seen=4, pack_id=2)
    assert v2.acc == G.NONFINITE and v3.acc == G.NONFINITE | G.RANGE_GUARD and np.isposinf(poison)
    _, poison = G.scan(v, guard=[3, 0, 0, 0, 0, 0], seen=4, pack_id=2)
    assert poison == 0.0 and not np.signbit(poison)


def test_seal_go_and_skip():
    v = G.seeded(0.9, 0.999, 7)
    go, found, counters = G.seal(v, 6e-3, 0.9, 0.999, 1e-15, 2e-6, [5, 0, 9])
    assert found == 0.0 and counters == [0, 0, 0] and go.skip == 0 and go.acc == 0 and go.skipped == 0
    assert go.b1_pow == math.pow(0.9, 7) * 0.9 and go.b2_pow == math.pow(0.999, 7) * 0.999
    assert go.lr_over_bc1 == 6e-3 / (1.0 - go.b1_pow) and go.bc2_sqrt == math.sqrt(1.0 - go.b2_pow)
    assert (go.one_minus_b1, go.b2, go.one_minus_b2, go.eps, go.wd) == (1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-15, 2e-6)
    bad, _ = G.scan(go, [np.array([np.inf], f32)])
    skip, found, counters = G.seal(bad, 3e-3, 0.9, 0.999, 1e-15, 2e-6, [5, 0, 9])
    assert found == 1.0 and counters == [5, 0, 9]
    assert skip.skip == G.NONFINITE and skip.acc == 0 and skip.skipped == 1 and skip.reasons_seen == G.NONFINITE
    assert skip.doubles() == go.doubles()                                # products and scalars: untouched
    again, found, _ = G.seal(skip, 3e-3, 0.9, 0.999, 1e-15, 2e-6)        # the accumulation word was cleared: go
    assert found == 0.0 and again.skip == 0 and again.skipped == 1 and again.reasons_seen == G.NONFINITE
    assert again.b1_pow == go.b1_pow * 0.9


@pytest.mark.parametrize("b", [0.9, 0.999, 0.5, 0.99])
def test_running_products_stay_within_t_ulps_of_the_power(b):
    """t multiplications, each rounded once (relative 2^-53): the product is within (1 + 2^-53)^t - 1 < t 2^-52 of the exact
    b^t — exact as a fraction of the double b — for t up to 30 000, wherever b^t is a normal double.  Below the normal range
    (0.9^t from t = 6 725 on) a relative bound cannot hold for any double arithmetic, pow included; there the product and
    pow(b, t) are both under 2^-1022 and the only use made of either, 1 - b^t, is exactly 1."""
    N, D = Fraction(b).numerator, Fraction(b).denominator            # the double b, exactly: N / 2^k
    shift = D.bit_length() - 1
    assert D == 1 << shift

    def within(x, t, ulps):
        """|x - b^t| <= ulps 2^-52 b^t, in integers: x = a / 2^s, b^t = N^t / 2^(k t)."""
        a, den = Fraction(x).numerator, Fraction(x).denominator
        s_ = den.bit_length() - 1
        Nt = N ** t
        return abs((a << (shift * t)) - (Nt << s_)) << 52 <= ulps * (Nt << s_)

    checkpoints = {1, 2, 3, 7, 10, 100, 1000, 5000, 6000, 10000, 20000, 30000}
    prod = np.float64(1.0)
    checked = 0
    for t in range(1, 30001):
        prod = prod * np.float64(b)
        if t not in checkpoints:
            continue
        if shift * t <= 1022 or (N ** t) >> (shift * t - 1022):         # b^t >= 2^-1022: a normal double
            assert within(float(prod), t, t), (b, t)
            assert within(math.pow(b, t), t, 1)                          # what the product replaces
            checked += 1
        else:
            assert float(prod) < 2.0 ** -1022 and math.pow(b, t) < 2.0 ** -1022
            assert 1.0 - float(prod) == 1.0 == 1.0 - math.pow(b, t)
    assert checked >= 7
    assert float(np.float64(1.0) * np.float64(b)) == math.pow(b, 1)      # t = 1: the product IS the power


def test_twin_seal_chain_matches_a_plain_loop():
    """Five seals from t0 = 7: the products are the seed times b, five times over, in double."""
    v = G.seeded(0.9, 0.999, 7)
    p1, p2 = math.pow(0.9, 7), math.pow(0.999, 7)
    for k in range(5):
        v, _, _ = G.seal(v, 6e-3 * (k + 1), 0.9, 0.999, 1e-15, 0.0)
        p1, p2 = p1 * 0.9, p2 * 0.999
        assert (v.b1_pow, v.b2_pow) == (p1, p2)
        assert v.lr_over_bc1 == 6e-3 * (k + 1) / (1.0 - p1)


def _state(rng, n):
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    p = (sgn() * 10.0 ** rng.uniform(-4, 0, n)).astype(f32)
    m = (sgn() * 10.0 ** rng.uniform(-6, 2, n)).astype(f32)
    v = (10.0 ** rng.uniform(-10, 5, n)).astype(f32)
    g = (sgn() * 10.0 ** rng.uniform(-6, 3, n)).astype(f32)
    return p, m, v, g


@pytest.mark.parametrize("wd", [0.0, 2e-6])
def test_guarded_go_step_is_adam_step_with_the_same_scalars(wd):
    rng = np.random.default_rng(3)
    n = 4100
    p, m, v, g = _state(rng, n)
    pieces = [(g, 0, n), (g[:96], 4, 100)]
    ver = G.seeded(0.9, 0.999, 0)
    ver, _, _ = G.seal(ver, 6e-3, 0.9, 0.999, 1e-15, wd)
    got = G.guarded_adam_step(ver, p, m, v, pieces, n, 0.9, 0.999)
    want = T.adam_step(p, m, v, pieces, n, 6e-3, 0.9, 0.999, 1e-15, wd, 1)       # t = 1: the product equals pow
    for a, b in ((got.p, want.p), (got.m, want.m), (got.v, want.v)):
        assert np.array_equal(a.view(u32), b.view(u32))
    assert np.array_equal(got.bits if got.bits is not None else 0, want.bits if want.bits is not None else 0)
    # a late step: the scalars are the verdict's, and adam_step fed those very scalars gives the same bits
    ver = G.seeded(0.9, 0.999, 40)
    for _ in range(3):
        ver, _, _ = G.seal(ver, 5e-3, 0.9, 0.999, 1e-15, wd)
    got = G.guarded_adam_step(ver, p, m, v, pieces, n, 0.9, 0.999)
    want = G.adam_step_with_scalars(p, m, v, pieces, n, 5e-3 / (1.0 - ver.b1_pow), math.sqrt(1.0 - ver.b2_pow), 0.9, 0.999,
                                    1e-15, wd)
    for a, b in ((got.p, want.p), (got.m, want.m), (got.v, want.v)):
        assert np.array_equal(a.view(u32), b.view(u32))
    # ... and against pow at that step: m and v do not see the scalars' difference, p moves by at most one float32 ulp
    ref = T.adam_step(p, m, v, pieces, n, 5e-3, 0.9, 0.999, 1e-15, wd, 43)
    assert np.array_equal(got.m.view(u32), ref.m.view(u32)) and np.array_equal(got.v.view(u32), ref.v.view(u32))
    assert np.abs(got.p.view(np.int32).astype(np.int64) - ref.p.view(np.int32).astype(np.int64)).max() <= 1
    assert T.scalars is not None and T.scalars(6e-3, 0.9, 0.999, 1)[0] == 6e-3 / (1.0 - 0.9)      # the twin's hook was put back


def test_skip_step_returns_its_inputs():
    rng = np.random.default_rng(4)
    p, m, v, g = _state(rng, 64)
    ver, _ = G.scan(G.seeded(0.9, 0.999, 3), [np.array([np.nan], f32)])
    ver, found, _ = G.seal(ver, 6e-3, 0.9, 0.999, 1e-15, 0.0)
    assert found == 1.0 and G.guarded_adam_step(ver, p, m, v, [(g, 0, 64)], 64, 0.9, 0.999) is None


def test_verdict_structs_have_the_layout_of_the_header(tmp_path):
    """The three structs of the guarded step cross the C ABI by pointer (and the verdict is read by the host as raw words):
    the ctypes mirrors must have the size and member offsets a C compiler gives the header's declarations."""
    from cnc_amd import _lib
    members = {"cnc_step_verdict_t": _lib.StepVerdict, "cnc_verdict_scan_t": _lib.VerdictScan,
               "cnc_verdict_seal_t": _lib.VerdictSeal}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <stdint.h>', '#include "cnc_hip.h"', 'int main(void) {']
    for t, cls in members.items():
        lines.append(f'  printf("{t} size %zu\\n", sizeof({t}));')
        for n, _ in cls._fields_:
            lines.append(f'  printf("{t} {n} %zu\\n", offsetof({t}, {n}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    seen = 0
    for line in out.splitlines():
        t, name, value = line.split()
        cls = members[t]
        want = ctypes.sizeof(cls) if name == "size" else getattr(cls, name).offset
        assert int(value) == want, (t, name, int(value), want)
        seen += 1
    assert seen == sum(len(c._fields_) + 1 for c in members.values())
    assert ctypes.sizeof(_lib.StepVerdict) == 88 and _lib.StepVerdict.b1_pow.offset == 16
    assert _lib.CNC_VERDICT_MAX_TENSORS == len(_lib.VerdictScan().ptr) == 48


def test_mode_is_off_by_default_and_has_its_switches():
    from cnc_amd import train
    from cnc_amd.trainer import TrainConfig
    assert TrainConfig().guarded_step is False
    ap = train.build_parser()
    assert ap.parse_args([]).guarded_step is False and ap.parse_args(["--guarded-step"]).guarded_step is True
