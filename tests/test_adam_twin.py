"""tests/adam_twin.py (the NumPy twin that tests/test_gpu_table_adam_matrix.py holds cnc_table_adam to, bit for bit)
kept honest without a GPU: against the same update in float64 throughout, under the componentwise bound derived in the
twin's docstring, and against torch.optim.Adam on float64 parameters over six steps under the same bound carried from
step to step."""
import numpy as np
import pytest
import torch

import adam_twin as T

f32, f64 = np.float32, np.float64
_RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_margins():
    yield
    print("\nadam twin, largest |twin - float64| / bound: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_RATIOS.items())))


def _within(group, got, ref, bound):
    err = np.abs(got.astype(f64) - ref)
    ok = bound > 0
    assert np.all(err[~ok] == 0), group
    r = float((err[ok] / bound[ok]).max()) if ok.any() else 0.0
    _RATIOS[group] = max(_RATIOS.get(group, 0.0), r)
    assert r <= 1.0, (group, r)


def _mixed(rng, n, lo_exp, hi_exp):
    """Signed values whose magnitudes spread over 10^lo_exp .. 10^hi_exp."""
    return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo_exp, hi_exp, n)).astype(f32)


def _pieces(rng, n):
    g = [_mixed(rng, n, -6, 3) for _ in range(3)]
    g[0][rng.integers(0, 7, n) == 0] = 0.0
    lo, hi = n // 4, n // 2 + 3
    return [(g[0], 0, n), None, (g[1][lo:hi], lo, hi), (g[2][: n // 3], 0, n // 3)]


def test_gradient_sum_follows_the_slots():
    n = 12
    a, b, c = (np.arange(n, dtype=f32) + k for k in (1, 100, 1000))
    g = T.grad_sum([None, (a[4:8], 4, 8), (b, 0, n), (c[:2], 10, 12)], n)
    want = b.copy()
    want[4:8] = a[4:8] + b[4:8]
    want[10:12] = b[10:12] + c[:2]
    assert np.array_equal(g, want)
    assert np.array_equal(T.grad_sum([None] * 4, 5), np.zeros(5, f32))
    z = T.grad_sum([(np.array([-0.0], f32), 1, 2)], 3)                    # the first piece is copied: -0.0 stays -0.0
    assert np.signbit(z[1]) and not np.signbit(z[0])
    big = f32(2.0 ** 24)                                                  # ((g0 + g1) + g2), not g0 + (g1 + g2)
    one = np.array([1.0], f32)
    assert T.grad_sum([(np.array([big]), 0, 1), (one, 0, 1), (one, 0, 1)], 1)[0] == big
    assert T.grad_sum([(one, 0, 1), (one, 0, 1), (np.array([big]), 0, 1)], 1)[0] == big + f32(2.0)


def test_sign_plane_and_clip_count():
    p = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2)), np.nan, -np.inf], f32)
    bits, clipped = T.sign_plane(p)
    assert bits.tolist() == [0b00010111] and clipped == 4
    assert T.sign_plane(p[:5])[0] is None


@pytest.mark.parametrize("hyper", [(0.9, 0.999, 1e-15, 0.0), (0.9, 0.999, 1e-15, 2e-6), (0.5, 0.9, 1e-8, 0.0), (0.5, 0.9, 1e-8, 1e-2)],
                         ids=["trainer", "trainer_decay", "other", "other_decay"])
@pytest.mark.parametrize("step", [1, 6, 1000, 20000])
def test_one_step_against_float64_from_the_same_state(hyper, step):
    b1, b2, eps, wd = hyper
    rng = np.random.default_rng(step)
    n = 1 << 16
    p, m, v = _mixed(rng, n, -4, 0), _mixed(rng, n, -6, 3), np.abs(_mixed(rng, n, -12, 6))
    m[::11], v[::13] = 0.0, 0.0
    pcs = _pieces(rng, n)
    lr = 6e-3
    before = T.Step(p, m, v, None, 0, None, None)
    got = T.adam_step(p, m, v, pcs, n, lr, b1, b2, eps, wd, step)
    p64, m64, v64 = T.float64_step(p, m, v, T.grad_sum(pcs, n), lr, b1, b2, eps, wd, step)
    e_p, e_m, e_v = T.error_bound(before, got, lr, b1, b2, eps, wd, step)
    _within("one step m", got.m, m64, e_m)
    _within("one step v", got.v, v64, e_v)
    _within("one step p", got.p, p64, e_p)
    # the bound is a rounding bound, not a licence: a few units of the largest term involved
    assert np.all(e_m <= 4 * T.U * (np.abs(m64) + np.abs(got.g.astype(f64)) + np.abs(m.astype(f64))) + 1e-300)


@pytest.mark.parametrize("wd", [0.0, 2e-6], ids=["no_decay", "decay"])
def test_six_steps_against_the_library_adam_in_float64(wd):
    rng = np.random.default_rng(5)
    n = 1 << 14
    b1, b2, eps = 0.9, 0.999, 1e-15
    p = _mixed(rng, n, -4, 0)
    m, v = np.zeros(n, f32), np.zeros(n, f32)
    ref = torch.nn.Parameter(torch.tensor(p.astype(f64)))
    opt = torch.optim.Adam([ref], lr=6e-3, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    e_p = e_m = e_v = 0.0
    for step in range(1, 7):
        lr = opt.param_groups[0]["lr"] = 6e-3 * (0.5 + 0.1 * step)
        pcs = _pieces(rng, n)
        before = T.Step(p, m, v, None, 0, None, None)
        got = T.adam_step(p, m, v, pcs, n, lr, b1, b2, eps, wd, step)
        e_p, e_m, e_v = T.error_bound(before, got, lr, b1, b2, eps, wd, step, e_p, e_m, e_v)
        ref.grad = torch.tensor(T.grad_sum(pcs, n).astype(f64))
        opt.step()
        st = opt.state[ref]
        _within(f"six steps m", got.m, st["exp_avg"].numpy(), e_m)
        _within(f"six steps v", got.v, st["exp_avg_sq"].numpy(), e_v)
        _within(f"six steps p", got.p, ref.detach().numpy(), e_p)
        p, m, v = got.p, got.m, got.v
    assert float(st["step"]) == 6


def test_flushing_variant_differs_only_on_subnormals():
    rng = np.random.default_rng(9)
    n = 4096
    p, m, v = _mixed(rng, n, -4, 0), _mixed(rng, n, -6, 3), np.abs(_mixed(rng, n, -12, 6))
    pcs = _pieces(rng, n)
    a = T.adam_step(p, m, v, pcs, n, 6e-3, 0.9, 0.999, 1e-15, 2e-6, 3)
    b = T.adam_step_flushing(p, m, v, pcs, n, 6e-3, 0.9, 0.999, 1e-15, 2e-6, 3)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    m2 = _mixed(rng, n, -38.5, -37.5)
    g2 = [(m2 * f32(0.9), 0, n)]
    a = T.adam_step(p, m2, np.zeros(n, f32), g2, n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 3)
    b = T.adam_step_flushing(p, m2, np.zeros(n, f32), g2, n, 6e-3, 0.9, 0.999, 1e-15, 0.0, 3)
    assert not np.array_equal(a.m.view(np.uint32), b.m.view(np.uint32))
