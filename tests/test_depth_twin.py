"""CPU: the NumPy twin of depth supervision (tests/depth_twin.py) — the closed form by hand, the gradient against a
float64 finite difference, the validity rules, the offset case (the centred float32 form inside the derived bound, the
prefix form outside it) — and `cnc_amd.nerfacc.losses.depth_loss` on CPU tensors against the twin's float64 definition."""
import numpy as np
import pytest
import torch

import depth_twin as T

f32, f64 = np.float32, np.float64


def _ray(rng, n, lo=0.5, hi=6.0):
    edges = np.sort(rng.uniform(lo, hi, 2 * n)).astype(f32)
    return (rng.uniform(0, 1, n) ** 2).astype(f32), edges[0::2].copy(), edges[1::2].copy()


def test_closed_form_by_hand():
    # midpoints .5 and 2.5, target 2: e = -1.5, .5;  S1 = -.75 + .25 = -.5;  S2 = 1.125 + .125 = 1.25
    loss, grad, s1, s2 = T.direct64([.5, .5], [0., 2.], [1., 3.], 2.0, spread=1.0)
    assert (s1, s2) == (-0.5, 1.25) and loss == 0.25 + 1.25
    assert np.array_equal(grad, [2 * -0.5 * -1.5 + 2.25, 2 * -0.5 * 0.5 + 0.25])
    # three samples, spread 2.5, a target in front of all of them: e = 1, 2, 4 with w = .25, .5, .125
    loss, grad, s1, s2 = T.direct64([.25, .5, .125], [1.5, 2.5, 4.0], [2.5, 3.5, 6.0], 1.0, spread=2.5)
    assert s1 == 0.25 + 1.0 + 0.5 and s2 == 0.25 + 2.0 + 2.0
    assert loss == 1.75 ** 2 + 2.5 * 4.25
    assert np.array_equal(grad, [3.5 * 1 + 2.5 * 1, 3.5 * 2 + 2.5 * 4, 3.5 * 4 + 2.5 * 16])
    # spread 0: the expected-depth error alone; for an opaque ray (sum w = 1) it is (d - D)^2
    loss, _, _, _ = T.direct64([.5, .5], [0., 2.], [1., 3.], 2.0, spread=0.0)
    assert loss == (0.5 * 0.5 + 0.5 * 2.5 - 2.0) ** 2


@pytest.mark.parametrize("spread", [0.0, 1.0, 2.5])
def test_gradient_against_a_finite_difference(spread):
    rng = np.random.default_rng(3)
    w, t0, t1 = _ray(rng, 40)
    D = 3.1
    _, grad, _, _ = T.direct64(w, t0, t1, D, spread)
    w64, h = w.astype(f64), 1e-6
    for i in (0, 7, 39):
        # (the loss is quadratic in w: the central difference is exact up to rounding)
        up, dn = w64.copy(), w64.copy()
        up[i] += h
        dn[i] -= h
        e = 0.5 * (t0.astype(f64) + t1.astype(f64)) - f64(f32(D))
        L = lambda x: np.sum(x * e) ** 2 + spread * np.sum(x * e * e)          # noqa: E731
        assert abs((L(up) - L(dn)) / (2 * h) - grad[i]) <= 1e-8 * max(1.0, abs(grad[i]))


@pytest.mark.parametrize("D", [0.0, -1.0, np.nan, np.inf, -np.inf])
def test_no_measurement_is_exactly_zero(D):
    rng = np.random.default_rng(5)
    w, t0, t1 = _ray(rng, 33)
    loss, grad, s1, s2 = T.direct64(w, t0, t1, D)
    assert loss == 0.0 and s1 == 0.0 and s2 == 0.0 and not grad.any()
    l32, g32, s32 = T.kernel32(w, t0, t1, D, spread=2.5, upstream=np.nan)
    assert l32 == 0.0 and s32 == 0.0 and not np.signbit(g32).any() and not g32.any()
    assert T.bound(33, w, t0, t1, D) [1] == 0.0


def test_an_empty_ray_is_zero():
    z = np.zeros(0, f32)
    assert T.direct64(z, z, z, 2.0)[0] == 0.0 and T.kernel32(z, z, z, 2.0)[0] == 0.0


@pytest.mark.parametrize("S", [1, 31, 32, 33, 200])
@pytest.mark.parametrize("spread", [0.0, 1.0, 2.5])
def test_the_float32_restatement_is_within_the_bound(S, spread):
    rng = np.random.default_rng(S)
    w, t0, t1 = _ray(rng, S)
    for D in (float(t0[S // 2]), 0.25, float(0.5 * (t0[0] + t1[-1]))):
        want_l, want_g, want_s1, _ = T.direct64(w, t0, t1, D, spread)
        got_l, got_g, got_s1 = T.kernel32(w, t0, t1, D, spread, upstream=-0.75)
        b1, bl, bg = T.bound(S, w, t0, t1, D, spread, upstream=-0.75)
        assert T.ratio(got_s1, want_s1, b1) <= 1 and T.ratio(got_l, want_l, bl) <= 1
        assert T.ratio(got_g, -0.75 * want_g, bg) <= 1


@pytest.mark.parametrize("seed", range(20))
def test_offset_case_centred_inside_the_bound_and_prefix_outside(seed):
    """S = 64 samples of width 1e-3 within +-0.05 of D ~ 4096: the centred form stays inside the bound, the prefix form
    sum w m - D sum w is far outside it, on every seed."""
    w, t0, t1, D = T.offset_case(seed)
    want_l, want_g, want_s1, _ = T.direct64(w, t0, t1, D)
    got_l, got_g, got_s1 = T.kernel32(w, t0, t1, D)
    b1, bl, bg = T.bound(64, w, t0, t1, D)
    assert T.ratio(got_s1, want_s1, b1) <= 1 and T.ratio(got_l, want_l, bl) <= 1 and T.ratio(got_g, want_g, bg) <= 1
    outside = T.ratio(T.prefix32(w, t0, t1, D), want_s1, b1)
    print(f"seed {seed}: centred {T.ratio(got_s1, want_s1, b1):.3g} of the bound, prefix {outside:.3g}")
    assert outside > 1


# ------------------------------------------------------------------------------------- losses.depth_loss on CPU tensors
def _flat(rng, counts):
    parts = [_ray(rng, c) for c in counts]
    cat = lambda k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, f32)       # noqa: E731
    cnts = np.asarray(counts, np.int64)
    return cat(0), cat(1), cat(2), np.cumsum(cnts) - cnts, cnts


@pytest.mark.parametrize("spread", [0.0, 1.0, 2.5])
def test_depth_loss_float64_against_the_definition(spread):
    from cnc_amd.nerfacc.losses import depth_loss
    rng = np.random.default_rng(11)
    counts = [5, 0, 33, 1, 7, 12]
    w, t0, t1, starts, cnts = _flat(rng, counts)
    target = np.array([2.0, 1.0, 3.5, np.nan, 0.0, np.inf], f32)
    up = np.array([1.0, -2.0, 0.5, np.nan, 3.0, -1.0])
    wt = torch.from_numpy(w.astype(f64)).requires_grad_(True)
    tt = lambda a: torch.from_numpy(a.astype(f64))          # noqa: E731
    info = torch.from_numpy(np.stack([starts, cnts], -1))
    loss = depth_loss(wt, tt(t0), tt(t1), tt(target), packed_info=info, spread=spread)
    assert loss.dtype == torch.float64 and tuple(loss.shape) == (6,)
    loss.backward(torch.from_numpy(up))
    by_index = depth_loss(wt.detach(), tt(t0), tt(t1), tt(target), spread=spread, n_rays=6,
                          ray_indices=torch.arange(6).repeat_interleave(torch.from_numpy(cnts)))
    assert torch.equal(by_index, loss.detach())
    for r, (s, c) in enumerate(zip(starts, cnts)):
        seg = slice(int(s), int(s + c))
        want_l, want_g, _, _ = T.direct64(w[seg], t0[seg], t1[seg], target[r], spread)
        assert abs(loss[r].item() - want_l) <= 1e-12 * max(1.0, abs(want_l))
        got_g = wt.grad[seg].numpy()
        if not T.valid_target(target[r]):
            assert loss[r].item() == 0.0 and not got_g.any() and not np.signbit(got_g).any()       # NaN upstream: still +0
        else:
            assert np.all(np.abs(got_g - up[r] * want_g) <= 1e-12 * np.maximum(1.0, np.abs(up[r] * want_g)))


def test_depth_loss_batched_rows_and_float32_on_cpu():
    from cnc_amd.nerfacc.losses import depth_loss
    rng = np.random.default_rng(13)
    w, t0, t1, starts, cnts = _flat(rng, [9] * 6)
    target = np.array([2.0, 1.0, 3.5, -1.0, 0.0, 4.0], f32).reshape(2, 3)
    shape = (2, 3, 9)
    rows = depth_loss(torch.from_numpy(w.reshape(shape)), torch.from_numpy(t0.reshape(shape)), torch.from_numpy(t1.reshape(shape)),
                      torch.from_numpy(target), spread=2.5)
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (2, 3)
    for r in range(6):
        seg = slice(9 * r, 9 * r + 9)
        want_l, _, _, _ = T.direct64(w[seg], t0[seg], t1[seg], target.reshape(-1)[r], 2.5)
        assert abs(rows.reshape(-1)[r].item() - want_l) <= 1e-5 * max(1.0, abs(want_l))
    empty = depth_loss(torch.zeros(4, 0), torch.zeros(4, 0), torch.zeros(4, 0), torch.ones(4))
    assert tuple(empty.shape) == (4,) and not empty.any()
    with pytest.raises(AssertionError):
        depth_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(3))
    with pytest.raises(ValueError):
        depth_loss(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4), spread=-1.0)


def test_depth_loss_gradcheck():
    from cnc_amd.nerfacc.losses import depth_loss
    rng = np.random.default_rng(17)
    w, t0, t1, starts, cnts = _flat(rng, [4, 0, 6, 3])
    tt = lambda a: torch.from_numpy(a.astype(f64))          # noqa: E731
    info = torch.from_numpy(np.stack([starts, cnts], -1))
    target = torch.tensor([2.0, 1.0, 3.0, float("nan")], dtype=torch.float64)
    wt = tt(w).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: depth_loss(x, tt(t0), tt(t1), target, packed_info=info, spread=2.5), (wt,))
    rows = tt(w[:4].reshape(1, 4)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: depth_loss(x, tt(t0[:4]).reshape(1, 4), tt(t1[:4]).reshape(1, 4),
                                                         torch.tensor([2.5], dtype=torch.float64)), (rows,))
