"""GPU: the depth-loss kernels (cnc_amd/csrc/depth_loss.hip) against the float64 definition of the NumPy twin
(tests/depth_twin.py) within the bound derived there — the packed layout through the C ABI between sentinel-filled guards
with NaN in the slots no ray owns, targets with and without a measurement, an upstream gradient with zeros, negatives and a
NaN, three values of `spread`; the offset case; the batched layout bit-equal to the packed one; run-to-run bits; autograd
bit-equal to the C ABI; the composition with `rendering`; host synchronisation."""
import numpy as np
import pytest
import torch

import depth_twin as T
from guarded import Guarded, sentinel
from test_gpu_distortion import GuardedI64

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
HOLE = 3          # slots between two rays that belong to no ray: poisoned inputs, sentinel outputs
TEN = [33, 0, 200, 1, 64, 31, 65, 2, 63, 32]


def _rays(rng, counts, hole=0):
    """Flattened rays with the given counts, `hole` unowned slots behind each ray (NaN inputs): weights in [0, 1), intervals
    with gaps in [0.5, 6).  -> (w, t0, t1, starts, cnts, owned mask)."""
    cnts = np.asarray(counts, i64)
    starts = np.cumsum(cnts + hole) - (cnts + hole)
    N = int((cnts + hole).sum())
    w, t0, t1 = (np.full(N, np.nan, f32) for _ in range(3))
    owned = np.zeros(N, bool)
    for s, c in zip(starts, cnts):
        if c:
            w[s:s + c] = rng.uniform(0, 1, c).astype(f32) ** 2
            edges = np.sort(rng.uniform(0.5, 6.0, 2 * c)).astype(f32)
            t0[s:s + c], t1[s:s + c] = edges[0::2], edges[1::2]
            owned[s:s + c] = True
    return w, t0, t1, starts, cnts, owned


def _targets(t0, t1, starts, cnts, first=0):
    """One per ray, cycling: a distance inside the ray, one in front of all its samples, 0, NaN, +inf, -1."""
    out = np.zeros(len(cnts), f32)
    for r, (s, c) in enumerate(zip(starts, cnts)):
        kind = (r + first) % 6
        inside = 0.5 * (t0[s + c // 2] + t1[s + c // 2]) if c else 3.0
        out[r] = (inside, 0.25, 0.0, np.nan, np.inf, -1.0)[kind]
    return out


def _upstream(rng, target):
    up = rng.normal(size=len(target)).astype(f32)
    up[::4] = 0.0
    up[1::4] = -np.abs(up[1::4]) - 0.5
    none = [r for r, D in enumerate(target) if not T.valid_target(D)]
    if none:
        up[none[0]] = np.nan          # upstream of a ray without a measurement: must not reach its samples
    return up


def _check_against_twin(loss, g_w, w, t0, t1, starts, cnts, target, up, spread):
    """-> the largest error as a fraction of its bound."""
    worst = 0.0
    for r, (s, c) in enumerate(zip(starts, cnts)):
        seg = slice(int(s), int(s + c))
        want_l, want_g, _, _ = T.direct64(w[seg], t0[seg], t1[seg], target[r], spread)
        if not T.valid_target(target[r]) or c == 0:
            assert loss[r].view(np.uint32) == 0, (r, loss[r])                      # exactly +0
            assert not g_w[seg].view(np.uint32).any(), (r, g_w[seg])              # every one of them +0, NaN upstream or not
            continue
        _, bl, bg = T.bound(int(c), w[seg], t0[seg], t1[seg], target[r], spread, up[r])
        rl, rg = T.ratio(loss[r], want_l, bl), T.ratio(g_w[seg], f64(up[r]) * want_g, bg)
        print(f"ray {r} S={c} D={target[r]:.4g}: loss {rl:.3g} grad {rg:.3g} of the bound")
        assert rl <= 1 and rg <= 1, (r, c, rl, rg)
        worst = max(worst, rl, rg)
    print(f"largest |got - direct64| / bound: {worst:.3g}")
    return worst


def _c_abi(cuda, w, t0, t1, starts, cnts, target, up, spread):
    from cnc_amd import _lib
    n = len(cnts)
    gs, gc = GuardedI64(starts, cuda), GuardedI64(cnts, cuda)
    gw, g0, g1, gt, gu = (Guarded(a, cuda) for a in (w, t0, t1, target, up))
    loss, s1, g_w = Guarded.empty((n,), f32, cuda), Guarded.empty((n,), f32, cuda), Guarded.empty(w.shape, f32, cuda)
    L, st = _lib.lib(), _lib.stream(cuda)
    _lib.check(L.cnc_depth_loss_forward(gs.ptr, gc.ptr, 0, g0.ptr, g1.ptr, gw.ptr, gt.ptr, spread, loss.ptr, s1.ptr, n, st),
               "forward")
    _lib.check(L.cnc_depth_loss_backward(gs.ptr, gc.ptr, 0, g0.ptr, g1.ptr, gt.ptr, spread, s1.ptr, gu.ptr, g_w.ptr, n, st),
               "backward")
    torch.cuda.synchronize()
    for g in (gs, gc, gw, g0, g1, gt, gu, loss, s1, g_w):
        assert g.intact()
    return loss.get(), s1.get(), g_w.get()


@pytest.mark.parametrize("spread", [0.0, 1.0, 2.5])
@pytest.mark.parametrize("counts", [
    pytest.param(TEN, id="ten_shuffled"),
    pytest.param(TEN + [100], id="odd_n_rays"),
    pytest.param([200], id="one_ray"),
    pytest.param([0], id="one_empty_ray"),
    pytest.param([0, 2049], id="long_next_to_empty"),
])
def test_packed_layout_through_the_c_abi(cuda, counts, spread):
    """Largest |got - direct64| / bound measured on the MI355X: 0.21 over the ten- and eleven-ray cases (all six shifts of
    the targets, the three spreads), 0.051 on the ray alone, 0.010 on the 2049-sample ray (65 tiles); 0.25 over the batched
    rows of the test below, 0.16 on the offset case."""
    rng = np.random.default_rng(len(counts))
    w, t0, t1, starts, cnts, owned = _rays(rng, counts, hole=HOLE)
    # every shift of the cycle, so that every ray meets every kind of target; a ray alone, and the long ray of the pair, get
    # the measurement inside the ray
    for first in (range(6) if len(counts) > 2 else [5 if len(counts) == 2 else 0]):
        target = _targets(t0, t1, starts, cnts, first)
        up = _upstream(rng, target)
        if len(counts) <= 2:
            up[-1] = -0.75
        _one_packed_call(cuda, w, t0, t1, starts, cnts, owned, target, up, spread)


def _one_packed_call(cuda, w, t0, t1, starts, cnts, owned, target, up, spread):
    got_l, got_s1, got_g = _c_abi(cuda, w, t0, t1, starts, cnts, target, up, spread)
    # what belongs to no ray — the holes, an empty ray's among them — was neither read (NaN inputs) nor written
    assert np.all(got_g[~owned].view(np.uint32) == sentinel(np.uint32))
    assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_g[owned])) and np.all(np.isfinite(got_s1))
    _check_against_twin(got_l, got_g, w, t0, t1, starts, cnts, target, up, spread)
    for r, (s, c) in enumerate(zip(starts, cnts)):
        want = T.direct64(w[s:s + c], t0[s:s + c], t1[s:s + c], target[r], spread)[2]
        assert T.ratio(got_s1[r], want, T.bound(int(c), w[s:s + c], t0[s:s + c], t1[s:s + c], target[r])[0]) <= 1


def test_c_abi_refuses_half_a_layout(cuda):
    from cnc_amd import _lib
    x = torch.zeros(8, device=cuda)
    s = torch.zeros(1, dtype=torch.int64, device=cuda)
    L, st = _lib.lib(), _lib.stream(cuda)
    p = x.data_ptr()
    assert L.cnc_depth_loss_forward(s.data_ptr(), None, 0, p, p, p, p, 1.0, p, p, 1, st) != 0
    assert L.cnc_depth_loss_forward(None, None, -1, p, p, p, p, 1.0, p, p, 1, st) != 0
    assert L.cnc_depth_loss_forward(None, None, 4, p, p, p, None, 1.0, p, p, 1, st) != 0
    assert L.cnc_depth_loss_backward(None, s.data_ptr(), 0, p, p, p, 1.0, p, p, p, 1, st) != 0
    assert L.cnc_depth_loss_backward(None, None, 4, p, p, p, 1.0, None, p, p, 1, st) != 0


def _api(cuda, w, t0, t1, target, up, spread=1.0, **layout):
    """losses.depth_loss on the device -> (loss, dL/dw) as NumPy, L = sum(loss * up)."""
    from cnc_amd.nerfacc.losses import depth_loss
    wt = torch.from_numpy(w).to(cuda).requires_grad_(True)
    loss = depth_loss(wt, torch.from_numpy(t0).to(cuda), torch.from_numpy(t1).to(cuda), torch.from_numpy(target).to(cuda),
                      spread=spread, **layout)
    loss.backward(torch.from_numpy(up).to(cuda).view(loss.shape))
    return loss.detach().cpu().numpy(), wt.grad.cpu().numpy()


def test_offset_case(cuda):
    """A thin surface at t ~ 4096, the case the prefix form fails (tests/test_depth_twin.py), in both layouts."""
    for seed in (0, 19):
        w, t0, t1, D = T.offset_case(seed)
        want_l, want_g, want_s1, _ = T.direct64(w, t0, t1, D)
        b1, bl, bg = T.bound(64, w, t0, t1, D)
        assert T.ratio(T.prefix32(w, t0, t1, D), want_s1, b1) > 1
        target, up = np.array([D], f32), np.array([1.0], f32)
        for layout in (dict(packed_info=torch.tensor([[0, 64]], device=cuda)), None):
            if layout is None:
                got_l, got_g = _api(cuda, w[None], t0[None], t1[None], target, up)
            else:
                got_l, got_g = _api(cuda, w, t0, t1, target, up, **layout)
            rl, rg = T.ratio(got_l.reshape(-1)[0], want_l, bl), T.ratio(got_g.reshape(-1), want_g, bg)
            print(f"offset seed {seed}: loss {rl:.3g} grad {rg:.3g} of the bound")
            assert rl <= 1 and rg <= 1


@pytest.mark.parametrize("S", [1, 32, 33, 97])
def test_batched_layout_equals_the_packed_call_bit_for_bit(cuda, S):
    rng = np.random.default_rng(S)
    lead = (3, 5)
    n = lead[0] * lead[1]
    w, t0, t1, starts, cnts, _ = _rays(rng, [S] * n)
    target = _targets(t0, t1, starts, cnts)
    up = _upstream(rng, target)
    shape = lead + (S,)
    bl, bg = _api(cuda, w.reshape(shape), t0.reshape(shape), t1.reshape(shape), target.reshape(lead), up.reshape(lead), 2.5)
    assert bl.shape == lead and bg.shape == shape
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    pl, pg = _api(cuda, w, t0, t1, target, up, 2.5, packed_info=info)
    assert np.array_equal(bl.reshape(-1).view(np.uint32), pl.view(np.uint32))
    assert np.array_equal(bg.reshape(-1).view(np.uint32), pg.view(np.uint32))
    rl, rg = _api(cuda, w, t0, t1, target, up, 2.5, ray_indices=torch.arange(n, device=cuda).repeat_interleave(S), n_rays=n)
    assert np.array_equal(rl.view(np.uint32), pl.view(np.uint32)) and np.array_equal(rg.view(np.uint32), pg.view(np.uint32))
    _check_against_twin(pl, pg, w, t0, t1, starts, cnts, target, up, 2.5)


def test_two_calls_give_equal_bits_and_autograd_equals_the_c_abi(cuda):
    rng = np.random.default_rng(31)
    w, t0, t1, starts, cnts, _ = _rays(rng, TEN + [1500])
    target = _targets(t0, t1, starts, cnts)
    up = _upstream(rng, target)
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    l1, g1 = _api(cuda, w, t0, t1, target, up, 2.5, packed_info=info)
    l2, g2 = _api(cuda, w, t0, t1, target, up, 2.5, packed_info=info)
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    cl, _, cg = _c_abi(cuda, w, t0, t1, starts, cnts, target, up, 2.5)
    assert np.array_equal(l1.view(np.uint32), cl.view(np.uint32)) and np.array_equal(g1.view(np.uint32), cg.view(np.uint32))
    _check_against_twin(l1, g1, w, t0, t1, starts, cnts, target, up, 2.5)


def test_it_composes_with_rendering(cuda):
    """depth_loss(extras["weights"]).sum() behind rendering(): sigmas.grad is finite and not zero, and bit for bit what
    volrend_backward gives for grad_weights = cnc_depth_loss_backward's output."""
    from cnc_amd.backends import volrend_backend as K
    from cnc_amd.nerfacc.losses import depth_loss
    from cnc_amd.nerfacc.volrend import rendering
    rng = np.random.default_rng(41)
    counts = rng.integers(0, 70, 64)
    counts[5] = 0
    _, t0, t1, starts, cnts, _ = _rays(rng, counts)
    N = int(cnts.sum())
    target = torch.from_numpy(_targets(t0, t1, starts, cnts)).to(cuda)
    ts, te = torch.from_numpy(t0).to(cuda), torch.from_numpy(t1).to(cuda)
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    ray_indices = torch.arange(64, device=cuda).repeat_interleave(torch.from_numpy(cnts).to(cuda))
    sigmas = torch.from_numpy((rng.uniform(size=N) ** 3 * 20).astype(f32)).to(cuda).requires_grad_(True)
    rgbs = torch.from_numpy(rng.uniform(size=(N, 3)).astype(f32)).to(cuda)
    _, _, _, extras = rendering(ts, te, ray_indices, n_rays=64, rgb_sigma_fn=lambda a, b, c: (rgbs, sigmas, None),
                                packed_info=info)
    depth_loss(extras["weights"], ts, te, target, packed_info=info, spread=1.0).sum().backward()
    assert bool(torch.isfinite(sigmas.grad).all()) and sigmas.grad.abs().max().item() > 0
    s, c = K.split_packed(info)
    with torch.no_grad():
        weights, trans, alphas, _, opacity, depth = K.volrend_forward(s, c, ts, te, sigmas.detach(), rgbs, finalize=True)
        _, s1 = K.depth_loss_forward(s, c, ts, te, weights, target, 1.0)
        g_w = K.depth_loss_backward(s, c, ts, te, weights, target, 1.0, s1, torch.ones(64, device=cuda))
        want, _ = K.volrend_backward(s, c, ts, te, rgbs, weights, trans, alphas, opacity=opacity, depth=depth,
                                     grad_weights=g_w, finalize=True)
    assert torch.equal(sigmas.grad.view(torch.int32), want.view(torch.int32))


def test_batched_calls_do_not_synchronise(cuda):
    from cnc_amd.nerfacc.losses import depth_loss
    rng = np.random.default_rng(51)
    w, t0, t1, _, _, _ = _rays(rng, [48] * 64)
    dev = lambda a: torch.from_numpy(a.reshape(64, 48)).to(cuda)       # noqa: E731
    wt, a, b = dev(w).requires_grad_(True), dev(t0), dev(t1)
    target = torch.full((64,), 3.0, device=cuda)
    depth_loss(wt, a, b, target).sum().backward()            # warm up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        depth_loss(wt, a, b, target).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
