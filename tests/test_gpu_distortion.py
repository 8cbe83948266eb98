"""GPU: the distortion kernels (cnc_amd/csrc/distortion.hip) against the float64 definition of the NumPy twin
(tests/distortion_twin.py) within the derived bound (2 S + 8) 2^-24 — the packed layout through the C ABI between
sentinel-filled guards, the offset case the prefix-difference form fails, the batched layout bit-equal to the packed one,
run-to-run bits, the composition with `rendering` under autograd, and host synchronisation."""
import numpy as np
import pytest
import torch

import distortion_twin as T
from guarded import Guarded, sentinel

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64
COUNTS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 200]
HOLE = 3          # slots between two rays that belong to no ray: poisoned inputs, sentinel outputs


class GuardedI64(Guarded):
    """tests/guarded.py's buffer for int64 host arrays (chunk_starts / chunk_cnts)."""

    def __init__(self, host, dev):
        super().__init__(np.ascontiguousarray(host, i64), dev)

    def tensor(self):
        return self.alloc[self.lo:self.lo + self.nbytes].view(torch.int64).view(self.shape)


def _rays(rng, counts, hole=0):
    """Flattened rays with the given counts, `hole` unowned slots behind each ray (NaN inputs): weights in [0, 1),
    intervals with gaps.  -> (w, t0, t1, starts, cnts, owned mask)."""
    cnts = np.asarray(counts, i64)
    starts = np.cumsum(cnts + hole) - (cnts + hole)
    N = int((cnts + hole).sum())
    w, t0, t1 = (np.full(N, np.nan, f32) for _ in range(3))
    owned = np.zeros(N, bool)
    for s, c in zip(starts, cnts):
        if c:
            w[s:s + c] = rng.uniform(0, 1, c).astype(f32) ** 2
            t0[s:s + c], t1[s:s + c] = T.gapped_intervals(rng, int(c))
            owned[s:s + c] = True
    return w, t0, t1, starts, cnts, owned


def _upstream(rng, n):
    up = rng.normal(size=n).astype(f32)
    up[::4] = 0.0
    up[1::4] = -np.abs(up[1::4]) - 0.5
    return up


def _check_against_twin(loss, g_w, w, t0, t1, starts, cnts, up):
    """-> the largest error as a fraction of its bound."""
    ratio = 0.0
    for r, (s, c) in enumerate(zip(starts, cnts)):
        seg = slice(int(s), int(s + c))
        want_l, want_g = T.direct64(w[seg], t0[seg], t1[seg])
        want_g = want_g * f64(up[r])
        print(f"ray {r} S={c}: loss {T.worst(loss[r], want_l):.3g} grad {T.worst(g_w[seg], want_g):.3g} "
              f"bound {T.bound(c):.3g}")
        assert T.within(loss[r], want_l, c), (r, c, loss[r], want_l)
        assert T.within(g_w[seg], want_g, c), (r, c, T.worst(g_w[seg], want_g))
        if c == 0:
            assert loss[r] == 0.0
        else:
            ratio = max(ratio, T.worst(loss[r], want_l) / T.bound(c), T.worst(g_w[seg], want_g) / T.bound(c))
    print(f"largest |got - direct64| / bound(S): {ratio:.3g}")
    return ratio


@pytest.mark.parametrize("counts", [
    pytest.param([33, 0, 200, 1, 64, 31, 65, 2, 63, 32], id="ten_shuffled"),
    pytest.param([200, 32, 0, 65, 1, 63, 33, 2, 64, 31, 100], id="odd_n_rays"),
    pytest.param([200], id="one_ray"),
    pytest.param([0], id="one_empty_ray"),
])
def test_packed_layout_through_the_c_abi(cuda, counts):
    assert set(COUNTS) <= set(counts) or len(counts) == 1
    _packed_through_the_c_abi(cuda, counts)


# k_distortion_bwd keeps kKeepTiles = 32 tiles (1024 samples) of B per ray in LDS; a longer ray is walked in stretches of
# 1024 samples, front to back, the A recurrence carried from one stretch to the next.  The two rays of a wave (2k, 2k + 1)
# share the loop: the stretch's end and both sides of it, a long ray next to a short one, exactly two stretches, three
# stretches next to an empty ray and next to a one-sample ray.
STRETCH_PAIRS = [(1023, 1024), (1025, 5), (33, 2049), (2048, 2048), (0, 3100), (3100, 1)]


def test_backward_stretches_of_rays_over_1024_samples(cuda):
    """Largest |got - direct64| / bound(S) measured on the MI355X: 0.12 over all twelve rays (on a short one); on the rays
    of more than one stretch 0.0036 (S = 1025: 4.4e-7 of a bound of 1.2e-4), 0.0024 at S = 3100."""
    _packed_through_the_c_abi(cuda, [c for pair in STRETCH_PAIRS for c in pair])


def _packed_through_the_c_abi(cuda, counts):
    from cnc_amd import _lib
    rng = np.random.default_rng(len(counts))
    w, t0, t1, starts, cnts, owned = _rays(rng, counts, hole=HOLE)
    n = len(counts)
    up = _upstream(rng, n)
    if n == 1:
        up[0] = -0.75
    assert all(up[r] != 0 for r, c in enumerate(counts) if c > 1024), "a ray of several stretches needs a gradient to show"
    gs, gc = GuardedI64(starts, cuda), GuardedI64(cnts, cuda)
    gw, g0, g1, gu = (Guarded(a, cuda) for a in (w, t0, t1, up))
    loss, g_w = Guarded.empty((n,), f32, cuda), Guarded.empty(w.shape, f32, cuda)
    L, st = _lib.lib(), _lib.stream(cuda)
    _lib.check(L.cnc_distortion_forward(gs.ptr, gc.ptr, 0, g0.ptr, g1.ptr, gw.ptr, loss.ptr, n, st), "forward")
    _lib.check(L.cnc_distortion_backward(gs.ptr, gc.ptr, 0, g0.ptr, g1.ptr, gw.ptr, gu.ptr, g_w.ptr, n, st), "backward")
    torch.cuda.synchronize()
    for g in (gs, gc, gw, g0, g1, gu, loss, g_w):
        assert g.intact()
    got_l, got_g = loss.get(), g_w.get()
    # what belongs to no ray — the holes, an empty ray's among them — was neither read (NaN inputs) nor written
    assert np.all(got_g[~owned].view(np.uint32) == sentinel(np.uint32))
    assert np.all(np.isfinite(got_l)) and np.all(np.isfinite(got_g[owned]))
    _check_against_twin(got_l, got_g, w, t0, t1, starts, cnts, up)


def test_c_abi_refuses_half_a_layout(cuda):
    from cnc_amd import _lib
    x = torch.zeros(8, device=cuda)
    s = torch.zeros(1, dtype=torch.int64, device=cuda)
    L, st = _lib.lib(), _lib.stream(cuda)
    p = x.data_ptr()
    assert L.cnc_distortion_forward(s.data_ptr(), None, 0, p, p, p, p, 1, st) != 0
    assert L.cnc_distortion_forward(None, None, -1, p, p, p, p, 1, st) != 0
    assert L.cnc_distortion_backward(None, s.data_ptr(), 0, p, p, p, p, p, 1, st) != 0
    assert L.cnc_distortion_forward(None, None, 4, p, p, p, None, 1, st) != 0


def _api(cuda, w, t0, t1, up, **layout):
    """losses.distortion on the device -> (loss, dL/dw) as NumPy, L = sum(loss * up)."""
    from cnc_amd.nerfacc.losses import distortion
    wt = torch.from_numpy(w).to(cuda).requires_grad_(True)
    loss = distortion(wt, torch.from_numpy(t0).to(cuda), torch.from_numpy(t1).to(cuda), **layout)
    (loss * torch.from_numpy(up).to(cuda).view(loss.shape)).sum().backward()
    return loss.detach().cpu().numpy(), wt.grad.cpu().numpy()


def test_offset_case(cuda):
    """A thin surface at t = 4096: exactly representable inputs, the case the prefix-difference formulation fails."""
    rng = np.random.default_rng(21)
    w, t0, t1 = T.offset_case(rng, 64)
    want_l, want_g = T.direct64(w, t0, t1)
    assert not T.within(T.prefix_difference32(w, t0, t1), want_l, 64)
    up = np.array([1.0], f32)
    for layout in (dict(packed_info=torch.tensor([[0, 64]], device=cuda)), None):
        if layout is None:
            got_l, got_g = _api(cuda, w[None], t0[None], t1[None], up)
        else:
            got_l, got_g = _api(cuda, w, t0, t1, up, **layout)
        print("offset:", T.worst(got_l, want_l), T.worst(got_g.reshape(-1), want_g), "bound", T.bound(64))
        assert T.within(got_l.reshape(-1)[0], want_l, 64)
        assert T.within(got_g.reshape(-1), want_g, 64)


@pytest.mark.parametrize("S", [1, 32, 33, 97])
def test_batched_layout_equals_the_packed_call_bit_for_bit(cuda, S):
    rng = np.random.default_rng(S)
    lead = (3, 5)
    n = lead[0] * lead[1]
    w, t0, t1, starts, cnts, _ = _rays(rng, [S] * n)
    up = _upstream(rng, n)
    shape = lead + (S,)
    bl, bg = _api(cuda, w.reshape(shape), t0.reshape(shape), t1.reshape(shape), up.reshape(lead))
    assert bl.shape == lead and bg.shape == shape
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    pl, pg = _api(cuda, w, t0, t1, up, packed_info=info)
    assert np.array_equal(bl.reshape(-1).view(np.uint32), pl.view(np.uint32))
    assert np.array_equal(bg.reshape(-1).view(np.uint32), pg.view(np.uint32))
    rl, rg = _api(cuda, w, t0, t1, up, ray_indices=torch.arange(n, device=cuda).repeat_interleave(S), n_rays=n)
    assert np.array_equal(rl.view(np.uint32), pl.view(np.uint32)) and np.array_equal(rg.view(np.uint32), pg.view(np.uint32))
    _check_against_twin(pl, pg, w, t0, t1, starts, cnts, up)


def test_two_calls_give_equal_bits(cuda):
    rng = np.random.default_rng(31)
    w, t0, t1, starts, cnts, _ = _rays(rng, [33, 0, 200, 1, 64, 31, 65, 2, 63, 32, 1500])
    up = _upstream(rng, len(cnts))
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    l1, g1 = _api(cuda, w, t0, t1, up, packed_info=info)
    l2, g2 = _api(cuda, w, t0, t1, up, packed_info=info)
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32))
    # (the 1500-sample ray takes the backward's second stretch: the same bound holds)
    _check_against_twin(l1, g1, w, t0, t1, starts, cnts, up)


def test_autograd_composition_with_rendering_is_exact(cuda):
    """distortion(extras["weights"]).sum() behind rendering(): sigmas.grad is, bit for bit, what volrend_backward gives for
    grad_weights = cnc_distortion_backward's output."""
    from cnc_amd.backends import volrend_backend as K
    from cnc_amd.nerfacc.losses import distortion
    from cnc_amd.nerfacc.volrend import rendering
    rng = np.random.default_rng(41)
    counts = rng.integers(0, 70, 64)
    counts[5] = 0
    w_, t0, t1, starts, cnts, _ = _rays(rng, counts)
    N = int(cnts.sum())
    ts, te = torch.from_numpy(t0).to(cuda), torch.from_numpy(t1).to(cuda)
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    ray_indices = torch.arange(64, device=cuda).repeat_interleave(torch.from_numpy(cnts).to(cuda))
    sigmas = torch.from_numpy((rng.uniform(size=N) ** 3 * 20).astype(f32)).to(cuda).requires_grad_(True)
    rgbs = torch.from_numpy(rng.uniform(size=(N, 3)).astype(f32)).to(cuda)
    _, _, _, extras = rendering(ts, te, ray_indices, n_rays=64, rgb_sigma_fn=lambda a, b, c: (rgbs, sigmas, None),
                                packed_info=info)
    distortion(extras["weights"], ts, te, packed_info=info).sum().backward()
    s, c = K.split_packed(info)
    with torch.no_grad():
        weights, trans, alphas, _, opacity, depth = K.volrend_forward(s, c, ts, te, sigmas.detach(), rgbs, finalize=True)
        g_w = K.distortion_backward(s, c, ts, te, weights, torch.ones(64, device=cuda))
        want, _ = K.volrend_backward(s, c, ts, te, rgbs, weights, trans, alphas, opacity=opacity, depth=depth,
                                     grad_weights=g_w, finalize=True)
    assert torch.equal(extras["weights"], weights)
    assert sigmas.grad.abs().max().item() > 0
    assert torch.equal(sigmas.grad.view(torch.int32), want.view(torch.int32))


def test_batched_calls_do_not_synchronise(cuda):
    from cnc_amd.nerfacc.losses import distortion
    rng = np.random.default_rng(51)
    w, t0, t1, _, _, _ = _rays(rng, [48] * 64)
    dev = lambda a: torch.from_numpy(a.reshape(64, 48)).to(cuda)       # noqa: E731
    wt, a, b = dev(w).requires_grad_(True), dev(t0), dev(t1)
    distortion(wt, a, b).sum().backward()            # warm up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        distortion(wt, a, b).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(0)
