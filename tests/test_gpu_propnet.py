"""GPU: the proposal-network route end to end — PropNetEstimator sampling on an analytic density, training a tiny
proposal network with update_every_n_steps, render_image_with_propnet against a dense uniform render, and the
names the reference's examples import after install_dropins()."""
import math

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu


def _slab_fn(lo, hi, sigma=3.0):
    """Density `sigma` for t in [lo, hi] of each ray ((n_rays,) bounds), 0 elsewhere; at interval midpoints."""
    def fn(t_starts, t_ends):
        mid = (t_starts + t_ends) / 2
        inside = (mid >= lo[:, None]) & (mid <= hi[:, None])
        return torch.where(inside, torch.full_like(mid, sigma), torch.zeros_like(mid))
    return fn


@pytest.mark.parametrize("sampling_type", ["uniform", "lindisp"])
def test_samples_gather_in_the_dense_slab(cuda, sampling_type):
    from cnc_amd.nerfacc import PropNetEstimator
    n_rays, near, far = 512, 1.0, 10.0
    g = torch.Generator(device="cpu").manual_seed(0)
    lo = (2.0 + 5.0 * torch.rand(n_rays, generator=g)).to(cuda)
    hi = lo + 2.5
    est = PropNetEstimator().to(cuda)
    fn = _slab_fn(lo, hi)
    t0, t1 = est.sampling([fn, fn], [64, 32], 16, n_rays=n_rays, near_plane=near, far_plane=far,
                          sampling_type=sampling_type)
    assert t0.shape == (n_rays, 16) and t1.shape == (n_rays, 16)
    assert torch.equal(t0[:, 1:], t1[:, :-1])
    assert (t1 >= t0).all()
    tol = 1e-5 * far
    assert (t0 >= near - tol).all() and (t1 <= far + tol).all()
    mid = (t0 + t1) / 2
    inside = ((mid >= lo[:, None]) & (mid <= hi[:, None])).float().mean().item()
    assert inside >= 0.9, inside
    assert est.prop_cache == []


class _Fourier(nn.Module):
    """A tiny proposal network: Fourier features of the normalised distance -> nn.Linear -> softplus."""

    def __init__(self, near, far, n_freq=8):
        super().__init__()
        self.near, self.far = near, far
        self.register_buffer("freqs", 2.0 ** torch.arange(n_freq) * math.pi)
        self.lin = nn.Linear(2 * n_freq + 1, 1)

    def forward(self, t_starts, t_ends):
        s = ((t_starts + t_ends) / 2 - self.near) / (self.far - self.near)
        x = s[..., None] * self.freqs
        feat = torch.cat([s[..., None], torch.sin(x), torch.cos(x)], -1)
        return nn.functional.softplus(self.lin(feat).squeeze(-1) * 4.0)


def test_training_the_proposal_network(cuda):
    from cnc_amd.nerfacc import PropNetEstimator
    from cnc_amd.nerfacc.volrend import render_transmittance_from_density
    torch.manual_seed(0)
    n_rays, near, far = 256, 1.0, 10.0
    net = _Fourier(near, far).to(cuda)
    opt = torch.optim.Adam(net.parameters(), lr=2e-2)
    est = PropNetEstimator(opt).to(cuda)
    lo = torch.full((n_rays,), 4.0, device=cuda)
    truth = _slab_fn(lo, lo + 1.5, sigma=4.0)
    losses = []
    for _ in range(50):
        t0, t1 = est.sampling([net], [32], 16, n_rays=n_rays, near_plane=near, far_plane=far,
                              sampling_type="uniform", stratified=True, requires_grad=True)
        trans, _ = render_transmittance_from_density(t0, t1, truth(t0, t1))
        losses.append(est.update_every_n_steps(trans, requires_grad=True))
    assert est.prop_cache == []
    first, last = sum(losses[:5]) / 5, sum(losses[-5:]) / 5
    assert last < 0.5 * first, (first, last)
    # without requires_grad nothing is cached and nothing is trained
    est.sampling([net], [32], 16, n_rays=n_rays, near_plane=near, far_plane=far, sampling_type="uniform")
    assert est.prop_cache == [] and est.update_every_n_steps(trans, requires_grad=False) == 0.0


class _Ball(nn.Module):
    """A ball of radius 1 at the origin: density `sigma` inside, colour varying with position."""

    def __init__(self, sigma=10.0):
        super().__init__()
        self.sigma = sigma

    def density(self, x):
        return torch.where(x.norm(dim=-1, keepdim=True) <= 1.0, torch.full_like(x[..., :1], self.sigma),
                           torch.zeros_like(x[..., :1]))

    def forward(self, x, d=None):
        rgb = (0.5 + 0.45 * torch.tanh(x * torch.tensor([1.5, -1.0, 2.0], device=x.device))).clamp(0, 1)
        return (self.density(x) if d is None else (rgb, self.density(x)))


class _BallDensity(nn.Module):
    def __init__(self, ball):
        super().__init__()
        self.ball = ball

    def forward(self, x):
        return self.ball.density(x)


def _camera_rays(cuda, H=24, W=24):
    from cnc_amd.render import Rays
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(i + 0.5 - W / 2) / (W * 0.9), -(j + 0.5 - H / 2) / (H * 0.9), -torch.ones_like(i)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    o = torch.tensor([0.0, 0.0, 4.0]).expand(H, W, 3)
    return Rays(origins=o.contiguous().to(cuda), viewdirs=d.contiguous().to(cuda))


def _dense_render(ball, rays, near, far, n=4096, bkgd=None):
    from cnc_amd.nerfacc import rendering
    o, d = rays.origins.reshape(-1, 3), rays.viewdirs.reshape(-1, 3)
    t = torch.linspace(near, far, n + 1, device=o.device).expand(o.shape[0], n + 1)
    t0, t1 = t[:, :-1].contiguous(), t[:, 1:].contiguous()

    def rgb_sigma_fn(ts, te, _ri):
        x = o[:, None, :] + d[:, None, :] * ((ts + te) / 2)[..., None]
        rgb, s = ball(x.reshape(-1, 3), d[:, None, :].expand(x.shape).reshape(-1, 3))
        return rgb.reshape(x.shape), s.reshape(ts.shape), x

    rgb, _, _, _ = rendering(t0, t1, rgb_sigma_fn=rgb_sigma_fn, render_bkgd=bkgd)
    return rgb.reshape(*rays.origins.shape[:-1], 3)


@pytest.mark.parametrize("training", [True, False])
def test_render_image_with_propnet_matches_a_dense_render(cuda, training):
    from cnc_amd.nerfacc import PropNetEstimator
    from cnc_amd.render import render_image_with_propnet
    torch.manual_seed(1)
    ball = _Ball().to(cuda)
    props = [_BallDensity(ball), _BallDensity(ball)]
    rays = _camera_rays(cuda)
    bkgd = torch.ones(3, device=cuda)
    near, far = 2.0, 6.0
    with torch.no_grad():
        want = _dense_render(ball, rays, near, far, bkgd=bkgd)
    ball.train(training)
    est = PropNetEstimator().to(cuda)
    with torch.no_grad():
        rgb, opacity, depth, extras = render_image_with_propnet(
            ball, props, est, rays, num_samples=64, num_samples_per_prop=[128, 64], near_plane=near, far_plane=far,
            sampling_type="uniform", opaque_bkgd=False, render_bkgd=bkgd, test_chunk_size=100)
    assert rgb.shape == (24, 24, 3) and opacity.shape == (24, 24, 1) and depth.shape == (24, 24, 1)
    mse = ((rgb - want) ** 2).mean().item()
    psnr = -10 * math.log10(max(mse, 1e-12))
    assert psnr >= 30.0, psnr
    assert "weights" in extras


def test_each_level_uses_its_own_network(cuda):
    """render_image_with_propnet binds every proposal network in its own closure (the reference's
    `lambda *args: prop_sigma_fn(*args, p) for p in ...` would call the last one for every level)."""
    from cnc_amd.nerfacc import PropNetEstimator
    from cnc_amd.render import render_image_with_propnet
    ball = _Ball().to(cuda).eval()
    calls = []

    class Tagged(_BallDensity):
        def __init__(self, tag):
            super().__init__(ball)
            self.tag = tag

        def forward(self, x):
            calls.append((self.tag, x.shape[0]))
            return super().forward(x)

    rays = _camera_rays(cuda, 4, 4)
    with torch.no_grad():
        render_image_with_propnet(ball, [Tagged("a"), Tagged("b")], PropNetEstimator().to(cuda), rays, 8, [32, 16],
                                  near_plane=2.0, far_plane=6.0, sampling_type="uniform")
    assert calls == [("a", 16 * 32), ("b", 16 * 16)]


def test_dropins_resolve_to_the_proposal_route(cuda):
    import cnc_amd
    cnc_amd.install_dropins()
    import nerfacc
    import nerfacc.pdf
    from nerfacc.estimators.prop_net import PropNetEstimator, get_proposal_requires_grad_fn
    from cnc_amd.nerfacc import pdf as ours
    from cnc_amd.nerfacc.estimators import prop_net as ours_pn
    assert PropNetEstimator is ours_pn.PropNetEstimator
    assert get_proposal_requires_grad_fn is ours_pn.get_proposal_requires_grad_fn
    assert nerfacc.importance_sampling is ours.importance_sampling
    assert nerfacc.pdf.searchsorted is ours.searchsorted and nerfacc.searchsorted is ours.searchsorted
    assert nerfacc.PropNetEstimator is PropNetEstimator
    # the docstring examples of nerfacc/pdf.py:39-56,104-120, reproduced exactly on the device
    seq = nerfacc.RayIntervals(vals=torch.tensor([0.0, 1.0, 0.0, 1.0, 2.0], device=cuda),
                               packed_info=torch.tensor([[0, 2], [2, 3]], device=cuda))
    vals = nerfacc.RayIntervals(vals=torch.tensor([0.5, 1.5, 2.5], device=cuda),
                                packed_info=torch.tensor([[0, 1], [1, 2]], device=cuda))
    left, right = nerfacc.pdf.searchsorted(seq, vals)
    assert left.tolist() == [0, 3, 3] and right.tolist() == [1, 4, 4]
    iv, sm = nerfacc.pdf.importance_sampling(seq, torch.tensor([0.0, 0.5, 0.0, 0.5, 1.0], device=cuda), 2)
    assert iv.vals.tolist() == [[0.0, 0.5, 1.0], [0.0, 1.0, 2.0]] and sm.vals.tolist() == [[0.25, 0.75], [0.5, 1.5]]
