"""A learned environment-map background: a small equirectangular RGB texture indexed by ray direction
and composited behind the field, `out = rgb + (1 - opacity) env(dir)`, learned next to it — what instant-ngp calls its
envmap.  The lookup, the composite and both sides of the gradient are HIP kernels (csrc/envmap.hip); the texture's
gradient is a grouped sum in a fixed order, so it is bit-reproducible as it stands.  GPU tensors only.
"""
from __future__ import annotations

import torch

from .backends import envmap_backend as _K


class _Composite(torch.autograd.Function):
    """rgb + (1 - opacity) env(dirs) over the three launches.  No gradient with respect to the direction."""

    @staticmethod
    def forward(ctx, texture, rgb, opacity, dirs):
        out, cell, frac = _K.envmap_forward(dirs, texture, rgb, opacity)
        ctx.save_for_backward(texture, opacity, cell, frac)
        return out

    @staticmethod
    def backward(ctx, g_out):
        texture, opacity, cell, frac = ctx.saved_tensors
        g_opacity, s, keys = _K.envmap_backward_rays(g_out.contiguous(), opacity, cell, frac, texture)
        g_texture = _K.envmap_backward_texture(keys, frac, s, texture.shape[0]) if ctx.needs_input_grad[0] else None
        return g_texture, g_out, g_opacity, None


class EnvMapBackground(torch.nn.Module):
    """`texture` [H, 2H, 3], float32, initialised to 0.5 (mid grey); H even, 2 <= H <= 64 (ValueError otherwise)."""

    def __init__(self, resolution: int = 16, device=None):
        super().__init__()
        H = _K.check_resolution(resolution)
        self.texture = torch.nn.Parameter(torch.full((H, 2 * H, 3), 0.5, dtype=torch.float32, device=device))

    @property
    def resolution(self) -> int:
        return self.texture.shape[0]

    def forward(self, rgb, opacity, dirs):
        """rgb [..., 3], opacity [..., 1] or [...], dirs [..., 3] (any length; zero or non-finite: no background) ->
        rgb + (1 - opacity) env(dirs), shaped like rgb.  Gradients: rgb, opacity, the texture."""
        lead = rgb.shape
        n = rgb.numel() // 3
        op = opacity.reshape(n).float().contiguous()
        out = _Composite.apply(self.texture, rgb.reshape(n, 3).float().contiguous(), op,
                               dirs.detach().reshape(n, 3).float().contiguous())
        return out.view(lead)

    @torch.no_grad()
    def colors(self, dirs):
        """env(dirs) [..., 3]: the same launch as the composite's, without rgb and opacity."""
        lead = dirs.shape
        out, _, _ = _K.envmap_forward(dirs.reshape(-1, 3).float().contiguous(), self.texture.detach(), want_coords=False)
        return out.view(lead)

    @torch.no_grad()
    def clamp_(self):
        """Project the texture into [0, 1] (behind every optimizer step: what `quantized` can hold)."""
        self.texture.clamp_(0.0, 1.0)
        return self

    @torch.no_grad()
    def quantized(self) -> torch.Tensor:
        """uint8 [H, 2H, 3] = round(255 clamp(texture, 0, 1)): the container's section."""
        return torch.round(self.texture.clamp(0.0, 1.0) * 255.0).to(torch.uint8)

    @torch.no_grad()
    def load_quantized(self, u8) -> None:
        """texture = u8 / 255, exactly what a receiver renders with."""
        u8 = torch.as_tensor(u8)
        if u8.dtype != torch.uint8 or tuple(u8.shape) != tuple(self.texture.shape):
            raise ValueError(f"environment map: expected uint8 {list(self.texture.shape)}, got {u8.dtype} {list(u8.shape)}")
        self.texture.copy_(u8.to(self.texture.device).to(torch.float32) / 255.0)
