"""Error-map pixel sampling: a coarse per-image map of the recent loss, training pixels drawn in
proportion to it, and every ray's loss divided by its sampling density — what instant-ngp calls its error map.

The state is one map f32 [n_cams, G, G]; cell (gy, gx) of a camera covers the pixel rows [gy H / G, (gy + 1) H / G) and the
matching columns.  A pixel of cell c is drawn with probability

    p(pixel) = p(c) / a_c ,    p(c) = (1 - u) m_c a_c / sum(m a) + u a_c / sum(a)

(a_c the cell's pixel count, u the uniform floor), and carries the weight w = (1 / N_pix) / p(pixel) <= 1 / u, so that
the expectation of w f(pixel) under the draw is the plain mean of f over all pixels: the gradient's expectation is the
uniform sampler's.  The sampler, the map's update, the CDF and the weighted loss are HIP kernels (csrc/error_map.hip) in a
fixed order of operations: equal inputs give equal bits.  Host tensors take the torch restatement.

Not modelled: instant-ngp's sharpness term, data-parallel training, and loaders other than `TransformsLoader`.
"""
from __future__ import annotations

import torch

from .backends import errmap_backend as _K

# None of these has been tuned: nobody has run this on a real capture here.  `UNIFORM_FLOOR`: every pixel keeps at least
# this share of its uniform probability (weights <= 1 / floor); `DECAY`: the weight of the map's old value at an update;
# `REFRESH_EVERY`: steps between rebuilds of the CDF
RESOLUTION = 16
UNIFORM_FLOOR = 0.5
DECAY = 0.9
REFRESH_EVERY = 16
INITIAL_ERROR = 1.0         # the constant a map starts from: the first draws are uniform


class _WeightedLoss(torch.autograd.Function):
    """(rgb, pixels, weight) -> (loss, err): two launches forward, one backward.  Only rgb has a gradient."""

    @staticmethod
    def forward(ctx, rgb, pixels, weight):
        loss, err = _K.loss_forward(rgb, pixels, weight)
        ctx.save_for_backward(rgb, pixels, weight)
        ctx.mark_non_differentiable(err)
        return loss, err

    @staticmethod
    def backward(ctx, g_loss, _g_err):
        rgb, pixels, weight = ctx.saved_tensors
        return _K.loss_backward(g_loss.float().contiguous(), rgb, pixels, weight), None, None


def weighted_mse(rgb, pixels, weight):
    """-> (loss, err): loss = (1 / 3n) sum_i w_i sum_c (rgb - pixels)^2, differentiable in rgb, and the per-ray unweighted
    error err_i = (1 / 3) sum_c (rgb - pixels)^2 (detached) the map learns from.  All weights 1: the mse."""
    n = rgb.numel() // 3
    rgb, pixels, weight = rgb.reshape(n, 3), pixels.reshape(n, 3), weight.reshape(n)
    if not rgb.is_cuda:
        return _K.loss_forward_torch(rgb, pixels, weight)
    return _WeightedLoss.apply(rgb.float().contiguous(), pixels.detach().float().contiguous(),
                               weight.detach().float().contiguous())


class ErrorMapSampler:
    """The map and its sampling distribution for a capture of `n_cams` images of `height` x `width` pixels.

    `draw` reads the distribution as of the last `refresh`; `observe` folds a step's per-ray errors into the map;
    `refresh` rebuilds the distribution from the map.  A `refresh` leaves an event behind and a `draw` on another stream
    waits for it — no stream of the sampler's own.  (Not an nn.Module: nothing here is learned by an optimizer.)"""

    def __init__(self, n_cams: int, height: int, width: int, resolution: int = RESOLUTION,
                 uniform_floor: float = UNIFORM_FLOOR, decay: float = DECAY, refresh_every: int = REFRESH_EVERY, device=None):
        self.n_cams, self.height, self.width, self.resolution = _K.check_shape(n_cams, height, width, resolution)
        if not 0.0 < float(uniform_floor) <= 1.0:
            raise ValueError("error map: the uniform floor must lie in (0, 1] (it bounds the weights by its reciprocal)")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("error map: the decay must lie in [0, 1)")
        if isinstance(refresh_every, bool) or int(refresh_every) != refresh_every or refresh_every < 1:
            raise ValueError("error map: refresh_every must be a positive integer")
        self.uniform_floor, self.decay, self.refresh_every = float(uniform_floor), float(decay), int(refresh_every)
        G = self.resolution
        self.map = torch.full((self.n_cams, G, G), INITIAL_ERROR, dtype=torch.float32, device=device)
        self.prob = torch.empty(self.n_cams * G * G, dtype=torch.float32, device=device)
        self.cdf = torch.empty_like(self.prob)
        self._areas = _K.areas(self.n_cams, self.height, self.width, G, self.map.device).to(torch.float32)
        self._ready = None
        self.refresh()

    @property
    def n_pixels(self) -> int:
        return self.n_cams * self.height * self.width

    @torch.no_grad()
    def refresh(self) -> None:
        """The sampling distribution from the map as it stands."""
        if self.map.is_cuda:
            _K.cdf(self.map, self.height, self.width, self.uniform_floor, out=(self.prob, self.cdf))
            self._ready = torch.cuda.current_stream(self.map.device).record_event()
        else:
            prob, cdf = _K.cdf_torch(self.map, self.height, self.width, self.uniform_floor)
            self.prob.copy_(prob)
            self.cdf.copy_(cdf)

    @torch.no_grad()
    def draw(self, n: int, generator=None):
        """-> (cam_ids, px, py i64 [n], weight f32 [n]): one `torch.rand` and one launch."""
        dev = self.map.device
        args = (self.cdf, self.prob, self.n_cams, self.height, self.width, self.resolution)
        if not self.map.is_cuda:
            return _K.sample_torch(torch.rand((int(n), 3), dtype=torch.float32, device=dev, generator=generator), *args)
        if self._ready is not None:
            torch.cuda.current_stream(dev).wait_event(self._ready)
        return _K.sample(torch.rand((int(n), 3), dtype=torch.float32, device=dev, generator=generator), *args)

    @torch.no_grad()
    def observe(self, cam_ids, px, py, err) -> None:
        """map <- decay map + (1 - decay) mean(err) in every cell one of these rays lies in; a ray whose err is not finite
        is ignored on the device, and a cell without a ray keeps its bits."""
        shape = (self.n_cams, self.height, self.width, self.resolution)
        if self.map.is_cuda:
            _K.update(self.map, _K.keys(cam_ids.contiguous(), px.contiguous(), py.contiguous(), *shape),
                      err.detach().float().contiguous(), self.decay)
        else:
            _K.update_torch(self.map, _K.keys_torch(cam_ids, px, py, *shape), err.detach().float(), self.decay)

    @torch.no_grad()
    def effective_fraction(self) -> float:
        """1 / (N_pix sum over the pixels of p(pixel)^2): the share of the capture the draw effectively covers, 1 for the
        uniform draw (a synchronisation: logging only)."""
        live = self._areas > 0
        s = (self.prob[live].double() ** 2 / self._areas[live].double()).sum()
        return float(1.0 / (self.n_pixels * s))

    def state_dict(self):
        return {"map": self.map.detach().clone(), "prob": self.prob.detach().clone(), "cdf": self.cdf.detach().clone(),
                "shape": (self.n_cams, self.height, self.width, self.resolution), "uniform_floor": self.uniform_floor,
                "decay": self.decay, "refresh_every": self.refresh_every}

    @torch.no_grad()
    def load_state_dict(self, state) -> None:
        """The map and the distribution drawn from (which a `refresh` would not restore: it lags the map)."""
        if tuple(state["shape"]) != (self.n_cams, self.height, self.width, self.resolution):
            raise ValueError(f"error map: the state is of shape {tuple(state['shape'])}, this sampler of "
                             f"{(self.n_cams, self.height, self.width, self.resolution)}")
        self.uniform_floor, self.decay = float(state["uniform_floor"]), float(state["decay"])
        self.refresh_every = int(state["refresh_every"])
        self.map.copy_(state["map"])
        self.prob.copy_(state["prob"])
        self.cdf.copy_(state["cdf"])
        if self.map.is_cuda:
            self._ready = torch.cuda.current_stream(self.map.device).record_event()
