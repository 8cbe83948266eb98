"""The ray-side chain of a training step in plain torch on the CPU, any dtype — test infrastructure, no GPU and no product
code.  What the per-kernel twins hold one kernel at a time (render_twin, distortion_twin, envmap_twin, exposure_twin,
pose_twin) is joined here the way `Trainer._render_and_update` joins the kernels, and differentiated by torch autograd:

    x      = o + tau[cam] + m (d + phi[cam] x d),  m = (t0 + t1) / 2        (phi, tau) leaves at zero: poses.py's left
                                                                            perturbation, exact at phi = 0
    sigma, rgb = field(x, d)          d detached: the product does not differentiate the view direction's path
    alpha  = 1 - exp(-sigma dt),  w = T_excl alpha,  c = sum w rgb,  a = sum w
    pixel  = A       c + (1 - a) env(d)            bilinear, wrapped columns, clamped rows; coordinates from
                                                    envmap_twin.coords in float64; the direction is not differentiated
             B       g_k (c + (1 - a) b)
             C       g_k c + (1 - a) b
             A+gain  g_k (c + (1 - a) env(d))
             solid   c + (1 - a) b
             gain    g_k c                          (the gain without any background: what exposure_twin calls b = None)
    g      = exp(e - mean over the cameras of e), per channel
    loss   = mse(pixel, pixels) + lambda * mean over ALL rays (a ray without samples counts as 0) of
             sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 (t1_i - t0_i)

`chain(..., dtype=torch.float64)` is the reference, `dtype=torch.float32` the yardstick of what float32 arithmetic costs on
the same samples.  The samples (ray_indices, t_starts, t_ends) are inputs: the device run's own are fed in, the marcher is
not re-derived.  `field=None` with `sigma_rgb=(sigmas, rgbs)` starts the chain at the field's outputs (then nothing
upstream of them — x, phi, tau — has a gradient)."""
import numpy as np
import torch

import envmap_twin as EM

MODES = ("A", "B", "C", "A+gain", "solid")
LOSS_SCALE = 2.0 ** 10

# The closed-form field of the chain tests: density s softplus(k (r0^2 - |x|^2)), colour sigmoid(Wx x + Wv v + c0 + A sin(F x)).
# Every constant is a float32 number, so the float32 module and the float64 twin hold the same weights.
FIELD = {
    "s": 512.0, "k": 96.0, "r0": 0.125,
    "Wx": ((1.5, -0.75, 0.25), (-0.5, 1.25, 0.75), (0.375, 0.5, -1.5)),
    "Wv": ((0.5, 0.25, -0.75), (-0.25, 0.625, 0.5), (0.75, -0.5, 0.125)),
    "c0": (0.125, -0.25, 0.0625),
    "A": (0.5, -0.375, 0.25), "F": (3.0, 2.0, 2.5),
}


def field_terms(x, v, dtype):
    """(sigma [N], rgb [N, 3]) of the closed-form field in `dtype`: elementwise operations only, so that the float32 module
    of tests/test_gpu_ray_chain.py (which calls this very function on device tensors) and the twin differ by rounding alone."""
    c = {k: torch.tensor(val, dtype=dtype, device=x.device) for k, val in FIELD.items()}
    r2 = (x * x).sum(-1)
    sigma = c["s"] * torch.nn.functional.softplus(c["k"] * (c["r0"] * c["r0"] - r2))
    pre = (x[:, None, :] * c["Wx"][None]).sum(-1) + (v[:, None, :] * c["Wv"][None]).sum(-1) + c["c0"] \
        + c["A"] * torch.sin(c["F"] * x)
    return sigma, torch.sigmoid(pre)


def rows(ray_indices, n_rays):
    """The flattened samples as padded rows: (starts, counts, index [n_rays, longest] into the samples, mask)."""
    ri = np.asarray(ray_indices, np.int64)
    assert ri.size == 0 or (np.diff(ri) >= 0).all(), "ray_indices must be sorted"
    counts = np.bincount(ri, minlength=n_rays).astype(np.int64)
    starts = np.cumsum(counts) - counts
    longest = int(counts.max(initial=0))
    k = np.arange(max(longest, 1))[None, :]
    mask = k < counts[:, None]
    idx = np.where(mask, starts[:, None] + k, 0)
    return starts, counts, torch.from_numpy(idx), torch.from_numpy(mask)


def env_lookup(dirs, texture):
    """env(d) [n, 3] as a differentiable function of `texture` [H, 2H, 3]: the four texels and weights of
    envmap_twin (coordinates in float64), the mix in the texture's dtype; 0 for a dead ray."""
    H = texture.shape[0]
    cell, frac = EM.coords(np.asarray(dirs, np.float64), H, np.float64)
    t = torch.from_numpy(EM.texels(cell, H).astype(np.int64))
    w = torch.from_numpy(EM.weights(frac)).to(texture.dtype)
    flat = torch.cat([texture.reshape(-1, 3), torch.zeros((1, 3), dtype=texture.dtype)])        # the dead rays' bin
    e = sum(w[:, k:k + 1] * flat[t[:, k]] for k in range(4))
    return torch.where(torch.from_numpy(cell < 0)[:, None], torch.zeros_like(e), e), t.numpy(), cell


def distortion_rows(w_rows, m_rows, dt_rows):
    """sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i per row of padded samples (w = 0 behind a ray's end)."""
    gap = (m_rows[:, :, None] - m_rows[:, None, :]).abs()
    return torch.einsum("ri,rij,rj->r", w_rows, gap, w_rows) + (w_rows * w_rows * dt_rows).sum(dim=1) / 3


def chain(o, d, cam_ids, ray_indices, t_starts, t_ends, pixels, n_cameras, mode, lam, dtype=torch.float64,
          field=field_terms, sigma_rgb=None, bkgd=None, texture=None, log_gain=None):
    """The whole chain -> dict of float64 NumPy arrays: loss, mse, distortion (the mean over all rays), pixel [n, 3], c
    [n, 3], a [n], weights [N], and the gradients of the loss g_sigma [N], g_rgb [N, 3], g_x [N, 3], g_pose [C, 6] =
    (phi, tau), g_texture, g_log_gain (the centred form: what autograd leaves in `.grad`), g_eff (e_eff as a leaf: what
    `effective_grad` holds), g_a [n], g_c [n, 3], g_weights [N] (the total into each weight) — None where the mode or the inputs leave a tensor out."""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(dtype)
    o, d, t0, t1, pixels = T(o).reshape(-1, 3), T(d).reshape(-1, 3), T(t_starts), T(t_ends), T(pixels).reshape(-1, 3)
    n, N, C = o.shape[0], t0.shape[0], int(n_cameras)
    cams = torch.from_numpy(np.asarray(cam_ids, np.int64).reshape(-1))
    ri = torch.from_numpy(np.asarray(ray_indices, np.int64))
    starts, counts, idx, mask = rows(ri.numpy(), n)
    m, dt = (t0 + t1) / 2, t1 - t0

    phi = torch.zeros((C, 3), dtype=dtype, requires_grad=True)
    tau = torch.zeros((C, 3), dtype=dtype, requires_grad=True)
    x = None
    if sigma_rgb is None:
        dr, cr = d[ri], cams[ri]
        x = o[ri] + tau[cr] + m[:, None] * (dr + torch.linalg.cross(phi[cr], dr))
        x.retain_grad()
        sigma, rgb = field(x, dr.detach(), dtype)
        sigma.retain_grad(); rgb.retain_grad()
    else:
        sigma, rgb = (T(v).requires_grad_(True) for v in sigma_rgb)
        rgb = rgb.reshape(-1, 3) if rgb.dim() != 2 else rgb

    def padded(v):                                   # [N, ...] -> [n, longest, ...], zeros behind a ray's end
        if N == 0:
            return torch.zeros((n, 1) + tuple(v.shape[1:]), dtype=v.dtype)
        p = v[idx]
        return torch.where(mask.reshape(mask.shape + (1,) * (v.dim() - 1)), p, torch.zeros_like(p))

    depth = padded(sigma * dt)                       # optical depth per sample, ray by ray: no running total across rays
    before = torch.cumsum(depth, dim=1) - depth
    w_rows = torch.exp(-before) * (1 - torch.exp(-depth))
    w_rows = torch.where(mask, w_rows, torch.zeros_like(w_rows))
    w_rows.retain_grad()
    c = (w_rows[..., None] * padded(rgb)).sum(dim=1)
    a = w_rows.sum(dim=1)
    c.retain_grad(); a.retain_grad()

    env = e = e_eff = None
    if mode in ("A", "A+gain"):
        texture = T(texture).requires_grad_(True)
        env, _, _ = env_lookup(d.numpy(), texture)
    gain = None
    if mode in ("B", "C", "A+gain", "gain"):
        e = T(log_gain).requires_grad_(True)
        e_eff = e - e.mean(dim=0, keepdim=True)
        e_eff.retain_grad()
        gain = torch.exp(e_eff)[cams]
    b = None
    if mode in ("B", "C", "solid"):
        b = T(bkgd)
        b = b.reshape(1, 3) if b.dim() == 1 else b.reshape(-1, 3)
    om = (1 - a)[:, None]
    pixel = {"A": lambda: c + om * env, "B": lambda: gain * (c + om * b), "C": lambda: gain * c + om * b,
             "A+gain": lambda: gain * (c + om * env), "solid": lambda: c + om * b, "gain": lambda: gain * c}[mode]()
    mse = ((pixel - pixels) ** 2).mean()

    per_ray = distortion_rows(w_rows, padded(m), padded(dt))
    distortion = per_ray.sum() / max(n, 1)
    loss = mse + lam * distortion
    loss.backward()

    def G(v):
        return None if v is None or v.grad is None else v.grad.detach().double().numpy()

    def V(v):
        return None if v is None else v.detach().double().numpy()
    upstream = sigma_rgb is None
    g_w = G(w_rows)
    g_phi, g_tau = G(phi), G(tau)
    zero3 = np.zeros((C, 3))
    g_pose = np.concatenate([zero3 if g_phi is None else g_phi, zero3 if g_tau is None else g_tau], axis=1)
    return {
        "loss": float(loss.detach()),
        "mse": float(mse.detach()),
        "distortion": float(distortion.detach()),
        "per_ray_distortion": V(per_ray),
        "pixel": V(pixel),
        "c": V(c),
        "a": V(a),
        "weights": V(w_rows[mask]),
        "env": V(env),
        "gain": V(gain),
        "sigma": V(sigma),
        "rgb": V(rgb),
        "x": V(x),
        "g_weights": None if g_w is None else g_w[mask.numpy()],
        "g_sigma": G(sigma),
        "g_rgb": G(rgb),
        "g_x": G(x) if upstream else None,
        "g_pose": g_pose if upstream else None,
        "g_texture": G(texture) if env is not None else None,
        "g_log_gain": G(e),
        "g_eff": G(e_eff),
        "g_a": G(a),
        "g_c": G(c),
        "starts": starts,
        "counts": counts,
    }


def forward_only(o, d, ray_indices, t_starts, t_ends, bkgd=None, texture=None, dtype=torch.float64):
    """(pixel, a) of the evaluation routes: mode A with a texture, solid with a colour, the bare c with neither."""
    n = np.asarray(o).reshape(-1, 3).shape[0]
    mode = "A" if texture is not None else "solid"
    r = chain(o, d, np.zeros(n, np.int64), ray_indices, t_starts, t_ends, np.zeros((n, 3)), 1, mode, 0.0, dtype,
              bkgd=np.zeros(3) if bkgd is None and texture is None else bkgd, texture=texture)
    return r["pixel"], r["a"]


# ---------------------------------------------------------------------------------------------------------------------
# the layout of the chain tests
# ---------------------------------------------------------------------------------------------------------------------
RESOLUTION, STEP, N_CAMERAS = 16, 0.04, 7
BALL_RADIUS = 1.4                                     # occupied: the cells whose centre lies inside, + the far corner cell
CAMERA_RUNS = (0, 1, 2, 4, 5)                         # cameras 3 and 6 have no ray
EARLY_STOP = 1e-4                                     # the sampler's default `early_stop_eps`


def occupancy():
    """bool [1, 16, 16, 16] over [-1, 1]^3: a ball and one detached cell behind it (the corner cell (15, 15, 15); its
    diagonal neighbour (14, 14, 14) is empty, so rays that reach it have a gap in t)."""
    c = (np.arange(RESOLUTION) + 0.5) / RESOLUTION * 2 - 1
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    occ = (X * X + Y * Y + Z * Z) < BALL_RADIUS ** 2
    assert not occ[15, 15, 15] and not occ[14, 14, 14] and not occ[15, 14, 14] and not occ[14, 15, 15]
    occ[15, 15, 15] = True
    return occ[None]


def rays(n, seed=7):
    """(o, d, cam_ids) float32 / int64: n rays from origins on the sphere of radius 2.5, in camera runs of unequal length
    over CAMERA_RUNS.  Every ray looks at a target point: most inside the ball of radius 0.9 (through the field's core: opaque,
    or past it: long and thin), one in eight at the corner cell (a short crossing of one or two samples, or the ball and then
    the cell), one in sixteen far outside the box (no sample).  n = 1: one half-transparent ray."""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    o = 2.5 * u / np.linalg.norm(u, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3))
    t = t / np.linalg.norm(t, axis=1, keepdims=True) * (0.9 * rng.uniform(size=(n, 1)))
    k = np.arange(n)
    at_corner = k % 8 == 3                        # just inside the box's edge x = y = 1 in the corner cell: 0 to 3 samples
    nc = int(at_corner.sum())
    t[at_corner] = np.stack([1 - rng.uniform(0.004, 0.03, nc), 1 - rng.uniform(0.004, 0.03, nc),
                             rng.uniform(0.89, 0.99, nc)], axis=1)
    long = k % 8 == 5                             # along a diagonal of the box, 0.26 to 0.34 past the centre: >= 65 thin samples
    nl = int(long.sum())
    diag = rng.choice([-1.0, 1.0], size=(nl, 3)) / np.sqrt(3.0)
    side = np.cross(diag, rng.normal(size=(nl, 3)))
    side = side / np.linalg.norm(side, axis=1, keepdims=True) * rng.uniform(0.26, 0.34, size=(nl, 1))
    o[long], t[long] = 2.5 * diag + side, side
    o[long] = 2.5 * o[long] / np.linalg.norm(o[long], axis=1, keepdims=True)
    away = k % 16 == 9
    t[away] = 3.0 * o[away] / 2.5 + rng.normal(size=(int(away.sum()), 3))
    if n == 1:
        # the one ray passes the core at 0.25: half transparent, so that the background, the map's gradient and the position
        # gradients it carries are of the size of every other batch's and not at rounding level behind an opaque ray
        side = np.cross(o[0], (0.3, -0.5, 0.8))
        t[0] = 0.25 * side / np.linalg.norm(side)
    d = t - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    # unequal runs: camera j of CAMERA_RUNS takes a share proportional to j + 1
    share = np.cumsum(np.arange(1, len(CAMERA_RUNS) + 1, dtype=np.float64))
    edges = np.floor(share / share[-1] * n).astype(np.int64)
    cam = np.asarray(CAMERA_RUNS, np.int64)[np.searchsorted(edges, k, side="right").clip(max=len(CAMERA_RUNS) - 1)]
    return o.astype(np.float32), d.astype(np.float32), cam


def inputs(n):
    """Everything a case of n rays is fed but the samples: rays and camera ids, pixels, the colour as "[3]" and "[n,3]", the
    texture at H = 4 and 16 (keys 4, 16), and `log_gain` with max |e| = 0.3 — float32 / int64 arrays."""
    o, d, cam = rays(n)
    rng = np.random.default_rng(100 + n)
    e = rng.uniform(-1.0, 1.0, (N_CAMERAS, 3))
    f32 = np.float32
    return {"o": o, "d": d, "cam": cam, "pixels": rng.uniform(0, 1, (n, 3)).astype(f32),
            "[3]": rng.uniform(0, 1, 3).astype(f32), "[n,3]": rng.uniform(0, 1, (n, 3)).astype(f32),
            4: rng.uniform(0, 1, (4, 8, 3)).astype(f32), 16: rng.uniform(0, 1, (16, 32, 3)).astype(f32),
            "log_gain": (0.3 * e / np.abs(e).max()).astype(f32)}


def case_twin(inp, samples, mode, lam, variant, dtype):
    """`chain` on the inputs of `inputs(n)`: `variant` is the colour's key for modes B, C, solid, the map's H for A, A+gain."""
    ri, t0, t1 = samples
    env = mode in ("A", "A+gain")
    return chain(inp["o"], inp["d"], inp["cam"], ri, t0, t1, inp["pixels"], N_CAMERAS, mode, lam, dtype,
                 bkgd=None if env else inp[variant], texture=inp[variant] if env else None, log_gain=inp["log_gain"])


def visible(ray_indices, t_starts, t_ends, sigma, n_rays):
    """The sampler's visibility test in float64: keep a sample while the transmittance in front of it is >= EARLY_STOP."""
    starts, counts, idx, mask = rows(ray_indices, n_rays)
    depth = np.where(mask.numpy(), (np.asarray(sigma, np.float64) * (np.asarray(t_ends, np.float64) - t_starts))[idx.numpy()], 0.0)
    before = np.cumsum(depth, axis=1) - depth
    keep = (np.exp(-before) >= EARLY_STOP) & mask.numpy()
    return keep[mask.numpy()]


# ---------------------------------------------------------------------------------------------------------------------
# the "8 times" rule
# ---------------------------------------------------------------------------------------------------------------------
MARGIN = 8.0
# No tensor's floor may be looser than this.  The chain's longest sums are ~70 samples and 257 rays, a few hundred float32
# roundings at the very most: relative 1e-6 to 1e-5 measured.  1024 u = 6e-5 leaves room for cancellation; a floor above
# it means one degenerate case (a reference at rounding level, say behind an opaque ray) is setting every case's bound.
FLOOR_LIMIT = 1024 * 2.0 ** -24


class Yardstick:
    """Per (case, tensor): err = max |device - twin64|, e32 = max |twin32 - twin64| on the case's own samples, ref = max
    |twin64|.  The bound of a tensor in a case is MARGIN * max(e32, floor * ref) with floor = the tensor's worst e32 / ref
    over every case added — so that a one-ray case does not bound itself with zero.  The margin is for the different order
    of the device's reductions."""

    def __init__(self):
        self.rows = {}

    def add(self, case, name, device, twin64, twin32):
        dev, r64, r32 = (np.asarray(v, np.float64) for v in (device, twin64, twin32))
        assert dev.shape == r64.shape == r32.shape, (case, name, dev.shape, r64.shape, r32.shape)
        assert np.isfinite(dev).all() and np.isfinite(r64).all(), (case, name)
        z = lambda v: float(np.abs(v).max(initial=0.0))
        self.rows[(case, name)] = (z(dev - r64), z(r32 - r64), z(r64))

    def floor(self, name):
        return max((e32 / ref for (_, nm), (_, e32, ref) in self.rows.items() if nm == name and ref > 0), default=0.0)

    def floors(self):
        """{tensor: (floor, the case that sets it)}: printed by the tests, so that a loose bound shows."""
        out = {}
        for (case, nm), (_, e32, ref) in self.rows.items():
            if ref > 0 and e32 / ref >= out.get(nm, (0.0, None))[0]:
                out[nm] = (e32 / ref, case)
        return out

    def check_floors(self, report=print):
        """Print `FLOOR <tensor> <floor> <case>` and assert that none is looser than FLOOR_LIMIT."""
        for nm, (f, case) in sorted(self.floors().items()):
            report(f"FLOOR {nm} {f:.3g} {case}")
            assert f <= FLOOR_LIMIT, (nm, f, case)

    def ratio(self, case, name):
        err, e32, ref = self.rows[(case, name)]
        bound = MARGIN * max(e32, self.floor(name) * ref)
        return (err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))), err, bound

    def names(self, case):
        return [nm for (c, nm) in self.rows if c == case]

    def check(self, case, report=print):
        """Print `RATIO <name> <err / bound>` for every tensor of the case, then assert that all are <= 1."""
        worst = {}
        for nm in self.names(case):
            r, err, bound = self.ratio(case, nm)
            report(f"RATIO {case}/{nm} {r:.4g}   (err {err:.3e}, bound {bound:.3e})")
            worst[nm] = r
        bad = {k: v for k, v in worst.items() if not v <= 1.0}
        assert not bad, (case, bad)
        return worst
