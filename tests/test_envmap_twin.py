"""CPU: the environment-map background's model through its NumPy twin — the float64 gradients against
central differences, the seam, the poles, texel centres, non-unit and dead directions, a fit of the whole chain to a bound
derived from the interpolation error — and the host-side pieces that need no GPU: the module's construction and
quantisation, the mirrors' refusal of host tensors, the container section, the flags."""
import numpy as np
import pytest
import torch

import envmap_twin as E


def _texture(H, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(H, 2 * H, 3))


def _unit(n, seed=1):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _centre_direction(H, i, j):
    """The direction whose (u, v) is exactly (j, i): the centre of texel (i, j)."""
    W = 2 * H
    phi, theta = ((j + 0.5) / W - 0.5) * 2 * np.pi, (i + 0.5) / H * np.pi
    return np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])


@pytest.mark.parametrize("H", [2, 4, 16])
def test_float64_gradients_against_central_differences(H):
    rng = np.random.default_rng(H)
    n = 40
    # (no derivative is taken in the direction, so no difference crosses a cell border)
    dirs, T = _unit(n, seed=H) * rng.uniform(0.5, 3.0, size=(n, 1)), _texture(H, seed=H)
    rgb, op, g = rng.uniform(size=(n, 3)), rng.uniform(size=n), rng.normal(size=(n, 3))
    _, g_rgb, g_op, g_T = E.loss_and_grads64(dirs, T, rgb, op, g)
    f = lambda T_=T, rgb_=rgb, op_=op: E.loss_and_grads64(dirs, T_, rgb_, op_, g)[0]
    h = 1e-6
    assert np.array_equal(g_rgb, g)
    for r in range(n):
        e = np.zeros(n); e[r] = h
        assert abs((f(op_=op + e) - f(op_=op - e)) / (2 * h) - g_op[r]) < 1e-8
    for idx in np.ndindex(H, 2 * H, 3):          # the composite is linear in T: the difference is exact up to rounding
        e = np.zeros_like(T); e[idx] = h
        assert abs((f(T_=T + e) - f(T_=T - e)) / (2 * h) - g_T[idx]) < 1e-8, idx
    assert np.abs(g_T).sum() > 0


@pytest.mark.parametrize("H", [2, 16, 64])
def test_columns_wrap_at_the_seam(H):
    W, T = 2 * H, _texture(H, seed=3)
    d = np.array([[-1.0, 0.0, 0.0], [-1.0, 1e-7, 0.0], [-1.0, -1e-7, 0.0]])
    env, cell, frac = E.forward(d, T)
    t = E.texels(cell, H)
    assert (t[:, 0] % W == W - 1).all() and (t[:, 1] % W == 0).all()        # columns W - 1 and 0, whichever side of the seam
    assert (cell % W == 0).all()                                            # one name for the pair: x0 = -1
    du = 1e-7 / (2 * np.pi) * W                                             # what 1e-7 rad is in columns
    assert np.abs(frac[:, 0] - 0.5).max() < 1.01 * du + 1e-12
    assert np.abs(env[1:] - env[0]).max() < 2.0 * du                        # continuous across it (|dT| <= 1 per column)
    row = H // 2 - 1                                                        # theta = pi/2: v = H/2 - 1/2, rows H/2 - 1 and H/2
    want = 0.25 * (T[row, W - 1] + T[row, 0] + T[row + 1, W - 1] + T[row + 1, 0])
    assert np.abs(env[0] - want).max() < 1e-12


@pytest.mark.parametrize("H", [2, 16, 64])
def test_rows_clamp_at_both_poles(H):
    W, T = 2 * H, _texture(H, seed=4)
    env, cell, frac = E.forward(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1e-12, 0.0, 5.0]]), T)
    t = E.texels(cell, H)
    assert (t[0] // W == 0).all() and (t[1] // W == H - 1).all()            # both rows are the same row
    assert cell[0] // W == 0 and cell[1] // W == H                          # y0 = -1 and y0 = H - 1
    x0 = W // 2 - 1                                                         # atan2(0, 0) = 0: u = W/2 - 1/2
    assert np.abs(env[0] - 0.5 * (T[0, x0] + T[0, x0 + 1])).max() < 1e-12
    assert np.abs(env[1] - 0.5 * (T[H - 1, x0] + T[H - 1, x0 + 1])).max() < 1e-12
    assert np.abs(env[2] - env[0]).max() < 1e-9


@pytest.mark.parametrize("H", [2, 16, 64])
def test_texel_centres_return_the_texel(H):
    W, T = 2 * H, _texture(H, seed=5)
    ij = [(i, j) for i in range(H) for j in range(W)]
    d = np.stack([_centre_direction(H, i, j) for i, j in ij])
    env, cell, _ = E.forward(d, T)
    assert (cell >= 0).all()
    assert np.abs(env - T.reshape(-1, 3)).max() < 1e-9
    env32, _, _ = E.forward(d.astype(np.float32), T.astype(np.float32), dtype=np.float32)
    assert env32.dtype == np.float32 and np.abs(env32 - T.reshape(-1, 3)).max() < 2e-4 * H / 16 + 1e-5


def test_length_does_not_matter():
    H, T, d = 16, _texture(16, seed=6), _unit(200, seed=6)
    base = E.forward(d, T)[0]
    for scale in (0.5, 3.0):
        assert np.abs(E.forward(d * scale, T)[0] - base).max() < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dead_rays_give_nothing_and_take_nothing(dtype):
    H, T = 4, _texture(4, seed=7).astype(dtype)
    d = np.array([[0, 0, 0], [np.nan, 0, 1], [1, np.inf, 0], [0, -np.inf, np.nan], [1, 2, 3]], dtype)
    rgb, op = np.full((5, 3), 0.25, dtype), np.full(5, 0.5, dtype)
    out, cell, frac = E.forward(d, T, rgb, op, dtype)
    assert list(cell[:4]) == [-1] * 4 and cell[4] >= 0 and not frac[:4].any()
    assert np.array_equal(out[:4], rgb[:4]) and np.isfinite(out).all()
    g = np.ones((5, 3), dtype)
    go, s, keys = E.backward_rays(cell, frac, op, g, T)
    assert not go[:4].any() and go[4] < 0 and (keys[:4] == H * 2 * H).all()
    gT, count, _ = E.backward_texture(cell, frac, s, H)
    alone = E.backward_texture(cell[4:], frac[4:], s[4:], H)[0]
    assert gT.dtype == dtype and np.array_equal(gT, alone) and count.sum() == 4


def test_float32_mode_follows_the_float64_mode():
    for H, bound in ((2, 2e-6), (16, 2e-5), (64, 1e-4)):
        T, d = _texture(H, seed=8), _unit(4000, seed=8)
        rgb, op = np.random.default_rng(9).uniform(size=(4000, 3)), np.random.default_rng(10).uniform(size=4000)
        o64 = E.forward(d.astype(np.float32).astype(np.float64), T.astype(np.float32).astype(np.float64),
                        rgb.astype(np.float32), op.astype(np.float32))[0]
        o32 = E.forward(d.astype(np.float32), T.astype(np.float32), rgb.astype(np.float32), op.astype(np.float32), np.float32)[0]
        assert o32.dtype == np.float32 and np.abs(o32 - o64).max() < bound


def test_texture_sum_is_a_function_of_the_segments_alone():
    """Two evaluations give the same bytes, and the float32 order stays within (n_t + 8) 2^-24 sum|c| of the float64 sum."""
    H, n = 2, 700
    rng = np.random.default_rng(11)
    cell, frac = E.coords(_unit(n, seed=11).astype(np.float32), H, np.float32)
    s = rng.normal(size=(n, 3)).astype(np.float32)
    a = E.backward_texture(cell, frac, s, H)[0]
    b = E.backward_texture(cell.copy(), frac.copy(), s.copy(), H)[0]
    assert a.tobytes() == b.tobytes()
    exact = E.backward_texture(cell, frac.astype(np.float64), s.astype(np.float64), H)
    assert np.abs(a - exact[0]).max() <= ((exact[1].max() + 8) * 2.0 ** -24 * exact[2]).max()


def test_resolution_is_checked():
    from cnc_amd.backends.envmap_backend import check_resolution
    for bad in (0, 1, 3, 15, 66, 128, -2):
        with pytest.raises(ValueError):
            check_resolution(bad)
        with pytest.raises(ValueError):
            E.check_resolution(bad)
    assert [check_resolution(h) for h in (2, 16, 64)] == [2, 16, 64]


def test_adam_fits_the_sky_through_the_twins_gradient():
    """Adam (rate 1e-2, 300 steps) on the H = 16 texture, 4,096 random directions a step with opacity in [0, 1/2], the loss
    the mean squared error of the composite against the same composite over sky(d) = 1/2 + 1/2 d.  The grey start is 0.24
    away in mean absolute error; bilinear interpolation of this sky at H = 16 errs by h^2 / 8 |f''| ~ 0.0025, and the bound
    is 8 times that."""
    H, lr, b1, b2, eps = 16, 1e-2, 0.9, 0.999, 1e-15
    rng = np.random.default_rng(12)
    T = np.full((H, 2 * H, 3), 0.5)
    m, v = np.zeros_like(T), np.zeros_like(T)
    probe = _unit(20000, seed=13)

    def mae(T):
        return float(np.abs(E.forward(probe, T)[0] - E.sky(probe)).mean())

    start = mae(T)
    assert 0.2 < start < 0.28
    for step in range(1, 301):
        d = rng.normal(size=(4096, 3))
        op = rng.uniform(0.0, 0.5, size=4096)
        rgb = np.zeros((4096, 3))
        out, cell, frac = E.forward(d, T, rgb, op)
        target = (1.0 - op)[:, None] * E.sky(d)
        g_out = 2.0 * (out - target) / out.size
        _, s, _ = E.backward_rays(cell, frac, op, g_out, T)
        g = E.backward_texture(cell, frac, s, H)[0]
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        T = T - lr * (m / (1 - b1 ** step)) / (np.sqrt(v / (1 - b2 ** step)) + eps)
        T = np.clip(T, 0.0, 1.0)
    end = mae(T)
    print(f"mean absolute error: {start:.4f} -> {end:.5f}")
    assert end < 0.02


# ---------------------------------------------------------------------------------------------- host side, no GPU
def test_module_construction_and_quantisation_on_the_host():
    from cnc_amd.envmap import EnvMapBackground
    for bad in (3, 0, 66):
        with pytest.raises(ValueError):
            EnvMapBackground(bad)
    env = EnvMapBackground(4)
    assert tuple(env.texture.shape) == (4, 8, 3) and env.texture.dtype == torch.float32 and bool((env.texture == 0.5).all())
    assert [n for n, _ in env.named_parameters()] == ["texture"]
    with torch.no_grad():
        env.texture.copy_(torch.linspace(-0.5, 1.5, 96).view(4, 8, 3))
    q = env.quantized()
    assert q.dtype == torch.uint8 and tuple(q.shape) == (4, 8, 3)
    assert torch.equal(q, torch.round(env.texture.detach().clamp(0, 1) * 255).to(torch.uint8))
    env.clamp_()
    assert float(env.texture.detach().min()) == 0.0 and float(env.texture.detach().max()) == 1.0
    other = EnvMapBackground(4)
    other.load_quantized(q)
    assert torch.equal(other.texture.detach(), q.float() / 255.0) and torch.equal(other.quantized(), q)
    with pytest.raises(ValueError):
        other.load_quantized(torch.zeros(2, 4, 3, dtype=torch.uint8))


def test_mirrors_refuse_host_tensors():
    from cnc_amd.backends import envmap_backend as K
    from cnc_amd.envmap import EnvMapBackground
    T, d = torch.full((2, 4, 3), 0.5), torch.ones(5, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        K.envmap_forward(d, T)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        K.envmap_backward_rays(torch.ones(5, 3), torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 2), T)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        K.envmap_backward_texture(torch.zeros(5, 4, dtype=torch.int32), torch.zeros(5, 2), torch.ones(5, 3), 2)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        EnvMapBackground(2).colors(d)


def _write(path, **kw):
    from cnc_amd.container import write_container
    g = torch.Generator().manual_seed(0)
    binaries = torch.rand(1, 8, 8, 8, generator=g) < 0.3
    mlp = {"w": torch.randn(6, 5, generator=g)}
    ctx = {"c": torch.randn(7, generator=g)}
    return write_container(str(path), meta={"Pgs": {}}, table_streams={"a": b"abc", "b": b"\x00\x01"}, binaries=binaries,
                           field_mlp=mlp, context_state=ctx, **kw)


def test_container_section(tmp_path):
    from cnc_amd.container import read_container, read_envmap, section_sizes
    u8 = torch.arange(8 * 16 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).view(8, 16, 3)
    _write(tmp_path / "off.cnc")
    _write(tmp_path / "none.cnc", envmap=None)
    size = _write(tmp_path / "on.cnc", envmap=u8)
    off, none, on = (open(tmp_path / f, "rb").read() for f in ("off.cnc", "none.cnc", "on.cnc"))
    assert off == none and "envmap" not in section_sizes(str(tmp_path / "off.cnc")) and read_envmap(str(tmp_path / "off.cnc")) is None
    sizes = section_sizes(str(tmp_path / "on.cnc"))
    assert sizes["envmap"] == 8 * 16 * 3 and list(sizes)[-1] == "envmap" and size == len(on)
    assert on.endswith(off[off.index(b"abc"):] + u8.numpy().tobytes())          # the other sections, then the map, raw
    back = read_envmap(str(tmp_path / "on.cnc"))
    assert back.dtype == torch.uint8 and torch.equal(back, u8)
    a, b = read_container(str(tmp_path / "on.cnc")), read_container(str(tmp_path / "off.cnc"))
    assert len(a) == 5 and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3]["w"], b[3]["w"])
    with pytest.raises(ValueError):
        _write(tmp_path / "bad.cnc", envmap=torch.zeros(3, 5, 3, dtype=torch.uint8))


def test_flags_reach_the_config_and_bad_values_raise():
    from cnc_amd.train import build_parser, make_config_and_data
    from cnc_amd.trainer import TrainConfig, Trainer
    cfg = TrainConfig()
    assert (cfg.background, cfg.envmap_resolution, cfg.envmap_lr) == ("solid", 16, 1e-2)
    args = build_parser().parse_args(["--dataset", "procedural"])
    assert (args.background, args.envmap_resolution, args.envmap_lr) == ("solid", 16, 1e-2)
    args = build_parser().parse_args(["--dataset", "procedural", "--background", "envmap", "--envmap-resolution", "8",
                                      "--envmap-lr", "0.02"])
    _, cfg, _ = make_config_and_data(args, "cpu")
    assert (cfg.background, cfg.envmap_resolution, cfg.envmap_lr) == ("envmap", 8, 0.02)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--background", "sky"])
    with pytest.raises(ValueError, match="background"):
        Trainer(TrainConfig(background="sky"), device="cpu")
    with pytest.raises(ValueError, match="resolution"):
        Trainer(TrainConfig(background="envmap", envmap_resolution=7), device="cpu")
