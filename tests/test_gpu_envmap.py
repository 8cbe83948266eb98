"""GPU: the environment-map kernels (csrc/envmap.hip) through the C ABI, every output inside a
sentinel-filled allocation (tests/guarded.py), against tests/envmap_twin.py.

Inputs.  Per H one pool of 4,099 rays, built once; a case of N rays takes its first N (so the references are computed once
per H and shared).  The live rays open with the six axes (the poles among them), the seam (-1, 0, 0), (-1, +-1e-7, 0), a
near-pole pair, texel centres, the same directions at lengths 0.5 and 3, then normal draws (non-unit).  Dead rays (zero,
NaN, +-inf in turn) are INSERTED at every eleventh position from the sixth on, so no named direction is lost to them;
`pool` asserts that every named direction is there and live.  Opacity is random with exact 0 and 1 interleaved; two cases
run all-0 and all-1, and two more send 4,099 identical rays (a generic direction: four texels of 4,099 contributions; a
pole: two of 8,198).

Forward bound.  `out` and `colors` must lie within  8 * e32 + 4 * 2^-23  of the float64 twin on the same float32 inputs,
e32 the float32 twin's own largest error against the float64 twin ON THE CASE'S OWN RAYS: the device's atan2f / acosf carry
bounds of up to 6 ulp where the host's carry about 1, everything else is the same correctly rounded float32 arithmetic.
Over one ray, or 4,099 identical ones, "the largest error" is whatever that ray happens to give, zero included, which
bounds nothing; so e32 has a floor: the twin's error at that H on random textures, 2e-7, 1.6e-6, 1.4e-5 at H = 2, 16, 64,
or the twin's error over the H's whole pool where that is smaller (no case is given more than the pool's own e32 by it).

Coordinates, read as the continuous (x0 + fx, y0 + fy) with x modulo W: u is held to the case's colour bound as it
stands.  v is held to the same bound plus, per ray, what the conditioning of theta = acos(cz) makes of cz's rounding, which
host and device share bit for bit: cz = dz / sqrt((dx dx + dy dy) + dz dz) carries at most 3.5 roundings (three products
and two sums of positive terms, halved by the root, the root, the quotient), delta = 4 * 2^-24 with |cz| <= 1, and
|d theta| <= min(2 delta / sin(theta), 1.1 sqrt(2 delta)) — the linear term with a factor 2 for its second order, capped
by the worst case at the pole itself, where 1 - cos(theta) = theta^2 / 2.  In rows that is H / pi times as much: 7e-6 of a
row for a generic ray at H = 64, 7e-3 for (1e-3, 1e-3, -1), where the colour does not move at all (both rows are the same
row).  A flip of the integer part at a cell border is not an error.

Backward.  Fed the device's own cell and frac, the float32 twin gives the device's bits for g_opacity, s, the keys and the
texture gradient.  Against the float64 twin on the same cell and frac (so the forward's share is zero by construction):
per texel (n_t + 8) 2^-24 sum|c| — a contribution carries at most five roundings ((1 - fx), the weight, (1 - opacity), s,
the product) and the fixed tree adds fewer than n_t more; g_opacity within 16 2^-24 sum|g_c| (env: two roundings per
weight, four products, three sums; the dot: three products, two sums; env <= 1).  No launch caps its grid, so there is no
later trip to reach."""
import numpy as np
import pytest
import torch

import envmap_twin as E
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu

N_POOL = 4099
E32_FLOOR = {2: 2e-7, 16: 1.6e-6, 64: 1.4e-5}       # the float32 twin's own error on random textures, per H
CZ_DELTA = 4 * 2.0 ** -24                            # rounding of cz = dz / |d| (see above)
HS = (2, 16, 64)
NS = (1, 65, 257, 4099)


def _centre(H, i, j):
    W = 2 * H
    phi, theta = ((j + 0.5) / W - 0.5) * 2 * np.pi, (i + 0.5) / H * np.pi
    return [np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)]


def _coordinate_gap(H, cell_a, frac_a, cell_b, frac_b, live):
    """(du, dv) [2, n_live] between two sets of coordinates read as continuous numbers, u modulo W."""
    W = 2 * H
    ya, xa = np.divmod(cell_a[live].astype(np.int64), W)
    yb, xb = np.divmod(cell_b[live].astype(np.int64), W)
    du = ((xa - 1) + frac_a[live, 0].astype(np.float64)) - ((xb - 1) + frac_b[live, 0].astype(np.float64))
    dv = ((ya - 1) + frac_a[live, 1].astype(np.float64)) - ((yb - 1) + frac_b[live, 1].astype(np.float64))
    return np.stack([(du + W / 2) % W - W / 2, dv])


_POOLS = {}


def pool(H):
    """The H's inputs and references, built once and never written to."""
    if H in _POOLS:
        return _POOLS[H]
    rng = np.random.default_rng(100 + H)
    W = 2 * H
    head = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
            [-1, 1e-7, 0], [-1, -1e-7, 0], [1e-12, 0, 5], [1e-3, 1e-3, -1]]
    centres = [(i, j) for i in sorted({0, 1, H // 2, H - 1}) for j in sorted({0, 1, W // 2, W - 1})]
    head += [_centre(H, i, j) for i, j in centres]
    head = np.asarray(head, np.float64)
    head = np.concatenate([head, 0.5 * head[6:], 3.0 * head[6:]]).astype(np.float32)
    dead = np.array([[0, 0, 0], [np.nan, 0.5, 0.5], [0.5, np.inf, 0], [0, 1, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    is_dead = np.zeros(N_POOL, bool)
    is_dead[5::11] = True
    n_live = int((~is_dead).sum())
    d = np.empty((N_POOL, 3), np.float32)
    d[is_dead] = dead[np.arange(N_POOL - n_live) % dead.shape[0]]
    d[~is_dead] = np.concatenate([head, rng.normal(size=(n_live - head.shape[0], 3)).astype(np.float32)])
    named = np.flatnonzero(~is_dead)[:head.shape[0]]                # where the named directions ended up: all of them, live
    assert np.array_equal(d[named], head) and np.isfinite(d[named]).all() and named[-1] < 257
    assert np.array_equal(d[named[4]], [0, 0, 1]) and np.array_equal(d[named[5]], [0, 0, -1]) and named[5] < 65
    op = rng.uniform(size=N_POOL).astype(np.float32)
    op[3::7], op[4::13] = 0.0, 1.0
    p = dict(H=H, dirs=d, dead=is_dead, named=named, T=rng.uniform(size=(H, W, 3)).astype(np.float32),
             rgb=rng.uniform(size=(N_POOL, 3)).astype(np.float32), op=op, g=rng.normal(size=(N_POOL, 3)).astype(np.float32))
    w = lambda a: a.astype(np.float64)
    p["out64"], p["cell64"], p["frac64"] = E.forward(w(d), w(p["T"]), w(p["rgb"]), w(op))
    p["env64"] = E.forward(w(d), w(p["T"]))[0]
    out32 = E.forward(d, p["T"], p["rgb"], op, np.float32)[0]
    env32 = E.forward(d, p["T"], dtype=np.float32)[0]
    p["err_out"], p["err_env"] = np.abs(out32 - p["out64"]).max(axis=1), np.abs(env32 - p["env64"]).max(axis=1)
    p["floor"] = min(E32_FLOOR[H], float(max(p["err_out"].max(), p["err_env"].max())))
    with np.errstate(all="ignore"):
        p["sin_theta"] = np.hypot(w(d)[:, 0], w(d)[:, 1]) / np.sqrt((w(d) ** 2).sum(axis=1))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _POOLS[H] = p
    return p


def _call(name, *args):
    from cnc_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, _lib.stream()), name)


def run_forward(dev, dirs, T, rgb=None, op=None, coords=True):
    n, H = dirs.shape[0], T.shape[0]
    ins = [Guarded(dirs, dev), Guarded(T, dev)] + ([Guarded(rgb, dev), Guarded(op, dev)] if rgb is not None else [])
    snaps = [g.snapshot() for g in ins]
    out = Guarded.empty((n, 3), np.float32, dev)
    cell = Guarded.empty((n,), np.int32, dev) if coords else None
    frac = Guarded.empty((n, 2), np.float32, dev) if coords else None
    _call("cnc_envmap_forward", ins[0].ptr, ins[2].ptr if rgb is not None else None, ins[3].ptr if rgb is not None else None,
          ins[1].ptr, H, n, out.ptr, cell.ptr if coords else None, frac.ptr if coords else None)
    torch.cuda.synchronize()
    for g, s in zip(ins, snaps):
        assert g.intact() and g.unchanged_since(s)
    for g in (out, cell, frac):
        assert g is None or g.intact()
    return out.get(), (cell.get() if coords else None), (frac.get() if coords else None)


def run_backward(dev, g_out, op, cell, frac, T):
    """-> (g_opacity, s, keys, g_T), the texture side behind the mirror's own sort."""
    n, H = g_out.shape[0], T.shape[0]
    ins = [Guarded(g_out, dev), Guarded(op, dev), Guarded(cell, dev), Guarded(frac, dev), Guarded(T, dev)]
    go, s = Guarded.empty((n,), np.float32, dev), Guarded.empty((n, 3), np.float32, dev)
    keys = Guarded.empty((n, 4), np.int32, dev)
    _call("cnc_envmap_backward_rays", ins[0].ptr, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, H, n, go.ptr, s.ptr, keys.ptr)
    sorted_keys, order = torch.sort(keys.tensor().reshape(-1), stable=True)
    offsets = torch.searchsorted(sorted_keys, torch.arange(2 * H * H + 1, dtype=torch.int32, device=dev))
    order_g, offsets_g = Guarded.like(order.contiguous()), Guarded.like(offsets.contiguous())
    gT = Guarded.empty((H, 2 * H, 3), np.float32, dev)
    _call("cnc_envmap_backward_texture", order_g.ptr, offsets_g.ptr, ins[3].ptr, s.ptr, H, n, gT.ptr)
    torch.cuda.synchronize()
    for g in ins + [go, s, keys, order_g, offsets_g, gT]:
        assert g.intact()
    return go.get(), s.get(), keys.get(), gT.get()


def forward_bound(p, per_ray_e32):
    """8 * e32 + 4 * 2^-23 with e32 the float32 twin's largest error on the case's own rays, floored (see the top)."""
    e32 = max(float(per_ray_e32.max()) if per_ray_e32.size else 0.0, p["floor"])
    return 8.0 * e32 + 4.0 * 2.0 ** -23, e32


def check_forward(p, n, out, cell, frac, ref, per_ray_e32, what):
    H, W = p["H"], 2 * p["H"]
    tol, e32 = forward_bound(p, per_ray_e32[:n])
    dead = p["dead"][:n]
    err = float(np.abs(out.astype(np.float64) - ref[:n]).max())
    print(f"{what}: H={H} N={n}  max |device - float64 twin| = {err:.3e}  bound = {tol:.3e}  (e32 = {e32:.3e})")
    assert np.isfinite(out).all() and err <= tol
    if cell is None:
        return
    assert (cell[dead] == -1).all() and not frac[dead].any() and (cell[~dead] >= 0).all()
    live = ~dead
    y1, x1 = np.divmod(cell[live].astype(np.int64), W)
    assert (x1 <= W - 1).all() and (y1 <= H).all() and (frac >= 0).all() and (frac <= 1).all()
    north, south = p["named"][4], p["named"][5]
    assert north >= n or cell[north] // W == 0                      # y0 = -1
    assert south >= n or cell[south] // W == H                      # y0 = H - 1: the largest cell row
    du, dv = _coordinate_gap(H, cell, frac, p["cell64"][:n], p["frac64"][:n], live)
    with np.errstate(divide="ignore"):
        dtheta = np.minimum(2 * CZ_DELTA / p["sin_theta"][:n][live], 1.1 * np.sqrt(2 * CZ_DELTA))
    tol_v = tol + H / np.pi * dtheta
    print(f"{what}: coordinates  max |du| = {np.abs(du).max():.3e}  bound = {tol:.3e};  max |dv| / its bound = "
          f"{(np.abs(dv) / tol_v).max():.3f}  (max |dv| = {np.abs(dv).max():.3e})")
    assert (np.abs(du) <= tol).all() and (np.abs(dv) <= tol_v).all()


def check_backward(T, g, op, cell, frac, got):
    go, s, keys, gT = got
    H = T.shape[0]
    go32, s32, keys32 = E.backward_rays(cell, frac, op, g, T)
    gT32, count, _ = E.backward_texture(cell, frac, s32, H)
    assert same_bits(go, go32) and same_bits(s, s32) and same_bits(keys, keys32) and same_bits(gT, gT32)
    w = lambda a: a.astype(np.float64)
    go64, s64, _ = E.backward_rays(cell, w(frac), w(op), w(g), w(T))
    gT64, _, mag = E.backward_texture(cell, w(frac), s64, H)
    assert (np.abs(go - go64) <= 16 * 2.0 ** -24 * np.abs(w(g)).sum(axis=1)).all()
    assert (np.abs(s - s64) <= 3 * 2.0 ** -24 * np.abs(s64)).all()          # two roundings: (1 - opacity), the product
    bound = (count.reshape(H, 2 * H, 1) + 8) * 2.0 ** -24 * mag
    assert (np.abs(gT - gT64) <= bound).all(), float((np.abs(gT - gT64) - bound).max())
    assert not gT[count.reshape(H, 2 * H) == 0].any()
    return count


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("H", HS)
def test_forward_and_backward_over_the_shape_matrix(cuda, H, N):
    p = pool(H)
    d, T, rgb, op, g = p["dirs"][:N], p["T"], p["rgb"][:N], p["op"][:N], p["g"][:N]
    out, cell, frac = run_forward(cuda, d, T, rgb, op)
    check_forward(p, N, out, cell, frac, p["out64"], p["err_out"], "out")
    assert same_bits(out[p["dead"][:N]], rgb[p["dead"][:N]])                 # env = 0: rgb + (1 - opacity) 0
    env, no_cell, _ = run_forward(cuda, d, T, coords=False)
    assert no_cell is None
    check_forward(p, N, env, None, None, p["env64"], p["err_env"], "colors")
    assert not env[p["dead"][:N]].any()
    got = run_backward(cuda, g, op, cell, frac, T)
    count = check_backward(T, g, op, cell, frac, got)
    assert count.sum() == 4 * int((~p["dead"][:N]).sum())
    again = run_backward(cuda, g, op, cell, frac, T)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    out2, cell2, frac2 = run_forward(cuda, d, T, rgb, op)
    assert same_bits(out, out2) and same_bits(cell, cell2) and same_bits(frac, frac2)


@pytest.mark.parametrize("level", [0.0, 1.0])
def test_opacity_zero_and_one(cuda, level):
    p = pool(16)
    d, T, rgb, g = p["dirs"][:257], p["T"], p["rgb"][:257], p["g"][:257]
    op = np.full(257, level, np.float32)
    out, cell, frac = run_forward(cuda, d, T, rgb, op)
    want = p["rgb"][:257].astype(np.float64) + (1.0 - level) * p["env64"][:257]
    tol, _ = forward_bound(p, np.abs(E.forward(d, T, rgb, op, np.float32)[0] - want).max(axis=1))
    assert np.abs(out - want).max() <= tol
    if level == 1.0:
        assert same_bits(out, rgb)                                          # rgb + 0 env
    go, s, keys, gT = got = run_backward(cuda, g, op, cell, frac, T)
    check_backward(T, g, op, cell, frac, got)
    assert level == 0.0 or (not s.any() and not gT.any())
    assert go[~p["dead"][:257]].any()


@pytest.mark.parametrize("kind", ["generic", "pole"])
def test_all_rays_identical_is_the_longest_segment(cuda, kind):
    p = pool(16)
    one = np.array([0.3, -0.7, 0.4] if kind == "generic" else [0.0, 0.0, -2.0], np.float32)
    d = np.tile(one, (N_POOL, 1))
    out, cell, frac = run_forward(cuda, d, p["T"], p["rgb"], p["op"])
    assert (cell == cell[0]).all() and same_bits(frac, np.tile(frac[0], (N_POOL, 1)))
    ref = E.forward(d.astype(np.float64), p["T"].astype(np.float64), p["rgb"].astype(np.float64), p["op"].astype(np.float64))[0]
    tol, _ = forward_bound(p, np.abs(E.forward(d, p["T"], p["rgb"], p["op"], np.float32)[0] - ref).max(axis=1))
    assert np.abs(out - ref).max() <= tol
    got = run_backward(cuda, p["g"], p["op"], cell, frac, p["T"])
    count = check_backward(p["T"], p["g"], p["op"], cell, frac, got)
    assert sorted(count[count > 0]) == ([N_POOL] * 4 if kind == "generic" else [2 * N_POOL] * 2)
    again = run_backward(cuda, p["g"], p["op"], cell, frac, p["T"])
    assert same_bits(got[3], again[3])


def test_no_rays_launch_nothing(cuda, monkeypatch):
    from cnc_amd import _lib
    from cnc_amd.backends import envmap_backend as K
    L = _lib.lib()
    for H in HS:        # the entry points: success with nothing to touch
        assert L.cnc_envmap_forward(None, None, None, None, H, 0, None, None, None, None) == 0
        assert L.cnc_envmap_backward_rays(None, None, None, None, None, H, 0, None, None, None, None) == 0
        assert L.cnc_envmap_backward_texture(None, None, None, None, H, 0, None, None) == 0
    for H in (0, 3, 66):
        assert L.cnc_envmap_forward(None, None, None, None, H, 0, None, None, None, None) != 0
    T = torch.full((4, 8, 3), 0.5, device=cuda)
    e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=cuda)

    def no_library():
        raise AssertionError("an empty call reached the library")
    monkeypatch.setattr(K._lib, "lib", no_library)
    out, cell, frac = K.envmap_forward(e(0, 3), T, e(0, 3), e(0))
    assert tuple(out.shape) == (0, 3) and tuple(cell.shape) == (0,) and tuple(frac.shape) == (0, 2)
    go, s, keys = K.envmap_backward_rays(e(0, 3), e(0), cell, frac, T)
    assert tuple(go.shape) == (0,) and tuple(s.shape) == (0, 3) and tuple(keys.shape) == (0, 4)
    gT = K.envmap_backward_texture(keys, frac, s, 4)
    assert tuple(gT.shape) == (4, 8, 3) and not gT.any()


def test_module_composites_and_differentiates_through_the_kernels(cuda):
    """`EnvMapBackground.forward` on image-shaped tensors: the entry points' bits, gradients for rgb, opacity and the texture
    (none for the direction), twice the same bits; `colors` is the lookup."""
    from cnc_amd.envmap import EnvMapBackground
    p = pool(16)
    n = 16 * 16
    env = EnvMapBackground(16, device=cuda)
    with torch.no_grad():
        env.texture.copy_(torch.from_numpy(p["T"].copy()))
    t = lambda a, *shape: torch.from_numpy(a[:n].copy()).to(cuda).view(*shape)
    rgb, op, d, g = t(p["rgb"], 16, 16, 3).requires_grad_(), t(p["op"], 16, 16, 1).requires_grad_(), t(p["dirs"], 16, 16, 3), t(p["g"], 16, 16, 3)
    grads = []
    for _ in range(2):
        env.texture.grad = rgb.grad = op.grad = None
        out = env(rgb, op, d)
        assert tuple(out.shape) == (16, 16, 3)
        out.backward(g)
        grads.append((out.detach().clone(), rgb.grad.clone(), op.grad.clone(), env.texture.grad.clone()))
    assert all(same_bits(a, b) for a, b in zip(*grads))
    out_k, cell, frac = run_forward(cuda, p["dirs"][:n], p["T"], p["rgb"][:n], p["op"][:n])
    go, s, keys, gT = run_backward(cuda, p["g"][:n], p["op"][:n], cell, frac, p["T"])
    out, g_rgb, g_op, g_T = grads[0]
    assert same_bits(out.view(n, 3), out_k) and same_bits(g_rgb, g) and same_bits(g_op.view(n), go) and same_bits(g_T, gT)
    assert same_bits(env.colors(d).view(n, 3), run_forward(cuda, p["dirs"][:n], p["T"], coords=False)[0])
    env.texture.grad = None
    with torch.no_grad():
        assert same_bits(env(rgb, op, d), out)
