"""The reference of tests/test_gpu_ray_chain.py and tests/test_gpu_ray_chain_trainer.py, pinned before anyone trusts it:
the float64 chain of tests/ray_chain_twin.py agrees, piece by piece, with the twins that are pinned already — render_twin
(composite forward and backward), distortion_twin.direct64, envmap_twin.loss_and_grads64, exposure_twin.backward and
pose_twin.ray_pose_grad in float64 — to 1e-12 of each tensor's largest entry, and the layout of the GPU tests meets its
conditions on the oracle's marcher (a NumPy jitter in place of the device's).  CPU only."""
import numpy as np
import pytest
import torch

import distortion_twin as DT
import envmap_twin as EM
import exposure_twin as EX
import pose_twin as PT
import ray_chain_twin as RC
import render_twin as RT

AGREE = 1e-12
C = RC.N_CAMERAS


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = np.abs(want).max(initial=0.0)
    err = np.abs(got - want).max(initial=0.0)
    assert err <= AGREE * scale, (what, err, scale)
    assert scale > 0, what


def _march(oracle, n, jitter_seed=0):
    """The layout's samples from the oracle's marcher and the float64 visibility test."""
    o, d, cam = RC.rays(n)
    near = (np.random.default_rng(jitter_seed).uniform(size=n) * RC.STEP).astype(np.float32)
    aabbs = np.array([[-1, -1, -1, 1, 1, 1]], np.float32)
    iv, sm, _ = oracle.traverse_grids(o, d, RC.occupancy(), aabbs, near, np.full(n, 1e10, np.float32), RC.STEP, 0.0)
    ri = sm["ray_indices"][sm["is_valid"]]
    t0, t1 = iv["vals"][iv["is_left"]], iv["vals"][iv["is_right"]]
    x = o[ri].astype(np.float64) + d[ri].astype(np.float64) * ((t0.astype(np.float64) + t1) / 2)[:, None]
    sigma = RC.field_terms(torch.from_numpy(x), torch.from_numpy(d[ri].astype(np.float64)), torch.float64)[0].numpy()
    keep = RC.visible(ri, t0, t1, sigma, n)
    return o, d, cam, ri[keep], t0[keep], t1[keep]


@pytest.fixture(scope="module")
def batch(oracle):
    o, d, cam, ri, t0, t1 = _march(oracle, 257)
    rng = np.random.default_rng(3)
    e = rng.uniform(-1, 1, (C, 3))
    return {"o": o, "d": d, "cam": cam, "ri": ri, "t0": t0, "t1": t1, "pixels": rng.uniform(0, 1, (257, 3)).astype(np.float32),
            "b3": rng.uniform(0, 1, 3).astype(np.float32), "bn": rng.uniform(0, 1, (257, 3)).astype(np.float32),
            "T": rng.uniform(0, 1, (16, 32, 3)).astype(np.float32), "e": (0.3 * e / np.abs(e).max()).astype(np.float32)}


def _chain(b, mode, lam, dtype=torch.float64, bkgd="b3", **kw):
    return RC.chain(b["o"], b["d"], b["cam"], b["ri"], b["t0"], b["t1"], b["pixels"], C, mode, lam, dtype,
                    bkgd=b[bkgd], texture=b["T"], log_gain=b["e"], **kw)


@pytest.mark.parametrize("jitter_seed", [0, 1, 2])
def test_layout_meets_its_conditions(oracle, jitter_seed):
    """What tests/test_gpu_ray_chain.py asserts on the device's `packed_info`, here for three jitters of the oracle's march:
    rays with 0, 1, 31..33 and >= 65 samples, rays with a gap in t, opaque central rays and thin grazing ones, cameras 3
    and 6 without a ray, runs of unequal length, at most 15 000 samples."""
    o, d, cam, ri, t0, t1 = _march(oracle, 257, jitter_seed)
    counts = np.bincount(ri, minlength=257)
    starts = np.cumsum(counts) - counts
    assert ri.shape[0] <= 15000
    for want in (0, 1, 31, 32, 33):
        assert (counts == want).any(), (want, np.bincount(counts))
    assert (counts >= 65).sum() >= 8
    gapped = [r for r in np.nonzero(counts > 1)[0] if (np.diff(t0[starts[r]:starts[r] + counts[r]]) > 1.5 * RC.STEP).any()]
    assert len(gapped) >= 3
    runs = np.bincount(cam, minlength=C)
    assert runs[3] == 0 and runs[6] == 0 and len(set(runs[list(RC.CAMERA_RUNS)])) == len(RC.CAMERA_RUNS)
    assert (np.diff(cam) >= 0).all()                                             # runs, not a shuffle
    a = RC.chain(o, d, cam, ri, t0, t1, np.zeros((257, 3)), C, "solid", 0.0, bkgd=np.ones(3))["a"]
    assert (a > 1 - 1e-6).sum() >= 5 and ((a < 0.5) & (counts > 0)).sum() >= 20
    occ = RC.occupancy()[0]
    assert occ[15, 15, 15] and not occ[14:, 14:, 14:].sum() > 1                  # the corner cell stands alone
    for n in (1, 65):
        _, _, cam_n, ri_n, _, _ = _march(oracle, n, jitter_seed)
        assert ri_n.shape[0] > 0 and not np.isin(cam_n, (3, 6)).any()


@pytest.mark.parametrize("mode,lam", [("solid", 0.0), ("A", 1e-2), ("B", 1e-2), ("C", 0.0), ("A+gain", 1e-2)])
def test_composite_is_render_twin(batch, mode, lam):
    """Weights, opacity and colour are render_twin.forward's; the gradients at sigma and rgb are render_twin.backward's of
    the gradients the chain hands the composite (colour, opacity, and the distortion term's at the weights)."""
    r = _chain(batch, mode, lam)
    lay = RT.Layout(r["starts"], r["counts"])
    f = RT.forward(lay, batch["t0"], batch["t1"], r["sigma"], r["rgb"])
    _close(r["weights"], f.w, "weights")
    _close(r["a"], f.op, "opacity")
    _close(r["c"], f.col, "colour")
    g_w = r["g_weights"] - (r["g_a"][lay.ri] + (r["g_c"][lay.ri] * r["rgb"]).sum(axis=1))    # what reaches w past c and a
    if lam == 0:
        assert np.abs(g_w).max() <= 1e-18
    else:
        assert np.abs(g_w).max() > 0
    b = RT.backward(f, grad_colors=r["g_c"], grad_opacity=r["g_a"], grad_weights=g_w)
    _close(r["g_sigma"], b.g_sigmas, "g_sigma")
    _close(r["g_rgb"], b.g_rgbs, "g_rgb")
    if mode == "solid":                             # ... and the finalised form with the colour inside the composite
        gp = 2.0 * (r["pixel"] - batch["pixels"].astype(np.float64)) / r["pixel"].size
        f = RT.forward(lay, batch["t0"], batch["t1"], r["sigma"], r["rgb"], render_bkgd=batch["b3"])
        _close(r["pixel"], f.col_f, "pixel")
        b = RT.backward(f, grad_colors=gp, finalize=True)
        _close(r["g_sigma"], b.g_sigmas, "g_sigma, finalised")


def test_distortion_is_direct64(batch):
    """distortion_twin.direct64 takes float32 weights: the chain's term on the same float32 weights, loss and gradient, ray
    by ray; and the chain's mean counts every ray, also those without samples."""
    r = _chain(batch, "solid", 1e-2)
    starts, counts, idx, mask = RC.rows(batch["ri"], 257)
    w32 = r["weights"].astype(np.float32)
    T = lambda a: torch.from_numpy(np.where(mask.numpy(), np.asarray(a, np.float64)[idx.numpy()], 0.0))
    w_rows = T(w32).requires_grad_(True)
    t0, t1 = batch["t0"].astype(np.float64), batch["t1"].astype(np.float64)
    per_ray = RC.distortion_rows(w_rows, T((t0 + t1) / 2), T(t1 - t0))
    per_ray.sum().backward()
    want = [DT.direct64(w32[s:s + c], batch["t0"][s:s + c], batch["t1"][s:s + c]) for s, c in zip(starts, counts)]
    _close(per_ray.detach().numpy(), np.array([w[0] for w in want]), "per-ray loss")
    _close(w_rows.grad.numpy()[mask.numpy()], np.concatenate([w[1] for w in want]), "d loss / d w")
    assert (counts == 0).any()
    _close(r["distortion"], r["per_ray_distortion"].sum() / 257, "mean over all rays")
    assert r["loss"] == pytest.approx(r["mse"] + 1e-2 * r["distortion"], rel=1e-15)


@pytest.mark.parametrize("H", [4, 16])
def test_background_is_envmap_twin(batch, H):
    b = dict(batch, T=np.random.default_rng(H).uniform(0, 1, (H, 2 * H, 3)).astype(np.float32))
    r = _chain(b, "A", 0.0)
    gp = 2.0 * (r["pixel"] - b["pixels"].astype(np.float64)) / r["pixel"].size
    loss, g_rgb, g_opacity, g_T = EM.loss_and_grads64(b["d"].astype(np.float64), b["T"], r["c"], r["a"], gp)
    out, _, _ = EM.forward(b["d"].astype(np.float64), b["T"], r["c"], r["a"], np.float64)
    _close(r["pixel"], out, "pixel")
    _close(r["g_c"], g_rgb, "g_rgb")
    _close(r["g_a"], g_opacity, "g_opacity")
    _close(r["g_texture"], g_T, "g_texture")


@pytest.mark.parametrize("bkgd", ["b3", "bn"])
@pytest.mark.parametrize("mode", ["B", "C", "gain"])
def test_gain_is_exposure_twin(batch, mode, bkgd):
    r = _chain(batch, mode, 0.0, bkgd=bkgd)
    gains = EX.gains(batch["e"], np.float64)
    _close(r["gain"], gains[batch["cam"]], "gains")
    b = None if mode == "gain" else batch[bkgd]
    a = None if mode == "gain" else r["a"]
    _close(r["pixel"], EX.forward(r["c"], a, b, batch["cam"], gains, mode != "C", np.float64), "pixel")
    gp = 2.0 * (r["pixel"] - batch["pixels"].astype(np.float64)) / r["pixel"].size
    g_rgb, g_opacity, G_eff, G = EX.backward(gp, r["c"], a, b, batch["cam"], gains, mode != "C", np.float64)
    _close(r["g_c"], g_rgb, "g_rgb")
    if mode != "gain":
        _close(r["g_a"], g_opacity, "g_opacity")
    _close(r["g_eff"], G_eff, "effective gradient")
    _close(r["g_log_gain"], G, "centred gradient")
    assert not r["g_eff"][[3, 6]].any() and r["g_log_gain"][[3, 6]].any()        # the centring reaches the rayless cameras


def test_gained_envmap_is_both_twins(batch):
    """A+gain: exposure_twin without a background on envmap_twin's output."""
    r = _chain(batch, "A+gain", 0.0)
    gains = EX.gains(batch["e"], np.float64)
    inner, _, _ = EM.forward(batch["d"].astype(np.float64), batch["T"], r["c"], r["a"], np.float64)
    _close(r["pixel"], EX.forward(inner, None, None, batch["cam"], gains, True, np.float64), "pixel")
    gp = 2.0 * (r["pixel"] - batch["pixels"].astype(np.float64)) / r["pixel"].size
    g_inner, _, G_eff, G = EX.backward(gp, inner, None, None, batch["cam"], gains, True, np.float64)
    _, g_rgb, g_opacity, g_T = EM.loss_and_grads64(batch["d"].astype(np.float64), batch["T"], r["c"], r["a"], g_inner)
    _close(r["g_c"], g_rgb, "g_rgb")
    _close(r["g_a"], g_opacity, "g_opacity")
    _close(r["g_texture"], g_T, "g_texture")
    _close(r["g_eff"], G_eff, "effective gradient")
    _close(r["g_log_gain"], G, "centred gradient")


def test_pose_gradient_is_pose_twin(batch):
    """(phi, tau) by autograd through x = o + tau + m (d + phi x d) equal pose_twin's fold of the chain's own dL/dx; the
    translation part also equals a central difference of the loss under a shift of one camera's origins."""
    r = _chain(batch, "B", 1e-2)
    G = PT.ray_pose_grad(r["g_x"], batch["t0"], batch["t1"], r["starts"], r["counts"], batch["d"], batch["cam"], C,
                         dtype=np.float64)
    _close(r["g_pose"], G, "g_pose")
    assert not r["g_pose"][[3, 6]].any() and all(r["g_pose"][k].any() for k in RC.CAMERA_RUNS)
    # the float32 inputs' midpoints: pose_twin forms (t0 + t1) 0.5 from the float32 inputs in float64, as the chain does
    cam, axis, h = 4, 1, 1e-6
    shifted = []
    for sign in (1.0, -1.0):
        o = batch["o"].astype(np.float64).copy()
        o[batch["cam"] == cam, axis] += sign * h
        shifted.append(_chain(dict(batch, o=o), "B", 1e-2)["loss"])
    fd = (shifted[0] - shifted[1]) / (2 * h)
    assert fd == pytest.approx(r["g_pose"][cam, 3 + axis], rel=1e-5), (fd, r["g_pose"][cam, 3 + axis])


def test_no_degenerate_case_sets_the_floor(oracle):
    """Over the chain test's cases on the oracle's samples: every tensor's floor (its worst relative float32 error) stays
    below ray_chain_twin.FLOOR_LIMIT, the one-ray batch included — its ray is half transparent, so that its background and
    the gradients it carries are not at rounding level."""
    yard = RC.Yardstick()
    for n in (1, 65, 257):
        inp = RC.inputs(n)
        samples = _march(oracle, n)[3:]
        for mode in RC.MODES:
            for variant in ((4, 16) if mode in ("A", "A+gain") else ("[3]", "[n,3]")):
                r64 = RC.case_twin(inp, samples, mode, 1e-2, variant, torch.float64)
                r32 = RC.case_twin(inp, samples, mode, 1e-2, variant, torch.float32)
                if n == 1:
                    assert 0.2 <= r64["a"][0] <= 0.9, r64["a"]
                for k in ("loss", "pixel", "a", "g_sigma", "g_rgb", "g_x", "g_pose", "g_texture", "g_log_gain", "g_eff"):
                    if r64[k] is not None:
                        yard.add(f"n{n}-{mode}-{variant}", k, r64[k], r64[k], r32[k])
    assert set(yard.floors()) == {"loss", "pixel", "a", "g_sigma", "g_rgb", "g_x", "g_pose", "g_texture", "g_log_gain", "g_eff"}
    yard.check_floors()


def test_float32_run_is_a_yardstick(batch):
    """The float32 run of the same chain differs from the float64 run by rounding: small and nonzero in every tensor, and
    the chain started at the field's outputs reproduces everything downstream of them."""
    r64, r32 = _chain(batch, "A+gain", 1e-2), _chain(batch, "A+gain", 1e-2, torch.float32)
    for k in ("loss", "pixel", "a", "g_sigma", "g_rgb", "g_x", "g_pose", "g_texture", "g_log_gain", "g_eff"):
        err = np.abs(np.asarray(r32[k]) - np.asarray(r64[k])).max()
        assert 0 < err <= 1e-3 * np.abs(np.asarray(r64[k])).max(), (k, err)
    tail = _chain(batch, "A+gain", 1e-2, field=None, sigma_rgb=(r64["sigma"], r64["rgb"]))
    for k in ("loss", "pixel", "a", "g_sigma", "g_rgb", "g_texture", "g_log_gain", "g_eff"):
        _close(tail[k], r64[k], k)
    assert tail["g_x"] is None and tail["g_pose"] is None
