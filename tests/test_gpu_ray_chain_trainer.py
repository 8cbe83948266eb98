"""GPU: the Trainer's own step from the field's outputs on, with every ray-side option switched on at once — pose
refinement, exposure compensation, the distortion loss, and the learned background in one variant / the batch's colour
behind a foreground-only gain in the other (the map and the batch colour exclude each other) — on the capture of
tests/test_gpu_transforms_loader.py with the Trainer of tests/test_gpu_pose_trainer.py.

`render_image_with_occgrid`, `ExposureCompensation.__call__` and `_take_batch` are wrapped as pass-through recorders; after
three warm-up steps one `train_step` is recorded and everything downstream of the field is recomputed in float64
(tests/ray_chain_twin.py started at the recorded sigmas / rgbs; the pose fold by tests/pose_twin.py from the recorded
`positions.grad`) from the BATCH — its pixels, colour and camera ids — not from what the step handed its own functions.  The
tolerance is the "8 times" rule of ray_chain_twin.Yardstick with the 2^10 loss scale divided out; the measured ratios are in
profiles/ray_chain.md.  Each of the three schedules of `_backward_single` is held to that reference.

The schedules do not follow one trajectory (outside the reproducible mode the warm-up steps differ in their last bits, and
with them the recorded step's samples), so "the three agree in the bits of everything the entropy pass does not touch"
cannot be asked across them.  In its place every schedule's step is held to the bits of a REPLAY: the same kernels on the
recorded tensors, alone on the main stream.  The replay takes the camera ids, the colour and `gain_background` as the step
handed them to its own functions, so it sees what a schedule does to the gradients (cleared or assembled at the wrong
point, a race with the entropy pass) and NOT a wiring fault; wiring is what the float64 comparison holds."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pose_twin as PT
import ray_chain_twin as RC
import test_gpu_reproducible_step as R
from test_gpu_guarded_trainer import _differing, _everything, _nan_batch
from test_gpu_pose_trainer import _trainer
from test_gpu_transforms_loader import capture  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
LAMBDA = 1e-2
OPTIONS = dict(pose_lr=5e-3, exposure_lr=5e-3, distortion_weight=LAMBDA)
SCHEDULES = ("plain", "side_stream", "context_thread")
VARIANTS = ("envmap", "rgba")


def _all_options(cuda, tmp_path, root, variant, schedule="plain", **kw):
    extra = dict(background="envmap", envmap_resolution=4) if variant == "envmap" else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")             # (the map's warning about a capture with alpha)
        tr = _trainer(cuda, tmp_path, root, reproducible=schedule == "plain", **OPTIONS, **extra, **kw)
    if schedule == "side_stream":
        tr.ctx_thread = False
    assert (tr.ctx_stream is None) == (schedule == "plain") and bool(tr.ctx_thread) == (schedule == "context_thread")
    assert tr.cfg.lmbda > 0 and tr.bucket is None
    assert tr.pose_refiner is not None and tr.exposure is not None and (tr.envmap is not None) == (variant == "envmap")
    assert tr._exposure_foreground                  # the capture's images carry alpha
    return tr


class Recorder:
    """Pass-through recorders around the step's ray side; they change nothing but `retain_grad` on the extras."""

    def __init__(self, tr, monkeypatch):
        import cnc_amd.trainer as T
        from cnc_amd.exposure import ExposureCompensation
        self.on, self.render, self.gain, self.data = False, [], [], []
        inner_render, inner_gain, inner_take = T.render_image_with_occgrid, ExposureCompensation.__call__, tr._take_batch

        def render(field, estimator, rays, *a, **k):
            out = inner_render(field, estimator, rays, *a, **k)
            if self.on and field is tr.field and field.training:
                extra = out[4]
                extra["sigmas"].retain_grad(); extra["rgbs"].retain_grad()
                self.render.append(dict(rays=rays, render_bkgd=k.get("render_bkgd"), rgb=out[0], acc=out[1], extra=extra))
            return out

        def gain(this, rgb, camera_ids, opacity=None, bkgd=None, gain_background=True):
            out = inner_gain(this, rgb, camera_ids, opacity, bkgd, gain_background)
            if self.on:
                self.gain.append(dict(camera_ids=camera_ids, opacity=opacity, bkgd=bkgd, gain_background=gain_background, out=out))
            return out

        def take():
            data = inner_take()
            if self.on:
                self.data.append(data)
            return data
        monkeypatch.setattr(T, "render_image_with_occgrid", render)
        monkeypatch.setattr(ExposureCompensation, "__call__", gain)
        tr._take_batch = take


def _np(t):
    return t.detach().double().cpu().numpy()


def _recorded_step(cuda, tmp_path, root, variant, schedule, monkeypatch):
    """Three warm-up steps, then one recorded step -> everything the comparisons need, as device tensors."""
    tr = _all_options(cuda, tmp_path, root, variant, schedule)
    rec = Recorder(tr, monkeypatch)
    for s in range(3):
        assert tr.train_step(s, want_stats=False) is not None
    torch.cuda.synchronize()
    before = {"log_gain": tr.exposure.log_gain.detach().clone(),
              "texture": tr.envmap.texture.detach().clone() if tr.envmap is not None else None}
    assert bool(before["log_gain"].abs().sum() > 0)
    rec.on = True
    stats = tr.train_step(3)
    rec.on = False
    torch.cuda.synchronize()
    assert stats is not None and len(rec.render) == len(rec.gain) == len(rec.data) == 1
    return tr, rec.render[0], rec.gain[0], rec.data[0], before, stats


def _flat_rays(data):
    from cnc_amd.render import _as_ray_list
    return _as_ray_list(data["rays"])[0]


def _scalar_bounds(n, s_max, r64, pixel_bound):
    """The step's two statistics are float32 scalars, means over the batch; one float32 run of the twin is no yardstick for
    one number (it can land on the float64 value by chance), so they get bounds from the operation counts, u = 2^-24:
      distortion   per ray (2 S + 8) u relative (distortion_twin.bound, the kernel's own bound), the sum of n non-negative
                   terms n u more in any order, the division one:   (2 S_max + n + 9) u |ref|
      mse          the mean of 3 n squares of differences: a pixel off by e moves a square by at most (2 |p - q| + e) e;
                   difference, square, the sum of 3 n non-negative terms, the division:   that + (3 n + 3) u |ref|"""
    u = 2.0 ** -24
    worst = float(np.abs(r64["pixel"] - r64["pixels"]).max())
    return {"distortion": (2 * s_max + n + 9) * u * abs(r64["distortion"]),
            "mse": (2 * worst + pixel_bound) * pixel_bound + (3 * n + 3) * u * abs(r64["mse"])}


def _measure(yard, tr, variant, render, gain, data, before, stats, name):
    rays, extra = _flat_rays(data), render["extra"]
    n, C = rays.origins.shape[0], tr.exposure.n_cameras
    assert C == tr.pose_refiner.n_cameras == len(tr.dataset.train) and data["pixels"].reshape(-1, 3).shape[0] == n
    cams = data["camera_ids"].reshape(-1).cpu().numpy()
    ri, t0, t1 = (extra[k].cpu().numpy() for k in ("ray_indices", "t_starts", "t_ends"))
    info = extra["packed_info"].cpu().numpy()
    assert ri.shape[0] > 0 and (np.bincount(cams, minlength=C) > 0).sum() >= 2
    mode = "A+gain" if variant == "envmap" else "C"
    o, d = _np(rays.origins), _np(rays.viewdirs)

    def twin(dtype):
        return RC.chain(o, d, cams, ri, t0, t1, _np(data["pixels"]).reshape(-1, 3), C, mode, LAMBDA, dtype, field=None,
                        sigma_rgb=(_np(extra["sigmas"]), _np(extra["rgbs"])), bkgd=_np(data["color_bkgd"]),
                        texture=None if before["texture"] is None else _np(before["texture"]), log_gain=_np(before["log_gain"]))
    r64, r32 = twin(torch.float64), twin(torch.float32)
    assert np.array_equal(info[:, 0], r64["starts"]) and np.array_equal(info[:, 1], r64["counts"])
    s = RC.LOSS_SCALE
    r64["pixels"] = _np(data["pixels"]).reshape(-1, 3)

    def add(key, device, k64=None):
        k64 = k64 or key
        yard.add(name, key, np.asarray(device, np.float64).reshape(np.shape(r64[k64])), r64[k64], r32[k64])
    add("pixel", _np(gain["out"]).reshape(-1, 3))
    add("a", _np(render["acc"]).reshape(-1))
    add("g_sigma", _np(extra["sigmas"].grad) / s)
    add("g_rgb", _np(extra["rgbs"].grad) / s)
    # `_exposure_gradient`: what the gains' Adam descends along is the effective form
    assert tr.exposure.log_gain.grad is tr.exposure.effective_grad
    add("g_eff", _np(tr.exposure.log_gain.grad) / s)
    if variant == "envmap":
        add("g_texture", _np(tr.envmap.texture.grad) / s)
    # the pose fold, from the gradient that arrived at the positions
    g_x = _np(extra["positions"].grad) / s
    assert np.abs(g_x).max() > 0
    fold = lambda dtype: PT.ray_pose_grad(g_x, t0, t1, info[:, 0], info[:, 1], d, cams, C, dtype=dtype)
    yard.add(name, "g_pose", _np(tr.pose_refiner.delta.grad) / s, fold(np.float64), fold(np.float32).astype(np.float64))
    rayless = np.bincount(cams, minlength=C) == 0
    assert not _np(tr.pose_refiner.delta.grad)[rayless].any() and not _np(tr.exposure.effective_grad)[rayless].any()
    return r64, n, int(info[:, 1].max())


def _replay(tr, variant, render, gain, data, before):
    """The same kernels on the recorded tensors, alone on the main stream, in the Trainer's order -> the gradients."""
    from cnc_amd.envmap import EnvMapBackground
    from cnc_amd.exposure import ExposureCompensation
    from cnc_amd.nerfacc.volrend import rendering
    from cnc_amd.poses import ray_pose_grad
    from cnc_amd.trainer import Trainer
    rays, extra, dev = _flat_rays(data), render["extra"], tr.device
    n, C = rays.origins.shape[0], tr.exposure.n_cameras
    sig = extra["sigmas"].detach().clone().requires_grad_(True)
    rgbs = extra["rgbs"].detach().clone().requires_grad_(True)
    samples = {k: extra[k] for k in ("t_starts", "t_ends", "ray_indices", "packed_info")}
    rgb, acc, _, again = rendering(samples["t_starts"], samples["t_ends"], samples["ray_indices"], n_rays=n,
                                   rgb_sigma_fn=lambda *a: (rgbs, sig, None),
                                   render_bkgd=None if variant == "envmap" else render["render_bkgd"],      # (`background=`)
                                   packed_info=samples["packed_info"])
    exposure = ExposureCompensation(C, dev)
    with torch.no_grad():
        exposure.log_gain.copy_(before["log_gain"])
    envmap = None
    if variant == "envmap":
        envmap = EnvMapBackground(before["texture"].shape[0], device=dev)
        with torch.no_grad():
            envmap.texture.copy_(before["texture"])
        rgb = exposure(envmap(rgb, acc, rays.viewdirs), gain["camera_ids"])
    else:
        rgb = exposure(rgb, gain["camera_ids"], acc, gain["bkgd"], gain_background=gain["gain_background"])
    loss = F.mse_loss(rgb, data["pixels"]) + LAMBDA * Trainer._distortion(dict(again, **samples), n)
    (loss * RC.LOSS_SCALE).backward()
    info = samples["packed_info"]
    fold = ray_pose_grad(extra["positions"].grad.reshape(-1, 3).contiguous(), samples["t_starts"].contiguous(),
                         samples["t_ends"].contiguous(), info[:, 0].contiguous(), info[:, 1].contiguous(),
                         rays.viewdirs.reshape(-1, 3).contiguous(), data["camera_ids"].reshape(-1).contiguous(), C)
    torch.cuda.synchronize()
    return {"pixel": rgb, "g_sigma": sig.grad, "g_rgb": rgbs.grad, "g_eff": exposure.effective_grad, "g_pose": fold,
            "g_texture": envmap.texture.grad if envmap is not None else None}


@pytest.fixture(scope="module")
def steps(cuda, capture, tmp_path_factory):  # noqa: F811
    """The recorded step of every (variant, schedule), measured into ONE Yardstick: the floor of a tensor's bound is its
    worst float32 error over the module's six cases."""
    yard, out = RC.Yardstick(), {}
    for variant in VARIANTS:
        for schedule in SCHEDULES:
            name = f"{variant}-{schedule}"
            with pytest.MonkeyPatch.context() as mp:
                rec = _recorded_step(cuda, tmp_path_factory.mktemp(name), capture[0], variant, schedule, mp)
            out[name] = rec + _measure(yard, rec[0], variant, *rec[1:], name)
    return yard, out


def test_no_degenerate_case_sets_the_floor(steps):
    steps[0].check_floors()


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_against_float64_under_every_schedule(steps, variant, schedule):
    yard, out = steps
    name = f"{variant}-{schedule}"
    tr, render, gain, data, before, stats, r64, n, s_max = out[name]
    yard.check(name)
    pixel_bound = yard.ratio(name, "pixel")[2]
    for key, bound in _scalar_bounds(n, s_max, r64, pixel_bound).items():
        err = abs(stats[key] - r64[key])
        print(f"RATIO {name}/{key} {err / bound:.4g}   (err {err:.3e}, bound {bound:.3e})")
        assert err <= bound, (key, err, bound)
    # the render took the batch's colour only where nothing composites it later, and the gain saw the batch's cameras
    assert render["render_bkgd"] is None or variant == "envmap"
    assert torch.equal(gain["camera_ids"].reshape(-1), data["camera_ids"].reshape(-1))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_has_the_bits_of_its_kernels_alone(steps, variant, schedule):
    """What the entropy pass does not touch: the step's ray-side gradients are, bit for bit, those of the same kernels
    replayed on the recorded tensors alone on the main stream — under every schedule.  A substitute for bit equality across
    the schedules (see the module's docstring); it is fed what the step handed its own functions and holds no wiring."""
    tr, render, gain, data, before, stats = steps[1][f"{variant}-{schedule}"][:6]
    again = _replay(tr, variant, render, gain, data, before)
    step = {"pixel": gain["out"], "g_sigma": render["extra"]["sigmas"].grad, "g_rgb": render["extra"]["rgbs"].grad,
            "g_eff": tr.exposure.log_gain.grad, "g_pose": tr.pose_refiner.delta.grad,
            "g_texture": tr.envmap.texture.grad if variant == "envmap" else None}
    for k, v in step.items():
        if v is not None:
            assert R._bits(v.reshape(-1)).equal(R._bits(again[k].reshape(-1))), (k, schedule)


def _learned(tr):
    torch.cuda.synchronize()
    out = R._state(tr)                              # the field's and the context models' parameters and Adam states
    out["delta"] = tr.pose_refiner.delta.detach().clone()
    out["log_gain"] = tr.exposure.log_gain.detach().clone()
    out["texture"] = tr.envmap.texture.detach().clone()
    out["cameras"] = tr.dataset.train.cameras.clone()
    return out


def test_two_reproducible_runs_agree_in_every_learned_tensor(cuda, capture, tmp_path):  # noqa: F811
    """6 steps, all options: the field, the context models, the poses, the gains and the map, bit for bit."""
    runs = []
    for k in range(2):
        tr = _all_options(cuda, tmp_path / str(k), capture[0], "envmap")
        assert all(tr.train_step(s, want_stats=False) is not None for s in range(6))
        runs.append(_learned(tr))
    assert not _differing(*runs)
    start = _learned(_all_options(cuda, tmp_path / "start", capture[0], "envmap"))
    for group in ("delta", "log_gain", "texture"):
        assert not torch.equal(runs[0][group], start[group]), group
    assert any(k.startswith("field.") and not torch.equal(runs[0][k], start[k]) for k in start)
    assert any(k.startswith("context.") and not torch.equal(runs[0][k], start[k]) for k in start)


def _optimizer_states(tr):
    torch.cuda.synchronize()
    out = {}
    for name in ("opt", "opt2", "opt_pose", "opt_env", "opt_exposure"):
        opt = getattr(tr, name)
        for gi, group in enumerate(opt.param_groups):
            for pi, p in enumerate(group["params"]):
                out[f"{name}.{gi}.{pi}.param"] = p.detach().clone()
                for k, v in opt.state.get(p, {}).items():
                    if isinstance(v, torch.Tensor):
                        out[f"{name}.{gi}.{pi}.{k}"] = v.detach().clone()
    return out


def test_nan_batch_leaves_all_five_optimizers_untouched(cuda, capture, tmp_path):  # noqa: F811
    tr = _all_options(cuda, tmp_path, capture[0], "envmap", guarded_step=True)
    for s in range(3):
        assert tr.train_step(s) is not None
    assert tr.step_guard.stats() == {"skipped": 0, "reasons": 0}
    before, everything = _optimizer_states(tr), _everything(tr)
    small = ("opt_pose", "opt_env", "opt_exposure")
    for name in small:
        assert {f"{name}.0.0.{k}" for k in ("param", "exp_avg", "exp_avg_sq", "step")} <= set(before), name
    tr._next_data = _nan_batch(tr)
    assert "camera_ids" in tr._next_data
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = tr.train_step(3)
    assert out is not None and out["mse"] != out["mse"] and tr.step_guard.stats()["skipped"] == 1
    assert not _differing(before, _optimizer_states(tr))
    assert not _differing(everything, _everything(tr))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tr.train_step(4) is not None
    after = _optimizer_states(tr)
    steps = [k for k in before if k.endswith(".step")]
    assert {k.split(".")[0] for k in steps} == {"opt", "opt2", *small}
    for k in steps:
        assert float(after[k]) == float(before[k]) + 1, k
    for name in small:
        assert not torch.equal(after[f"{name}.0.0.param"], before[f"{name}.0.0.param"]), name
        assert bool(torch.isfinite(after[f"{name}.0.0.param"]).all())
