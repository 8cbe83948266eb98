"""GPU: depth supervision in the Trainer (`TrainConfig.depth_weight` / `depth_spread`) on the procedural scene, the small
configuration of tests/test_gpu_reproducible_step.py (the one tests/test_gpu_distortion_trainer.py uses): off, nothing moves;
on, it is bit-reproducible, its statistic is the public function's value, it pulls the weight towards the measured surface,
the guarded step covers it, what cannot work is refused at construction, and the CLI takes the flags."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_twin as T
from test_gpu_reproducible_step import _bits, _cfg, _state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(cuda, tmp_path, **kw):
    from cnc_amd.trainer import Trainer
    torch.manual_seed(1234)
    tr = Trainer(_cfg(tmp_path, seed=3, **kw), device=cuda)
    g = torch.Generator(device=cuda)         # the context pass's window draw from a generator of its own (no race with the
    g.manual_seed(77)                        # sampler's on the default one when the mode is off)
    tr.context.rand_like = lambda t: torch.rand(t.shape, generator=g, device=t.device, dtype=t.dtype)
    return tr


def _run(cuda, tmp_path, steps, **kw):
    tr = _trainer(cuda, tmp_path, **kw)
    out = [tr.train_step(s) for s in range(steps)]
    torch.cuda.synchronize()
    return tr, out, _state(tr)


def _same_bits(st_a, st_b):
    assert set(st_a) == set(st_b)
    for k in st_a:
        assert int((_bits(st_a[k]) != _bits(st_b[k])).sum()) == 0, k


def test_a_weight_zero_is_inert(cuda, tmp_path):
    tr_a, out_a, st_a = _run(cuda, tmp_path, 5, reproducible=True)
    tr_b, out_b, st_b = _run(cuda, tmp_path, 5, reproducible=True, depth_spread=7.0)
    assert tr_a._depth_weight == 0.0 and tr_a.dataset.with_depth is False
    assert "depth" not in tr_a.dataset.fetch()
    assert all(o is None or "depth" not in o for o in out_a + out_b)
    assert out_a == out_b and any(o is not None for o in out_a)
    _same_bits(st_a, st_b)


def test_b_reproducible_mode_gives_equal_bits(cuda, tmp_path):
    _, out_a, st_a = _run(cuda, tmp_path, 10, depth_weight=1.0, reproducible=True)
    _, out_b, st_b = _run(cuda, tmp_path, 10, depth_weight=1.0, reproducible=True)
    taken = [o for o in out_a if o is not None]
    assert taken and out_a == out_b
    for o in taken:
        assert math.isfinite(o["depth"]) and o["depth"] > 0
        assert set(o) == {"mse", "psnr", "bpp", "embed_bits_MB", "n_rendering_samples", "num_rays", "depth"}
    _same_bits(st_a, st_b)


def test_c_the_statistic_is_the_public_function_on_the_steps_samples(cuda, tmp_path):
    """`stats["depth"]` of one step against the float64 definition on that step's samples (`Trainer.on_depth_loss`), within
    the twin's bound per ray plus the mean's own rounding ((n - 1) 2^-24 sum |L_ray| in any order of summation)."""
    from cnc_amd.nerfacc.losses import depth_loss
    tr = _trainer(cuda, tmp_path, depth_weight=1.0, depth_spread=2.5)
    seen = []
    tr.on_depth_loss = lambda extra, target, per_ray: seen.append(
        ({k: extra[k].detach().clone() for k in ("weights", "t_starts", "t_ends", "ray_indices", "packed_info")},
         target.clone(), per_ray.detach().clone()))
    stats = tr.train_step(0)
    torch.cuda.synchronize()
    assert stats is not None and len(seen) == 1
    extra, target, per_ray = seen[0]
    n = stats["num_rays"]
    assert tuple(target.shape) == (n,) and tuple(per_ray.shape) == (n,) and int((target > 0).sum()) > 0
    again = depth_loss(extra["weights"], extra["t_starts"], extra["t_ends"], target, ray_indices=extra["ray_indices"],
                       n_rays=n, packed_info=extra["packed_info"], spread=2.5)
    assert torch.equal(again.view(torch.int32), per_ray.view(torch.int32))
    w, t0, t1 = (extra[k].cpu().numpy() for k in ("weights", "t_starts", "t_ends"))
    info, D = extra["packed_info"].cpu().numpy(), target.cpu().numpy()
    want = tol = sum_abs = 0.0
    for r in range(n):
        seg = slice(int(info[r, 0]), int(info[r, 0] + info[r, 1]))
        L = T.direct64(w[seg], t0[seg], t1[seg], D[r], 2.5)[0]
        want, sum_abs = want + L, sum_abs + abs(L)
        tol += T.bound(int(info[r, 1]), w[seg], t0[seg], t1[seg], D[r], 2.5)[1]
    want, tol = want / n, (tol + (n - 1) * T.U * sum_abs) / n + T.U * want / n
    print(f"stats {stats['depth']:.9g} direct64 {want:.9g} |diff| / bound {abs(stats['depth'] - want) / tol:.3g}")
    assert want > 0 and abs(stats["depth"] - want) <= tol


def _mean_s2(tr, batch):
    """Mean over the batch's rays with a measurement of S2 = sum w e^2, from the public function: L(spread 1) - L(spread 0)."""
    from cnc_amd.nerfacc.losses import depth_loss
    from cnc_amd.render import render_image_with_occgrid
    c = tr.cfg
    tr.field.eval(); tr.estimator.eval()
    with torch.no_grad():
        _, _, _, _, extra = render_image_with_occgrid(
            tr.field, tr.estimator, batch["rays"], near_plane=c.near_plane, render_step_size=c.render_step_size,
            render_bkgd=batch["color_bkgd"], cone_angle=c.cone_angle, alpha_thre=c.alpha_thre, return_extra=True,
            with_samples=True)
        n = batch["depth"].shape[0]
        args = (extra["weights"], extra["t_starts"], extra["t_ends"], batch["depth"])
        kw = dict(ray_indices=extra["ray_indices"], n_rays=n, packed_info=extra["packed_info"])
        s2 = depth_loss(*args, spread=1.0, **kw).double() - depth_loss(*args, spread=0.0, **kw).double()
        opacity = torch.zeros(n, device=s2.device).index_add_(0, extra["ray_indices"], extra["weights"])
    hit = batch["depth"] > 0
    return float(s2[hit].mean()), float(opacity[hit].mean())


def _probe_batch(cuda, image_size):
    from cnc_amd.datasets import SyntheticBallDataset
    probe = SyntheticBallDataset(image_size, device=cuda, seed=99)       # the training views, draws of its own
    probe.with_depth = True
    batch = probe.fetch(4096)
    assert int((batch["depth"] > 0).sum()) > 100
    return batch


@pytest.fixture(scope="module")
def without_depth(cuda, tmp_path_factory):
    """150 steps with the option off, shared by the two direction tests: (mean S2, mean opacity) on the probe batch.  All three
    runs are made under `reproducible`: one seed, one trajectory each, the same on every run of the tests."""
    tr, _, _ = _run(cuda, tmp_path_factory.mktemp("off"), 150, reproducible=True)
    return _mean_s2(tr, _probe_batch(cuda, tr.cfg.image_size))


def test_d_the_weight_moves_towards_the_measured_surface(cuda, tmp_path, without_depth):
    """150 steps from one seed with depth_weight = 1 and with it off; mean S2 of 4096 fixed training rays with a measurement.
    Measured on the MI355X: 1.68e-5 with the weight against 7.0e-3 .. 7.2e-3 without — but S2 also falls when the weights
    vanish, and that is what happens here: the mean opacity of those rays is 0.0000 with the weight against 0.985 without.
    At weight 1 the depth term, which never pushes opacity up, outweighs the colour loss on this scene and the field goes
    transparent; the direction holds, the run is useless.  The test below takes a weight at which it is not."""
    tr_on, _, _ = _run(cuda, tmp_path, 150, depth_weight=1.0, reproducible=True)
    (on, opacity_on), (off, opacity_off) = _mean_s2(tr_on, _probe_batch(cuda, tr_on.cfg.image_size)), without_depth
    print(f"mean S2 over rays with a measurement after 150 steps: depth_weight=1: {on:.6g}   off: {off:.6g}")
    print(f"mean opacity of those rays: depth_weight=1: {opacity_on:.4f}   off: {opacity_off:.4f}")
    assert on < off


def test_d_a_small_weight_moves_the_weight_and_keeps_the_surface(cuda, tmp_path, without_depth):
    """The same at depth_weight = 0.01: S2 falls AND the rays that hit the ball stay opaque.  The opacity bound is not a
    measurement: the ball is opaque, so a field that explains its colours renders those rays with opacity near 1, and a
    collapsed one with opacity near 0; 0.5 separates the two.  Measured on the MI355X: see profiles/depth_supervision.md."""
    tr_on, _, _ = _run(cuda, tmp_path, 150, depth_weight=0.01, reproducible=True)
    (on, opacity_on), (off, opacity_off) = _mean_s2(tr_on, _probe_batch(cuda, tr_on.cfg.image_size)), without_depth
    print(f"mean S2 over rays with a measurement after 150 steps: depth_weight=0.01: {on:.6g}   off: {off:.6g}")
    print(f"mean opacity of those rays: depth_weight=0.01: {opacity_on:.4f}   off: {opacity_off:.4f}")
    assert on < off and opacity_on > 0.5 and opacity_off > 0.5


def test_e_the_guarded_step_covers_the_term(cuda, tmp_path):
    tr = _trainer(cuda, tmp_path, depth_weight=1.0, guarded_step=True)
    tr.prefetch = False                       # every step draws its batch at its top: the batch below is the step's
    assert tr.step_guard is not None
    assert tr.train_step(0) is not None
    fetch = tr.dataset.fetch

    def no_measurement():
        d = fetch()
        d["depth"] = torch.full_like(d["depth"], float("inf"))
        return d

    # +inf on every ray means "no measurement", not an error: the step is taken
    tr.dataset.fetch = no_measurement
    before = _state(tr)
    stats = tr.train_step(1)
    torch.cuda.synchronize()
    assert stats["depth"] == 0.0 and tr.step_guard.stats()["skipped"] == 0
    after = _state(tr)
    assert any(k.startswith("field.") and int((_bits(before[k]) != _bits(after[k])).sum()) for k in before)
    # a scalar that is not finite — spread = inf on targets off the samples — and the step updates nothing
    tr.dataset.fetch = fetch
    tr.cfg.depth_spread = float("inf")
    stats = tr.train_step(2)
    torch.cuda.synchronize()
    assert stats is not None and not math.isfinite(stats["depth"])
    assert tr.step_guard.stats()["skipped"] == 1
    _same_bits({k: v for k, v in after.items() if k != "binaries"},
               {k: v for k, v in _state(tr).items() if k != "binaries"})
    tr.cfg.depth_spread = 1.0
    lines = []
    tr.train(steps=0, log=lines.append)
    assert len(lines) == 1 and " | skipped=1" in lines[0] and " | depth=" in lines[0]


def test_f_what_cannot_work_is_refused_at_construction(cuda, tmp_path, monkeypatch):
    from cnc_amd import dist as cdist
    from cnc_amd.trainer import Trainer

    class NoDepth:
        def update_num_rays(self, n):
            pass

    with pytest.raises(ValueError, match="measured depth"):
        Trainer(_cfg(tmp_path, depth_weight=1.0), device=cuda, dataset=NoDepth())
    with pytest.raises(ValueError, match="must be positive"):
        Trainer(_cfg(tmp_path, depth_weight=-1.0), device=cuda)
    with pytest.raises(ValueError, match="depth_spread"):
        Trainer(_cfg(tmp_path, depth_weight=1.0, depth_spread=-1.0), device=cuda)
    monkeypatch.setenv("CNC_DEPTH_WEIGHT", "0.5")
    assert Trainer(_cfg(tmp_path), device=cuda)._depth_weight == 0.5
    monkeypatch.delenv("CNC_DEPTH_WEIGHT")
    monkeypatch.setattr(cdist, "init", lambda: (0, 0, 2))           # what a second rank's process group would answer
    with pytest.raises(ValueError, match="data-parallel"):
        Trainer(_cfg(tmp_path, depth_weight=1.0), device=cuda)


def test_h_composes_with_the_distortion_loss(cuda, tmp_path):
    _, out, _ = _run(cuda, tmp_path, 3, depth_weight=0.01, distortion_weight=1e-2, guarded_step=True)
    taken = [o for o in out if o is not None]
    assert taken
    for o in taken:
        assert math.isfinite(o["depth"]) and o["depth"] > 0 and math.isfinite(o["distortion"]) and o["distortion"] > 0


def test_g_cli(cuda, tmp_path):
    argv = ["--dataset", "procedural", "--depth-weight", "0.1", "--depth-spread", "0.5", "--max_steps", "20", "--n_features", "2",
            "--sample_num", "20000", "--test_views", "1", "--log2_hashmap_size", "14", "--log2_hashmap_size_2D", "12",
            "--image_size", "48", "--results", str(tmp_path / "out.txt"), "--out_dir", str(tmp_path / "bits")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "cnc_amd.train"] + argv, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    logged = [ln for ln in r.stdout.splitlines() if ln.startswith("elapsed_time=")]
    assert logged and all(" | depth=" in ln for ln in logged)
    assert len(open(tmp_path / "out.txt").read().strip().split("\n")) == 1
