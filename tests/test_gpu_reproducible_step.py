"""The reproducible training step (`TrainConfig.reproducible`, cnc_amd._repro): two Trainers from one seed give the same
bits for 20 steps (across the occupancy refresh at step 16) — every entry of every step's result, every parameter, every
Adam moment, the occupancy grid — the second one next to a side stream kept busy with large matmuls.  With the mode off no
ordered route runs, and the first steps agree with the mode's within the bounds
tests/test_gpu_trainer.py::test_threaded_context_pass_equals_the_sequential_schedule holds its schedules to."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _cfg(tmp_path, **kw):
    from cnc_amd.trainer import TrainConfig
    base = dict(lmbda=2e-3, Pg_level=5, Pg_level_2D=3, log2_hashmap_size=12, log2_hashmap_size_2D=9,
                sample_num=3000, max_context_layer_num=3, n_features=2, n_neurons=32,
                resolutions_list=(10, 14, 18, 26, 34), resolutions_list_2D=(18, 34, 66),
                skip_levels_3D=(0, 1, 2), skip_levels_2D=(0,), max_steps=150, init_batch_size=512,
                target_sample_batch_size=1 << 14, grid_resolution=16, render_step_size=2e-2,
                milestones=(100, 130), warmup_iters=20, test_views=2, image_size=48,
                out_dir=str(tmp_path / "bits"), log_every=50)
    base.update(kw)
    return TrainConfig(**base)


def _state(tr):
    out = {}
    for name, mod in (("field", tr.field), ("context", tr.context)):
        for n, p in mod.named_parameters():
            out[f"{name}.{n}"] = p.detach().clone()
    for oname, opt in (("opt", tr.opt), ("opt2", tr.opt2)):
        for gi, group in enumerate(opt.param_groups):
            for pi, p in enumerate(group["params"]):
                for k, v in opt.state.get(p, {}).items():
                    if isinstance(v, torch.Tensor):
                        out[f"{oname}.{gi}.{pi}.{k}"] = v.detach().clone()
    out["binaries"] = tr.estimator.binaries.detach().clone()
    return out


def _run(cuda, tmp_path, steps, interfere=False, own_draws=False, **kw):
    from cnc_amd.trainer import Trainer
    torch.manual_seed(1234)
    tr = Trainer(_cfg(tmp_path, seed=3, **kw), device=cuda)
    if own_draws:        # the context pass's window draw from a generator of its own: no race with the sampler's (mode off)
        g = torch.Generator(device=cuda)
        g.manual_seed(77)
        tr.context.rand_like = lambda t: torch.rand(t.shape, generator=g, device=t.device, dtype=t.dtype)
    side = torch.cuda.Stream(cuda) if interfere else None
    m = torch.full((4096, 4096), 0.5, device=cuda) if interfere else None      # (no draw from the default generator)
    out = []
    for s in range(steps):
        if side is not None:
            with torch.cuda.stream(side):
                for _ in range(8):
                    m @ m
        out.append(tr.train_step(s))
    torch.cuda.synchronize()
    return tr, out, _state(tr)


def _bits(t):
    return t.reshape(-1).view(torch.uint8) if t.dtype == torch.bool else t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("shape", ["unfused_h32", "fused_f2_h64"])
def test_two_trainers_from_one_seed_give_the_same_bits(cuda, tmp_path, shape):
    from cnc_amd import _repro
    from cnc_amd.backends.gridencoder_backend import ROUTE_CALLS
    kw = {} if shape == "unfused_h32" else dict(n_features=2, n_neurons=64)
    before, enc_before = dict(_repro.ROUTE_CALLS), dict(ROUTE_CALLS)
    tr_a, out_a, st_a = _run(cuda, tmp_path, 20, reproducible=True, **kw)
    assert tr_a.ctx_stream is None and tr_a.planes_graph is None and not tr_a.ctx_thread
    assert _repro.ROUTE_CALLS["ctx_ordered"] > before["ctx_ordered"] and _repro.ROUTE_CALLS["ctx_default"] == before["ctx_default"]
    assert _repro.ROUTE_CALLS["field_default"] == before["field_default"]
    assert ROUTE_CALLS["ordered"] > enc_before["ordered"] and ROUTE_CALLS["default"] == enc_before["default"]
    if shape == "fused_f2_h64":
        assert _repro.ROUTE_CALLS["field_ordered"] > before["field_ordered"]
    assert not _repro.explicitly_enabled()                 # the Trainer holds the mode for its steps only
    tr_b, out_b, st_b = _run(cuda, tmp_path, 20, interfere=True, reproducible=True, **kw)
    assert sum(o is not None for o in out_a) >= 18
    for s, (a, b) in enumerate(zip(out_a, out_b)):
        assert (a is None) == (b is None), s
        if a is not None:
            assert set(a) == set(b)
            for k in a:
                assert a[k] == b[k], (s, k, a[k], b[k])
    assert set(st_a) == set(st_b)
    assert any(k.endswith("exp_avg_sq") for k in st_a) and any(k.startswith("opt2.") for k in st_a)
    for k in st_a:
        differ = int((_bits(st_a[k]) != _bits(st_b[k])).sum())
        assert differ == 0, (k, differ)


def test_mode_off_runs_no_ordered_route_and_agrees_with_the_mode(cuda, tmp_path):
    from cnc_amd import _repro
    from cnc_amd.backends.gridencoder_backend import ROUTE_CALLS
    before, enc_before = dict(_repro.ROUTE_CALLS), dict(ROUTE_CALLS)
    tr, off, _ = _run(cuda, tmp_path, 4, own_draws=True)
    assert tr.reproducible is False
    assert _repro.ROUTE_CALLS["ctx_ordered"] == before["ctx_ordered"] and _repro.ROUTE_CALLS["field_ordered"] == before["field_ordered"]
    assert ROUTE_CALLS["ordered"] == enc_before["ordered"]
    assert _repro.ROUTE_CALLS["ctx_default"] > before["ctx_default"] and ROUTE_CALLS["default"] > enc_before["default"]
    _, on, _ = _run(cuda, tmp_path, 4, own_draws=True, reproducible=True)
    for a, b in zip(off, on):
        assert a["n_rendering_samples"] == b["n_rendering_samples"] and a["num_rays"] == b["num_rays"]
        assert abs(a["mse"] - b["mse"]) <= 1e-5 * max(a["mse"], 1e-6) + 1e-9
        assert abs(a["bpp"] - b["bpp"]) <= 1e-5 * a["bpp"]
