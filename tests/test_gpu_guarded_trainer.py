"""The guarded training step (`TrainConfig.guarded_step`, cnc_amd._step_guard) through the Trainer, on the small procedural
configuration of tests/test_gpu_trainer.py with the fused training forward (n_features = 2, n_neurons = 64) and
`reproducible=True`: the first step equals the unguarded one bit for bit; a batch with one NaN pixel, and a forward that
trips the fp16 range guard, move nothing — parameters, both optimizers' moments and step counts, the encoders' sign planes
and clip counters — and the step after a skipped one goes ahead; with the mode off the same NaN batch leaves non-finite
moments behind (the control: the assertions of the skip tests can fail)."""
import warnings

import pytest
import torch

import test_gpu_reproducible_step as R

pytestmark = pytest.mark.gpu

NONFINITE, RANGE_GUARD = 1, 2
SHAPE = dict(n_features=2, n_neurons=64)


def _trainer(cuda, tmp_path, **kw):
    from cnc_amd.trainer import Trainer
    torch.manual_seed(1234)
    return Trainer(R._cfg(tmp_path, seed=3, reproducible=True, **SHAPE, **kw), device=cuda)


def _everything(tr):
    """Every parameter, every optimizer state tensor (exp_avg, exp_avg_sq, step), the occupancy grid, and the encoders' sign
    planes and clip counters."""
    torch.cuda.synchronize()
    out = R._state(tr)
    for k, e in enumerate(tr.field.mlp_base._encoders()):
        for name in ("_bits", "_clip_count"):
            t = getattr(e, name, None)
            if isinstance(t, torch.Tensor):
                out[f"encoder{k}.{name}"] = t.detach().clone()
    return out


def _differing(a, b):
    assert set(a) == set(b)
    return [k for k in a if a[k].shape != b[k].shape or int((R._bits(a[k]) != R._bits(b[k])).sum())]


def _steps(state):
    return {k: float(v) for k, v in state.items() if k.endswith(".step")}


def _nan_batch(tr):
    data = dict(tr.dataset.fetch())
    pixels = data["pixels"].clone()
    pixels.view(-1)[pixels.numel() // 2] = float("nan")
    data["pixels"] = pixels
    return data


def test_first_step_equals_the_unguarded_step(cuda, tmp_path):
    """t = 1: the running product b^1 IS pow(b, 1), `found_inf` = 0 leaves torch's fused Adam its arithmetic: every
    parameter and moment bit-equal, mode on against mode off."""
    states = []
    for guarded in (False, True):
        tr = _trainer(cuda, tmp_path, guarded_step=guarded)
        assert (tr.step_guard is not None) == guarded
        out = tr.train_step(0)
        assert out is not None
        states.append(_everything(tr))
        if guarded:
            assert tr.step_guard.stats() == {"skipped": 0, "reasons": 0}
            assert tr.table_adam is not None and tr.fused_table_adam, "the tables did not go through the guarded kernel"
    assert any(k.endswith("exp_avg_sq") for k in states[0]) and any(k.startswith("encoder") for k in states[0])
    assert _differing(states[0], states[1]) == []


def test_nan_pixel_batch_updates_nothing(cuda, tmp_path):
    tr = _trainer(cuda, tmp_path, guarded_step=True)
    for s in range(3):
        assert tr.train_step(s) is not None
    assert tr.step_guard.stats() == {"skipped": 0, "reasons": 0}
    before = _everything(tr)
    assert any(k.startswith("opt2.") and k.endswith("exp_avg") for k in before) and any(k.startswith("encoder") for k in before)
    tr._next_data = _nan_batch(tr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = tr.train_step(3)
    after = _everything(tr)
    stats = tr.step_guard.stats()
    print("stats after the NaN batch:", stats, "differing:", _differing(before, after)[:8])
    assert out is not None and out["mse"] != out["mse"]                    # the step did see the NaN
    assert _differing(before, after) == []
    assert stats == {"skipped": 1, "reasons": NONFINITE}
    assert float(tr.step_guard.found_inf) == 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert tr.train_step(4) is not None                                # a clean batch: the step goes ahead
    later = _everything(tr)
    moved = _differing(before, later)
    params = [k for k in before if k.startswith("field.")]
    assert all(k in moved for k in params), [k for k in params if k not in moved]
    assert sum(k in moved for k in before if k.startswith("context.")) >= 1
    assert _steps(later) == {k: v + 1.0 for k, v in _steps(before).items()} and len(_steps(before)) > 10
    assert all(bool(torch.isfinite(v.float()).all()) for v in later.values())
    assert tr.step_guard.stats() == {"skipped": 1, "reasons": NONFINITE} and float(tr.step_guard.found_inf) == 0.0
    assert tr.table_adam.steps_done == 5                                   # attempts; the device counts 4
    tr.table_adam.resync()
    assert tr.table_adam.steps_done == 4


def test_range_guard_trip_updates_nothing(cuda, tmp_path):
    tr = _trainer(cuda, tmp_path, guarded_step=True)
    for s in range(3):
        assert tr.train_step(s) is not None
    f = tr.field
    assert f.fused_train and f._field_fused and f._field_fused._train_calls, "the fused training forward did not run"
    with torch.no_grad():                                                  # hidden activations past fp16's 65504
        f.mlp_base.network[0].weight.mul_(300.0)
        f.mlp_base.network[0].bias.fill_(7.0e4)
        f.mlp_base.network[2].weight.mul_(1.0e-5)
    before = _everything(tr)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = tr.train_step(3)
    after = _everything(tr)
    stats = tr.step_guard.stats()
    print("stats after the saturating forward:", stats, "differing:", _differing(before, after)[:8])
    assert out is not None
    assert _differing(before, after) == []
    assert stats == {"skipped": 1, "reasons": RANGE_GUARD}
    assert f.fused_train                                                   # the host has not looked yet ...
    torch.cuda.synchronize()
    with pytest.warns(UserWarning, match="left fp16's range"):
        assert f.poll_range_guard()                                        # ... and finds it at the next poll, as before
    assert not f.fused_train


def test_control_the_unguarded_step_lets_the_nan_through(cuda, tmp_path):
    tr = _trainer(cuda, tmp_path, guarded_step=False)
    for s in range(3):
        assert tr.train_step(s) is not None
    before = _everything(tr)
    tr._next_data = _nan_batch(tr)
    tr.train_step(3)
    after = _everything(tr)
    assert _differing(before, after) != []
    bad = [k for k, v in after.items() if k.endswith(("exp_avg", "exp_avg_sq")) and not bool(torch.isfinite(v).all())]
    assert bad, "the NaN batch left every moment finite: the skip tests' assertions could not fail"
