"""GPU: the Trainer's distortion regulariser (`TrainConfig.distortion_weight`) on the small configuration of
tests/test_gpu_reproducible_step.py, three steps: off, it runs no distortion kernel; on, the stats carry the term and the
parameters move differently; it is bit-reproducible under `reproducible`, and its steps are taken under `guarded_step`."""
import math

import pytest
import torch

from test_gpu_reproducible_step import _bits, _cfg, _state

pytestmark = pytest.mark.gpu
STEPS = 3


def _run(cuda, tmp_path, **kw):
    from cnc_amd.trainer import Trainer
    torch.manual_seed(1234)
    tr = Trainer(_cfg(tmp_path, seed=3, **kw), device=cuda)
    g = torch.Generator(device=cuda)         # the context pass's window draw from a generator of its own (no race with the
    g.manual_seed(77)                        # sampler's on the default one when the mode is off)
    tr.context.rand_like = lambda t: torch.rand(t.shape, generator=g, device=t.device, dtype=t.dtype)
    out = [tr.train_step(s) for s in range(STEPS)]
    torch.cuda.synchronize()
    return tr, out, _state(tr)


@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of the two distortion mirrors."""
    from cnc_amd.backends import volrend_backend as K
    seen = {"forward": 0, "backward": 0}
    fwd, bwd = K.distortion_forward, K.distortion_backward

    def forward(*a, **k):
        seen["forward"] += 1
        return fwd(*a, **k)

    def backward(*a, **k):
        seen["backward"] += 1
        return bwd(*a, **k)

    monkeypatch.setattr(K, "distortion_forward", forward)
    monkeypatch.setattr(K, "distortion_backward", backward)
    return seen


def test_weight_zero_calls_nothing_and_a_weight_changes_the_steps(cuda, tmp_path, calls):
    _, off, st_off = _run(cuda, tmp_path)
    assert calls == {"forward": 0, "backward": 0}
    assert all(o is None or "distortion" not in o for o in off)
    _, on, st_on = _run(cuda, tmp_path, distortion_weight=1e-2)
    taken = [o for o in on if o is not None]
    assert taken and calls["forward"] == len(taken) and calls["backward"] == len(taken)
    for o in taken:
        assert math.isfinite(o["distortion"]) and o["distortion"] > 0
        assert set(o) == {"mse", "psnr", "bpp", "embed_bits_MB", "n_rendering_samples", "num_rays", "distortion"}
    moved = [k for k in st_off if k.startswith("field.") and int((_bits(st_off[k]) != _bits(st_on[k])).sum())]
    assert moved


def test_reproducible_mode_gives_equal_bits(cuda, tmp_path, calls):
    _, out_a, st_a = _run(cuda, tmp_path, distortion_weight=1e-2, reproducible=True)
    _, out_b, st_b = _run(cuda, tmp_path, distortion_weight=1e-2, reproducible=True)
    assert calls["backward"] > 0
    assert out_a == out_b and any(o is not None for o in out_a)
    assert set(st_a) == set(st_b)
    for k in st_a:
        assert int((_bits(st_a[k]) != _bits(st_b[k])).sum()) == 0, k


def test_guarded_steps_are_taken(cuda, tmp_path, calls):
    tr, out, st = _run(cuda, tmp_path, distortion_weight=1e-2, guarded_step=True)
    assert calls["backward"] > 0 and tr.step_guard is not None
    assert tr.step_guard.stats()["skipped"] == 0
    assert any(o is not None and o["distortion"] > 0 for o in out)
    assert any(k.endswith("exp_avg") and float(v.abs().sum()) > 0 for k, v in st.items())      # updates were applied
