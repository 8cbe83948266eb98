"""GPU: the Trainer's learned background (`TrainConfig.background = "envmap"`) on the small configuration of
tests/test_gpu_reproducible_step.py, three steps.  The scene is the procedural ball in front of sky(d) = 1/2 + 1/2 d instead
of a flat colour, so the pixels are opaque.  "solid": no envmap object and no envmap launch; "envmap": the mirrors run once
per taken step, the texture moves inside [0, 1] and its Adam has moments; bit-reproducible under `reproducible`; its steps
are taken under `guarded_step`; bad options raise; a container carries the map to a fresh Trainer."""
import math

import pytest
import torch

from test_gpu_reproducible_step import _bits, _cfg, _state

pytestmark = pytest.mark.gpu
STEPS = 3


def _sky_dataset(cuda, cfg):
    from cnc_amd.datasets import SyntheticBallDataset
    from cnc_amd.render import Rays

    class BallUnderASky(SyntheticBallDataset):
        has_alpha = False        # every pixel is opaque: the sky stands where the parent class blends a colour

        @staticmethod
        def _sky(d):
            return 0.5 + 0.5 * d

        def fetch(self, num_rays=None):
            n = self.num_rays if num_rays is None else num_rays
            img = torch.randint(0, self.train_c2w.shape[0], (n,), device=self.device, generator=self.gen)
            xi = torch.randint(0, self.W, (n,), device=self.device, generator=self.gen)
            yi = torch.randint(0, self.H, (n,), device=self.device, generator=self.gen)
            o, d = self._rays(self.train_c2w[img], xi.float(), yi.float())
            rgb, alpha = self._shade(o, d)
            return {"rays": Rays(o, d), "pixels": rgb * alpha + self._sky(d) * (1 - alpha),
                    "color_bkgd": torch.ones(3, device=self.device)}

        def view(self, i):
            out = super().view(i)
            o, d = out["rays"].origins.reshape(-1, 3), out["rays"].viewdirs.reshape(-1, 3)
            rgb, alpha = self._shade(o, d)
            out["pixels"] = (rgb * alpha + self._sky(d) * (1 - alpha)).view(self.H, self.W, 3)
            return out

    return BallUnderASky(cfg.image_size, device=cuda, seed=cfg.seed)


def _trainer(cuda, tmp_path, **kw):
    from cnc_amd.trainer import Trainer
    torch.manual_seed(1234)
    cfg = _cfg(tmp_path, seed=3, **kw)
    tr = Trainer(cfg, device=cuda, dataset=_sky_dataset(cuda, cfg))
    g = torch.Generator(device=cuda)         # the context pass's window draw from a generator of its own (no race with the
    g.manual_seed(77)                        # sampler's on the default one when the mode is off)
    tr.context.rand_like = lambda t: torch.rand(t.shape, generator=g, device=t.device, dtype=t.dtype)
    return tr


def _full_state(tr):
    st = _state(tr)
    if tr.envmap is not None:
        st["envmap.texture"] = tr.envmap.texture.detach().clone()
        for k, v in tr.opt_env.state.get(tr.envmap.texture, {}).items():
            if isinstance(v, torch.Tensor):
                st[f"opt_env.{k}"] = v.detach().clone()
    return st


def _run(cuda, tmp_path, **kw):
    tr = _trainer(cuda, tmp_path, **kw)
    out = [tr.train_step(s) for s in range(STEPS)]
    torch.cuda.synchronize()
    return tr, out, _full_state(tr)


@pytest.fixture
def calls(monkeypatch):
    """Counts the calls of the three envmap mirrors."""
    from cnc_amd.backends import envmap_backend as K
    seen = {"envmap_forward": 0, "envmap_backward_rays": 0, "envmap_backward_texture": 0}

    def counted(name):
        fn = getattr(K, name)

        def call(*a, **k):
            seen[name] += 1
            return fn(*a, **k)
        return call

    for name in seen:
        monkeypatch.setattr(K, name, counted(name))
    return seen


def test_solid_calls_nothing_and_envmap_learns_a_texture(cuda, tmp_path, calls):
    tr, off, st_off = _run(cuda, tmp_path)
    assert tr.envmap is None and tr.opt_env is None and tr.cfg.background == "solid"
    assert calls == {"envmap_forward": 0, "envmap_backward_rays": 0, "envmap_backward_texture": 0}
    assert "envmap" not in tr.sizes_MB(0.0)
    tr, on, st = _run(cuda, tmp_path, background="envmap")
    taken = [o for o in on if o is not None]
    assert taken and calls["envmap_backward_rays"] == len(taken) and calls["envmap_backward_texture"] == len(taken)
    assert len(taken) <= calls["envmap_forward"] <= STEPS       # (the composite also runs in a step that then finds no samples)
    tex = st["envmap.texture"]
    assert tuple(tex.shape) == (16, 32, 3)
    assert bool(torch.isfinite(tex).all()) and float(tex.min()) >= 0.0 and float(tex.max()) <= 1.0
    assert int((tex != 0.5).sum()) > 0
    assert float(st["opt_env.exp_avg"].abs().sum()) > 0 and float(st["opt_env.exp_avg_sq"].abs().sum()) > 0
    assert float(st["opt_env.step"]) == len(taken)
    for o in taken:
        assert set(o) == {"mse", "psnr", "bpp", "embed_bits_MB", "n_rendering_samples", "num_rays"} and math.isfinite(o["mse"])
    assert tr.sizes_MB(0.0)["envmap"] == 16 * 32 * 3 / 1024.0 / 1024.0
    assert math.isfinite(tr.evaluate(1))


def test_reproducible_mode_gives_equal_bits(cuda, tmp_path, calls):
    _, out_a, st_a = _run(cuda, tmp_path, background="envmap", reproducible=True)
    _, out_b, st_b = _run(cuda, tmp_path, background="envmap", reproducible=True)
    assert calls["envmap_backward_texture"] > 0
    assert out_a == out_b and any(o is not None for o in out_a)
    assert set(st_a) == set(st_b) and {"envmap.texture", "opt_env.exp_avg", "opt_env.exp_avg_sq"} <= set(st_a)
    for k in st_a:
        assert int((_bits(st_a[k]) != _bits(st_b[k])).sum()) == 0, k


def test_guarded_steps_are_taken(cuda, tmp_path, calls):
    tr, out, st = _run(cuda, tmp_path, background="envmap", guarded_step=True)
    assert calls["envmap_backward_texture"] > 0 and tr.step_guard is not None
    assert tr.step_guard.stats()["skipped"] == 0
    assert tr.opt_env.found_inf is tr.step_guard.found_inf
    assert int((st["envmap.texture"] != 0.5).sum()) > 0 and float(st["opt_env.exp_avg"].abs().sum()) > 0
    assert any(k.endswith("exp_avg") and k.startswith("opt.") and float(v.abs().sum()) > 0 for k, v in st.items())


def test_alpha_warning_follows_what_the_dataset_says(cuda, tmp_path):
    import warnings
    from cnc_amd.trainer import Trainer
    with pytest.warns(UserWarning, match="alpha below 1"):          # the procedural ball: transparent where rays miss it
        Trainer(_cfg(tmp_path, background="envmap"), device=cuda)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        _trainer(cuda, tmp_path, background="envmap")               # the opaque ball under a sky: has_alpha = False
        Trainer(_cfg(tmp_path), device=cuda)                        # no map, nothing to warn about
    assert not [w for w in seen if "alpha below 1" in str(w.message)]


def test_bad_options_raise(cuda, tmp_path, monkeypatch):
    from cnc_amd import dist as cdist
    from cnc_amd.trainer import Trainer
    with pytest.raises(ValueError, match="background"):
        Trainer(_cfg(tmp_path, background="sky"), device=cuda)
    for bad in (1, 7, 66):
        with pytest.raises(ValueError, match="resolution"):
            Trainer(_cfg(tmp_path, background="envmap", envmap_resolution=bad), device=cuda)
    monkeypatch.setattr(cdist, "init", lambda: (0, 0, 2))           # what a second rank's process group would answer
    with pytest.raises(ValueError, match="data-parallel"):
        Trainer(_cfg(tmp_path, background="envmap"), device=cuda)


def test_container_carries_the_map_to_a_fresh_trainer(cuda, tmp_path, calls):
    from cnc_amd.container import read_envmap, section_sizes
    tr, _, _ = _run(cuda, tmp_path, background="envmap", envmap_resolution=8)
    path = str(tmp_path / "scene.cnc")
    tr.save_container(path)
    assert section_sizes(path)["envmap"] == 8 * 16 * 3
    q = tr.envmap.quantized()
    assert torch.equal(read_envmap(path), q.cpu())
    fresh = _trainer(cuda, tmp_path, background="envmap", envmap_resolution=8)
    fresh.load_container(path)
    assert torch.equal(fresh.envmap.texture.detach(), q.float() / 255.0)
    assert math.isfinite(fresh.evaluate(1))
    # the mismatches, both ways round, and another resolution
    solid = _trainer(cuda, tmp_path)
    with pytest.raises(RuntimeError, match="background"):
        solid.load_container(path)
    plain = str(tmp_path / "plain.cnc")
    solid.save_container(plain)
    assert "envmap" not in section_sizes(plain) and read_envmap(plain) is None
    with pytest.raises(RuntimeError, match="background"):
        fresh.load_container(plain)
    other = _trainer(cuda, tmp_path, background="envmap", envmap_resolution=4)
    assert bool((fresh.envmap.texture == q.float() / 255.0).all())       # a refused load left the map as it was
    with pytest.raises(RuntimeError, match="envmap_resolution"):
        other.load_container(path)
