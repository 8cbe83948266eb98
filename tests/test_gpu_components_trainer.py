"""`Trainer.prune_floaters` on the small configuration of tests/test_gpu_mesh_trainer.py, 120 steps on the
procedural ball.  Nothing here depends on the ball having floaters after 120 steps: they are planted — a singleton in one
cleared corner block, a (+1, +1, -1) pair in the opposite one — and the pruned grid must be the NumPy twin's prune of that
very grid.  With the option off nothing may differ from a run that never heard of it."""
import collections
import math

import numpy as np
import pytest
import torch

import components_twin as T
from test_gpu_mesh_trainer import _cfg

pytestmark = pytest.mark.gpu

TABLES = (lambda t: (t.encoding_xyz, t.encoding_xy, t.encoding_xz, t.encoding_yz))


def _plant(tr):
    """-> the planted grid (host bool), installed in the estimator with `occs` to match."""
    est = tr.estimator
    b = est.binaries.clone()
    assert tuple(b.shape) == (1, 16, 16, 16)
    b[:, 0:5, 0:5, 0:5] = False
    b[:, 2, 2, 2] = True                                  # a singleton at every connectivity
    b[:, 11:16, 11:16, 11:16] = False
    b[:, 13, 13, 13] = True                               # a pair that only the 26 neighbourhood joins
    b[:, 14, 14, 12] = True
    occs = est.occs.view(b.shape)
    occs[b & (occs <= 0)] = 1.0
    occs[~b] = 0.0
    est.binaries = b
    return b.cpu().numpy()


@pytest.fixture(scope="module")
def trained(cuda, tmp_path_factory):
    from cnc_amd.trainer import Trainer
    tmp = tmp_path_factory.mktemp("prune")
    tr = Trainer(_cfg(tmp), device=cuda)
    tr.train(steps=120, log=None)
    return tr, tmp


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
def test_prune_floaters_equals_the_twins_prune(trained, connectivity):
    tr, _ = trained
    est = tr.estimator
    planted = _plant(tr)
    want, want_stats = T.prune_small(planted, 3, connectivity)
    address, occs_before = est.binaries.data_ptr(), est.occs.clone()
    all_visible = est._all_visible()
    stats = tr.prune_floaters(min_cells=3, connectivity=connectivity)
    got = est.binaries
    assert got.dtype == torch.bool and tuple(got.shape) == planted.shape and got.data_ptr() != address       # a new tensor
    assert np.array_equal(got.cpu().numpy(), want) and stats == want_stats
    assert stats["removed_components"] >= 2 and stats["removed_cells"] >= 3
    assert not got[0, 2, 2, 2] and not got[0, 13, 13, 13] and not got[0, 14, 14, 12]
    cleared = torch.from_numpy(planted & ~want).to(got.device).view(-1)
    assert bool((est.occs[cleared] == 0).all()) and torch.equal(est.occs[~cleared], occs_before[~cleared])
    assert bool((est.occs >= 0).all()) and est._all_visible() == all_visible
    assert getattr(est, "_vis_key", None) == (id(est.occs), est.occs._version)            # the cache was kept, not rebuilt
    # pruning again finds nothing to do
    again = tr.prune_floaters(min_cells=3, connectivity=connectivity)
    assert again["removed_cells"] == 0 and again["components"] == stats["components"] - stats["removed_components"]
    assert np.array_equal(est.binaries.cpu().numpy(), want)
    assert math.isfinite(tr.evaluate())


def test_config_defaults_and_the_pruned_container(trained, cuda):
    from cnc_amd.trainer import TrainConfig, Trainer
    tr, tmp = trained
    assert TrainConfig().prune_floaters == 0 and TrainConfig().prune_connectivity == 26
    planted = _plant(tr)
    tr.cfg.prune_floaters, tr.cfg.prune_connectivity = 3, 14
    try:
        stats = tr.prune_floaters()                                   # the arguments default to the configuration's
    finally:
        tr.cfg.prune_floaters, tr.cfg.prune_connectivity = 0, 26
    want, want_stats = T.prune_small(planted, 3, 14)
    assert stats == want_stats and np.array_equal(tr.estimator.binaries.cpu().numpy(), want)
    path = str(tmp / "pruned.cnc")
    tr.save_container(path)
    orig = [torch.where(t.params.data >= 0, 1.0, -1.0) for t in TABLES(tr.field.mlp_base)]
    fresh = Trainer(_cfg(tmp, seed=7), device=cuda)
    fresh.load_container(path)
    assert torch.equal(fresh.estimator.binaries, tr.estimator.binaries) and fresh.estimator.binaries.dtype == torch.bool
    for t, o in zip(TABLES(fresh.field.mlp_base), orig):
        dec = t.params.data
        uncoded = (dec == 1).all(dim=1)
        assert torch.all(dec.abs() == 1) and torch.equal(dec[~uncoded], o[~uncoded])
    assert math.isfinite(fresh.evaluate())
    with pytest.raises(ValueError):
        Trainer(_cfg(tmp, prune_connectivity=8), device=cuda)
    with pytest.raises(RuntimeError, match="connectivity"):
        tr.prune_floaters(min_cells=3, connectivity=8)


class _Counting:
    """The HIP library with every entry-point call counted."""

    def __init__(self, real):
        self.real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("cnc_"):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted


def test_off_is_a_run_that_never_heard_of_the_option(cuda, tmp_path, monkeypatch):
    """Two reproducible runs from one seed, 40 steps: the configuration built without the two fields, and with
    prune_floaters=0 spelled out.  The grid, `occs`, the container's bytes and the calls into the HIP library made by the
    tail (evaluate, save_container; counted per entry point) are the same, and no components entry point is among them."""
    from cnc_amd import _lib
    from cnc_amd.nerfacc.estimators.occ_grid import OccGridEstimator
    from cnc_amd.trainer import Trainer

    def never(*a, **k):
        raise AssertionError("prune_small_components was called with the option off")
    monkeypatch.setattr(OccGridEstimator, "prune_small_components", never)
    runs = []
    for i, kw in enumerate(({}, dict(prune_floaters=0, prune_connectivity=26))):
        tr = Trainer(_cfg(tmp_path / f"run{i}", reproducible=True, **kw), device=cuda)
        tr.train(steps=40, log=None)
        counting = _Counting(_lib.lib())
        monkeypatch.setattr(_lib, "_lib", counting)
        try:
            psnr = tr.evaluate()
            path = str(tmp_path / f"run{i}.cnc")
            tr.save_container(path)
        finally:
            monkeypatch.setattr(_lib, "_lib", counting.real)
        runs.append((tr.estimator.binaries.clone(), tr.estimator.occs.clone(), open(path, "rb").read(), counting.calls, psnr))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and len(a[2]) > 0
    assert a[3] == b[3] and sum(a[3].values()) > 0 and not [n for n in a[3] if "components" in n]
    assert a[4] == b[4]
