"""CPU: the proposal-network twin (tests/propnet_twin.py) against numbers the reference's pure-torch helpers returned
(tests/golden/propnet_outer.npz, written by tests/golden/make_golden_propnet.py), against the searchsorted form of the
outer weights, and the package's training schedule and transform against the same golden numbers."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import propnet_twin as P

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "propnet_outer.npz"))


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_golden_propnet",
                                                  os.path.join(HERE, "golden", "make_golden_propnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _schedule(golden, j):
    return np.unpackbits(golden[f"schedule_{j}"])[:int(golden["n_steps"])].astype(bool)


def test_golden_matches_its_generator(golden, generator):
    assert golden["outer_cases"].tolist() == [list(c) for c in generator.OUTER_CASES]
    assert golden["schedules"].tolist() == [list(c) for c in generator.SCHEDULES]
    assert golden["ranges"].tolist() == [list(c) for c in generator.RANGES]
    assert int(golden["n_steps"]) == 2500 and int(golden["transform_seed"]) == generator.TRANSFORM_SEED


def test_outer_weights_against_the_reference_measure(golden):
    """Within 1e-12: the reference sums the key weights it is given (a running sum of float64 differences), the twin
    multiplies them by a mask."""
    for i, (seed, n_rays, n_key, n_query) in enumerate(golden["outer_cases"].tolist()):
        key, cdf, q = (torch.from_numpy(x) for x in P.histograms(seed, n_rays, n_key, n_query))
        got = P.outer_weights(q, key, cdf).numpy()
        want = golden[f"outer_{i}"]
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12, (i, np.abs(got - want).max())


def test_outer_weights_against_the_searchsorted_form(golden):
    """The overlap sum with its zero-width exception selects the same key intervals as cdf[right] - cdf[left]."""
    exceptions = 0
    for seed, n_rays, n_key, n_query in golden["outer_cases"].tolist() + [[11, 40, 9, 12], [12, 40, 5, 40]]:
        key, cdf, q = (torch.from_numpy(x) for x in P.histograms(seed, n_rays, n_key, n_query))
        a = P.outer_weights(q, key, cdf).numpy()
        b = P.outer_weights_searchsorted(q, key, cdf).numpy()
        assert np.abs(a - b).max() <= 1e-12, (seed, np.abs(a - b).max())
        lo, hi = P.bracket(q, key)
        mask = P.overlap_mask(q, key).numpy()
        k = np.arange(n_key - 1)
        assert np.array_equal(mask, (k >= lo.numpy()[..., None]) & (k < hi.numpy()[..., None]))
        exceptions += int((q[:, :-1] >= key[:, -1:]).sum())
    assert exceptions > 0          # the zero-width interval on the key's last edge occurs


def test_zero_width_exception_is_the_last_key_weight():
    key = torch.tensor([[0.0, 0.25, 1.0]], dtype=torch.float64)
    cdf = torch.tensor([[0.0, 0.3, 1.0]], dtype=torch.float64)
    q = torch.tensor([[0.0, 0.0, 0.25, 0.25, 1.0, 1.0]], dtype=torch.float64)
    # [0, 0] lies in interval 0; [0, .25] touches both; [.25, .25] and [.25, 1] lie in the second (a key interval holds
    # its left edge, not its right one); [1, 1] is the exception
    assert P.outer_weights(q, key, cdf).tolist() == [[0.3, 1.0, 0.7, 0.7, 0.7]]
    assert P.outer_weights_searchsorted(q, key, cdf).tolist() == [[0.3, 1.0, 0.7, 0.7, 0.7]]


def test_outer_weights_refuses_edges_outside_the_key():
    key = torch.tensor([[0.2, 0.5, 0.8]], dtype=torch.float64)
    cdf = torch.tensor([[0.0, 0.5, 1.0]], dtype=torch.float64)
    for q in ([[0.1, 0.5]], [[0.3, 0.9]]):
        with pytest.raises(ValueError):
            P.outer_weights(torch.tensor(q, dtype=torch.float64), key, cdf)


def test_outer_weights_gradient_is_the_mask():
    key, cdf, q = (torch.from_numpy(x) for x in P.histograms(21, 6, 9, 7))
    cdf.requires_grad_(True)
    g = torch.from_numpy(np.random.default_rng(0).normal(size=(6, 6)))
    (P.outer_weights(q, key, cdf) * g).sum().backward()
    lo, hi = P.bracket(q, key)
    want = torch.zeros_like(cdf).scatter_add_(-1, hi, g).scatter_add_(-1, lo, -g)
    assert torch.allclose(cdf.grad, want, rtol=0, atol=1e-14)


def test_transform_against_the_reference(golden, generator):
    """Within 4 float64 ulp of the result (the same formula; the order of its operations may differ)."""
    s = torch.from_numpy(generator.transform_inputs())
    for j, (t_min, t_max) in enumerate(golden["ranges"].tolist()):
        for kind in ("uniform", "lindisp"):
            got, want = P.transform_stot(kind, s, t_min, t_max).numpy(), golden[f"stot_{kind}_{j}"]
            assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all(), (kind, j)
            # the inverse pair: s -> t -> s, to the conditioning of the map (|ds/dt| t eps per rounding)
            back = P.transform_ttos(kind, torch.from_numpy(want), t_min, t_max).numpy()
            assert np.abs(back - s.numpy()).max() <= 64 * np.finfo(np.float64).eps * t_max / t_min, (kind, j)
            assert abs(got[0] - t_min) <= 2 * np.spacing(t_min) and abs(got[-1] - t_max) <= 2 * np.spacing(t_max)


def test_package_transform_against_the_reference(golden, generator):
    from cnc_amd.nerfacc.estimators.prop_net import _transform_stot
    s = torch.from_numpy(generator.transform_inputs())
    for j, (t_min, t_max) in enumerate(golden["ranges"].tolist()):
        for kind in ("uniform", "lindisp"):
            got, want = _transform_stot(kind, s, t_min, t_max).numpy(), golden[f"stot_{kind}_{j}"]
            assert (np.abs(got - want) <= 4 * np.spacing(np.abs(want))).all(), (kind, j)
    with pytest.raises(ValueError):
        _transform_stot("log", s, 1.0, 2.0)


@pytest.mark.parametrize("j", [0, 1])
def test_schedule_against_the_reference(golden, j):
    from cnc_amd.nerfacc.estimators.prop_net import get_proposal_requires_grad_fn
    target, num_steps = golden["schedules"][j].tolist()
    want = _schedule(golden, j)
    steps = list(range(int(golden["n_steps"])))
    assert want.any() and not want.all()
    assert P.requires_grad_schedule(steps, target, int(num_steps)) == want.tolist()
    fn = get_proposal_requires_grad_fn(target, int(num_steps))
    assert [fn(step) for step in steps] == want.tolist()
    # past num_steps the gap is `target` steps: one training step in every target + 1
    tail = want[int(num_steps) + 10:]
    period = int(target) + 1
    assert tail[:period * 20].reshape(20, period).sum(1).tolist() == [1] * 20


def test_compute_loss_takes_the_levels_last_to_first_and_detaches_the_target():
    key1, cdf1, q = (torch.from_numpy(x) for x in P.histograms(31, 5, 33, 17))
    key2, cdf2, _ = (torch.from_numpy(x) for x in P.histograms(32, 5, 17, 17))
    lo = torch.maximum(key1[:, :1], key2[:, :1])
    hi = torch.minimum(key1[:, -1:], key2[:, -1:])
    q = lo + (q - q[:, :1]) / (q[:, -1:] - q[:, :1]) * (hi - lo)
    q = torch.minimum(torch.maximum(q, lo), hi)
    trans = torch.from_numpy(np.sort(np.random.default_rng(1).uniform(size=(5, 16)), -1)[:, ::-1].copy())
    trans.requires_grad_(True)
    cdf1.requires_grad_(True)
    cdf2.requires_grad_(True)
    total = P.compute_loss([(key1, cdf1), (key2, cdf2)], q, trans, 3.0)
    target = P.opacity_cdf(trans.detach())
    parts = [P.pdf_loss(q, target, k, c)[0].mean() for k, c in ((key2, cdf2), (key1, cdf1))]
    assert total.item() == ((0.0 + parts[0] + parts[1]) * 3.0).item() and total.item() > 0
    total.backward()
    assert trans.grad is None and cdf1.grad.abs().sum() > 0 and cdf2.grad.abs().sum() > 0
    assert float(P.compute_loss([], q, trans)) == 0.0


def test_bounds_hold_for_the_float32_twin():
    """The derived bounds against the twin itself run in float32 (they are derived, not fitted: this only shows that
    the derivation is not too tight for a plain float32 evaluation)."""
    worst = 0.0
    for seed, n_key, n_query in ((41, 33, 17), (42, 65, 130), (43, 3, 65)):
        key, cdf, q = P.histograms(seed, 65, n_key, n_query, np.float32)
        rng = np.random.default_rng(seed)
        cq = np.sort(rng.uniform(size=q.shape), -1).astype(np.float32)
        cq[:, 0], cq[:, -1] = 0.0, 1.0
        t = lambda x, dt: torch.from_numpy(x).to(dt)        # noqa: E731
        c64 = t(cdf, torch.float64).requires_grad_(True)
        c32 = t(cdf, torch.float32).requires_grad_(True)
        l64, w, wo = P.pdf_loss(t(q, torch.float64), t(cq, torch.float64), t(key, torch.float64), c64)
        l32, _, _ = P.pdf_loss(t(q, torch.float32), t(cq, torch.float32), t(key, torch.float32), c32,
                               outer=P.outer_weights_searchsorted)
        bound = P.loss_bound(w.detach().numpy(), wo.detach().numpy())
        err = np.abs(l32.detach().numpy().astype(np.float64) - l64.detach().numpy())
        assert (err <= bound).all()
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (l32.detach().numpy()[(w <= wo).numpy()] == 0).all()
    assert 0.0 < worst <= 1.0


def test_transmittance_and_opacity_cdf():
    t = torch.tensor([[1.0, 2.0, 4.0, 7.0]], dtype=torch.float64)
    sigma = torch.tensor([[0.5, 0.0, 2.0]], dtype=torch.float64)
    T = P.transmittance(t[:, :-1], t[:, 1:], sigma)
    assert torch.allclose(T, torch.exp(-torch.tensor([[0.0, 0.5, 0.5]], dtype=torch.float64)), rtol=0, atol=1e-16)
    cdf = P.opacity_cdf(T)
    assert cdf.shape == (1, 4) and cdf[0, 0] == 0 and cdf[0, -1] == 1
    from cnc_amd.nerfacc.estimators.prop_net import _opacity_cdf
    assert torch.equal(_opacity_cdf(T), cdf)
