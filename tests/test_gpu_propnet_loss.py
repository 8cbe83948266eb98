"""GPU: what is built on the proposal-sampling kernels (cnc_amd/csrc/pdf.hip) — `_pdf_loss` in its batched and
flattened forms, `PropNetEstimator.compute_loss`, the wiring of `sampling`, the gradients of a proposal network through
both, and the batched route of `rendering()` — against the float64 twin (tests/propnet_twin.py, tests/render_twin.py).

Tolerances: the bounds derived in propnet_twin's docstring (loss elements, their derivative, the scatter into the key
CDF, a level's CDF), render_twin's forward bounds, 4 float32 ulp for the s -> t transform, and for gradients that pass
through a network or the plain-torch scan the "8 times" rule: the device's worst error against float64 is at most 8
times the worst error of the same chain run in float32 on the CPU (the margin is for the different order of the
device's reductions and scatter-adds); the measured figures are in profiles/propnet_loss.md.  Every test prints its worst
error / bound ratio (`pytest -s`)."""
import copy

import numpy as np
import pytest
import torch

import pdf_twin
import propnet_twin as P
import render_twin as RT

pytestmark = pytest.mark.gpu
f32, f64, i64 = np.float32, np.float64, np.int64

RAYS = [1, 3, 65]
KEY_EDGES = [2, 3, 33, 65, 600]          # 600 is above kPdfCap = 512 of pdf.hip: the global route
QUERY_EDGES = [2, 17, 65, 130]


def _t64(x):
    return torch.from_numpy(np.asarray(x, f64))


def _ratio(err, bound):
    """max err / bound (0 / 0 counts as 0); every element must be within its bound."""
    err, bound = np.asarray(err, f64), np.asarray(bound, f64)
    assert err.shape == bound.shape
    bad = ~(err <= bound)
    assert not bad.any(), (int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))


def _report(name, value):
    print(f"RATIO {name} {value:.4g}")


def _case(seed, n_rays, n_key, n_query, unit_ends=False):
    """float32 key edges, key CDF, query edges, query CDF, cotangent.  Next to propnet_twin.histograms' ties, clamped ends,
    flat runs and flat row: rows 0, 8, .. saturate (the CDF reaches 1.0 midway and stays), rows 4, 12, .. have zero
    density (all mass in the closing interval); the query CDF has a flat run on every third row."""
    key, ck, q = P.histograms(seed, n_rays, n_key, n_query, f32, unit_ends=unit_ends)
    rng = np.random.default_rng(seed + 1000)
    for r in range(n_rays):
        if r % 8 == 0 and n_key > 3:
            ck[r] = np.minimum(1.0, np.arange(n_key) / float(n_key // 2)).astype(f32)
        if r % 8 == 4:
            ck[r, :-1], ck[r, -1] = 0.0, 1.0
    cq = np.sort(rng.uniform(size=q.shape), -1).astype(f32)
    cq[:, 0], cq[:, -1] = 0.0, 1.0
    if n_query > 4:
        cq[::3, n_query // 3: n_query // 2] = cq[::3, n_query // 3: n_query // 3 + 1]
    g = rng.normal(size=(n_rays, n_query - 1)).astype(f32)
    return key, ck, q, cq, g


def _twin(key, ck, q, cq, g):
    """float64: loss elements, their bound, the gradient w.r.t. the key CDF under cotangent g, its bound, and the
    mask of the elements that are exactly zero (w <= w_outer)."""
    c = _t64(ck).requires_grad_(True)
    loss, w, wo = P.pdf_loss(_t64(q), _t64(cq), _t64(key), c, snap_zero=True)
    (grad,) = torch.autograd.grad(loss, c, _t64(g))
    # the bounds (0 where w <= w_outer) take w_outer as the one difference ck[hi] - ck[lo]
    w, wo = w.numpy(), P.outer_weights_searchsorted(_t64(q), _t64(key), _t64(ck)).numpy()
    lo, hi = P.bracket(torch.from_numpy(q), torch.from_numpy(key))
    terms = -2.0 * g.astype(f64) * np.maximum(w - wo, 0.0) / (w + P.EPS)
    gb = P.scatter_bound(lo.numpy(), hi.numpy(), terms, P.dloss_bound(w, wo, g.astype(f64)), key.shape[-1])
    return loss.detach().numpy(), P.loss_bound(w, wo), grad.numpy(), gb, w <= wo


def _reached(q, key):
    """(n, K + 1) bool: the key entries whose CDF value enters some query interval's w_outer (as hi or as lo)."""
    lo, hi = (x.numpy() for x in P.bracket(torch.from_numpy(q), torch.from_numpy(key)))
    out = np.zeros(key.shape, bool)
    rows = np.repeat(np.arange(key.shape[0]), lo.shape[1]).reshape(lo.shape)
    out[rows, lo] = True
    out[rows, hi] = True
    return out


def _reached_only_by(zero, q, key):
    """(n, K + 1) bool: the key entries that no interval outside the mask `zero` (n, Q) reaches: their gradient is 0."""
    lo, hi = (x.numpy() for x in P.bracket(torch.from_numpy(q), torch.from_numpy(key)))
    hit = np.zeros(key.shape, bool)
    rows = np.repeat(np.arange(key.shape[0]), lo.shape[1]).reshape(lo.shape)
    hit[rows[~zero], lo[~zero]] = True
    hit[rows[~zero], hi[~zero]] = True
    return ~hit


def _on(cuda, x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _flat(cuda, rows, flags=False):
    """Flattened RayIntervals of a list of 1-D rows (packed_info; is_left / is_right when `flags`)."""
    from cnc_amd.nerfacc import RayIntervals
    cnts = np.asarray([len(r) for r in rows], i64)
    starts = np.cumsum(cnts) - cnts
    vals = np.concatenate([np.asarray(r, f32) for r in rows]) if len(rows) else np.zeros(0, f32)
    rec = RayIntervals(vals=_on(cuda, vals), packed_info=_on(cuda, np.stack([starts, cnts], -1)))
    if flags:
        k = np.concatenate([np.arange(c) for c in cnts]) if len(rows) else np.zeros(0, i64)
        n = np.repeat(cnts, cnts)
        rec.is_left, rec.is_right = _on(cuda, k < n - 1), _on(cuda, k > 0)
    return rec


# ----------------------------------------------------------------------------------------------------------------------
# a. _pdf_loss, batched
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_query", QUERY_EDGES)
@pytest.mark.parametrize("n_key", KEY_EDGES)
def test_pdf_loss_batched(cuda, n_key, n_query):
    from cnc_amd.nerfacc import RayIntervals
    from cnc_amd.nerfacc.estimators.prop_net import _pdf_loss
    worst_l = worst_g = 0.0
    for n_rays in RAYS:
        key, ck, q, cq, g = _case(7 * n_key + n_query + n_rays, n_rays, n_key, n_query)
        want, bound, want_g, bound_g, zero = _twin(key, ck, q, cq, g)
        c = _on(cuda, ck).requires_grad_(True)
        got = _pdf_loss(RayIntervals(vals=_on(cuda, q)), _on(cuda, cq), RayIntervals(vals=_on(cuda, key)), c)
        (got_g,) = torch.autograd.grad(got, c, _on(cuda, g), retain_graph=True)
        assert got.shape == (n_rays, n_query - 1) and got.dtype == torch.float32
        got_t, got, got_g = got, got.detach().cpu().numpy(), got_g.cpu().numpy()
        worst_l = max(worst_l, _ratio(np.abs(got - want), bound))
        worst_g = max(worst_g, _ratio(np.abs(got_g - want_g), bound_g))
        # w <= w_outer: exactly 0 (the bounds are 0 there), and the gradient too: a key entry that only such intervals
        # reach is exactly 0, and so is the whole gradient under a cotangent masked to these elements
        assert (bound[zero] == 0).all() and (got[zero] == 0).all()
        only_zero = _reached_only_by(zero, q, key)
        assert (bound_g[only_zero] == 0).all() and (got_g[only_zero] == 0).all()
        (masked_g,) = torch.autograd.grad(got_t, c, _on(cuda, np.where(zero, g, f32(0))))
        assert not masked_g.any()
        if n_rays == 65 and n_key > 3 and n_query > 4:
            assert zero.any() and not zero.all() and (only_zero & _reached(q, key)).any()
    _report(f"pdf_loss_batched[{n_key}-{n_query}] loss", worst_l)
    _report(f"pdf_loss_batched[{n_key}-{n_query}] grad", worst_g)


# ----------------------------------------------------------------------------------------------------------------------
# b. _pdf_loss, flattened query
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_key,n_query", [(2, 2), (33, 17), (65, 130), (600, 65)])
def test_pdf_loss_flattened_equals_batched_on_equal_rays(cuda, n_key, n_query):
    """Flattened query against a flattened key, and against a batched key (the ids of a flattened query index the
    key's values as a whole either way): bit-equal to the batched result; gradients within the bound."""
    from cnc_amd.nerfacc import RayIntervals
    from cnc_amd.nerfacc.estimators.prop_net import _pdf_loss
    n_rays = 65
    key, ck, q, cq, g = _case(3 * n_key + n_query, n_rays, n_key, n_query)
    _, _, want_g, bound_g, _ = _twin(key, ck, q, cq, g)
    batched = _pdf_loss(RayIntervals(vals=_on(cuda, q)), _on(cuda, cq), RayIntervals(vals=_on(cuda, key)), _on(cuda, ck))
    fq = _flat(cuda, list(q), flags=True)
    worst = 0.0
    for flat_key in (True, False):
        c = _on(cuda, ck.reshape(-1) if flat_key else ck).requires_grad_(True)
        k = _flat(cuda, list(key)) if flat_key else RayIntervals(vals=_on(cuda, key))
        got = _pdf_loss(fq, _on(cuda, cq.reshape(-1)), k, c)
        assert got.shape == (n_rays * (n_query - 1),)
        assert torch.equal(got.detach(), batched.reshape(-1)), flat_key
        (got_g,) = torch.autograd.grad(got, c, _on(cuda, g.reshape(-1)))
        assert got_g.shape == c.shape
        worst = max(worst, _ratio(np.abs(got_g.cpu().numpy().reshape(n_rays, n_key) - want_g), bound_g))
    _report(f"pdf_loss_flattened_equal[{n_key}-{n_query}] grad", worst)


def test_pdf_loss_flattened_ragged(cuda):
    """Rays of different key and query sizes, empty query rays among them (one the last ray), against the twin run
    ray by ray."""
    from cnc_amd.nerfacc.estimators.prop_net import _pdf_loss
    n_key = [2, 3, 33, 65, 600, 33, 65, 3, 600, 2, 33, 17]
    n_query = [17, 0, 2, 130, 65, 17, 0, 65, 2, 130, 17, 0]
    # ray r is row r % 8 of an 8-ray case of its own sizes: a saturating key (rays 0, 8), a flat run (1, 5, 9), a flat
    # CDF (2), repeated key edges (3, 7, 11) and a zero-density key (4) are all among them
    rows = [_case(500 + r, 8, nk, max(nq, 2)) for r, (nk, nq) in enumerate(zip(n_key, n_query))]
    keys, cks, qs, cqs, gs = ([] for _ in range(5))
    for r, (case, nq) in enumerate(zip(rows, n_query)):
        key, ck, q, cq, g = (a[r % 8] for a in case)
        keys.append(key)
        cks.append(ck)
        for out, a in ((qs, q), (cqs, cq), (gs, g)):
            out.append(a if nq else np.zeros(0, f32))           # a ray without a query keeps its key
    c = _on(cuda, np.concatenate(cks)).requires_grad_(True)
    got = _pdf_loss(_flat(cuda, qs, flags=True), _on(cuda, np.concatenate(cqs)), _flat(cuda, keys), c)
    (got_g,) = torch.autograd.grad(got, c, _on(cuda, np.concatenate(gs)))
    assert got.shape == (sum(max(nq - 1, 0) for nq in n_query),)
    got, got_g = got.detach().cpu().numpy(), got_g.cpu().numpy()
    worst_l = worst_g = 0.0
    at_l = at_g = 0
    for r, nq in enumerate(n_query):
        part_g = got_g[at_g: at_g + n_key[r]]
        at_g += n_key[r]
        if nq == 0:
            assert (part_g == 0).all()                 # nothing reaches the key of a ray without query intervals
            continue
        want, bound, want_g, bound_g, zero = _twin(keys[r][None], cks[r][None], qs[r][None], cqs[r][None], gs[r][None])
        part = got[at_l: at_l + nq - 1]
        at_l += nq - 1
        worst_l = max(worst_l, _ratio(np.abs(part - want[0]), bound[0]))
        worst_g = max(worst_g, _ratio(np.abs(part_g - want_g[0]), bound_g[0]))
        assert (part[zero[0]] == 0).all()
        assert (part_g[_reached_only_by(zero, qs[r][None], keys[r][None])[0]] == 0).all()
    assert at_l == got.shape[0] and at_g == got_g.shape[0]
    _report("pdf_loss_flattened_ragged loss", worst_l)
    _report("pdf_loss_flattened_ragged grad", worst_g)


def test_pdf_loss_refuses_mixed_layouts_it_cannot_index(cuda):
    """A batched query counts its ids from the start of the row: against a flattened key CDF that is an error, said
    so; a flattened query without its flags too."""
    from cnc_amd.nerfacc import RayIntervals
    from cnc_amd.nerfacc.estimators.prop_net import _pdf_loss
    key, ck, q, cq, _ = _case(5, 3, 33, 17)
    with pytest.raises(AssertionError, match="batched key"):
        _pdf_loss(RayIntervals(vals=_on(cuda, q)), _on(cuda, cq), _flat(cuda, list(key)), _on(cuda, ck.reshape(-1)))
    with pytest.raises(AssertionError, match="is_left"):
        _pdf_loss(_flat(cuda, list(q)), _on(cuda, cq.reshape(-1)), _flat(cuda, list(key)), _on(cuda, ck.reshape(-1)))


# ----------------------------------------------------------------------------------------------------------------------
# c. compute_loss
# ----------------------------------------------------------------------------------------------------------------------
def _cached(cuda, n_rays=65, sizes=(65, 33), n_final=17, seed=90):
    """Two levels of different sizes and the final edges, all on [0, 1]; transmittance on the grid k / 2^20, so that
    1 - T is exact in float32 and the target CDF is the same number in the twin and on the device."""
    levels = []
    for i, n_key in enumerate(sizes):
        key, ck, q, _, _ = _case(seed + i, n_rays, n_key, n_final, unit_ends=True)
        levels.append((key, ck))
        final = q if i == 0 else final
    rng = np.random.default_rng(seed + 50)
    trans = np.sort(rng.integers(0, 2 ** 20 + 1, (n_rays, n_final - 1)), -1)[:, ::-1] / float(2 ** 20)
    trans[:, 0] = 1.0
    trans[1, 5:] = 0.0                                   # a ray that turns opaque part-way
    return levels, final, trans.astype(f32)


def _estimator_with_cache(cuda, levels, final):
    from cnc_amd.nerfacc import PropNetEstimator, RayIntervals
    est = PropNetEstimator().to(cuda)
    cdfs = [_on(cuda, ck).requires_grad_(True) for _, ck in levels]
    est.prop_cache = [(RayIntervals(vals=_on(cuda, key)), c) for (key, _), c in zip(levels, cdfs)]
    est.prop_cache.append((RayIntervals(vals=_on(cuda, final)), None))
    return est, cdfs


def _loss_twin(levels, final, trans, scaler):
    """float64 value of compute_loss, the bound of its float32 evaluation, the gradients w.r.t. the levels' CDFs and
    their bounds.  Value: per level the mean of the elements' bounds plus the n - 1 additions and the division of the
    mean (gamma_n of it); then the sum of the means and the product with the scaler (gamma_2).  Gradients: the
    elements' derivative under the cotangent scaler / n, itself rounded once (the division by n; gamma_2 allowed),
    scattered into the level's CDF."""
    n = final.shape[0] * (final.shape[1] - 1)
    cdfs = [_t64(ck).requires_grad_(True) for _, ck in levels]
    want = P.compute_loss([(_t64(k), c) for (k, _), c in zip(levels, cdfs)], _t64(final), _t64(trans), scaler,
                          snap_zero=True)
    want_g = [g.numpy() for g in torch.autograd.grad(want, cdfs)]
    target = P.opacity_cdf(_t64(trans))
    cot = np.full((final.shape[0], final.shape[1] - 1), scaler / n, f64)
    means = bounds = 0.0
    grad_bounds = []
    for (key, ck) in levels:
        loss, w, _ = P.pdf_loss(_t64(final), target, _t64(key), _t64(ck), snap_zero=True)
        w, wo = w.numpy(), P.outer_weights_searchsorted(_t64(final), _t64(key), _t64(ck)).numpy()
        means += float(loss.mean())
        bounds += float(P.loss_bound(w, wo).mean()) + P.gamma(n) * float(loss.mean())
        lo, hi = P.bracket(torch.from_numpy(final), torch.from_numpy(key))
        terms = -2.0 * cot * np.maximum(w - wo, 0.0) / (w + P.EPS)
        tb = P.dloss_bound(w, wo, cot) + P.gamma(2) * np.abs(terms)
        grad_bounds.append(P.scatter_bound(lo.numpy(), hi.numpy(), terms, tb, key.shape[-1]))
    return want.item(), scaler * (bounds + P.gamma(2) * (means + bounds)), want_g, grad_bounds


def test_compute_loss_two_levels(cuda):
    levels, final, trans = _cached(cuda)
    values = {}
    for scaler in (1.0, 3.0, 4.0):
        want, bound, want_g, bound_g = _loss_twin(levels, final, trans, scaler)
        est, cdfs = _estimator_with_cache(cuda, levels, final)
        tr = _on(cuda, trans).requires_grad_(True)
        got = est.compute_loss(tr, scaler)
        assert est.prop_cache == []                                     # emptied
        assert got.shape == () and want > 0
        _report(f"compute_loss[{scaler}] value", _ratio(np.abs(got.item() - want), np.float64(bound)))
        got.backward()
        assert tr.grad is None or not tr.grad.any()                     # the target is a constant
        worst = 0.0
        for c, wg, gb in zip(cdfs, want_g, bound_g):
            assert np.abs(wg).sum() > 0
            worst = max(worst, _ratio(np.abs(c.grad.cpu().numpy() - wg), gb))
        _report(f"compute_loss[{scaler}] grad", worst)
        values[scaler] = got.item()
        # an empty cache gives 0
        again = est.compute_loss(tr, scaler)
        assert again.item() == 0.0 and again.shape == () and again.device == tr.device
    assert values[4.0] == 4.0 * values[1.0]                              # a power of two scales exactly


def test_compute_loss_pairs_every_level_with_its_own_cdf(cuda):
    """Two levels of EQUAL size, so that a level paired with the other's CDF would still run: the value is the twin's,
    and the bound is far below the difference to the value of the swapped pairing."""
    levels, final, trans = _cached(cuda, sizes=(33, 33), seed=120)
    # level 1 unlike level 0: its edges crowd towards 0 and its mass sits late on the ray
    levels[1] = ((levels[1][0].astype(f64) ** 3).astype(f32), (levels[1][1].astype(f64) ** 4).astype(f32))
    want, bound, _, _ = _loss_twin(levels, final, trans, 1.0)
    swapped = P.compute_loss([(_t64(levels[0][0]), _t64(levels[1][1])), (_t64(levels[1][0]), _t64(levels[0][1]))],
                             _t64(final), _t64(trans)).item()
    est, _ = _estimator_with_cache(cuda, levels, final)
    got = est.compute_loss(_on(cuda, trans)).item()
    assert abs(got - want) <= bound < 0.1 * abs(swapped - want)


def test_compute_loss_adds_the_levels_last_to_first(cuda):
    """Three levels of unequal size.  The order of a float32 sum of three shows only in its last bit, so this is held
    bit for bit: the total is fl(fl(m3 + m2) + m1) of the levels' own means m_i (each from a one-level cache, the same
    reduction on the same numbers), for every seed; and on at least one of the seeds fl(fl(m1 + m2) + m3) is a
    different number, so that the other order would be noticed."""
    told_apart = 0
    for seed in range(300, 316):
        levels, final, trans = _cached(cuda, n_rays=9, sizes=(65, 33, 17), seed=seed)
        tr = _on(cuda, trans)
        est, _ = _estimator_with_cache(cuda, levels, final)
        total = est.compute_loss(tr).detach().cpu().numpy()
        m = []
        for level in levels:
            est, _ = _estimator_with_cache(cuda, [level], final)
            m.append(est.compute_loss(tr).detach().cpu().numpy())
        assert total.dtype == f32 and all(x.dtype == f32 and x > 0 for x in m)
        assert total == (m[2] + m[1]) + m[0], seed
        told_apart += int((m[2] + m[1]) + m[0] != (m[0] + m[1]) + m[2])
    assert told_apart > 0


# ----------------------------------------------------------------------------------------------------------------------
# d. sampling, stage by stage
# ----------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """A density function of t that keeps what it was handed and what it returned.  Ray 0 has zero density, ray 1 a
    density that saturates the CDF (the transmittance underflows inside the slab), the others a slab of density 3."""

    def __init__(self, lo, hi, scale):
        self.lo, self.hi, self.scale, self.calls = lo, hi, scale, []

    def __call__(self, t0, t1):
        mid = (t0 + t1) / 2
        inside = (mid >= self.lo[:, None]) & (mid <= self.hi[:, None])
        sig = torch.where(inside, self.scale[:, None].expand_as(mid), torch.zeros_like(mid)) * (1 + 0.1 * torch.sin(mid))
        self.calls.append((t0, t1, sig))
        return sig


def _ulps32(got, want64):
    return np.abs(got.astype(f64) - want64) / np.spacing(np.abs(want64).astype(f32)).astype(f64)


@pytest.mark.parametrize("stratified", [False, True])
@pytest.mark.parametrize("sampling_type", ["uniform", "lindisp"])
def test_sampling_stage_by_stage(cuda, sampling_type, stratified):
    from cnc_amd.nerfacc import PropNetEstimator
    n_rays, near, far, sizes, n_final = 65, 1.0, 10.0, [64, 32], 16
    g = torch.Generator().manual_seed(3)
    lo = (2.0 + 4.0 * torch.rand(n_rays, generator=g)).to(cuda)
    scale = torch.full((n_rays,), 3.0)
    scale[0], scale[1] = 0.0, 400.0
    fns = [_Recorder(lo, lo + 2.5, scale.to(cuda)), _Recorder(lo, lo + 2.5, scale.to(cuda) * 1.5)]
    est = PropNetEstimator().to(cuda)
    torch.manual_seed(7)
    t0, t1 = est.sampling(fns, sizes, n_final, n_rays=n_rays, near_plane=near, far_plane=far,
                          sampling_type=sampling_type, stratified=stratified, requires_grad=True)
    jitters = [None] * 3
    if stratified:          # one torch.rand draw of n_rays biases per importance_sampling call, in order
        torch.manual_seed(7)
        jitters = [torch.rand(n_rays, device=cuda).cpu().numpy() for _ in range(3)]
    cache = est.prop_cache
    assert len(cache) == 3 and cache[2][1] is None and all(len(f.calls) == 1 for f in fns)

    prev_e = np.tile(np.asarray([0.0, 1.0], f32), (n_rays, 1))       # the first level: the segment [0, 1], CDF [0, 1]
    prev_c = prev_e.copy()
    worst_t = worst_c = worst_d = 0.0
    for i, n_level in enumerate(sizes + [n_final]):
        edges = cache[i][0].vals.cpu().numpy()
        E = prev_e.shape[1]
        _, want_e = pdf_twin.importance_sampling_batched(prev_e, prev_c, np.arange(n_rays) * E, np.full(n_rays, E),
                                                         n_level, jitters[i])
        assert edges.shape == (n_rays, n_level + 1)
        assert np.array_equal(edges.view(np.int32), want_e.view(np.int32)), i
        # the precondition of the loss: inside the previous level's range, sorted, in s-space
        assert (edges >= prev_e[:, :1]).all() and (edges <= prev_e[:, -1:]).all() and (np.diff(edges, axis=1) >= 0).all()
        assert edges.min() >= 0.0 and edges.max() <= 1.0
        want_t = P.transform_stot(sampling_type, _t64(edges), near, far).numpy()
        if i == len(sizes):
            got_t0, got_t1 = t0.cpu().numpy(), t1.cpu().numpy()
        else:
            h0, h1, sig = fns[i].calls[0]
            got_t0, got_t1 = h0.cpu().numpy(), h1.cpu().numpy()
        assert got_t0.shape == (n_rays, n_level)
        worst_t = max(worst_t, _ulps32(got_t0, want_t[:, :-1]).max(), _ulps32(got_t1, want_t[:, 1:]).max())
        if i == len(sizes):
            break
        # the level's CDF from the float32 t and densities it was computed from
        cdf = cache[i][1].detach().cpu().numpy()
        sig = sig.detach().cpu().numpy()
        want_c = P.opacity_cdf(P.transmittance(_t64(got_t0), _t64(got_t1), _t64(sig))).numpy()
        worst_c = max(worst_c, _ratio(np.abs(cdf - want_c), P.cdf_bound(got_t0, got_t1, sig, RT.E_EXP)))
        # and as the requirement is stated: within u times the row's optical depth (exact on the row of zero density)
        worst_d = max(worst_d, _ratio(np.abs(cdf - want_c), P.optical_depth_bound(got_t0, got_t1, sig)))
        assert (cdf[:, 0] == 0).all() and (cdf[:, -1] == 1).all()
        assert (cdf[0, :-1] == 0).all()                              # zero density: all mass in the closing interval
        assert (cdf[1] == 1.0).sum() > 2                             # saturated: 1.0 before the end, flat from there
        prev_e, prev_c = edges, cdf
    assert worst_t <= 4.0, worst_t
    _report(f"sampling[{sampling_type}-{stratified}] t ulps / 4", worst_t / 4.0)
    _report(f"sampling[{sampling_type}-{stratified}] cdf", worst_c)
    _report(f"sampling[{sampling_type}-{stratified}] cdf / (u optical depth)", worst_d)
    est.prop_cache.clear()


# ----------------------------------------------------------------------------------------------------------------------
# e. parameter gradients of a proposal network through sampling + compute_loss
# ----------------------------------------------------------------------------------------------------------------------
def _cpu_chain(nets, cache_edges, trans, sampling_type, near, far, dtype):
    """The chain from the cached float32 edges on: t, densities, CDFs, loss, parameter gradients; in `dtype` on the CPU.
    float64 takes the overlap form of the outer weights, float32 the estimator's gather form."""
    nets = [copy.deepcopy(n).to(dtype) for n in nets]
    outer = P.outer_weights if dtype == torch.float64 else P.outer_weights_searchsorted
    levels = []
    for net, edges in zip(nets, cache_edges[:-1]):
        e = torch.from_numpy(edges).to(dtype)
        t = P.transform_stot(sampling_type, e, near, far)
        t0, t1 = t[:, :-1], t[:, 1:]
        levels.append((e, P.opacity_cdf(P.transmittance(t0, t1, net(t0, t1)))))
    loss = P.compute_loss(levels, torch.from_numpy(cache_edges[-1]).to(dtype), torch.from_numpy(trans).to(dtype),
                          outer=outer)
    loss.backward()
    return loss.item(), [p.grad.numpy().astype(f64) for n in nets for p in n.parameters()]


@pytest.mark.parametrize("sampling_type", ["uniform", "lindisp"])
def test_network_gradients_through_sampling_and_loss(cuda, sampling_type):
    from cnc_amd.nerfacc import PropNetEstimator
    from cnc_amd.nerfacc.volrend import render_transmittance_from_density
    from test_gpu_propnet import _Fourier
    torch.manual_seed(11)
    n_rays, near, far = 65, 1.0, 10.0
    nets = [_Fourier(near, far), _Fourier(near, far)]
    dev_nets = [copy.deepcopy(n).to(cuda) for n in nets]
    est = PropNetEstimator().to(cuda)
    t0, t1 = est.sampling(dev_nets, [64, 32], 16, n_rays=n_rays, near_plane=near, far_plane=far,
                          sampling_type=sampling_type, requires_grad=True)
    mid = (t0 + t1) / 2
    truth = torch.where((mid >= 4.0) & (mid <= 5.5), torch.full_like(mid, 4.0), torch.zeros_like(mid))
    trans, _ = render_transmittance_from_density(t0, t1, truth)
    edges = [rec.vals.cpu().numpy() for rec, _ in est.prop_cache]
    loss = est.compute_loss(trans)
    loss.backward()
    got = [p.grad.cpu().numpy().astype(f64) for n in dev_nets for p in n.parameters()]
    trans = trans.cpu().numpy()
    want_l, want = _cpu_chain(nets, edges, trans, sampling_type, near, far, torch.float64)
    cpu_l, cpu = _cpu_chain(nets, edges, trans, sampling_type, near, far, torch.float32)
    assert want_l > 0 and len(got) == len(want) == 4
    names = [f"net{i}.{k}" for i in range(2) for k, _ in nets[0].named_parameters()]
    print(f"ERR {sampling_type} loss device {abs(loss.item() - want_l):.3e} cpu32 {abs(cpu_l - want_l):.3e} "
          f"value {want_l:.6e}")
    worst = 0.0
    failed = []
    for name, g, c, w in zip(names, got, cpu, want):
        assert np.abs(w).max() > 0
        e_dev, e_cpu = np.abs(g - w).max(), np.abs(c - w).max()
        print(f"ERR {sampling_type} {name} device {e_dev:.3e} cpu32 {e_cpu:.3e} ratio {e_dev / max(e_cpu, 1e-300):.3f} "
              f"largest |grad| {np.abs(w).max():.3e}")
        worst = max(worst, e_dev / max(e_cpu, 1e-300))
        if not e_dev <= 8.0 * e_cpu:
            failed.append(name)
    assert not failed, failed
    _report(f"network_gradients[{sampling_type}] device / cpu32 / 8", worst / 8.0)


# ----------------------------------------------------------------------------------------------------------------------
# f. the batched route of rendering()
# ----------------------------------------------------------------------------------------------------------------------
def _render_inputs(n_rays, S, seed):
    rng = np.random.default_rng(seed)
    dt = rng.uniform(0.01, 0.3, (n_rays, S))
    t1 = 1.0 + np.cumsum(dt, -1)
    t0 = np.concatenate([np.ones((n_rays, 1)), t1[:, :-1]], -1)
    scale = rng.choice([0.0, 1e-3, 1.0, 10.0, 300.0], n_rays)
    scale[:2] = 0.0, 300.0
    sig = rng.uniform(size=(n_rays, S)) ** 2 * scale[:, None]
    rgb = rng.uniform(size=(n_rays, S, 3))
    cot = [rng.normal(size=(n_rays, 3)), rng.normal(size=(n_rays, 1)), rng.normal(size=(n_rays, 1))]
    return [a.astype(f32) for a in (t0, t1, sig, rgb)], [a.astype(f32) for a in cot]


def _render(device, inputs, cot, opaque, bkgd):
    from cnc_amd.nerfacc import rendering
    from cnc_amd.render import _last_sample_opaque
    t0, t1, sig, rgb = (torch.from_numpy(a).to(device) for a in inputs)
    sig.requires_grad_(True)
    rgb.requires_grad_(True)

    def rgb_sigma_fn(ts, te, ray_indices):
        assert ray_indices is None and ts.shape == sig.shape
        return rgb, (_last_sample_opaque(sig) if opaque else sig), None

    bk = None if bkgd is None else torch.from_numpy(bkgd).to(device)
    colors, opacity, depth, extras = rendering(t0, t1, rgb_sigma_fn=rgb_sigma_fn, render_bkgd=bk)
    gc, go, gd = (torch.from_numpy(a).to(device) for a in cot)
    ((colors * gc).sum() + (opacity * go).sum() + (depth * gd).sum()).backward()
    out = dict(colors=colors, opacity=opacity, depth=depth, weights=extras["weights"], trans=extras["trans"],
               alphas=extras["alphas"], g_sig=sig.grad, g_rgb=rgb.grad)
    return {k: v.detach().cpu().numpy().astype(f64) for k, v in out.items()}


@pytest.mark.parametrize("with_bkgd", [False, True])
@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("S", [1, 16, 33])
def test_rendering_batched_route(cuda, S, opaque, with_bkgd):
    n_rays = 65
    inputs, cot = _render_inputs(n_rays, S, 200 + S)
    bkgd = np.asarray([0.2, 0.4, 0.9], f32) if with_bkgd else None
    got = _render(cuda, inputs, cot, opaque, bkgd)
    cpu = _render(torch.device("cpu"), inputs, cot, opaque, bkgd)
    t0, t1, sig, rgb = inputs
    sig_in = sig.copy()
    if opaque:
        sig_in[:, -1] = np.inf
    lay = RT.Layout(np.arange(n_rays) * S, np.full(n_rays, S))
    f = RT.forward(lay, t0.reshape(-1), t1.reshape(-1), sig_in.reshape(-1), rgb.reshape(-1, 3), render_bkgd=bkgd)
    b = RT.forward_bounds(f)
    assert got["colors"].shape == (n_rays, 3) and got["opacity"].shape == (n_rays, 1) and got["weights"].shape == (n_rays, S)
    ratios = {
        "colors": _ratio(np.abs(got["colors"] - f.col_f), b.e_col_f),
        "opacity": _ratio(np.abs(got["opacity"][:, 0] - f.op), b.e_op),
        "depth": _ratio(np.abs(got["depth"][:, 0] - f.depth), b.e_depth),
        "weights": _ratio(np.abs(got["weights"].reshape(-1) - f.w), b.eW),
        "trans": _ratio(np.abs(got["trans"].reshape(-1) - f.trans), b.eT),
        "alphas": _ratio(np.abs(got["alphas"].reshape(-1) - f.alpha), b.eA),
    }
    if opaque:
        assert (got["alphas"][:, -1] == 1).all() and np.abs(f.op - 1).max() <= 1e-12
    # gradients: finite, and within 8 times the float32 CPU run's worst error of the twin's closed form
    bw = RT.backward(f, grad_colors=cot[0], grad_opacity=cot[1], grad_depth=cot[2], finalize=True)
    want = {"g_sig": bw.g_sigmas.reshape(n_rays, S), "g_rgb": bw.g_rgbs.reshape(n_rays, S, 3)}
    # (a ray of zero density has depth 0 / eps: its density gradients are of the order 1e7 and would alone decide the
    # worst error of the tensor, so the rule is also applied with every ray's errors divided by its largest gradient)
    row_scale = np.abs(want["g_sig"]).max(-1, keepdims=True)
    row_scale = np.where(row_scale > 0, row_scale, 1.0)
    for k, scale in (("g_sig", 1.0), ("g_sig per ray", row_scale), ("g_rgb", 1.0)):
        name = k.split()[0]
        assert np.isfinite(got[name]).all() and np.isfinite(want[name]).all()
        e_dev, e_cpu = (np.abs(got[name] - want[name]) / scale).max(), (np.abs(cpu[name] - want[name]) / scale).max()
        print(f"ERR rendering[{S}-{opaque}-{with_bkgd}] {k} device {e_dev:.3e} cpu32 {e_cpu:.3e} "
              f"largest {(np.abs(want[name]) / scale).max():.3e}")
        assert e_dev <= 8.0 * e_cpu, (k, e_dev, e_cpu)
        ratios[k + " device / cpu32 / 8"] = e_dev / e_cpu / 8.0 if e_cpu > 0 else 0.0
    if opaque:
        assert (got["g_sig"][:, -1] == 0).all()                      # the density that was replaced gets no gradient
    for k, v in ratios.items():
        _report(f"rendering[{S}-{opaque}-{with_bkgd}] {k}", v)
