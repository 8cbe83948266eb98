"""CPU: the NumPy twin of the proposal-sampling kernels (tests/pdf_twin.py) pinned to hand-worked values, the
reference's docstring examples and np.searchsorted; the pure-torch parts of the proposal estimator; the ctypes
mirror of cnc_pdf_rows_t."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import pdf_twin as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _exact_fma32(a, b, c):
    """a * b + c rounded once to float32, by exact rational arithmetic."""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = f32(float(x))
    cands = [g, np.nextafter(g, f32(np.inf)), np.nextafter(g, f32(-np.inf))]
    best = min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.array(v).view(np.int32)) & 1))
    return best


def test_fmaf_rounds_once():
    rng = np.random.default_rng(0)
    a = rng.uniform(-4, 4, 3000).astype(f32)
    b = rng.uniform(-4, 4, 3000).astype(f32)
    c = rng.uniform(-4, 4, 3000).astype(f32)
    got = T.fmaf(a, b, c)
    want = np.array([_exact_fma32(*v) for v in zip(a, b, c)], f32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # products whose float64 sum with c lands exactly on a float32 tie, where rounding twice goes wrong
    a = f32(1 + 2 ** -12)
    b = f32(1 + 2 ** -12)              # a * b = 1 + 2^-11 + 2^-24 exactly: a tie between two float32
    for c, want in ((f32(0), f32(1 + 2 ** -11)), (f32(2 ** -60), f32(1 + 2 ** -11 + 2 ** -23)),
                    (f32(-2 ** -60), f32(1 + 2 ** -11))):
        assert T.fmaf(a, b, c) == want == _exact_fma32(a, b, c), (c, T.fmaf(a, b, c), want)
    assert np.isnan(T.fmaf(f32(np.inf), f32(0), f32(1)))
    assert T.fmaf(f32(2), f32(3), f32(np.inf)) == np.inf


def test_docstring_examples():
    """nerfacc/pdf.py:39-56 (searchsorted) and :104-120 (importance_sampling), numbers as recorded there."""
    vals = np.array([0.0, 1.0, 0.0, 1.0, 2.0], f32)
    left, right = T.searchsorted(vals, [0, 2], [2, 3], np.array([0.5, 1.5, 2.5], f32), [0, 1, 1], local=False)
    assert left.tolist() == [0, 3, 3] and right.tolist() == [1, 4, 4]
    assert vals[left].tolist() == [0.0, 1.0, 1.0] and vals[right].tolist() == [1.0, 2.0, 2.0]
    assert T.query_rays_from_starts([0, 1], 3).tolist() == [0, 1, 1]
    cdfs = np.array([0.0, 0.5, 0.0, 0.5, 1.0], f32)
    s, e = T.importance_sampling_batched(vals, cdfs, [0, 2], [2, 3], 2)
    assert e.tolist() == [[0.0, 0.5, 1.0], [0.0, 1.0, 2.0]]
    assert s.tolist() == [[0.25, 0.75], [0.5, 1.5]]


def test_searchsorted_matches_numpy_right_plus_clamp():
    rng = np.random.default_rng(1)
    for E in (1, 2, 3, 17, 64, 65, 300):
        keys = np.sort(rng.uniform(0, 1, (7, E)).astype(f32), axis=1)
        keys[2, : E // 2] = keys[2, 0]                       # duplicate keys
        q = rng.uniform(-0.2, 1.2, (7, 40)).astype(f32)
        q[3, : min(E, 5)] = keys[3, :5]                      # queries exactly on keys
        left, right = T.searchsorted(keys.reshape(-1), np.arange(7) * E, np.full(7, E), q,
                                     np.repeat(np.arange(7), 40), local=True)
        for r in range(7):
            p = np.searchsorted(keys[r, : E - 1], q[r], side="right")    # the bound is exclusive of the last key
            assert np.array_equal(left.reshape(7, 40)[r], np.clip(p - 1, 0, E - 1))
            assert np.array_equal(right.reshape(7, 40)[r], np.clip(p, 0, E - 1))


def test_searchsorted_nan_and_empty_and_outside():
    keys = np.array([0.0, 1.0, 2.0, 5.0], f32)
    # NaN goes right: the last key of the segment
    left, right = T.searchsorted(keys, [0], [4], np.array([np.nan, -1.0, 9.0], f32), [0, 0, 0], local=True)
    assert left.tolist() == [2, 0, 2] and right.tolist() == [3, 0, 3]
    # an empty key segment: both ids at its start; a ray outside the key: -1
    left, right = T.searchsorted(keys, [0, 4], [4, 0], np.array([1.5, 1.5, 1.5], f32), [0, 1, 2], local=False)
    assert left.tolist() == [1, 4, -1] and right.tolist() == [2, 4, -1]


def _one_ray(vals, cdfs, n, jitter=None):
    s, e = T.importance_sampling_batched(np.array(vals, f32), np.array(cdfs, f32), [0], [len(vals)], n,
                                         None if jitter is None else np.array([jitter], f32))
    return s[0], e[0]


def test_importance_sampling_hand_worked():
    # linear CDF on [0, 4]: the samples are the stratum midpoints
    s, e = _one_ray([0, 4], [0, 1], 4)
    assert s.tolist() == [0.5, 1.5, 2.5, 3.5] and e.tolist() == [0, 1, 2, 3, 4]
    # jitter 0 puts every sample at the stratum start; edge 0 is clamped to vals[base]
    s, e = _one_ray([0, 4], [0, 1], 4, jitter=0.0)
    assert s.tolist() == [0, 1, 2, 3] and e.tolist() == [0, 0.5, 1.5, 2.5, 3.5]
    # a flat run of the CDF (the < 1e-10 branch): u = 0.25 falls right of the flat [0, 0] part
    s, e = _one_ray([0, 1, 3], [0, 0, 1], 2)
    assert s.tolist() == [1.5, 2.5]
    # an entirely flat CDF: every u = 0 lands right of all but the last (exclusive) edge -> the midpoint of the
    # last two edges
    s, _ = _one_ray([0, 1, 3], [0.5, 0.5, 0.5], 3)
    assert s.tolist() == [2.0, 2.0, 2.0]
    # duplicate CDF values inside: the search goes past them
    s, _ = _one_ray([0, 1, 2, 3], [0, 0.5, 0.5, 1], 2)
    assert s.tolist() == [0.5, 2.5]
    # n == 1: edges are the segment's ends
    s, e = _one_ray([1, 3], [0, 1], 1)
    assert s.tolist() == [2.0] and e.tolist() == [1.0, 3.0]
    # a segment of one edge: every sample and edge is that edge
    s, e = _one_ray([7], [0.3], 3)
    assert s.tolist() == [7, 7, 7] and e.tolist() == [7, 7, 7, 7]
    # u outside [cdf[base], cdf[last]] (a jitter past 1 or below 0): extrapolated along the end interval above,
    # clamped to the first edge below; the edges stay within the segment
    s, e = _one_ray([0, 1], [0, 1], 2, jitter=1.5)
    assert s.tolist() == [0.75, 1.25] and e.tolist() == [0.5, 1.0, 1.0]
    s, _ = _one_ray([0, 1], [0, 1], 2, jitter=-1.0)
    assert s.tolist() == [0.0, 0.0]
    # a decreasing CDF: every u lies below cdf[base], p = base, the flat branch at the first edge
    s, _ = _one_ray([0, 1], [1, 0], 2)
    assert s.tolist() == [0.0, 0.0]
    # NaN in the CDF: u is NaN, every sample NaN, and the edges clamp to the segment
    s, e = _one_ray([0, 1], [0, np.nan], 2)
    assert np.isnan(s).all() and e[0] == 0 and e[-1] == 1


def test_importance_sampling_packed_layout_and_edge_cases():
    vals = np.array([0, 1, 2, 5, 6], f32)
    cdfs = np.array([0, 0.5, 1, 0, 1], f32)
    r = T.importance_sampling(vals, cdfs, [0, 3, 5], [3, 2, 0], [2, 0, 3])
    assert r["edge_cnts"].tolist() == [3, 0, 4]
    assert r["sample_rays"].tolist() == [0, 0, 2, 2, 2] and r["edge_rays"].tolist() == [0, 0, 0, 2, 2, 2, 2]
    assert r["is_left"].tolist() == [True, True, False, True, True, True, False]
    assert r["is_right"].tolist() == [False, True, True, False, True, True, True]
    assert r["samples"][:2].tolist() == [0.5, 1.5] and r["edges"][:3].tolist() == [0, 1, 2]
    assert np.isnan(r["samples"][2:]).all() and np.isnan(r["edges"][3:]).all()     # empty input segment
    s, e = T.importance_sampling_batched(vals, cdfs, [0, 3], [3, 0], 0)
    assert s.shape == (2, 0) and e[0, 0] == 0 and np.isnan(e[1, 0])


def test_importance_sampling_matches_a_scalar_restatement():
    """The vectorised twin against a plain per-sample loop of the same formulas."""
    rng = np.random.default_rng(2)
    for E, n in ((2, 5), (9, 64), (33, 65), (5, 1)):
        vals = np.sort(rng.uniform(0, 3, (6, E)).astype(f32), axis=1)
        cdfs = np.sort(rng.uniform(0, 1, (6, E)).astype(f32), axis=1)
        cdfs[1] = cdfs[1, 0]
        jit = rng.uniform(0, 1, 6).astype(f32)
        s, e = T.importance_sampling_batched(vals.reshape(-1), cdfs.reshape(-1), np.arange(6) * E, np.full(6, E), n, jit)
        for r in range(6):
            c, v = cdfs[r], vals[r]
            step = (c[-1] - c[0]) / f32(n)
            ts = []
            for k in range(n):
                u = T.fmaf(f32(k) + jit[r], step, c[0])
                p = int(np.searchsorted(c[:-1], u, side="right"))
                p0, p1 = min(max(p - 1, 0), E - 1), min(max(p, 0), E - 1)
                if c[p1] - c[p0] < f32(1e-10):
                    t = (v[p0] + v[p1]) * f32(0.5)
                else:
                    t = T.fmaf(u - c[p0], (v[p1] - v[p0]) / (c[p1] - c[p0]), v[p0])
                ts.append(f32(t))
            assert np.array_equal(s[r], np.array(ts, f32)), (E, n, r)
            if n > 1:
                inner = [(ts[k] + ts[k - 1]) * f32(0.5) for k in range(1, n)]
                first = max(ts[0] - (ts[1] - ts[0]) * f32(0.5), v[0])
                lastv = min(ts[-1] + (ts[-1] - ts[-2]) * f32(0.5), v[-1])
                assert np.array_equal(e[r], np.array([first] + inner + [lastv], f32))


def test_proposal_requires_grad_schedule():
    from cnc_amd.nerfacc.estimators.prop_net import get_proposal_requires_grad_fn
    fn = get_proposal_requires_grad_fn(target=2.0, num_steps=4)
    assert [fn(s) for s in range(10)] == [False, True, False, True, False, False, True, False, False, True]
    fn = get_proposal_requires_grad_fn()        # target 5 over 1000 steps: every step early on
    assert [fn(s) for s in range(6)] == [False, True, True, True, True, True]


def test_transform_stot():
    from cnc_amd.nerfacc.estimators.prop_net import _transform_stot
    s = torch.tensor([0.0, 0.25, 0.5, 1.0])
    assert torch.allclose(_transform_stot("uniform", s, 2.0, 6.0), torch.tensor([2.0, 3.0, 4.0, 6.0]))
    want = 1.0 / (s * (1 / 6.0) + (1 - s) * (1 / 2.0))      # [2, 2.4, 3, 6]
    got = _transform_stot("lindisp", s, 2.0, 6.0)
    assert torch.allclose(got, want) and torch.allclose(got, torch.tensor([2.0, 2.4, 3.0, 6.0]))
    with pytest.raises(ValueError):
        _transform_stot("log", s, 2.0, 6.0)


def test_pdf_loss_on_batched_cpu_ids():
    """_pdf_loss's arithmetic on ids given by the twin: a key that bounds the query from above costs nothing, one
    that misses its mass costs (w - w_outer)^2 / w."""
    from unittest import mock
    from cnc_amd.nerfacc.data_specs import RayIntervals
    from cnc_amd.nerfacc.estimators import prop_net
    q = RayIntervals(vals=torch.tensor([[0.0, 0.5, 1.0]]))
    k = RayIntervals(vals=torch.tensor([[0.0, 0.25, 0.75, 1.0]]))

    def twin_searchsorted(key, query):
        left, right = T.searchsorted(key.vals.numpy().reshape(-1), [0], [key.vals.shape[-1]], query.vals.numpy(),
                                     np.zeros(query.vals.numel(), np.int64), local=True)
        return torch.from_numpy(left).view(query.vals.shape), torch.from_numpy(right).view(query.vals.shape)

    with mock.patch.object(prop_net, "searchsorted", twin_searchsorted):
        cq = torch.tensor([[0.0, 0.5, 1.0]])
        loss = prop_net._pdf_loss(q, cq, k, torch.tensor([[0.0, 0.4, 0.9, 1.0]]), eps=0.0)
        assert torch.allclose(loss, torch.zeros(1, 2))
        loss = prop_net._pdf_loss(q, cq, k, torch.tensor([[0.0, 0.1, 0.2, 0.3]]), eps=0.0)
        # intervals [0, .5] and [.5, 1] are covered by key intervals [0, .75] and [.25, 1]: w_outer .2, .2
        assert torch.allclose(loss, torch.tensor([[0.3 ** 2 / 0.5, 0.3 ** 2 / 0.5]]))


def test_pdf_rows_mirror_has_the_header_layout(tmp_path):
    from cnc_amd import _lib
    names = [f[0] for f in _lib.PdfRows._fields_]
    seg = [f[0] for f in _lib.RaySegments._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include <stdint.h>', '#include "cnc_hip.h"',
             'int main(void) {', '  printf("size %zu\\n", sizeof(cnc_pdf_rows_t));']
    lines += [f'  printf("{n} %zu\\n", offsetof(cnc_pdf_rows_t, {n}));' for n in names]
    lines += [f'  printf("seg.{n} %zu\\n", offsetof(cnc_pdf_rows_t, seg.{n}));' for n in seg]
    lines += ['  return 0;', '}']
    src = tmp_path / "pdf_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "pdf_layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.splitlines())
    assert int(out["size"]) == ctypes.sizeof(_lib.PdfRows)
    for n in names:
        assert int(out[n]) == getattr(_lib.PdfRows, n).offset, n
    for n in seg:
        assert int(out["seg." + n]) == _lib.PdfRows.seg.offset + getattr(_lib.RaySegments, n).offset, n
    assert _lib.ABI_VERSION == 33       # the rows struct arrived with v32; v33 removed fused-field members only


def test_proposal_api_refuses_cpu_tensors():
    """No CPU fallback: the proposal route raises on host tensors like the reference's CHECK_CUDA."""
    from cnc_amd.nerfacc import RayIntervals, importance_sampling, searchsorted
    iv = RayIntervals(vals=torch.tensor([[0.0, 1.0]]))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        importance_sampling(iv, torch.tensor([[0.0, 1.0]]), 4)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        searchsorted(iv, iv)
