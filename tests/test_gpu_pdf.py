"""GPU: the proposal-sampling kernels (cnc_amd/csrc/pdf.hip) through the nerfacc API, bit-equal to the NumPy twin
(tests/pdf_twin.py) over batched and flattened inputs and outputs, the LDS and the global route, the defined edge
cases, stratified sampling, out-of-bounds guards and host synchronisation."""
import ctypes

import numpy as np
import pytest
import torch

import pdf_twin as T

pytestmark = pytest.mark.gpu
f32, i64 = np.float32, np.int64
CAP = 512             # kPdfCap of pdf.hip: longer rows take the global route
BIG = CAP + 88


def _bits_equal(got, want):
    """Bit-equal, except that any NaN matches any NaN (the payload and sign of a NaN are not specified)."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    if got.shape != want.shape:
        return False
    same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    return bool(same.all())


def _rows(rng, counts, flat_every=5, nan_every=0):
    """Flattened segments with the given edge counts: sorted t in [0, 10), CDFs sorted in [0, 1] with flat runs."""
    vals, cdfs = [], []
    for r, c in enumerate(counts):
        v = np.sort(rng.uniform(0, 10, c)).astype(f32)
        u = np.sort(rng.uniform(0, 1, c)).astype(f32)
        if c > 3 and r % flat_every == 1:
            u[c // 3: 2 * c // 3] = u[c // 3]         # a flat run: the < 1e-10 branch
        if c > 2 and r % flat_every == 2:
            u[:] = u[0]                               # an entirely flat CDF
        if nan_every and c > 1 and r % nan_every == 3:
            u[c // 2] = np.nan
        vals.append(v)
        cdfs.append(u)
    cnts = np.asarray(counts, i64)
    starts = np.cumsum(cnts) - cnts
    cat = lambda xs: np.concatenate(xs).astype(f32) if xs else np.zeros(0, f32)   # noqa: E731
    return cat(vals), cat(cdfs), starts, cnts


def _intervals(cuda, vals, starts, cnts, batched_E=None):
    from cnc_amd.nerfacc import RayIntervals
    v = torch.from_numpy(vals).to(cuda)
    if batched_E is not None:
        return RayIntervals(vals=v.view(-1, batched_E))
    info = torch.from_numpy(np.stack([starts, cnts], -1)).to(cuda)
    return RayIntervals(vals=v, packed_info=info)


def _check_packed(iv, sm, want):
    assert _bits_equal(sm.vals.cpu().numpy(), want["samples"])
    assert _bits_equal(iv.vals.cpu().numpy(), want["edges"])
    assert np.array_equal(sm.packed_info[:, 0].cpu().numpy(), want["sample_starts"])
    assert np.array_equal(iv.packed_info[:, 0].cpu().numpy(), want["edge_starts"])
    assert np.array_equal(iv.packed_info[:, 1].cpu().numpy(), want["edge_cnts"])
    assert np.array_equal(sm.ray_indices.cpu().numpy(), want["sample_rays"])
    assert np.array_equal(iv.ray_indices.cpu().numpy(), want["edge_rays"])
    assert np.array_equal(iv.is_left.cpu().numpy(), want["is_left"])
    assert np.array_equal(iv.is_right.cpu().numpy(), want["is_right"])


@pytest.mark.parametrize("E", [2, 3, 64, 65, 257, BIG])
def test_batched_in_batched_out(cuda, E):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(E)
    n_rays = 23
    vals, cdfs, starts, cnts = _rows(rng, [E] * n_rays, nan_every=7)
    iv = _intervals(cuda, vals, starts, cnts, batched_E=E)
    for n in (0, 1, 2, 63, 64, 65, 257, 1000):
        out_iv, sm = importance_sampling(iv, torch.from_numpy(cdfs).to(cuda).view(n_rays, E), n)
        s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, n)
        assert sm.vals.shape == (n_rays, n) and out_iv.vals.shape == (n_rays, n + 1)
        assert sm.packed_info is None and out_iv.packed_info is None
        assert _bits_equal(sm.vals.cpu().numpy(), s), (E, n)
        assert _bits_equal(out_iv.vals.cpu().numpy(), e), (E, n)


def test_batched_leading_axes_kept(cuda):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(3)
    vals, cdfs, starts, cnts = _rows(rng, [9] * 12)
    iv = _intervals(cuda, vals, starts, cnts, batched_E=9)
    iv.vals = iv.vals.view(3, 4, 9)
    out_iv, sm = importance_sampling(iv, torch.from_numpy(cdfs).to(cuda).view(3, 4, 9), 5)
    assert sm.vals.shape == (3, 4, 5) and out_iv.vals.shape == (3, 4, 6)
    s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, 5)
    assert _bits_equal(sm.vals.cpu().numpy().reshape(12, 5), s)
    assert _bits_equal(out_iv.vals.cpu().numpy().reshape(12, 6), e)


@pytest.mark.parametrize("seed", [0, 1])
def test_packed_in_packed_out(cuda, seed):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(10 + seed)
    n_rays = 60
    counts = rng.choice([0, 1, 2, 3, 64, 65, 257, BIG], n_rays)
    vals, cdfs, starts, cnts = _rows(rng, counts, nan_every=11)
    n = rng.choice([0, 1, 2, 63, 64, 65, 257, 1000], n_rays).astype(i64)
    iv = _intervals(cuda, vals, starts, cnts)
    out_iv, sm = importance_sampling(iv, torch.from_numpy(cdfs).to(cuda), torch.from_numpy(n).to(cuda))
    _check_packed(out_iv, sm, T.importance_sampling(vals, cdfs, starts, cnts, n))


def test_packed_in_batched_out_and_batched_in_packed_out(cuda):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(20)
    counts = rng.choice([1, 2, 3, 64, 65, 257, BIG], 40)
    vals, cdfs, starts, cnts = _rows(rng, counts)
    out_iv, sm = importance_sampling(_intervals(cuda, vals, starts, cnts), torch.from_numpy(cdfs).to(cuda), 65)
    s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, 65)
    assert sm.vals.shape == (40, 65) and _bits_equal(sm.vals.cpu().numpy(), s)
    assert _bits_equal(out_iv.vals.cpu().numpy(), e)

    vals, cdfs, starts, cnts = _rows(rng, [65] * 30)
    n = rng.choice([0, 1, 2, 63, 64, 65, 257, 1000], 30).astype(i64)
    iv = _intervals(cuda, vals, starts, cnts, batched_E=65)
    out_iv, sm = importance_sampling(iv, torch.from_numpy(cdfs).to(cuda).view(30, 65), torch.from_numpy(n).to(cuda))
    _check_packed(out_iv, sm, T.importance_sampling(vals, cdfs, starts, cnts, n))


def test_supplied_jitter_and_u_outside_the_cdf(cuda):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(30)
    for E in (2, 65, BIG):
        vals, cdfs, starts, cnts = _rows(rng, [E] * 17)
        jit = rng.uniform(0, 1, 17).astype(f32)
        jit[:4] = [0.0, np.nextafter(f32(1), f32(0)), 1.5, -1.0]     # bounds of [0, 1), and u outside the CDF
        iv = _intervals(cuda, vals, starts, cnts, batched_E=E)
        for n in (1, 64, 257):
            out_iv, sm = importance_sampling(iv, torch.from_numpy(cdfs).to(cuda).view(17, E), n,
                                             jitter=torch.from_numpy(jit).to(cuda))
            s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, n, jit)
            assert _bits_equal(sm.vals.cpu().numpy(), s) and _bits_equal(out_iv.vals.cpu().numpy(), e), (E, n)


def test_docstring_examples_on_the_device(cuda):
    """nerfacc/pdf.py:39-56,104-120 through `nerfacc` as the drop-ins install it."""
    import cnc_amd
    cnc_amd.install_dropins()
    import nerfacc
    import nerfacc.pdf
    from nerfacc import RayIntervals
    seq = RayIntervals(vals=torch.tensor([0.0, 1.0, 0.0, 1.0, 2.0], device=cuda),
                       packed_info=torch.tensor([[0, 2], [2, 3]], device=cuda))
    vals = RayIntervals(vals=torch.tensor([0.5, 1.5, 2.5], device=cuda),
                        packed_info=torch.tensor([[0, 1], [1, 2]], device=cuda))
    left, right = nerfacc.pdf.searchsorted(seq, vals)
    assert left.tolist() == [0, 3, 3] and right.tolist() == [1, 4, 4]
    assert seq.vals.gather(-1, left).tolist() == [0.0, 1.0, 1.0] and seq.vals.gather(-1, right).tolist() == [1.0, 2.0, 2.0]
    iv, sm = nerfacc.importance_sampling(seq, torch.tensor([0.0, 0.5, 0.0, 0.5, 1.0], device=cuda), 2)
    assert iv.vals.tolist() == [[0.0, 0.5, 1.0], [0.0, 1.0, 2.0]]
    assert sm.vals.tolist() == [[0.25, 0.75], [0.5, 1.5]]


def _search_case(rng, n_rays, key_counts, q_per_row):
    kv, _, ks, kc = _rows(rng, key_counts)
    q = rng.uniform(-1, 11, (n_rays, q_per_row)).astype(f32)
    q[:, 0] = np.nan
    for r in range(n_rays):
        if kc[r] > 2 and q_per_row >= 3:
            q[r, 1:3] = kv[ks[r]: ks[r] + 2]          # exactly on a key
    return kv, ks, kc, q


@pytest.mark.parametrize("key_batched", [True, False])
def test_searchsorted_batched_query(cuda, key_batched):
    from cnc_amd.nerfacc import RayIntervals, searchsorted
    rng = np.random.default_rng(40 + key_batched)
    for K in (2, 3, 65, 257, BIG):
        counts = [K] * 19 if key_batched else list(rng.choice([0, 1, 2, 3, 65, 257, BIG], 19))
        kv, ks, kc, q = _search_case(rng, 19, counts, 49)
        key = _intervals(cuda, kv, ks, kc, batched_E=K if key_batched else None)
        query = RayIntervals(vals=torch.from_numpy(q).to(cuda))
        left, right = searchsorted(key, query)
        wl, wr = T.searchsorted(kv, ks, kc, q, np.repeat(np.arange(19), 49), local=True)
        assert left.shape == q.shape
        assert np.array_equal(left.cpu().numpy().reshape(-1), wl) and np.array_equal(right.cpu().numpy().reshape(-1), wr)


@pytest.mark.parametrize("key_batched", [True, False])
@pytest.mark.parametrize("with_ray_indices", [True, False])
def test_searchsorted_flattened_query(cuda, key_batched, with_ray_indices):
    from cnc_amd.nerfacc import RayIntervals, searchsorted
    rng = np.random.default_rng(50 + 2 * key_batched + with_ray_indices)
    for K in (2, 65, BIG):
        counts = [K] * 21 if key_batched else list(rng.choice([0, 1, 2, 65, BIG], 21))
        kv, ks, kc, _ = _search_case(rng, 21, counts, 1)
        qc = rng.choice([0, 1, 5, 64, 65, 130], 21).astype(i64)
        qs = np.cumsum(qc) - qc
        qv = rng.uniform(-1, 11, int(qc.sum())).astype(f32)
        qv[::17] = np.nan
        rays = np.repeat(np.arange(21), qc)
        key = _intervals(cuda, kv, ks, kc, batched_E=K if key_batched else None)
        query = RayIntervals(vals=torch.from_numpy(qv).to(cuda), packed_info=torch.from_numpy(np.stack([qs, qc], -1)).to(cuda),
                             ray_indices=torch.from_numpy(rays).to(cuda) if with_ray_indices else None)
        left, right = searchsorted(key, query)
        q_rays = rays if with_ray_indices else T.query_rays_from_starts(qs, len(qv))
        wl, wr = T.searchsorted(kv, ks, kc, qv, q_rays, local=False)
        assert np.array_equal(left.cpu().numpy(), wl) and np.array_equal(right.cpu().numpy(), wr)


def test_stratified_through_the_api(cuda):
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(60)
    vals, cdfs, starts, cnts = _rows(rng, [33] * 50)
    iv = _intervals(cuda, vals, starts, cnts, batched_E=33)
    c = torch.from_numpy(cdfs).to(cuda).view(50, 33)
    torch.manual_seed(7)
    a_iv, a_sm = importance_sampling(iv, c, 40, stratified=True)
    torch.manual_seed(7)
    b_iv, b_sm = importance_sampling(iv, c, 40, stratified=True)
    assert torch.equal(a_sm.vals, b_sm.vals) and torch.equal(a_iv.vals, b_iv.vals)
    # one bias per ray, drawn by torch.rand on the device: the twin with that draw as its jitter is bit-equal
    torch.manual_seed(7)
    jit = torch.rand(50, device=cuda).cpu().numpy()
    assert ((jit >= 0) & (jit < 1)).all()
    s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, 40, jit)
    assert _bits_equal(a_sm.vals.cpu().numpy(), s) and _bits_equal(a_iv.vals.cpu().numpy(), e)
    assert not torch.equal(a_sm.vals, importance_sampling(iv, c, 40)[1].vals)
    # edges monotone and inside [vals[base], vals[last]]
    ev = a_iv.vals.cpu().numpy()
    v = vals.reshape(50, 33)
    assert (np.diff(ev, axis=1) >= 0).all()
    assert (ev >= v[:, :1]).all() and (ev <= v[:, -1:]).all()
    # the packed output draws its biases the same way
    n = torch.full((50,), 40, dtype=torch.int64, device=cuda)
    torch.manual_seed(7)
    p_iv, p_sm = importance_sampling(iv, c, n, stratified=True)
    assert torch.equal(p_sm.vals.view(50, 40), a_sm.vals) and torch.equal(p_iv.vals.view(50, 41), a_iv.vals)


def test_batched_calls_do_not_synchronise(cuda):
    from cnc_amd.nerfacc import RayIntervals, importance_sampling, searchsorted
    rng = np.random.default_rng(70)
    vals, cdfs, starts, cnts = _rows(rng, [65] * 64)
    iv = _intervals(cuda, vals, starts, cnts, batched_E=65)
    c = torch.from_numpy(cdfs).to(cuda).view(64, 65)
    importance_sampling(iv, c, 48, stratified=True)      # warm up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out_iv, sm = importance_sampling(iv, c, 48, stratified=True)
        out_iv2, _ = importance_sampling(out_iv, c[:, :49].contiguous(), 16)
        searchsorted(out_iv, RayIntervals(vals=out_iv2.vals))
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_no_write_past_a_ray_row(cuda):
    """Every output buffer of the C ABI is followed by a guard of sentinel values that must survive, for
    n = 1 (the reference's FIXME read / uninitialised edge), n = 65 and the flattened layout."""
    from cnc_amd import _lib
    rng = np.random.default_rng(80)
    L = _lib.lib()
    G = 4096
    for E, n_list in ((2, [1, 65]), (BIG, [1, 65])):
        vals, cdfs, starts, cnts = _rows(rng, [E] * 37)
        v, c = torch.from_numpy(vals).to(cuda), torch.from_numpy(cdfs).to(cuda)
        seg = _lib.PdfRows(_lib.RaySegments(v.data_ptr(), None, None, None, None, None, None), 37, E, v.numel())
        for n in n_list:
            sbuf = torch.full((37 * n + G,), -7.0, device=cuda)
            ebuf = torch.full((37 * (n + 1) + G,), -7.0, device=cuda)
            smp = _lib.PdfRows(_lib.RaySegments(sbuf.data_ptr(), None, None, None, None, None, None), 37, n, 37 * n)
            itv = _lib.PdfRows(_lib.RaySegments(ebuf.data_ptr(), None, None, None, None, None, None), 37, n + 1,
                               37 * (n + 1))
            _lib.check(L.cnc_importance_sampling(ctypes.byref(seg), c.data_ptr(), None, ctypes.byref(smp),
                                                 ctypes.byref(itv), _lib.stream(cuda)), "importance_sampling")
            s, e = T.importance_sampling_batched(vals, cdfs, starts, cnts, n)
            assert _bits_equal(sbuf[:37 * n].cpu().numpy(), s.reshape(-1))
            assert _bits_equal(ebuf[:37 * (n + 1)].cpu().numpy(), e.reshape(-1))
            assert (sbuf[37 * n:] == -7.0).all() and (ebuf[37 * (n + 1):] == -7.0).all()
    # flattened output: every per-entry buffer guarded
    counts = rng.choice([0, 1, 2, 65, BIG], 29)
    vals, cdfs, starts, cnts = _rows(rng, counts)
    n = rng.choice([0, 1, 2, 65, 257], 29).astype(i64)
    want = T.importance_sampling(vals, cdfs, starts, cnts, n)
    S, Ee = len(want["samples"]), len(want["edges"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)     # noqa: E731
    v, c, st, ct = t(vals), t(cdfs), t(starts), t(cnts)
    sv, sri = torch.full((S + G,), -7.0, device=cuda), torch.full((S + G,), -7, dtype=torch.int64, device=cuda)
    ev, eri = torch.full((Ee + G,), -7.0, device=cuda), torch.full((Ee + G,), -7, dtype=torch.int64, device=cuda)
    el, er = torch.full((Ee + G,), 9, dtype=torch.uint8, device=cuda), torch.full((Ee + G,), 9, dtype=torch.uint8, device=cuda)
    s_starts, s_cnts = t(want["sample_starts"]), t(n)
    e_starts, e_cnts = t(want["edge_starts"]), t(want["edge_cnts"])
    seg = _lib.PdfRows(_lib.RaySegments(v.data_ptr(), st.data_ptr(), ct.data_ptr(), None, None, None, None), 29, -1,
                       v.numel())
    smp = _lib.PdfRows(_lib.RaySegments(sv.data_ptr(), s_starts.data_ptr(), s_cnts.data_ptr(), sri.data_ptr(), None,
                                        None, None), 29, -1, S)
    itv = _lib.PdfRows(_lib.RaySegments(ev.data_ptr(), e_starts.data_ptr(), e_cnts.data_ptr(), eri.data_ptr(),
                                        el.data_ptr(), er.data_ptr(), None), 29, -1, Ee)
    _lib.check(L.cnc_importance_sampling(ctypes.byref(seg), c.data_ptr(), None, ctypes.byref(smp), ctypes.byref(itv),
                                         _lib.stream(cuda)), "importance_sampling")
    assert _bits_equal(sv[:S].cpu().numpy(), want["samples"]) and _bits_equal(ev[:Ee].cpu().numpy(), want["edges"])
    assert np.array_equal(sri[:S].cpu().numpy(), want["sample_rays"]) and np.array_equal(eri[:Ee].cpu().numpy(), want["edge_rays"])
    assert np.array_equal(el[:Ee].cpu().numpy().astype(bool), want["is_left"])
    assert np.array_equal(er[:Ee].cpu().numpy().astype(bool), want["is_right"])
    assert (sv[S:] == -7).all() and (sri[S:] == -7).all() and (ev[Ee:] == -7).all() and (eri[Ee:] == -7).all()
    assert (el[Ee:] == 9).all() and (er[Ee:] == 9).all()


def test_last_row_ends_a_fresh_allocation(cuda):
    """Outputs sized to whole 2 MiB allocator segments in a fresh pool: the last ray's row ends where the mapping
    may end (tests/test_gpu_mlp.py uses the same trick), for n = 1 and for the flattened layout."""
    from cnc_amd.nerfacc import importance_sampling
    rng = np.random.default_rng(90)
    n_rays = 1 << 19                                   # (n_rays, 1) f32 = 2 MiB, (n_rays, 2) = 4 MiB
    vals = np.sort(rng.uniform(0, 10, (n_rays, 2)), axis=1).astype(f32)
    cdfs = np.tile(np.array([0.0, 1.0], f32), (n_rays, 1))
    iv = _intervals(cuda, vals.reshape(-1), None, None, batched_E=2)
    c = torch.from_numpy(cdfs).to(cuda)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out_iv, sm = importance_sampling(iv, c, 1)
    starts = np.arange(n_rays, dtype=i64) * 2
    s, e = T.importance_sampling_batched(vals.reshape(-1), cdfs.reshape(-1), starts, np.full(n_rays, 2, i64), 1)
    assert _bits_equal(sm.vals.cpu().numpy(), s) and _bits_equal(out_iv.vals.cpu().numpy(), e)
    del out_iv, sm
    n = torch.full((n_rays // 8,), 8, dtype=torch.int64, device=cuda)      # 2^19 samples: 2 MiB of f32
    sub = _intervals(cuda, vals[: n_rays // 8].reshape(-1), None, None, batched_E=2)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out_iv, sm = importance_sampling(sub, c[: n_rays // 8].contiguous(), n)
    want = T.importance_sampling(vals[: n_rays // 8].reshape(-1), cdfs[: n_rays // 8].reshape(-1), starts[: n_rays // 8],
                                 np.full(n_rays // 8, 2, i64), np.full(n_rays // 8, 8, i64))
    _check_packed(out_iv, sm, want)
