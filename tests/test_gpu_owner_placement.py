"""The paired owner placement (CNC_FLAG_OWNER_XCD_PAIRS: the owner waves of two binned levels on complementary halves of
the workgroup labels, grid_encode_binned.hip owner_slab) gives the gradient of the default placement: against the CPU
oracle's float64 shadow with the bound of test_gpu_binned_backward.py (`_check_bwd`: (n + 2) eps sum|terms| per entry), and
against the default placement itself with that file's figures (1e-5 of the largest entry; 2e-5 for coherent points).  The
id decoding itself is checked slab by slab, without a GPU, in test_owner_grid.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import make_grid
from test_gpu_encoder import _check_bwd, _points

pytestmark = pytest.mark.gpu

RES7 = [6, 14, 31, 44, 60, 83, 120]    # log2_T = 10: level 0 dense with 216 rows (a partial slab), 1-6 hashed, 1024 rows


def _bwd_binned(dev, g, x, emb, offs, res, n_binned, level_rows, paired, ste=False, ld=0, col=0, g_dev=None, want_ws=False):
    from cnc_amd import _lib
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)
    L = len(res)
    N, D = x.shape
    F = emb.shape[1]
    lib = _lib.lib()
    ws_bytes = int(lib.cnc_grid_encode_backward_binned_workspace(N, n_binned, level_rows))
    ws = torch.full((max(ws_bytes, 4),), 0xAB, dtype=torch.uint8, device=dev)   # library must clear it
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=dev)
    gd = t(g) if g_dev is None else g_dev
    xd, ed, od, rd = t(x), t(emb), t(offs), t(res)
    flags = (_lib.CNC_FLAG_STE_BINARY if ste else 0) | (_lib.CNC_FLAG_OWNER_XCD_PAIRS if paired else 0)
    rc = lib.cnc_grid_encode_backward_binned(
        gd.data_ptr(), xd.data_ptr(), ed.data_ptr(), od.data_ptr(), rd.data_ptr(), ge.data_ptr(),
        N, D, F, L, flags, None, ld, col, n_binned, level_rows, ws.data_ptr(), ws_bytes, _lib.stream())
    _lib.check(rc, "binned")
    torch.cuda.synchronize()
    if want_ws:
        return ge.cpu().numpy(), ws.cpu().numpy()
    return ge.cpu().numpy()


def _shadow(oracle, g, x, emb, offs, resl, ste):
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=ste, want_acc64=True)
    _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, resl, ste_binary=ste, want_acc64=True)
    return want32, acc64, abs64


@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("ste", [False, True])
@pytest.mark.parametrize("n_binned", [1, 2, 3, 4, 5, 6])
def test_paired_placement_against_float64_shadow(cuda, oracle, F, ste, n_binned):
    """Pairs only (2, 4, 6), a pair plus a level without a partner (3, 5), and no pair at all (1); 4 bins per level, so
    the paired ranges carry padding ids."""
    offs, resl, emb = make_grid(RES7, 10, 3, F, seed=41)
    x = _points(9001, 3, seed=42)
    g = np.random.default_rng(43).normal(size=(len(RES7), x.shape[0], F)).astype(np.float32)
    want32, acc64, abs64 = _shadow(oracle, g, x, emb, offs, resl, ste)
    new = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 1024, True, ste=ste)
    _check_bwd(new, want32, acc64, abs64, n_terms_max=x.shape[0] * 8)
    if ste:
        assert np.all(new[np.abs(emb) > 1] == 0)
    old = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 1024, False, ste=ste)
    assert np.abs(new - old).max() <= 1e-5 * np.abs(old).max()


@pytest.mark.parametrize("level_rows", [700, 1024, 1280, 3300])
@pytest.mark.parametrize("n_binned", [2, 5])
def test_paired_placement_bin_counts_off_the_multiple_of_eight(cuda, oracle, level_rows, n_binned):
    """3 bins (fewer rows than the hashed levels have: those levels go to atomics entirely, and the ids of the padding must
    not read their neighbours' counters), 4, 5 and 13 bins per level."""
    F = 8
    offs, resl, emb = make_grid(RES7, 10, 3, F, seed=51)
    x = _points(6000, 3, seed=52)
    g = np.random.default_rng(53).normal(size=(len(RES7), x.shape[0], F)).astype(np.float32)
    want32, acc64, abs64 = _shadow(oracle, g, x, emb, offs, resl, True)
    new = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, level_rows, True, ste=True)
    _check_bwd(new, want32, acc64, abs64, n_terms_max=x.shape[0] * 8)
    old = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, level_rows, False, ste=True)
    assert np.abs(new - old).max() <= 1e-5 * np.abs(old).max()


@pytest.mark.parametrize("N", [1, 63, 4097, 70001])
@pytest.mark.parametrize("n_binned", [3, 6])
def test_paired_placement_ragged_sizes(cuda, oracle, N, n_binned):
    offs, resl, emb = make_grid(RES7, 10, 3, 8, seed=61)
    x = _points(N, 3, seed=62)
    g = np.random.default_rng(63).normal(size=(len(RES7), N, 8)).astype(np.float32)
    want32, acc64, abs64 = _shadow(oracle, g, x, emb, offs, resl, False)
    new = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 1024, True)
    _check_bwd(new, want32, acc64, abs64, n_terms_max=N * 8)
    old = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 1024, False)
    assert np.abs(new - old).max() <= 1e-5 * max(np.abs(old).max(), 1e-6)


@pytest.mark.parametrize("n_binned", [3, 4])
def test_paired_placement_overloaded_bins_run_their_extra_waves(cuda, oracle, n_binned):
    """Two thirds of the points sit in one cell of every binned level (a cube a thousandth of the unit cube wide, clear of
    the cell faces of resolutions 44 to 120): their 4 x 6000 items per level go to at most 4 of the 16 bins, each more
    than one wave's share, so the `part` > 0 waves of those bins run and add their partial slabs atomically."""
    F, N = 8, 9000
    offs, resl, emb = make_grid(RES7, 12, 3, F, seed=91)
    rng = np.random.default_rng(92)
    x = rng.uniform(0.05, 0.95, size=(N, 3)).astype(np.float32)
    x[:6000] = 0.4 + x[:6000] / 1000.0
    x = x[np.lexsort((x[:, 0], x[:, 1], x[:, 2]))]
    g = rng.normal(size=(len(RES7), N, F)).astype(np.float32)
    want32, acc64, abs64 = _shadow(oracle, g, x, emb, offs, resl, True)
    new, ws = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 4096, True, ste=True, want_ws=True)
    _check_bwd(new, want32, acc64, abs64, n_terms_max=N * 8)
    # the bin counters lead the workspace; `part` as owner_part() sizes it: twice the mean load
    bins = 16
    mean = (4 * N + bins - 1) // bins
    part = max(64, (2 * mean + 63) // 64 * 64)
    counts = ws[: n_binned * bins * 4].view(np.uint32).reshape(n_binned, bins)
    assert counts.sum() >= 4 * 8000 * n_binned and np.all(counts.max(axis=1) > part)
    old = _bwd_binned(cuda, g, x, emb, offs, resl, n_binned, 4096, False, ste=True)
    assert np.abs(new - old).max() <= 2e-5 * np.abs(old).max()


def test_paired_placement_point_major_gradient(cuda, oracle):
    """grad_ld / grad_col: the gradient read in place from a wider [N, ld] matrix."""
    F, N, ld, col = 4, 5000, 40, 8
    offs, resl, emb = make_grid(RES7, 10, 3, F, seed=71)
    x = _points(N, 3, seed=72)
    g = np.random.default_rng(73).normal(size=(len(RES7), N, F)).astype(np.float32)
    wide = torch.randn(N, ld, device=cuda)
    wide[:, col:col + len(RES7) * F] = torch.as_tensor(g, device=cuda).permute(1, 0, 2).reshape(N, -1)
    want32, acc64, abs64 = _shadow(oracle, g, x, emb, offs, resl, False)
    new = _bwd_binned(cuda, None, x, emb, offs, resl, 5, 1024, True, ld=ld, col=col, g_dev=wide.contiguous())
    _check_bwd(new, want32, acc64, abs64, n_terms_max=N * 8)
    old = _bwd_binned(cuda, None, x, emb, offs, resl, 5, 1024, False, ld=ld, col=col, g_dev=wide.contiguous())
    assert np.abs(new - old).max() <= 1e-5 * np.abs(old).max()


@pytest.mark.parametrize("group_split", [None, "2", "4", "3"])
def test_paired_placement_through_the_overlapped_entry(cuda, oracle, monkeypatch, group_split):
    """cnc_grid_encode_backward_overlapped as a C host calls it, on a non-default stream with the caller's own scratch of
    the size the library asks for, next to the coarse levels: the six finest levels as one group (the default) or,
    CNC_BWD_GROUP_SPLIT read at plan creation, as 2 + 4 / 4 + 2 / 3 + 3 (a pair cut in two)."""
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    from cnc_amd.synthetic import RES_16L, level_offsets
    F, L, N = 8, 16, (1 << 16) + 77
    offs = level_offsets(RES_16L, 19, 3)
    gen = np.random.default_rng(9)
    emb = np.sign(gen.uniform(-1, 1, size=(int(offs[-1]), F))).astype(np.float32)
    x = gen.uniform(0, 1, size=(N, 3)).astype(np.float32)
    g = gen.normal(size=(L, N, F)).astype(np.float32)
    resl = np.asarray(RES_16L, np.int32)
    n_binned, level_rows = be.plan_binned_levels(RES_16L, [int(v) for v in offs], 3, F, N, min_work=0)
    assert n_binned == 6
    threads = oracle.max_threads()
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, np.asarray(offs, np.int32), resl, ste_binary=True, want_acc64=True,
                                                threads=threads)
    _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, np.asarray(offs, np.int32), resl, ste_binary=True,
                                           want_acc64=True, threads=threads)
    lib = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    t = lambda a: torch.as_tensor(a, device=cuda)
    gd, xd, ed, od, rd = t(g), t(x), t(emb), t(np.asarray(offs, np.int32)), t(resl)
    if group_split is None:
        monkeypatch.delenv("CNC_BWD_GROUP_SPLIT", raising=False)
    else:
        monkeypatch.setenv("CNC_BWD_GROUP_SPLIT", group_split)
    plan = C.c_void_p()
    assert lib.cnc_backward_plan_create(C.byref(plan)) == 0 and plan.value
    nbytes = int(lib.cnc_grid_encode_backward_overlapped_workspace(N, n_binned, level_rows))
    assert nbytes >= int(lib.cnc_grid_encode_backward_binned_workspace(N, n_binned, level_rows))
    outs = []
    side = torch.cuda.Stream(device=cuda)
    for paired in (True, False):
        ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=cuda)
        got = torch.empty_like(ed)
        flags = _lib.CNC_FLAG_STE_BINARY | (_lib.CNC_FLAG_OWNER_XCD_PAIRS if paired else 0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(2):                           # a plan is reusable call after call
                got.zero_()                              # queued on the caller's stream right before
                rc = lib.cnc_grid_encode_backward_overlapped(plan, p(gd), p(xd), p(ed), p(od), p(rd), p(got), N, 3, F, L,
                                                             flags, None, 0, 0, n_binned, level_rows, p(ws), ws.numel(),
                                                             C.c_void_p(side.cuda_stream))
                assert rc == 0
            snap = got.clone()                           # queued right after: must see both halves
        side.synchronize()
        outs.append(snap.cpu().numpy())
    assert lib.cnc_backward_plan_destroy(plan) == 0
    new, old = outs
    _check_bwd(new, want32, acc64, abs64, n_terms_max=N * 8)
    assert np.abs(new - old).max() <= 1e-5 * np.abs(old).max()
    assert np.abs(new[: int(offs[1])]).max() > 0 and np.abs(new[int(offs[-2]):]).max() > 0
