"""The chain walk and the wave prefixes of k_grid_encode_bwd_merge (grid_encode_merge.hip) on point sets made to give the
walk every shape it has code for, against the oracle's float64 sums with the bound of tests/test_gpu_merge_tiles.py:
every table entry within (n_e + 2) * eps * sum|terms| of the float64 sum, the two tilings within twice that bound of
each other; the coarse call and the overlapped entry, STE on and off.

Two forms of the kernel: 1,024 threads per block (N = 8 * 1,024 + 1 with as many small levels as launch_bwd_merge wants
for it: `_run_case` of test_gpu_merge_tiles, which also checks the segment order the tiled form left in the scratch) and
512 threads (`small`: N = 4 * 512 + 1 with ten coarse levels).  Both N are a whole number of blocks plus one sample.

The shapes are shapes of the runs (consecutive samples of one cell) and chains (runs of one cell) of a block of MB
consecutive samples.  Which samples share a cell depends on the level, and on the levels of R >= 52 the tiled form takes
other samples than consecutive ones, so each shape is built for, and asserted on (`_block_shapes`, numpy, before anything
runs on the GPU), the level of R = 31: fine enough for 1,024 distinct cells, coarse enough to keep consecutive samples in
either form.  Every other level of the call sees some other mix of runs and is checked all the same.

  one_cell        all samples of a block in one cell: ONE lone run of MB samples, which the walk splits in two halves
  alternating     two cells, sample by sample: two chains of MB / 2 runs of length 1 (even number of runs: all pairs)
  run_cycle       run lengths 1, 2, 3, 4, 5, 7, 8, 9 in a fixed cycle over three cells: chains of an odd and of an even
                  number of runs (the last run of an odd chain is a lone run that splits), partial MFMA steps
  outside_cut     runs of nine with the fifth sample outside the unit cube: its key ~0 cuts the run in 4 + 4
  distinct        every sample of a block opens a cell of its own: MB runs, MB chains of one run of one sample
  wave_edges      run heads on lane 63 of one wave and lane 0 of the next, for every pair of neighbouring waves: a run
                  number is the exclusive prefix of the earlier waves' head counts plus the heads below the lane, and
                  s_run_start[run + 1] is the run's end — a prefix that loses or gains a wave's count moves every later
                  run's samples to the wrong cell, far outside the bound
"""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_grid

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_merge_tiles import EPS, RES_BINNED, RES_CYCLE, _check, _coarse, _levels_for, _run_case  # noqa: E402

pytestmark = pytest.mark.gpu

R_SHAPE = 31                                 # the level the shapes are built for (in RES_CYCLE, below kMergeTileMinRes)
RUN_CYCLE = [1, 2, 3, 4, 5, 7, 8, 9]
SHAPES = ["one_cell", "alternating", "run_cycle", "outside_cut", "distinct", "wave_edges"]


def _cells(x, R):
    """Cell key per sample on a level of resolution R (the float32 arithmetic of Corners::setup), -1 outside [0, 1]."""
    x = np.asarray(x, np.float32)
    p = x * np.float32(R - 2) + np.float32(0.5)
    c = np.floor(p).astype(np.int64)
    key = c[:, 0] | c[:, 1] << 16 | c[:, 2] << 32
    return np.where(((x < 0) | (x > 1)).any(axis=1), -1, key)


def _block_shapes(x, R, MB):
    """Per block of MB consecutive samples: the lengths of its runs, in order, and the runs per chain (outside points cut
    runs and join no chain)."""
    key = _cells(x, R)
    out = []
    for b0 in range(0, len(key), MB):
        k = key[b0:b0 + MB]
        heads = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
        lens = np.diff(np.r_[heads, len(k)])
        inside = k[heads] >= 0
        chains = {}
        for h in heads[inside]:
            chains[int(k[h])] = chains.get(int(k[h]), 0) + 1
        out.append({"lens": lens[inside], "heads": heads, "chains": np.asarray(sorted(chains.values()))})
    return out


def _centre(c):
    """The centre of cell c (three integers) of the R_SHAPE level: fractions of one half, far from any rounding."""
    return (np.asarray(c, np.float64) / (R_SHAPE - 2)).astype(np.float32)


P = [_centre((5, 9, 14)), _centre((20, 6, 11)), _centre((12, 22, 3))]


def _points(shape, N, MB):
    x = np.empty((N, 3), np.float32)
    i = np.arange(N)
    if shape == "one_cell":
        x[:] = P[0]
    elif shape == "alternating":
        x[:] = np.where((i % 2 == 0)[:, None], P[0], P[1])
    elif shape in ("run_cycle", "outside_cut"):
        lens = RUN_CYCLE if shape == "run_cycle" else [9]
        n_cells = 3 if shape == "run_cycle" else 2
        at, r = 0, 0
        while at < N:
            n = lens[r % len(lens)]
            x[at:at + n] = P[r % n_cells]
            if shape == "outside_cut" and at + 4 < N:
                x[at + 4] += 2.0
            at, r = at + n, r + 1
    elif shape == "distinct":
        j = i % 19683                                        # 27^3 interior cells
        x[:] = np.stack([1 + j % 27, 1 + j // 27 % 27, 1 + j // 729], axis=1).astype(np.float64) / (R_SHAPE - 2)
    elif shape == "wave_edges":
        # a run of 63, a run of one (lane 63), then the next wave starts a run at its lane 0
        x[:] = np.where((i % 64 == 63)[:, None], P[1], np.where((i // 64 % 2 == 0)[:, None], P[0], P[2]))
    return x


def _assert_shape(shape, x, MB):
    """The condition on the inputs: the blocks of MB consecutive samples have the shape the case is named after."""
    blocks = _block_shapes(x, R_SHAPE, MB)
    full, last = blocks[:-1], blocks[-1]
    assert len(last["lens"]) == 1 and last["lens"][0] == 1                    # N = k MB + 1
    for b in full:
        if shape == "one_cell":
            assert list(b["lens"]) == [MB] and list(b["chains"]) == [1]
        elif shape == "alternating":
            assert np.all(b["lens"] == 1) and list(b["chains"]) == [MB // 2, MB // 2]
        elif shape == "distinct":
            assert len(b["lens"]) == MB and np.all(b["chains"] == 1) and len(b["chains"]) == MB
        elif shape == "outside_cut":
            assert np.isin(b["lens"], [1, 2, 3, 4]).all() and (b["lens"] == 4).sum() >= 2 * (MB // 9 - 1)
            assert b["lens"].sum() < MB - MB // 9 + 1                          # the outside samples are in no run
        elif shape == "wave_edges":
            assert np.array_equal(b["heads"], np.sort(np.r_[np.arange(0, MB, 64), np.arange(63, MB, 64)]))
    if shape == "run_cycle":
        lens = np.concatenate([b["lens"] for b in full])
        assert set(RUN_CYCLE) <= set(lens.tolist())
        parities = {int(c) % 2 for b in full for c in b["chains"]}
        assert parities == {0, 1}, "chains of an odd and of an even number of runs"
        assert all(len(b["chains"]) == 3 for b in full)


def _overlapped_small(dev, g, x, emb, offs, res, L, n_binned, level_rows, ste, consecutive):
    """The overlapped entry in a workspace of exactly the size it asks for (below 2^16 points it hands the call to the serial
    binned entry; the 512-thread form writes no segment order, so there is no tail to compare)."""
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    lib = _lib.lib()
    N = x.shape[0]
    ge = torch.zeros_like(emb)
    flags = (_lib.CNC_FLAG_STE_BINARY if ste else 0) | (_lib.CNC_FLAG_MERGE_CONSECUTIVE if consecutive else 0)
    nbytes = int(lib.cnc_grid_encode_backward_overlapped_workspace(N, n_binned, level_rows))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.cnc_grid_encode_backward_overlapped(
        be._plan(dev, cur), g.data_ptr(), x.data_ptr(), emb.data_ptr(), offs.data_ptr(), res.data_ptr(), ge.data_ptr(), N, 3, 8,
        L, flags, None, 0, 0, n_binned, level_rows, ws.data_ptr(), nbytes, _lib.stream())
    _lib.check(rc, "grid_encode_backward_overlapped")
    torch.cuda.synchronize()
    return ge.cpu().numpy()


def _run_small(cuda, oracle, x, seed):
    """`_run_case` for the 512-thread form: ten coarse levels and one binned level behind them."""
    import np_twins as tw
    N, L_coarse = x.shape[0], 10
    assert -(-N // 1024) * L_coarse < 4096                   # launch_bwd_merge: `small`
    res = [RES_CYCLE[i % len(RES_CYCLE)] for i in range(L_coarse)] + [RES_BINNED]
    L = len(res)
    offs, resl, emb = make_grid(res, 10, 3, 8, seed=seed)
    g = np.random.default_rng(seed + 1).normal(size=(L, N, 8)).astype(np.float32)
    n_e = tw.grid_entry_counts(x, offs, resl)
    t = lambda a: torch.as_tensor(a, device=cuda)
    xd, gd, ed, od, rd = t(x), t(g), t(emb), t(offs), t(resl)
    coarse_rows = int(offs[L_coarse])
    for ste in (False, True):
        assert not ste or (np.abs(emb) > 1).any()
        _, acc64 = oracle.grid_encode_backward(g, x, emb, offs, resl, ste_binary=ste, want_acc64=True)
        _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, resl, ste_binary=ste, want_acc64=True)
        bound = (n_e[:, None] + 2) * EPS * abs64 + 1e-30
        outs = {}
        for cons in (False, True):
            outs["coarse", cons] = _coarse(cuda, gd, xd, ed, od, rd, L_coarse, ste, cons)
            outs["overlapped", cons] = _overlapped_small(cuda, gd, xd, ed, od, rd, L, 1, 1024, ste, cons)
        for (entry, cons), o in outs.items():
            _check(f"small N={N} ste={ste} {entry} consecutive={cons}", o, acc64, bound,
                   coarse_rows if entry == "coarse" else None)
            if entry == "coarse":
                assert np.all(o[coarse_rows:] == 0)
            if ste:
                assert np.all(o[np.abs(emb) > 1] == 0)
            assert np.all(o[abs64 == 0] == 0)
            assert np.isfinite(o).all()
        for entry in ("coarse", "overlapped"):
            d = np.abs(outs[entry, False].astype(np.float64) - outs[entry, True])
            assert np.all(d <= 2 * bound), f"{entry}: the tilings differ by {np.max(d / bound):.3f} x the bound"


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_shapes_1024_threads(cuda, oracle, shape):
    N, MB = 8 * 1024 + 1, 1024
    x = _points(shape, N, MB)
    _assert_shape(shape, x, MB)
    L_coarse = _levels_for(N)
    assert RES_CYCLE[4] == R_SHAPE and L_coarse > 4
    _run_case(cuda, oracle, x, L_coarse, seed=40 + SHAPES.index(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_chain_shapes_512_threads(cuda, oracle, shape):
    N, MB = 4 * 512 + 1, 512
    x = _points(shape, N, MB)
    _assert_shape(shape, x, MB)
    assert RES_CYCLE[4] == R_SHAPE
    _run_small(cuda, oracle, x, seed=60 + SHAPES.index(shape))
