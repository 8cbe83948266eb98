"""The sorted bin pass (k_bwd_bin_sorted, grid_encode_binned.hip) computes 1 / (sum of the valid corner weights) once per sample
in its count phase, keeps it in LDS (one float per sample slot of the 4,096-sample block) and the walk's lane reads it for
the sample of its item.  tests/test_gpu_bin_pass_exact.py stops at 1,000 points: one block, and only the first of a thread's
four sample slots.  Here the exact (one-contribution) point sets of that file — cells with even coordinates, lines along x,
taken whole or not at all by its collision filter — are made for 8,200 points on two hashed levels of R = 300, one of 2^19
rows (masked) and one of 500,000 rows (the modulo): N = 1025 (slot k = 1 of a thread), 4096 (every slot of one block), 4097
and 8200 (a second and a third block), F = 2, 4, 8, through cnc_grid_encode_backward_binned with n_binned = L (the sorted
pass).  A one-term sum has no order, so the table gradient must equal oracle.grid_encode_backward in every bit: a normaliser
read at another sample's slot shows in every row of the sample.  Points outside [0, 1] (two, early in the set) write no
slot, and points on all six faces are among the first 63.

The condition on the inputs is asserted without a GPU (test_big_exact_point_set_survives_the_collision_filter): the filter
keeps at least 90 % of the constructed set, and the oracle's float32 gradient equals its float64 one.  The table sizes are
what makes that possible: a line of 150 cells takes four aligned 512-row blocks per level, 55 lines 220 of the 1,024 such
blocks of 2^19 rows.

One bounded case, 3 * 4096 + 1 uniform points, with the bound of tests/test_gpu_encoder.py (`_check_bwd`)."""
import functools

import numpy as np
import pytest

import test_gpu_bin_pass_exact as E
from test_gpu_encoder import _check_bwd, _points

gpu = pytest.mark.gpu

BIG = ((300, 1 << 19), (300, 500000))
N_MAX = 8200


@functools.lru_cache(maxsize=None)
def _big_points():
    """test_gpu_bin_pass_exact._exact_points on the two levels above: its table of sets holds the entry only during the call."""
    E.EXACT_SETS["big"] = (BIG, N_MAX, 15, None)      # (levels, points wanted, seed, whole lines)
    try:
        return E._exact_points.__wrapped__("big")
    finally:
        del E.EXACT_SETS["big"]


def test_big_exact_point_set_survives_the_collision_filter(oracle):
    """CPU only."""
    x, keep = _big_points()
    assert keep.sum() >= 0.9 * len(x) and keep.sum() >= N_MAX, (int(keep.sum()), len(x))
    x = x[keep][:N_MAX]
    head = x[:63]
    for d in range(3):
        assert (head[:, d] == 0).any() and (head[:, d] == 1).any(), d
    assert ((head < 0) | (head > 1)).any(axis=1).sum() == 2
    offs, res, emb = E._grid(BIG, 2, 1)
    g = np.random.default_rng(2).normal(size=(len(BIG), len(x), 2)).astype(np.float32)
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=False, want_acc64=True)
    assert np.array_equal(want32.astype(np.float64), acc64)
    assert (acc64 != 0).any(axis=1).sum() > 3 * N_MAX * len(BIG)


@gpu
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("N", [1025, 4096, 4097, N_MAX])
def test_exact_beyond_the_first_sample_slot(cuda, oracle, N, F):
    ste = F != 4
    offs, res, emb = E._grid(BIG, F, seed=21)
    x, keep = _big_points()
    x = np.ascontiguousarray(x[keep][:N])
    assert len(x) == N
    g = np.random.default_rng(22 + N).normal(size=(len(BIG), N, F)).astype(np.float32)
    want32 = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=ste)
    got = E._call(cuda, g, x, emb, offs, res, len(BIG), 1 << 19, ste)
    E._assert_bit_equal(got, want32)
    assert (want32 != 0).any()
    if ste:
        assert np.all(got[np.abs(emb) > 1] == 0)


@gpu
def test_bounded_three_blocks_and_one_sample(cuda, oracle):
    N, F = 3 * 4096 + 1, 8
    offs, res, emb = E._grid(BIG, F, seed=31)
    x = _points(N, 3, seed=32)
    g = np.random.default_rng(33).normal(size=(len(BIG), N, F)).astype(np.float32)
    want32, acc64, abs64 = E._shadow(oracle, g, x, emb, offs, res, True)
    got = E._call(cuda, g, x, emb, offs, res, len(BIG), 1 << 19, True)
    _check_bwd(got, want32, acc64, abs64, n_terms_max=N * 8)
