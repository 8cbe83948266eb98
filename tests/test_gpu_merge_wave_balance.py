"""The work units of k_grid_encode_bwd_merge's phase B (grid_encode_merge.hip: the samples of a block laid out by cell,
cells cut at CNC_MERGE_UNIT_CAP samples, units handed to the waves from a block-wide counter) on point sets made to give
the layout, the cut and the hand-out every shape they have code for, against the oracle's float64 sums with the bound of
tests/test_gpu_merge_tiles.py: every table entry within (n_e + 2) * eps * sum|terms| of the float64 sum, the two tilings
within twice that bound of each other; the coarse call and the overlapped entry, STE on and off.  A sample that lands in
two units or in none, or a unit no wave takes, is far outside that bound.

Two forms of the kernel, as in tests/test_gpu_merge_chain_shapes.py: 1,024 threads per block (N = 8 * 1,024 + 1) and 512
threads (N = 4 * 512 + 1 with ten coarse levels).

The shapes are built for the level of R = 31 (consecutive samples in either form) by tests/test_merge_units.py, which
also holds the numpy twin's checks; each is asserted on every block (`assert_block_shape`, numpy, with the cap the
library is built with) before anything runs on the GPU.  Every other level of the call sees some other mix — on the
levels of R = 4 ... 8 a few cells hold the whole block — and is checked all the same.

  one_cell         one cell per block: a lone run of MB samples, cut into MB / cap units
  chain_lengths    one chain per block, of exactly cap, cap + 1 and 2 cap - 1 samples in turn (those that fit a block),
                   made of runs of 1 ... 9 with an outside sample between them
  three_cells      three chains of no more than cap samples: fewer units than waves, most waves take nothing
  seventeen_cells  17 cells of 60 (30) samples in runs dealt to the cells in turn: one unit more than waves at least
  outside_blocks   every other block has all its samples outside the unit cube: no cell, no unit, the counter is never asked
  distinct         every sample in a cell of its own: MB units of one sample
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_merge_chain_shapes import _run_small  # noqa: E402
from test_gpu_merge_tiles import EPS, RES_CYCLE, _check, _levels_for, _run_case  # noqa: E402,F401
from test_merge_units import R_SHAPE, SHAPES, assert_block_shape, kernel_cap, shape_points  # noqa: E402
from tools.merge_wave_load import cell_keys  # noqa: E402

pytestmark = pytest.mark.gpu


def _points(shape, n_blocks, MB):
    cap = kernel_cap()
    x = shape_points(shape, n_blocks, MB, cap)
    keys = cell_keys(x, R_SHAPE)
    assert len(keys) == n_blocks * MB + 1 and keys[-1] >= 0
    for b in range(n_blocks):
        k = keys[b * MB:(b + 1) * MB]
        if shape == "outside_blocks" and b % 2:
            assert (k < 0).all()
        else:
            assert_block_shape(shape, k, MB, cap, b)
    return x


@pytest.mark.parametrize("shape", SHAPES)
def test_units_1024_threads(cuda, oracle, shape):
    x = _points(shape, 8, 1024)
    L_coarse = _levels_for(x.shape[0])
    assert RES_CYCLE[4] == R_SHAPE and L_coarse > 4
    _run_case(cuda, oracle, x, L_coarse, seed=140 + SHAPES.index(shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_units_512_threads(cuda, oracle, shape):
    x = _points(shape, 4, 512)
    assert RES_CYCLE[4] == R_SHAPE
    _run_small(cuda, oracle, x, seed=160 + SHAPES.index(shape))
