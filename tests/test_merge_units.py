"""The rule that lays the samples of a block of k_grid_encode_bwd_merge (grid_encode_merge.hip) out by cell and cuts each
cell into work units of at most CNC_MERGE_UNIT_CAP samples, on its numpy twin (tools/merge_wave_load.split_units).  No GPU.

The twin does what a run's thread does, LDS atomic by LDS atomic (hash probe for the cell, add on the cell's sample count),
then what a cell's representative does (one add on the block's packed place | unit counter), and lets a random schedule
decide which run and which cell goes next: the orders the hardware can produce, not only sample order.  On random run
sequences and on the shapes of tests/test_gpu_merge_wave_balance.py, for several caps and both block sizes:

  * the places are a permutation: every sample with a cell has exactly one place below the number of such samples, no
    two share one, samples without a cell have none;
  * the units are disjoint and cover exactly those places: every sample lies in exactly one unit;
  * a unit holds one cell's samples only, at least one and at most cap (cells are cut by arithmetic on places: there
    is no overhang); a cell of n samples makes ceil(n / cap) units whatever the order of arrival;
  * the samples of a run keep their order on consecutive places;
  * units never outnumber the block's threads (the records share the threads' 16-byte slots).

Phase B walks a unit with a counted loop over its places, lo to hi: there are no chain records left that could point at
themselves, and hi <= the block size bounds every walk.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.merge_wave_load import cell_keys, split_units  # noqa: E402

R_SHAPE = 31                                 # the level the shapes are built for (test_gpu_merge_chain_shapes.py)
SHAPES = ["one_cell", "chain_lengths", "three_cells", "seventeen_cells", "outside_blocks", "distinct"]


def kernel_cap():
    """CNC_MERGE_UNIT_CAP as the library is built by default."""
    src = open(os.path.join(ROOT, "cnc_amd", "csrc", "grid_encode_merge.hip")).read()
    return int(re.search(r"#define CNC_MERGE_UNIT_CAP (\d+)", src).group(1))


def _centre(c):
    """The centre of cell c (three integers) of the R_SHAPE level: fractions of one half, far from any rounding."""
    return (np.asarray(c, np.float64) / (R_SHAPE - 2)).astype(np.float32)


CELLS = [_centre((1 + j % 27, 1 + j // 27 % 27, 1 + j // 729)) for j in range(17)]
OUTSIDE = np.float32(2.0)


def chain_lengths(cap, MB):
    """The chain lengths of the `chain_lengths` shape, one chain per block in turn: cap, cap + 1 and 2 cap - 1, those that
    fit a block together with the outside samples that cut the chain's runs apart (a quarter as many at most); where not
    even cap fits (the 512-thread form under a cap of 512) the longest chain that does."""
    fit = [n for n in (cap, cap + 1, 2 * cap - 1) if n + n // 4 + 9 <= MB]
    return fit or [(MB - 9) * 4 // 5]


def block_points(shape, MB, cap, block=0):
    """The points of one block of MB samples ([MB, 3] float32), shaped on the level of R_SHAPE."""
    x = np.empty((MB, 3), np.float32)
    x[:] = CELLS[0] + OUTSIDE                               # outside the unit cube: no cell
    if shape == "one_cell":
        x[:] = CELLS[0]
    elif shape == "chain_lengths":
        # one chain of runs of 1 ... 9 samples, an outside sample between two runs
        lens = chain_lengths(cap, MB)
        left, at, r = lens[block % len(lens)], 0, 0
        while left:
            n = min(1 + r % 9, left)
            x[at:at + n] = CELLS[2]
            left, at, r = left - n, at + n + 1, r + 1
        assert at - 1 <= MB
    elif shape == "three_cells":
        n = min(cap, MB // 3) // 5 * 5                       # three chains of runs of 5, none above the cap
        for r in range(3 * n // 5):
            x[5 * r:5 * r + 5] = CELLS[r % 3]
    elif shape == "seventeen_cells":
        run = MB // 256                                      # 17 cells x 15 runs of 4 (2): about 60 (30) samples each
        for r in range(15 * 17):
            x[run * r:run * r + run] = CELLS[r % 17]
    elif shape == "outside_blocks":
        if block % 2 == 0:                                   # every other block has no sample inside the cube
            lens = [1, 2, 3, 4, 5, 7, 8, 9]
            at, r = 0, 0
            while at < MB:
                x[at:at + lens[r % 8]] = CELLS[r % 3]
                at, r = at + lens[r % 8], r + 1
    elif shape == "distinct":
        j = (block * MB + np.arange(MB)) % 19683             # 27^3 interior cells
        x[:] = np.stack([1 + j % 27, 1 + j // 27 % 27, 1 + j // 729], axis=1).astype(np.float64) / (R_SHAPE - 2)
    return x


def shape_points(shape, n_blocks, MB, cap):
    """n_blocks blocks of the shape and one more sample: N = n_blocks MB + 1."""
    return np.concatenate([block_points(shape, MB, cap, b) for b in range(n_blocks)] + [CELLS[1][None, :]])


def check_units(keys, cap, units, place):
    """The properties of the module docstring, for one block."""
    keys = np.asarray(keys)
    MB = len(keys)
    inside = keys >= 0
    n_in = int(inside.sum())
    assert len(units) <= MB
    assert np.all(place[~inside] == -1)
    assert np.array_equal(np.sort(place[inside]), np.arange(n_in)), "the places are a permutation"
    key_at = np.empty(n_in, np.int64)
    key_at[place[inside]] = keys[inside]
    covered = np.zeros(n_in, np.int64)
    for u in units:
        assert 0 <= u["lo"] < u["hi"] <= n_in and u["hi"] - u["lo"] <= cap
        assert np.all(key_at[u["lo"]:u["hi"]] == u["key"])
        covered[u["lo"]:u["hi"]] += 1
    assert np.all(covered == 1), "every sample in exactly one unit"
    same_run = inside[1:] & (keys[1:] == keys[:-1])
    assert np.all(place[1:][same_run] == place[:-1][same_run] + 1), "a run keeps its order on consecutive places"
    per_cell = {}
    for k in keys[inside].tolist():
        per_cell[k] = per_cell.get(k, 0) + 1
    assert len(units) == sum(-(-n // cap) for n in per_cell.values())
    return per_cell


def assert_block_shape(shape, keys, MB, cap, block=0):
    """The condition on the inputs (numpy, sample order): the block has the shape the case is named after.  Returns the
    number of units of the block."""
    units, place = split_units(keys, cap)
    per_cell = check_units(keys, cap, units, place)
    keys = np.asarray(keys)
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    lens = np.diff(np.r_[heads, len(keys)])[keys[heads] >= 0]
    if shape == "one_cell":
        assert list(per_cell.values()) == [MB] and len(lens) == 1 and len(units) == -(-MB // cap)
    elif shape == "chain_lengths":
        want = chain_lengths(cap, MB)
        assert list(per_cell.values()) == [want[block % len(want)]]
        assert lens.min() >= 1 and lens.max() <= 9 and len(lens) > 1
        assert len(units) == -(-want[block % len(want)] // cap)
    elif shape == "three_cells":
        assert len(per_cell) == 3 and len(units) == 3 and len(units) < MB // 64 and max(per_cell.values()) <= cap
    elif shape == "seventeen_cells":
        assert len(per_cell) == 17 and len(units) >= MB // 64 + 1 and set(per_cell.values()) == {15 * (MB // 256)}
    elif shape == "distinct":
        assert len(units) == MB and len(per_cell) == MB
    return len(units)


@pytest.mark.parametrize("MB", [1024, 512])
@pytest.mark.parametrize("cap", sorted({16, 32, 64, 128, kernel_cap()}))
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(shape, cap, MB):
    n_blocks = 3 if shape == "chain_lengths" else 2 if shape in ("outside_blocks", "distinct") else 1
    x = shape_points(shape, n_blocks, MB, cap)
    keys = cell_keys(x, R_SHAPE)
    rng = np.random.default_rng(SHAPES.index(shape) + cap + MB)
    for b in range(n_blocks + 1):
        k = keys[b * MB:(b + 1) * MB]
        if b < n_blocks:
            if shape == "outside_blocks" and b % 2:
                assert np.all(k < 0) and split_units(k, cap)[0] == []
            else:
                assert_block_shape(shape, k, MB, cap, b)
        for trial in range(3):
            check_units(k, cap, *split_units(k, cap, rng))


@pytest.mark.parametrize("MB", [1024, 512])
@pytest.mark.parametrize("cap", sorted({16, 32, 128, kernel_cap()}))
def test_random_runs(cap, MB):
    rng = np.random.default_rng(cap * 7 + MB)
    for trial in range(12):
        n_cells = int(rng.choice([1, 2, 5, 40, 300]))
        longest = int(rng.choice([1, 4, 9, 40, 3 * cap]))
        keys = np.empty(MB, np.int64)
        at = 0
        while at < MB:
            n = int(rng.integers(1, longest + 1))
            c = int(rng.integers(-1, n_cells))                # -1: outside the cube
            keys[at:at + n] = -1 if c < 0 else (3 + c % 29) | (5 + c // 29) << 16 | 7 << 32
            at += n
        for schedule in (None, rng, rng):
            check_units(keys, cap, *split_units(keys, cap, schedule))
