"""The owner pass's 1-D grid (grid_encode_binned.hip: owner_slab / owner_grid_size), restated in Python: every workgroup id
of a few grid shapes is decoded and every (level, bin, part) slab must come out exactly once — a dropped or doubled slab is
a wrong gradient that a GPU test at one shape may miss — and the two levels of a pair must sit on complementary halves of
the id labels (id % 8), which is what the paired placement is for.  Runs without a GPU."""
import itertools

import pytest


def owner_bins_padded(bins):
    return (bins + 7) & ~7


def owner_grid_size(n_binned, bins, parts, n_pairs):
    return n_pairs * 2 * parts * owner_bins_padded(bins) + (n_binned - 2 * n_pairs) * parts * bins


def owner_slab(w, bins, parts, n_pairs):
    """id -> (level, bin, part); bin >= bins: padding, the workgroup returns at once."""
    padded = owner_bins_padded(bins)
    pair_ids = 2 * parts * padded
    if w < n_pairs * pair_ids:
        pair, v = divmod(w, pair_ids)
        idx = (v >> 3) * 4 + (v & 3)
        return 2 * pair + ((v >> 2) & 1), idx % padded, idx // padded
    v = w - n_pairs * pair_ids
    lv, u = divmod(v, parts * bins)
    return 2 * n_pairs + lv, u % bins, u // bins


SHAPES = [(n_binned, bins, parts) for n_binned in (1, 2, 3, 4, 5, 6) for bins, parts in ((2048, 5), (4, 5), (5, 3), (13, 1), (1, 2))]


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("n_binned,bins,parts", SHAPES)
def test_every_slab_is_owned_exactly_once(n_binned, bins, parts, paired):
    n_pairs = n_binned // 2 if paired else 0
    grid = owner_grid_size(n_binned, bins, parts, n_pairs)
    seen = {}
    surplus = 0
    for w in range(grid):
        level, b, part = owner_slab(w, bins, parts, n_pairs)
        assert 0 <= level < n_binned and 0 <= part < parts
        if b >= bins:
            assert level < 2 * n_pairs and b < owner_bins_padded(bins)      # padding exists in paired ranges only
            surplus += 1
            continue
        assert (level, b, part) not in seen, (w, seen[(level, b, part)])
        seen[(level, b, part)] = w
    assert set(seen) == set(itertools.product(range(n_binned), range(bins), range(parts)))
    assert surplus == 2 * n_pairs * parts * (owner_bins_padded(bins) - bins)


@pytest.mark.parametrize("n_binned,bins,parts", SHAPES)
def test_paired_levels_sit_on_disjoint_label_halves(n_binned, bins, parts):
    n_pairs = n_binned // 2
    labels = {}
    first_wave_last, later_wave_first = {}, {}
    for w in range(owner_grid_size(n_binned, bins, parts, n_pairs)):
        level, b, part = owner_slab(w, bins, parts, n_pairs)
        if b >= bins:
            continue
        labels.setdefault(level, set()).add(w % 8)
        if part == 0:
            first_wave_last[level] = w
        else:
            later_wave_first.setdefault(level, w)
    for pair in range(n_pairs):
        assert labels[2 * pair] <= {0, 1, 2, 3} and labels[2 * pair + 1] <= {4, 5, 6, 7}
        if bins >= 4:
            assert labels[2 * pair] == {0, 1, 2, 3} and labels[2 * pair + 1] == {4, 5, 6, 7}
    if n_binned % 2 and bins * parts >= 8:
        assert labels[n_binned - 1] == set(range(8))            # the level without a partner keeps all eight labels
    # the extra waves of overloaded bins still come after every bin's first wave of their level
    for level, w in later_wave_first.items():
        assert w > first_wave_last[level]


def test_unset_flag_is_the_level_major_grid():
    """n_pairs = 0: id = (level * parts + part) * bins + bin, the order of the two-dimensional launch it replaces."""
    bins, parts, n_binned = 2048, 5, 6
    for w in range(0, owner_grid_size(n_binned, bins, parts, 0), 97):
        level, b, part = owner_slab(w, bins, parts, 0)
        assert w == (level * parts + part) * bins + b
