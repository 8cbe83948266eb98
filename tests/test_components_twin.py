"""The NumPy twin of the connected-component kernels (tests/components_twin.py) against sources it shares no
code with: scipy.ndimage.label with the matching 3x3x3 structure, relabelled to "smallest linear index", for the grids;
the host union-find of `Mesh.components()` for the face lists.  The GPU tests compare the kernels with this twin bit for
bit, so the twin has to be right first.  CPU only."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import components_twin as T


def _structure(connectivity):
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for o in T.offsets(connectivity):
        s[o[0] + 1, o[1] + 1, o[2] + 1] = True
    return s


def _scipy_labels(mask, connectivity):
    lab, n = ndimage.label(mask, structure=_structure(connectivity))
    smallest = np.full(n + 1, mask.size, np.int64)
    np.minimum.at(smallest, lab.reshape(-1), np.arange(mask.size))
    return np.where(mask, smallest[lab], -1).astype(np.int32), n


def test_the_three_neighbourhoods():
    assert [len(T.offsets(c)) for c in T.CONNECTIVITIES] == [6, 14, 26]
    from cnc_amd.mesh import DIRECTIONS
    kuhn = set(DIRECTIONS) | {tuple(-v for v in d) for d in DIRECTIONS}
    assert set(T.offsets(14)) == kuhn                                  # symmetric under axis permutations, so no axis order matters
    assert {tuple(reversed(o)) for o in kuhn} == kuhn
    assert (1, 1, 1) in kuhn and (1, 1, -1) not in kuhn


@pytest.mark.parametrize("shape,a,b,counts", T.PINS)
def test_pins_tell_the_neighbourhoods_apart(shape, a, b, counts):
    m = T.pair_grid(shape, a, b)
    for c, want in zip(T.CONNECTIVITIES, counts):
        lab = T.label_grid(m, c)
        assert T.n_components(lab) == want == _scipy_labels(m, c)[1]
        assert np.array_equal(lab, _scipy_labels(m, c)[0])


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
def test_grid_labels_equal_scipys(connectivity):
    cases = [np.zeros((5, 4, 3), bool), np.ones((5, 4, 3), bool), np.ones((1, 1, 1), bool), np.ones((1, 1, 37), bool),
             np.ones((1, 19, 1), bool), np.ones((2, 2, 2), bool), T.checkerboard((13, 9, 21)), T.serpentine((13, 9, 21))]
    cases += [T.random_grid((33, 20, 17), p, seed=7) for p in (0.10, 0.18, 0.31)]
    cases.append(T.random_grid((40, 40, 40), 0.18, seed=8))
    for m in cases:
        lab = T.label_grid(m, connectivity)
        want, n = _scipy_labels(m, connectivity)
        assert lab.dtype == np.int32 and np.array_equal(lab, want)
        assert T.n_components(lab) == n
        sz = T.sizes(lab)
        assert int(sz.sum()) == int(m.sum()) and np.array_equal(np.flatnonzero(sz), np.flatnonzero(lab.reshape(-1) == np.arange(m.size)))
        if n:
            assert np.array_equal(np.sort(sz[sz > 0]), np.sort(ndimage.sum_labels(m, ndimage.label(m, _structure(connectivity))[0],
                                                                                  np.arange(1, n + 1)).astype(np.int32)))


def test_the_inputs_have_the_stated_properties():
    cb = T.checkerboard((13, 9, 21))
    assert T.n_components(T.label_grid(cb, 6)) == int(cb.sum()) and T.n_components(T.label_grid(cb, 26)) == 1
    s = T.serpentine((13, 9, 21))
    for c in T.CONNECTIVITIES:
        lab = T.label_grid(s, c)
        assert T.n_components(lab) == 7 and set(T.sizes(lab)[T.sizes(lab) > 0].tolist()) == {109}
    big = T.serpentine((128, 128, 128))
    lab, n = _scipy_labels(big, 6)
    assert n == 64 and int(big.sum()) == 64 * 8255
    assert _scipy_labels(big, 26)[1] == 64


def test_four_dimensional_masks_are_labelled_grid_by_grid():
    m = np.stack([T.random_grid((9, 10, 11), p, seed=3) for p in (0.1, 0.2, 0.3)])
    lab = T.label_grid(m, 14)
    for g in range(3):
        assert np.array_equal(lab[g], _scipy_labels(m[g], 14)[0])


def test_prune_keeps_the_largest_and_breaks_ties_by_root():
    m = np.zeros((1, 1, 12), bool)
    m[0, 0, [0, 1, 3, 4, 6, 9, 10]] = True                      # sizes 2, 2, 1, 2 at roots 0, 3, 6, 9
    for k in (-3, 0, 1):
        out, st = T.prune_small(m, k, 6)
        assert np.array_equal(out, m) and st == dict(components=4, cells=7, removed_components=0, removed_cells=0)
    out, st = T.prune_small(m, 3, 6)
    assert np.flatnonzero(out).tolist() == [0, 1] and st == dict(components=4, cells=7, removed_components=3, removed_cells=5)
    out, st = T.prune_small(m, 2, 6)
    assert np.flatnonzero(out).tolist() == [0, 1, 3, 4, 9, 10] and st["removed_cells"] == 1
    out, st = T.prune_small(np.zeros((2, 2, 2), bool), 5, 26)
    assert not out.any() and st == dict(components=0, cells=0, removed_components=0, removed_cells=0)


def test_prune_equals_a_prune_built_on_scipy():
    m = T.random_grid((33, 20, 17), 0.18, seed=7)
    for c in T.CONNECTIVITIES:
        lab, n = ndimage.label(m, structure=_structure(c))
        count = np.bincount(lab.reshape(-1))
        count[0] = 0
        for k in (0, 1, 2, 5, 10 ** 9):
            keep = count >= k
            smallest = np.full(n + 1, m.size, np.int64)
            np.minimum.at(smallest, lab.reshape(-1), np.arange(m.size))
            top = [i for i in range(1, n + 1) if count[i] == count.max()]
            keep[min(top, key=lambda i: smallest[i])] = True
            keep[0] = False
            out, st = T.prune_small(m, k, c)
            assert np.array_equal(out, keep[lab])
            assert st == dict(components=n, cells=int(m.sum()), removed_components=int((~keep[1:]).sum()),
                              removed_cells=int(count[~keep].sum()))


def _soup(seed, n_vertices=400, n_faces=260):
    """Faces over clusters of vertices, some vertices unused."""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 23, n_vertices)
    faces = []
    while len(faces) < n_faces:
        g = rng.integers(0, 23)
        pool = np.flatnonzero(group == g)
        if pool.size >= 3:
            faces.append(rng.choice(pool, 3, replace=False))
    return np.asarray(faces, np.int32), n_vertices


def test_graph_counts_equal_the_host_mesh_components():
    from cnc_amd.mesh import Mesh
    for seed in (1, 2, 3):
        f, V = _soup(seed)
        mesh = Mesh(torch.zeros((V, 3)), torch.from_numpy(f))
        assert np.array_equal(T.graph_counts(f, V), mesh.components())
        lab = T.label_graph(f, V)
        assert lab.dtype == np.int32 and (lab <= np.arange(V)).all() and (lab[lab] == lab).all()
        used = np.zeros(V, bool)
        used[f.reshape(-1)] = True
        assert np.array_equal(lab[~used], np.arange(V)[~used])
    two = np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2], [5, 6, 7], [5, 7, 8], [5, 8, 6], [6, 8, 7]], np.int32)
    assert T.label_graph(two, 9).tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5]
    assert T.graph_counts(np.zeros((0, 3), np.int32), 4).size == 0
