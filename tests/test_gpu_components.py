"""The connected-component kernels (csrc/components.hip) against the NumPy twin (tests/components_twin.py,
itself pinned against scipy in tests/test_components_twin.py).  The labels are unique by definition — the smallest linear
index of the component — so every comparison here is an equality, at all three connectivities, with the outputs in
sentinel-guarded allocations.

No kernel of components.hip caps its launch grid or strides: every launch has one lane per cell, tile cell, face or
vertex, so there is no later trip of a loop to take; the loops there are find / hook loops, whose long trips the
serpentines (one path of 8 255 cells across hundreds of tile seams) and the percolating random grids exercise."""
import numpy as np
import pytest
import torch

import components_twin as T
from guarded import Guarded, moved_with_fill, same_bits, under_fills

pytestmark = pytest.mark.gpu


def _seam(pin, axes_crossed):
    """Pin `pin`'s pair in a 16x16x16 grid, placed so that the two cells lie in different 8x8x8 tiles and meet across a tile
    face (1 axis crosses 7|8), edge (2) or corner (3)."""
    _, a, b, _ = T.PINS[pin]
    o = [y - x for x, y in zip(a, b)]
    base, crossed = [], 0
    for v in o:
        if v != 0 and crossed < axes_crossed:
            base.append(7 if v > 0 else 8)
            crossed += 1
        else:
            base.append(3)
    assert crossed == axes_crossed
    return T.pair_grid((16, 16, 16), tuple(base), tuple(x + v for x, v in zip(base, o)))


CASES = {
    "unset_5x4x3": lambda: np.zeros((5, 4, 3), bool),
    "set_5x4x3": lambda: np.ones((5, 4, 3), bool),
    "set_9x17x10": lambda: np.ones((9, 17, 10), bool),
    "one_cell": lambda: np.ones((1, 1, 1), bool),
    "one_unset_cell": lambda: np.zeros((1, 1, 1), bool),
    "row_1x1x37": lambda: np.ones((1, 1, 37), bool),
    "row_1x19x1": lambda: np.ones((1, 19, 1), bool),
    "set_2x2x2": lambda: np.ones((2, 2, 2), bool),
    "pin0": lambda: T.pair_grid(*T.PINS[0][:3]),
    "pin1": lambda: T.pair_grid(*T.PINS[1][:3]),
    "pin2": lambda: T.pair_grid(*T.PINS[2][:3]),
    "pin0_face": lambda: _seam(0, 1), "pin0_edge": lambda: _seam(0, 2), "pin0_corner": lambda: _seam(0, 3),
    "pin1_face": lambda: _seam(1, 1), "pin1_edge": lambda: _seam(1, 2), "pin1_corner": lambda: _seam(1, 3),
    "pin2_face": lambda: _seam(2, 1), "pin2_edge": lambda: _seam(2, 2),          # two non-zero axes: no corner to meet across
    "checkerboard_13x9x21": lambda: T.checkerboard((13, 9, 21)),
    "serpentine_13x9x21": lambda: T.serpentine((13, 9, 21)),
    "serpentine_128": lambda: T.serpentine((128, 128, 128)),
    "random_10_33x20x17": lambda: T.random_grid((33, 20, 17), 0.10, 7),
    "random_18_33x20x17": lambda: T.random_grid((33, 20, 17), 0.18, 7),
    "random_31_33x20x17": lambda: T.random_grid((33, 20, 17), 0.31, 7),
    "random_10_128": lambda: T.random_grid((128, 128, 128), 0.10, 9),
    "random_18_128": lambda: T.random_grid((128, 128, 128), 0.18, 9),
    "random_31_128": lambda: T.random_grid((128, 128, 128), 0.31, 9),
}
_masks, _twins = {}, {}


def mask_of(name):
    if name not in _masks:
        _masks[name] = CASES[name]()
        _masks[name].setflags(write=False)
    return _masks[name]


def twin_of(name, connectivity):
    key = (name, connectivity)
    if key not in _twins:
        _twins[key] = T.label_grid(mask_of(name), connectivity)
        _twins[key].setflags(write=False)
    return _twins[key]


def _label(mask4, connectivity, dev, fill=0xA5):
    from cnc_amd.backends import components as C
    m = Guarded(mask4.astype(np.uint8), dev, fill=fill)
    out = Guarded.empty(mask4.shape, np.int32, dev, fill=fill)
    C.label_grid(m.tensor(), connectivity, out.tensor())
    torch.cuda.synchronize()
    assert out.intact() and m.intact()
    return out


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_equal_the_twins(cuda, name, connectivity):
    want = twin_of(name, connectivity)
    out = _label(mask_of(name)[None], connectivity, cuda)
    assert same_bits(out.get()[0], want)


def test_the_cases_have_the_stated_properties(cuda):
    """Component counts of the pins (apart and across tile seams), the checkerboard, the serpentines — from the device's
    labels, which the test above holds equal to the twin's."""
    count = lambda name, c: T.n_components(_label(mask_of(name)[None], c, cuda).get()[0])
    for pin in range(3):
        want = T.PINS[pin][3]
        for name in [f"pin{pin}", f"pin{pin}_face", f"pin{pin}_edge"] + ([f"pin{pin}_corner"] if pin < 2 else []):
            assert tuple(count(name, c) for c in T.CONNECTIVITIES) == want, name
    cb = mask_of("checkerboard_13x9x21")
    assert count("checkerboard_13x9x21", 6) == int(cb.sum()) and count("checkerboard_13x9x21", 26) == 1
    for c in T.CONNECTIVITIES:
        assert count("serpentine_13x9x21", c) == 7 and count("serpentine_128", c) == 64
    assert int(mask_of("serpentine_13x9x21").sum()) == 7 * 109 and int(mask_of("serpentine_128").sum()) == 64 * 8255


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
def test_three_grids_in_one_call_equal_three_calls(cuda, connectivity):
    masks = np.stack([T.random_grid((11, 19, 10), p, 21 + i) for i, p in enumerate((0.1, 0.2, 0.3))])
    together = _label(masks, connectivity, cuda).get()
    for g in range(3):
        alone = _label(masks[g][None], connectivity, cuda).get()[0]
        assert same_bits(together[g], alone) and same_bits(alone, T.label_grid(masks[g], connectivity))


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["unset_5x4x3", "set_9x17x10", "serpentine_13x9x21", "random_18_33x20x17", "random_18_128",
                                  "random_31_128"])
def test_sizes_equal_the_twins(cuda, name, connectivity):
    from cnc_amd.backends import components as C
    want_labels = twin_of(name, connectivity)
    labels = Guarded(want_labels[None], cuda)
    sizes = Guarded.empty(labels.shape, np.int32, cuda)
    C.sizes(labels.tensor(), sizes.tensor())
    torch.cuda.synchronize()
    assert sizes.intact() and labels.intact()
    got = sizes.get()[0]
    assert same_bits(got, T.sizes(want_labels)) and int(got.sum(dtype=np.int64)) == int(mask_of(name).sum())
    # a second call on the used buffer: the call zeroes it itself
    C.sizes(labels.tensor(), sizes.tensor())
    assert same_bits(sizes.get()[0], got)


def test_three_grids_of_sizes(cuda):
    from cnc_amd.backends import components as C
    masks = np.stack([T.random_grid((11, 19, 10), p, 21 + i) for i, p in enumerate((0.1, 0.2, 0.3))])
    want = T.label_grid(masks, 14)
    labels = Guarded(want, cuda)
    sizes = Guarded.empty(want.shape, np.int32, cuda)
    C.sizes(labels.tensor(), sizes.tensor())
    torch.cuda.synchronize()
    assert sizes.intact() and same_bits(sizes.get(), T.sizes(want))


def test_public_functions(cuda):
    from cnc_amd import components as P
    m = mask_of("random_18_33x20x17")
    for c in T.CONNECTIVITIES:
        want = twin_of("random_18_33x20x17", c)
        for t in (torch.from_numpy(m.copy()).to(cuda), torch.from_numpy(m.astype(np.uint8) * 3).to(cuda)):    # bool; uint8, non-zero = set
            lab = P.label_grid(t, c)
            assert lab.dtype == torch.int32 and same_bits(lab, want)
        roots, sizes = P.component_sizes(lab)
        sz = T.sizes(want).reshape(-1)
        assert roots.dtype == sizes.dtype == torch.int64
        assert np.array_equal(roots.cpu().numpy(), np.flatnonzero(sz)) and np.array_equal(sizes.cpu().numpy(), sz[sz > 0])
    assert same_bits(P.label_grid(torch.from_numpy(m.copy()).to(cuda)), twin_of("random_18_33x20x17", 26))        # the default
    four = torch.from_numpy(np.stack([m, ~m])).to(cuda)
    assert same_bits(P.label_grid(four, 6), T.label_grid(np.stack([m, ~m]), 6))
    sliced = torch.from_numpy(np.stack([m, m], -1).copy()).to(cuda)[..., 0]            # not contiguous
    assert same_bits(P.label_grid(sliced, 14), twin_of("random_18_33x20x17", 14))


@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["random_18_128", "random_18_33x20x17"])
def test_prune_small_equals_the_twins(cuda, name, connectivity):
    from cnc_amd import components as P
    m = mask_of(name)
    t = torch.from_numpy(m.copy()).to(cuda)
    for k in (0, 1, 2, 5, 10 ** 9):
        want, want_stats = T.prune_small(m, k, connectivity)
        got, stats = P.prune_small(t, k, connectivity)
        assert got.dtype == torch.bool and same_bits(got, want) and stats == want_stats, k
        if k <= 1:
            assert stats["removed_cells"] == 0 and same_bits(got, m)
    assert torch.equal(t.cpu(), torch.from_numpy(m.copy()))                         # the input is not modified


def test_prune_small_ties_go_to_the_smaller_root(cuda):
    from cnc_amd import components as P
    m = np.zeros((2, 3, 12, 9), bool)
    m[0, 2, 10:12, 8] = True          # grid 0: two components of two cells (roots 314 and 16) and a singleton
    m[0, 0, 1, 7:9] = True
    m[0, 1, 5, 5] = True
    m[1, 1, 3:6, 4] = True            # grid 1: 3 cells (root 139), 3 cells (root 279), 2 cells
    m[1, 2, 7:10, 0] = True
    m[1, 0, 0, 0:2] = True
    for c in T.CONNECTIVITIES:
        for k in (0, 2, 3, 4, 100):
            want, want_stats = T.prune_small(m, k, c)
            got, stats = P.prune_small(torch.from_numpy(m.copy()).to(cuda), k, c)
            assert same_bits(got, want) and stats == want_stats
        got, stats = P.prune_small(torch.from_numpy(m.copy()).to(cuda), 100, c)
        keep = np.zeros_like(m)
        keep[0, 0, 1, 7:9] = True
        keep[1, 1, 3:6, 4] = True
        assert same_bits(got, keep) and stats == dict(components=6, cells=13, removed_components=4, removed_cells=8)
    # an empty grid stays empty, next to one that is not
    e = np.zeros((2, 4, 4, 4), bool)
    e[1, 1, 1, 1] = True
    got, stats = P.prune_small(torch.from_numpy(e).to(cuda), 7, 26)
    assert same_bits(got, e) and stats == dict(components=1, cells=1, removed_components=0, removed_cells=0)


# ---- graph
TWO_TETRAHEDRA = np.asarray([[5, 6, 7], [5, 7, 8], [5, 8, 6], [6, 8, 7], [0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)


def _blob_lattice():
    """float32 [25, 22, 27]: five balls of different sizes, apart from each other and from the box."""
    z, y, x = np.meshgrid(np.arange(25), np.arange(22), np.arange(27), indexing="ij")
    D = np.zeros((25, 22, 27), np.float32)
    for cz, cy, cx, r in ((7, 7, 8, 5.2), (18, 15, 20, 4.1), (19, 5, 6, 2.6), (5, 16, 21, 3.3), (12, 11, 14, 1.4)):
        D = np.maximum(D, (2.0 - np.sqrt((z - cz) ** 2 + (y - cy) ** 2 + (x - cx) ** 2) / r).astype(np.float32))
    return np.maximum(D, 0).astype(np.float32)


def test_label_graph_equals_the_twins(cuda):
    from cnc_amd.backends import components as C
    from cnc_amd import components as P
    faces = Guarded(TWO_TETRAHEDRA, cuda)
    labels = Guarded.empty((9,), np.int32, cuda)
    C.label_graph(faces.tensor(), 9, labels.tensor())
    torch.cuda.synchronize()
    assert labels.intact() and faces.intact()
    assert same_bits(labels.get(), T.label_graph(TWO_TETRAHEDRA, 9)) and labels.get().tolist() == [0, 0, 0, 0, 4, 5, 5, 5, 5]
    # a soup with long chains: a strip of 3 000 triangles, its faces shuffled, and a second strip
    rng = np.random.default_rng(5)
    strip = np.stack([np.arange(3000), np.arange(3000) + 1, np.arange(3000) + 2], 1)
    soup = np.concatenate([strip, strip[:700] + 3500]).astype(np.int32)
    perm = rng.permutation(4300)                   # vertex names shuffled too: roots are not the strips' ends
    soup = perm[soup][rng.permutation(len(soup))].astype(np.int32)
    got = P.label_graph(torch.from_numpy(soup).to(cuda), 4300)
    assert same_bits(got, T.label_graph(soup, 4300))
    assert same_bits(P.label_graph(torch.zeros((0, 3), dtype=torch.int32, device=cuda), 5), np.arange(5, dtype=np.int32))


def test_mesh_components_on_device_equal_the_host_path(cuda):
    from cnc_amd.mesh import extract_mesh
    mesh = extract_mesh(torch.from_numpy(_blob_lattice()).to(cuda), [0.0, 0.0, 0.0, 2.7, 2.2, 2.5], threshold=1.0)
    host = mesh.components()
    dev = mesh.components(on_device=True)
    assert host.size == 5 and host.dtype == dev.dtype and np.array_equal(host, dev)
    assert np.array_equal(dev, T.graph_counts(mesh.faces.cpu().numpy(), mesh.vertices.shape[0]))
    empty = extract_mesh(torch.zeros((4, 4, 4), device=cuda), [0.0, 0.0, 0.0, 1.0, 1.0, 1.0], threshold=1.0)
    assert empty.components(on_device=True).size == 0


# ---- footprint
@pytest.mark.parametrize("connectivity", T.CONNECTIVITIES)
def test_footprint(cuda, connectivity):
    """The same bits with 0x00, 0xA5 and 0xFF around every buffer; the inputs unchanged, nothing written outside.  The
    shapes are no multiples of the tile, so the tiles' overhang lies in the surroundings."""
    from cnc_amd.backends import components as C
    masks = np.stack([T.random_grid((11, 19, 10), p, 21 + i) for i, p in enumerate((0.15, 0.3))]).astype(np.uint8)
    masks[masks != 0] = 0xA5                                   # non-zero = set, whatever the byte
    want = T.label_grid(masks, connectivity)
    rng = np.random.default_rng(4)
    faces = np.concatenate([TWO_TETRAHEDRA, rng.integers(9, 40, (30, 3)).astype(np.int32)])

    def build(fill):
        e = lambda shape: Guarded.empty(shape, np.int32, cuda, fill=fill)
        return {"mask": Guarded(masks, cuda, fill=fill), "labels": e(masks.shape), "sizes": e(masks.shape),
                "faces": Guarded(faces, cuda, fill=fill), "vertex_labels": e((41,))}

    def run(b):
        t = {k: g.tensor() for k, g in b.items()}
        C.label_grid(t["mask"], connectivity, t["labels"])
        C.sizes(t["labels"], t["sizes"])
        C.label_graph(t["faces"], 41, t["vertex_labels"])
    res = under_fills(build, run)
    assert moved_with_fill(res) == []
    out = res[0xA5]
    assert same_bits(out["labels"], want) and same_bits(out["sizes"], T.sizes(want))
    assert same_bits(out["vertex_labels"], T.label_graph(faces, 41))


# ---- bad arguments
def test_bad_arguments_are_refused(cuda):
    from cnc_amd import _lib, components as P
    from cnc_amd.backends import components as C
    m = torch.ones((1, 4, 4, 4), dtype=torch.uint8, device=cuda)
    lab = torch.full((1, 4, 4, 4), -5, dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match="connectivity"):
        C.label_grid(m, 8, lab)
    with pytest.raises(RuntimeError, match="connectivity"):
        P.label_grid(m, 8)
    with pytest.raises(RuntimeError):
        P.label_grid(torch.ones((4, 0, 4), dtype=torch.bool, device=cuda))
    with pytest.raises(RuntimeError):
        C.label_grid(torch.ones((1, 4, 0, 4), dtype=torch.uint8, device=cuda), 6, torch.empty((1, 4, 0, 4), dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.label_grid(torch.ones((4, 4, 4), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        C.label_grid(m.cpu(), 6, lab)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        C.sizes(lab.cpu(), lab)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        P.label_graph(torch.zeros((2, 3), dtype=torch.int32), 4)
    with pytest.raises(RuntimeError):
        P.label_grid(torch.ones((4, 4, 4), dtype=torch.float32, device=cuda))
    with pytest.raises(RuntimeError):
        C.label_grid(m, 6, torch.empty((1, 4, 4, 5), dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError):
        C.label_graph(torch.zeros((2, 3), dtype=torch.int64, device=cuda), 4, torch.empty(4, dtype=torch.int32, device=cuda))
    # the C ABI itself: an error code, nothing launched
    L = _lib.lib()
    s = _lib.stream(cuda)
    assert L.cnc_components_label_grid(m.data_ptr(), 1, 4, 4, 4, 8, lab.data_ptr(), s) == -1
    assert L.cnc_components_label_grid(m.data_ptr(), 1, 4, 0, 4, 6, lab.data_ptr(), s) == -1
    assert L.cnc_components_label_grid(m.data_ptr(), 0, 4, 4, 4, 6, lab.data_ptr(), s) == -1
    assert L.cnc_components_label_grid(m.data_ptr(), 1 << 11, 1 << 10, 1 << 10, 1, 6, lab.data_ptr(), s) == -1       # 2^31 cells
    assert L.cnc_components_label_grid(None, 1, 4, 4, 4, 6, lab.data_ptr(), s) == -1
    assert L.cnc_components_sizes(lab.data_ptr(), 1, 4, 4, -1, lab.data_ptr(), s) == -1
    assert L.cnc_components_label_graph(None, 3, 4, lab.data_ptr(), s) == -1
    assert L.cnc_components_label_graph(m.data_ptr(), -1, 4, lab.data_ptr(), s) == -1
    torch.cuda.synchronize()
    assert bool((lab == -5).all())
