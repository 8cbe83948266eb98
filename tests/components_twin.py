"""NumPy twin of cnc_amd.components: a plain union-find over the cells of a 3-D mask with the three
neighbourhoods, component sizes, the prune with its largest-kept and tie rules, and the labelling of a face list.  Nothing
here is fast or clever: hook the larger root under the smaller, compress by pointer jumping, repeat until no pair of
neighbours disagrees."""
import numpy as np

CONNECTIVITIES = (6, 14, 26)


def offsets(connectivity):
    """The neighbourhood's offsets (all of them, both signs)."""
    out = []
    for o0 in (-1, 0, 1):
        for o1 in (-1, 0, 1):
            for o2 in (-1, 0, 1):
                o = (o0, o1, o2)
                nz = [v for v in o if v]
                if not nz:
                    continue
                if connectivity == 6 and len(nz) != 1:
                    continue
                if connectivity == 14 and len(set(nz)) != 1:         # the non-zero components all have one sign
                    continue
                out.append(o)
    assert len(out) == connectivity
    return out


def _pairs(mask, connectivity):
    """(u, w): linear indices of every pair of set neighbour cells, one direction of each pair."""
    d = mask.shape
    lin = np.arange(mask.size, dtype=np.int64).reshape(d)
    us, ws = [], []
    for o in offsets(connectivity):
        if o < (0, 0, 0):
            continue
        a = tuple(slice(max(0, -v), d[k] - max(0, v)) for k, v in enumerate(o))
        b = tuple(slice(max(0, v), d[k] - max(0, -v)) for k, v in enumerate(o))
        both = mask[a] & mask[b]
        us.append(lin[a][both])
        ws.append(lin[b][both])
    return np.concatenate(us), np.concatenate(ws)


def _union_find(n, u, w):
    parent = np.arange(n, dtype=np.int64)
    while True:
        pu, pw = parent[u], parent[w]
        apart = pu != pw
        if not apart.any():
            return parent
        np.minimum.at(parent, np.maximum(pu, pw)[apart], np.minimum(pu, pw)[apart])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up


def label_grid(mask, connectivity):
    """int32 labels of a 3-D or 4-D mask: the smallest linear index within its grid of a cell's component, -1 unset."""
    mask = np.asarray(mask) != 0
    if mask.ndim == 4:
        return np.stack([label_grid(m, connectivity) for m in mask])
    u, w = _pairs(mask, connectivity)
    parent = _union_find(mask.size, u, w)
    return np.where(mask.reshape(-1), parent, -1).astype(np.int32).reshape(mask.shape)


def sizes(labels):
    """int32, of labels' shape: the component's cell count at its root, 0 elsewhere (per grid for 4-D labels)."""
    labels = np.asarray(labels)
    if labels.ndim == 4:
        return np.stack([sizes(l) for l in labels])
    flat = labels.reshape(-1)
    return np.bincount(flat[flat >= 0], minlength=flat.size).astype(np.int32).reshape(labels.shape)


def prune_small(mask, min_cells, connectivity):
    """(pruned bool mask, stats): components below min_cells cleared, every grid's largest kept (a tie: the smaller root)."""
    mask = np.asarray(mask) != 0
    grids = mask if mask.ndim == 4 else mask[None]
    out = np.zeros_like(grids)
    stats = dict(components=0, cells=0, removed_components=0, removed_cells=0)
    for g, m in enumerate(grids):
        lab = label_grid(m, connectivity).reshape(-1)
        sz = sizes(lab.reshape(m.shape)).reshape(-1).astype(np.int64)
        keep = sz >= min_cells
        if sz.max() > 0:
            keep[int(np.flatnonzero(sz == sz.max())[0])] = True
        gone = (sz > 0) & ~keep
        stats["components"] += int((sz > 0).sum())
        stats["cells"] += int(sz.sum())
        stats["removed_components"] += int(gone.sum())
        stats["removed_cells"] += int(sz[gone].sum())
        out[g] = ((lab >= 0) & keep[np.maximum(lab, 0)]).reshape(m.shape)
    return out.reshape(mask.shape), stats


def label_graph(faces, n_vertices):
    """int32 [n_vertices]: the smallest vertex index of every vertex's component; its own where no face uses it."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    u, w = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    return _union_find(int(n_vertices), u, w).astype(np.int32)


def graph_counts(faces, n_vertices):
    """Face count of every component, largest first: what Mesh.components() returns."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return np.zeros(0, np.int64)
    _, counts = np.unique(label_graph(f, n_vertices)[f[:, 0]], return_counts=True)
    return np.sort(counts)[::-1].astype(np.int64)


# ---- the inputs the tests share
def pair_grid(shape, a, b):
    m = np.zeros(shape, bool)
    m[a] = m[b] = True
    return m


PINS = (            # (shape, cell, cell, component counts at 6 / 14 / 26)
    ((2, 2, 2), (0, 0, 0), (1, 1, 1), (2, 1, 1)),
    ((2, 2, 2), (0, 0, 1), (1, 1, 0), (2, 2, 1)),
    ((2, 2, 1), (0, 1, 0), (1, 0, 0), (2, 2, 1)),
)


def checkerboard(shape):
    i, j, k = np.indices(shape)
    return (i + j + k) % 2 == 0


def serpentine(shape):
    """Rows mask[i, j, :] for even i, j, joined at alternating ends: ceil(d0 / 2) components at every connectivity, each
    one path."""
    d0, d1, d2 = shape
    m = np.zeros(shape, bool)
    m[0::2, 0::2, :] = True
    for j in range(1, d1, 2):
        if j + 1 < d1:              # a connector only between two rows
            m[0::2, j, d2 - 1 if (j // 2) % 2 == 0 else 0] = True
    return m


def random_grid(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def n_components(labels):
    labels = np.asarray(labels).reshape(-1)
    return int((labels == np.arange(labels.size)).sum())
