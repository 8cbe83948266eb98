"""NumPy twin of the mesh export: an independent restatement of the extraction rule, for the CPU tests and as
the reference of the GPU tests.  It shares nothing with cnc_amd/mesh.py: the triangles of a (tetrahedron, mask) pair are
decided here by the geometric rule directly (`direct_triangles`, floating-point midpoints and a cross product), never
through `tet_table()`.

`extract(..., dtype=np.float32)` keeps the kernels' operation order — every +, -, x, / a separate float32 operation, the
square root correctly rounded — so that vertices and normals can be compared bit for bit; `dtype=np.float64` is the same
rule in double.  Helpers: the directed-edge manifold check, the Euler characteristic, the signed volume in float64.
"""
import itertools

import numpy as np

DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]], np.int64)      # (dx, dy, dz)
PERMS = list(itertools.permutations(range(3)))         # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


def tet_local(tet):
    """int [4, 3]: v0 = 0, v1 = e_p1, v2 = e_p1 + e_p2, v3 = (1, 1, 1)."""
    v = np.zeros((4, 3), np.int64)
    for k, axis in enumerate(PERMS[tet]):
        v[k + 1] = v[k]
        v[k + 1, axis] += 1
    return v


def direct_triangles(tet, mask):
    """The triangles of one (tetrahedron, mask) pair by the rule itself: lists of three local edges (i, j), i < j."""
    V = tet_local(tet).astype(np.float64)
    ins = [k for k in range(4) if (mask >> k) & 1]
    outs = [k for k in range(4) if not (mask >> k) & 1]
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        tris = [[(ins[0], o) for o in outs]]
    elif len(outs) == 1:
        tris = [[(outs[0], i) for i in ins]]
    else:
        q = [(ins[0], outs[0]), (ins[0], outs[1]), (ins[1], outs[1]), (ins[1], outs[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    toward_low = V[outs].mean(axis=0) - V[ins].mean(axis=0)
    res = []
    for tri in tris:
        a, b, c = (0.5 * (V[i] + V[j]) for i, j in tri)
        if np.dot(np.cross(b - a, c - a), toward_low) < 0:
            tri = [tri[0], tri[2], tri[1]]
        res.append([(min(e), max(e)) for e in tri])
    return res


def cells_of(lo, hi, resolution):
    ext = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return tuple(int(max(1, round(resolution * e / ext.max()))) for e in ext)


def spacing(lo, hi, n, dtype=np.float32):
    lo, hi = np.asarray(lo, dtype), np.asarray(hi, dtype)
    return lo, ((hi - lo) / np.asarray(n, dtype)).astype(dtype)


def axes(lo, hi, n, dtype=np.float32):
    """Per axis the lattice's coordinates: lo + float(i) * h, a multiply and then an add."""
    lo, h = spacing(lo, hi, n, dtype)
    return [(lo[a] + (np.arange(n[a] + 1).astype(dtype) * h[a]).astype(dtype)).astype(dtype) for a in range(3)]


def positions(lo, hi, n, dtype=np.float32):
    """[points, 3] in lattice order, x fastest."""
    X, Y, Z = axes(lo, hi, n, dtype)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    return np.stack([xx, yy, zz], -1).reshape(-1, 3)


def capped(D):
    D = np.array(D, np.float32, copy=True)
    D[0], D[-1], D[:, 0], D[:, -1], D[:, :, 0], D[:, :, -1] = 0, 0, 0, 0, 0, 0
    return D


def active_points(occ, n):
    """bool [pz, py, px]: some set cell of `occ` [Gx, Gy, Gz] overlaps [p - h, p + h]; per axis in integers, cell j
    overlaps point i iff j n <= (i + 1) G and (j + 1) n >= (i - 1) G."""
    occ = np.asarray(occ, bool)
    M = []
    for a in range(3):
        G, i, j = occ.shape[a], np.arange(n[a] + 1)[:, None], np.arange(occ.shape[a])[None, :]
        M.append(((j * n[a] <= (i + 1) * G) & ((j + 1) * n[a] >= (i - 1) * G)).astype(np.int64))
    return np.einsum("xa,yb,zc,abc->zyx", M[0], M[1], M[2], occ.astype(np.int64)) > 0


def _gradients(D, h, dtype):
    """Central differences over 2 h, one-sided over h on the boundary; [3][pz, py, px]."""
    D = D.astype(dtype)
    out = []
    for a in range(3):
        Dm = np.moveaxis(D, 2 - a, 0)                 # axis a first (x is the last array axis)
        g = np.empty_like(Dm)
        g[0] = (Dm[1] - Dm[0]) / h[a]
        g[-1] = (Dm[-1] - Dm[-2]) / h[a]
        if Dm.shape[0] > 2:
            g[1:-1] = (Dm[2:] - Dm[:-2]) / (dtype(2.0) * h[a])
        out.append(np.moveaxis(g, 0, 2 - a))
    return out


def extract(D, lo, hi, threshold, cap=True, normals=True, dtype=np.float32, want_pairs=False):
    """-> (vertices [V, 3] dtype, faces [F, 3] int32, normals [V, 3] dtype or None).  D: [nz + 1, ny + 1, nx + 1], taken as
    float32.  want_pairs: also the set of (tetrahedron, mask) pairs that gave a triangle."""
    D = capped(D) if cap else np.array(D, np.float32, copy=True)
    pz, py, px = D.shape
    n = (px - 1, py - 1, pz - 1)
    thr = np.float32(threshold)
    inside = D >= thr                                  # NaN compares false
    lo_, h = spacing(lo, hi, n, dtype)
    X, Y, Z = axes(lo, hi, n, dtype)

    # ---- vertices: by owner, then direction
    cross = np.zeros((pz, py, px, 7), bool)
    for k, (dx, dy, dz) in enumerate(DIRS):
        a = inside[:pz - dz, :py - dy, :px - dx]
        b = inside[dz:, dy:, dx:]
        cross[:pz - dz, :py - dy, :px - dx, k] = a != b
    flat = cross.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - 1
    at = np.nonzero(flat)[0]
    owner, k = at // 7, at % 7
    x, y, z = owner % px, (owner // px) % py, owner // (px * py)
    xb, yb, zb = x + DIRS[k, 0], y + DIRS[k, 1], z + DIRS[k, 2]
    Dd = D.astype(dtype)
    with np.errstate(all="ignore"):
        da, db = Dd[z, y, x], Dd[zb, yb, xb]
        t = ((dtype(thr) - da) / (db - da)).astype(dtype)
        pa = np.stack([X[x], Y[y], Z[z]], -1)
        pb = np.stack([X[xb], Y[yb], Z[zb]], -1)
        vertices = (pa + (t[:, None] * (pb - pa)).astype(dtype)).astype(dtype)
        nrm = None
        if normals:
            g = _gradients(D, h, dtype)
            ga = np.stack([g[a][z, y, x] for a in range(3)], -1)
            gb = np.stack([g[a][zb, yb, xb] for a in range(3)], -1)
            nrm = (-(ga + (t[:, None] * (gb - ga)).astype(dtype))).astype(dtype)
            length = np.sqrt(((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]).astype(dtype)).astype(dtype)
            divide = length != 0
            nrm[divide] = (nrm[divide] / length[divide, None]).astype(dtype)

    # ---- faces: by cell, tetrahedron, triangle
    nx, ny, nz = n
    cz, cy, cx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cz, cy, cx = cz.reshape(-1), cy.reshape(-1), cx.reshape(-1)
    keys, rows, pairs = [], [], set()
    for tet in range(6):
        V = tet_local(tet)
        mask = np.zeros(nx * ny * nz, np.int64)
        for kk in range(4):
            mask |= inside[cz + V[kk, 2], cy + V[kk, 1], cx + V[kk, 0]].astype(np.int64) << kk
        for m in range(1, 15):
            cells = np.nonzero(mask == m)[0]
            if cells.size == 0:
                continue
            pairs.add((tet, m))
            for ti, tri in enumerate(direct_triangles(tet, m)):
                ids = []
                for i, j in tri:
                    d = int(np.nonzero((DIRS == (V[j] - V[i])).all(axis=1))[0][0])
                    own = ((cz[cells] + V[i, 2]) * py + cy[cells] + V[i, 1]) * px + cx[cells] + V[i, 0]
                    assert flat[own * 7 + d].all()
                    ids.append(vid[own * 7 + d])
                keys.append((cells * 6 + tet) * 2 + ti)
                rows.append(np.stack(ids, -1))
    if rows:
        order = np.argsort(np.concatenate(keys), kind="stable")
        faces = np.concatenate(rows)[order].astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    res = (vertices.reshape(-1, 3), faces, nrm.reshape(-1, 3) if normals else None)
    return res + (pairs,) if want_pairs else res


# ---------------------------------------------------------------------------------------------- mesh properties
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_directed_manifold(faces, n_vertices):
    """Every directed edge occurs once, and its reverse once: closed, edge-manifold, consistently oriented."""
    e = directed_edges(faces)
    if e.shape[0] == 0:
        return True
    code, back = e[:, 0] * n_vertices + e[:, 1], e[:, 1] * n_vertices + e[:, 0]
    if np.unique(code).size != code.size or (e[:, 0] == e[:, 1]).any():
        return False
    return bool(np.array_equal(np.sort(code), np.sort(back)))


def euler_characteristic(faces, n_vertices):
    e = np.sort(directed_edges(faces), axis=1)
    n_edges = np.unique(e[:, 0] * n_vertices + e[:, 1]).size
    return int(np.unique(np.asarray(faces)).size) - n_edges + int(np.asarray(faces).shape[0])


def signed_volume(vertices, faces):
    """In float64; positive for a closed surface whose faces wind counter-clockwise seen from outside."""
    v = np.asarray(vertices, np.float64)
    a, b, c = (v[np.asarray(faces)[:, i]] for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def canonical_faces(faces):
    """Each triangle rotated to its smallest index first, the rows sorted."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    r = np.argmin(f, axis=1)
    f = np.stack([f[np.arange(len(f)), (r + i) % 3] for i in range(3)], -1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


# ---------------------------------------------------------------------------------------------- PLY
def parse_ply(path):
    """A reader of its own for the binary little-endian PLY the exporter writes -> {property: array}, faces [F, 3]."""
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements = []
    for line in lines[2:]:
        w = line.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        else:
            assert w[0] == "property"
            elements[-1][2].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    _, nv, props = elements[0]
    vdt = np.dtype([(p[1], kinds[p[0]]) for p in props])
    verts = np.frombuffer(body, vdt, nv)
    _, nf, fprops = elements[1]
    assert fprops == [["list", "uchar", "int", "vertex_indices"]]
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    faces = np.frombuffer(body, fdt, nf, offset=nv * vdt.itemsize)
    assert len(body) == nv * vdt.itemsize + nf * fdt.itemsize and (faces["n"] == 3).all()
    return {name: verts[name] for name in vdt.names}, faces["i"]


# ---------------------------------------------------------------------------------------------- lattices of the tests
def noise_lattice(n, seed):
    """U[0, 1) on an (nx, ny, nz)-cell lattice, float32 [nz + 1, ny + 1, nx + 1]."""
    return np.random.default_rng(seed).uniform(size=(n[2] + 1, n[1] + 1, n[0] + 1)).astype(np.float32)


def tie_lattice(n, seed):
    """Multiples of 0.25 in [0, 1]: many values equal to the threshold 0.5."""
    return (np.random.default_rng(seed).integers(0, 5, size=(n[2] + 1, n[1] + 1, n[0] + 1)) * 0.25).astype(np.float32)


def sphere_lattice(cells, radius=0.6):
    X, Y, Z = axes([-1] * 3, [1] * 3, (cells,) * 3, np.float64)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    return (1.0 + radius - np.sqrt(xx * xx + yy * yy + zz * zz)).astype(np.float32)


def torus_lattice(cells, R=0.55, r=0.2):
    X, Y, Z = axes([-1] * 3, [1] * 3, (cells,) * 3, np.float64)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    dist = np.sqrt((np.sqrt(xx * xx + yy * yy) - R) ** 2 + zz * zz)
    return (1.2 - dist).astype(np.float32)


def smooth_lattice(n):
    """A smooth field with several sheets through an odd-sized lattice; box [-1, 1] x [-0.5, 0.5] x [-0.6, 0.6]."""
    X, Y, Z = axes([-1, -0.5, -0.6], [1, 0.5, 0.6], n, np.float64)
    zz, yy, xx = np.meshgrid(Z, Y, X, indexing="ij")
    return (1.0 + 0.8 * np.sin(5.0 * xx) * np.cos(7.0 * yy) + 0.5 * np.sin(4.0 * zz + xx)).astype(np.float32)


def special_lattice(n, seed):
    """Noise with NaN, +inf and -inf entries."""
    D = noise_lattice(n, seed)
    rng = np.random.default_rng(seed + 1)
    kind = rng.integers(0, 12, size=D.shape)
    D[kind == 0] = np.nan
    D[kind == 1] = np.inf
    D[kind == 2] = -np.inf
    return D
