"""The bin pass of the binned backward (k_bwd_bin_sorted / k_bwd_bin, grid_encode_binned.hip) builds its items from two cut-down
corner set-ups (encoder_common.hpp: corner_rows3 in the count phase, CornerPair3 in the walk) that must return, bit for bit,
what Corners<3, false>::setup returns.  Checked here through the C ABI (cnc_grid_encode_backward_binned, n_binned = L):

  * EXACT cases: point sets in which, by the oracle's own row arithmetic, no table row receives more than one contribution.
    A one-term sum has no order, so the table gradient must equal oracle.grid_encode_backward in every bit of every row:
    a weight with w0 / w1 swapped, a sum of the valid weights taken in another order, a wrong row or validity flag all
    show (the mutation runs are in profiles/r14_bin_pass_setup.md).
  * BOUNDED cases: uniform points over one block plus one sample, three blocks and many blocks against the oracle's float64
    sums with the bound of test_gpu_binned_backward.py (`_check_bwd`: (n + 2) eps sum|terms| per entry).

How the exact point sets are made.  Uniform points cannot be used: a cell's eight corners are table rows, and the filter
"drop a point that touches a row already taken" keeps far fewer than 90 % of N = 1,000 uniform points on 2^16 rows (8,000 rows
wanted of 65,536: about a third of the late points collide) and next to none on the dense R = 16 level.  So the points are
CONSTRUCTED: they sit in cells with even coordinates (no two such cells share a vertex), on lines along x.  On a hashed level
the row of a corner is (x ^ h(y, z)) mod rows with x < 512, so one line fills four aligned 512-row blocks without a
collision inside a block, and a line is taken whole or not at all, by the same collision filter, until enough points exist.
The filter then runs over the finished set point by point (`_collision_filter`, the rows from oracle.grid_index) and must
keep at least 90 % of it (it keeps all of it for the seeds below: test_exact_point_sets_survive_the_collision_filter, no GPU
needed), and the oracle itself confirms the property: its float32 gradient equals its float64 one exactly.
  The dense R = 16 level has 15^3 cells of which at most 8^3 = 512 share no vertex, so N = 1,000 cannot exist there whatever
the choice; its exact cases stop at 300 points (and those of the dense R = 12 level with 1,728 rows, 6^3 such cells, at 130).  No cell of R = 16 has eight border corners (that needs R = 2), and a point
without a valid corner emits no item, so the `wn == 0` replacement cannot show in a table gradient; points outside [0, 1]
and on all six faces are in every set of 63 points and more."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from test_gpu_encoder import _check_bwd, _points

gpu = pytest.mark.gpu

DENSE = ((16, 4096),)                          # R^3 = rows: dense
DENSE12 = ((12, 1728),)                        # dense, rows no power of two: the sum of the strides, then the modulo test
HASHED = ((300, 1 << 16), (300, 65000))        # hashed: power-of-two rows (mask), other rows (modulo)
SMALL = ((300, 1024),)                         # hashed, 4 slabs: the level the bin-count variants use
ALL3 = DENSE + HASHED
EXACT_SETS = {"dense": (DENSE, 300, 11, None), "hashed": (HASHED, 1000, 12, None), "small": (SMALL, 65, 13, 16),
              "dense12": (DENSE12, 130, 14, None)}
EXACT_N = {"dense": [1, 63, 64, 65, 300], "hashed": [1, 63, 64, 65, 1000], "dense12": [1, 63, 64, 65, 130]}


def _grid(levels, F, seed):
    offs = np.concatenate([[0], np.cumsum([rows for _, rows in levels])]).astype(np.int32)
    res = np.asarray([R for R, _ in levels], np.int32)
    emb = np.random.default_rng(seed).uniform(-1.5, 1.5, size=(int(offs[-1]), F)).astype(np.float32)
    return offs, res, emb


def _corner_rows(orc, x, R, rows):
    """rows [N, 8] and validity [N, 8] of the corners of every point on one level: the cell as the encoder floors it (float32),
    the row from the oracle's own grid_index."""
    x = np.asarray(x, np.float32)
    p = (x * np.float32(R - 2)).astype(np.float32) + np.float32(0.5)
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    cell = np.where(inside[:, None], np.floor(p), 0).astype(np.int64)
    bits = np.asarray([[i & 1, (i >> 1) & 1, (i >> 2) & 1] for i in range(8)], np.int64)
    q = np.minimum(cell[:, None, :] + bits[None], R - 1)
    valid = inside[:, None] & np.all((q != 0) & (q != R - 1), axis=2)
    return orc.grid_index(q.astype(np.uint32), rows, R), valid


def _collision_filter(orc, x, levels, used=None):
    """keep[i]: point i touches no row (through a valid corner, on any level) that an earlier kept point or another of its
    own corners touches."""
    per_level = [_corner_rows(orc, x, R, rows) for R, rows in levels]
    used = [set() for _ in levels] if used is None else used
    keep = np.zeros(len(x), bool)
    for i in range(len(x)):
        mine = [r[i][v[i]].tolist() for r, v in per_level]
        if all(len(set(m)) == len(m) and not (set(m) & u) for m, u in zip(mine, used)):
            keep[i] = True
            for m, u in zip(mine, used):
                u.update(m)
    return keep


@functools.lru_cache(maxsize=None)
def _exact_points(name):
    import oracle as orc
    orc.build()
    levels, n_max, seed, line_len = EXACT_SETS[name]
    R = levels[0][0]
    assert all(r == R for r, _ in levels)
    S = R - 2
    rng = np.random.default_rng(seed)
    even = np.arange(0, S + 1, 2)

    def coord(c):       # a position in cell c, clear of the cell faces and inside [0, 1]
        f = rng.uniform(0.5 if c == 0 else 0.1, 0.5 if c == S else 0.9)
        return np.float32((c + f - 0.5) / S)

    faces = [(np.float32(0), None), (np.float32(1), None), (None, np.float32(0)), (None, np.float32(1))]
    used, lines = [set() for _ in levels], []
    for _ in range(4000):
        t = len(lines)                  # the first four lines lie in the faces y = 0, y = 1, z = 0, z = 1
        y, z = faces[t] if t < 4 else (None, None)
        y = coord(rng.choice(even)) if y is None else y
        z = coord(rng.choice(even)) if z is None else z
        cells = even
        if line_len is not None:        # a short line: the first at x = 0, the second up to x = 1, the others anywhere
            a = 0 if t == 0 else len(even) - line_len if t == 1 else int(rng.integers(0, len(even) - line_len + 1))
            cells = even[a:a + line_len]
        xs = np.asarray([coord(c) for c in cells], np.float32)
        if cells[0] == 0 and t % 2 == 0:
            xs[0] = 0.0                 # on the face x = 0: p = 0.5, cell 0
        if cells[-1] == S and t % 2 == 1:
            xs[-1] = 1.0                # on the face x = 1: p = R - 1.5, cell R - 2
        line = np.stack([xs, np.full_like(xs, y), np.full_like(xs, z)], axis=1)
        trial = [set(u) for u in used]
        if _collision_filter(orc, line, levels, trial).all():
            used = trial
            order = rng.permutation(len(line))
            face_first = sorted(order, key=lambda k: not (line[k, 0] in (0.0, 1.0)))
            lines.append(line[face_first])
        if sum(len(l) for l in lines) >= n_max:
            break
    pts = []
    for k in range(max(len(l) for l in lines)):     # round robin over the lines: a short prefix already mixes them
        pts += [l[k] for l in lines if k < len(l)]
    pts.insert(5, np.asarray([-1e-3, 0.3, 0.3], np.float32))            # outside the box: contribute nothing
    pts.insert(40, np.asarray([0.4, 0.4, 1 + 1e-3], np.float32))
    x = np.asarray(pts, np.float32)
    keep = _collision_filter(orc, x, levels)
    return x, keep


def _exact_x(name, N):
    x, keep = _exact_points(name)
    x = x[keep]
    assert len(x) >= N
    return np.ascontiguousarray(x[:N])


def _shadow(oracle, g, x, emb, offs, res, ste):
    want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=ste, want_acc64=True)
    _, abs64 = oracle.grid_encode_backward(np.abs(g), x, emb, offs, res, ste_binary=ste, want_acc64=True)
    return want32, acc64, abs64


def test_exact_point_sets_survive_the_collision_filter(oracle):
    """CPU only.  Every constructed set keeps at least 90 % of its points through the filter, has the faces and the outside
    points early, and in the oracle's backward no row sums more than one term: float32 and float64 gradients are equal."""
    for name, (levels, n_max, _, _) in EXACT_SETS.items():
        x, keep = _exact_points(name)
        assert keep.sum() >= 0.9 * len(x) and keep.sum() >= n_max, (name, int(keep.sum()), len(x))
        x = x[keep][:n_max]
        head = x[:63]
        for d in range(3):
            assert (head[:, d] == 0).any() and (head[:, d] == 1).any(), (name, d)
        assert ((head < 0) | (head > 1)).any(axis=1).sum() == 2
        offs, res, emb = _grid(levels, 2, 1)
        g = np.random.default_rng(2).normal(size=(len(levels), len(x), 2)).astype(np.float32)
        want32, acc64 = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=False, want_acc64=True)
        assert np.array_equal(want32.astype(np.float64), acc64), name
        assert (acc64 != 0).any(axis=1).sum() > 3 * n_max * len(levels)      # and the rows are many: 8 a point but for the faces


def _call(dev, g, x, emb, offs, res, n_binned, level_rows, ste, flags=0, ws_bytes=None, point_major=False, overlapped=False):
    from cnc_amd import _lib
    lib = _lib.lib()
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    L, N, F = g.shape
    ld = col = 0
    gd = t(g)
    if point_major:      # the gradient read in place from a wider [N, ld] matrix
        ld, col = L * F + 8, 4
        wide = torch.randn(N, ld, device=dev)
        wide[:, col:col + L * F] = gd.permute(1, 0, 2).reshape(N, L * F)
        gd = wide.contiguous()
    size = lib.cnc_grid_encode_backward_overlapped_workspace if overlapped else lib.cnc_grid_encode_backward_binned_workspace
    if ws_bytes is None:
        ws_bytes = int(size(N, n_binned, level_rows))
    ws = torch.full((max(ws_bytes, 16),), 0xAB, dtype=torch.uint8, device=dev)      # the library must clear what it reads
    ge = torch.zeros(emb.shape, dtype=torch.float32, device=dev)
    xd, ed, od, rd = t(x), t(emb), t(offs), t(res)
    flags |= _lib.CNC_FLAG_STE_BINARY if ste else 0
    p = lambda a: C.c_void_p(a.data_ptr())
    tail = (N, 3, F, L, flags, None, ld, col, n_binned, level_rows, p(ws), ws_bytes)
    if overlapped:
        plan = C.c_void_p()
        assert lib.cnc_backward_plan_create(C.byref(plan)) == 0 and plan.value
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            rc = lib.cnc_grid_encode_backward_overlapped(plan, p(gd), p(xd), p(ed), p(od), p(rd), p(ge), *tail,
                                                         C.c_void_p(side.cuda_stream))
        side.synchronize()
        assert lib.cnc_backward_plan_destroy(plan) == 0
    else:
        rc = lib.cnc_grid_encode_backward_binned(p(gd), p(xd), p(ed), p(od), p(rd), p(ge), *tail, _lib.stream())
    _lib.check(rc, "binned")
    torch.cuda.synchronize()
    return ge.cpu().numpy()


def _assert_bit_equal(got, want32):
    same = got.view(np.uint32) == want32.view(np.uint32)
    assert same.all(), f"{(~same).sum()} of {same.size} entries differ; first at {np.argwhere(~same)[0].tolist()}"


def _exact_case(cuda, oracle, name, N, F, ste, point_major, level_rows, flags=0):
    levels = EXACT_SETS[name][0]
    offs, res, emb = _grid(levels, F, seed=21)
    x = _exact_x(name, N)
    g = np.random.default_rng(22 + N).normal(size=(len(levels), N, F)).astype(np.float32)
    want32 = oracle.grid_encode_backward(g, x, emb, offs, res, ste_binary=ste)
    got = _call(cuda, g, x, emb, offs, res, len(levels), level_rows, ste, flags=flags, point_major=point_major)
    _assert_bit_equal(got, want32)
    if N >= 63:
        assert (want32 != 0).any()
    if ste:
        assert np.all(got[np.abs(emb) > 1] == 0)


@gpu
@pytest.mark.parametrize("point_major", [False, True])
@pytest.mark.parametrize("ste", [False, True])
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("N", EXACT_N["dense"])
def test_exact_dense_level(cuda, oracle, N, F, ste, point_major):
    _exact_case(cuda, oracle, "dense", N, F, ste, point_major, 4096)


@gpu
@pytest.mark.parametrize("lane_stores", [False, True])
@pytest.mark.parametrize("F,ste,point_major", [(8, True, False), (2, False, True), (4, True, True)])
@pytest.mark.parametrize("N", EXACT_N["dense12"])
def test_exact_dense_level_other_rows(cuda, oracle, N, F, ste, point_major, lane_stores):
    """A dense level whose row count is no power of two (R = 12, 1,728 rows, 7 slabs): the general form's sum of strides
    and its modulo test, in both bin kernels.  6^3 = 216 cells share no vertex there; 130 points."""
    from cnc_amd import _lib
    _exact_case(cuda, oracle, "dense12", N, F, ste, point_major, 1728,
                flags=_lib.CNC_FLAG_BIN_LANE_STORES if lane_stores else 0)


@gpu
@pytest.mark.parametrize("point_major", [False, True])
@pytest.mark.parametrize("ste", [False, True])
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("N", EXACT_N["hashed"])
def test_exact_hashed_levels(cuda, oracle, N, F, ste, point_major):
    """Two levels of R = 300 in one call: 2^16 rows (masked) and 65,000 rows (the modulo)."""
    _exact_case(cuda, oracle, "hashed", N, F, ste, point_major, 1 << 16)


@gpu
@pytest.mark.parametrize("N", [65, 1000])
def test_exact_hashed_levels_lane_stores(cuda, oracle, N):
    """CNC_FLAG_BIN_LANE_STORES: k_bwd_bin, whose count phase takes the rows-only set-up too."""
    from cnc_amd import _lib
    _exact_case(cuda, oracle, "hashed", N, 8, True, False, 1 << 16, flags=_lib.CNC_FLAG_BIN_LANE_STORES)


@gpu
@pytest.mark.parametrize("lane_stores", [False, True])
@pytest.mark.parametrize("level_rows", [700, 1024, 1280, 3300])
def test_exact_bin_counts_off_the_power_of_two(cuda, oracle, level_rows, lane_stores):
    """3 bins (fewer than the level's 4 slabs: every corner goes to atomics), 4, 5 and 13 bins per level."""
    from cnc_amd import _lib
    _exact_case(cuda, oracle, "small", 65, 8, True, False, level_rows,
                flags=_lib.CNC_FLAG_BIN_LANE_STORES if lane_stores else 0)


@functools.lru_cache(maxsize=None)
def _bounded_reference(N, F, ste, coarse):
    import oracle as orc
    orc.build()
    levels = (((6, 216), (12, 1728)) if coarse else ()) + ALL3
    offs, res, emb = _grid(levels, F, seed=31)
    x = _points(N, 3, seed=32)
    g = np.random.default_rng(33).normal(size=(len(levels), N, F)).astype(np.float32)
    return (offs, res, emb, x, g) + _shadow(orc, g, x, emb, offs, res, ste)


@gpu
@pytest.mark.parametrize("F,ste", [(8, True), (4, True), (2, False)])
@pytest.mark.parametrize("N", [4097, 9001, 70001])
def test_bounded_uniform_points(cuda, oracle, N, F, ste):
    """One block plus one sample, three blocks, many blocks; the dense and both hashed levels in one call."""
    offs, res, emb, x, g, want32, acc64, abs64 = _bounded_reference(N, F, ste, False)
    got = _call(cuda, g, x, emb, offs, res, 3, 1 << 16, ste)
    _check_bwd(got, want32, acc64, abs64, n_terms_max=N * 8)


@gpu
@pytest.mark.parametrize("case", ["minimum_workspace", "lane_stores", "overlapped_with_coarse_levels"])
def test_bounded_further_routes(cuda, oracle, case):
    """The minimum workspace (64 item slots per bin: most items take the spill path, from the walk's one-pair set-up), the
    lane-store bin pass, and the overlapped entry with two coarse levels on the merge kernel next to the three binned."""
    from cnc_amd import _lib
    N, F = (70001, 8) if case == "overlapped_with_coarse_levels" else (9001, 8)
    coarse = case == "overlapped_with_coarse_levels"
    offs, res, emb, x, g, want32, acc64, abs64 = _bounded_reference(N, F, True, coarse)
    kw = {}
    if case == "minimum_workspace":
        kw["ws_bytes"] = 3 * 256 * (16 + 64 * 16)
    elif case == "lane_stores":
        kw["flags"] = _lib.CNC_FLAG_BIN_LANE_STORES
    else:
        kw["overlapped"] = True
    got = _call(cuda, g, x, emb, offs, res, 3, 1 << 16, True, **kw)
    _check_bwd(got, want32, acc64, abs64, n_terms_max=N * 8)
    if coarse:
        assert np.abs(got[: int(offs[2])]).max() > 0 and np.abs(got[int(offs[2]):]).max() > 0
