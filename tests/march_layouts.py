"""Ray sets and occupancy grids for the marcher tests (tests/test_march_layouts.py on the CPU, tests/test_gpu_march_matrix.py
on the GPU), from NumPy and cnc_amd.synthetic alone.  A helper module, not a conftest.

A layout is (o [n,3], d [n,3], near [n], far [n]) in float32.  Every input is finite except `far = inf` where the bench
frame has it.

  frame(far)    bench.py's own frame, constants restated here: 800 x 800 pinhole rays (angle 0.6911, radius 4, azimuth
                0.7, elevation 0.5) in image order, step 5e-3, near 0, far inf (bench.build_workload) or 1e10 (the
                estimator).  `with_edges` overwrites a few dozen of its rays with the edge rays below.
  batch(n)      a training batch: n rays (37 000 by default) drawn at random from six cameras, so not in image order,
                stratified near = U[0, step), far 1e10; its grid is the ball with 4 % of the cells flipped.
  lengths(n)    rays of the bench camera that cross a 128^3 grid with every cell set; far = t_enter + (k + 0.25) step sets
                the sample count of each ray to k or k + 1.  k runs through TARGETS (and TARGETS_ROW8 for the 8-entry
                staging row), in an order (CYCLE) in which neighbours differ by an order of magnitude, shifted by five
                places per 64-ray block, so that every length comes to stand in lane 0 and lane 63 of a 64-ray block and
                in lanes 0 and 15 of a 16-ray block.  k = 0 is far before the entry.
  edge_rays()   axis-aligned rays (two zero components, one), an origin inside the box, one on a face, misses, grazes of
                an edge and a corner, near beyond the exit, far before the entry; shuffled among the others by
                `with_edges` wherever a layout has four times as many rays as there are edge rays.

Grids (GRIDS): one 128^3; two nested 128^3 (2 048 coarse words: the limit of the LDS bitmap); two nested 132^3 (just
over it: no bitmap); four nested 64^3; one 64 x 32 x 48.  Level k covers the box scaled by 2^k, as OccGridEstimator has
it; level 0 holds the ball, outer levels a sparse speckle, so a frame stays near 10^8 samples."""
import math

import numpy as np

from cnc_amd import synthetic

f32 = np.float32
STEP = 5e-3                                     # bench.STEP_SIZE
CAMERA = (800, 800, 0.6911, 4.0, 0.7, 0.5)      # bench.build_workload: height, width, angle, radius, azimuth, elevation
BOX = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)         # bench.AABB
FAR_ESTIMATOR = 1e10
N_BATCH = 37_000
TARGETS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 400)
TARGETS_ROW8 = (7, 8, 9)
# neighbours in the cycle are far apart in length; 19 entries, and 5 is coprime to 19
CYCLE = (400, 0, 256, 1, 65, 7, 257, 2, 64, 15, 255, 8, 63, 16, 33, 9, 32, 17, 31)
assert sorted(CYCLE) == sorted(TARGETS + TARGETS_ROW8)

_FRAME = {}


def _camera_rays(height, width, angle, radius, azimuth, elevation):
    o, d = synthetic.pinhole_rays(height, width, angle, radius, azimuth, elevation)
    return o.numpy().copy(), d.numpy().copy()


def frame(far=np.inf):
    """The bench frame: 640 000 rays in image order."""
    if "rays" not in _FRAME:
        _FRAME["rays"] = _camera_rays(*CAMERA)
    o, d = _FRAME["rays"]
    n = o.shape[0]
    return o.copy(), d.copy(), np.zeros(n, f32), np.full(n, far, f32)


def edge_rays():
    """(o, d, near, far) of the edge cases, for the box BOX; near / far are NaN where the layout's own value stays."""
    s = 1.0 / math.sqrt(2.0)
    rows = [
        # origin, direction, near, far
        ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), None, None),            # two zero components
        ((0.3, -4.0, 0.1), (0.0, 1.0, 0.0), None, None),
        ((4.0, -0.2, 0.7), (-1.0, 0.0, 0.0), None, None),
        ((0.2, 0.1, 4.0), (0.0, 0.0, -1.0), None, None),
        ((-4.0, 0.3, 0.2), (s, s, 0.0), None, None),                 # one zero component
        ((0.1, 4.0, -3.0), (0.0, -0.8, 0.6), None, None),
        ((3.0, 0.0, 0.4), (-0.6, 0.0, -0.8), None, None),
        ((0.1, 0.2, 0.3), (1.0, 0.0, 0.0), None, None),              # origin inside the box
        ((-0.4, 0.5, 0.2), (0.48, -0.6, 0.64), None, None),
        ((0.0, 0.0, 0.0), (-s, 0.0, s), None, None),
        ((1.5, 0.2, -0.3), (-0.8, 0.6, 0.0), None, None),            # origin on a face, pointing in
        ((0.3, -1.5, 0.4), (0.36, 0.8, 0.48), None, None),
        ((1.5, 0.2, -0.3), (0.8, 0.6, 0.0), None, None),             # origin on a face, pointing out
        ((4.0, 4.0, 4.0), (0.57735026, 0.57735026, 0.57735026), None, None),   # misses: pointing away
        ((5.0, 5.0, 5.0), (1.0, 0.0, 0.0), None, None),
        ((0.0, 4.0, 1.6), (0.0, -1.0, 0.0), None, None),             # parallel to a face, just outside
        ((-4.0, 2.5, 0.0), (0.8, 0.6, 0.0), None, None),
        ((-4.0, 1.5, 1.5), (1.0, 0.0, 0.0), None, None),             # along an edge of the box
        ((-4.0, 1.4999, 1.4999), (1.0, 0.0, 0.0), None, None),       # just inside that edge
        ((-3.0, 3.0, 0.2), (s, -s, 0.0), None, None),                # through the edge x = -1.5 .. y = 1.5: grazes it
        ((-3.0, 2.999, 0.2), (s, -s, 0.0), None, None),
        ((-3.0, -3.0, -3.0), (0.57735026, 0.57735026, 0.57735026), None, None),   # corner to corner
        ((-3.0, 3.0, -1.4999), (0.57735026, -0.57735026, 0.57735026), None, None),  # clips a corner
        ((0.0, 0.0, -4.0), (0.0, 0.0, 1.0), 6.0, None),              # near beyond the exit (t_exit = 5.5)
        ((0.2, -4.0, 0.3), (0.0, 0.6, 0.8), 9.0, None),
        ((0.1, 0.1, -4.0), (0.0, 0.0, 1.0), None, 2.0),              # far before the entry (t_enter = 2.5)
        ((-4.0, 0.3, 0.2), (s, s, 0.0), None, 1.0),
        ((0.1, 0.1, -4.0), (0.0, 0.0, 1.0), 3.0, 3.0),               # near == far inside the box
        ((0.1, 0.1, -4.0), (0.0, 0.0, 1.0), 3.0, 3.0125),            # two and a half steps wide
    ]
    o = np.array([r[0] for r in rows], f32)
    d = np.array([r[1] for r in rows], f32)
    near = np.array([np.nan if r[2] is None else r[2] for r in rows], f32)
    far = np.array([np.nan if r[3] is None else r[3] for r in rows], f32)
    return o, d, near, far


def edge_positions(n, seed=5):
    """Where `with_edges` puts the edge rays in a layout of n rays."""
    return np.random.default_rng(seed).choice(n, size=edge_rays()[0].shape[0], replace=False)


def with_edges(layout, seed=5):
    """The layout with the edge rays written over rays at seeded random places (none when it has too few rays)."""
    o, d, near, far = (a.copy() for a in layout)
    eo, ed, en, ef = edge_rays()
    n, m = o.shape[0], eo.shape[0]
    if n < 4 * m:
        return o, d, near, far
    at = edge_positions(n, seed)
    o[at], d[at] = eo, ed
    near[at] = np.where(np.isnan(en), near[at], en)
    far[at] = np.where(np.isnan(ef), far[at], ef)
    return o, d, near, far


def batch(n=N_BATCH, seed=11, step=STEP, edges=True):
    """n rays drawn at random from six cameras (so not in image order), stratified near, far = 1e10."""
    rng = np.random.default_rng(seed)
    cams = [(0.6911, 4.0, 0.7, 0.5), (0.6911, 4.0, 2.3, 0.2), (0.6911, 4.0, -1.1, -0.4), (0.9, 5.0, 3.9, 0.9),
            (0.6911, 6.5, 0.1, -0.8), (1.1, 3.2, 5.2, 0.05)]
    which = rng.integers(0, len(cams), size=n)
    o, d = np.empty((n, 3), f32), np.empty((n, 3), f32)
    for c, (angle, radius, az, el) in enumerate(cams):
        co, cd = _camera_rays(200, 200, angle, radius, az, el)
        sel = np.nonzero(which == c)[0]
        pix = rng.integers(0, co.shape[0], size=sel.size)
        o[sel], d[sel] = co[pix], cd[pix]
    near = rng.uniform(0.0, step, size=n).astype(f32)
    far = np.full(n, FAR_ESTIMATOR, f32)
    lay = (o, d, near, far)
    return with_edges(lay, seed + 1) if edges else lay


def edges_first(n, seed=19):
    """The edge rays (near 0 and far 1e10 where they name none) followed by rays of a batch: the first n of them."""
    eo, ed, en, ef = edge_rays()
    bo, bd, bn, bf = batch(max(n, 1), seed, edges=False)
    en, ef = np.where(np.isnan(en), f32(0), en), np.where(np.isnan(ef), f32(FAR_ESTIMATOR), ef)
    return tuple(np.concatenate([a, b])[:n].astype(f32) for a, b in ((eo, bo), (ed, bd), (en, bn), (ef, bf)))


def _slab(o, d, box=BOX):
    """Entry and exit distances of the box in float64 (to choose rays by; every assertion goes through the oracle)."""
    o, d = o.astype(np.float64), d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = (np.asarray(box[:3]) - o) / d
        b = (np.asarray(box[3:]) - o) / d
    lo, hi = np.minimum(a, b).max(-1), np.maximum(a, b).min(-1)
    return lo, hi


def lengths_targets(n, cycle=CYCLE):
    """The length asked of ray r: cycle[(lane + 5 block) mod len], lane and block those of 64-ray blocks."""
    r = np.arange(n)
    return np.asarray(cycle)[((r % 64) + 5 * (r // 64)) % len(cycle)]


def lengths(n=16_384, seed=3, step=STEP, cycle=CYCLE, edges=True):
    """Rays of the bench camera whose chord through the box is longer than the longest target, drawn at random; the
    grid to march is GRIDS['full128'].  Returns the layout and the targets (-1 where an edge ray stands)."""
    o, d, _, _ = frame()
    lo, hi = _slab(o, d)
    ok = np.nonzero((hi - lo) > (max(cycle) + 4) * step)[0]
    pick = np.random.default_rng(seed).choice(ok, size=n, replace=n > ok.size)
    o, d, lo = o[pick], d[pick], lo[pick]
    k = lengths_targets(n, cycle)
    far = np.where(k == 0, lo - step, lo + (k + 0.25) * step).astype(f32)
    lay = (o, d, np.zeros(n, f32), far)
    if edges:
        out = with_edges(lay, seed + 1)
        k = np.where((out[0] != lay[0]).any(-1) | (out[1] != lay[1]).any(-1), -1, k)
        lay = out
    return lay, k


# ----------------------------------------------------------------------------------------------------------------------
# grids
# ----------------------------------------------------------------------------------------------------------------------
def level_boxes(levels, box=BOX):
    """Level k = the box scaled by 2^k about its centre (OccGridEstimator)."""
    b = np.asarray(box, np.float64)
    c, h = (b[:3] + b[3:]) / 2, (b[3:] - b[:3]) / 2
    return np.stack([np.concatenate([c - h * 2 ** k, c + h * 2 ** k]) for k in range(levels)]).astype(f32)


def ball(res, box=BOX, radius=1.0):
    """Cells of a (rx, ry, rz) grid over `box` whose centre lies inside the ball."""
    ax = [((np.arange(r, dtype=f32) + f32(0.5)) / f32(r) * f32(box[3 + a] - box[a]) + f32(box[a])) for a, r in enumerate(res)]
    gx, gy, gz = np.meshgrid(*ax, indexing="ij")
    return (gx * gx + gy * gy + gz * gz) < f32(radius * radius)


def nested(levels, res, flip=0.04, speckle=0.01, seed=17):
    """Level 0: the ball with `flip` of its cells flipped; outer levels: `speckle` of the cells set."""
    rng = np.random.default_rng(seed)
    shape = (res,) * 3 if np.isscalar(res) else tuple(res)
    out = np.zeros((levels,) + shape, bool)
    out[0] = ball(shape) ^ (rng.uniform(size=shape) < flip)
    for k in range(1, levels):
        out[k] = rng.uniform(size=shape) < speckle
    return out


def _grids():
    g = {}
    g["ball128"] = lambda: (synthetic.ball_binaries(128, radius=1.0).numpy().copy(), level_boxes(1))      # the bench grid
    g["flipped128"] = lambda: (nested(1, 128), level_boxes(1))                                            # the batch's grid
    g["full128"] = lambda: (np.ones((1, 128, 128, 128), bool), level_boxes(1))                            # the lengths' grid
    g["nested2x128"] = lambda: (nested(2, 128), level_boxes(2))                                           # 2 048 words
    g["nested2x132"] = lambda: (nested(2, 132), level_boxes(2))                                           # 2 247: none
    g["nested4x64"] = lambda: (nested(4, 64, speckle=0.004), level_boxes(4))
    g["box64x32x48"] = lambda: (nested(1, (64, 32, 48)), level_boxes(1))
    return g


GRIDS = _grids()
SINGLE = ("ball128", "flipped128", "full128", "box64x32x48")
NESTED = ("nested2x128", "nested2x132", "nested4x64")
_GRID_CACHE = {}


def grid(name):
    """(binaries [levels, rx, ry, rz] bool, aabbs [levels, 6] float32); built once."""
    if name not in _GRID_CACHE:
        _GRID_CACHE[name] = GRIDS[name]()
    return _GRID_CACHE[name]


def coarse_words(binaries):
    """Bit (((g cx + x) cy + y) cz + z) = any cell of the 4 x 4 x 4 block, packed into uint32 words, low bit first."""
    n, rx, ry, rz = binaries.shape
    blocks = binaries.reshape(n, rx // 4, 4, ry // 4, 4, rz // 4, 4).any(axis=(2, 4, 6)).reshape(-1)
    bits = np.zeros((blocks.size + 31) // 32 * 32, np.uint32)
    bits[:blocks.size] = blocks
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(-1).astype(np.uint32)


def crossings(t_lo, t_hi):
    """The box crossings of every ray in order along it, as OccGridEstimator._march hands them to the march: sorted
    (entry..., exit...) distances and which crossing each is.  One box: (entry, exit) as it stands."""
    cat = np.concatenate([t_lo, t_hi], axis=-1).astype(f32)
    if t_lo.shape[1] == 1:
        order = np.broadcast_to(np.arange(2, dtype=np.int64), cat.shape).copy()
        return cat, order
    order = np.argsort(cat, axis=-1, kind="stable").astype(np.int64)
    return np.take_along_axis(cat, order, axis=-1), order


def whole_blocks(n, at_most=4096, seed=1):
    """Indices of whole 64-ray blocks, at most `at_most` rays of them (all rays when there are fewer)."""
    if n <= at_most:
        return np.arange(n)
    blocks = np.sort(np.random.default_rng(seed).choice(n // 64, size=at_most // 64, replace=False))
    return (blocks[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)


def mask_every_fourth(n):
    m = np.ones(n, bool)
    m[::4] = False
    return m


def mask_whole_waves(n, seed=9):
    """Kills about a third of the 64-ray blocks whole, and the first and the last one."""
    blocks = (n + 63) // 64
    dead = np.random.default_rng(seed).uniform(size=blocks) < 0.33
    dead[0] = dead[-1] = True
    return ~np.repeat(dead, 64)[:n]


# ----------------------------------------------------------------------------------------------------------------------
# checks and loops that the CPU and the GPU tests share
# ----------------------------------------------------------------------------------------------------------------------
def lengths_coverage(counts, wanted):
    """Every wanted length occurs, in lane 0 and lane 63 of some 64-ray block and in lanes 0 and 15 of some 16-ray block."""
    r = np.arange(counts.shape[0])
    for k in wanted:
        has = counts == k
        assert has.any(), k
        for lanes, width in ((0, 64), (63, 64), (0, 16), (15, 16)):
            assert (has & (r % width == lanes)).any(), (k, lanes, width)


def eval_loop_rounds(march, n, limit):
    """The evaluation renderer's loop (render_image_with_occgrid_test): march at most `limit` samples on the live rays,
    restart the rays that used them all from their termination planes, until none is left.  `march(mask, near)` ->
    (counts, terminate planes).  Returns the summed counts and the number of rounds."""
    mask, near = np.ones(n, bool), None
    totals, rounds = np.zeros(n, np.int64), 0
    while mask.any():
        assert rounds < 64
        cnt, term = march(mask, near, rounds)
        totals += cnt
        near = term if near is None else np.where(mask, term, near).astype(np.float32)
        mask = mask & (cnt == limit)
        rounds += 1
    return totals, rounds


EVAL_N, EVAL_LIMIT = (1 << 17) + 1, 64


def eval_loop_layout():
    """2^17 + 1 rays of the bench frame, in image order, with the edge rays mixed in."""
    o, d, near, far = frame(FAR_ESTIMATOR)
    at = np.sort(np.random.default_rng(4).choice(o.shape[0], size=EVAL_N, replace=False))
    return with_edges((o[at], d[at], near[at], far[at]))
