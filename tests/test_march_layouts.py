"""The reference of tests/test_gpu_march_matrix.py, pinned before anyone trusts it: on the layouts of tests/march_layouts.py
the oracle's marcher (oracle/cnc_oracle.c) equals the independent NumPy twin (tests/np_twins.py) on whole 64-ray blocks,
the lengths layouts hold every length they are built for in the lanes they are built for, the nested grids have rays
that cross several levels and rays that only hit the outer one, and the evaluation loop's allowance holds on the oracle
alone.  CPU only; about 13 s on 16 cores, of the order of tests/test_np_twins.py (most of it the twin's 4 096-ray marches)."""
import numpy as np
import pytest

import march_layouts as ML
import np_twins as tw

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")     # 1/0 for axis-parallel rays, as on the GPU


def _layout(name):
    if name == "frame":
        return ML.with_edges(ML.frame(ML.FAR_ESTIMATOR)), "ball128"
    if name == "frame_bench":
        return ML.frame(), "ball128"
    if name == "batch":
        return ML.batch(), "flipped128"
    if name == "batch_noncubic":
        return ML.batch(8192, seed=13), "box64x32x48"
    if name == "lengths":
        return ML.lengths(16_384)[0], "full128"
    raise KeyError(name)


@pytest.mark.parametrize("limit", [-1, 9])
@pytest.mark.parametrize("name", ["frame", "frame_bench", "batch", "batch_noncubic", "lengths"])
def test_oracle_equals_the_numpy_twin(oracle, name, limit):
    """Counts, t_left, t_right, t_mid and termination planes on at most 4 096 rays in whole 64-ray blocks (single grids:
    the twin handles one)."""
    (o, d, near, far), gname = _layout(name)
    if name == "frame_bench" and limit > 0:
        limit = 64
    most = 4096 if limit < 0 else 2048
    at = ML.whole_blocks(o.shape[0], most)
    if name == "frame":               # the blocks of half of the edge rays take the place of as many random blocks
        extra = (np.unique(ML.edge_positions(o.shape[0])[::2] // 64)[:, None] * 64 + np.arange(64)[None]).reshape(-1)
        at = np.unique(np.concatenate([extra, ML.whole_blocks(o.shape[0], most - extra.size)]))
        assert at.size <= most and at.size % 64 == 0
    o, d, near, far = o[at], d[at], near[at], far[at]
    binaries, aabbs = ML.grid(gname)
    n = o.shape[0]
    tmin, tmax, hits = oracle.ray_aabb_intersect(o, d, aabbs)
    iv, sm, term = oracle.traverse_grids(o, d, binaries, aabbs, near, far, ML.STEP, 0.0,
                                         traverse_steps_limit=limit if limit > 0 else None, over_allocate=limit > 0)
    got = tw.traverse_grids(o, d, binaries, aabbs[0], tmin[:, 0], tmax[:, 0], hits[:, 0], near, far, ML.STEP, limit)
    cnts = np.asarray(sm["chunk_cnts"])
    assert np.array_equal(got["counts"], cnts)
    assert cnts.sum() > 2 * n and (cnts == 0).any()
    valid = sm["is_valid"]
    assert np.array_equal(sm["vals"][valid], got["t_mid"])
    assert np.array_equal(sm["ray_indices"][valid], got["ray"])
    assert np.array_equal(iv["vals"][iv["is_left"]], got["t_left"])
    assert np.array_equal(iv["vals"][iv["is_right"]], got["t_right"])
    wrote = np.ones(n, bool) if limit > 0 else cnts > 0            # the rule of test_np_twins.test_traverse_grids
    assert np.array_equal(term[wrote], got["terminate"][wrote])
    assert np.array_equal(iv["chunk_cnts"], cnts + np.bincount(got["ray"][got["first"]], minlength=n))


def test_bench_frame_is_the_bench_frame(oracle):
    """The figures bench.py's frame is known by: 640 000 rays, 68 022 266 samples, at most 406 on a ray."""
    o, d, near, far = ML.frame()
    binaries, aabbs = ML.grid("ball128")
    _, sm, _ = oracle.traverse_grids(o, d, binaries, aabbs, near, far, ML.STEP, 0.0)
    assert o.shape[0] == 640_000 and int(sm["chunk_cnts"].sum()) == 68_022_266 and int(sm["chunk_cnts"].max()) == 406


@pytest.mark.parametrize("n", [16_384, (1 << 17) + 1])
def test_lengths_layout_covers_every_length(oracle, n):
    (o, d, near, far), k = ML.lengths(n)
    binaries, aabbs = ML.grid("full128")
    _, sm, _ = oracle.traverse_grids(o, d, binaries, aabbs, near, far, ML.STEP, 0.0)
    counts = sm["chunk_cnts"]
    ML.lengths_coverage(counts, ML.TARGETS + ML.TARGETS_ROW8)
    asked = k >= 0
    assert np.isin(counts[asked] - k[asked], (0, 1)).all()                  # k or k + 1, nothing else
    assert 0.6 < (counts[asked] == k[asked]).mean() < 0.9
    # neighbouring lanes hold very different lengths: some rows fill many times over while others hold nothing
    blocks = counts[: n // 64 * 64].reshape(-1, 64)
    assert (blocks.max(1) >= 400).all() and (blocks.min(1) <= 1).all()


@pytest.mark.parametrize("gname", ML.NESTED)
@pytest.mark.parametrize("lname", ["batch", "frame"])
def test_nested_layouts_cross_levels(oracle, gname, lname):
    """Rays with samples in two or more levels, and rays that hit only an outer level and have samples there."""
    o, d, near, far = ML.batch() if lname == "batch" else ML.with_edges(ML.frame(ML.FAR_ESTIMATOR))
    binaries, aabbs = ML.grid(gname)
    if lname == "frame":
        at = ML.whole_blocks(o.shape[0], 65_536, seed=2)
        o, d, near, far = o[at], d[at], near[at], far[at]
    t0, t1, hits = oracle.ray_aabb_intersect(o, d, aabbs)
    t_sorted, t_indices = ML.crossings(t0, t1)
    _, sm, _ = oracle.traverse_grids(o, d, binaries, aabbs, near, far, ML.STEP, 0.0, t_sorted=t_sorted,
                                     t_indices=t_indices, hits=hits)
    cnt, ri, t = sm["chunk_cnts"], sm["ray_indices"], sm["vals"]
    inner = (t >= t0[ri, 0]) & (t <= t1[ri, 0]) & hits[ri, 0]
    n = o.shape[0]
    n_in, n_out = np.bincount(ri[inner], minlength=n), np.bincount(ri[~inner], minlength=n)
    assert ((n_in > 0) & (n_out > 0)).sum() > n // 100
    outer_only = ~hits[:, 0] & hits[:, 1:].any(-1)
    if lname == "batch":
        assert (outer_only & (cnt > 0)).sum() >= 16
    assert cnt.mean() < 400                           # the outer levels stay sparse: a frame is ~10^8 samples at most


def test_eval_loop_allowance_holds_on_the_oracle_alone(oracle):
    """The rounds of the loop sum to one unlimited march up to the allowance of
    test_gpu_march.test_traverse_over_allocate_iterative (a restart recomputes the cell crossings from another origin:
    at most 2 samples on a ray, on fewer than 5 % of the rays) — on the oracle, on the layout the GPU test uses."""
    o, d, near0, far = ML.eval_loop_layout()
    binaries, aabbs = ML.grid("ball128")
    t0, t1, hits = oracle.ray_aabb_intersect(o, d, aabbs)
    t_sorted, t_indices = ML.crossings(t0, t1)
    kw = dict(t_sorted=t_sorted, t_indices=t_indices, hits=hits)
    _, full, _ = oracle.traverse_grids(o, d, binaries, aabbs, near0, far, ML.STEP, 0.0, **kw)

    def march(mask, near, _):
        _, sm, term = oracle.traverse_grids(o, d, binaries, aabbs, near0 if near is None else near, far, ML.STEP, 0.0,
                                            traverse_steps_limit=ML.EVAL_LIMIT, over_allocate=True, rays_mask=mask, **kw)
        return sm["chunk_cnts"], term

    totals, rounds = ML.eval_loop_rounds(march, ML.EVAL_N, ML.EVAL_LIMIT)
    diff = np.abs(totals - full["chunk_cnts"])
    assert rounds >= 6 and diff.max() <= 2 and (diff > 0).mean() < 0.05


def test_coarse_words_and_crossings_helpers():
    b = np.zeros((2, 8, 4, 4), bool)
    b[0, 5, 1, 2] = b[1, 0, 0, 0] = True
    assert ML.coarse_words(b).tolist() == [0b0110]
    binaries, _ = ML.grid("nested2x128")
    assert ML.coarse_words(binaries).size == 2048
    t_lo, t_hi = np.array([[2.0, 1.0]], np.float32), np.array([[3.0, 5.0]], np.float32)
    ts, ti = ML.crossings(t_lo, t_hi)
    assert ts.tolist() == [[1.0, 2.0, 3.0, 5.0]] and ti.tolist() == [[1, 0, 2, 3]]
    assert not ML.mask_whole_waves(1000)[:64].any() and ML.mask_whole_waves(1000)[64:].any()
