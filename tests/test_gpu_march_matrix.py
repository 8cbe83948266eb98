"""The occupancy-grid marcher (cnc_amd/csrc/march.hip) at frame and batch size against the CPU oracle, bit for bit, on the
layouts of tests/march_layouts.py (tests/test_march_layouts.py pins the oracle on them to the NumPy twin).

The C ABI is called directly and the caller owns every buffer.  Result buffers are `total + 4096` long and start as NaN
(floats), -1 (indices) and 0xFF (flags); `chunk_cnts` starts as 0, as the ABI asks.  Every march asserts: counts and
starts equal the oracle's; t_starts == vals[is_left] and t_ends == vals[is_right]; the ray ids, as int64 and as int32;
the termination planes on the rays for which the reference defines them (test_gpu_march._cmp_segments' rule), with the
poison kept on masked-out rays; nothing written behind `total`; positions and directions equal to the float32 expression
of test_gpu_march.test_sample_positions_equals_torch_expression evaluated by torch on the oracle's (ray, t0, t1), with and
without the unit-cube mapping.  No tolerance anywhere.

Launch paths of cnc_march_samples[_coarse] and the cases that reach them (each with the bitmap, through
cnc_march_samples_coarse, and without, through cnc_march_samples; each resumed at the first sample and whole-ray):

  direct fill, k_traverse<3>            test_below_2p17 (1 .. 65 and 2^17 - 1 rays, switch set and unset), test_training_batch
                                        (37 000 rays), test_grids[4096], test_limits_and_masks[4096]
  staged, 16 rays per block             the same cases with CNC_MARCH_DIRECT_MAX=0
  staged, 64 rays per block,            test_from_2p17 (2^17, 2^17 + 1 rays of the lengths layout), test_grids[131073],
  rows of 8, 16, 32, 64 and unset       test_limits_and_masks[131073]; test_frame (640 000 rays: the default and every
                                        switch flipped once, the 64-entry row with the 2 048-word bitmap among them)
  CONE0 / general dt                    every case above runs cone_angle 0 and 4e-3
  the evaluation loop                   test_eval_loop (2^17 + 1 rays, mask + limit + restart from the planes)

cnc_traverse_grids (k_traverse<0> / <1>): test_traverse_grids_route.  cnc_ray_aabb_intersect: test_ray_aabb_at_frame_size.
cnc_occupancy_coarse_bits: test_coarse_bits.

The product rows x resume x bitmap runs on the lengths layout and on 2^17 + 1 rays of every grid; the 640 000-ray frame
takes the default configuration and each switch flipped once (the whole product there costs more than a tenth of the
rest of the GPU suite: profiles/r12_march_matrix.md)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import march_layouts as ML
from march_layouts import EVAL_LIMIT, EVAL_N, eval_loop_layout, eval_loop_rounds, lengths_coverage

pytestmark = pytest.mark.gpu
PAD = 4096
P17 = 1 << 17
CNC_ERR_UNSUPPORTED = -2
UNIT_BOX = (-1.5, -1.4, -1.3, 1.5, 1.6, 1.7)          # the mapping box of test_gpu_march's position checks
CONES = [0.0, 4e-3]
_REF = {}                                              # the last reference and its device copies


def _api():
    from cnc_amd import _lib as L
    return L.lib(), L.stream


def _p(t):
    """Device address of a tensor THE CALLER HOLDS until the synchronise."""
    return None if t is None else t.data_ptr()


def _dev(cuda, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=cuda)


def _poison(cuda, shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, float("nan"), dtype=dtype, device=cuda)
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=dtype, device=cuda)
    return torch.full(shape, -1, dtype=dtype, device=cuda)


def _untouched(buf):
    if buf.dtype == torch.float32:
        return bool(torch.isnan(buf).all())
    return bool((buf == (0xFF if buf.dtype == torch.uint8 else -1)).all())


def _same_bits(a, b):
    """Equal bit for bit, the NaN poison included (NaN != NaN for torch.equal)."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# a scene on the device, and the oracle's answer for it
# ----------------------------------------------------------------------------------------------------------------------
class Scene:
    """Rays and grid on the device.  The box crossings come from cnc_ray_aabb_intersect on poisoned buffers, are held
    against the oracle's, and are sorted as OccGridEstimator._march sorts them."""

    def __init__(self, cuda, oracle, layout, gname):
        lib, stream = _api()
        self.cuda, self.gname = cuda, gname
        self.o, self.d, self.near, self.far = (np.ascontiguousarray(a, np.float32) for a in layout)
        self.binaries, self.aabbs = ML.grid(gname)
        self.n, self.levels = self.o.shape[0], self.binaries.shape[0]
        self.res = tuple(int(v) for v in self.binaries.shape[1:])
        t0, t1, hits = oracle.ray_aabb_intersect(self.o, self.d, self.aabbs)
        self.D = NS(o=_dev(cuda, self.o), d=_dev(cuda, self.d), near=_dev(cuda, self.near), far=_dev(cuda, self.far),
                    binaries=_dev(cuda, self.binaries.astype(np.uint8)), aabbs=_dev(cuda, self.aabbs))
        g0, g1 = (_poison(cuda, (self.n, self.levels), torch.float32) for _ in range(2))
        gh = _poison(cuda, (self.n, self.levels), torch.uint8)
        rc = lib.cnc_ray_aabb_intersect(_p(self.D.o), _p(self.D.d), _p(self.D.aabbs), self.n, self.levels, -float("inf"),
                                        float("inf"), float("inf"), _p(g0), _p(g1), _p(gh), stream(cuda))
        torch.cuda.synchronize()
        assert rc == 0
        assert np.array_equal(g0.cpu().numpy(), t0) and np.array_equal(g1.cpu().numpy(), t1)
        assert np.array_equal(gh.cpu().numpy(), hits.astype(np.uint8))
        self.hits = hits
        self.t_sorted, self.t_indices = ML.crossings(t0, t1)
        self.D.hits, self.D.t_sorted, self.D.t_indices = gh, _dev(cuda, self.t_sorted), _dev(cuda, self.t_indices)
        self.D.box = _dev(cuda, np.asarray(UNIT_BOX, np.float32))
        # the coarse bitmap, where the kernels take one for this shape
        self.words = None
        nw = int(lib.cnc_occupancy_coarse_words(self.levels, *self.res))
        if nw:
            self.words = _poison(cuda, (nw,), torch.int32)
            rc = lib.cnc_occupancy_coarse_bits(_p(self.D.binaries), self.levels, *self.res, _p(self.words), stream(cuda))
            torch.cuda.synchronize()
            assert rc == 0
            assert np.array_equal(self.words.cpu().numpy().view(np.uint32), ML.coarse_words(self.binaries))

    def oracle_kw(self):
        return dict(t_sorted=self.t_sorted, t_indices=self.t_indices, hits=self.hits)


def reference(oracle, sc, step, cone, limit=-1, mask=None, near=None, key=None):
    """The oracle's march in the form cnc_march_samples returns: counts, starts, (ray, t0, t1) per sample, planes.
    limit > 0: the over-allocated single pass with the mask (grid.cu:400-440); unlimited: the two passes, which take no
    mask, with the masked-out rays' samples removed afterwards (the rays are independent of each other)."""
    if key is not None and _REF.get("key") == key:
        return _REF["ref"]
    _REF.clear()
    near = sc.near if near is None else near
    if limit > 0:
        m = np.ones(sc.n, bool) if mask is None else mask
        iv, sm, term = oracle.traverse_grids(sc.o, sc.d, sc.binaries, sc.aabbs, near, sc.far, step, cone,
                                             traverse_steps_limit=limit, over_allocate=True, rays_mask=m, **sc.oracle_kw())
        counts, ray = sm["chunk_cnts"], sm["ray_indices"][sm["is_valid"]]
        t0, t1 = iv["vals"][iv["is_left"]], iv["vals"][iv["is_right"]]
        term_on = m.copy()
    else:
        iv, sm, term = oracle.traverse_grids(sc.o, sc.d, sc.binaries, sc.aabbs, near, sc.far, step, cone, **sc.oracle_kw())
        counts, ray = sm["chunk_cnts"], sm["ray_indices"]
        t0, t1 = iv["vals"][iv["is_left"]], iv["vals"][iv["is_right"]]
        term_on = counts > 0
        if mask is not None:
            keep = mask[ray]
            ray, t0, t1 = ray[keep], t0[keep], t1[keep]
            counts = counts * mask
            term_on = term_on & mask
    assert t0.shape == t1.shape == ray.shape and int(counts.sum()) == ray.shape[0]
    cuda = sc.cuda
    r = NS(counts=counts, total=int(counts.sum()), term=term, term_on=term_on, dead=~mask if mask is not None else None)
    r.D = NS(counts=_dev(cuda, counts), starts=_dev(cuda, np.cumsum(counts) - counts), ray=_dev(cuda, ray),
             t0=_dev(cuda, t0), t1=_dev(cuda, t1))
    # the reference's rgb_sigma_fn expression (examples/utils.py:251-262) and the field's box mapping (ngp.py:518-519)
    D, box = r.D, sc.D.box
    D.dirs = sc.D.d[D.ray]
    D.pos = sc.D.o[D.ray] + D.dirs * (D.t0 + D.t1)[:, None] / 2.0
    D.pos_box = (D.pos - box[:3]) / (box[3:] - box[:3])
    if key is not None:
        _REF.update(key=key, ref=r)
    return r


def march(sc, ref, step, cone, *, limit=-1, mask=None, near=None, coarse=False, resume=True, what=""):
    """Count pass, fill pass with every extra (twice: positions with and without the box mapping), all on poisoned
    buffers, through cnc_march_samples_coarse (`coarse`) or cnc_march_samples; asserts everything the module names."""
    lib, stream = _api()
    cuda, n, D = sc.cuda, sc.n, sc.D
    s = stream(cuda)
    mask_d = None if mask is None else _dev(cuda, mask.astype(np.uint8))
    near_d = D.near if near is None else _dev(cuda, near)
    counts = torch.zeros(n, dtype=torch.int64, device=cuda)
    term = _poison(cuda, (n,), torch.float32)
    rstate = _poison(cuda, (n, 8), torch.int32) if resume else None
    head = (_p(D.o), _p(D.d), _p(mask_d), n, _p(D.binaries), sc.levels, *sc.res, _p(D.aabbs), _p(D.hits), _p(D.t_sorted),
            _p(D.t_indices), _p(near_d), _p(D.far), float(step), float(cone), int(limit))

    def call(*tail):
        if coarse:
            assert sc.words is not None
            rc = lib.cnc_march_samples_coarse(*head, *tail, _p(sc.words), s)
        else:
            rc = lib.cnc_march_samples(*head, *tail, s)
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)

    call(_p(counts), None, None, None, None, _p(term), _p(rstate), None, None, None, None)
    assert torch.equal(counts, ref.D.counts), (what, "counts")
    starts = torch.cumsum(counts, 0) - counts
    assert torch.equal(starts, ref.D.starts), (what, "starts")
    got_term = term.cpu().numpy()
    assert np.array_equal(got_term[ref.term_on], ref.term[ref.term_on]), (what, "terminate planes")
    if ref.dead is not None:
        assert np.isnan(got_term[ref.dead]).all(), (what, "a masked-out ray's plane was written")
    total = ref.total
    for box in (D.box, None):
        ts, te = (_poison(cuda, (total + PAD,), torch.float32) for _ in range(2))
        ri, ri32 = _poison(cuda, (total + PAD,), torch.int64), _poison(cuda, (total + PAD,), torch.int32)
        pos, dirs = (_poison(cuda, (total + PAD, 3), torch.float32) for _ in range(2))
        call(_p(counts), _p(starts), _p(ts), _p(te), _p(ri), None, _p(rstate), _p(pos), _p(dirs), _p(ri32), _p(box))
        tag = (what, "box" if box is not None else "no box")
        assert torch.equal(counts, ref.D.counts), tag + ("counts after the fill",)
        assert torch.equal(ts[:total], ref.D.t0), tag + ("t_starts",)
        assert torch.equal(te[:total], ref.D.t1), tag + ("t_ends",)
        assert torch.equal(ri[:total], ref.D.ray), tag + ("ray ids int64",)
        assert torch.equal(ri32[:total].long(), ref.D.ray), tag + ("ray ids int32",)
        assert torch.equal(pos[:total], ref.D.pos_box if box is not None else ref.D.pos), tag + ("positions",)
        assert torch.equal(dirs[:total], ref.D.dirs), tag + ("directions",)
        for name, buf in (("t_starts", ts), ("t_ends", te), ("ray ids", ri), ("ray ids int32", ri32), ("positions", pos),
                          ("directions", dirs)):
            assert _untouched(buf[total:]), tag + (name, "written behind the total")


def launch_paths(sc):
    """(name, environment, resume, coarse) of every launch path a ray count of this size class can take."""
    if sc.n < P17:
        ways = [("direct", {"CNC_MARCH_DIRECT_MAX": str(P17)}), ("staged_16_rays", {"CNC_MARCH_DIRECT_MAX": "0"}), ("unset", {})]
    else:
        ways = [(f"row_{r}", {"CNC_PAIR_STAGE": str(r)}) for r in (8, 16, 32, 64)] + [("row_unset", {})]
    for name, env in ways:
        for resume in (True, False):
            for coarse in ((True, False) if sc.words is not None else (False,)):
                yield f"{name}/{'resume' if resume else 'whole_ray'}/{'bitmap' if coarse else 'no_bitmap'}", env, resume, coarse


def set_switches(monkeypatch, env):
    for k in ("CNC_MARCH_DIRECT_MAX", "CNC_PAIR_STAGE"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def run_paths(monkeypatch, sc, ref, step, cone, **kw):
    names = []
    for name, env, resume, coarse in launch_paths(sc):
        set_switches(monkeypatch, env)
        march(sc, ref, step, cone, coarse=coarse, resume=resume, what=name, **kw)
        names.append(name)
    set_switches(monkeypatch, {})
    return names


@pytest.fixture(scope="module", autouse=True)
def _drop_reference():
    yield
    _REF.clear()


def _lengths_scene(cuda, oracle, n):
    lay, k = ML.lengths(n)
    return Scene(cuda, oracle, lay, "full128"), k


# ----------------------------------------------------------------------------------------------------------------------
# cnc_march_samples / cnc_march_samples_coarse
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cone", CONES)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, P17 - 1])
def test_below_2p17(cuda, oracle, monkeypatch, n, cone):
    """Direct fill, staged fill with 16 rays per block, and the switch unset; the lengths layout (rows that fill many times
    over next to rows that hold nothing) and, for the small counts, the head of a batch on the flipped ball."""
    sc, _ = _lengths_scene(cuda, oracle, n)
    ref = reference(oracle, sc, ML.STEP, cone)
    assert ref.total >= 100
    if n == P17 - 1 and cone == 0.0:
        lengths_coverage(ref.counts, ML.TARGETS + ML.TARGETS_ROW8)
    names = run_paths(monkeypatch, sc, ref, ML.STEP, cone)
    assert len(names) == 12
    if n < 100:                                   # the edge rays themselves, then rays of a batch
        sc = Scene(cuda, oracle, ML.edges_first(n), "flipped128")
        ref = reference(oracle, sc, ML.STEP, cone)
        assert len(run_paths(monkeypatch, sc, ref, ML.STEP, cone)) == 12


@pytest.mark.parametrize("cone", CONES)
@pytest.mark.parametrize("n", [P17, P17 + 1])
def test_from_2p17(cuda, oracle, monkeypatch, n, cone):
    """The staged fill with 64 rays per block: rows of 8, 16, 32, 64 and the default, resumed and whole-ray, with and
    without the bitmap, on the lengths layout — every length in lane 0 and in lane 63 of some block."""
    sc, _ = _lengths_scene(cuda, oracle, n)
    ref = reference(oracle, sc, ML.STEP, cone)
    if cone == 0.0:
        lengths_coverage(ref.counts, ML.TARGETS + ML.TARGETS_ROW8)
    else:
        assert ref.counts.max() >= 400 and (ref.counts == 0).any()
    assert len(run_paths(monkeypatch, sc, ref, ML.STEP, cone)) == 20


@pytest.mark.parametrize("cone", CONES)
def test_training_batch(cuda, oracle, monkeypatch, cone):
    """The training batch itself: 37 000 rays drawn at random from six cameras, stratified near, the ball with 4 % of its
    cells flipped — the direct fill, the staged fill with 16 rays per block and the switch unset, each resumed and
    whole-ray, with and without the bitmap."""
    sc = Scene(cuda, oracle, ML.batch(), "flipped128")
    ref = reference(oracle, sc, ML.STEP, cone)
    assert sc.n == ML.N_BATCH and ref.total > 20 * sc.n and (ref.counts == 0).any()
    assert len(run_paths(monkeypatch, sc, ref, ML.STEP, cone)) == 12


def _grid_layout(gname, n):
    if gname == "full128":
        return ML.lengths(n)[0]
    return ML.batch(n, seed=29)


@pytest.mark.parametrize("cone", CONES)
@pytest.mark.parametrize("n", [4096, P17 + 1])
@pytest.mark.parametrize("gname", ["flipped128", "nested2x128", "nested2x132", "nested4x64", "box64x32x48"])
def test_grids(cuda, oracle, monkeypatch, gname, n, cone):
    """Every grid, at both size classes, through every launch path: the 2 048-word bitmap behind every row length (the
    64-entry row is the largest LDS footprint), the 132^3 pair the kernels take no bitmap for, four nested levels with
    the crossings sorted as the estimator sorts them, a grid that is no cube."""
    lib, stream = _api()
    sc = Scene(cuda, oracle, _grid_layout(gname, n), gname)
    ref = reference(oracle, sc, ML.STEP, cone)
    assert ref.total > 20 * n and (ref.counts == 0).any()
    names = run_paths(monkeypatch, sc, ref, ML.STEP, cone)
    if gname == "nested2x132":
        assert sc.words is None and not any(x.endswith("/bitmap") for x in names)
        # a bitmap handed over for a shape that takes none is refused, not read
        some = torch.zeros(4096, dtype=torch.int32, device=cuda)
        counts = torch.zeros(sc.n, dtype=torch.int64, device=cuda)
        D = sc.D
        rc = lib.cnc_march_samples_coarse(_p(D.o), _p(D.d), None, sc.n, _p(D.binaries), sc.levels, *sc.res, _p(D.aabbs),
                                          _p(D.hits), _p(D.t_sorted), _p(D.t_indices), _p(D.near), _p(D.far), ML.STEP, cone,
                                          -1, _p(counts), None, None, None, None, None, None, None, None, None, None,
                                          _p(some), stream(cuda))
        torch.cuda.synchronize()
        assert rc == CNC_ERR_UNSUPPORTED and int(counts.sum()) == 0
    else:
        assert sc.words is not None and sc.words.numel() == {"flipped128": 1024, "nested2x128": 2048, "nested4x64": 512,
                                                             "box64x32x48": 48}[gname]


MASKS = {"every_fourth": ML.mask_every_fourth, "whole_waves": ML.mask_whole_waves}


@pytest.mark.parametrize("cone", CONES)
@pytest.mark.parametrize("mname", list(MASKS))
@pytest.mark.parametrize("limit", [-1, 1, 9, 64])
@pytest.mark.parametrize("n", [4096, P17 + 1])
def test_limits_and_masks(cuda, oracle, monkeypatch, n, limit, mname, cone):
    """traverse_steps_limit and rays_mask through every launch path: a limit that stops a ray inside a staging row, at its
    end (64 = the longest row) and after one sample; masks that thin every wave and masks that empty whole waves."""
    sc = Scene(cuda, oracle, ML.batch(n, seed=31), "flipped128")
    mask = MASKS[mname](n)
    ref = reference(oracle, sc, ML.STEP, cone, limit=limit, mask=mask)
    assert ref.total > n // 4 and not ref.counts[~mask].any()
    if limit > 0:
        assert ref.counts.max() == limit and (ref.counts[mask] < limit).any()
    run_paths(monkeypatch, sc, ref, ML.STEP, cone, limit=limit, mask=mask)


# the 640 000-ray frame: (name, layout, grid, cone, switches, resume, coarse)
FRAME_CASES = [
    ("default", "bench", "ball128", 0.0, {}, True, True),                       # bench.py's own call: row 16, resumed, bitmap
    ("no_bitmap", "edges", "ball128", 0.0, {}, True, False),
    ("whole_ray", "edges", "ball128", 0.0, {}, False, True),                    # row 32
    ("row_8", "edges", "ball128", 0.0, {"CNC_PAIR_STAGE": "8"}, True, True),
    ("row_32", "edges", "ball128", 0.0, {"CNC_PAIR_STAGE": "32"}, True, True),
    ("row_64", "edges", "ball128", 0.0, {"CNC_PAIR_STAGE": "64"}, True, True),
    ("row_16_whole_ray", "edges", "ball128", 0.0, {"CNC_PAIR_STAGE": "16"}, False, False),
    ("cone", "edges", "ball128", 4e-3, {}, True, True),
    ("cone_whole_ray_no_bitmap", "edges", "ball128", 4e-3, {}, False, False),
    ("nested_default", "edges", "nested2x128", 0.0, {}, True, True),
    ("nested_row_64", "edges", "nested2x128", 0.0, {"CNC_PAIR_STAGE": "64"}, True, True),   # the largest LDS footprint
    ("nested_row_64_whole_ray", "edges", "nested2x128", 0.0, {"CNC_PAIR_STAGE": "64"}, False, True),
]


def _frame_layout(kind):
    return ML.frame() if kind == "bench" else ML.with_edges(ML.frame(ML.FAR_ESTIMATOR))


@pytest.mark.parametrize("case", FRAME_CASES, ids=[c[0] for c in FRAME_CASES])
def test_frame(cuda, oracle, monkeypatch, case):
    """The bench frame (800 x 800 rays, 68 M samples; far = inf as bench.py sets it, and far = 1e10 with the edge rays
    mixed in): the configuration bench.py and every evaluation frame run, and each switch flipped once."""
    name, kind, gname, cone, env, resume, coarse = case
    sc = Scene(cuda, oracle, _frame_layout(kind), gname)
    ref = reference(oracle, sc, ML.STEP, cone, key=(kind, gname, cone))
    assert sc.n == 640_000 and ref.total > 2e7
    if name == "default":
        assert ref.total == 68_022_266 and int(ref.counts.max()) == 406
    set_switches(monkeypatch, env)
    march(sc, ref, ML.STEP, cone, coarse=coarse, resume=resume, what=name)


def test_eval_loop(cuda, oracle):
    """render_image_with_occgrid_test's loop through cnc_march_samples_coarse at 2^17 + 1 rays: rounds of at most 64
    samples on the live rays, restarted from the previous round's termination planes, each round against the oracle's
    round fed the same planes; the rounds' counts sum to one unlimited march within the allowance of
    test_gpu_march.test_traverse_over_allocate_iterative (tests/test_march_layouts.py shows the oracle alone keeps it)."""
    sc = Scene(cuda, oracle, eval_loop_layout(), "ball128")
    full = reference(oracle, sc, ML.STEP, 0.0)
    full_counts = full.counts.copy()

    def one_round(mask, near, k):
        ref = reference(oracle, sc, ML.STEP, 0.0, limit=EVAL_LIMIT, mask=mask, near=near)
        march(sc, ref, ML.STEP, 0.0, limit=EVAL_LIMIT, mask=mask, near=near, coarse=True, resume=True, what=f"round {k}")
        if k % 2:
            march(sc, ref, ML.STEP, 0.0, limit=EVAL_LIMIT, mask=mask, near=near, coarse=False, resume=False, what=f"round {k}")
        return ref.counts, ref.term

    totals, rounds = eval_loop_rounds(one_round, EVAL_N, EVAL_LIMIT)
    diff = np.abs(totals - full_counts)
    assert rounds >= 6 and diff.max() <= 2 and (diff > 0).mean() < 0.05


# ----------------------------------------------------------------------------------------------------------------------
# cnc_traverse_grids: the nerfacc-boundary route
# ----------------------------------------------------------------------------------------------------------------------
def _segments(L, bufs):
    return L.RaySegments(*[_p(bufs.get(k)) for k in ("vals", "chunk_starts", "chunk_cnts", "ray_indices", "is_left",
                                                     "is_right", "is_valid")])


def _traverse(sc, step, cone, limit, first_pass, mask_d, iv, sm, term):
    from cnc_amd import _lib as L
    import ctypes
    lib, stream = _api()
    D = sc.D
    siv, ssm = _segments(L, iv), _segments(L, sm)
    rc = lib.cnc_traverse_grids(_p(D.o), _p(D.d), _p(mask_d), sc.n, _p(D.binaries), sc.levels, *sc.res, _p(D.aabbs),
                                _p(D.hits), _p(D.t_sorted), _p(D.t_indices), _p(D.near), _p(D.far), float(step), float(cone),
                                int(limit), int(first_pass), ctypes.byref(siv), ctypes.byref(ssm), _p(term), stream(sc.cuda))
    torch.cuda.synchronize()
    assert rc == 0


def _alloc(cuda, size, masks, valid):
    b = dict(vals=_poison(cuda, (size + PAD,), torch.float32), ray_indices=_poison(cuda, (size + PAD,), torch.int64))
    if masks:
        b["is_left"], b["is_right"] = (_poison(cuda, (size + PAD,), torch.uint8) for _ in range(2))
    if valid:
        b["is_valid"] = _poison(cuda, (size + PAD,), torch.uint8)
    return b


def _expect(cuda, want, written, dtype):
    """The oracle's array where a ray's march wrote, the poison everywhere else (and in the pad behind)."""
    out = _poison(cuda, (written.shape[0] + PAD,), dtype)
    idx = _dev(cuda, np.nonzero(written)[0])
    out[idx] = _dev(cuda, want[written]).to(dtype)
    return out


def _cmp_route(cuda, got, want, written, what):
    for k, buf in got.items():
        if k in ("chunk_cnts", "chunk_starts"):
            continue
        assert _same_bits(buf, _expect(cuda, np.asarray(want[k]), written, buf.dtype)), (what, k)


def _written(alloc_cnts, cnts):
    """Slots [start, start + count) of every ray among its allocated ones."""
    size = int(alloc_cnts.sum())
    starts = np.cumsum(alloc_cnts) - alloc_cnts
    within = np.arange(size) - np.repeat(starts, alloc_cnts)
    return within < np.repeat(cnts, alloc_cnts)


ROUTE_CASES = [
    # layout, grid, rays, step, cone, limit of the over-allocated pass
    ("frame", "ball128", 640_000, ML.STEP, 0.0, 9),
    ("frame", "nested2x128", 640_000, ML.STEP, 0.0, 64),
    ("frame", "nested4x64", 640_000, ML.STEP, 4e-3, 9),
    ("lengths", "full128", 640_000, ML.STEP, 0.0, 64),
    ("lengths", "full128", P17 + 1, ML.STEP, 4e-3, 9),
    ("batch", "nested2x128", P17 + 1, ML.STEP, 4e-3, 64),
    ("batch", "nested2x132", P17 + 1, ML.STEP, 0.0, 9),
    ("batch", "nested4x64", P17 + 1, ML.STEP, 0.0, 1),
    ("batch", "nested2x128", P17 + 1, 0.0, 0.0, 9),          # step_size = 0: one sample per occupied cell
    ("frame", "ball128", 640_000, 0.0, 0.0, 64),
]


@pytest.mark.parametrize("case", ROUTE_CASES, ids=["-".join(str(v) for v in c) for c in ROUTE_CASES])
def test_traverse_grids_route(cuda, oracle, case):
    """cnc_traverse_grids (k_traverse<0> counts, k_traverse<1> fills through flush_stage), two-pass and over-allocated with
    a mask: vals, is_left, is_right, is_valid, ray_indices and both count arrays equal the oracle's; no value, index or
    flag byte outside the slots the rays filled is written."""
    lname, gname, n, step, cone, limit = case
    if lname == "frame":
        lay = ML.with_edges(ML.frame(ML.FAR_ESTIMATOR))
    elif lname == "lengths":
        lay = ML.lengths(n)[0]
    else:
        lay = ML.batch(n, seed=37)
    sc = Scene(cuda, oracle, lay, gname)
    # two passes: count, allocate exactly, fill
    oiv, osm, oterm = oracle.traverse_grids(sc.o, sc.d, sc.binaries, sc.aabbs, sc.near, sc.far, step, cone, **sc.oracle_kw())
    iv, sm = dict(chunk_cnts=_poison(cuda, (n,), torch.int64)), dict(chunk_cnts=_poison(cuda, (n,), torch.int64))
    _traverse(sc, step, cone, -1, 1, None, iv, sm, None)
    assert np.array_equal(iv["chunk_cnts"].cpu().numpy(), oiv["chunk_cnts"])
    assert np.array_equal(sm["chunk_cnts"].cpu().numpy(), osm["chunk_cnts"])
    assert osm["chunk_cnts"].sum() > 10 * n
    for b, want in ((iv, oiv), (sm, osm)):
        b["chunk_starts"] = torch.cumsum(b["chunk_cnts"], 0) - b["chunk_cnts"]
        assert np.array_equal(b["chunk_starts"].cpu().numpy(), want["chunk_starts"])
    iv.update(_alloc(cuda, int(oiv["chunk_cnts"].sum()), True, False))
    sm.update(_alloc(cuda, int(osm["chunk_cnts"].sum()), False, True))
    term = _poison(cuda, (n,), torch.float32)
    _traverse(sc, step, cone, -1, 0, None, iv, sm, term)
    assert np.array_equal(iv["chunk_cnts"].cpu().numpy(), oiv["chunk_cnts"])
    assert np.array_equal(sm["chunk_cnts"].cpu().numpy(), osm["chunk_cnts"])
    _cmp_route(cuda, iv, oiv, np.ones(int(oiv["chunk_cnts"].sum()), bool), "two-pass intervals")
    _cmp_route(cuda, sm, osm, np.ones(int(osm["chunk_cnts"].sum()), bool), "two-pass samples")
    marched = osm["chunk_cnts"] > 0                               # _cmp_segments' rule; the others keep the poison
    got = term.cpu().numpy()
    assert np.array_equal(got[marched], oterm[marched]) and np.isnan(got[~(marched | (oiv["chunk_cnts"] > 0))]).all()
    del iv, sm
    # one pass into an upper-bound allocation, with a mask
    for mname, make in MASKS.items():
        mask = make(n)
        oiv, osm, oterm = oracle.traverse_grids(sc.o, sc.d, sc.binaries, sc.aabbs, sc.near, sc.far, step, cone,
                                                traverse_steps_limit=limit, over_allocate=True, rays_mask=mask,
                                                **sc.oracle_kw())
        a_iv, a_sm = (2 * limit) * mask.astype(np.int64), limit * mask.astype(np.int64)
        iv, sm = dict(chunk_cnts=_dev(cuda, a_iv)), dict(chunk_cnts=_dev(cuda, a_sm))
        iv["chunk_starts"], sm["chunk_starts"] = _dev(cuda, np.cumsum(a_iv) - a_iv), _dev(cuda, np.cumsum(a_sm) - a_sm)
        iv.update(_alloc(cuda, int(a_iv.sum()), True, False))
        sm.update(_alloc(cuda, int(a_sm.sum()), False, True))
        term = _poison(cuda, (n,), torch.float32)
        _traverse(sc, step, cone, limit, 0, _dev(cuda, mask.astype(np.uint8)), iv, sm, term)
        assert np.array_equal(iv["chunk_cnts"].cpu().numpy(), oiv["chunk_cnts"]), mname
        assert np.array_equal(sm["chunk_cnts"].cpu().numpy(), osm["chunk_cnts"]), mname
        assert not osm["chunk_cnts"][~mask].any() and osm["chunk_cnts"].max() == limit
        _cmp_route(cuda, iv, oiv, _written(a_iv, oiv["chunk_cnts"]), mname + " intervals")
        _cmp_route(cuda, sm, osm, _written(a_sm, osm["chunk_cnts"]), mname + " samples")
        got = term.cpu().numpy()
        assert np.array_equal(got[mask], oterm[mask]) and np.isnan(got[~mask]).all(), mname
        del iv, sm


# ----------------------------------------------------------------------------------------------------------------------
# the slab test and the coarse bitmap
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("near,far,miss", [(-np.inf, np.inf, np.inf), (0.5, 4.2, -1.0), (0.0, 1e10, 1e10), (-np.inf, 3.0, np.inf)])
def test_ray_aabb_at_frame_size(cuda, oracle, near, far, miss):
    """cnc_ray_aabb_intersect at 640 000 rays x 4 boxes, the edge rays among them: bit-equal to the oracle."""
    lib, stream = _api()
    o, d, _, _ = ML.with_edges(ML.frame())
    rng = np.random.default_rng(41)
    at = rng.choice(o.shape[0], size=64_000, replace=False)       # a tenth of the frame from other cameras: misses, origins
    bo, bd, _, _ = ML.batch(64_000, seed=43)                      # inside the larger boxes
    o[at], d[at] = bo, bd
    aabbs = np.concatenate([ML.level_boxes(3), np.array([[-0.2, -1.5, 0.1, 0.9, 0.3, 1.2]], np.float32)])
    n, m = o.shape[0], aabbs.shape[0]
    w0, w1, wh = oracle.ray_aabb_intersect(o, d, aabbs, near, far, miss)
    assert n == 640_000 and 0 < wh[:, 0].sum() < n and 0 < wh[:, 3].sum() < n
    od, dd, bd_ = _dev(cuda, o), _dev(cuda, d), _dev(cuda, aabbs)
    g0, g1 = (_poison(cuda, (n * m + PAD,), torch.float32) for _ in range(2))
    gh = _poison(cuda, (n * m + PAD,), torch.uint8)
    rc = lib.cnc_ray_aabb_intersect(_p(od), _p(dd), _p(bd_), n, m, float(near), float(far), float(miss), _p(g0), _p(g1),
                                    _p(gh), stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(gh[: n * m].cpu().numpy(), wh.reshape(-1).astype(np.uint8))
    assert np.array_equal(g0[: n * m].cpu().numpy(), w0.reshape(-1)) and np.array_equal(g1[: n * m].cpu().numpy(), w1.reshape(-1))
    assert _untouched(g0[n * m:]) and _untouched(g1[n * m:]) and _untouched(gh[n * m:])


def test_ray_aabb_behind_its_grid_cap(cuda, oracle):
    """k_ray_aabb launches at most 65535 blocks of 256 lanes (16,776,960 ray-box pairs) and walks on by the grid's width:
    70 000 rays x 240 boxes = 16,800,000 pairs, the last 23,040 of them on a lane's second trip.  Bit-equal to the oracle
    (on the MI355X: no element of hits, t_min or t_max differs); nothing written behind the pairs."""
    lib, stream = _api()
    n, m = 70_000, 240
    o, d, _, _ = ML.batch(n, seed=47)
    rng = np.random.default_rng(48)
    centre = rng.uniform(-1.2, 1.2, size=(m, 3))
    half = rng.uniform(0.05, 1.5, size=(m, 3))
    aabbs = np.concatenate([centre - half, centre + half], axis=1).astype(np.float32)
    assert n * m > 65535 * 256
    near, far, miss = 0.5, 4.2, -1.0
    w0, w1, wh = oracle.ray_aabb_intersect(o, d, aabbs, near, far, miss)
    behind = wh.reshape(-1)[65535 * 256:]
    assert 0 < behind.sum() < behind.size
    od, dd, bd_ = _dev(cuda, o), _dev(cuda, d), _dev(cuda, aabbs)
    g0, g1 = (_poison(cuda, (n * m + PAD,), torch.float32) for _ in range(2))
    gh = _poison(cuda, (n * m + PAD,), torch.uint8)
    rc = lib.cnc_ray_aabb_intersect(_p(od), _p(dd), _p(bd_), n, m, float(near), float(far), float(miss), _p(g0), _p(g1),
                                    _p(gh), stream(cuda))
    torch.cuda.synchronize()
    assert rc == 0
    wrong = [int((got[: n * m].cpu().numpy() != want.reshape(-1)).sum())
             for got, want in ((gh, wh.astype(np.uint8)), (g0, w0), (g1, w1))]
    print(f"ray_aabb {n} x {m}: elements that differ from the oracle (hits, t_min, t_max): {wrong}")
    assert wrong == [0, 0, 0]
    assert _untouched(g0[n * m:]) and _untouched(g1[n * m:]) and _untouched(gh[n * m:])


@pytest.mark.parametrize("gname", ["ball128", "flipped128", "full128", "nested2x128", "nested4x64", "box64x32x48", "nested2x132"])
def test_coarse_bits(cuda, gname):
    """cnc_occupancy_coarse_bits against NumPy's `any` over the 4 x 4 x 4 blocks; CNC_ERR_UNSUPPORTED, and nothing written,
    for the 132^3 pair (2 247 words)."""
    lib, stream = _api()
    binaries, _ = ML.grid(gname)
    want = ML.coarse_words(binaries)
    shape = [int(v) for v in binaries.shape]
    b = _dev(cuda, binaries.astype(np.uint8))
    words = _poison(cuda, (want.size + PAD,), torch.int32)
    rc = lib.cnc_occupancy_coarse_bits(_p(b), *shape, _p(words), stream(cuda))
    torch.cuda.synchronize()
    nw = int(lib.cnc_occupancy_coarse_words(*shape))
    if gname == "nested2x132":
        assert want.size == 2247 and nw == 0 and rc == CNC_ERR_UNSUPPORTED and _untouched(words)
        return
    assert rc == 0 and nw == want.size
    assert np.array_equal(words[:nw].cpu().numpy().view(np.uint32), want) and _untouched(words[nw:])
    if gname not in ("full128",):
        assert 0 < np.unpackbits(want.view(np.uint8)).sum() < 32 * want.size
