"""The depth-ranked sample tiles of k_grid_encode_bwd_merge (grid_encode_merge.hip, k_merge_tile_order) against the
oracle's float64 sums: the coarse call (cnc_grid_encode_backward with CNC_FLAG_LEVELS_FINEST_FIRST) and the overlapped
entry, new tiling and CNC_FLAG_MERGE_CONSECUTIVE, STE on (with clipped rows) and off.  Every table entry must lie within
the float32 summation bound (n_e + 2) * eps * sum|terms| of the float64 sum (tests/test_gpu_binned_backward.py), and the two
tilings within twice that bound of each other.  A sample the tiling drops or takes twice is far outside that bound.

The tiles serve the 1,024-thread form of the kernel only, which a call gets from 4,096 (block, level) pairs on: the small
sample counts come with as many (small) levels as that takes.  The segment order needs scratch, which the overlapped
entry asks for (below N = 2^16 it hands call and scratch to the serial binned entry): `_overlapped` checks the order the
library left there against tools/merge_tiles.py, so every size below really runs the tiled kernel.  The coarse call has no
scratch and keeps consecutive samples under either flag value (checked all the same: the flag must not change it)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import make_grid

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float32).eps
# log2_T = 10: dense levels of 64 ... 512 rows and hashed ones of 1,024; every other one is fine enough for the ranked
# tiles (kMergeTileMinRes = 52: the coarser ones keep consecutive samples under either setting)
RES_CYCLE = [4, 64, 6, 120, 31, 52, 8, 83]
RES_BINNED = 44                              # the one level the overlapped entry bins (1,024 rows)


def _levels_for(N):
    """Coarse levels that put a call of N samples on the 1,024-thread form (launch_bwd_merge: not `small`)."""
    blocks = -(-N // 1024)
    return max(10, -(-4096 // blocks))


def _coarse(dev, g, x, emb, offs, res, L, ste, consecutive, clip=None):
    """cnc_grid_encode_backward on the first L levels of a level-major gradient, as the binned entries call it."""
    from cnc_amd import _lib
    ge = torch.zeros_like(emb)
    flags = _lib.CNC_FLAG_LEVELS_FINEST_FIRST | (_lib.CNC_FLAG_STE_BINARY if ste else 0) \
        | (_lib.CNC_FLAG_MERGE_CONSECUTIVE if consecutive else 0)
    rc = _lib.lib().cnc_grid_encode_backward(
        g.data_ptr(), x.data_ptr(), emb.data_ptr(), offs.data_ptr(), res.data_ptr(), ge.data_ptr(), x.shape[0], 3, 8, L,
        128, None, None, None, None, flags, _lib.ptr(clip), None, None, None, 0, 0, _lib.stream())
    _lib.check(rc, "grid_encode_backward")
    torch.cuda.synchronize()
    return ge.cpu().numpy()


W, S = 8192, 8                               # kMergeTileWindow, kMergeTileSegment
POISON = 0xAB


def _overlapped(dev, g, x, emb, offs, res, L, n_binned, level_rows, ste, consecutive, clip=None):
    """The overlapped entry with exactly the workspace it asks for, poisoned.  The tail of that workspace is where the
    library keeps the segment order of the depth-ranked tiles (k_merge_tile_order: 2 bytes per segment, W / S segments per
    window): with the new tiling every window's entries must be what tools/merge_tiles.window_order gives — the kernel's
    rule and its torch restatement agree, and the tiled path really ran — and with CNC_FLAG_MERGE_CONSECUTIVE the tail must
    come back untouched."""
    from cnc_amd import _lib
    from cnc_amd.backends import gridencoder_backend as be
    from tools import merge_tiles
    lib = _lib.lib()
    N = x.shape[0]
    ge = torch.zeros_like(emb)
    flags = (_lib.CNC_FLAG_STE_BINARY if ste else 0) | (_lib.CNC_FLAG_MERGE_CONSECUTIVE if consecutive else 0)
    nbytes = int(lib.cnc_grid_encode_backward_overlapped_workspace(N, n_binned, level_rows))
    order_bytes = -(-N // W) * (W // S) * 2
    assert nbytes % 256 == 0 and nbytes > order_bytes
    ws = torch.full((nbytes,), POISON, dtype=torch.uint8, device=dev)
    cur = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.cnc_grid_encode_backward_overlapped(
        be._plan(dev, cur), g.data_ptr(), x.data_ptr(), emb.data_ptr(), offs.data_ptr(), res.data_ptr(), ge.data_ptr(), N, 3, 8,
        L, flags, _lib.ptr(clip), 0, 0, n_binned, level_rows, ws.data_ptr(), nbytes, _lib.stream())
    _lib.check(rc, "grid_encode_backward_overlapped")
    torch.cuda.synchronize()
    tail = ws[nbytes - order_bytes:].cpu()
    if consecutive:
        assert bool((tail == POISON).all()), "CNC_FLAG_MERGE_CONSECUTIVE: the order scratch must stay untouched"
    else:
        got = tail.view(torch.int16).to(torch.int64).reshape(-1, W // S) & 0xFFFF
        xc = x.cpu()
        for w in range(got.shape[0]):
            assert torch.equal(torch.sort(got[w]).values, torch.arange(W // S)), f"window {w}: not a permutation"
            want, _ = merge_tiles.window_order(xc, w * W, N, W, S)
            assert torch.equal(got[w], want), f"window {w}: the kernel's order differs from tools/merge_tiles.py"
    return ge.cpu().numpy()


def _check(name, got, acc64, bound, rows=None, ignore=None):
    sl = slice(None) if rows is None else slice(0, rows)
    ratio = np.abs(got[sl].astype(np.float64) - acc64[sl]) / bound[sl]
    if ignore is not None:
        ratio = np.where(ignore[sl], 0.0, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name}: worst entry {worst:.3f} x its bound")
    assert worst <= 1.0, f"{name}: worst entry {worst:.3f} x its bound"      # (a NaN fails it too)


def _run_case(cuda, oracle, x, L_coarse, seed, poisoned=None):
    """Both entries, both tilings, STE on and off, on the points x (numpy [N, 3]) with L_coarse small coarse levels and one
    binned level behind them.  poisoned: samples with a NaN coordinate — the float64 reference leaves them out, the rows
    the kernel makes NaN for them (the one valid vertex of cell 0 per level) must be the same in both tilings and are not
    compared."""
    import np_twins as tw
    N = x.shape[0]
    assert -(-N // 1024) * L_coarse >= 4096                 # the 1,024-thread form
    res = [RES_CYCLE[i % len(RES_CYCLE)] for i in range(L_coarse)] + [RES_BINNED]
    L = len(res)
    offs, resl, emb = make_grid(res, 10, 3, 8, seed=seed)
    g = np.random.default_rng(seed + 1).normal(size=(L, N, 8)).astype(np.float32)
    keep = np.ones(N, bool) if poisoned is None else ~poisoned
    xo, go = x[keep], np.ascontiguousarray(g[:, keep])
    n_e = tw.grid_entry_counts(xo, offs, resl)
    t = lambda a: torch.as_tensor(a, device=cuda)
    xd, gd, ed, od, rd = t(x), t(g), t(emb), t(offs), t(resl)
    coarse_rows = int(offs[L_coarse])
    for ste in (False, True):
        assert not ste or (np.abs(emb) > 1).any()
        _, acc64 = oracle.grid_encode_backward(go, xo, emb, offs, resl, ste_binary=ste, want_acc64=True)
        _, abs64 = oracle.grid_encode_backward(np.abs(go), xo, emb, offs, resl, ste_binary=ste, want_acc64=True)
        bound = (n_e[:, None] + 2) * EPS * abs64 + 1e-30
        outs = {}
        for cons in (False, True):
            outs["coarse", cons] = _coarse(cuda, gd, xd, ed, od, rd, L_coarse, ste, cons)
            outs["overlapped", cons] = _overlapped(cuda, gd, xd, ed, od, rd, L, 1, 1024, ste, cons)
        ignore = None
        if poisoned is not None:
            # what the consecutive tiling makes NaN: the coarse levels from the coarse call, the binned level from the other
            ignore = np.isnan(outs["coarse", True])
            ignore[coarse_rows:] = np.isnan(outs["overlapped", True][coarse_rows:])
            assert ignore.any(axis=1).sum() <= L, "the poisoned samples share one cell: one valid vertex row per level"
            for k, o in outs.items():
                rows = coarse_rows if k[0] == "coarse" else emb.shape[0]
                assert np.array_equal(np.isnan(o[:rows]), ignore[:rows]), k
                o[:rows][ignore[:rows]] = 0.0
            acc64 = np.where(ignore, 0.0, acc64)
        for (entry, cons), o in outs.items():
            rows = coarse_rows if entry == "coarse" else None
            _check(f"N={N} L={L_coarse} ste={ste} {entry} consecutive={cons}", o, acc64, bound, rows, ignore)
            if entry == "coarse":
                assert np.all(o[coarse_rows:] == 0)
            if ste:
                assert np.all(o[np.abs(emb) > 1] == 0)
            assert np.all(o[(abs64 == 0) & (True if ignore is None else ~ignore)] == 0)
            assert np.isfinite(o).all()
        for entry in ("coarse", "overlapped"):
            d = np.abs(outs[entry, False].astype(np.float64) - outs[entry, True])
            assert np.all(d <= 2 * bound), f"{entry}: the tilings differ by {np.max(d / bound):.3f} x the bound"


def _ray_points(N, seed, n_samples=200):
    """Neighbouring parallel rays across the cube, `n_samples` samples each."""
    rng = np.random.default_rng(seed)
    n_rays = -(-N // n_samples)
    d = np.array([0.62, 0.33, 0.71])
    d /= np.linalg.norm(d)
    side = np.cross(d, [0.0, 0.0, 1.0])
    side /= np.linalg.norm(side)
    o = np.array([0.07, 0.31, 0.05]) + side[None, :] * (0.4 / max(n_rays, 1)) * np.arange(n_rays)[:, None]
    tt = (0.9 / n_samples) * (np.arange(n_samples)[None, :] + rng.uniform(0, 1, size=(n_rays, 1)))
    return (o[:, None, :] + d[None, None, :] * tt[:, :, None]).reshape(-1, 3)[:N].astype(np.float32)


@pytest.mark.parametrize("N", [1, 7, 1023, 8191, 8192, 8193, 70001])
def test_ragged_sizes(cuda, oracle, N):
    _run_case(cuda, oracle, _ray_points(N, seed=N), _levels_for(N), seed=100 + N % 97)


@pytest.mark.parametrize("name", ["one_position", "plane_across_axis", "zero_axis", "outside_and_nan", "shuffled_rays"])
def test_degenerate_depths(cuda, oracle, name):
    N = 70001
    x = _ray_points(N, seed=7)
    poisoned = None
    if name == "one_position":
        x[:] = np.array([0.3, 0.4, 0.55], np.float32)
    elif name == "plane_across_axis":
        # the axis candidates step along x0, every other sample has the same x0: all depths tie exactly
        x = np.random.default_rng(8).uniform(0.02, 0.98, size=(N, 3)).astype(np.float32)
        x[:, 0] = 0.5
        x[:24, 0] = 0.1 + 0.01 * np.arange(24, dtype=np.float32)
        x[:24, 1:] = 0.5
    elif name == "zero_axis":
        x[:32] = x[0]
    elif name == "outside_and_nan":
        x[4::7] += 2.0                       # midpoints (sample 4 of a segment of 8) and others outside the cube
        poisoned = np.zeros(N, bool)
        poisoned[12::640] = True             # midpoints
        poisoned[1] = True                   # an axis candidate
        x[poisoned] = np.nan                 # (all three: cell 0 of every level, whose one valid vertex row turns NaN)
    elif name == "shuffled_rays":
        x = x[np.random.default_rng(9).permutation(N)]
    _run_case(cuda, oracle, x, _levels_for(N), seed=11, poisoned=poisoned)


@pytest.mark.parametrize("which", ["middle", "first", "middle_shuffled"])
def test_bench_chunks_ten_and_eleven_coarse_levels(cuda, oracle, which):
    """The bench's own call (16L x 2^19 x F8, raw table, clip count) on its middle and first chunk, and on the middle chunk
    shuffled: the plan's ten coarse levels and eleven (five binned), both entries, both tilings, STE on and off."""
    import bench
    import np_twins as tw
    from cnc_amd.backends import gridencoder_backend as be
    w = bench.build_workload(cuda, 0)
    box = {}
    bench.march_frame(w, box)
    pos = box["ex"]["positions"]
    S, N, L = pos.shape[0], bench.CHUNK, bench.L
    c = 0 if which == "first" else (S // N) // 2
    xs = pos[c * N:(c + 1) * N].contiguous()
    if which == "middle_shuffled":
        xs = xs[torch.randperm(N, device=cuda, generator=torch.Generator(device=cuda).manual_seed(3))].contiguous()
    plan = be.plan_binned_levels(bench.synthetic.RES_16L, w["offsets_host"], 3, 8, N)
    assert plan is not None and L - plan[0] == 10
    g = torch.randn((L, N, 8), device=cuda, generator=torch.Generator(device=cuda).manual_seed(4))
    xn, gn, table = xs.cpu().numpy(), g.cpu().numpy(), w["table"].cpu().numpy()
    offs, res = w["offsets"].cpu().numpy(), w["resolutions"].cpu().numpy()
    n_e = tw.grid_entry_counts(xn, offs, res)
    threads = oracle.max_threads()
    for ste in (True, False):
        _, acc64 = oracle.grid_encode_backward(gn, xn, table, offs, res, ste_binary=ste, want_acc64=True, threads=threads)
        _, abs64 = oracle.grid_encode_backward(np.abs(gn), xn, table, offs, res, ste_binary=ste, want_acc64=True,
                                               threads=threads)
        bound = (n_e[:, None] + 2) * EPS * abs64 + 1e-30
        clip = w["clip"] if ste else None
        for Lc in (10, 11):
            rows = int(offs[Lc])
            outs = {}
            for cons in (False, True):
                outs["coarse", cons] = _coarse(cuda, g, xs, w["table"], w["offsets"], w["resolutions"], Lc, ste, cons, clip)
                outs["overlapped", cons] = _overlapped(cuda, g, xs, w["table"], w["offsets"], w["resolutions"], L, L - Lc,
                                                       plan[1], ste, cons, clip)
            for (entry, cons), o in outs.items():
                _check(f"{which} coarse levels {Lc} ste={ste} {entry} consecutive={cons}", o, acc64, bound,
                       rows if entry == "coarse" else None)
                assert np.all(o[abs64 == 0] == 0)
            for entry in ("coarse", "overlapped"):
                r = rows if entry == "coarse" else table.shape[0]
                d = np.abs(outs[entry, False][:r].astype(np.float64) - outs[entry, True][:r])
                assert np.all(d <= 2 * bound[:r]), f"{entry}: the tilings differ by {np.max(d / bound[:r]):.3f} x the bound"
