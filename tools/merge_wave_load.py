#!/usr/bin/env python3
"""How phase B of k_grid_encode_bwd_merge (grid_encode_merge.hip) loads the 16 waves of a block: a CPU model on the bench
frame's own samples, and the numpy twin of the rule that lays a block's samples out by cell and cuts them into work units.

    python tools/merge_wave_load.py [--cap 512] [--handout dynamic] [--windows 12]

No GPU: the bench's rays are marched with the oracle (oracle.traverse_grids), the tiles come from tools/merge_tiles.py (the
restatement of k_merge_tile_order), the units from `split_units` below.  Per level of the ten coarse ones and per chunk
(first, quarter-way, middle) it prints, for the walk before the units and for the units of --cap / --handout,

    held      sum over blocks of the busiest wave's cost: how long phase B keeps the block's LDS and wave slots
    balanced  the same work spread evenly over the waves: the work itself
    flushes   units - cells, in % of the cells: the sets of atomics the cap adds

Before: one wave walks a cell's chain of runs, cell g goes to wave g % 16; 60 + per run pair (25 + 20 * ceil(longer run
/ 4)), about the static instruction counts per cell, pair and step (profiles/r17_backward_issue_slots.md).  Now: a cell's
samples lie side by side, 60 + 20 per step of eight.  The constants are approximations: the table says where the work and
the imbalance are, not what the clock will show (profiles/r18_merge_wave_balance.md has what it showed).

`split_units` follows the kernel operation by operation (hash probe for the cell, add on the cell's sample count, the
cells' add on the block's packed place | unit counter), one generator per run that yields before every LDS atomic, so that a
caller can interleave the runs of a block in any order the hardware could: tests/test_merge_units.py.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_WAVES = 16


def cell_keys(x, R):
    """Cell key per sample on a level of resolution R (the float32 arithmetic of Corners::setup), -1 outside [0, 1]."""
    x = np.asarray(x, np.float32)
    p = x * np.float32(R - 2) + np.float32(0.5)
    c = np.floor(p).astype(np.int64)
    key = c[:, 0] | c[:, 1] << 16 | c[:, 2] << 32
    return np.where(((x < 0) | (x > 1)).any(axis=1) | ~np.isfinite(x).all(axis=1), -1, key)


def split_units(keys, cap, rng=None):
    """The work units of one block.  keys: int64 per thread of the block (-1: no sample, the kernel's key ~0);
    cap: CNC_MERGE_UNIT_CAP; rng: None = the runs and cells arrive one after the other in sample order, else a numpy
    Generator that decides which run does its next LDS atomic, and in which order the cells take their places.

    Returns (units, place): units = list of {"key", "lo", "hi"}, the places [lo, hi) of s_w4 / s_g the unit sums, in
    the order of the unit records; place[t] = where thread t's sample goes, -1 for a sample without a cell."""
    keys = np.asarray(keys, np.int64)
    MB = len(keys)
    n_slots = 1024 if MB <= 512 else 2048
    shift = 32 - (n_slots.bit_length() - 1)
    assert cap >= 8 and cap % 8 == 0
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    run_start = np.r_[heads, MB].tolist()
    n_runs = len(heads)
    kl = keys.tolist()
    h_slot = [0] * n_slots
    cell_n = [0] * MB
    run_rec = [None] * n_runs                               # (representative run, place in the cell, first thread)
    claimers = []

    def thread(r):
        tid, end = run_start[r], run_start[r + 1]
        key = kl[tid]
        sl = ((key ^ key >> 16 ^ key >> 32) * 2654435761 & 0xFFFFFFFF) >> shift
        while True:
            yield
            seen = h_slot[sl]
            if seen == 0:
                h_slot[sl] = r + 1
                claimers.append(r)
                rep = r
                break
            rep = seen - 1
            if kl[run_start[rep]] == key:
                break
            sl = (sl + 1) & (n_slots - 1)
        yield
        run_rec[r] = (rep, cell_n[rep], tid)
        cell_n[rep] += end - tid

    live = []
    for r in range(n_runs):
        if kl[run_start[r]] < 0:
            continue
        t = thread(r)
        if rng is None:
            for _ in t:
                pass
        else:
            live.append(t)
    while live:
        i = int(rng.integers(len(live)))
        try:
            next(live[i])
        except StopIteration:
            live[i] = live[-1]
            live.pop()

    units, placed = [], 0
    for r in (sorted(claimers) if rng is None else rng.permutation(claimers).tolist()):
        n, first = cell_n[r], placed
        placed += n
        cell_n[r] = first
        for p in range(first, first + n, cap):
            units.append({"key": kl[run_start[r]], "lo": p, "hi": min(p + cap, first + n)})
    place = np.full(MB, -1, np.int64)
    for r in range(n_runs):
        if run_rec[r] is not None:
            rep, at, tid = run_rec[r]
            n = run_start[r + 1] - tid
            place[tid:tid + n] = cell_n[rep] + at + np.arange(n)
    return units, place


def chains_before(keys):
    """The chains of the walk before the units (one wave per cell, runs taken in pairs, newest first): per cell the list
    of its runs (start, end)."""
    keys = np.asarray(keys, np.int64)
    heads = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    ends = np.r_[heads[1:], len(keys)]
    chains = {}
    for h, e in zip(heads.tolist(), ends.tolist()):
        if keys[h] >= 0:
            chains.setdefault(int(keys[h]), []).insert(0, (h, e))
    return list(chains.values())


def chain_cost(runs):
    """The walk before the units: 60 + per run pair (25 + 20 * ceil(longer run / 4)); the last run of an odd chain is
    split in two halves (the first half rounded up to whole steps)."""
    cost = 60
    for i in range(0, len(runs), 2):
        a = runs[i][1] - runs[i][0]
        if i + 1 < len(runs):
            b = runs[i + 1][1] - runs[i + 1][0]
        else:
            first = min(a, (((a + 1) >> 1) + 3) & ~3)
            a, b = first, a - first
        cost += 25 + 20 * -(-max(a, b) // 4)
    return cost


def unit_cost(n):
    """A unit of n samples that lie side by side: 60 + 20 per step of eight."""
    return 60 + 20 * -(-n // 8)


def held(costs, handout):
    """The busiest wave's cost: unit g to wave g % 16, or the next unit to the first free wave."""
    if not costs:
        return 0
    if handout == "static":
        return max(sum(costs[w::N_WAVES]) for w in range(N_WAVES))
    busy = [0] * N_WAVES
    for c in costs:
        w = busy.index(min(busy))
        busy[w] += c
    return max(busy)


def block_load(keys, cap, handout):
    """(held, balanced, units, cells) of one block under the units; cap None: the walk before them."""
    if cap is None:
        costs = [chain_cost(c) for c in chains_before(keys)]
        return held(costs, "static"), sum(costs) / N_WAVES, len(costs), len(costs)
    units, _ = split_units(keys, cap)
    costs = [unit_cost(u["hi"] - u["lo"]) for u in units]
    return held(costs, handout), sum(costs) / N_WAVES, len(units), len({u["key"] for u in units})


def march_bench_chunks(which, chunk, windows, window):
    """Positions (unit cube, float32) of `windows` evenly spaced windows of the bench frame's chunks `which` (fractions
    of the frame's sample stream): {fraction: [(first sample of the window, x [window, 3]), ...]}."""
    import torch

    import oracle
    from cnc_amd import synthetic
    aabb = (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5)
    binaries = synthetic.ball_binaries(128, aabb, 1.0).numpy()
    aabbs = np.asarray([aabb], np.float32)
    o, d = synthetic.pinhole_rays(800, 800, 0.6911, 4.0, azimuth=0.7, elevation=0.5)
    o, d = o.numpy().astype(np.float32), d.numpy().astype(np.float32)
    rows = 40 * 800
    counts = []
    for r0 in range(0, o.shape[0], rows):
        _, sm, _ = oracle.traverse_grids(o[r0:r0 + rows], d[r0:r0 + rows], binaries, aabbs, step_size=5e-3)
        counts.append(sm["chunk_cnts"])
    counts = np.concatenate(counts)
    first = np.cumsum(counts) - counts
    total = int(counts.sum())
    n_chunks = total // chunk
    out = {}
    for frac in which:
        c0 = int(frac * n_chunks) * chunk
        wins = []
        for w in np.linspace(0, chunk // window - 1, windows).astype(int):
            s0 = c0 + int(w) * window
            r0 = int(np.searchsorted(first, s0, side="right")) - 1
            r1 = int(np.searchsorted(first, s0 + window, side="left"))
            _, sm, _ = oracle.traverse_grids(o[r0:r1], d[r0:r1], binaries, aabbs, step_size=5e-3)
            t = sm["vals"][:, None]
            ray = sm["ray_indices"]
            p = (o[r0:r1][ray] + d[r0:r1][ray] * t - np.float32(-1.5)) / np.float32(3.0)
            at = s0 - int(first[r0])
            wins.append((s0, p[at:at + window].astype(np.float32)))
        out[frac] = wins
    return out, total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cap", type=int, default=512, help="CNC_MERGE_UNIT_CAP (a multiple of 8)")
    ap.add_argument("--handout", choices=["static", "dynamic"], default="dynamic")
    ap.add_argument("--windows", type=int, default=12, help="windows of 8,192 samples taken from each chunk")
    ap.add_argument("--min-res", type=int, default=None, help="CNC_MERGE_TILE_MIN_RES (default: tools/merge_tiles.MIN_RES)")
    args = ap.parse_args()
    import torch

    from cnc_amd import synthetic
    from tools import merge_tiles
    W, S, MB, chunk = 8192, 8, 1024, 1 << 20
    min_res = merge_tiles.MIN_RES if args.min_res is None else args.min_res
    levels = synthetic.RES_16L[:10]
    chunks, total = march_bench_chunks([0.0, 0.25, 0.5], chunk, args.windows, W)
    print(f"frame: {total:,} samples; cap {args.cap}, hand-out {args.handout}, tiles from R >= {min_res}, "
          f"{args.windows} windows of {W:,} per chunk")
    for frac, wins in chunks.items():
        print(f"\nchunk at {frac:.2f} of the frame")
        print("|   R | held, before | work, before | held / work | held, now | work, now | held now / before | cells | units | added flushes |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        tot = np.zeros(6)
        for R in levels:
            row = np.zeros(6)
            for s0, x in wins:
                keys = cell_keys(x, R)
                if R >= min_res:
                    order, _ = merge_tiles.window_order(torch.from_numpy(x), 0, x.shape[0], W, S, MB)
                    idx = (order.numpy()[:, None] * S + np.arange(S)[None, :]).reshape(-1)
                    keys = np.where(idx < x.shape[0], keys[np.minimum(idx, x.shape[0] - 1)], -1)
                for b0 in range(0, len(keys), MB):
                    k = keys[b0:b0 + MB]
                    h0, bal0, _, cells = block_load(k, None, "static")
                    h1, bal1, units, _ = block_load(k, args.cap, args.handout)
                    row += (h0, bal0, h1, bal1, cells, units)
            tot += row
            for name, r in ((f"{R:3d}", row),) + ((("sum", tot),) if R == levels[-1] else ()):
                print(f"| {name} | {r[0] / 1e3:.1f} k | {r[1] / 1e3:.1f} k | {r[0] / r[1]:.2f} | {r[2] / 1e3:.1f} k | {r[3] / 1e3:.1f} k | "
                      f"{r[2] / r[0]:.3f} | {int(r[4]):,} | {int(r[5]):,} | {100 * (r[5] - r[4]) / r[4]:.2f} % |")


if __name__ == "__main__":
    main()
