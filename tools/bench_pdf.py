#!/usr/bin/env python3
"""Proposal-sampling kernels (cnc_amd/csrc/pdf.hip) against a plain-torch restatement on the same GPU.

    python tools/bench_pdf.py [--reps 20] [--json out.jsonl]

Importance sampling on nerfacc's mip-NeRF 360 schedule (props 256 -> 96 -> final 48: (E, n) = (2, 256), (257, 96),
(97, 48)) for 4096 / 65536 / 262144 rays, batched (int n) and packed (per-ray n drawn from [0, 2n], flattened in
and out; the call includes its one host read of the totals); searchsorted as _pdf_loss calls it, a (n_rays, 49)
query against (n_rays, 257) and (n_rays, 97) keys.  Milliseconds per call (median of --reps timed windows of 10
calls each, device events), and the bytes a call must move over that time against the 8 TB/s HBM peak."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cnc_amd.backends import nerfacc_cuda as C  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps, inner=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    times.sort()
    return times[len(times) // 2]


def spec(vals, starts=None, cnts=None):
    s = C.RaySegmentsSpec()
    s.vals, s.chunk_starts, s.chunk_cnts = vals, starts, cnts
    return s


def torch_sampling_batched(vals, cdfs, n, bias):
    """The reference's two kernels restated in torch ops for rows of E edges."""
    R, E = vals.shape
    floor, ceil = cdfs[:, :1], cdfs[:, -1:]
    step = (ceil - floor) / n
    u = (torch.arange(n, device=vals.device, dtype=torch.float32)[None, :] + bias[:, None]) * step + floor
    p = torch.searchsorted(cdfs[:, :-1].contiguous(), u, right=True)
    p0, p1 = (p - 1).clamp(0, E - 1), p.clamp(0, E - 1)
    c0, c1, v0, v1 = cdfs.gather(1, p0), cdfs.gather(1, p1), vals.gather(1, p0), vals.gather(1, p1)
    dc = c1 - c0
    t = torch.where(dc < 1e-10, (v0 + v1) * 0.5, (u - c0) * ((v1 - v0) / dc) + v0)
    mid = (t[:, 1:] + t[:, :-1]) * 0.5
    first = torch.maximum(t[:, :1] - (t[:, 1:2] - t[:, :1]) * 0.5, vals[:, :1])
    last = torch.minimum(t[:, -1:] + (t[:, -1:] - t[:, -2:-1]) * 0.5, vals[:, -1:])
    return t, torch.cat([first, mid, last], 1)


def torch_sampling_packed(vals, cdfs, counts, bias):
    """Packed outputs in torch: the padded (R, max n) grid, masked, then flattened with ray ids and edge flags."""
    R, E = vals.shape
    nmax = int(counts.max().item())
    k = torch.arange(nmax, device=vals.device)[None, :]
    nf = counts.clamp_min(1).to(torch.float32)[:, None]
    step = (cdfs[:, -1:] - cdfs[:, :1]) / nf
    u = (k.to(torch.float32) + bias[:, None]) * step + cdfs[:, :1]
    p = torch.searchsorted(cdfs[:, :-1].contiguous(), u, right=True)
    p0, p1 = (p - 1).clamp(0, E - 1), p.clamp(0, E - 1)
    c0, c1, v0, v1 = cdfs.gather(1, p0), cdfs.gather(1, p1), vals.gather(1, p0), vals.gather(1, p1)
    dc = c1 - c0
    t = torch.where(dc < 1e-10, (v0 + v1) * 0.5, (u - c0) * ((v1 - v0) / dc) + v0)
    live = k < counts[:, None]
    prev = torch.cat([t[:, :1], t[:, :-1]], 1)
    nxt = torch.cat([t[:, 1:], t[:, -1:]], 1)
    inner = (t + prev) * 0.5
    e0 = torch.maximum(t - (nxt - t) * 0.5, vals[:, :1])
    e0 = torch.where(counts[:, None] == 1, vals[:, :1], e0)
    edges = torch.where(k == 0, e0, inner)
    el = torch.minimum(t + (t - prev) * 0.5, vals[:, -1:])
    el = torch.where(counts[:, None] == 1, vals[:, -1:], el)
    is_last = k == counts[:, None] - 1
    lastcol = (el * is_last).sum(1, keepdim=True)
    kk = torch.arange(nmax + 1, device=vals.device)[None, :]
    e_full = torch.cat([edges, torch.zeros_like(edges[:, :1])], 1)
    e_full = torch.where(kk == counts[:, None], lastcol, e_full)
    e_live = (kk <= counts[:, None]) & (counts[:, None] > 0)
    rays = torch.arange(R, device=vals.device)[:, None]
    samples = t[live]
    s_ri = rays.expand(R, nmax)[live]
    edge_vals = e_full[e_live]
    e_ri = rays.expand(R, nmax + 1)[e_live]
    is_left = (kk < counts[:, None]).expand(R, nmax + 1)[e_live]
    is_right = (kk > 0).expand(R, nmax + 1)[e_live]
    return samples, s_ri, edge_vals, e_ri, is_left, is_right


def rows(R, E, dev, g):
    vals = torch.sort(torch.rand(R, E, device=dev, generator=g) * 10, 1).values.contiguous()
    cdfs = torch.sort(torch.rand(R, E, device=dev, generator=g), 1).values
    cdfs = torch.cat([torch.zeros_like(cdfs[:, :1]), cdfs[:, 1:-1], torch.ones_like(cdfs[:, :1])], 1).contiguous() \
        if E > 1 else cdfs.contiguous()
    return vals, cdfs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = []

    def emit(**r):
        r["hip_GBps"] = r["bytes"] / (r["hip_ms"] * 1e-3) / 1e9
        r["torch_GBps"] = r["bytes"] / (r["torch_ms"] * 1e-3) / 1e9
        r["hip_peak_frac"] = r["bytes"] / (r["hip_ms"] * 1e-3) / PEAK
        r["speedup"] = r["torch_ms"] / r["hip_ms"]
        out.append(r)
        print(json.dumps(r), flush=True)

    for E, n in ((2, 256), (257, 96), (97, 48)):
        for R in (4096, 65536, 262144):
            vals, cdfs = rows(R, E, dev, g)
            bias = torch.full((R,), 0.5, device=dev)
            seg = spec(vals)
            hip = lambda: C.importance_sampling(seg, cdfs, n, False)        # noqa: E731
            ref = lambda: torch_sampling_batched(vals, cdfs, n, bias)       # noqa: E731
            iv, sm = hip()
            t, e = ref()
            diff = max((sm.vals - t).abs().max().item(), (iv.vals - e).abs().max().item())
            nbytes = R * E * 8 + R * n * 4 + R * (n + 1) * 4
            emit(op="importance_sampling", layout="batched", E=E, n=n, n_rays=R, bytes=nbytes,
                 hip_ms=timed(hip, a.reps), torch_ms=timed(ref, a.reps), max_abs_diff=diff)

            counts = torch.randint(0, 2 * n + 1, (R,), device=dev, generator=g)
            starts = torch.arange(R, device=dev, dtype=torch.int64) * E
            pseg = spec(vals.view(-1), starts, torch.full((R,), E, device=dev, dtype=torch.int64))
            hip_p = lambda: C.importance_sampling(pseg, cdfs.view(-1), counts, False)   # noqa: E731
            ref_p = lambda: torch_sampling_packed(vals, cdfs, counts, bias)             # noqa: E731
            iv, sm = hip_p()
            s_t, _, e_t, _, _, _ = ref_p()
            diff = max((sm.vals - s_t).abs().max().item(), (iv.vals - e_t).abs().max().item())
            S = int(counts.sum().item())
            Ee = S + int((counts > 0).sum().item())
            nbytes = R * E * 8 + R * 8 * 2 + S * (4 + 8) + Ee * (4 + 8 + 2) + R * 8 * 4
            emit(op="importance_sampling", layout="packed", E=E, n=n, n_rays=R, bytes=nbytes,
                 hip_ms=timed(hip_p, a.reps), torch_ms=timed(ref_p, a.reps), max_abs_diff=diff)

    for K in (257, 97):
        for R in (4096, 65536, 262144):
            kv, _ = rows(R, K, dev, g)
            q = torch.sort(torch.rand(R, 49, device=dev, generator=g) * 10, 1).values.contiguous()
            ks, qs = spec(kv), spec(q)
            hip = lambda: C.searchsorted(qs, ks)        # noqa: E731

            def ref():
                p = torch.searchsorted(kv[:, :-1].contiguous(), q, right=True)
                return (p - 1).clamp(0, K - 1), p.clamp(0, K - 1)

            l1, r1 = hip()
            l2, r2 = ref()
            assert torch.equal(l1, l2) and torch.equal(r1, r2), "searchsorted differs from torch.searchsorted + clamp"
            nbytes = R * K * 4 + R * 49 * 4 + 2 * R * 49 * 8
            emit(op="searchsorted", layout="batched", E=K, n=49, n_rays=R, bytes=nbytes,
                 hip_ms=timed(hip, a.reps), torch_ms=timed(ref, a.reps), max_abs_diff=0.0)

    if a.json:
        with open(a.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")
    print("| op | layout | E | n | rays | HIP ms | torch ms | speedup | HIP GB/s | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in out:
        print(f"| {r['op']} | {r['layout']} | {r['E']} | {r['n']} | {r['n_rays']} | {r['hip_ms']:.4f} | "
              f"{r['torch_ms']:.4f} | {r['speedup']:.1f}x | {r['hip_GBps']:.0f} | {100 * r['hip_peak_frac']:.1f} % |")


if __name__ == "__main__":
    main()
