"""Bit-plane forward of the bench, one level at a time: bench.py's marched chunk (probe_chunk_of, 2^20 samples of the
800x800 frame), 16L x 2^19 x F8, the sign bit plane of the bench's table.  Times the whole call (L = 16, level-major
[L, N, F]) and each level alone as an L = 1 call on that level's offsets and resolution views, under each sign-table
mode (CNC_FWD_LUT, read per launch: 0 shift + bfi, 1 table on every level, 2 on the dense levels).  One JSON line per
row.  --pair: the same rows under the paired-gather modes instead (CNC_FWD_PAIR, read per launch: 0 byte gathers, 1 the
default policy, 2 every hashed level), sign table as shipped, the modes alternating twice per row.

    python tools/fwd_levels.py                    # the table
    python tools/fwd_levels.py --pair 0,2         # per level: byte gathers against paired gathers
    python tools/fwd_levels.py --only 15,3,all --reps 3   # just these calls in this order, `reps` each: for a
                                                          # counter run (rocprofv3 --pmc ... --); 'all' = the L = 16 call
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from cnc_amd.backends import gridencoder_backend as enc  # noqa: E402


def timeit(fn, n=50):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="comma-separated level indices, 'all' for the L = 16 call")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--pair", default=None, help="comma-separated CNC_FWD_PAIR modes to compare per row")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    w = bench.build_workload(dev, 0)
    box = {}
    bench.march_frame(w, box)
    x = bench.probe_chunk_of(box["ex"]["positions"]).contiguous()
    N, F, L, D = x.shape[0], bench.F, bench.L, bench.D
    enc.pack_sign_bits(w["table"], w["bits"], w["clip"])
    o_t, r_t = w["offsets"], w["resolutions"]
    out = torch.empty((L, N, F), device=dev)

    def call(l):
        if l is None:
            return lambda: enc.grid_encode_forward_bits(x, w["bits"], o_t, r_t, out, N, D, F, L, 128)
        return lambda: enc.grid_encode_forward_bits(x, w["bits"], o_t[l:l + 2], r_t[l:l + 1], out[l:l + 1], N, D, F,
                                                    1, 128)

    if args.only is not None:
        for o in args.only.split(","):
            fn = call(None if o == "all" else int(o))
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
        return
    if args.pair is not None:
        os.environ.pop("CNC_FWD_LUT", None)
        pairs = args.pair.split(",")
        total = dict.fromkeys(pairs, 0.0)
        for l in [None] + list(range(L)):
            row = {"levels": "all", "N": N} if l is None else {
                "level": l, "R": int(bench.synthetic.RES_16L[l]), "rows": int(w["offsets_host"][l + 1] - w["offsets_host"][l])}
            ms = {m: [] for m in pairs}
            for _ in range(2):
                for m in pairs:
                    os.environ["CNC_FWD_PAIR"] = m
                    ms[m].append(round(timeit(call(l), args.reps), 4))
            for m in pairs:
                row["ms_pair%s" % m] = ms[m]
                if l is not None:
                    total[m] += min(ms[m])
            print(json.dumps(row), flush=True)
        print(json.dumps({"levels": "sum of the L = 1 calls (min of the two passes)",
                          **{"ms_pair" + k: round(v, 4) for k, v in total.items()}}))
        del os.environ["CNC_FWD_PAIR"]
        return
    modes = ("0", "1", "2")
    for lut in modes:
        os.environ["CNC_FWD_LUT"] = lut
        print(json.dumps({"levels": "all", "N": N, "lut": int(lut), "ms": round(timeit(call(None), args.reps), 4)}))
    total = dict.fromkeys(modes, 0.0)
    for l in range(L):
        row = {"level": l, "R": int(bench.synthetic.RES_16L[l]), "rows": int(w["offsets_host"][l + 1] - w["offsets_host"][l])}
        for lut in modes[:2]:
            os.environ["CNC_FWD_LUT"] = lut
            row["ms_lut%s" % lut] = round(timeit(call(l), args.reps), 4)
            total[lut] += row["ms_lut%s" % lut]
        print(json.dumps(row))
    print(json.dumps({"levels": "sum of the L = 1 calls", **{"ms_lut" + k: round(v, 4) for k, v in total.items() if v}}))
    del os.environ["CNC_FWD_LUT"]

if __name__ == "__main__":
    main()
