"""Default against paired owner placement (CNC_FLAG_OWNER_XCD_PAIRS) on the headline backward call — bench.py's middle
chunk (or `--chunk first`: grazing rays, bins up to 7.7x the mean), 16 levels, F = 8, STE — in ONE process, alternating:

    fine     the binned finest levels alone (cnc_grid_encode_backward_binned on those levels, one stream)
    call     the whole overlapped call (cnc_grid_encode_backward_overlapped) on one plan

The plan splits the finest levels as CNC_BWD_GROUP_SPLIT in the environment says (unset: one group); compare splits ACROSS
processes, one plan each, as the product has it — a second plan's side streams may share a hardware queue with the first
one's or with the caller's stream, which cost a 2 + 4 split 0.2 ms when four plans were timed in one process.

HIP events, median of 20 per variant and round, `--rounds` rounds (default 3); one JSON line per variant and round, then
the item count of the owner pass and the largest difference between the two placements' gradients.  What
profiles/r09_owner_xcd_placement.md tabulates."""
import ctypes as C
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from bench import enc, synthetic, D, F, L
from cnc_amd import _lib

rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
which = sys.argv[sys.argv.index("--chunk") + 1] if "--chunk" in sys.argv else "middle"
dev = torch.device("cuda:0")
w = bench.build_workload(dev, 0)
box = {}
bench.march_frame(w, box)
pos = box["ex"]["positions"]
xs = (bench.probe_chunk_of(pos) if which == "middle" else pos[: bench.CHUNK]).contiguous()
n = xs.shape[0]
out = torch.empty((L, n, F), device=dev)
enc.pack_sign_bits(w["table"], w["bits"], w["clip"])
enc.grid_encode_forward_bits(xs, w["bits"], w["offsets"], w["resolutions"], out, n, D, F, L, 128)
n_binned, level_rows = enc.plan_binned_levels(synthetic.RES_16L, w["offsets_host"], D, F, n)
lib = _lib.lib()
p = lambda t: C.c_void_p(t.data_ptr())
cur = _lib.stream(dev)
STE, PAIRS = _lib.CNC_FLAG_STE_BINARY, _lib.CNC_FLAG_OWNER_XCD_PAIRS
l0 = L - n_binned
offs_f, res_f, out_f = w["offsets"][l0:].contiguous(), w["resolutions"][l0:].contiguous(), out[l0:]
ws = torch.empty(int(lib.cnc_grid_encode_backward_overlapped_workspace(n, n_binned, level_rows)), dtype=torch.uint8, device=dev)
gt = torch.zeros_like(w["table"])


def fine(flags):
    rc = lib.cnc_grid_encode_backward_binned(p(out_f), p(xs), p(w["table"]), p(offs_f), p(res_f), p(gt), n, D, F, n_binned,
                                             flags, p(w["clip"]), 0, 0, n_binned, level_rows, p(ws), ws.numel(), cur)
    assert rc == 0, rc


plan = C.c_void_p()
assert lib.cnc_backward_plan_create(C.byref(plan)) == 0
split = os.environ.get("CNC_BWD_GROUP_SPLIT", "one group")


def whole(flags):
    rc = lib.cnc_grid_encode_backward_overlapped(plan, p(out), p(xs), p(w["table"]), p(w["offsets"]), p(w["resolutions"]), p(gt),
                                                 n, D, F, L, flags, p(w["clip"]), 0, 0, n_binned, level_rows, p(ws), ws.numel(),
                                                 cur)
    assert rc == 0, rc


variants = [("fine default", lambda: fine(STE)), ("fine paired", lambda: fine(STE | PAIRS)),
            ("call default", lambda: whole(STE)), ("call paired", lambda: whole(STE | PAIRS))]


def median_ms(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return round(sorted(ts)[10], 4)


print(json.dumps({"chunk": which, "samples": n, "n_binned": n_binned, "level_rows": level_rows, "group_split": split}), flush=True)
for r in range(rounds):
    for name, fn in variants:
        print(json.dumps({"round": r, "variant": name, "ms_per_call": median_ms(fn)}), flush=True)
fine(STE); torch.cuda.synchronize()
heads = n_binned * ((level_rows + 255) // 256)         # the bin counters lead the workspace
print(json.dumps({"owner_items_per_call": int(ws[: heads * 4].view(torch.int32).sum())}))
grads = []
for flags in (STE, STE | PAIRS):
    gt.zero_(); whole(flags); torch.cuda.synchronize()
    grads.append(gt.clone())
print(json.dumps({"max_abs_diff_between_placements": float((grads[0] - grads[1]).abs().max()), "largest": float(grads[0].abs().max())}))
lib.cnc_backward_plan_destroy(plan)
