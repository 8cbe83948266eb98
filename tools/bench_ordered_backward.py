"""The ordered encoder backward (cnc_grid_encode_backward_ordered: gradients bit-equal to the serial oracle) next to the
default routes, on the two calls profiles/ordered_backward.md tabulates:

    chunk     the bench chunk: 16 levels x 2^19 x F8, 2^20 marched samples from the middle of the frame; default = the
              bench's own call (merge kernel on the coarse levels + the binned finest ones, overlapped)
    input_b   Input B: the four encoders of the reference composition (12 x 3-D + 3 planes x 4), 2^18 samples, F = 8,
              through `_FusedFeatures.scatter` as the training step's render pass calls them

HIP events, 3 warm-up calls, then the two routes alternating in one process; medians and min .. max.  In the same run
the two results are compared within the float64-shadow bound of the atomic routes' tests — |fp32 sum in any order -
exact| <= (n + 2) eps sum|terms| for each of them, so twice that between them — with sum|terms| from the ordered route
on |grad| (a sum of non-negative terms: exact to n eps relative) and n = N 2^D as in tests/test_gpu_encoder.py.

    --call chunk|input_b|both (default both)    --reps K (default 9)
    --only-ordered    no default-route call and no comparison: what a `rocprofv3 --kernel-trace --stats` run of this
                      tool profiles for the emit / sort / reduce split"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import bench
import cnc_amd
from bench import enc, synthetic, D, F, L
from cnc_amd import _lib

arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
which, reps, only_ordered = arg("--call", "both"), int(arg("--reps", "9")), "--only-ordered" in sys.argv
dev = torch.device("cuda:0")
w = bench.build_workload(dev, 0)
box = {}
bench.march_frame(w, box)
xs = bench.probe_chunk_of(box["ex"]["positions"]).contiguous()
torch.cuda.synchronize()
EPS = float(np.finfo(np.float32).eps)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def measure(default, ordered):
    """ms per call of the two routes, alternating."""
    for _ in range(3):
        ordered()
        if not only_ordered:
            default()
    t = {"default": [], "ordered": []}
    for _ in range(reps):
        if not only_ordered:
            t["default"].append(timed(default))
        t["ordered"].append(timed(ordered))
    return {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
            for k, v in t.items() if v}


def agree(got, want, mag, n_terms):
    """Both within (n + 2) eps sum|terms| of the exact sum -> within twice that of each other."""
    bound = 2.0 * (n_terms + 2) * EPS * mag.double() * (1.0 + n_terms * EPS) + 1e-30
    diff = (got.double() - want.double()).abs()
    return {"within_bound": bool((diff <= bound).all().item()), "max_abs_diff": float(diff.max()),
            "max_diff_over_bound": float((diff / bound).max()), "largest_value": float(want.abs().max())}


def ws_bytes(n, dims, rows):
    return int(_lib.lib().cnc_grid_encode_backward_ordered_workspace(n, dims, rows))


result = {}
if which in ("chunk", "both"):
    n = xs.shape[0]
    out = torch.empty((L, n, F), device=dev)
    enc.pack_sign_bits(w["table"], w["bits"], w["clip"])
    enc.grid_encode_forward_bits(xs, w["bits"], w["offsets"], w["resolutions"], out, n, D, F, L, 128)
    gt = torch.zeros_like(w["table"])
    plan = enc.plan_binned_levels(synthetic.RES_16L, w["offsets_host"], D, F, n)

    def call(grad=out, table=gt, **kw):
        enc.grid_encode_backward(grad, xs, w["table"], w["offsets"], w["resolutions"], table, n, D, F, L, 0, 128, None, None,
                                 None, None, ste_binary=True, ste_clip_count=w["clip"], **kw)

    r = measure(lambda: call(binned=plan, ordered=False), lambda: call(ordered=True))
    r["samples"], r["levels"], r["workspace_bytes"] = n, L, ws_bytes(n, D, w["table"].shape[0])
    if not only_ordered:
        got, want, mag = torch.zeros_like(gt), torch.zeros_like(gt), torch.zeros_like(gt)
        call(table=got, ordered=True)
        call(table=want, binned=plan, ordered=False)
        call(grad=out.abs(), table=mag, ordered=True)
        again = torch.zeros_like(gt)
        call(table=again, ordered=True)
        torch.cuda.synchronize()
        r["ordered_vs_default"] = agree(got, want, mag, n << D)
        r["ordered_twice_identical"] = bool(torch.equal(got.view(torch.int32), again.view(torch.int32)))
        r["slowdown"] = round(r["ordered"]["median_ms"] / r["default"]["median_ms"], 1)
        del got, want, mag, again
    result["chunk"] = r
    del out, gt

if which in ("input_b", "both"):
    from cnc_amd.field import NGPRadianceField_mygrid_2D3D, _FusedFeatures
    from cnc_amd._gradsink import GradSink
    n = min(bench.N_INPUT_B, xs.shape[0])
    x = xs[:n].contiguous()
    torch.manual_seed(3)
    f = NGPRadianceField_mygrid_2D3D(aabb=list(bench.AABB), n_features_per_level=8, n_neurons=160,
                                     resolutions_list=bench.RES_3D_B, log2_hashmap_size=19,
                                     resolutions_list_2D=bench.RES_2D_B, log2_hashmap_size_2D=17).to(dev)
    mb = f.mlp_base
    encs = mb._encoders()
    with torch.no_grad():
        for e in encs:
            e.params.uniform_(-1, 1)
    params = [e.params for e in encs]
    sink = GradSink(params, [])
    ld, cols = mb._layout()
    pts = (x, x[:, :2].contiguous(), x[:, ::2].contiguous(), x[:, 1:].contiguous())
    clips = [e._bit_plane(e.params)[1] for e in encs]
    grad = torch.randn(n, ld, device=dev)

    def scatter(ordered, g=grad, into=sink):
        with cnc_amd.ordered_backward(ordered):
            return _FusedFeatures.scatter(mb, g, pts, params, clips, n, into)

    r = measure(lambda: scatter(False), lambda: scatter(True))
    r["samples"], r["encoders"] = n, [f"{e.num_dim}-D x {e.n_levels} levels" for e in encs]
    r["workspace_bytes"] = {f"{e.num_dim}-D": ws_bytes(n, e.num_dim, e.params.shape[0]) for e in encs[:2]}
    if not only_ordered:
        got, want = scatter(True, into=None), scatter(False, into=None)
        mag, again = scatter(True, g=grad.abs(), into=None), scatter(True, into=None)
        torch.cuda.synchronize()
        r["ordered_vs_default"] = [agree(a, b, m, n << e.num_dim) for a, b, m, e in zip(got, want, mag, encs)]
        r["ordered_twice_identical"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))
        r["slowdown"] = round(r["ordered"]["median_ms"] / r["default"]["median_ms"], 1)
    result["input_b"] = r

print(json.dumps(result, indent=1))
