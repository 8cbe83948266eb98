"""The guarded step, data parallel (cnc_amd/trainer.py): the replicas reach one verdict without a collective of their own.
Two ranks on one device over gloo, worker scripts in child processes as tests/test_gpu_dp_table_adam.py runs them (its toy
configuration, step_update = 4, the schedule that ships).  Rank 1 ALONE is fed a batch with a NaN pixel at step 4: its
non-finite ray gradient reaches rank 0 in the all-reduced sum, both ranks skip — every parameter, moment and step count
keeps every bit on both — `skipped == 1` on both, the sample-count slot of the bucket still carries the two ranks' count next
to the new guard slot, and after three more steps (a resync behind the last) the replicas are bit-identical and finite."""
import pytest

import test_gpu_dp_table_adam as D

pytestmark = pytest.mark.gpu

_WORKER = D._HEAD + r"""
world = {world}
tr = new_trainer(guarded_step=True)
assert torch.distributed.get_world_size() == world == 2
assert tr.step_guard is not None and tr.bucket.tail.numel() == 2 and tr._count_host.numel() == 1

def everything():
    torch.cuda.synchronize()
    out = {{}}
    for name, mod in (("field", tr.field), ("context", tr.context)):
        for n, p in mod.named_parameters():
            out[name + "." + n] = p.detach().clone()
    for oname, opt in (("opt", tr.opt), ("opt2", tr.opt2)):
        for gi, group in enumerate(opt.param_groups):
            for pi, p in enumerate(group["params"]):
                for k, v in opt.state.get(p, {{}}).items():
                    if isinstance(v, torch.Tensor):
                        out["%s.%d.%d.%s" % (oname, gi, pi, k)] = v.detach().clone()
    return out

def differing(a, b):
    return [k for k in a if not torch.equal(a[k].contiguous().reshape(-1).view(torch.uint8), b[k].contiguous().reshape(-1).view(torch.uint8))]

for s in range(4):                          # the replicas are compared and aligned behind step 3
    tr.train_step(s)
assert tr.step_guard.stats() == dict(skipped=0, reasons=0)
before = everything()
if tr.rank == 1:
    data = dict(tr.dataset.fetch())
    px = data["pixels"].clone()
    px.view(-1)[px.numel() // 2] = float("nan")
    data["pixels"] = px
    tr._next_data = data
import warnings
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    out = tr.train_step(4)
after = everything()
moved = differing(before, after)
stats = tr.step_guard.stats()
count = float(tr._count_host[0])
slot = float(tr.bucket.tail[1])
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    for s in range(5, 8):                   # clean batches: the steps go ahead; the replicas are compared behind step 7
        tr.train_step(s)
later = everything()
params = list(tr.field.parameters()) + list(tr.context.parameters())
sums = [float(p.detach().double().sum()) for p in params]
absum = [float(p.detach().double().abs().sum()) for p in params]
steps = sorted({{float(v) for k, v in later.items() if k.endswith(".step")}})
finish(rank=tr.rank, moved=moved, n_state=len(before), stats=stats, final=tr.step_guard.stats(), count=count, slot=slot,
       samples=out["n_rendering_samples"], mse_is_nan=bool(out["mse"] != out["mse"]), steps=steps, sums=sums, absum=absum,
       finite=all(bool(torch.isfinite(v.float()).all()) for v in later.values()),
       moved_later=len(differing(before, later)), attempts=tr.table_adam.steps_done)
"""


def test_one_ranks_nan_batch_makes_both_ranks_skip(cuda, tmp_path):
    outs = sorted(D._run(tmp_path, _WORKER, 2, CNC_DIST_ONE_DEVICE="1"), key=lambda d: d["rank"])
    a, b = outs
    print({k: v for k, v in a.items() if k not in ("sums", "absum")})
    print({k: v for k, v in b.items() if k not in ("sums", "absum")})
    assert a["rank"] == 0 and b["rank"] == 1
    assert b["mse_is_nan"] and not a["mse_is_nan"]                       # rank 1 alone saw the NaN
    for o in outs:
        assert o["n_state"] > 40 and o["moved"] == [], o["moved"][:8]     # nothing moved on either rank
        assert o["stats"] == {"skipped": 1, "reasons": 1} == o["final"]
        assert o["count"] == float(a["samples"] + b["samples"])         # the lagged sample count still rides along
        assert o["slot"] == 0.0                                          # no rank's range guard tripped
        assert o["steps"] == [7.0] and o["attempts"] == 8                # 8 steps attempted, 7 taken, everywhere
        assert o["finite"] and o["moved_later"] > 20
    assert a["sums"] == b["sums"] and a["absum"] == b["absum"] and sum(a["absum"]) > 0       # bit-identical replicas
