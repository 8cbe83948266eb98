"""The data-parallel training step with the tables' Adam kernel (cnc_amd/trainer.py, cnc_amd/_table_adam.py): the tables'
share of the all-reduced bucket is the kernel's first piece with the factor 1 / world, the entropy gradient follows as
further pieces, only the rest of the bucket is divided.  Worker scripts in child processes, as tests/test_gpu_multi.py
runs them (its toy configuration, step_update = 4), each under its own time limit:

 * a forced one-rank world (CNC_DIST_FORCE=1, gloo), reproducible mode: the kernel is on, `.grad` is None behind a step, the
   step counters agree, two Trainers from one seed agree bit for bit — and then the twin: at steps 0, 5 and 8 the kernel's
   p, m, v equal tests/adam_twin.py on the SINGLE gradient the library path of the same step had summed into `.grad`
   (piece order, grouping and scale held to that path's own sum);
 * the same world with the schedule that ships (threads, streams, the planes' graph): 12 steps, finite tables, the first
   four steps' losses within the relative 1e-5 of a `fused_table_adam = False` run that tests/test_gpu_table_adam.py uses for
   this comparison at N = 1;
 * two ranks on one device over gloo: `last_grad_scale == 0.5`, replicas bit-identical, rank 0's first four steps within
   the same 1e-5 of a two-rank library-path run; and a resync that fires behind the kernel's step (rank 1's table flipped
   through `.data`) leaves the plane the kernel wrote stale, so the next forward repacks it from the re-aligned table."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
CHILD_LIMIT = 600          # seconds per child; a run takes well under a minute

_HEAD = r"""
import os, sys, json, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from cnc_amd.trainer import TrainConfig, Trainer
import adam_twin as T

def config(**kw):
    return TrainConfig(lmbda=2e-3, Pg_level=5, Pg_level_2D=3, log2_hashmap_size=12, log2_hashmap_size_2D=9,
                       sample_num=3000, max_context_layer_num=3, n_features=2, n_neurons=32,
                       resolutions_list=(10, 14, 18, 26, 34), resolutions_list_2D=(18, 34, 66),
                       skip_levels_3D=(0, 1, 2), skip_levels_2D=(0,), max_steps=20, init_batch_size=512,
                       target_sample_batch_size=1 << 14, grid_resolution=16, render_step_size=2e-2,
                       milestones=(100, 130), warmup_iters=20, test_views=2, image_size=48, out_dir={out!r},
                       step_update=4, **kw)

def tables(tr):
    return [e.params for e in tr.field.mlp_base._encoders()]

def host(t):
    return t.detach().cpu().numpy().reshape(-1).copy()

def state(tr):
    # p, m, v of every table, on the host
    torch.cuda.synchronize()
    return [(host(p), host(tr.opt.state[p]["exp_avg"]), host(tr.opt.state[p]["exp_avg_sq"])) for p in tables(tr)]

def differing(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())

def new_trainer(fused=True, **kw):
    tr = Trainer(config(**kw), device="cuda")
    assert tr.dp and tr.bucket is not None and torch.distributed.is_initialized()
    assert tr.table_adam is not None and tr.fused_table_adam, "the data-parallel Trainer has no TableAdam"
    tr.fused_table_adam = fused
    return tr

def finish(**result):
    print("RESULT " + json.dumps(result), flush=True)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
"""

_REPRODUCIBLE = _HEAD + r"""
SNAP = (0, 5, 8)

# ---- the kernel throughout: Trainer Y, 10 steps, its state kept behind steps 0, 5 and 8
y = new_trainer(reproducible=True)
assert torch.distributed.get_world_size() == 1 and y.reproducible and not y.ctx_thread
y_after = {{}}
for s in range(10):
    y.train_step(s)
    assert all(p.grad is None for p in tables(y)), f"step {{s}}: a table's .grad is not None behind the kernel's step"
    assert y.table_adam.last_grad_scale == 1.0
    if s in SNAP:
        y_after[s] = state(y)
assert y.table_adam.steps_done == 10
for p in tables(y):
    assert float(y.opt.state[p]["step"]) == 10.0, float(y.opt.state[p]["step"])
y_end = state(y)
assert all(np.isfinite(x).all() for tab in y_end for x in tab)

# ---- two Trainers from one seed agree bit for bit (in front of the twin: it compares two Trainers' steps)
z = new_trainer(reproducible=True)
for s in range(10):
    z.train_step(s)
diff = [[differing(a, b) for a, b in zip(ta, tb)] for ta, tb in zip(y_end, state(z))]
assert not any(any(d) for d in diff), f"two reproducible data-parallel Trainers from one seed differ after 10 steps (p, m, v per table): {{diff}}"
del z

# ---- the twin: X runs the kernel up to step s - 1 and the library path at step s, where a hook in front of the optimizer's
# step clones what that path summed into `.grad`; Y's kernel step s must be adam_twin's step on it
report = {{}}
for s in SNAP:
    x = new_trainer(reproducible=True)
    for k in range(s):
        x.train_step(k)
    got = {{}}
    def hook(opt, args, kwargs):
        g = x.table_adam.group
        got["lr"], got["betas"], got["eps"], got["wd"] = float(g["lr"]), tuple(g["betas"]), float(g["eps"]), float(g["weight_decay"])
        got["tables"] = []
        for p in tables(x):
            assert p.grad is not None
            st = opt.state.get(p, {{}})
            zeros = np.zeros(p.numel(), np.float32)
            got["tables"].append((host(p.grad), host(p), host(st["exp_avg"]) if len(st) else zeros,
                                  host(st["exp_avg_sq"]) if len(st) else zeros.copy()))
    handle = x.opt.register_step_pre_hook(hook)
    x.fused_table_adam = False
    x.train_step(s)
    handle.remove()
    torch.cuda.synchronize()
    assert got and all(p.grad is not None for p in tables(x))
    b1, b2 = got["betas"]
    report[s] = []
    for k, ((g, p, m, v), (yp, ym, yv)) in enumerate(zip(got["tables"], y_after[s])):
        want = T.adam_step(p, m, v, [(g, 0, g.size)], g.size, got["lr"], b1, b2, got["eps"], got["wd"], s + 1)
        d = (differing(yp, want.p), differing(ym, want.m), differing(yv, want.v))
        report[s].append(d)
        assert float(np.abs(g).max()) > 0, f"step {{s}} table {{k}}: the captured gradient is all zero"
    del x
assert not any(any(d) for ds in report.values() for d in ds), \
    f"elements of (p, m, v) per table that differ from the twin on the library path's summed gradient: {{report}}"
finish(twin=report, determinism=diff)
"""

_SHIPPED = _HEAD + r"""
world = {world}
os.environ["CNC_PLANES_GRAPH_STRICT"] = "1"
tr = new_trainer()
assert torch.distributed.get_world_size() == world
assert not tr.reproducible and tr.ctx_thread and tr.planes_graph is not None
stats = [tr.train_step(s) for s in range(12)]
torch.cuda.synchronize()
assert tr.fused_table_adam and all(p.grad is None for p in tables(tr))
assert tr.table_adam.last_grad_scale == float(np.float32(1) / np.float32(world)), tr.table_adam.last_grad_scale
assert tr.table_adam.steps_done == 12 and all(float(tr.opt.state[p]["step"]) == 12.0 for p in tables(tr))
assert tr.planes_graph is not None and tr.planes_graph.replays > 0
assert all(bool(torch.isfinite(p).all()) for p in tables(tr))
params = list(tr.field.parameters()) + list(tr.context.parameters())
sums = [float(p.detach().double().sum()) for p in params]
absum = [float(p.detach().double().abs().sum()) for p in params]
resync, replays = tr.resync, tr.planes_graph.replays
del tr
lib = new_trainer(fused=False)
ref = [lib.train_step(s) for s in range(4)]
torch.cuda.synchronize()
assert not lib.fused_table_adam and all(p.grad is not None for p in tables(lib))
# ---- a resync that fires behind the kernel's step: the kernel has left the sign planes of the tables it updated and marked them
# current; `resync_parameters` then overwrites rank 1's table with rank 0's and must move the version the plane's cache is
# keyed on, so that the next forward repacks it (two ranks: with one, checksums cannot differ)
plane = None
if world > 1:
    del lib
    r = new_trainer()
    for s in range(3):
        r.train_step(s)
    enc = r.field.mlp_base.encoding_xyz
    p = enc.params
    assert enc.ste_binary and enc.bitplane
    if r.rank == 1:
        p.data.neg_()                       # through `.data`: the version does not move; every sign of the replica flips
        enc.invalidate_caches()
    r.train_step(3)                         # (3 + 1) % step_update == 0: the replicas are compared behind this step's update
    torch.cuda.synchronize()
    key_now = (p.data_ptr(), p._version, tuple(p.shape))
    stale = enc._bits_key != key_now
    bits, _ = enc._bit_plane(p)
    want_bits, _ = T.sign_plane(host(p))
    plane = dict(fired=r.resync["fired"], tensors=r.resync["tensors"], stale=bool(stale),
                 repacked=bool(np.array_equal(bits.cpu().numpy().reshape(-1), want_bits)),
                 table=[float(p.detach().double().sum()), float(p.detach().double().abs().sum())])
    lib = r
pick = lambda out: [dict(mse=s["mse"], bpp=s["bpp"], samples=s["n_rendering_samples"], rays=s["num_rays"]) for s in out[:4]]
finish(rank=lib.rank, device=str(lib.device), got=pick(stats), ref=pick(ref), sums=sums, absum=absum, resync=resync,
       replays=replays, scale=float(np.float32(1) / np.float32(world)), plane=plane)
"""


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CNC_TABLE_ADAM")}
    env.update(extra)
    return env


def _run(tmp_path, source, world, **env_extra):
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    script = tmp_path / "worker.py"
    script.write_text(source.format(root=ROOT, tests=TESTS, out=str(tmp_path / "bits"), world=world))
    procs = []
    for rank in range(world):
        env = _clean_env(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                         MASTER_PORT=str(port), CNC_DIST_BACKEND="gloo", **env_extra)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            o, e = p.communicate(timeout=CHILD_LIMIT)
            assert p.returncode == 0, e[-3000:]
            outs.append(json.loads([l for l in o.splitlines() if l.startswith("RESULT ")][0][7:]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return outs


def _same_losses(got, ref):
    """tests/test_gpu_table_adam.py's comparison of the first four steps of a kernel run and a library-path run."""
    assert len(got) == len(ref) == 4
    for a, b in zip(ref, got):
        print("library path", a, "kernel", b)
        assert a["samples"] == b["samples"] and a["rays"] == b["rays"]
        assert abs(a["mse"] - b["mse"]) <= 1e-5 * max(a["mse"], 1e-6) + 1e-9
        assert abs(a["bpp"] - b["bpp"]) <= 1e-5 * a["bpp"]


def test_forced_one_rank_world_reproducible_against_the_twin(cuda, tmp_path):
    """The assertions are the worker's own (its stderr tail is this test's message): the kernel is on, `.grad` None, the step
    counters, bit-equal Trainers from one seed, then the twin at steps 0, 5 and 8."""
    out, = _run(tmp_path, _REPRODUCIBLE, 1, CNC_DIST_FORCE="1")
    print(out)
    assert sorted(out["twin"]) == ["0", "5", "8"] and all(len(v) == 4 for v in out["twin"].values())
    assert not any(any(d) for ds in out["twin"].values() for d in ds)


def test_forced_one_rank_world_shipped_schedule(cuda, tmp_path):
    out, = _run(tmp_path, _SHIPPED, 1, CNC_DIST_FORCE="1")
    assert out["replays"] > 0 and out["scale"] == 1.0
    _same_losses(out["got"], out["ref"])


def test_two_ranks_on_one_device(cuda, tmp_path):
    """World 2 is a power of two: `x * (1 / world)` and `x / world` coincide, so beyond the 1e-5 asserted here the two paths
    differ only by the order of the entropy pass's float atomics."""
    outs = sorted(_run(tmp_path, _SHIPPED, 2, CNC_DIST_ONE_DEVICE="1"), key=lambda d: d["rank"])
    a, b = outs
    assert a["rank"] == 0 and b["rank"] == 1 and a["device"] == b["device"] == "cuda:0"
    assert a["scale"] == b["scale"] == 0.5
    assert a["sums"] == b["sums"] and a["absum"] == b["absum"]          # bit-identical replicas behind the last resync
    assert sum(a["absum"]) > 0 and a["resync"] == b["resync"] and a["resync"]["checks"] == 3
    assert [s["rays"] for s in a["got"]] == [s["rays"] for s in b["got"]]
    assert [s["mse"] for s in a["got"]] != [s["mse"] for s in b["got"]]   # ... trained on different rays
    _same_losses(a["got"], a["ref"])
    # the resync that fired behind the kernel's step: the plane the kernel left is no longer current, the next one is the table's
    for o in outs:
        assert o["plane"]["fired"] == 1 and o["plane"]["tensors"] >= 1, o["plane"]
        assert o["plane"]["stale"] and o["plane"]["repacked"], o["plane"]
    assert a["plane"]["table"] == b["plane"]["table"]
