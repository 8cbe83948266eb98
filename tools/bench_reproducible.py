"""What the reproducible mode costs (profiles/reproducible_step.md).

    python tools/bench_reproducible.py entries      # the two ordered entries alone against their plain forms (HIP events)
    python tools/bench_reproducible.py step         # ms per training step, mode off / on, alternating blocks in one process

`step` builds two Trainers of the bench's train_step configuration (tools/ab_train.py's), one per mode, and alternates
blocks of 30 timed steps between them (8 untimed steps in front of each block), as tools/ab_train.py does for a switch."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn


def timed(fn, n=9, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def entries():
    import cnc_amd
    from cnc_amd.backends import context_backend as K
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    print("| call | plain, ms (min .. max) | ordered, ms (min .. max) | ordered / plain |\n|---|---|---|---|")
    for name, N, seq, Ca, Cb, table in (
            ("three-layer head 25-32-32-8, 750 k rows, pg_index over 12 levels", 750000,
             nn.Sequential(nn.Linear(25, 32), nn.LeakyReLU(), nn.Linear(32, 32), nn.LeakyReLU(), nn.Linear(32, 8)), 24, 0, 12),
            ("single Linear 33 -> 8, 640 k rows, scalar Pg", 640000, nn.Sequential(nn.Linear(33, 8)), 24, 8, 0),
            ("single Linear 17 -> 8, 160 k rows, scalar Pg", 160000, nn.Sequential(nn.Linear(17, 8)), 8, 8, 0)):
        seq = seq.to(dev)
        a = torch.randn(N, Ca, device=dev, requires_grad=True)
        b = torch.randn(N, Cb, device=dev, requires_grad=True) if Cb else None
        pg = torch.rand(max(table, 1), device=dev, requires_grad=True)
        idx = torch.sort(torch.randint(0, table, (N,), device=dev))[0] if table else None
        go = torch.randn(N, 8, device=dev)
        res = {}
        for mode in (False, True):
            with cnc_amd.reproducible(mode):
                y = K.context_mlp(seq, a, b, pg if table else pg[0], idx)

                def bwd():
                    torch.autograd.grad(y, [a, pg] + list(seq.parameters()), go, retain_graph=True)
                res[mode] = timed(bwd)
        p, o = res[False], res[True]
        print(f"| context heads' backward (autograd call): {name} | {p[0]:.3f} ({p[1]:.3f} .. {p[2]:.3f}) | "
              f"{o[0]:.3f} ({o[1]:.3f} .. {o[2]:.3f}) | {o[0] / p[0]:.2f} |")
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_gpu_field_fused import CONFIGS, _field, _inputs
    for cfg, n in (("f8_full", 1 << 18), ("f2_toy", 1 << 18)):
        f = _field(dev, CONFIGS[cfg], seed=8)
        f.fused_chain, f.fused_train, f._chain_supported = True, False, None
        x, d = _inputs(dev, n, seed=1)
        res = {}
        for mode in (False, True):
            # the encoder's scatter is not part of this comparison: gradients of the MLP parameters only
            params = [p for nme, p in f.named_parameters() if not nme.endswith("params")]
            with cnc_amd.reproducible(mode):
                rgb, den = f(x, d)

                def bwd():
                    torch.autograd.grad(rgb.sum() + den.sum(), params, retain_graph=True)
                res[mode] = timed(bwd)
        p, o = res[False], res[True]
        print(f"| field gradient pass, MLP parameters only (chain + weight gradients): {cfg}, 2^18 samples | {p[0]:.3f} ({p[1]:.3f} .. {p[2]:.3f}) | "
              f"{o[0]:.3f} ({o[1]:.3f} .. {o[2]:.3f}) | {o[0] / p[0]:.2f} |")


def step():
    from cnc_amd.trainer import TrainConfig, Trainer
    dev = torch.device("cuda", 0)
    trs = {}
    for mode in (False, True):
        cfg = TrainConfig(n_features=8, sample_num=150000, max_steps=2000, image_size=400, out_dir="./bitstreams/bench_repro",
                          reproducible=mode)
        trs[mode] = [Trainer(cfg, device=dev), 0]
    for mode in (False, True):
        for _ in range(int(os.environ.get("WARM_STEPS", "120"))):
            trs[mode][0].train_step(trs[mode][1], want_stats=False)
            trs[mode][1] += 1
    res = {False: [], True: []}
    for rep in range(4):
        for mode in (False, True):
            tr = trs[mode]
            for _ in range(8):
                tr[0].train_step(tr[1], want_stats=False); tr[1] += 1
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(30):
                tr[0].train_step(tr[1], want_stats=False); tr[1] += 1
            torch.cuda.synchronize()
            res[mode].append((time.perf_counter() - t0) / 30 * 1e3)
    for mode in (False, True):
        r = sorted(res[mode])
        print(f"reproducible {'on ' if mode else 'off'}: median {r[len(r) // 2]:.2f} ms / step  min {r[0]:.2f}  max {r[-1]:.2f}   "
              f"{['%.2f' % x for x in res[mode]]}")


if __name__ == "__main__":
    {"entries": entries, "step": step}[sys.argv[1] if len(sys.argv) > 1 else "entries"]()
