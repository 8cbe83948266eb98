"""`python bench.py` as the driver runs it: the plain run prints the headline line without the --full blocks, and
`--dump-outputs DIR` leaves the last timed step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "roofline_forward", "field", "roofline_input_B", "train_step", "eval_render", "codec",
             "cpu_baseline", "cpu_baseline_torch")


def _bench(out_dir, steps):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "CNC_DIST_FORCE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(out_dir)], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir)}


def test_plain_bench_line_and_dumped_outputs(cuda, tmp_path):
    out, a = _bench(tmp_path / "a", 2)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["metric"].startswith("ray-samples/s") and out["unit"] == "ray-samples/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["value"] > 1e8 and out["ms_per_step"] > 0
    assert out["kernels"]["grid_encode_backward"]["launches"] > 0
    assert not [k for k in FULL_ONLY if k in out]
    # what was written: float32 / float64 only, 64 MB at most, consistent with the line and with itself
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    S = int(a["n_samples"][0])
    assert S == out["config"]["samples_per_step_rank0"] and a["chunk_cnts"].shape == (640000,) and a["chunk_cnts"].sum(dtype=np.float64) == S
    K = a["sample_index"].shape[0]
    assert 0 < K <= S and np.all(np.diff(a["sample_index"]) >= 0) and a["sample_index"][-1] < S
    assert a["ray_indices"].shape == a["t_starts"].shape == a["t_ends"].shape == (K,) and a["positions"].shape == (K, 3)
    assert np.all(np.diff(a["ray_indices"]) >= 0) and a["ray_indices"].max() < 640000       # samples come ray by ray
    assert np.all(a["t_starts"] < a["t_ends"]) and np.all((a["positions"] >= 0) & (a["positions"] <= 1))
    E = a["encoding_index"].shape[0]
    last_chunk = (S - 1) // (1 << 20) * (1 << 20)                                               # the rows come from it
    assert a["encoding"].shape == (16, E, 8) and last_chunk <= a["encoding_index"].min() <= a["encoding_index"].max() < S
    assert np.all(np.abs(a["encoding"]) <= 1.0 + 1e-6) and np.any(a["encoding"] != 0)         # sign(table) x weights
    assert a["grad_table_rows"].shape == (a["grad_table_row_index"].shape[0], 8) and a["grad_table_sums"].shape == (2, 8)
    assert np.all(a["grad_table_sums"][1] >= np.abs(a["grad_table_sums"][0])) and a["grad_table_sums"][1].sum() > 0
    # same arguments, same inputs: the march and the forward are bit-identical, the atomic backward equal up to order
    out_b, b = _bench(tmp_path / "b", 1)
    assert sorted(b) == sorted(a)
    for k in ("chunk_cnts", "n_samples", "sample_index", "ray_indices", "t_starts", "t_ends", "positions",
              "encoding_index", "encoding", "grad_table_row_index", "clip_count"):
        assert np.array_equal(a[k], b[k]), k
    scale = np.abs(a["grad_table_rows"]).max()
    assert np.allclose(a["grad_table_rows"], b["grad_table_rows"], rtol=1e-4, atol=1e-5 * scale)
    assert np.allclose(a["grad_table_sums"], b["grad_table_sums"], rtol=1e-4, atol=1e-5 * a["grad_table_sums"][1].max())
