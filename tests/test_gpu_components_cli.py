"""`python -m cnc_amd.train --prune-floaters N` on the small procedural run of
tests/test_gpu_mesh_trainer.py's CLI test, each in a fresh child process: with the flag the run evaluates before pruning,
prints the `pruned:` line and both PSNR lines and appends the usual results line; without it neither line appears."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = 9 + 3 + 6 + 3      # the results line of tests/test_gpu_cli.py


def _run(tmp_path, *extra):
    argv = [sys.executable, "-m", "cnc_amd.train", "--max_steps", "40", "--n_features", "2", "--sample_num", "20000",
            "--test_views", "1", "--log2_hashmap_size", "14", "--log2_hashmap_size_2D", "12",
            "--results", str(tmp_path / "out.txt"), "--out_dir", str(tmp_path / "bits"), "--dataset", "procedural",
            "--image_size", "48"] + list(extra)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(argv, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = open(tmp_path / "out.txt").read().strip().split("\n")
    assert len(lines) == 1
    return r.stdout, lines[0].split("\t")


def test_prune_floaters_prints_its_lines_and_keeps_the_results_line(cuda, tmp_path):
    out, cols = _run(tmp_path, "--prune-floaters", "3", "--prune-connectivity", "14")
    m = re.findall(r"^pruned: (\d+) components / (\d+) cells removed, (\d+) components kept$", out, flags=re.M)
    assert len(m) == 1 and int(m[0][2]) >= 1 and int(m[0][1]) >= int(m[0][0])
    before = re.findall(r"^evaluation_before_pruning: psnr_avg=(\S+)$", out, flags=re.M)
    after = re.findall(r"^evaluation: psnr_avg=([^,\s]+),", out, flags=re.M)
    assert len(before) == 1 and len(after) == 1 and float(before[0]) > 0 and float(after[0]) > 0
    assert out.index("evaluation_before_pruning:") < out.index("pruned:") < out.index("evaluation: psnr_avg")
    assert len(cols) == N_COLS and cols[0] == "ball" and abs(float(cols[1]) - float(after[0])) <= 1e-4     # 4 decimals


def test_without_the_flag_neither_line_appears(cuda, tmp_path):
    out, cols = _run(tmp_path)
    assert "pruned:" not in out and "evaluation_before_pruning" not in out
    assert len(re.findall(r"^evaluation: psnr_avg=", out, flags=re.M)) == 1
    assert len(cols) == N_COLS and cols[0] == "ball"


def test_the_parser_refuses_another_connectivity():
    from cnc_amd.train import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--dataset", "procedural", "--scene", "ball", "--prune-connectivity", "8"])
    ns = build_parser().parse_args(["--dataset", "procedural", "--scene", "ball"])
    assert ns.prune_floaters == 0 and ns.prune_connectivity == 26 and ns.mesh_min_component == 0
