"""`python -m cnc_amd.train --background envmap` in a fresh child process: the protocol runs to its results line and leaves
a container whose `envmap` section holds the H x 2H x 3 bytes of the learned background."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_COLS = 9 + 3 + 6 + 3      # the results line of tests/test_gpu_cli.py


def test_cli_trains_with_an_envmap_and_writes_it_into_the_container(cuda, tmp_path):
    from cnc_amd.container import read_envmap, section_sizes
    argv = ["--dataset", "procedural", "--background", "envmap", "--envmap-resolution", "8", "--max_steps", "20",
            "--n_features", "2", "--sample_num", "20000", "--test_views", "1", "--log2_hashmap_size", "14",
            "--log2_hashmap_size_2D", "12", "--image_size", "48", "--results", str(tmp_path / "out.txt"),
            "--out_dir", str(tmp_path / "bits")]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "cnc_amd.train"] + argv, cwd=str(tmp_path), env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "alpha below 1" in r.stderr                      # the procedural ball's pixels are transparent where rays miss it
    line = open(tmp_path / "out.txt").read().strip().split("\t")
    assert len(line) == N_COLS and line[0] == "ball"
    box = str(tmp_path / "bits" / "scene.cnc")
    assert section_sizes(box)["envmap"] == 8 * 16 * 3
    u8 = read_envmap(box)
    assert tuple(u8.shape) == (8, 16, 3) and int((u8 != 128).sum()) > 0        # it moved off the grey start
