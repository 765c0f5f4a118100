"""GPU: bench.py's plain run prints the headline line alone, --full adds what it moved there, and both compute the same
outputs (a 512 x ~300 protein job: seconds per run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--nseq", "512", "--len", "300", "--dump-outputs", str(out_dir)] + extra
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])


def test_plain_run_is_the_headline_line_and_full_adds_the_rest(tmp_path):
    plain = run_bench([], tmp_path / "plain")
    full = run_bench(["--full", "--no-legs", "--no-cpu"], tmp_path / "full")
    for d in (plain, full):
        assert d["unit"] == "GCUPS" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
        assert d["roofline"]["kernel_ms_per_step"] > 0
    assert full["config"]["useful_cells_per_step"] == plain["config"]["useful_cells_per_step"]
    assert plain["config"]["guide_tree_ms"] is None and "gcups_profile_profile" not in plain["config"]
    assert full["config"]["guide_tree_ms"] > 0 and full["config"]["gcups_profile_profile"]["profile_profile_tasks"] > 0
    assert not {"cpu_baseline", "saturation", "c2_1024x400_protein", "t_dp_with_transfers"} & set(plain)
    for name in ("records", "paths", "gaps"):
        assert np.array_equal(np.load(str(tmp_path / "plain" / (name + ".npy"))), np.load(str(tmp_path / "full" / (name + ".npy"))))
