"""bench.py's command line on a small crowd: a plain run carries the headline fields and none of the legs that are runs of their
own, `--dump-outputs` writes what the last timed step left (float32 / float64, the same from run to run), `--full` adds the legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LEGS = ("lbs_alone", "world_sync", "real_mesh", "cpu_baseline")
CHARS = 384


def run_bench(*flags):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--chars", str(CHARS), "--steps", "3", "--warmup", "2"] + list(flags)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_and_dump_outputs(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    rec = run_bench("--dump-outputs", a)
    assert rec["steps"] == 3 and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["value"] == pytest.approx(CHARS / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert (rec["metric"], rec["unit"], rec["higher_is_better"], rec["dtype"]) == ("characters/sec (skin+CCD)", "characters/s", True, "f32")
    assert not [k for k in LEGS if k in rec]
    run_bench("--dump-outputs", b)
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and all(f.endswith(".npy") for f in files)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in files) < 64e6
    arrays = {f[:-4]: np.load(os.path.join(a, f)) for f in files}
    for f, x in arrays.items():
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), f
        assert np.array_equal(x, np.load(os.path.join(b, f + ".npy"))), f + " differs between two runs with the same arguments"
    V = rec["config"]["vertices_per_character"]
    k = len(arrays["skinned_characters"])
    assert arrays["bodies_position"].shape == (CHARS, 3) and np.array_equal(arrays["state_characters"], np.arange(CHARS))
    assert 0 < k <= CHARS and arrays["skinned_positions"].shape == (k, V, 3) and arrays["skinned_tangents"].shape == (k, V, 4)
    assert arrays["palettes"].shape == (k, rec["config"]["bones"], 16)
    assert np.abs(arrays["skinned_positions"]).max(axis=(1, 2)).min() > 0.1  # every sampled character holds skinned output, not zeros


def test_full_adds_the_other_legs():
    """(`world_sync` and `real_mesh` build a second context and step it some hundred times: left out here with --no-extras, as the
    profiling scripts under tools/ do; the whole --full line is the benchmark's own business.)"""
    rec = run_bench("--full", "--no-extras", "--cpu-sample-chars", "64", "--cpu-sample-steps", "2")
    assert rec["lbs_alone"]["launches"] == 8 and rec["lbs_alone"]["ms_per_launch"] > 0 and rec["cpu_baseline"]["value"] > 0
    assert "world_sync" not in rec and "real_mesh" not in rec
