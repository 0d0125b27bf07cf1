"""bench.py with and without --full on the GPU: a plain run prints the headline line alone (no true residual, no per-kernel pass,
no side legs, no detail file named); --full adds them to the same timed configuration."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _line(extra, tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", "16", "--steps", "2", "--warmup", "1"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(tmp_path):
    out = _line([], tmp_path)
    assert all(k in out for k in HEADLINE), out
    assert out["unit"] == "DoF/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    assert out["config"]["fgmres_iters"] > 0
    for k in ("roofline", "cpu_baseline", "value_cold", "value_sustained", "value_matrix_free", "side_legs", "detail"):
        assert k not in out, k
    assert "true_rel_residual" not in out["config"]


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_side_legs(tmp_path):
    out = _line(["--full", "--cpu-cells", "0", "--fsi", "0", "--cylinder-legs", "0"], tmp_path)
    assert all(k in out for k in HEADLINE), out
    assert out["detail"] == "bench_detail.json"
    assert out["roofline"]["kernel_ms_per_step"]["assemble_cells"] > 0
    assert 0 < out["config"]["true_rel_residual"] < 1e-2
    assert out["value_cold"] > 0
