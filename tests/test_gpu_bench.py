"""bench.py as a plain run: the JSON line carries the headline figure and the fields of the timed steps, nothing that takes a run of
its own (those come with --full), and --dump-outputs writes the logits the last timed step computed."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_line_and_dumped_logits(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--hyps", "256", "--panos", "8",
           "--dump-outputs", str(tmp_path / "out")]
    proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "hypotheses/s" and out["higher_is_better"] is True and out["dtype"] == "fp16"
    assert out["ms_per_step"] > 0 and abs(out["value"] - 256 * 1e3 / out["ms_per_step"]) <= 1e-3 * out["value"]
    assert out["roofline"]["renders_per_launch"] == 256 and out["roofline_verifier"]["samples_per_launch"] == 256
    assert "config5" not in out and "cpu_baseline" not in out
    assert "hbm_copy_gbs_measured" not in out["roofline"] and "gemm_reference" not in out["roofline_verifier"] and "power_w" not in out["roofline_verifier"]
    logits = np.load(tmp_path / "out" / "logits.npy")
    assert logits.dtype == np.float32 and logits.shape == (256, 2) and np.isfinite(logits).all()
