"""bench.py's plain run on the GPU: a few decode steps of a 4-layer QCN-shaped model, the line it prints, and --dump-outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_plain(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2", "--layers", "4", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    """the line holds the timed steps only; the dump is the last timed step's logits and greedy token (the first maximum of those logits), and a second
    run with the same arguments writes the same bits"""
    a = run_plain(tmp_path / "a")
    assert a["steps"] == 6 and a["warmup"] == 2 and a["value"] > 0 and abs(a["ms_per_step"] - 1e3 / a["value"]) <= 1e-3 * a["ms_per_step"]
    assert "roofline" not in a and "cpu_baseline" not in a and "prefill" not in a and "configs" not in a
    logits, token = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "token.npy")
    assert logits.dtype == np.float32 and logits.shape == (151936,) and np.isfinite(logits).all() and logits.std() > 0
    assert token.dtype == np.float64 and token.shape == (1,) and int(token[0]) == int(np.argmax(logits))
    run_plain(tmp_path / "b")
    for f in ("logits.npy", "token.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f).view(np.uint8), np.load(tmp_path / "b" / f).view(np.uint8)), f
