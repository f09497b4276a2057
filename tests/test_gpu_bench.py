"""bench.py on one GPU as the driver runs it: a plain run does only what its headline figure needs; --full adds the
diagnostic legs to the same line and leaves the timed steps, and what they dump, as they are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
DIAGNOSTIC = ("median_ms", "p10_ms", "p90_ms", "value_at_median", "spread", "other_configs", "cpu_baseline")


def _bench(outdir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--dump-outputs", str(outdir), *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "one bench line"
    return json.loads(lines[0]), np.load(outdir / "actions.npy")


def test_plain_run_is_lean_and_full_adds_the_diagnostic_legs(tmp_path):
    plain, acts = _bench(tmp_path / "plain")
    assert all(k in plain for k in HEADLINE)
    assert plain["unit"] == "action-chunks/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["value"] > 0 and abs(plain["value"] - 256 / (plain["ms_per_step"] * 1e-3)) <= 1e-3 * plain["value"]
    assert not [k for k in DIAGNOSTIC if k in plain] and "dominant_kernel" not in plain["roofline"]
    assert acts.shape == (256, 10, 7) and np.isfinite(acts).all()

    full, acts_full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline")
    assert all(k in full for k in HEADLINE)
    assert full["spread"]["calls"] == 50 and 0 < full["p10_ms"] <= full["median_ms"] <= full["p90_ms"]
    dk = full["roofline"]["dominant_kernel"]
    assert "error" not in dk and dk["avg_us"] > 0 and dk["alone"]["avg_us"] > 0
    assert "other_configs" not in full and "cpu_baseline" not in full  # --no-cpu-baseline
    # the diagnostic legs run behind the timed steps: the same seeded steps dump the same actions
    np.testing.assert_allclose(acts_full, acts, rtol=1e-5, atol=1e-6)
