"""A plain bench.py run: the headline line only (nothing of what --full adds), --steps
timed steps, and --dump-outputs writing the state the timed chain ended in, identical
from run to run and different after another number of steps."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _bench(dump, steps):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", "2", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_bench_line_and_dump(tmp_path):
    out = _bench(tmp_path / "a", 4)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 4 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(
        out["config"]["N"] * (out["config"]["L"] - out["config"]["W"] + 1) * 1e3 / out["ms_per_step"])
    for k in ("cpu_baseline", "roofline_cfg3", "cfg4", "cfg5", "cfg2_uniform"):
        assert k not in out, k
    assert out["roofline"]["dispatch_event_ms"] is None and out["roofline"]["traffic"] is None
    N, L, W = (out["config"][k] for k in "NLW")
    pos, pw = np.load(tmp_path / "a" / "positions.npy"), np.load(tmp_path / "a" / "pwms.npy")
    assert pos.dtype == np.float64 and pw.dtype == np.float64 and pos.shape == pw.shape == (N,)
    assert (pos == np.floor(pos)).all() and pos.min() >= -1 and pos.max() <= L - W
    assert np.isfinite(pw).all()
    _bench(tmp_path / "b", 4)
    for name in ("positions", "pwms"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"),
                              np.load(tmp_path / "b" / f"{name}.npy")), name
    # --steps sets the timed sweeps: one more sweep (fresh draws, a resampled start for
    # every sequence) ends in another state
    assert _bench(tmp_path / "c", 5)["steps"] == 5
    assert not np.array_equal(pos, np.load(tmp_path / "c" / "positions.npy"))
    assert not np.array_equal(pw, np.load(tmp_path / "c" / "pwms.npy"))
