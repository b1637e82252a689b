"""bench.py as the driver runs it (no --full): set-up, warm-up, the K timed steps and the headline line only; --dump-outputs
writes what the last timed step computed, and two runs with the same arguments write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    d = _bench(tmp_path / "a")
    assert d["metric"].startswith("scans/sec") and d["unit"] == "scans/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["units_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "parity", "cpu_baseline", "single_stream", "sustained", "instrumented", "other_configs"):
        assert k not in d, k                                   # measured with --full only
    names = ("poses", "T", "iters", "pmap", "pmap_index")
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in names)
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in names) <= 64 << 20
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    L = d["config"]["trajectories_per_step"]
    assert a["poses"].shape == (L, 999, 3) and a["poses"].dtype == np.float64 and a["T"].shape == (L, 999, 3, 3)
    assert a["iters"].shape == (L, 999) and a["iters"].min() >= 1 and a["iters"].max() <= 30
    assert a["pmap"].shape == (L, 400, 400) and set(np.unique(a["pmap"]).tolist()) == {0.0, 50.0, 100.0}
    assert np.array_equal(a["pmap_index"], np.arange(L))
    _bench(tmp_path / "b")                                     # the same arguments again: the same inputs, the same outputs
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in names}
    for k in ("iters", "pmap", "pmap_index"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("poses", "T"):
        assert np.max(np.abs(a[k] - b[k])) < 1e-12, k
