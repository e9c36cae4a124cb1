"""bench.py's one-line contract on a small workload: the keys the driver reads, the roofline and CPU-baseline objects of
--full, kernel time per step no larger than the step itself, and the plain run's line and --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, full=True):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "4", "--warmup", "2", "--clips", "96"]
    if full:
        cmd += ["--full", "--cpu-clips", "8", "--cpu-pool-seconds", "0"]
    cmd += list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [(), ("--inflight", "1"), ("--streams", "2"), ("--config", "3"), ("--config", "5")])
def test_bench_line(extra):
    d = _run(*extra)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert "traffic" in r and r["fp32"]["peak"] == 157.3
    assert r["kernel_ms_per_step"] <= d["ms_per_step"] * 1.001          # union of the launch intervals, never more than the step
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "frames/s" and c["sample"]


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    """Without --full: the headline keys only, and --dump-outputs writes the last timed step's per-clip results, the same
    from run to run (the inputs depend only on the arguments)."""
    runs = []
    for name in ("a", "b"):
        d = _run("--dump-outputs", str(tmp_path / name), full=False)
        for k in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
            assert k in d, k
        for k in ("roofline", "cpu_baseline", "host_to_result_frames_per_s", "distinct_batches_frames_per_s"):
            assert k not in d, k
        assert d["steps"] == 4 and d["unit"] == "frames/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
        fpstep = d["config"]["frames_per_gpu_step"]
        assert abs(d["value"] - fpstep / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
        out = {k: np.load(tmp_path / name / (k + ".npy")) for k in ("stats", "status", "trim", "nframes")}
        assert out["stats"].dtype == np.float32 and out["stats"].shape == (96, 4 * 13 + 3)
        assert all(out[k].dtype == np.float64 for k in ("status", "trim", "nframes"))
        assert out["trim"].shape == (96, 2) and out["status"].shape == out["nframes"].shape == (96,)
        assert (out["status"] == 0).all() and out["nframes"].sum() == fpstep
        assert np.isfinite(out["stats"]).all()
        runs.append(out)
    for k in ("status", "trim", "nframes"):
        np.testing.assert_array_equal(runs[0][k], runs[1][k])
    np.testing.assert_allclose(runs[0]["stats"], runs[1]["stats"], rtol=1e-5, atol=1e-5)
