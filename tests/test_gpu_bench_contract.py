"""The driver's contract with bench.py, checked on an MI355X: `python bench.py --steps K --warmup W` prints ONE JSON line
on stdout with the agreed keys (metric / value / unit / n_gpus / steps / warmup / ms_per_step / higher_is_better / scaling /
vs_baseline / dtype / data / config.workload), `value` consistent with `ms_per_step`; with --full also the `roofline` and
`cpu_baseline` objects, the roofline fraction a fraction; --dump-outputs writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_line_contract():
    # (--no-batch1: without the information-only legs `batch1` / `c3_regime` / `c4` / `config5`, which are best-effort
    # objects behind try / except -- tools/profile_r06.sh runs the whole --full line; this test keeps the GPU suite short)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--cpu-iters",
                        "1", "--cpu-pairs", "1", "--no-batch1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines  # exactly one line on stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "BASELINE.json configs[1]" in d["config"]["workload"] and "model" not in d["config"]
    pairs = d["config"]["pairs_per_gpu_per_step"]
    assert abs(d["value"] - pairs / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]  # value = pairs / time
    assert 300 < d["value"] < 5000
    roof = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in roof, key
    assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 157.3
    assert 0.3 < roof["frac"] <= 1.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert roof["launches_timed"] == 18 * 3  # live HIP events around every attention launch of the timed region
    cpu = d["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in cpu, key
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] >= 1
    assert d["self_check"]["pairs_equal"] is True and d["self_check"]["keypoint_sets_equal"] is True
    assert not any(k in d for k in ("batch1", "c3_regime", "c4", "config5"))  # skipped by --no-batch1
    # every rank's own numbers ride on the line (one row at N = 1): the N > 1 line explains itself
    per = d["config"]["per_rank"]
    assert len(per) == 1 and per[0]["rank"] == 0 and d["config"]["rccl_ranks"] == 1
    assert 0 < per[0]["busy_s"] <= per[0]["elapsed_s"] and abs(per[0]["elapsed_s"] - d["ms_per_step"] * 3e-3) < 1e-3
    assert abs(per[0]["attention_avg_launch_ms"] - roof["avg_launch_ms"]) < 1e-3 and per[0]["stem_avg_launch_ms"] > 0
    assert per[0]["probe_tflops"] == roof["sustained_mfma_probe"]["tflops"] and 1.0 < per[0]["probe_shader_clock_ghz"] < 2.6
    assert d["config"]["per_rank_summary"]["busy_s"] == [per[0]["busy_s"]] * 3


def test_plain_bench_line_and_dump_outputs(tmp_path):
    """The plain command: the headline keys, nothing measured beyond them, and --dump-outputs writing the last timed
    step's outputs (float32 / float64, at most 64 MB; the large arrays as a fixed sample of rows)."""
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "image-pairs/sec" and d["dtype"] == "f32" and "1024 kpts, 640x480" in d["metric"]
    pairs = d["config"]["pairs_per_gpu_per_step"]
    assert abs(d["value"] - pairs / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"] and 300 < d["value"] < 5000
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert not any(k in d for k in ("self_check", "batch1", "c3_regime", "c4", "config5"))
    assert abs(d["config"]["per_rank"][0]["elapsed_s"] - d["ms_per_step"] * 2e-3) < 1e-3
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert not any("_time_ms" in name for name in files)  # host timings are not outputs to compare
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64e6
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    for name in ("keypoints0", "keypoints1", "keypoint_scores0", "matches0", "matches1", "matching_scores0"):
        assert files[name].shape[:2] == (pairs, 1024), name
    assert files["keypoints0"].shape == (pairs, 1024, 2)
    m0 = files["matches0"]
    assert (m0 == np.round(m0)).all() and m0.min() >= -1 and m0.max() < 1024
    assert abs(float((m0 >= 0).sum()) / pairs - d["config"]["mean_matches_per_pair"]) < 0.1
    for name in ("descriptors0", "descriptors1"):
        rows = files[name + "_rows"].astype(np.int64)
        assert files[name].shape == (len(rows), 256) and 0 < len(rows) < pairs * 1024
        assert np.allclose(np.linalg.norm(files[name], axis=1), 1.0, atol=1e-4)  # L2-normalised descriptor rows
