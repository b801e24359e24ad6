"""bench.py's plain run (the headline alone) and --dump-outputs: what the timed path computed, written as .npy files that two builds
can compare output for output."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--config", "C4", "--N", "2000", "--P", "6400", "--steps", "8", "--warmup", "1"]
FULL_ONLY = ("roofline", "effective_samples", "compact_storage", "chains_per_gpu", "chains_per_pass", "cpu_baseline", "speedup_vs_cpu_baseline")


def _load(folder):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(folder, "*.npy")))}


def test_dump_keeps_a_fixed_sample_within_the_limit(tmp_path):
    """Outputs beyond the limit: every long array keeps the same seeded positions, in order; short ones are written whole.
    (In a child process: importing bench.py sets environment defaults meant for a benchmark process.)"""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); import bench\n"
            "a = np.arange(100000, dtype=np.float64); d = np.arange(100000, dtype=np.int64) % 2\n"
            "for f in sys.argv[2:]:\n"
            "    bench.dump_outputs(f, {'a': a, 'd': d, 'v': [2.5], 'w': np.ones(3, np.float32)}, limit=200000)\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(tmp_path / "x"), str(tmp_path / "y")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    x, y = _load(tmp_path / "x"), _load(tmp_path / "y")
    assert sorted(x) == ["a", "d", "v", "w"]
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "x" / "*.npy"))) <= 200000
    assert all(v.dtype == np.float64 for v in x.values())
    assert x["v"].tolist() == [2.5] and x["w"].tolist() == [1.0, 1.0, 1.0]
    a = x["a"]
    assert 1000 < a.size < 100000 and np.all(np.diff(a) > 0) and np.all(a == np.floor(a))   # positions of arange, sorted
    assert np.array_equal(x["d"], a % 2)                                                  # the same positions in every array
    assert all(np.array_equal(x[k], y[k]) for k in x)                                     # and in every run


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_its_outputs_repeat(tmp_path):
    """A plain run prints the headline fields and none of --full's; its dump equals that of a --full run with the same arguments
    (the inputs are seeded and --full works after the outputs are taken)."""
    runs = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline", "--no-compact", "--chains-per-pass", "0"])):
        folder = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + extra + ["--dump-outputs", str(folder)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        runs[name] = (json.loads(lines[0]), _load(folder), folder)
    d, out, folder = runs["plain"]
    assert d["metric"] == "gibbs_iterations_per_sec" and d["unit"] == "it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 8 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["pooled_kept_samples"] == 8
    assert d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    assert "roofline" in runs["full"][0] and "effective_samples" in runs["full"][0]
    assert sum(os.path.getsize(f) for f in glob.glob(str(folder / "*.npy"))) <= 64 << 20
    assert {"ycorr", "beta", "delta", "varE", "post_beta", "post_varE"} <= set(out)
    assert out["ycorr"].shape == (2000,) and out["beta"].shape == (6400,) and out["post_beta"].shape == (6400,)
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in out.values())
    assert out["post_varE"][0] == d["posterior_mean_varE"] and out["varE"][0] > 0
    full = runs["full"][1]
    assert sorted(full) == sorted(out) and all(np.array_equal(out[k], full[k]) for k in out), \
        [k for k in out if not np.array_equal(out[k], full[k])]
