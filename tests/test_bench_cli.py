"""bench.py's command line: a plain run prints the headline alone and times exactly --steps steps; --dump-outputs writes what the
timed path returned to its caller (the same matrix from run to run, and the same as a --full run's); --full carries the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_samples_rows_above_the_cap(tmp_path, monkeypatch):
    bench = _bench_module()
    m = np.random.RandomState(3).standard_normal((300, 40))
    bench.dump_outputs(str(tmp_path / "small"), m)
    assert sorted(os.listdir(tmp_path / "small")) == ["influence_matrix.npy"]
    got = np.load(tmp_path / "small" / "influence_matrix.npy")
    assert got.dtype == np.float64 and np.array_equal(got, m)

    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 32 * (40 + 1) * 8)      # room for 32 rows of 40 values and their indices
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), m)
    rows = np.load(tmp_path / "a" / "influence_matrix_rows.npy")
    got = np.load(tmp_path / "a" / "influence_matrix.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float64
    assert got.nbytes + rows.nbytes <= bench.DUMP_CAP_BYTES and len(rows) == 32
    assert np.all(np.diff(rows) > 0) and np.array_equal(got, m[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "influence_matrix_rows.npy"))          # a fixed, seeded sample
    assert np.array_equal(got, np.load(tmp_path / "b" / "influence_matrix.npy"))


def _run(args, env=None, timeout=600):
    e = dict(os.environ, PYTHONPATH=REPO, **(env or {}))
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_outputs(gpu, tmp_path):
    """Two plain runs with the same arguments: one timed block of exactly --steps steps, the headline keys only, and the same
    [n_test, n_test] float64 matrix written by both -- the matrix a --full run's headline steps return, and the fp32 device
    matrix of its device-resident steps widened."""
    plain = ["--gpus", "1", "--steps", "7", "--warmup", "2"]
    one = _run(plain + ["--dump-outputs", str(tmp_path / "one")])
    two = _run(plain + ["--dump-outputs", str(tmp_path / "two")])
    for line in (one, two):
        assert line["metric"] == "influence-matrix node-pairs/sec" and line["unit"] == "node-pairs/s"
        assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["n_gpus"] == 1
        assert line["steps"] == 7 and line["warmup"] == 2 and line["timing"]["blocks"] == 1
        ms = line["timing"]["block_ms"][0] / 7
        assert line["ms_per_step"] > 0 and abs(line["ms_per_step"] - ms) <= 1e-3 * ms + 1e-3
        assert abs(line["value"] - 500 * 500 / (ms * 1e-3)) <= 1e-2 * line["value"]
        for key in ("kernels", "roofline", "parity", "cpu_baseline", "api_wall", "value_device", "collectives"):
            assert key not in line, key
    a = np.load(tmp_path / "one" / "influence_matrix.npy")
    assert a.dtype == np.float64 and a.shape == (500, 500) and np.abs(a).max() > 0
    assert np.array_equal(a, np.load(tmp_path / "two" / "influence_matrix.npy"))

    full = _run(["--full", "--steps", "7", "--warmup", "2", "--blocks", "1", "--no-cpu-baseline", "--no-extras", "--no-pmc",
                 "--no-api-wall", "--no-scaling-workloads", "--dump-outputs", str(tmp_path / "full")],
                {"LT_BENCH_DUMP": str(tmp_path / "device.npy")})
    assert full["host_matrix_equals_device_matrix"] is True and "kernels" in full
    assert np.array_equal(a, np.load(tmp_path / "full" / "influence_matrix.npy"))
    assert np.array_equal(a, np.load(tmp_path / "device.npy").astype(np.float64))
