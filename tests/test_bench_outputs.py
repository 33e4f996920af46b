"""bench.py's outputs on the CPU stand-in of tests/bench_rehearsal.py (one process, the numpy engine): --steps is the
number of timed steps behind `ms_per_step`, --dump-outputs writes what the last timed step returned, the same
numbers from run to run and with --full, and a plain run's line carries the headline only."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

J = 64


def _bench(tmp_path, tag, *extra):
    env = dict(os.environ, CESX_BENCH_PREWARM_S="0", OMP_NUM_THREADS="2",
               BENCH_REHEARSAL_ARGS="--p 8 --n 6 --J %d --dtype float64 --no-extras" % J)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CESX_FORCE_COLLECTIVES"):
        env.pop(k, None)
    out = tmp_path / tag
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bench_rehearsal.py"), "--steps", "4", "--warmup", "1",
                          "--dump-outputs", str(out)] + list(extra), env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_bench_dump_outputs_and_steps(tmp_path):
    rec, first = _bench(tmp_path, "a")
    assert rec["steps"] == 4 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert abs(rec["value"] * rec["ms_per_step"] / (J * 1e3) - 1) < 1e-9          # value = J / (ms_per_step / 1e3)
    assert {"metric", "unit", "higher_is_better", "dtype"} <= set(rec) and rec["higher_is_better"] is True
    assert not {"roofline", "clock", "cpu_baseline", "e2e", "extra", "parity_err"} & set(rec)
    assert set(first) == {"U_next"} | set(bench.RESULT_FIELDS)
    assert first["U_next"].shape == (8, J)
    assert all(a.dtype in (np.float32, np.float64) for a in first.values())
    assert sum(a.nbytes for a in first.values()) <= 64e6
    # the same inputs every run: the same outputs, and --full measures more around the SAME timed path
    _, again = _bench(tmp_path, "b")
    full, with_full = _bench(tmp_path, "c", "--full")
    assert "roofline" in full and "cpu_baseline" in full
    for k, v in first.items():
        assert np.array_equal(v, again[k]) and np.array_equal(v, with_full[k]), k
    # another step count ends on another step
    _, other = _bench(tmp_path, "d", "--steps", "5")
    assert not np.array_equal(first["U_next"], other["U_next"])


def test_dump_outputs_samples_a_large_ensemble(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 8 * 4 * 100)
    U = torch.arange(8 * 1000, dtype=torch.float32).reshape(8, 1000)
    res = types.SimpleNamespace(**{k: float(i) for i, k in enumerate(bench.RESULT_FIELDS)})
    bench.dump_outputs(str(tmp_path / "a"), U, res)
    bench.dump_outputs(str(tmp_path / "b"), U, res)
    a, b = np.load(tmp_path / "a" / "U_next.npy"), np.load(tmp_path / "b" / "U_next.npy")
    assert a.shape == (8, 100) and a.dtype == np.float32 and np.array_equal(a, b)
    cols = a[0].astype(np.int64)                # row 0 of arange holds the column index
    assert np.all(np.diff(cols) > 0) and np.array_equal(a, U.numpy()[:, cols])
    assert float(np.load(tmp_path / "a" / "t_new.npy")) == bench.RESULT_FIELDS.index("t_new")
