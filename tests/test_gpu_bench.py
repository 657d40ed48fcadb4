"""bench.py's command line: a plain run prints the headline line only, `--dump-outputs DIR` writes the
last timed step's outputs as float64 .npy files, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--homes", "64"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_reproducible_outputs(gpu, tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(d)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for d in dirs]
    outs = [p.communicate(timeout=120) for p in procs]
    for p, (_, err) in zip(procs, outs):
        assert p.returncode == 0, err[-2000:]
    line = json.loads(outs[0][0].strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(64 * 3 / (3 * line["ms_per_step"] * 1e-3))
    assert (line["metric"], line["unit"], line["higher_is_better"], line["dtype"]) == (
        "home-MPC solves/sec (homes x steps)", "solves/s", True, "f64")
    for k in ("roofline", "cpu_baseline", "status_counts", "occupancy"):      # behind --full
        assert k not in line
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    masked = ["agg_sums", "vals", "fc", "history_row"]        # absent hash fields: 0, marked in <name>_present
    assert {f"{n}.npy" for n in masked + ["homes", "status", "int_path"]} | {f"{n}_present.npy" for n in masked} == set(names)
    total = 0
    for f in names:
        a, b = np.load(dirs[0] / f), np.load(dirs[1] / f)
        assert a.dtype == (np.float32 if f.endswith("_present.npy") else np.float64), f
        assert np.isfinite(a).all() and np.array_equal(a, b), f
        total += os.path.getsize(dirs[0] / f)
    assert total <= 64e6
    for n in masked:
        a, m = np.load(dirs[0] / f"{n}.npy"), np.load(dirs[0] / f"{n}_present.npy")
        assert a.shape == m.shape and set(np.unique(m)) <= {0.0, 1.0} and not a[m == 0].any(), n
    assert np.load(dirs[0] / "agg_sums.npy").shape == (3,) and np.load(dirs[0] / "homes.npy").tolist() == list(range(64))
    assert np.load(dirs[0] / "agg_sums_present.npy").all() and np.load(dirs[0] / "fc_present.npy").any()
    assert np.load(dirs[0] / "vals.npy").shape[1] == 64 and np.load(dirs[0] / "fc.npy").shape[2] == 64
