"""GPU: a plain `python bench.py --gpus 1 --steps K --warmup W` run prints the headline line only (everything else the
benchmark measures is behind `--full`), and `--dump-outputs DIR` writes what the last timed step computed -- the same
arrays from run to run, since the inputs are seeded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, timeout=300):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    out = {}
    for f in sorted(os.listdir(d)):
        a = np.load(os.path.join(d, f))
        assert a.dtype in (np.float32, np.float64), (f, a.dtype)
        out[f[:-4]] = a
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_plain_inference_run_dumps_the_last_step_reproducibly(tmp_path):
    runs = []
    for tag in ("a", "b"):
        r = _bench(["--steps", "3", "--warmup", "1", "--batch", "4", "--dump-outputs", str(tmp_path / tag)])
        assert all(k in r for k in HEADLINE) and r["steps"] == 3 and r["warmup"] == 1
        assert r["value"] > 0 and r["ms_per_step"] > 0 and r["higher_is_better"] is True and r["dtype"] == "bf16"
        for k in ("roofline", "decode", "pcie_inclusive", "batch_consistency", "cpu_baseline", "bf16_agreement"):
            assert k not in r, k
        assert r["value_windows"]["n"] == 1
        runs.append(_load(tmp_path / tag))
    a, b = runs
    assert sorted(a) == ["bbox", "count", "kp_cell", "limb_arg", "score"]
    assert a["count"].shape == (4,) and a["count"].sum() > 0
    n = a["kp_cell"].shape[1]
    assert a["kp_cell"].shape == (4, n, 18) and a["limb_arg"].shape == (4, n, 17) and a["bbox"].shape == (4, n, 18, 4)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_plain_training_run_dumps_losses_and_weights(tmp_path):
    r = _bench(["--workload", "train", "--steps", "2", "--warmup", "1", "--batch", "4",
                "--dump-outputs", str(tmp_path)])
    assert all(k in r for k in HEADLINE) and r["steps"] == 2 and "cpu_baseline" not in r
    d = _load(tmp_path)
    assert sorted(d) == ["losses", "params_sample", "task_weights"]
    assert np.allclose(d["losses"], r["losses"], atol=1e-4) and np.isfinite(d["params_sample"]).all()
    assert abs(float(d["task_weights"].sum()) - 5.0) < 1e-2
