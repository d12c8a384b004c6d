"""bench.py's own contract on one GPU: a plain run times exactly --steps steps, prints the line without the --full extras and writes no
detail file; --dump-outputs writes what the last timed step computed, the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"features": (8, 4096, 64), "loss": (1,), "grads": None, "params": None, "bn_moving_stats": None}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    return json.loads(lines[-1])


def _load(d):
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in DUMPED)
    out = {n: np.load(os.path.join(d, n + ".npy")) for n in DUMPED}
    for n, a in out.items():
        assert a.dtype == np.float32 and bool(np.isfinite(a).all()), n
        if DUMPED[n] is not None:
            assert a.shape == DUMPED[n], (n, a.shape)
    assert out["grads"].shape == out["params"].shape and out["grads"].size > 0
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    return out


def test_plain_run_and_dumped_outputs(tmp_path):
    lines, dumps = [], []
    for run in ("a", "b"):
        lines.append(_bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / run)))
        dumps.append(_load(tmp_path / run))
    for line in lines:
        assert line["steps"] == 3 and line["warmup"] == 2 and line["n_gpus"] == 1
        assert line["unit"] == "scenes/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(8 * 1e3 / line["ms_per_step"], rel=1e-4)
        assert line["cpu_baseline"] is None and line["detail_file"] is None and line["roofline"]["avg_launch_ms"] is None     # --full only
    a, b = dumps
    # same inputs, same weights: run-to-run differences can only come from the order of atomic gradient sums (in earlier steps' updates too)
    np.testing.assert_allclose(a["features"], b["features"], rtol=1e-4, atol=1e-5)
    for n in ("loss", "grads", "params", "bn_moving_stats"):
        np.testing.assert_allclose(a[n], b[n], rtol=1e-4, atol=1e-7, err_msg=n)
