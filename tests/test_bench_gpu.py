"""bench.py as every change runs it: a plain run measures the headline alone and prints ONE JSON line, and
--dump-outputs writes what the last timed step returned -- the same arrays from run to run with the same arguments, so
that two builds can be compared output for output.  (The --full side metrics: test_dp_gpu.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = dict(os.environ)
    env.pop("SRK_ENV_LIVE", None)     # the product configuration: switches read once
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_is_the_headline_and_dumps_its_last_step(gpu, tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--lr-size", "64"]
    recs, outs = [], []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        recs.append(_bench(args + ["--dump-outputs", d]))
        assert sorted(os.listdir(d)) == ["espcn_x4_hr.npy"]
        outs.append(np.load(os.path.join(d, "espcn_x4_hr.npy")))
    rec = recs[0]
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"]
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps (batch 4 per step)
    assert abs(4 * 1e3 / rec["ms_per_step"] - rec["value"]) <= 1e-2 * rec["value"], rec
    assert not set(rec) & {"extra", "roofline", "cpu_baseline"}, sorted(rec)
    a, b = outs
    assert a.dtype == np.float32 and a.shape == (4, 3, 4 * (64 - 8), 4 * (64 - 8)) and a.nbytes <= 64e6
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert np.array_equal(a, b)
