"""bench.py's plain run on the device: exactly --steps timed steps, the line's headline fields, none of what --full adds, and
--dump-outputs: the last timed step's outputs as float32 .npy files, the same from run to run (same seeded inputs, kernels
without atomics), within the size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ("steady_state", "extra", "limiter", "cpu_baseline", "gather")


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _check_line(rec, steps, dtype):
    assert rec["steps"] == steps and rec["legs"]["value"]["steps"] == steps
    assert rec["unit"] == "TFLOP/s" and rec["higher_is_better"] is True and rec["dtype"] == dtype
    assert rec["metric"].startswith("attention TFLOPS/GPU") and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert not any(k in rec for k in FULL_ONLY), sorted(rec)


def _load(d, names):
    out = {}
    for n in names:
        x = np.load(os.path.join(d, n + ".npy"))
        assert x.dtype == np.float32 and np.isfinite(x).all(), n
        out[n] = x
    assert sum(os.path.getsize(os.path.join(d, n + ".npy")) for n in names) <= 64 << 20
    return out


def test_plain_forward_dumps_the_same_outputs_twice(tmp_path):
    # C2 at B = 1: O is 64 MiB in float32, above the budget -> a seeded sample of its rows
    args = ["--gpus", "1", "--batch", "1", "--steps", "3", "--warmup", "1"]
    recs = [_bench(*args, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for rec in recs:
        _check_line(rec, 3, "bf16")
        assert rec["outputs"]["arrays"]["out"]["shape"] == [1, 32, 4096, 128]
        assert 0 < rec["outputs"]["arrays"]["out"]["rows_kept"] < 32 * 4096
    a, b = (_load(str(tmp_path / d), ["out"]) for d in ("a", "b"))
    assert a["out"].shape == (recs[0]["outputs"]["arrays"]["out"]["rows_kept"], 128)
    assert np.array_equal(a["out"], b["out"]) and np.abs(a["out"]).max() > 0


def test_plain_fwd_bwd_dumps_output_and_gradients(tmp_path):
    rec = _bench("--gpus", "1", "--config", "c3", "--batch", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    _check_line(rec, 2, "bf16")
    arr = rec["outputs"]["arrays"]
    assert arr["out"]["shape"] == arr["dq"]["shape"] == [1, 32, 2048, 128] and arr["dk"]["shape"] == [1, 8, 2048, 128]
    got = _load(str(tmp_path), ["out", "dq", "dk", "dv"])
    assert all(np.abs(x).max() > 0 for x in got.values())
