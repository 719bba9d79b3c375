"""bench.py's launch contract on CPU: `python bench.py --gpus N` without a launcher spawns
its own ranks the way the driver does (torch.distributed.run, 127.0.0.1), rank 0 prints ONE JSON line; without enough devices
it fails with that message and not with launch instructions.  --dry-run = the scaffolding only (gloo, no device, no kernels)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), cwd=ROOT, env=e, capture_output=True,
                          text=True, timeout=300)


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def test_plain_launch_with_two_ranks_spawns_itself():
    r = _run("--gpus", "2", "--dry-run", "--steps", "4", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    assert lines[0]["n_gpus"] == 2 and lines[0]["world_size"] == 2 and lines[0]["dry_run"] is True
    assert lines[0]["steps"] == 4 and lines[0]["warmup"] == 1 and lines[0]["value"] is None
    # N > 1 times BASELINE.json configs[3] (B=64 over 8 GPUs: 8 per GPU, S=8192), not the single-GPU headline's batch
    assert lines[0]["config"]["workload"].startswith("c4: B=8/GPU Hq=32 Hkv=32 Sq=8192 Sk=8192 D=128 bf16 causal fwd"), lines[0]["config"]


def test_dry_run_one_rank_needs_no_launcher():
    r = _run("--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["world_size"] == 1
    assert lines[0]["config"]["workload"].startswith("c2: B=4/GPU Hq=32 Hkv=32 Sq=4096 Sk=4096 D=128 bf16 causal fwd"), lines[0]["config"]


def test_launcher_with_wrong_rank_count_is_refused():
    # the driver's command shape with 2 ranks but --gpus 3: every rank refuses, nothing hangs
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                        "127.0.0.1", "--master-port", "29531", os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-run"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "--gpus 3 but the launcher made 2 rank(s)" in r.stderr + r.stdout


def test_without_devices_the_message_names_the_device_count():
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box has two devices")
    r = _run("--gpus", "2", "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert "needs 2 devices" in r.stderr + r.stdout
    assert "torch.distributed.run" not in r.stderr + r.stdout


def test_plain_launch_with_eight_ranks_names_c4_and_its_shards():
    """The driver's scaling run at its widest: 8 ranks rendezvous on 127.0.0.1, time, reduce MAX over ranks, and
    rank 0 prints one line for BASELINE configs[3] -- B = 64 over 8 GPUs, 8 per GPU, 512 MiB of output per rank, 4 GiB gathered."""
    r = _run("--gpus", "8", "--dry-run", "--steps", "3", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    rec = lines[0]
    assert rec["n_gpus"] == 8 and rec["world_size"] == 8 and rec["dry_run"] is True and rec["steps"] == 3
    assert rec["config"]["workload"].startswith("c4: B=8/GPU Hq=32 Hkv=32 Sq=8192 Sk=8192 D=128 bf16 causal fwd"), rec["config"]
    assert rec["gather_plan"] == {"bytes_per_rank": [512 << 20] * 8, "total_bytes": 4 << 30, "shard": "batch"}


def test_a_hung_exchange_section_still_prints_the_line():
    """The output-exchange variants have never met N > 1 GPUs: if one of them hangs (here: a barrier rank 1 never joins), the watchdog
    prints the contract's line with the reason and the process ends with status 0 -- the scaling record survives."""
    r = _run("--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "0", env={"AULE_BENCH_TEST_HANG": "1", "AULE_BENCH_GATHER_TIMEOUT": "3"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout
    assert lines[0]["world_size"] == 2 and "error" in lines[0]["gather"], lines[0]


def test_dump_outputs_whole_and_sampled(tmp_path):
    """--dump-outputs' writer: float32 .npy files, whole arrays when they fit the budget, otherwise the same fixed, seeded
    sample of rows from run to run, the budget shared in proportion to size and never exceeded."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    a = torch.randn(2, 3, 40, 16, generator=g, dtype=torch.float64).to(torch.bfloat16)
    b = torch.randn(2, 1, 40, 16, generator=g)
    rec = bench.dump_outputs(str(tmp_path / "whole"), [("a", a), ("b", b)])
    assert rec["a"] == {"shape": [2, 3, 40, 16], "rows": 240, "rows_kept": 240}
    for name, t in (("a", a), ("b", b)):
        x = np.load(str(tmp_path / "whole" / (name + ".npy")))
        assert x.dtype == np.float32 and x.shape == tuple(t.shape)
        assert np.array_equal(x, t.float().numpy())
    budget = 4 * 16 * 100          # room for 100 of the 320 rows
    rec1 = bench.dump_outputs(str(tmp_path / "s1"), [("a", a), ("b", b)], budget=budget)
    rec2 = bench.dump_outputs(str(tmp_path / "s2"), [("a", a), ("b", b)], budget=budget)
    assert rec1 == rec2 and rec1["a"]["rows_kept"] == 75 and rec1["b"]["rows_kept"] == 25
    total = 0
    for name, t in (("a", a), ("b", b)):
        x1, x2 = (np.load(str(tmp_path / d / (name + ".npy"))) for d in ("s1", "s2"))
        assert x1.dtype == np.float32 and x1.shape == (rec1[name]["rows_kept"], 16) and np.array_equal(x1, x2)
        rows = t.float().reshape(-1, 16).numpy()
        # every sampled row is a row of the array, in ascending row order
        idx = [int(np.flatnonzero((rows == r).all(axis=1))[0]) for r in x1]
        assert idx == sorted(set(idx))
        total += x1.nbytes
    assert total <= budget


def test_full_and_dump_outputs_are_options():
    r = _run("--help")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    # the launch scaffolding takes both (a dry run computes nothing, so it writes nothing)
    r = _run("--gpus", "1", "--dry-run", "--steps", "2", "--warmup", "0", "--full", "--dump-outputs", os.devnull)
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(_json_lines(r.stdout)) == 1
