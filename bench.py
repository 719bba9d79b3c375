#!/usr/bin/env python3
"""bench.py -- throughput of the FlashAttention hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4|c5] [--mode fwd|fwdbwd] [--dump-outputs DIR]
                    [--full [--condition-ms MS] [--no-cpu-baseline] [--no-extra]]
    (--config defaults to c2, the single-GPU headline, on one GPU and to c4 -- BASELINE configs[3]: B=64 over 8 GPUs, 8 per GPU, S=8192 -- with --gpus N > 1)

A plain run does what `value` needs and nothing else: set up, W warm-up steps, K timed steps, the outputs of the last timed step
to DIR/<name>.npy if --dump-outputs is given (float32; a fixed, seeded sample of rows where they exceed the size budget), one
JSON line.  Everything else the bench measures -- the conditioned "steady_state" leg, the hwmon power / clock sampler, the output
exchange of N > 1 ranks ("gather"), the other configs and precisions ("extra"), the limiter residencies, the reference harness
vs SDPA and the CPU baseline -- runs with --full only.

One "step" = one pass of the hot path (aule.flash_attention -> libaule.so -> gfx950
kernels) over one batch of synthetic [B,H,S,D] tensors already resident in HBM.
Default workload = BASELINE.json configs[1]:  B=4 H=32 S=4096 D=128 bf16 causal MHA, fwd.
With N > 1 (launched by torch.distributed.run, one rank per GPU, RCCL) every rank runs
configs[3]'s per-GPU batch (B=8 H=32 S=8192) on its own shard (weak scaling, no data-path collective); the
optional output all-gather over xGMI is timed separately and reported under "gather".

Rank 0 prints ONE JSON line.  FLOP convention: fwd = 4*B*Hq*D*P with
P = sum_i min(i+1, Sk) for the top-left causal mask, bwd = 2.5*fwd.

Protocol.  The forward leg runs with autograd enabled, so the kernel stores the log-sum-exp like the reference's forward
always does (python/aule/triton_flash_amd.py:410-432).  `value` is the contract's measurement and nothing else: W untimed
warm-up steps, then EXACTLY K timed steps between barrier + synchronize pairs, taken first, on the chip as the process finds
it.  MI355X clocks to its power budget: from an idle chip the first two launches of this kernel run at boost clock, launches
3-8 collapse to ~1.45x the steady time while the power controller overshoots, and it takes ~60 launches (35-40 ms) to settle
(profiles/r2_dvfs_trace.txt; same curve on every box) -- a 5 + 20 step measurement right after process start sits inside
that transient.  The number a long-running job sees is therefore measured too (--full) and reported SEPARATELY as "steady_state":
the same step repeated for --condition-ms of device time (default 250 ms), then W warm-up + K timed steps again.  (Round 2
printed the conditioned figure as `value` and the plain one as "cold_start"; the two have swapped places.)  Every timed step
has its own HIP event pair: mean, median, min and max per launch are in "roofline".

Round 6 (--full): every leg is a complete measurement.  A sampler thread reads the hwmon files of the device under test (socket power,
shader clock, power cap) every few milliseconds for the whole process; each leg reports the mean power and the mean / minimum
clock of ITS timed window next to the per-step mean, median, minimum and maximum ("legs").  A fwd+bwd step carries an event
between the forward call and `backward()`, so every backward figure (`*_bwd_ms`, `*_bwd_frac`) is the MEDIAN of the backward
segment of the very steps that were timed -- same conditioning, same clock -- and not a difference of two means taken minutes
apart; the difference against a fwd-only leg run right behind it rides along as `*_bwd_ms_by_difference`.  `roofline.power_w` /
`sclk_mhz` are measured in the timed window of this run; `traffic` stays the stored figure of the last PMC-profiled run.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "aule-attention_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# gfx950 dense peaks (MI355X_MICROARCH.md: 256 CU x 4 SIMD x 1024 FLOP/clk x 2.4 GHz; "~2.5 PF dense")
PEAK_TFLOPS = {"bf16": 2516.6, "fp16": 2516.6, "fp32": 157.3}

CONFIGS = {
    # name: (B per GPU, Hq, Hkv, Sq, Sk, D, dtype, causal, default mode)
    "c2": (4, 32, 32, 4096, 4096, 128, "bf16", True, "fwd"),      # configs[1] -- the headline
    "c3": (4, 32, 8, 2048, 2048, 128, "bf16", True, "fwdbwd"),    # configs[2] (B=4 assumed)
    "c4": (8, 32, 32, 8192, 8192, 128, "bf16", True, "fwd"),      # configs[3]: B=64 over 8 GPUs
    "c5": (1, 32, 1, 16384, 16384, 64, "fp16", False, "fwd"),     # configs[4]
    # SURVEY 8d note: the genuinely HBM-bound cross-attention points that bracket the regime configs[4] is labelled with
    # c5b / c5c: K+V is 4 MB, resident in L2 / the Infinity Cache across steps -- their "hbm" roofline entry is the
    # algorithmic byte rate of a launch-bound call, not DRAM traffic (tools/bench_decode_ws.py has the HBM rates)
    "c5b": (1, 32, 1, 1, 16384, 64, "fp16", False, "fwd"),        # decode-like: AI = 32 FLOP/B
    "c5c": (1, 32, 1, 64, 16384, 64, "fp16", False, "fwd"),       # AI ~ 1800 FLOP/B
}
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E ~8 TB/s
RIDGE = 315.0           # FLOP/B where the bf16/fp16 MFMA roof meets the HBM roof


def causal_pairs(Sq, Sk):
    n = min(Sq, Sk)
    return n * (n + 1) // 2 + max(0, Sq - Sk) * Sk


def fwd_flops(B, Hq, Sq, Sk, D, causal):
    P = causal_pairs(Sq, Sk) if causal else Sq * Sk
    return 4.0 * B * Hq * D * P


def stored_profile(config, mode):
    """What the LAST rocprofv3 run of this workload recorded (tools/profile.sh -> profiles/hbm_traffic.json): HBM bytes per
    launch from the PMC passes (FETCH_SIZE x2 per the gfx950 note in MI355X_MICROARCH.md, + WRITE_SIZE) and the effective
    clock (GRBM_GUI_ACTIVE / 8 XCDs / kernel time).  STORED figures of a profiled run, not measurements of this one."""
    try:
        with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as fh:
            return json.load(fh).get("%s_%s" % (config, mode), {})
    except (OSError, ValueError):
        return {}


def hbm_traffic(config, mode):
    return stored_profile(config, mode).get("bytes_per_launch")


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(budget_s=10.0):
    """The oracle's NumPy restatement of the reference CPU path (python/aule/__init__.py:247-271) on this box's host cores,
    by SURVEY.md 8d's protocol: config C1 exactly (B1 H8 S256 D64 fp32 causal; 3 warm-ups, median of 20) is `value`; one
    larger point that still fits the O(S^2) temporaries (B1 H8 S2048 D64) and a bounded sample of the bench workload itself
    (one batch element, 2 of the 32 heads of C2) ride along as structured fields.  BLAS thread settings are left at their
    defaults and printed; `cores` = CPU time / wall time of the C1 loop (the threads actually busy)."""
    import numpy as np
    import oracle
    rng = np.random.RandomState(0)

    def point(B, H, S, D, warm, reps, budget=None):
        q, k, v = (rng.randn(B, H, S, D).astype(np.float32) for _ in range(3))
        for _ in range(warm):
            oracle.cpu_attention(q, k, v, True)
        ts, c0, w0 = [], time.process_time(), time.perf_counter()
        for _ in range(reps):
            a = time.perf_counter()
            oracle.cpu_attention(q, k, v, True)
            ts.append(time.perf_counter() - a)
            if budget is not None and time.perf_counter() - w0 > budget:
                break
        wall, cpu = time.perf_counter() - w0, time.process_time() - c0
        med = sorted(ts)[len(ts) // 2]
        fl = fwd_flops(B, H, S, S, D, True)
        return {"shape": "B%d H%d S%d D%d fp32 causal" % (B, H, S, D), "reps": len(ts), "warmups": warm, "median_ms": med * 1e3,
                "tflops": fl / med / 1e12, "flops": fl, "threads_busy": round(cpu / wall, 2)}

    c1 = point(1, 8, 256, 64, 3, 20)
    big = point(1, 8, 2048, 64, 1, 5, budget=budget_s / 2)
    c2s = point(1, 2, 4096, 128, 0, 4, budget=budget_s / 2)
    return {
        "value": c1["tflops"],
        "unit": "TFLOP/s",
        "cores": max(1, int(round(c1["threads_busy"]))),
        "host_cores": os.cpu_count(),
        "cpu_model": _cpu_model(),
        "blas_threads": {k: os.environ.get(k, "default") for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS")},
        "kind": "port",
        "sample": "numpy restatement of _cpu_attention (oracle.cpu_attention) at config C1 exactly: B1 H8 S256 D64 fp32 causal, "
                  "3 warm-ups, median of 20 = %.2f ms (the reference's own code took 40.6 ms on 8 Xeon cores, BASELINE.md)" % c1["median_ms"],
        "c1": c1,
        "b1_h8_s2048_d64": big,
        "c2_sample": c2s,
    }


class Telemetry:
    """hwmon of the device under test, sampled by a daemon thread for the whole process: socket power (power1_input, else
    power1_average; microwatts), shader clock (freq1_input; Hz), power cap (power1_cap).  The device is found by its PCI address
    (torch's device properties -> /sys/bus/pci/devices/<domain:bus:device.0>/hwmon/hwmon*): with several cards on a node every
    rank reads its own.  A leg asks for the statistics of a [t0, t1] window of time.perf_counter().  No file, no permission
    or no samples -> every statistic is None and `source` says why; the bench never fails on telemetry.  enabled=False (a plain
    run): no thread, every statistic None."""

    PERIOD_S = 0.004

    def __init__(self, torch, index, enabled=True):
        self.rows, self.hw, self.source, self.cap_w, self.label, self.bdf = [], None, None, None, None, None
        if not enabled:
            self.source = "not sampled (plain run; --full samples hwmon)"
            return
        import glob
        try:
            pr = torch.cuda.get_device_properties(index)
            bdf = self.bdf = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            cand = sorted(glob.glob("/sys/bus/pci/devices/%s/hwmon/hwmon*" % bdf))
            how = "pci " + bdf
            if not cand:
                cand = sorted(h for h in glob.glob("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*") if "-" not in h.split("/")[4])
                how = "the only card with hwmon power" if len(cand) == 1 else None
                if len(cand) != 1:
                    self.source = "no hwmon directory for %s and %d candidate cards" % (bdf, len(cand))
                    return
            self.hw = cand[0]
            self.pfile = next((self.hw + "/" + f for f in ("power1_input", "power1_average") if os.path.exists(self.hw + "/" + f)), None)
            self.ffile = self.hw + "/freq1_input" if os.path.exists(self.hw + "/freq1_input") else None
            if self.pfile is None:
                self.hw, self.source = None, "%s has no power1_input / power1_average" % cand[0]
                return
            self.cap_w = self._rd(self.hw + "/power1_cap", 1e-6)
            try:
                with open(self.hw + "/power1_label") as fh:
                    self.label = fh.read().strip()
            except OSError:
                pass
            self.source = "hwmon %s (%s), %s + %s every %.0f ms" % (self.hw, how, os.path.basename(self.pfile),
                                                                    os.path.basename(self.ffile) if self.ffile else "no clock file", self.PERIOD_S * 1e3)
        except Exception as e:   # noqa: BLE001
            self.hw, self.source = None, "telemetry unavailable: %s: %s" % (type(e).__name__, str(e)[:120])
            return
        import threading
        self._stop = False
        self.th = threading.Thread(target=self._loop, daemon=True)
        self.th.start()

    @staticmethod
    def _rd(path, k):
        try:
            with open(path) as fh:
                return float(fh.read().split()[0]) * k
        except (OSError, ValueError, IndexError):
            return None

    def _loop(self):
        while not self._stop:
            t = time.perf_counter()
            p = self._rd(self.pfile, 1e-6)
            f = self._rd(self.ffile, 1e-6) if self.ffile else None
            self.rows.append((0.5 * (t + time.perf_counter()), p, f))
            time.sleep(self.PERIOD_S)

    def window(self, t0, t1):
        """{power_w, power_w_max, sclk_mhz, sclk_mhz_min, samples} over the samples taken in [t0, t1]; a window shorter than the
        sampling period takes the one sample nearest to its middle (samples = 1, flagged)."""
        out = {"power_w": None, "power_w_max": None, "sclk_mhz": None, "sclk_mhz_min": None, "power_cap_w": self.cap_w, "samples": 0}
        if self.hw is None or not self.rows:
            return out
        rows = [r for r in self.rows if t0 <= r[0] <= t1]
        if not rows:
            mid = 0.5 * (t0 + t1)
            r = min(self.rows, key=lambda x: abs(x[0] - mid))
            if abs(r[0] - mid) > 0.05:
                return out
            rows, out["nearest_sample_only"] = [r], True
        ps = [r[1] for r in rows if r[1] is not None]
        fs = [r[2] for r in rows if r[2] is not None]
        if ps:
            out["power_w"], out["power_w_max"] = sum(ps) / len(ps), max(ps)
        if fs:
            out["sclk_mhz"], out["sclk_mhz_min"] = sum(fs) / len(fs), min(fs)
        out["samples"] = len(rows)
        return out


class Limiter:
    """Which limiter holds the clock down, from a DOCUMENTED interface (round 5 read a guessed byte offset of the
    gpu_metrics blob): the amdsmi library's violation accumulators (amdsmi_get_violation_status -> amdsmi_violation_status_t:
    acc_counter, acc_ppt_pwr "PVIOL", acc_socket_thrm "TVIOL", acc_prochot_thrm, acc_vr_thrm, acc_hbm_thrm; the same numbers
    `amd-smi metric --violation` prints).  Residency of a limiter over a window = delta acc_x * 100 / delta acc_counter
    (rocm_smi.h's formula for PVIOL / TVIOL).  The two snapshots are taken by a helper thread WHILE the main thread keeps the
    workload running back to back, so the window holds nothing but the workload."""

    KEYS = (("ppt", "acc_ppt_pwr"), ("socket_thermal", "acc_socket_thrm"), ("prochot", "acc_prochot_thrm"),
            ("vr_thermal", "acc_vr_thrm"), ("hbm_thermal", "acc_hbm_thrm"))

    def __init__(self, bdf):
        self.h, self.source = None, None
        try:
            import amdsmi
            self.smi = amdsmi
            amdsmi.amdsmi_init()
            for h in amdsmi.amdsmi_get_processor_handles():
                if bdf is None or str(amdsmi.amdsmi_get_gpu_device_bdf(h)).lower() == bdf:
                    self.h = h
                    break
            self.source = ("amdsmi_get_violation_status (amdsmi %s), device %s" % (getattr(amdsmi, "__version__", "?"), bdf)) if self.h is not None \
                else "no amdsmi processor handle with BDF %s" % bdf
        except Exception as e:   # noqa: BLE001
            self.h, self.source = None, "amdsmi unavailable: %s: %s" % (type(e).__name__, str(e)[:120])

    def snap(self):
        v = self.smi.amdsmi_get_violation_status(self.h)
        return {k: v.get(k) for k in ("acc_counter",) + tuple(a for _, a in self.KEYS)}

    def during(self, torch, fn, tel, seconds=1.0):
        """Runs fn back to back while a helper thread takes two snapshots `seconds` apart; returns the residencies (percent of the
        window), the hwmon statistics of the same window, and the launch count."""
        if self.h is None:
            return {"error": self.source}
        import threading
        res = {}

        def helper():
            try:
                a = self.snap()
                t0 = time.perf_counter()
                time.sleep(seconds)
                b = self.snap()
                res.update(a=a, b=b, t0=t0, t1=time.perf_counter())
            except Exception as e:   # noqa: BLE001
                res["error"] = "%s: %s" % (type(e).__name__, str(e)[:160])

        for _ in range(8):
            fn()
        torch.cuda.synchronize()
        th = threading.Thread(target=helper, daemon=True)
        th.start()
        n = 0
        while th.is_alive():
            for _ in range(8):
                fn()
            n += 8
            torch.cuda.synchronize()
        th.join()
        if "error" in res:
            return res
        a, b = res["a"], res["b"]
        out = {"window_s": seconds, "launches": n, "source": self.source}
        try:
            dc = int(b["acc_counter"]) - int(a["acc_counter"])
            out["acc_counter_delta"] = dc
            for name, key in self.KEYS:
                out[name + "_residency_pct"] = (100.0 * (int(b[key]) - int(a[key])) / dc) if dc > 0 else None
        except (TypeError, ValueError) as e:
            out["error"] = "accumulators not numeric on this box: %s" % str(e)[:120]
        out.update(tel.window(res["t0"], res["t1"]))
        return out


def step_stats(xs):
    """mean / median / min / max of a list of per-step milliseconds + which steps were outliers (> 1.15 x median)."""
    if not xs:
        return {}
    o = sorted(xs)
    n = len(o)
    med = o[n // 2] if n % 2 else 0.5 * (o[n // 2 - 1] + o[n // 2])
    out = {"ms_mean": sum(xs) / n, "ms_median": med, "ms_min": o[0], "ms_max": o[-1], "steps": n}
    slow = [(i, round(x, 4)) for i, x in enumerate(xs) if x > 1.15 * med]
    if slow:
        out["steps_over_1p15_median"] = slow[:12]
    return out


DUMP_BUDGET_BYTES = 48 << 20   # float32 bytes over all dumped arrays (the files, headers included, stay under 64 MB)


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES, seed=0):
    """Writes every (name, tensor) of `arrays` as float32 to directory/<name>.npy.  When all of them fit in `budget` bytes they
    are written whole, in their own shape; otherwise the budget is shared in proportion to their sizes and each array is
    written as a fixed, seeded sample of its rows (the last dimension kept whole, rows in ascending order), shape
    [rows kept, last dim].  The sample depends only on the shapes and `seed`, so two runs with the same arguments write the
    same elements.  Returns {name: {"shape", "rows", "rows_kept"}}."""
    import numpy as np
    import torch
    os.makedirs(directory, exist_ok=True)
    total = 4 * sum(t.numel() for _, t in arrays)
    written = {}
    for name, t in arrays:
        t = t.detach()
        rows = t.reshape(-1, t.shape[-1])
        n = rows.shape[0]
        keep = n if total <= budget else max(1, n * budget // total)
        if keep < n:
            idx = np.sort(np.random.RandomState(seed).choice(n, keep, replace=False))
            a = rows[torch.from_numpy(idx).to(rows.device)].float().cpu().numpy()
        else:
            a = t.float().cpu().numpy()
        np.save(os.path.join(directory, name + ".npy"), a)
        written[name] = {"shape": list(t.shape), "rows": n, "rows_kept": keep}
    return written


def workload_string(config, B, mode=None):
    _, Hq, Hkv, Sq, Sk, D, dtype, causal, dmode = CONFIGS[config]
    return "%s: B=%d/GPU Hq=%d Hkv=%d Sq=%d Sk=%d D=%d %s %s %s" % (config, B, Hq, Hkv, Sq, Sk, D, dtype, "causal" if causal else "non-causal", mode or dmode)


def self_spawn(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: run `python -m torch.distributed.run --nnodes=1
    --nproc-per-node N --master-addr 127.0.0.1 --master-port <free> bench.py <the same arguments>` -- the command the driver
    uses -- as a fresh child process on this process's stdout / stderr, and exit with its status, so that rank 0's JSON line is
    this process's stdout and its exit code this process's.  The device count is checked first: a box with fewer GPUs fails
    here with that message, not inside a rendezvous."""
    if not args.dry_run:
        import torch
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if n < args.gpus:
            raise SystemExit("bench.py: --gpus %d needs %d devices, this node shows %d" % (args.gpus, args.gpus, n))
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.stdout.flush()
    import subprocess
    raise SystemExit(subprocess.call(cmd))


def gather_watchdog(result, rank, limit_s, before_print=None):
    """The output-exchange section is EXTRA to the contract's line and has never met N > 1 GPUs before the driver's run: whatever
    happens in it, the line with `value` (measured before it) gets printed.  Returns the Event the section sets when it is through;
    if it is not set within limit_s the watchdog thread records that in result["gather"]["error"], rank 0 prints the line, and the
    process ends with status 0 (a hung collective cannot be cancelled from Python; os._exit skips the process group's destructor,
    which would hang too).  tests/test_bench_spawn.py drives this path on gloo (AULE_BENCH_TEST_HANG)."""
    import threading
    done = threading.Event()

    def watchdog():
        if not done.wait(timeout=limit_s):
            result.setdefault("gather", {})["error"] = "the output-exchange section did not finish in %.0f s; line printed by the watchdog" % limit_s
            if before_print is not None:
                before_print()
            if rank == 0:
                print(json.dumps(result), flush=True)
            sys.stdout.flush()
            os._exit(0)

    threading.Thread(target=watchdog, daemon=True).start()
    return done


def dry_run(args):
    """The bench's launch contract without a device: process group (gloo) of --gpus ranks, the rank-count assertion, K timed
    no-op steps between barriers, MAX over ranks, rank 0 prints one line with "dry_run": true and no throughput."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 or "RANK" in os.environ:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        assert dist.get_world_size() == world
    else:
        dist = None
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but the launcher made %d rank(s)" % (args.gpus, world))
    for _ in range(args.warmup):
        pass
    if dist is not None:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pass
    wall = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([wall], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t[0])
        dist.barrier()
    result = {"metric": "attention TFLOPS/GPU (fwd, fwd+bwd) + % MFMA roofline at S=4096,D=128", "value": None,
              "unit": "TFLOP/s", "n_gpus": world, "world_size": world, "steps": args.steps, "warmup": args.warmup,
              "ms_per_step": wall * 1e3 / max(1, args.steps), "dry_run": True,
              "config": {"workload": workload_string(args.config, args.batch or CONFIGS[args.config][0], args.mode)}}
    if world > 1:
        # the sharding arithmetic of the real run, sizes only: who holds what of the gathered output (aule/dist.py)
        from aule import dist as adist
        _, Hq, Hkv, Sq, _, D, dtype, _, _ = CONFIGS[args.config]
        Bl = args.batch or CONFIGS[args.config][0]
        sizes, total = adist.gather_bytes(Bl * world, Hq, Hkv, Sq, D, 2 if dtype != "fp32" else 4, world)
        result["gather_plan"] = {"bytes_per_rank": sizes, "total_bytes": total, "shard": adist.shard_plan(Bl * world, Hkv, world)[0]}
    if os.environ.get("AULE_BENCH_TEST_HANG"):
        # test hook: an exchange section that never comes back (a collective one rank never joins) -> the watchdog prints the line
        result["gather"] = {"steps": 0}
        gather_watchdog(result, rank, float(os.environ.get("AULE_BENCH_GATHER_TIMEOUT", "240")))
        if dist is not None and rank != 0:
            time.sleep(3600)            # this rank never joins ...
        try:
            if dist is not None:
                dist.barrier()          # ... so this never returns on rank 0
            else:
                time.sleep(3600)
        except Exception as e:          # noqa: BLE001 -- (the peer's watchdog ended it first: recorded like any failure of the section)
            result["gather"]["error"] = (type(e).__name__ + ": " + str(e))[:200]
    if rank == 0:
        print(json.dumps(result), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default=None, choices=sorted(CONFIGS),
                    help="default: c2 (BASELINE configs[1], the headline) on one GPU, c4 (configs[3]: B=64 over 8 GPUs -> 8 per GPU, S=8192) with --gpus N > 1")
    ap.add_argument("--mode", default=None, choices=["fwd", "fwdbwd"])
    ap.add_argument("--batch", type=int, default=None, help="override the per-GPU batch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (out; dq, dk, dv in fwdbwd mode; rank 0's "
                         "shard) as float32 DIR/<name>.npy, a fixed seeded sample of rows where the whole exceeds %d MiB"
                         % (DUMP_BUDGET_BYTES >> 20))
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside `value`: the conditioned steady_state leg, hwmon telemetry, the output exchange "
                         "of N > 1 ranks, the extra configs / precisions, the limiter, the reference harness vs SDPA, the CPU baseline")
    ap.add_argument("--condition-ms", type=float, default=250.0,
                    help="(--full) device time spent repeating the step before warm-up (0: none); see the module docstring")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="(--full) skip the extra configs / precisions / limiter")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch / rendezvous / timing scaffolding only (gloo, no device, no kernels): what tests/test_bench_spawn.py drives")
    args = ap.parse_args()

    if args.config is None:
        # BASELINE.json: configs[1] is the single-GPU headline, configs[3] the multi-GPU scaling run (B=64 H=32 S=8192 D=128 over 8 GPUs =
        # 8 per GPU; weak scaling keeps that per-GPU batch at N = 2, 4)
        args.config = "c2" if args.gpus == 1 else "c4"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_spawn(args)

    if args.dry_run:
        return dry_run(args)

    import torch
    import aule  # raises AuleError at first use if libaule.so / a HIP device is missing

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: no ROCm device visible (there is no CPU fallback)")
    if torch.cuda.device_count() < max(args.gpus, local_rank + 1):
        raise SystemExit("bench.py: --gpus %d needs %d devices, this node shows %d" % (args.gpus, args.gpus, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or "RANK" in os.environ:   # launched by torch.distributed.run (also exercised with 1 rank)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world,
                                device_id=torch.device("cuda", local_rank))
    if dist is not None:
        assert dist.get_world_size() == world
    if args.gpus != world:
        # (the driver launches `--gpus N` under torch.distributed.run with N ranks; a plain `python bench.py --gpus N` spawns
        # them itself: self_spawn.  What is left is a launcher that made a different number of ranks than --gpus says.)
        raise SystemExit("bench.py: --gpus %d but the launcher made %d rank(s)" % (args.gpus, world))
    n_gpus = world

    B, Hq, Hkv, Sq, Sk, D, dtype, causal, mode = CONFIGS[args.config]
    if args.batch:
        B = args.batch
    mode = args.mode or mode
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[dtype]
    dev = torch.device("cuda", local_rank)
    gen = torch.Generator(device=dev).manual_seed(1234 + rank)
    q = torch.randn(B, Hq, Sq, D, device=dev, dtype=tdt, generator=gen)
    k = torch.randn(B, Hkv, Sk, D, device=dev, dtype=tdt, generator=gen)
    v = torch.randn(B, Hkv, Sk, D, device=dev, dtype=tdt, generator=gen)
    do = torch.randn(B, Hq, Sq, D, device=dev, dtype=tdt, generator=gen) if mode == "fwdbwd" else None
    # autograd on in both modes: the forward then stores LSE (what a training forward, and the reference's, does)
    q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)

    tel = Telemetry(torch, local_rank, enabled=args.full)
    dump_steps = bool(os.environ.get("AULE_BENCH_DUMP_STEPS"))
    # --dump-outputs: the output of the latest step is kept (otherwise it is dropped as soon as the step returns, as before)
    keep_last = args.dump_outputs is not None
    last = [None]

    def step(mid=None):
        if mode == "fwd":
            out = aule.flash_attention(q, k, v, causal=causal)
            if keep_last:
                last[0] = out
            return out
        q.grad = k.grad = v.grad = None
        out = aule.flash_attention(q, k, v, causal=causal)
        if keep_last:
            last[0] = out
        if mid is not None:
            mid()
        out.backward(do)
        return out

    def sync_all():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(fn, steps, split=False):
        """Barrier + synchronize, K steps, synchronize; wall clock and HIP-event time on the launch stream (torch's
        current stream = the stream the kernels are launched on), MAX over ranks.  Per-step event pairs give the
        per-launch spread (rank-local).  split: `fn(mid)` calls `mid()` between its forward call and its backward(), which
        records one more event per step -- the forward and the backward segment of every timed step."""
        sync_all()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        mids = [torch.cuda.Event(enable_timing=True) for _ in range(steps)] if split else None
        t0 = time.perf_counter()
        ev[0].record()
        for i in range(steps):
            if split:
                fn(mids[i].record)
            else:
                fn()
            ev[i + 1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        wall = t1 - t0
        dev_ms = ev[0].elapsed_time(ev[steps])
        rec = {"per_step": [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)], "t0": t0, "t1": t1}
        if split:
            rec["fwd_seg"] = [ev[i].elapsed_time(mids[i]) for i in range(steps)]
            rec["bwd_seg"] = [mids[i].elapsed_time(ev[i + 1]) for i in range(steps)]
        if dist is not None:
            t = torch.tensor([wall, dev_ms], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall, dev_ms = float(t[0]), float(t[1])
            dist.barrier()
        rec["wall_s"], rec["dev_ms"] = wall, dev_ms
        return rec

    def condition(fn, ms):
        """Repeat the step for ~ms of device time (power / clock controller into steady state); returns (steps, ms).
        The step is sized from the mean of three calls AFTER two untimed ones: the first call of a new workload pays its
        allocations (round 3 sized the loop from that call alone -- 5 ms instead of 0.6 -- and the "conditioned" extra legs
        then ran 30 ms, not 250, and were read inside the clock transient: profiles/r4_bench_conditioning.txt)."""
        if ms <= 0:
            return 0, 0.0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        fn()
        e0.record()
        for _ in range(3):
            fn()
        e1.record()
        torch.cuda.synchronize()
        first = e0.elapsed_time(e1)
        one = max(1e-3, first / 3)
        n = max(1, int(ms / one))
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return n + 3, e0.elapsed_time(e1) + first      # (the two untimed calls are neither counted nor timed)

    legs = {}

    def leg(name, fn, steps, cond_ms=0.0, warm=0, split=False, flops=None, peak=None):
        """One complete measurement: optional conditioning on the leg's own step, `warm` untimed steps, `steps` timed ones with
        an event pair each; statistics of the steps + the telemetry of the timed window -> legs[name].  Returns the record
        (with the raw `timed` result under "_raw")."""
        cs, cms = condition(fn, cond_ms)
        for _ in range(warm):
            fn()
        raw = timed(fn, steps, split)
        rec = step_stats(raw["per_step"])
        rec["ms_mean_events"] = raw["dev_ms"] / steps          # first event to last: includes the gaps between steps
        if split:
            rec["fwd_segment"] = step_stats(raw["fwd_seg"])
            rec["bwd_segment"] = step_stats(raw["bwd_seg"])
        if flops is not None:
            rec["tflops_mean"] = flops / (rec["ms_mean_events"] * 1e-3) / 1e12
            rec["tflops_median"] = flops / (rec["ms_median"] * 1e-3) / 1e12
            if peak:
                rec["frac_mean"], rec["frac_median"] = rec["tflops_mean"] / peak, rec["tflops_median"] / peak
        rec.update(tel.window(raw["t0"], raw["t1"]))
        if cond_ms > 0:
            rec["conditioning_ms"], rec["conditioning_steps"] = cms, cs
        if dump_steps:
            rec["per_step_ms"] = [round(x, 4) for x in raw["per_step"]]
            if split:
                rec["per_step_bwd_ms"] = [round(x, 4) for x in raw["bwd_seg"]]
        legs[name] = rec
        out = dict(rec)
        out["_raw"] = raw
        return out

    f_fwd = fwd_flops(B, Hq, Sq, Sk, D, causal)
    f_step = f_fwd * (3.5 if mode == "fwdbwd" else 1.0)
    split_main = mode == "fwdbwd"

    # 1. the contract's protocol, first thing, on the chip as the process finds it: W untimed steps, EXACTLY K timed steps -> `value`
    main_leg = leg("value", step, args.steps, 0.0, args.warmup, split_main, f_step, PEAK_TFLOPS[dtype])
    wall, dev_ms = main_leg["_raw"]["wall_s"], main_leg["_raw"]["dev_ms"]
    launches = sorted(main_leg["_raw"]["per_step"])
    dumped = None
    if args.dump_outputs is not None and rank == 0:
        # what the caller of the timed path received from its last step: O, and in fwdbwd mode the gradients
        arrays = [("out", last[0])] + ([("dq", q.grad), ("dk", k.grad), ("dv", v.grad)] if mode == "fwdbwd" else [])
        dumped = dump_outputs(args.dump_outputs, arrays)
    last[0] = None
    if args.full:
        # 2. the same protocol again behind a conditioning phase -> "steady_state" (reported beside `value`, never as it)
        steady_leg = leg("steady_state", step, args.steps, args.condition_ms, args.warmup, split_main, f_step, PEAK_TFLOPS[dtype])
        steady_wall, steady_dev_ms = steady_leg["_raw"]["wall_s"], steady_leg["_raw"]["dev_ms"]
        cond_steps, cond_ms = steady_leg.get("conditioning_steps", 0), steady_leg.get("conditioning_ms", 0.0)

    def launch_stats():
        n = len(launches)
        return {"kernel_ms_median": launches[n // 2], "kernel_ms_min": launches[0], "kernel_ms_max": launches[-1]}

    def measured_telemetry(rec):
        """what the hwmon sampler saw in the leg's timed window (None where the box has no readable hwmon)"""
        return {k: rec.get(k) for k in ("power_w", "power_w_max", "power_cap_w", "sclk_mhz", "sclk_mhz_min", "samples")}

    ms_per_step = wall * 1e3 / args.steps
    value = f_step * n_gpus * args.steps / wall / 1e12
    kern_ms = dev_ms / args.steps          # HIP events on the launch stream, per step
    achieved = f_step / (kern_ms * 1e-3) / 1e12
    elt = 2 if dtype != "fp32" else 4
    alg_bytes = elt * (2 * B * Hq * Sq * D + 2 * B * Hkv * Sk * D) + 4 * B * Hq * Sq
    hbm_bound = mode == "fwd" and f_step / alg_bytes < RIDGE
    tel_value = measured_telemetry(main_leg)
    steady = {}        # --full: the conditioned leg's figures beside `value` (top level "steady_state", roofline frac_steady / steady)
    if args.full:
        tel_steady = measured_telemetry(steady_leg)
        frac_steady = f_step / (steady_dev_ms / args.steps * 1e-3) / 1e12 / PEAK_TFLOPS[dtype]
        steady = {"steady_state": {"value": f_step * n_gpus * args.steps / steady_wall / 1e12, "ms_per_step": steady_wall * 1e3 / args.steps,
                         "frac": frac_steady,
                         "ms_per_step_median": steady_leg["ms_median"], "ms_per_step_min": steady_leg["ms_min"], "ms_per_step_max": steady_leg["ms_max"],
                         "frac_median": steady_leg.get("frac_median"),
                         "conditioning_ms": cond_ms, "conditioning_steps": cond_steps, **tel_steady,
                         "note": "the same W + K protocol AFTER repeating the step for --condition-ms of device time: past the MI355X DVFS "
                                 "transient that follows load onset (~60 launches / 40 ms, profiles/r2_dvfs_trace.txt).  What a long-"
                                 "running job sees; `value` above is the plain protocol (round 2 called that one cold_start); power_w / "
                                 "sclk_mhz: hwmon of this device in the timed window of THIS run"}}

    result = {
        "metric": "attention TFLOPS/GPU (fwd, fwd+bwd) + % MFMA roofline at S=4096,D=128",
        "value": value,
        "unit": "TFLOP/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": dtype,
        "data": "synthetic N(0,1) q,k,v resident in HBM, torch.Generator(seed 1234+rank)",
        "config": {"workload": workload_string(args.config, B, mode),
            "global_batch": B * n_gpus, "parallelism": "batch-sharded dp%d, no data-path collective" % n_gpus,
            "flop_convention": "4*B*Hq*D*sum_i min(i+1,Sk) (causal), bwd=2.5x fwd",
            "lse": "stored (autograd is on: the forward writes the log-sum-exp like the reference's, triton_flash_amd.py:410-432)"},
        **steady,
        "world_size": world,
        "per_gpu_tflops": value / n_gpus,
        "telemetry_source": tel.source,
        "roofline": ({"bound": "hbm", "achieved": alg_bytes / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "frac": alg_bytes / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": hbm_traffic(args.config, mode),
                      "kernel_ms": kern_ms, **launch_stats(), **tel_value,
                      "note": "arithmetic intensity %.0f FLOP/B < ridge %.0f: achieved = algorithmic bytes (%d) / HIP-event "
                              "time per step" % (f_step / alg_bytes, RIDGE, int(alg_bytes))}
                     if hbm_bound else
                     {"bound": "mfma", "achieved": achieved, "peak": PEAK_TFLOPS[dtype], "unit": "TFLOP/s",
                      "frac": achieved / PEAK_TFLOPS[dtype], "traffic": hbm_traffic(args.config, mode),
                      **({"frac_steady": frac_steady} if args.full else {}),
                      "traffic_source": "stored: rocprofv3 PMC passes of the last profiled run of this workload (profiles/hbm_traffic.json, "
                                        "FETCH_SIZE x2 + WRITE_SIZE per launch), not measured in this run",
                      "effective_clock_ghz_profiled": stored_profile(args.config, mode).get("effective_clock_ghz"),
                      # MEASURED in this run (round 6): hwmon socket power / shader clock of this device in the timed window of the
                      # `value` leg and of the conditioned leg; the power cap as hwmon reports it
                      **tel_value,
                      **({"steady": tel_steady} if args.full else {}),
                      "telemetry": "measured: hwmon sampler thread, the timed window of the `value` leg (top level) and of the conditioned leg (`steady`)",
                      # stored: what this chip sustains on N(0,1) operands as a fraction of `peak` -- a RANGE with its sources (round 5):
                      # bare-MFMA loops of two shapes, and the vendor GEMM (hipBLASLt bf16 8192^3) as the control (profiles/r5_ceiling_control.txt)
                      **{k: stored_profile(args.config, mode).get(k) for k in ("mfma_only_random_frac_of_peak", "power_profile")},
                      "kernel_ms": kern_ms, **launch_stats(),
                      "note": "achieved = algorithmic FLOPs per step / HIP-event time per step on the launch stream (the `value` leg: "
                              "plain W + K protocol); frac_steady = the same for the conditioned leg; algorithmic bytes %d; the nominal "
                              "peak assumes 2.4 GHz, sclk_mhz is what hwmon read while the leg ran" % int(alg_bytes)}),
    }
    if split_main:
        for nm, lg in (("value", main_leg),) + ((("steady_state", steady_leg),) if args.full else ()):
            b = lg["bwd_segment"]["ms_median"]
            result.setdefault("backward", {})[nm] = {"bwd_ms_median": b, "fwd_ms_median": lg["fwd_segment"]["ms_median"],
                                                     "bwd_tflops": 2.5 * f_fwd / (b * 1e-3) / 1e12,
                                                     "bwd_frac": 2.5 * f_fwd / (b * 1e-3) / 1e12 / PEAK_TFLOPS[dtype]}

    if args.full and dist is not None and (n_gpus > 1 or os.environ.get("AULE_BENCH_FORCE_GATHER")):
        # the one exchange of the sharded path: every rank receives every rank's O over xGMI (RCCL), timed separately
        # from `value` (kernel-only scaling): (a) one blocking all-gather behind the whole shard (round 1), (b) the shard
        # in pieces, each piece's all-gather overlapping the next piece's kernels, (c) the same with direct peer sends
        # (all links of the fully connected node at once) -- aule/dist.py, DESIGN.md "Multi-GPU"
        from aule import dist as adist
        out = step().detach()
        gathered = torch.empty((n_gpus,) + tuple(out.shape), device=dev, dtype=out.dtype)

        def attn_nograd(a, b, c, causal=True, scale=None):
            return aule.flash_attention(a.detach(), b.detach(), c.detach(), causal=causal, scale=scale)

        def step_blocking():
            o = step().detach()
            dist.all_gather_into_tensor(gathered, o.contiguous())

        variants = {"blocking_all_gather": step_blocking}
        if mode == "fwd" and B >= 2:
            nch = min(4, B)
            variants["chunked_all_gather"] = lambda: adist.attention_and_gather(q, k, v, causal=causal, attn_fn=attn_nograd,
                                                                                  chunks=nch, transport="allgather")
            variants["chunked_p2p"] = lambda: adist.attention_and_gather(q, k, v, causal=causal, attn_fn=attn_nograd,
                                                                           chunks=nch, transport="p2p")
            # (d) no RCCL in the data path: every piece copied straight into the peers' mapped buffers (aule_peer_* of the
            # C-ABI, one hipMemcpyAsync per peer and piece on per-peer streams).  Its set-up is collective and agrees on
            # failure across the ranks, so a node where IPC mapping does not work reports the reason instead of hanging.
            variants["chunked_peer"] = lambda: adist.attention_and_gather(q, k, v, causal=causal, chunks=nch, transport="peer")
        gsteps = max(1, min(args.steps, 20))
        result["gather"] = {"bytes_per_rank": out.numel() * out.element_size(), "steps": gsteps}
        # The exchange variants are EXTRA to the contract's line and none of them has met N > 1 GPUs before the driver's run:
        # whatever happens in here, the line with `value` (measured above) gets printed.  A watchdog prints it and ends the
        # process if the section does not come back (a hung collective would otherwise take the whole scaling record with it);
        # an exception is recorded in the line.
        def add_legs():
            result["legs"] = legs

        section_done = gather_watchdog(result, rank, float(os.environ.get("AULE_BENCH_GATHER_TIMEOUT", "240")), add_legs)
        if os.environ.get("AULE_BENCH_TEST_HANG"):       # test hook (tests/test_gpu_dist.py): the section never comes back
            time.sleep(3600)
        try:
            for name, fn in variants.items():
                try:
                    for _ in range(2):
                        fn()
                except aule.AuleError as e:     # (raised on every rank alike: aule.dist.PeerExchange)
                    result["gather"][name] = {"error": str(e)[:300]}
                    continue
                graw = timed(fn, gsteps)
                gwall = graw["wall_s"]
                result["gather"][name] = {"ms_per_step": gwall * 1e3 / gsteps, "value": f_step * n_gpus * gsteps / gwall / 1e12,
                                          "exposed_ms": gwall * 1e3 / gsteps - ms_per_step,
                                          "ms_per_step_median_rank0": step_stats(graw["per_step"])["ms_median"]}
            adist.release_peer_buffers()
        except Exception as e:   # noqa: BLE001 -- keep the contract's line
            result["gather"]["error"] = (type(e).__name__ + ": " + str(e))[:400]
        section_done.set()
        del gathered

    if args.full and rank == 0 and n_gpus == 1 and not args.no_extra and args.config == "c2":
        PK = PEAK_TFLOPS["bf16"]
        extra = result["extra"] = {}
        # which limiter holds the clock while the headline kernel runs back to back (documented amdsmi accumulators; one second of launches)
        lim = Limiter(tel.bdf)
        result["limiter"] = {"c2_fwd": lim.during(torch, step, tel),
                             "note": "residency = share of the window in which the firmware reports the limiter active (PPT = package power tracking: the "
                                     "socket power cap); window = the workload back to back for window_s, nothing else; power_w / sclk_mhz = hwmon over the same window"}

        def fwd_bwd_block(prefix, f1, step_fb, step_f, steps, workload, peak=PK):
            """A fwd+bwd leg with the event between forward and backward, conditioned on itself, and a fwd-only leg RIGHT behind
            it (no new conditioning: the chip is in the state the fwd+bwd steps left it in).  Every backward figure is a median
            over the timed steps' backward segments; `_by_difference` = median fwd+bwd step - median fwd-only step."""
            fb = leg(prefix + "_fwd_bwd", step_fb, steps, args.condition_ms, 0, True, 3.5 * f1, peak)
            fo = leg(prefix + "_fwd_only", step_f, steps, 0.0, 0, False, f1, peak)
            b = fb["bwd_segment"]["ms_median"]
            bd = fb["ms_median"] - fo["ms_median"]
            extra.update({
                prefix + "_fwd_bwd_tflops": fb["tflops_mean"], prefix + "_fwd_bwd_frac_of_peak": fb["frac_mean"],
                prefix + "_fwd_bwd_tflops_median": fb["tflops_median"],
                prefix + "_ms_per_step": fb["ms_mean_events"], prefix + "_ms_per_step_median": fb["ms_median"],
                prefix + "_ms_per_step_min": fb["ms_min"], prefix + "_ms_per_step_max": fb["ms_max"],
                prefix + "_fwd_ms": fo["ms_median"], prefix + "_fwd_tflops": f1 / (fo["ms_median"] * 1e-3) / 1e12,
                prefix + "_fwd_ms_in_step": fb["fwd_segment"]["ms_median"],
                prefix + "_bwd_ms": b, prefix + "_bwd_tflops": 2.5 * f1 / (b * 1e-3) / 1e12,
                prefix + "_bwd_frac": 2.5 * f1 / (b * 1e-3) / 1e12 / peak,
                prefix + "_bwd_ms_min": fb["bwd_segment"]["ms_min"], prefix + "_bwd_ms_max": fb["bwd_segment"]["ms_max"],
                prefix + "_bwd_ms_by_difference": bd,
                prefix + "_bwd_frac_by_difference": (2.5 * f1 / (bd * 1e-3) / 1e12 / peak) if bd > 0 else None,
                prefix + "_power_w": fb.get("power_w"), prefix + "_sclk_mhz": fb.get("sclk_mhz"), prefix + "_sclk_mhz_min": fb.get("sclk_mhz_min"),
                prefix + "_workload": workload + "; *_bwd_ms / *_bwd_frac = MEDIAN over the timed steps of the segment between the event behind the "
                                                 "forward call and the event behind backward(); *_by_difference = median step - median step of the fwd-only leg run right behind it"})
            return fb, fo

        # the other half of the metric: fwd+bwd on config #3 (GQA 32q/8kv S=2048, B=4 as SURVEY 8d assumes), and config #5
        # (MQA 32q/1kv S=16384 D=64 fp16 non-causal forward), outside the timed region of `value`
        B3, H3, K3, S3, _, D3, _, _, _ = CONFIGS["c3"]
        g3 = torch.Generator(device=dev).manual_seed(99)
        q3 = torch.randn(B3, H3, S3, D3, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        k3 = torch.randn(B3, K3, S3, D3, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        v3 = torch.randn(B3, K3, S3, D3, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        d3 = torch.randn(B3, H3, S3, D3, device=dev, dtype=torch.bfloat16, generator=g3)

        def step3(mid=None):
            q3.grad = k3.grad = v3.grad = None
            o = aule.flash_attention(q3, k3, v3, causal=True)
            if mid is not None:
                mid()
            o.backward(d3)

        def step3f():
            aule.flash_attention(q3, k3, v3, causal=True)

        fwd_bwd_block("c3", fwd_flops(B3, H3, S3, S3, D3, True), step3, step3f, 30,
                      "GQA 32q/8kv B=4 S=2048 D=128 bf16 causal fwd+bwd (autograd)")
        del q3, k3, v3, d3
        # the metric's own fwd+bwd shape: C2 (B4 H32 S4096 D128 bf16 causal) through autograd, on this run's q, k, v
        # (the reference harness sweeps these shapes fwd+bwd: tests/benchmark_mi300x.py:207-233)
        d2 = torch.randn(B, Hq, Sq, D, device=dev, dtype=tdt, generator=g3)

        def step2(mid=None):
            q.grad = k.grad = v.grad = None
            o = aule.flash_attention(q, k, v, causal=causal)
            if mid is not None:
                mid()
            o.backward(d2)

        fwd_bwd_block("c2", f_fwd, step2, step, 20, "MHA B=4 H=32 S=4096 D=128 bf16 causal fwd+bwd (autograd): the metric's own shape", PEAK_TFLOPS[dtype])
        # (key names of rounds 4-5)
        extra["c2_fwd_bwd_ms_per_step"], extra["c2_fwd_bwd_ms_per_step_median"] = extra["c2_ms_per_step"], extra["c2_ms_per_step_median"]
        result["limiter"]["c2_fwd_bwd"] = lim.during(torch, step2, tel)
        q.grad = k.grad = v.grad = None
        del d2
        B5, H5, K5, S5, _, D5, _, _, _ = CONFIGS["c5"]
        q5 = torch.randn(B5, H5, S5, D5, device=dev, dtype=torch.float16, generator=g3).requires_grad_(True)
        k5 = torch.randn(B5, K5, S5, D5, device=dev, dtype=torch.float16, generator=g3)
        v5 = torch.randn(B5, K5, S5, D5, device=dev, dtype=torch.float16, generator=g3)

        def step5():
            aule.flash_attention(q5, k5, v5, causal=False)

        l5 = leg("c5_fwd", step5, 20, args.condition_ms, 0, False, fwd_flops(B5, H5, S5, S5, D5, False), PEAK_TFLOPS["fp16"])
        extra.update({"c5_fwd_tflops": l5["tflops_mean"], "c5_fwd_frac_of_peak": l5["frac_mean"], "c5_ms_per_step": l5["ms_mean_events"],
                      "c5_ms_per_step_median": l5["ms_median"], "c5_power_w": l5.get("power_w"), "c5_sclk_mhz": l5.get("sclk_mhz"),
                      "c5_workload": "MQA 32q/1kv B=1 S=16384 D=64 fp16 non-causal fwd (LSE stored)"})

        del q5, k5, v5
        # single-sequence prefill, the small-grid corner (128 paired items on 256 CUs: route 7, pairs of Q blocks cut into
        # key ranges + merge), and RoPE + attention the inference way (K by the pass, Q rotated inside the kernel, 3.6)
        q6, k6, v6 = (torch.randn(1, 8, 8192, 128, device=dev, dtype=torch.bfloat16, generator=g3) for _ in range(3))

        def step6():
            with torch.no_grad():
                aule.flash_attention(q6, k6, v6, causal=True)

        l6 = leg("b1h8_s8192_fwd", step6, 20, args.condition_ms, 0, False, fwd_flops(1, 8, 8192, 8192, 128, True), PK)
        extra.update({"b1h8_s8192_fwd_tflops": l6["tflops_mean"], "b1h8_s8192_ms_per_step": l6["ms_mean_events"],
                      "b1h8_s8192_ms_per_step_median": l6["ms_median"], "b1h8_s8192_sclk_mhz": l6.get("sclk_mhz"),
                      "b1h8_s8192_workload": "MHA 8 heads B=1 S=8192 D=128 bf16 causal fwd (small grid, route 7: the one-wave-per-SIMD kernel over 256 key-range pieces + merge kernel)"})
        del q6, k6, v6
        B7, H7, S7, D7 = 4, 32, 2048, 128
        q7, k7, v7 = (torch.randn(B7, H7, S7, D7, device=dev, dtype=torch.bfloat16, generator=g3) for _ in range(3))
        cos7, sin7 = aule.precompute_rope_frequencies(S7, D7, device=dev)

        def step7():
            with torch.no_grad():
                aule.flash_attention_rope(q7, k7, v7, cos7, sin7, causal=True)

        l7 = leg("rope_attn", step7, 20, args.condition_ms, 0, False, fwd_flops(B7, H7, S7, S7, D7, True), PK)
        extra.update({"rope_attn_c2_tflops": l7["tflops_mean"], "rope_attn_c2_ms_per_step": l7["ms_mean_events"],
                      "rope_attn_c2_ms_per_step_median": l7["ms_median"],
                      "rope_attn_c2_workload": "RoPE + attention, B=4 H=32 S=2048 D=128 bf16 causal, inference: rope(K) pass + the "
                                               "one-wave-per-SIMD forward with Q rotated inside it (attention FLOPs only)"})
        del q7, k7, v7
        # sliding-window forward (round 6: the window instances of the one-wave-per-SIMD kernel; the shapes of the reference's README, python/README.md:36-40
        # -- S = 8192, window 256 -- and window 1024); FLOPs count the VISIBLE scores only (a band of W keys per query)
        qw, kw, vw = (torch.randn(4, 32, 8192, 128, device=dev, dtype=torch.bfloat16, generator=g3) for _ in range(3))
        for W in (256, 1024):
            vis = W * (W + 1) // 2 + (8192 - W) * W

            def stepw(W=W):
                with torch.no_grad():
                    aule.flash_attention(qw, kw, vw, causal=True, window_size=W)

            lw = leg("window_s8192_w%d_fwd" % W, stepw, 20, args.condition_ms, 0, False, 4.0 * 4 * 32 * 128 * vis, PK)
            extra.update({"window_s8192_w%d_fwd_tflops_visible" % W: lw["tflops_median"], "window_s8192_w%d_ms_per_step_median" % W: lw["ms_median"]})
        extra["window_workload"] = ("B=4 H=32 S=8192 D=128 bf16 causal, window_size 256 / 1024, fwd: route 8, the window instances of the one-wave-per-SIMD kernel "
                                    "(TFLOP/s of the visible scores only, median step)")
        del qw, kw, vw
        # D = 64 training (the one-wave-per-SIMD backward pair's D = 64 instances, round 4) and the fp32 kernels (what the legacy
        # C-ABI and NumPy / fp32 torch input run; priced against the 157.3 TF f32-MFMA roof, not the bf16 peak)
        q8 = torch.randn(8, 32, 2048, 64, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        k8 = torch.randn(8, 32, 2048, 64, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        v8 = torch.randn(8, 32, 2048, 64, device=dev, dtype=torch.bfloat16, generator=g3).requires_grad_(True)
        d8 = torch.randn(8, 32, 2048, 64, device=dev, dtype=torch.bfloat16, generator=g3)

        def step8(mid=None):
            q8.grad = k8.grad = v8.grad = None
            o = aule.flash_attention(q8, k8, v8, causal=True)
            if mid is not None:
                mid()
            o.backward(d8)

        def step8f():
            aule.flash_attention(q8, k8, v8, causal=True)

        fwd_bwd_block("d64", fwd_flops(8, 32, 2048, 2048, 64, True), step8, step8f, 20,
                      "MHA B=8 H=32 S=2048 D=64 bf16 causal fwd+bwd (autograd)")
        del q8, k8, v8, d8
        F32_ROOF = 157.3
        q9 = torch.randn(4, 32, 2048, 64, device=dev, dtype=torch.float32, generator=g3).requires_grad_(True)
        k9 = torch.randn(4, 32, 2048, 64, device=dev, dtype=torch.float32, generator=g3).requires_grad_(True)
        v9 = torch.randn(4, 32, 2048, 64, device=dev, dtype=torch.float32, generator=g3).requires_grad_(True)
        d9 = torch.randn(4, 32, 2048, 64, device=dev, dtype=torch.float32, generator=g3)

        def step9(mid=None):
            q9.grad = k9.grad = v9.grad = None
            o = aule.flash_attention(q9, k9, v9, causal=True)
            if mid is not None:
                mid()
            o.backward(d9)

        def step9f():
            aule.flash_attention(q9, k9, v9, causal=True)

        fwd_bwd_block("f32", fwd_flops(4, 32, 2048, 2048, 64, True), step9, step9f, 10,
                      "MHA B=4 H=32 S=2048 D=64 fp32 causal (v_mfma_f32_32x32x2_f32 kernels: the legacy C-ABI's dtype), priced against the f32 roof", F32_ROOF)
        extra.update({"f32_fwd_frac_of_f32_roof": extra["f32_fwd_tflops"] / F32_ROOF, "f32_bwd_frac_of_f32_roof": extra["f32_bwd_frac"],
                      "f32_roof_tflops": F32_ROOF})
        del q9, k9, v9, d9
        # The reference's OWN harness (python/aule/triton_flash_amd.py:775-813: fp16 causal forward, B 1 / 8, H 32, S 2048 / 8192, D 128, warm-up 10,
        # timed 50; tests/benchmark_mi300x.py:207-233 adds B 1 H 32 S 4096) and its comparator: the only number the reference publishes for
        # this path is relative to torch SDPA (python/README.md:20-23, "+6.1 .. +9.6 %").  Same process, same tensors, same protocol for both;
        # SDPA is a COMPARATOR here and nowhere else (never the product path).  FLOPs: the causal-discounted convention of `value`.
        # Medians (the reference's harness reports medians: tests/benchmark_mi300x.py).
        import torch.nn.functional as F
        harness = []
        for (Bh, Hh, Sh) in ((1, 32, 2048), (8, 32, 2048), (1, 32, 8192), (1, 32, 4096)):
            qh, kh, vh = (torch.randn(Bh, Hh, Sh, 128, device=dev, dtype=torch.float16, generator=g3) for _ in range(3))

            def step_a():
                with torch.no_grad():
                    return aule.flash_attention(qh, kh, vh, causal=True)

            def step_s():
                with torch.no_grad():
                    return F.scaled_dot_product_attention(qh, kh, vh, is_causal=True)

            fl = fwd_flops(Bh, Hh, Sh, Sh, 128, True)
            row = {"shape": "B%d H%d S%d D128 fp16 causal fwd" % (Bh, Hh, Sh)}
            la = leg("harness_b%d_s%d_aule" % (Bh, Sh), step_a, 50, args.condition_ms / 2, 10, False, fl, PEAK_TFLOPS["fp16"])
            msa = la["ms_median"]
            row.update({"aule_ms": msa, "aule_ms_mean": la["ms_mean_events"], "aule_tflops": fl / (msa * 1e-3) / 1e12, "aule_tokens_per_s": Bh * Sh / (msa * 1e-3),
                        "aule_tflops_ref_convention": 4.0 * Bh * Hh * Sh * Sh * 128 / (msa * 1e-3) / 1e12,
                        "aule_power_w": la.get("power_w"), "aule_sclk_mhz": la.get("sclk_mhz")})
            try:
                ls = leg("harness_b%d_s%d_sdpa" % (Bh, Sh), step_s, 50, args.condition_ms / 2, 10, False, fl, PEAK_TFLOPS["fp16"])
                mss = ls["ms_median"]
                err = (step_a().float() - step_s().float()).abs().max().item()
                row.update({"sdpa_ms": mss, "sdpa_tflops": fl / (mss * 1e-3) / 1e12, "speedup_vs_sdpa": mss / msa,
                            "max_abs_diff_vs_sdpa": err})
            except Exception as e:   # noqa: BLE001 -- the comparator must not take the line with it
                row["sdpa_error"] = (type(e).__name__ + ": " + str(e))[:200]
            harness.append(row)
            del qh, kh, vh
        extra["ref_harness"] = {
            "rows": harness,
            "protocol": "fp16 causal forward, no LSE (inference call), 10 warm-ups + 50 timed launches with an event pair each after conditioning, MEDIAN launch; "
                        "torch.nn.functional.scaled_dot_product_attention(is_causal=True) on the same tensors in the same process as the comparator "
                        "(torch %s; backend chosen by torch)" % torch.__version__,
            "reference_claim": "python/README.md:20-23: the reference's Triton kernel vs PyTorch SDPA on MI300X, +6.1 .. +9.6 %"}

        # Power: the same C2 forward on ALL-ZERO inputs (the same launch, the same instruction stream, the same MFMA count; no
        # data-dependent switching in the matrix pipes, the register files and LDS).  The distance between this figure and
        # `steady_state` is what the chip's power cap costs on N(0,1) data: the clock it sustains, not the kernel's schedule
        # (the backward kernels show the same ratio: tools/cbench.cpp with CB_AMP=0).
        qz, kz, vz = (torch.zeros(B, h, Sq, D, device=dev, dtype=tdt) for h in (Hq, Hkv, Hkv))

        def stepz():
            with torch.no_grad():
                aule.flash_attention(qz, kz, vz, causal=causal)

        lz = leg("c2_zero_inputs_fwd", stepz, 20, args.condition_ms, 0, False, fwd_flops(B, Hq, Sq, Sk, D, causal), PEAK_TFLOPS[dtype])
        tz = lz["tflops_mean"]
        extra.update({"c2_zero_inputs_fwd_tflops": tz, "c2_zero_inputs_frac_of_peak": tz / PEAK_TFLOPS[dtype],
                      "c2_zero_inputs_ms_per_step": lz["ms_mean_events"], "c2_zero_inputs_power_w": lz.get("power_w"),
                      "c2_zero_inputs_sclk_mhz": lz.get("sclk_mhz"),
                      "c2_zero_inputs_note": "the C2 forward on all-zero q, k, v (LSE not stored): the kernel's schedule without the "
                                             "data-dependent power of N(0,1) inputs -- NOT a throughput claim"})
        result["limiter"]["c2_fwd_zero_inputs"] = lim.during(torch, stepz, tel)
        if isinstance(result.get("roofline"), dict):
            # beside frac / frac_steady: what the same kernel reaches of the peak when the power cap is out of the way
            result["roofline"]["frac_zero_inputs"] = tz / PEAK_TFLOPS[dtype]
        del qz, kz, vz

    if rank == 0:
        result["legs"] = legs
        if dumped is not None:
            result["outputs"] = {"dir": args.dump_outputs, "arrays": dumped, "dtype": "float32",
                                 "note": "the last timed step's outputs; arrays with rows_kept < rows hold a fixed, seeded sample of rows"}

    if rank == 0:
        # the reference harness counts 4*B*H*S^2*D with NO causal discount (tests/benchmark_attention.zig:68-75):
        # for a causal shape that includes the masked half, so it is about twice `value`.  Printed for comparison with the
        # reference's own reports only, labelled, and never used for `value` or the roofline.
        f_ref = 4.0 * B * Hq * Sq * Sk * D * (3.5 if mode == "fwdbwd" else 1.0)
        result["ref_harness_convention"] = {
            "tflops": f_ref * n_gpus * args.steps / wall / 1e12,
            "formula": "4*B*Hq*Sq*Sk*D (x3.5 fwd+bwd), no causal discount -- counts masked work; NOT achieved throughput",
            "ratio_to_value": f_ref / f_step}

    if args.full and rank == 0 and n_gpus == 1 and not args.no_cpu_baseline:
        result["cpu_baseline"] = cpu_baseline()

    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
