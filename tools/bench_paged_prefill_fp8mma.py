#!/usr/bin/env python3
"""Paged prefill over an FP8 cache: aule.flash_attention_paged_prefill_fp8mma (both matrix products in e4m3, the cache's codes
multiplied as they are) against aule.flash_attention_paged_prefill (the codes turned back into bf16 on the way into LDS, 16-bit
MFMAs) on the same FP8 cache, the same tensors, in the same process, alternated round by round, warm.

Shapes: bf16 queries, 32 query / 8 KV heads, block 16, shuffled block table, the legs of tools/bench_paged_prefill.py:
  (a) 8 sequences x 512 new tokens behind prefixes of 0, 4 K and 32 K keys;
  (b) a mixed step at 8 K context: one 2048-token chunk, four 5-token verifies, 27 decodes;
at head_dim 128, and leg (a) behind the 32 K prefix at head_dim 64 as well.
Per leg the median over the rounds and the spread (min .. max) of both entries, the ratio, and the call's arithmetic (4 D flops per
visible (query, key) pair and head) over each time.  Before a leg is timed the two entries are compared: they differ by the e4m3
rounding of q and of the softmax weights, so the check is coarse (rms of the difference against the rms of the result) and only
catches a wrong kernel.

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in this one
process and the first failure stops the run.  A timed window repeats its call until it holds about 40 ms of device time.  --out FILE
also writes the table there.  --rounds N (default 5)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, BS = 32, 8, 16
WINDOW_MS = 40
LEGS = [  # name, head_dim, [(new tokens, keys in the cache, the new ones included)]
    ("8 x 512, no prefix", 128, [(512, 512)] * 8),
    ("8 x 512, prefix 4 K", 128, [(512, 4096 + 512)] * 8),
    ("8 x 512, prefix 32 K", 128, [(512, 32768 + 512)] * 8),
    ("mixed 2048 + 4 x 5 + 27 x 1 at 8 K", 128, [(2048, 8192)] + [(5, 8192)] * 4 + [(1, 8192)] * 27),
    ("8 x 512, prefix 32 K", 64, [(512, 32768 + 512)] * 8),
]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(name, D, seqs, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(len(seqs) + D + seqs[0][1])
    dt = torch.bfloat16
    B = len(seqs)
    ns, Ls = [n for n, _ in seqs], [L for _, L in seqs]
    nblk = [(L + BS - 1) // BS for L in Ls]
    nb, T = sum(nblk), sum(ns)
    q = torch.randn(T, HQ, D, device="cuda", dtype=dt, generator=g)
    kc, ks = aule.quantize_kv_cache_fp8(torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g))
    vc, vs = aule.quantize_kv_cache_fp8(torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g))
    kw = dict(k_scale=ks, v_scale=vs)
    perm = torch.randperm(nb, device="cuda", generator=g).to(torch.int32)
    bt = torch.zeros(B, max(nblk), device="cuda", dtype=torch.int32)
    at = 0
    for b in range(B):
        bt[b, :nblk[b]] = perm[at:at + nblk[b]]
        at += nblk[b]
    cl = torch.tensor(Ls, device="cuda", dtype=torch.int32)
    cu_host = [0]
    for n in ns:
        cu_host.append(cu_host[-1] + n)
    cu = torch.tensor(cu_host, device="cuda", dtype=torch.int32)
    max_sq = max(ns)
    calls = {"fp8mma": lambda: aule.flash_attention_paged_prefill_fp8mma(q, kc, vc, bt, cl, cu, max_seqlen_q=max_sq, **kw),
             "16-bit": lambda: aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=max_sq, **kw)}
    a, b_ = calls["fp8mma"]().float(), calls["16-bit"]().float()
    torch.cuda.synchronize()
    rel = float((a - b_).pow(2).mean().sqrt() / b_.pow(2).mean().sqrt())
    if not rel < 0.1:
        raise SystemExit(f"{name} D {D}: the two entries disagree (rms of the difference / rms of the result = {rel:.3g})")
    pairs = sum(sum(min(L - n + i + 1, L) for i in range(n) if L - n + i >= 0) for n, L in seqs)
    flops = 4.0 * D * HQ * pairs

    def window(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    # warm, then size every timed window to about WINDOW_MS of device time (a shorter one measures the clock and the scheduler)
    iters = {}
    for key, f in calls.items():
        window(f, 2)
        iters[key] = min(400, max(3, int(WINDOW_MS * 1e3 / window(f, 2)) + 1))
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(window(f, iters[key]))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    span = {k: f"{med[k]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})" for k, v in t.items()}
    tf = {k: flops / (med[k] * 1e-6) / 1e12 for k in calls}
    ratio = med["16-bit"] / med["fp8mma"]
    line = (f"  D {D:3d}  {name:36s}: fp8mma {span['fp8mma']} us = {tf['fp8mma']:6.1f} TFLOP/s   16-bit products {span['16-bit']} us = "
            f"{tf['16-bit']:6.1f} TFLOP/s   16-bit / fp8mma {ratio:5.2f}x {'      ' if ratio >= 1.0 else ' LOSES'}   "
            f"{flops / 1e9:8.1f} GFLOP   rms diff / rms {rel:.4f}")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_prefill_fp8mma needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_paged_prefill_fp8mma.py   (one MI355X; {HQ} q / {HKV} kv heads, block_size {BS}, bf16 queries, FP8 e4m3 cache, "
            f"shuffled block table; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for name, D, seqs in LEGS:
        signal.alarm(budget)
        leg(name, D, seqs, rounds, lines)
        signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
