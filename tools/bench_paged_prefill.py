#!/usr/bin/env python3
"""Paged prefill: aule.flash_attention_paged_prefill (one launch over the ragged batch, the cache read in place) against the
only route there was before it -- gather each sequence's whole history out of the block pool into contiguous K / V
[1, Hkv, L, D] (an FP8 cache: dequantised to the query's type on the way) and call
aule.flash_attention(causal="bottom-right") once per sequence -- on the same tensors in the same process, alternated round by
round, warm.  The gather route is timed twice: with the gather (what a serving step pays) and with K / V gathered beforehand
(the attention calls alone: what the tiled dense kernels do with the same problem).

Shapes: bf16 queries, 32 query / 8 KV heads, head_dim 128, block 16, shuffled block table; 16-bit and FP8 caches.
  (a) 8 sequences x 512 new tokens behind prefixes of 0, 4 K and 32 K keys;
  (b) a mixed step at 8 K context: one 2048-token chunk, four 5-token verifies, 27 decodes.
Per leg the median over the rounds and the spread (min .. max) of the three, the two ratios, and the call's arithmetic
(4 D flops per visible (query, key) pair and head) over its time.  Before a leg is timed the two routes are compared (the
forward bound of tests/util.py).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in this
one process and the first failure stops the run.  A timed window repeats its call until it holds about 40 ms of device time.  --out FILE also
writes the table there.  --rounds N (default 5)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
WINDOW_MS = 40
BATCHES = [  # name, [(new tokens, keys in the cache, the new ones included)]
    ("8 x 512, no prefix", [(512, 512)] * 8),
    ("8 x 512, prefix 4 K", [(512, 4096 + 512)] * 8),
    ("8 x 512, prefix 32 K", [(512, 32768 + 512)] * 8),
    ("mixed 2048 + 4 x 5 + 27 x 1 at 8 K", [(2048, 8192)] + [(5, 8192)] * 4 + [(1, 8192)] * 27),
]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(name, seqs, fp8, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(len(seqs) + 2 * fp8 + seqs[0][1])
    dt = torch.bfloat16
    B = len(seqs)
    ns, Ls = [n for n, _ in seqs], [L for _, L in seqs]
    nblk = [(L + BS - 1) // BS for L in Ls]
    nb, T = sum(nblk), sum(ns)
    q = torch.randn(T, HQ, D, device="cuda", dtype=dt, generator=g)
    kc = torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
    vc = torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
    kw = {}
    if fp8:
        kc, ks = aule.quantize_kv_cache_fp8(kc)
        vc, vs = aule.quantize_kv_cache_fp8(vc)
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
    rows = [bt[b, :nblk[b]].long() for b in range(B)]

    def paged():
        return aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=max_sq, **kw)

    def gather(c, s, b):
        x = c[rows[b]]                                            # [nblk, BS, HKV, D]
        if fp8:
            x = (x.float() * s.view(1, 1, HKV, 1)).to(dt)
        return x.view(1, nblk[b] * BS, HKV, D)[:, :Ls[b]].permute(0, 2, 1, 3).contiguous()

    def gather_all():
        return [(gather(kc, kw.get("k_scale"), b), gather(vc, kw.get("v_scale"), b)) for b in range(B)]

    def dense(kv):
        out = torch.empty_like(q)
        for b in range(B):
            qb = q[cu_host[b]:cu_host[b + 1]].permute(1, 0, 2).unsqueeze(0)          # [1, HQ, n, D] (flash_attention copies it)
            out[cu_host[b]:cu_host[b + 1]] = aule.flash_attention(qb, kv[b][0], kv[b][1], causal="bottom-right")[0].permute(1, 0, 2)
        return out

    held = gather_all()
    a, b_ = paged(), dense(held)
    torch.cuda.synchronize()
    vmax = float((vc.float() * vs.view(1, 1, HKV, 1)).abs().max()) if fp8 else float(vc.float().abs().max())
    bound = 1e-3 + 2.0 ** -9 * vmax + 2.0 ** -8 * b_.float().abs()
    if not bool(((a.float() - b_.float()).abs() <= bound).all()):
        raise SystemExit(f"{name} fp8 {fp8}: the paged prefill and the gather route disagree")
    pairs = sum(sum(min(L - n + i + 1, L) for i in range(n) if L - n + i >= 0) for n, L in seqs)
    flops = 4.0 * D * HQ * pairs
    calls = {"paged": paged, "gather+dense": lambda: dense(gather_all()), "dense": lambda: dense(held)}

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
    line = (f"  {name:36s} {'fp8' if fp8 else '16b'}: paged prefill {span['paged']} us   gather + per-sequence bottom-right {span['gather+dense']} us"
            f"   the same, K / V gathered beforehand {span['dense']} us   with gather / prefill {med['gather+dense'] / med['paged']:5.2f}x"
            f"   without gather / prefill {med['dense'] / med['paged']:5.2f}x   {flops / 1e9:8.1f} GFLOP -> {flops / (med['paged'] * 1e-6) / 1e12:6.1f} TFLOP/s")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_prefill needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_paged_prefill.py   (one MI355X; {HQ} q / {HKV} kv heads, head_dim {D}, block_size {BS}, bf16 queries, shuffled "
            f"block table; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for name, seqs in BATCHES:
        for fp8 in (False, True):
            signal.alarm(budget)
            leg(name, seqs, fp8, rounds, lines)
            signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
