#!/usr/bin/env python3
"""Paged attention for short multi-token queries: aule.flash_attention_paged_query (the cache is read in place) against what
a user had to write before it existed -- gather the pages into contiguous K / V [B, Hkv, L, D] (an FP8 cache: dequantised to
the query's type on the way) and call aule.flash_attention(causal="bottom-right") -- on the same tensors in the same
process, alternated round by round, warm.  At one token per sequence the comparison is aule.flash_attention_paged_amd.

Shapes: batch 8, 32 query / 8 KV heads, head_dim 128, block 16, shuffled block table, bf16 queries; 1, 4 and 8 tokens per
sequence at 8 K and 32 K context; 16-bit and FP8 caches.  Per leg the median over the rounds and the spread (min .. max)
of both, the ratio, and the call's algorithmic bytes (K and V of every sequence read once) over its time against the
8 TB/s HBM figure.  Before a leg is timed the two ways are compared (the forward bound of tests/util.py).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in
this one process and the first failure stops the run.  --out FILE also writes the table there.  --rounds N (default 7)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

B, HQ, HKV, D, BS = 8, 32, 8, 128, 16
HBM_PEAK = 8.0e12


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(ctx, Sq, fp8, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(ctx + 64 * Sq + fp8)
    dt = torch.bfloat16
    nb = ctx // BS
    q = torch.randn(B, HQ, Sq, D, device="cuda", dtype=dt, generator=g)
    if fp8:
        kc, ks = aule.quantize_kv_cache_fp8(torch.randn(B * nb, BS, HKV, D, device="cuda", dtype=dt, generator=g))
        vc, vs = aule.quantize_kv_cache_fp8(torch.randn(B * nb, BS, HKV, D, device="cuda", dtype=dt, generator=g))
        kw = dict(k_scale=ks, v_scale=vs)
    else:
        kc = torch.randn(B * nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
        vc = torch.randn(B * nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
        kw = {}
    bt = torch.randperm(B * nb, device="cuda", generator=g).to(torch.int32).view(B, nb)
    cl = torch.full((B,), ctx, device="cuda", dtype=torch.int32)
    rows = bt.long()

    def paged():
        return aule.flash_attention_paged_query(q, kc, vc, bt, cl, **kw)

    def gathered(c, s):
        x = c[rows]                                            # [B, nb, BS, HKV, D]
        if fp8:
            x = (x.float() * s.view(1, 1, 1, HKV, 1)).to(dt)
        return x.view(B, ctx, HKV, D).permute(0, 2, 1, 3).contiguous()

    if Sq == 1:
        other_name = "paged decode"

        def other():
            return aule.flash_attention_paged_amd(q[:, :, 0], kc, vc, bt, cl, **kw).unsqueeze(2)
    else:
        other_name = "gather + bottom-right"

        def other():
            return aule.flash_attention(q, gathered(kc, kw.get("k_scale")), gathered(vc, kw.get("v_scale")), causal="bottom-right")

    a, b = paged(), other()
    torch.cuda.synchronize()
    vmax = float((vc.float() * vs.view(1, 1, HKV, 1)).abs().max()) if fp8 else float(vc.float().abs().max())
    bound = 1e-3 + 2.0 ** -9 * vmax + 2.0 ** -8 * b.float().abs()
    if not bool(((a.float() - b.float()).abs() <= bound).all()):
        raise SystemExit(f"ctx {ctx} Sq {Sq} fp8 {fp8}: the paged query and {other_name} disagree")
    iters = 50 if ctx <= 8192 else 20
    calls = {"paged": paged, "other": other}
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / iters * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    byt = 2 * B * ctx * HKV * D * (1 if fp8 else 2)
    rate = byt / (med["paged"] * 1e-6)
    line = (f"  ctx {ctx:6d} Sq {Sq} {'fp8' if fp8 else '16b'}: paged query {med['paged']:8.1f} ({min(t['paged']):8.1f} .. {max(t['paged']):8.1f}) us   "
            f"{other_name:21s} {med['other']:8.1f} ({min(t['other']):8.1f} .. {max(t['other']):8.1f}) us   other / paged query "
            f"{med['other'] / med['paged']:6.2f}x   {byt / 1e6:7.1f} MB -> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f}% of 8 TB/s")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_query needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 7), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_paged_query.py   (one MI355X; batch {B}, {HQ} q / {HKV} kv heads, head_dim {D}, block_size {BS}, bf16 queries, "
            f"shuffled block table; {rounds} alternated rounds, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for ctx in (8192, 32768):
        for fp8 in (False, True):
            for Sq in (1, 4, 8):
                signal.alarm(budget)
                leg(ctx, Sq, fp8, rounds, lines)
                signal.alarm(0)
    if "--out" in sys.argv:
        with open(_arg("--out", "", str), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
