#!/usr/bin/env python3
"""Paged-KV decode throughput at the shape family of the reference's only published absolute numbers
(python/README.md:25-32: "PagedAttention Decode (batch=8)", context 1K/2K/4K/8K -> 34 397 / 20 083 / 10 915 /
5 744 tok/s on MI300X; heads and head_dim are not stated there -- LLaMA-style 32 q / 8 kv heads, D = 128, fp16,
block_size 16 are assumed here).  tok/s = batch / time per decode step (one attention layer).

--fp8 adds the FP8 leg: for fp16 and bf16 queries, the 16-bit call and the call on an e4m3fn cache with
per-head scales in the same process, alternated round by round, warm; per context the median over the rounds, the
spread (min .. max) of both, and the ratio.  K+V bytes are the bytes of the cache each call reads.  --rounds N sets the
number of rounds (default 15), --iters N the calls per round (default 50), --ctx N one context only (for a
`rocprofv3 --kernel-trace --stats` run of its own: split kernel vs combine, the KvFp8 against the Kv16 instance of fa_fwd_splitkv_kernel)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch
import aule

B, Hq, Hkv, D, bs = 8, 32, 8, 128, 16


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def fp8_leg():
    rounds, iters = _arg("--rounds", 15), _arg("--iters", 50)
    print(f"paged decode, 16-bit cache vs FP8 e4m3fn cache: batch {B}, heads {Hq}q/{Hkv}kv, head_dim {D}, block_size {bs}, "
          f"shuffled block table; {rounds} alternated rounds of {iters} calls, median (min .. max) us/step")
    for dt, name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for ctx in ((_arg("--ctx", 0),) if "--ctx" in sys.argv else (1024, 2048, 4096, 8192, 32768)):
            nb = ctx // bs
            kc = torch.randn(B * nb, bs, Hkv, D, device="cuda", dtype=dt)
            vc = torch.randn_like(kc)
            k8, ks = aule.quantize_kv_cache_fp8(kc)
            v8, vs = aule.quantize_kv_cache_fp8(vc)
            q = torch.randn(B, Hq, D, device="cuda", dtype=dt)
            bt = torch.randperm(B * nb, device="cuda").to(torch.int32).view(B, nb)
            cl = torch.full((B,), ctx, device="cuda", dtype=torch.int32)
            calls = {"16": lambda: aule.flash_attention_paged_amd(q, kc, vc, bt, cl),
                     "fp8": lambda: aule.flash_attention_paged_amd(q, k8, v8, bt, cl, k_scale=ks, v_scale=vs)}
            for f in calls.values():
                for _ in range(10):
                    f()
            torch.cuda.synchronize()
            t = {"16": [], "fp8": []}
            for _ in range(rounds):
                for key, f in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        f()
                    e1.record(); torch.cuda.synchronize()
                    t[key].append(e0.elapsed_time(e1) / iters * 1e3)
            med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
            for key, width in (("16", 2), ("fp8", 1)):
                byt = 2 * width * B * ctx * Hkv * D
                print(f"  {name} ctx {ctx:6d} {key:>3}: {med[key]:7.1f} ({min(t[key]):7.1f} .. {max(t[key]):7.1f}) us/step  "
                      f"{B / med[key] * 1e6:10.0f} tok/s  K+V read {byt / med[key] / 1e3:7.0f} GB/s")
            print(f"  {name} ctx {ctx:6d} fp8 / 16-bit time: {med['fp8'] / med['16']:.3f}")


if "--fp8" in sys.argv:
    fp8_leg()
    sys.exit(0)
print(f"paged decode: batch {B}, heads {Hq}q/{Hkv}kv, head_dim {D}, fp16, block_size {bs}")
for ctx in (1024, 2048, 4096, 8192, 32768):
    nb = ctx // bs
    kc = torch.randn(B * nb, bs, Hkv, D, device="cuda", dtype=torch.float16)
    vc = torch.randn_like(kc)
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.float16)
    bt = torch.randperm(B * nb, device="cuda").to(torch.int32).view(B, nb)
    cl = torch.full((B,), ctx, device="cuda", dtype=torch.int32)
    for _ in range(10):
        aule.flash_attention_paged_amd(q, kc, vc, bt, cl)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 200
    e0.record()
    for _ in range(n):
        aule.flash_attention_paged_amd(q, kc, vc, bt, cl)
    e1.record(); torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    byt = 2 * 2 * B * ctx * Hkv * D
    print(f"  ctx {ctx:6d}: {us:7.1f} us/step  {B / us * 1e6:10.0f} tok/s  K+V read {byt / us / 1e3:7.0f} GB/s")
