#!/usr/bin/env python3
"""Timing of head_dim 256 (fa_fwd_d256_gfx950.hip / fa_bwd_d256_gfx950.hip) and of a head size padded to it, against PyTorch's
own scaled_dot_product_attention on the same tensors (what the SDPA shim used to fall back to above head_dim 128) and against the
D = 128 C2 forward at equal FLOPs.

Device events around every step, median of --steps timed steps after --warmup untimed ones.  FLOPs: forward
4 B Hq D P with P the visible (query, key) pairs and D the LOGICAL head size (160 counts as 160, not as the padded 256); backward
2.5x the forward.  One JSON line per measurement.
    python tools/d256_bench.py [--steps 20] [--warmup 5] [--only fwd256,...]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import aule  # noqa: E402

SDPA = F.scaled_dot_product_attention   # PyTorch's own (aule.install() is never called here)


def pairs(Sq, Sk, causal):
    if not causal:
        return Sq * Sk
    return sum(min(i + 1, Sk) for i in range(Sq))


def fwd_flops(B, Hq, Sq, Sk, D, causal):
    return 4.0 * B * Hq * D * pairs(Sq, Sk, causal)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def make(B, Hq, Hkv, Sq, Sk, D, dtype, grad):
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda h, s: torch.randn(B, h, s, D, device="cuda", generator=g).to(dtype).requires_grad_(grad)
    return mk(Hq, Sq), mk(Hkv, Sk), mk(Hkv, Sk), torch.randn(B, Hq, Sq, D, device="cuda", generator=g).to(dtype)


def leg(name, impl, mode, shape, steps, warmup):
    B, Hq, Hkv, Sq, Sk, D, dtype, causal = shape
    q, k, v, do = make(B, Hq, Hkv, Sq, Sk, D, dtype, mode == "fwdbwd")
    if impl == "aule":
        run = lambda: aule.flash_attention(q, k, v, causal=causal)
    else:
        run = lambda: SDPA(q, k, v, is_causal=causal, enable_gqa=Hq != Hkv)
    if mode == "fwd":
        def step():
            with torch.no_grad():
                run()
    else:
        def step():
            q.grad = k.grad = v.grad = None
            run().backward(do)
    fl = fwd_flops(B, Hq, Sq, Sk, D, causal) * (1.0 if mode == "fwd" else 3.5)
    rec = {"leg": name, "impl": impl, "mode": mode, "shape": "B%d Hq%d Hkv%d Sq%d Sk%d D%d %s %s" % (
        B, Hq, Hkv, Sq, Sk, D, str(dtype).split(".")[-1], "causal" if causal else "non-causal")}
    try:
        ms = timed(step, steps, warmup)
        rec.update(ms_median=round(ms, 4), tflops=round(fl / (ms * 1e-3) / 1e12, 2))
    except (RuntimeError, torch.cuda.OutOfMemoryError) as e:   # (an SDPA backend without this shape)
        rec["error"] = str(e).splitlines()[0][:200]
    print(json.dumps(rec), flush=True)
    del q, k, v, do
    torch.cuda.empty_cache()
    return rec


LEGS = {
    "fwd256": ("fwd", (4, 16, 16, 4096, 4096, 256, torch.bfloat16, True)),
    "fwdbwd256": ("fwdbwd", (4, 16, 16, 4096, 4096, 256, torch.bfloat16, True)),
    "fwd160": ("fwd", (16, 8, 8, 1024, 1024, 160, torch.float16, False)),
    "fwdbwd160": ("fwdbwd", (16, 8, 8, 1024, 1024, 160, torch.float16, False)),
    "decode256": ("fwd", (8, 32, 8, 1, 8192, 256, torch.bfloat16, False)),
    "c2fwd128": ("fwd", (4, 32, 32, 4096, 4096, 128, torch.bfloat16, True)),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-torch", action="store_true", help="skip the PyTorch SDPA comparator")
    args = ap.parse_args()
    names = [n for n in LEGS if not args.only or n in args.only.split(",")]
    for n in names:
        mode, shape = LEGS[n]
        leg(n, "aule", mode, shape, args.steps, args.warmup)
        if not args.no_torch and n != "c2fwd128":
            leg(n, "torch_sdpa", mode, shape, args.steps, args.warmup)


if __name__ == "__main__":
    main()
