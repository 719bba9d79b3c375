#!/usr/bin/env python3
"""Paged KV cache append: the fused call (aule.paged_kv_append, one launch) against the composition a user had to write
before it existed -- gather the table rows, rope_raw on K, divide / clamp / cast for an FP8 cache, index_copy_ for K and
for V -- on the same tensors in the same process, alternated round by round, warm.

Shapes: decode-sized T = 8 and 64, prefill-sized T = 8192 and 65536; heads_kv 8, head_dim 128, bf16 inputs; 16-bit and
FP8 caches; with and without the rotation.  Per leg the median over the rounds and the spread (min .. max) of both, the
ratio, and for the prefill sizes the fused call's algorithmic bytes (read K and V, write both cache rows) over its time
against the 8 TB/s HBM figure.  Before a leg is timed, the two ways are checked to leave the same bits in the caches.

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in
this one process and the first failure stops the run.  --out FILE also writes the table there.
--rounds N (default 9), --tokens T (one size only)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402
from aule import _torch as at  # noqa: E402

HKV, D, BS = 8, 128, 16
HBM_PEAK = 8.0e12


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(T, fp8, rope, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(T + 2 * fp8 + rope)
    dt = torch.bfloat16
    key = torch.randn(T, HKV, D, device="cuda", dtype=dt, generator=g)
    value = torch.randn(T, HKV, D, device="cuda", dtype=dt, generator=g)
    nslots = max(2 * T, 4096)
    nb = nslots // BS
    slots = torch.randperm(nslots, device="cuda", generator=g)[:T].to(torch.int64)
    cdt = torch.uint8 if fp8 else dt
    caches = [torch.zeros(nb, BS, HKV, D, device="cuda", dtype=cdt) for _ in range(4)]
    if fp8:
        caches = [c.view(torch.float8_e4m3fn) for c in caches]
    fk, fv, ck, cv = caches
    ks = torch.linspace(0.01, 0.02, HKV, device="cuda")
    vs = torch.linspace(0.02, 0.01, HKV, device="cuda")
    cos, sin = aule.precompute_rope_frequencies(max(T, 4096), D, device="cuda")
    cos, sin = cos.contiguous(), sin.contiguous()
    pos = torch.randint(0, cos.shape[0], (T,), device="cuda", generator=g)
    kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    if rope:
        kw.update(cos=cos, sin=sin, positions=pos)

    def fused():
        aule.paged_kv_append(key, value, fk, fv, slots, **kw)

    def composed():
        kk = key
        if rope:
            kk = at.rope_raw(key.transpose(0, 1)[None].contiguous(), cos[pos], sin[pos], "half")[0].transpose(0, 1)
        if fp8:
            kq = (kk.float() / ks.view(1, -1, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
            vq = (value.float() / vs.view(1, -1, 1)).clamp_(-448, 448).to(torch.float8_e4m3fn)
            ck.view(torch.uint8).view(-1, HKV, D).index_copy_(0, slots, kq.view(torch.uint8))
            cv.view(torch.uint8).view(-1, HKV, D).index_copy_(0, slots, vq.view(torch.uint8))
        else:
            ck.view(-1, HKV, D).index_copy_(0, slots, kk)
            cv.view(-1, HKV, D).index_copy_(0, slots, value)

    fused(); composed()
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.uint8) if fp8 else t.view(torch.int16)   # noqa: E731
    if not (torch.equal(bits(fk), bits(ck)) and torch.equal(bits(fv), bits(cv))):
        raise SystemExit(f"T {T} fp8 {fp8} rope {rope}: the fused call and the composition left different caches")
    iters = 200 if T <= 64 else (50 if T <= 8192 else 20)
    calls = {"fused": fused, "composed": composed}
    for f in calls.values():
        for _ in range(10):
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
    byt = T * HKV * D * 2 * (2 + (1 if fp8 else 2))
    line = (f"  T {T:6d} {'fp8 ' if fp8 else '16b '} {'rope' if rope else 'plain'}: fused {med['fused']:8.1f} ({min(t['fused']):8.1f} .. "
            f"{max(t['fused']):8.1f}) us   composed {med['composed']:8.1f} ({min(t['composed']):8.1f} .. {max(t['composed']):8.1f}) us   "
            f"composed / fused {med['composed'] / med['fused']:6.2f}x")
    if T >= 8192:
        rate = byt / (med["fused"] * 1e-6)
        line += f"   fused {byt / 1e6:7.1f} MB -> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f}% of 8 TB/s"
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_append needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 9), _arg("--leg-timeout", 120)
    sizes = (_arg("--tokens", 0),) if "--tokens" in sys.argv else (8, 64, 8192, 65536)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_kv_append.py   (one MI355X; heads_kv {HKV}, head_dim {D}, block_size {BS}, bf16 key / value, random slots and "
            f"positions; {rounds} alternated rounds, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for T in sizes:
        for fp8 in (False, True):
            for rope in (False, True):
                signal.alarm(budget)
                leg(T, fp8, rope, rounds, lines)
                signal.alarm(0)
    if "--out" in sys.argv:
        with open(_arg("--out", "", str), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
