#!/usr/bin/env python3
"""The indexer's write side: the fused calls (aule.mla_indexer_k_append, aule.mla_indexer_q_rotate, one launch each) against the
torch-op route they replace -- LayerNorm, split / rotate / cat, the Hadamard matmul, amax / divide / clamp / cast and the scatters
through the slot mapping -- on the same tensors in the same process, alternated round by round, warm.

Shapes: keys T = 1, 64, 4096, 65536 into a 16-bit and an FP8 cache (norm with bias, "half" RoPE, Hadamard); queries T = 1, 64,
2048 x 64 heads (RoPE, Hadamard); bf16.  Per leg the median over the rounds and the spread (min .. max) of both, the ratio, and
for the large sizes the fused call's algorithmic bytes over its time against the 8 TB/s HBM figure.  Before a leg is timed the two
routes are compared (they round the same fp32 formulas once; the sums run in another order, so a 16-bit ulp may differ).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  --out FILE also
writes the table there.  --rounds N (default 9)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import aule  # noqa: E402

HQ, BS, EPS, TABLE = 64, 64, 1e-6, 8192
HBM_PEAK = 8.0e12


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _hadamard():
    i = torch.arange(128, device="cuda")
    bits = i[:, None] & i[None, :]
    parity = sum((bits >> n) & 1 for n in range(7)) & 1
    return (1 - 2 * parity).float() * 2.0 ** -3.5


def _rotate(x, c, s):
    """x [..., 128] fp32: "half" pairs of the first 64 elements by c, s broadcastable to [..., 32]"""
    x1, x2, rest = x[..., :32], x[..., 32:64], x[..., 64:]
    return torch.cat((x1 * c - x2 * s, x1 * s + x2 * c, rest), -1)


def _time(calls, iters, rounds):
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
    return t


def _line(what, t, nbytes, big):
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    ratio = med["torch"] / med["fused"]
    line = (f"  {what}: fused {med['fused']:8.1f} ({min(t['fused']):8.1f} .. {max(t['fused']):8.1f}) us   torch ops {med['torch']:8.1f} "
            f"({min(t['torch']):8.1f} .. {max(t['torch']):8.1f}) us   torch / fused {ratio:6.2f}x{'   **loses**' if ratio < 1 else ''}")
    if big:
        rate = nbytes / (med["fused"] * 1e-6)
        line += f"   fused {nbytes / 1e6:7.1f} MB -> {rate / 1e12:5.2f} TB/s = {100 * rate / HBM_PEAK:4.1f}% of 8 TB/s"
    return line


def key_leg(T, fp8, rounds, Hm, cos, sin):
    g = torch.Generator(device="cuda").manual_seed(T + fp8)
    k = torch.randn(T, 128, device="cuda", generator=g).to(torch.bfloat16)
    w, b = 1 + 0.1 * torch.randn(128, device="cuda", generator=g), 0.1 * torch.randn(128, device="cuda", generator=g)
    nb = max(2 * T, 4096) // BS
    slots = torch.randperm(nb * BS, device="cuda", generator=g)[:T]
    pos = torch.randint(0, TABLE, (T,), device="cuda", generator=g)
    cdt = torch.float8_e4m3fn if fp8 else torch.bfloat16
    fc, tc = (torch.zeros(nb, BS, 128, device="cuda", dtype=torch.uint8 if fp8 else cdt).view(cdt) for _ in range(2))
    fs, ts = (torch.ones(nb, BS, device="cuda") if fp8 else None for _ in range(2))

    def fused():
        aule.mla_indexer_k_append(k, fc, slots, k_scale=fs, norm_weight=w, norm_bias=b, eps=EPS, cos=cos, sin=sin, positions=pos)

    def composed():
        x = F.layer_norm(k.float(), (128,), w, b, EPS)
        r = (_rotate(x, cos[pos], sin[pos]) @ Hm).to(torch.bfloat16)
        if not fp8:
            tc.view(-1, 128).index_copy_(0, slots, r)
            return
        amax = r.float().abs().amax(-1)
        scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
        codes = (r.float() / scale[:, None]).clamp_(-448, 448).to(torch.float8_e4m3fn)
        tc.view(torch.uint8).view(-1, 128).index_copy_(0, slots, codes.view(torch.uint8))
        ts.view(-1).index_copy_(0, slots, scale)

    fused(); composed()
    torch.cuda.synchronize()
    deq = lambda c, s: c.float() * s[..., None] if fp8 else c.float()   # noqa: E731
    a, c = deq(fc, fs), deq(tc, ts)
    if not bool(((a - c).abs() <= (2.0 ** -3 if fp8 else 2.0 ** -7) * c.abs() + 1e-3).all()):
        raise SystemExit(f"keys T {T} fp8 {fp8}: the fused call and the torch route left different caches")
    t = _time({"fused": fused, "torch": composed}, 200 if T <= 64 else (50 if T <= 4096 else 20), rounds)
    return _line(f"keys    T {T:6d} {'fp8 ' if fp8 else '16b '}", t, T * (256 + (132 if fp8 else 256)), T >= 4096)


def query_leg(T, rounds, Hm, cos, sin):
    g = torch.Generator(device="cuda").manual_seed(T)
    q = torch.randn(T, HQ, 128, device="cuda", generator=g).to(torch.bfloat16)
    pos = torch.randint(0, TABLE, (T,), device="cuda", generator=g)
    out = torch.empty_like(q)
    res = {}

    def fused():
        aule.mla_indexer_q_rotate(q, cos=cos, sin=sin, positions=pos, out=out)

    def composed():
        res["q"] = (_rotate(q.float(), cos[pos][:, None], sin[pos][:, None]) @ Hm).to(torch.bfloat16)

    fused(); composed()
    torch.cuda.synchronize()
    if not bool(((out.float() - res["q"].float()).abs() <= 2.0 ** -7 * res["q"].float().abs() + 1e-3).all()):
        raise SystemExit(f"queries T {T}: the fused call and the torch route differ")
    t = _time({"fused": fused, "torch": composed}, 200 if T <= 64 else 50, rounds)
    return _line(f"queries T {T:6d} x {HQ} ", t, T * HQ * 512, T >= 2048)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_indexer_append needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 9), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    Hm = _hadamard()
    ang = torch.arange(TABLE, device="cuda", dtype=torch.float64)[:, None] * 10000.0 ** (-torch.arange(32, device="cuda", dtype=torch.float64) / 32)
    cos, sin = ang.cos().float(), ang.sin().float()
    head = (f"# tools/bench_mla_indexer_append.py   (one MI355X; bf16 rows of 128, block_size {BS}, random slots and positions; {rounds} "
            f"alternated rounds, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    legs = [lambda T=T, fp8=fp8: key_leg(T, fp8, rounds, Hm, cos, sin) for T in (1, 64, 4096, 65536) for fp8 in (False, True)]
    legs += [lambda T=T: query_leg(T, rounds, Hm, cos, sin) for T in (1, 64, 2048)]
    for leg in legs:
        signal.alarm(budget)
        lines.append(leg())
        signal.alarm(0)
        print(lines[-1], flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", "", str), "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
