#!/usr/bin/env python3
"""Variable-length packed batches: aule.flash_attention_varlen (one launch over the packed batch forward, three backward) against
the two routes there were before it, on the same tensors in the same process, alternated round by round, warm:
  per-sequence   one aule.flash_attention call per sequence on its slice of the packed tensors (needs the lengths on the host);
  padded         one aule.flash_attention call on [B, H, max length, D] tensors padded beforehand (the padding itself is NOT timed;
                 under the causal rule the padded keys lie behind every real query, so no extra mask is needed; the padded rows'
                 results are thrown away and their dout is zero).
Causal self-attention (n = L per sequence), bf16, 32 query / 8 KV heads, head_dim 128.  Forward alone (no autograd) and forward +
backward (torch.autograd.grad of all three inputs).

Shapes: (a) equal lengths 8 x 4096; (b) a packed SFT mix, 64 sequences of 64 .. 4096 tokens totalling 32 K (seeded); (c) 512 x 64.
Per leg the median over the rounds and the spread (min .. max) of each route, the two ratios (other route / varlen: above 1 the
varlen call wins), and the call's arithmetic (4 D flops per visible (query, key) pair and head forward, 2.5 times that backward)
over its time.  Before a leg is timed the varlen result is compared with the per-sequence route's (the forward bound of tests/util.py).

Every leg runs under its own alarm (--leg-timeout seconds, default 180): a leg that hangs ends the process.  A timed window repeats
its call until it holds about 40 ms of device time.  --out FILE also writes the table there.  --rounds N (default 5)."""
import os
import random
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, D = 32, 8, 128
WINDOW_MS = 40


def sft_mix(count=64, lo=64, hi=4096, total=32768, seed=0):
    """`count` lengths in [lo, hi], log-uniform before they are scaled to sum to `total`"""
    rng = random.Random(seed)
    raw = [lo * (hi / lo) ** rng.random() for _ in range(count)]
    f = (total - count * lo) / sum(x - lo for x in raw)
    ns = [int(lo + (x - lo) * f) for x in raw]
    ns[ns.index(min(ns))] += total - sum(ns)
    assert sum(ns) == total and lo <= min(ns) and max(ns) <= hi
    return ns


BATCHES = [("8 x 4096", [4096] * 8), ("SFT mix 64 seqs, 64 .. 4096, 32 K", sft_mix()), ("512 x 64", [64] * 512)]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(name, ns, backward, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(len(ns) + ns[0])
    dt = torch.bfloat16
    B, T, S = len(ns), sum(ns), max(ns)
    cu_host = [0]
    for n in ns:
        cu_host.append(cu_host[-1] + n)
    cu = torch.tensor(cu_host, device="cuda", dtype=torch.int32)
    q, dout = (torch.randn(T, HQ, D, device="cuda", dtype=dt, generator=g) for _ in range(2))
    k, v = (torch.randn(T, HKV, D, device="cuda", dtype=dt, generator=g) for _ in range(2))

    def padded_of(x):
        p = torch.zeros(B, x.shape[1], S, D, device="cuda", dtype=dt)
        for b in range(B):
            p[b, :, :ns[b]] = x[cu_host[b]:cu_host[b + 1]].permute(1, 0, 2)
        return p

    qp, kp, vp, dp = padded_of(q), padded_of(k), padded_of(v), padded_of(dout)
    if backward:
        for x in (q, k, v, qp, kp, vp):
            x.requires_grad_(True)

    def varlen():
        out = aule.flash_attention_varlen(q, k, v, cu, cu, max_seqlen_q=S, max_seqlen_k=S, causal=True)
        return torch.autograd.grad(out, (q, k, v), dout) if backward else out

    def per_sequence():
        outs = []
        for b in range(B):
            s, e = cu_host[b], cu_host[b + 1]
            qb, kb, vb = (x[s:e].permute(1, 0, 2).unsqueeze(0) for x in (q, k, v))     # [1, H, n, D] (flash_attention copies it)
            outs.append(aule.flash_attention(qb, kb, vb, causal=True)[0].permute(1, 0, 2))
        if backward:
            return torch.autograd.grad(outs, (q, k, v), [dout[cu_host[b]:cu_host[b + 1]] for b in range(B)])
        return torch.cat(outs)

    def padded():
        out = aule.flash_attention(qp, kp, vp, causal=True)
        return torch.autograd.grad(out, (qp, kp, vp), dp) if backward else out

    a, b_ = varlen(), per_sequence()
    torch.cuda.synchronize()
    if backward:
        for x, y, what in zip(a, b_, ("dq", "dk", "dv")):
            scale = max(1.0, float(y.float().abs().max()))
            if not bool(((x.float() - y.float()).abs() <= 5e-3 * scale + 1e-2 * y.float().abs()).all()):
                raise SystemExit(f"{name}: {what} of the varlen call and of the per-sequence route disagree")
    else:
        bound = 1e-3 + 2 * 2.0 ** -9 * float(v.float().abs().max()) + 2.0 ** -7 * b_.float().abs()
        if not bool(((a.float() - b_.float()).abs() <= bound).all()):
            raise SystemExit(f"{name}: the varlen call and the per-sequence route disagree")
    del a, b_
    pairs = sum(n * (n + 1) // 2 for n in ns)
    flops = 4.0 * D * HQ * pairs * (3.5 if backward else 1.0)
    calls = {"varlen": varlen, "per-sequence": per_sequence, "padded": padded}

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
    t = {key: [] for key in calls}
    with torch.set_grad_enabled(backward):
        for _ in range(rounds):
            for key, f in calls.items():
                t[key].append(window(f, iters[key]))
    med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
    span = {key: f"{med[key]:9.1f} ({min(x):9.1f} .. {max(x):9.1f})" for key, x in t.items()}
    line = (f"  {name:34s} {'fwd+bwd' if backward else 'fwd    '}: varlen {span['varlen']} us   one flash_attention per sequence {span['per-sequence']} us"
            f"   one padded dense call {span['padded']} us   per-sequence / varlen {med['per-sequence'] / med['varlen']:5.2f}x"
            f"   padded / varlen {med['padded'] / med['varlen']:5.2f}x   {flops / 1e9:8.1f} GFLOP -> {flops / (med['varlen'] * 1e-6) / 1e12:6.1f} TFLOP/s")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_varlen needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 180)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_varlen.py   (one MI355X; causal self-attention, {HQ} q / {HKV} kv heads, head_dim {D}, bf16; {rounds} alternated rounds of "
            f"~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included; the padded route's padding is not timed)")
    print(head, flush=True)
    lines = [head]
    for name, ns in BATCHES:
        for backward in (False, True):
            signal.alarm(budget)
            leg(name, ns, backward, rounds, lines)
            signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
