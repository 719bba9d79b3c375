#!/usr/bin/env python3
"""MLA prefill (the non-absorbed 192 / 128 form): aule.flash_attention_mla_prefill -- one launch over the packed batch, k_nope and v
read in place from the kv_b output [T, H, 256], k_pe from columns 512.. of the down-projection [T, 576] -- against the two routes
there were before it, on the same tensors in the same process, alternated round by round, warm (the method of tools/bench_varlen.py):
  dense 256   one aule.flash_attention call per sequence on [1, H, n, 256] tensors: q and K = [k_nope | k_pe] zero-padded from 192 to
              256, v from 128 to 256, the output cut back to 128 (needs the lengths on the host);
  SDPA        one torch.nn.functional.scaled_dot_product_attention call per sequence on q, K [1, H, n, 192] and v [1, H, n, 128].
Each of the two is timed twice: on tensors prepared beforehand ("bare"), and with its preparation -- building K from k_nope and
k_pe (k_pe copied into every head), the padding, the transposition -- inside the timed call ("+ prep"), which is what a caller who
holds the projections' outputs pays.  bf16, 16 heads (TP 8) and 128 heads (TP 1), scale 1/sqrt(192).

Legs: 1 x 8192 causal; 8 x 4096 causal; a ragged mix of 64 sequences of 64 .. 4096 tokens (32 K, seeded); a chunk of 2048 queries
against 8192 keys, bottom-right.  Per leg the median over the rounds and the spread (min .. max) of each route, the ratios (other
route / MLA prefill: above 1 the new call wins), and the call's arithmetic (2 (192 + 128) flops per visible (query, key) pair and
head) over its time.  Before a leg is timed the result is compared with the dense route's (the forward bound of tests/util.py for two
16-bit results).

Every leg runs under its own alarm (--leg-timeout seconds, default 240): a leg that hangs ends the process.  A timed window repeats
its call until it holds about 40 ms of device time.  --out FILE also writes the table there (after every leg).  --rounds N
(default 5), --heads 16,128, --legs 0,1,2,3."""
import math
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import aule  # noqa: E402
from bench_varlen import sft_mix  # noqa: E402

DQ, DN, DR, DV = 192, 128, 64, 128
SCALE = 1.0 / math.sqrt(DQ)
WINDOW_MS = 40
# (name, query lengths, key lengths, causal)
LEGS = [("1 x 8192 causal", [8192], [8192], True), ("8 x 4096 causal", [4096] * 8, [4096] * 8, True),
        ("ragged mix 64 seqs, 64 .. 4096, 32 K", sft_mix(), sft_mix(), True), ("chunk 2048 q x 8192 k, bottom-right", [2048], [8192], "bottom-right")]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _cu(ns):
    cu = [0]
    for n in ns:
        cu.append(cu[-1] + n)
    return cu


def leg(name, ns, ls, causal, H, rounds, emit):
    g = torch.Generator(device="cuda").manual_seed(len(ns) + ns[0] + H)
    dt = torch.bfloat16
    B, Tq, Tk = len(ns), sum(ns), sum(ls)
    hq, hk = _cu(ns), _cu(ls)
    cu_q, cu_k = (torch.tensor(c, device="cuda", dtype=torch.int32) for c in (hq, hk))
    q = torch.randn(Tq, H, DQ, device="cuda", dtype=dt, generator=g)
    kvb = torch.randn(Tk, H, DN + DV, device="cuda", dtype=dt, generator=g)     # the kv_b up-projection's output
    down = torch.randn(Tk, 512 + DR, device="cuda", dtype=dt, generator=g)      # the down-projection's: c_kv | k_pe
    k_nope, v, k_pe = kvb[..., :DN], kvb[..., DN:], down[:, 512:]
    br = causal == "bottom-right"

    def mla():
        return aule.flash_attention_mla_prefill(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q=max(ns), max_seqlen_k=max(ls), causal=causal)

    def prep_dense(b):
        """[1, H, n, 256] q, K and v of sequence b"""
        qs, ks = slice(hq[b], hq[b + 1]), slice(hk[b], hk[b + 1])
        L = hk[b + 1] - hk[b]
        qb = F.pad(q[qs], (0, 256 - DQ)).permute(1, 0, 2).unsqueeze(0).contiguous()
        kb = torch.zeros(1, H, L, 256, device="cuda", dtype=dt)
        kb[0, :, :, :DN] = k_nope[ks].permute(1, 0, 2)
        kb[0, :, :, DN:DQ] = k_pe[ks].unsqueeze(0)
        vb = F.pad(v[ks], (0, 256 - DV)).permute(1, 0, 2).unsqueeze(0).contiguous()
        return qb, kb, vb

    def prep_sdpa(b):
        qs, ks = slice(hq[b], hq[b + 1]), slice(hk[b], hk[b + 1])
        L = hk[b + 1] - hk[b]
        kb = torch.cat([k_nope[ks], k_pe[ks].unsqueeze(1).expand(L, H, DR)], dim=2).permute(1, 0, 2).unsqueeze(0)
        return q[qs].permute(1, 0, 2).unsqueeze(0), kb, v[ks].permute(1, 0, 2).unsqueeze(0)

    def run_dense(x):
        return aule.flash_attention(*x, causal=causal, scale=SCALE)[0, :, :, :DV].permute(1, 0, 2)

    masks = {}

    def run_sdpa(x):
        if not br:
            return F.scaled_dot_product_attention(*x, is_causal=True, scale=SCALE)[0].permute(1, 0, 2)
        n, L = x[0].shape[2], x[1].shape[2]
        if (n, L) not in masks:
            masks[n, L] = torch.ones(n, L, device="cuda", dtype=torch.bool).tril(L - n)
        return F.scaled_dot_product_attention(*x, attn_mask=masks[n, L], scale=SCALE)[0].permute(1, 0, 2)

    ready_dense = [prep_dense(b) for b in range(B)]
    ready_sdpa = [tuple(t.contiguous() for t in prep_sdpa(b)) for b in range(B)]
    calls = {
        "mla": mla,
        "dense": lambda: [run_dense(x) for x in ready_dense],
        "dense+prep": lambda: [run_dense(prep_dense(b)) for b in range(B)],
        "sdpa": lambda: [run_sdpa(x) for x in ready_sdpa],
        "sdpa+prep": lambda: [run_sdpa(prep_sdpa(b)) for b in range(B)],
    }
    with torch.no_grad():
        a, ref = mla(), torch.cat(calls["dense"]())
        torch.cuda.synchronize()
        bound = 1e-3 + 2 * 2.0 ** -9 * float(v.float().abs().max()) + 2.0 ** -7 * ref.float().abs()
        if not bool(((a.float() - ref.float()).abs() <= bound).all()):
            raise SystemExit(f"{name}, {H} heads: the MLA prefill call and the dense route disagree")
        del a, ref

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
            window(f, 1)
            iters[key] = min(400, max(2, int(WINDOW_MS * 1e3 / window(f, 1)) + 1))
        t = {key: [] for key in calls}
        for _ in range(rounds):
            for key, f in calls.items():
                t[key].append(window(f, iters[key]))
    med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
    span = {key: f"{med[key]:9.1f} ({min(x):9.1f} .. {max(x):9.1f})" for key, x in t.items()}
    pairs = sum((n * (n + 1) // 2 if L == n else sum(min(L, i + L - n + 1) for i in range(n) if i + L - n >= 0)) for n, L in zip(ns, ls))
    flops = 2.0 * (DQ + DV) * H * pairs
    ratio = lambda key: f"{med[key] / med['mla']:5.2f}x"   # noqa: E731
    emit(f"  {name:38s} H {H:3d}: MLA prefill {span['mla']} us   dense 256 per sequence: bare {span['dense']} us ({ratio('dense')}), + prep "
         f"{span['dense+prep']} us ({ratio('dense+prep')})   SDPA per sequence: bare {span['sdpa']} us ({ratio('sdpa')}), + prep {span['sdpa+prep']} us "
         f"({ratio('sdpa+prep')})   {flops / 1e9:8.1f} GFLOP -> {flops / (med['mla'] * 1e-6) / 1e12:6.1f} TFLOP/s")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_prefill needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 240)
    heads = [int(x) for x in _arg("--heads", "16,128", str).split(",")]
    legs = [int(x) for x in _arg("--legs", "0,1,2,3", str).split(",")]
    out = _arg("--out", "", str)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"# tools/bench_mla_prefill.py   (one MI355X; MLA prefill 192 / 128, bf16, scale 1/sqrt(192); {rounds} alternated rounds of ~{WINDOW_MS} ms "
         f"windows, median (min .. max) us per call, host launch cost included; (r x): that route's time / the MLA prefill call's)")
    for H in heads:
        for i in legs:
            name, ns, ls, causal = LEGS[i]
            signal.alarm(budget)
            leg(name, ns, ls, causal, H, rounds, emit)
            signal.alarm(0)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
