#!/usr/bin/env python3
"""MLA 192 / 128 attention, forward + backward: aule.flash_attention_mla_varlen with autograd -- one forward launch and three or four
backward launches over the packed batch, k_nope and v read in place from the kv_b output [T, H, 256], k_pe from columns 512.. of
the down-projection [T, 576], dk_nope and dv written as the halves of one [T, H, 256] buffer -- against the two routes there were
before it, on the same tensors in the same process, alternated round by round, warm (the method of tools/bench_mla_prefill.py):
  dense 256   one aule.flash_attention call per sequence, with autograd, on [1, H, n, 256] tensors: q and K = [k_nope | k_pe]
              zero-padded from 192 to 256, v from 128 to 256 (needs the lengths on the host);
  SDPA        one torch.nn.functional.scaled_dot_product_attention call per sequence, with autograd, on q, K [1, H, n, 192] and
              v [1, H, n, 128].
Each of the two is timed twice: on tensors prepared beforehand ("bare": the gradients are those of the padded / concatenated
tensors), and with its preparation -- building K from k_nope and k_pe (k_pe copied into every head), the padding, the transposition,
and on the way back autograd's slicing and its sum of the k_pe gradient over the heads -- inside the timed call ("+ prep"), which is
what a caller who holds the projections' outputs pays.  bf16, 16 heads (TP 8) and 128 heads (TP 1), scale 1/sqrt(192).

Legs: those of tools/bench_mla_prefill.py.  Per leg the median over the rounds and the spread (min .. max) of each route, the ratios
(other route / the MLA call: above 1 the new call wins), the MLA forward alone, and the backward's arithmetic
(2 (3 * 192 + 2 * 128) flops per visible (query, key) pair and head) over the difference of the two MLA times.  Before a leg is timed
the gradients are compared with the dense route's (twice tests/util.py's BWD_TOL: two 16-bit results).

Every leg runs under its own alarm (--leg-timeout seconds, default 300): a leg that hangs ends the process.  A timed window repeats
its call until it holds about 40 ms of device time.  --out FILE also writes the table there (after every leg).  --rounds N
(default 5), --heads 16,128, --legs 0,1,2,3."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import aule  # noqa: E402
from bench_mla_prefill import DN, DQ, DR, DV, LEGS, SCALE, WINDOW_MS, _arg, _cu  # noqa: E402


def leg(name, ns, ls, causal, H, rounds, emit):
    g = torch.Generator(device="cuda").manual_seed(len(ns) + ns[0] + H)
    dt = torch.bfloat16
    B, Tq, Tk = len(ns), sum(ns), sum(ls)
    hq, hk = _cu(ns), _cu(ls)
    cu_q, cu_k = (torch.tensor(c, device="cuda", dtype=torch.int32) for c in (hq, hk))
    q = torch.randn(Tq, H, DQ, device="cuda", dtype=dt, generator=g).requires_grad_(True)
    kvb = torch.randn(Tk, H, DN + DV, device="cuda", dtype=dt, generator=g)     # the kv_b up-projection's output
    down = torch.randn(Tk, 512 + DR, device="cuda", dtype=dt, generator=g)      # the down-projection's: c_kv | k_pe
    dout = torch.randn(Tq, H, DV, device="cuda", dtype=dt, generator=g)
    # leaves that ARE the slices (read in place): what comes back is the gradient of each slice, without autograd's slice-backward
    k_nope, v, k_pe = (x.detach().requires_grad_(True) for x in (kvb[..., :DN], kvb[..., DN:], down[:, 512:]))
    leaves = (q, k_nope, k_pe, v)
    br = causal == "bottom-right"

    def mla_fwd():
        with torch.no_grad():
            return aule.flash_attention_mla_varlen(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q=max(ns), max_seqlen_k=max(ls), causal=causal)

    def mla():
        out = aule.flash_attention_mla_varlen(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q=max(ns), max_seqlen_k=max(ls), causal=causal)
        return torch.autograd.grad(out, leaves, dout)

    def prep_dense(b):
        """[1, H, n, 256] q, K and v of sequence b (differentiable)"""
        qs, ks = slice(hq[b], hq[b + 1]), slice(hk[b], hk[b + 1])
        L = hk[b + 1] - hk[b]
        qb = F.pad(q[qs], (0, 256 - DQ)).permute(1, 0, 2).unsqueeze(0).contiguous()
        kb = F.pad(torch.cat([k_nope[ks], k_pe[ks].unsqueeze(1).expand(L, H, DR)], dim=2), (0, 256 - DQ)).permute(1, 0, 2).unsqueeze(0).contiguous()
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

    def ready(prep):
        return [tuple(t.detach().contiguous().requires_grad_(True) for t in prep(b)) for b in range(B)]

    def bare(run, sets):
        """forward + backward per sequence on prepared leaves: the gradients of the prepared tensors"""
        return [torch.autograd.grad(run(x), x, dout[hq[b]:hq[b + 1]]) for b, x in enumerate(sets)]

    def with_prep(run, prep):
        """... from the projections' outputs and back to them: one backward through the preparation of every sequence"""
        out = torch.cat([run(prep(b)) for b in range(B)])
        return torch.autograd.grad(out, leaves, dout)

    ready_dense, ready_sdpa = ready(prep_dense), ready(prep_sdpa)
    calls = {
        "mla": mla,
        "mla fwd": mla_fwd,
        "dense": lambda: bare(run_dense, ready_dense),
        "dense+prep": lambda: with_prep(run_dense, prep_dense),
        "sdpa": lambda: bare(run_sdpa, ready_sdpa),
        "sdpa+prep": lambda: with_prep(run_sdpa, prep_sdpa),
    }
    got, ref = mla(), with_prep(run_dense, prep_dense)
    torch.cuda.synchronize()
    for what, a, b in zip(("dq", "dk_nope", "dk_pe", "dv"), got, ref):
        a, b = a.float(), b.float()
        bound = 2 * (5e-3 * max(1.0, float(b.abs().max())) + 1e-2 * b.abs())
        if not bool(((a - b).abs() <= bound).all()):
            raise SystemExit(f"{name}, {H} heads: {what} of the MLA call and of the dense route disagree (max |diff| {float((a - b).abs().max()):.3e})")
    del got, ref

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
    bwd_flops = 2.0 * (3 * DQ + 2 * DV) * H * pairs
    bwd_us = med["mla"] - med["mla fwd"]
    ratio = lambda key: f"{med[key] / med['mla']:5.2f}x"   # noqa: E731
    emit(f"  {name:38s} H {H:3d}: MLA fwd + bwd {span['mla']} us (fwd alone {med['mla fwd']:9.1f})   dense 256 per sequence: bare {span['dense']} us "
         f"({ratio('dense')}), + prep {span['dense+prep']} us ({ratio('dense+prep')})   SDPA per sequence: bare {span['sdpa']} us ({ratio('sdpa')}), "
         f"+ prep {span['sdpa+prep']} us ({ratio('sdpa+prep')})   backward {bwd_flops / 1e9:8.1f} GFLOP in {bwd_us:9.1f} us -> "
         f"{bwd_flops / (bwd_us * 1e-6) / 1e12:6.1f} TFLOP/s")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_backward needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 300)
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

    emit(f"# tools/bench_mla_backward.py   (one MI355X; MLA 192 / 128 forward + backward with autograd, bf16, scale 1/sqrt(192); {rounds} alternated "
         f"rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included; (r x): that route's time / the MLA call's; "
         f"backward rate: 2 (3 * 192 + 2 * 128) flops per visible pair and head over (fwd + bwd) - (fwd alone))")
    for H in heads:
        for i in legs:
            name, ns, ls, causal = LEGS[i]
            signal.alarm(budget)
            leg(name, ns, ls, causal, H, rounds, emit)
            signal.alarm(0)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
