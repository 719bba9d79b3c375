#!/usr/bin/env python3
"""Attention sinks: each sink entry against its two comparators on the same tensors in the same process, alternated round by round, warm:
  (a) twin        the sinkless entry (what the sink costs on top of it);
  (b) twin + torch the sinkless entry with return_lse=True followed by the torch epilogue the sink entry replaces,
                  out * sigmoid(lse - sinks) -- the only way to get the result before, forward only (it has no gradient for sinks,
                  and the twin's lse is not differentiable, so the forward + backward legs have no (b)).
gpt-oss-like shapes: bf16, 64 query / 8 KV heads, head_dim 64, with and without the 128-key sliding window of every other layer.

Legs: variable-length causal self-attention 8 x 4096, forward and forward + backward (torch.autograd.grad of q, k, v and, for the sink
entry, sinks); the paged query as a decode step, batch 64 at 8 K keys, one token each; a mixed paged-prefill step (2 prompt chunks of
2048 tokens behind 2 K and 6 K cached keys, 4 verifies of 8 tokens and 58 decodes at 8 K).
Per leg the median over the rounds and the spread (min .. max) of each route and the two ratios, comparator / sink entry: above 1 the
sink entry wins; a ratio below 0.96 -- the sink entry slower than the comparator by more than the spread between boxes -- is set in
**bold**.  Before a leg is timed the sink entry's result is compared with route (b)'s (the forward bound of tests/util.py, two 16-bit
results).

Every leg runs under its own alarm (--leg-timeout seconds, default 180): a leg that hangs ends the process.  A timed window repeats
its call until it holds about 40 ms of device time.  --out FILE also writes the table there.  --rounds N (default 5)."""
import math
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, D = 64, 8, 64
BS = 16
WINDOW_MS = 40
LOSS = 0.96


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _sinks(g):
    """learned-sink-like logits: a spread around the log of a few hundred keys"""
    return (torch.randn(HQ, device="cuda", generator=g) * 2.0 + math.log(300.0)).float()


def _epilogue(out, lse, sinks, head_axis):
    shape = [1] * lse.dim()
    shape[head_axis] = HQ
    return out * torch.sigmoid(lse - sinks.view(shape)).unsqueeze(-1).to(out.dtype)


def _agree(name, a, b, vmax):
    bound = 1e-3 + 2 * 2.0 ** -9 * vmax + 2.0 ** -7 * b.float().abs()
    if not bool(((a.float() - b.float()).abs() <= bound).all()):
        raise SystemExit(f"{name}: the sink entry and the twin + torch epilogue disagree")


def varlen_leg(window, backward):
    g = torch.Generator(device="cuda").manual_seed(7)
    ns = [4096] * 8
    T, S = sum(ns), max(ns)
    cu = torch.tensor([4096 * i for i in range(9)], device="cuda", dtype=torch.int32)
    q, dout = (torch.randn(T, HQ, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    k, v = (torch.randn(T, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    sinks = _sinks(g)
    if backward:
        for x in (q, k, v, sinks):
            x.requires_grad_(True)
    kw = dict(max_seqlen_q=S, max_seqlen_k=S, causal=True, window_size=window)

    def sink():
        out = aule.flash_attention_varlen_sinks(q, k, v, sinks, cu, cu, **kw)
        return torch.autograd.grad(out, (q, k, v, sinks), dout) if backward else out

    def twin():
        out = aule.flash_attention_varlen(q, k, v, cu, cu, **kw)
        return torch.autograd.grad(out, (q, k, v), dout) if backward else out

    def twin_torch():
        out, lse = aule.flash_attention_varlen(q, k, v, cu, cu, return_lse=True, **kw)
        return _epilogue(out, lse, sinks, 1)

    with torch.no_grad():
        _agree("varlen", aule.flash_attention_varlen_sinks(q, k, v, sinks, cu, cu, **kw), twin_torch(), float(v.float().abs().max()))
    calls = {"sink": sink, "twin": twin}
    if not backward:
        calls["twin+torch"] = twin_torch
    return calls


def _cache(g, lens):
    """a paged cache holding `lens` keys per sequence, blocks handed out in order; returns k_cache, v_cache, block_tables"""
    nblk = [(n + BS - 1) // BS for n in lens]
    kc, vc = (torch.randn(sum(nblk), BS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    bt = torch.zeros(len(lens), max(nblk), device="cuda", dtype=torch.int32)
    at = 0
    for b, n in enumerate(nblk):
        bt[b, :n] = torch.arange(at, at + n, device="cuda", dtype=torch.int32)
        at += n
    return kc, vc, bt


def query_leg(window, backward):
    g = torch.Generator(device="cuda").manual_seed(8)
    lens = [8192] * 64
    kc, vc, bt = _cache(g, lens)
    cl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    q = torch.randn(64, HQ, 1, D, device="cuda", dtype=torch.bfloat16, generator=g)
    sinks = _sinks(g)
    kw = dict(window_size=window)

    def sink():
        return aule.flash_attention_paged_query_sinks(q, kc, vc, sinks, bt, cl, **kw)

    def twin():
        return aule.flash_attention_paged_query(q, kc, vc, bt, cl, **kw)

    def twin_torch():
        out, lse = aule.flash_attention_paged_query(q, kc, vc, bt, cl, return_lse=True, **kw)
        return _epilogue(out, lse, sinks, 1)

    _agree("paged query", sink(), twin_torch(), float(vc.float().abs().max()))
    return {"sink": sink, "twin": twin, "twin+torch": twin_torch}


def prefill_leg(window, backward):
    g = torch.Generator(device="cuda").manual_seed(9)
    ns = [2048, 2048] + [8] * 4 + [1] * 58
    lens = [2048 + 2048, 6144 + 2048] + [8192] * 62
    kc, vc, bt = _cache(g, lens)
    cl = torch.tensor(lens, device="cuda", dtype=torch.int32)
    cu_host = [0]
    for n in ns:
        cu_host.append(cu_host[-1] + n)
    cu = torch.tensor(cu_host, device="cuda", dtype=torch.int32)
    q = torch.randn(cu_host[-1], HQ, D, device="cuda", dtype=torch.bfloat16, generator=g)
    sinks = _sinks(g)
    kw = dict(max_seqlen_q=max(ns), window_size=window)

    def sink():
        return aule.flash_attention_paged_prefill_sinks(q, kc, vc, sinks, bt, cl, cu, **kw)

    def twin():
        return aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, **kw)

    def twin_torch():
        out, lse = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, return_lse=True, **kw)
        return _epilogue(out, lse, sinks, 1)

    _agree("paged prefill", sink(), twin_torch(), float(vc.float().abs().max()))
    return {"sink": sink, "twin": twin, "twin+torch": twin_torch}


LEGS = [("varlen 8 x 4096 causal", varlen_leg, (False, True)),
        ("paged query (decode) 64 x 8 K", query_leg, (False,)),
        ("paged prefill 2 x 2048 + 4 x 8 + 58 x 1", prefill_leg, (False,))]


def window_us(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def leg(name, make, window, backward, rounds, lines):
    with torch.set_grad_enabled(backward):
        calls = make(window, backward)
        torch.cuda.synchronize()
        # warm, then size every timed window to about WINDOW_MS of device time (a shorter one measures the clock and the scheduler)
        iters = {}
        for key, f in calls.items():
            window_us(f, 2)
            iters[key] = min(2000, max(3, int(WINDOW_MS * 1e3 / window_us(f, 2)) + 1))
        t = {key: [] for key in calls}
        for _ in range(rounds):
            for key, f in calls.items():
                t[key].append(window_us(f, iters[key]))
    med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
    span = {key: f"{med[key]:9.1f} ({min(x):9.1f} .. {max(x):9.1f})" for key, x in t.items()}

    def ratio(key):
        if key not in med:
            return "      n/a"
        r = med[key] / med["sink"]
        return f"**{r:5.3f}x**" if r < LOSS else f"  {r:5.3f}x  "

    line = (f"  {name:40s} {'window 128' if window > 0 else 'no window '} {'fwd+bwd' if backward else 'fwd    '}: sink entry {span['sink']} us"
            f"   (a) twin {span['twin']} us   (b) twin + torch epilogue {span.get('twin+torch', '      n/a' + ' ' * 26)} us"
            f"   (a) / sink {ratio('twin')}   (b) / sink {ratio('twin+torch')}")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinks needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 180)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_sinks.py   (one MI355X; {HQ} q / {HKV} kv heads, head_dim {D}, bf16; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, "
            f"median (min .. max) us per call, host launch cost included; ratios are comparator / sink entry, bold below {LOSS})")
    print(head, flush=True)
    lines = [head]
    for name, make, modes in LEGS:
        for window in (-1, 128):
            for backward in modes:
                signal.alarm(budget)
                leg(name, make, window, backward, rounds, lines)
                signal.alarm(0)
                torch.cuda.empty_cache()
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
