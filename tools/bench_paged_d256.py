#!/usr/bin/env python3
"""Paged attention at head_dim 256: aule.flash_attention_paged_d256 (the pages read in place, every sequence's keys split over the
device) against the routes a user had before it, on the same tensors in the same process, alternated round by round, warm:

  * gather + dense: per sequence, gather its pages into contiguous K / V [1, Hkv, L, 256] (an FP8 cache is dequantised on the way)
    and call aule.flash_attention(..., causal="bottom-right") at D = 256 -- timed with the gather (what a serving step pays) and
    with K / V gathered beforehand (the dense kernel alone);
  * gather + SDPA: the whole batch gathered into [B, Hkv, L, 256] and torch.nn.functional.scaled_dot_product_attention with
    enable_gqa (a boolean mask where there is more than one token per sequence or a window).

Legs: Gemma-3-12B-like (16 q / 8 kv heads) and Qwen3-Next-like (16 / 2) heads; batch 1 / 8 / 64 at 1 K / 8 K / 32 K; one token and 5
tokens per sequence; a 16-bit and an FP8 cache; with and without a 1024-key window; one 2048-token chunk behind 8 K; and on two
decode legs the plan's nsplit against forced 1 / half / double (aule_hip_debug_paged_d256_launch_nsplit).  bf16, block 16, shuffled
block table.  Per leg: the plan (row blocks x nsplit x KV heads x batch workgroups), the median over the rounds and the spread
(min .. max) of every route, the ratios over the paged call (below 1: the paged call LOSES), and the cache bytes a call must read
over its time.  Before a leg is timed the paged call is compared with the dense route (the forward bound of tests/util.py, both
sides 16-bit).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in this one
process and the first failure stops the run.  A timed window repeats its call until it holds about 20 ms of device time.
--out FILE also writes the table there.  --rounds N (default 3).  --heads 8 / --heads 2 runs one head configuration only."""
import ctypes
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import aule  # noqa: E402
from aule import _capi  # noqa: E402
from aule._torch import paged_d256  # noqa: E402

D, BS, HQ = 256, 16, 16
WINDOW_MS = 20
KV_HEADS, BATCH, CONTEXT, TOKENS, WINDOWS = (8, 2), (1, 8, 64), (1024, 8192, 32768), (1, 5), (-1, 1024)


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def plan(B, Hkv, n, L, window):
    d = _capi.PagedD256Desc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = _capi.DTYPE_BF16, B, HQ, Hkv, D
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q, d.q_token_stride, d.window_size = BS, L // BS, B * n, n, HQ * D, window
    d.cu_seqlens_q = 16   # (not read: non-null = ragged)
    out = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_paged_d256_plan(ctypes.byref(d), out, 6) == 6
    return out[0], out[2]


def _window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def _alternated(calls, rounds):
    """{name: (median, "median (min .. max)")} of `calls`, warm, alternated round by round, every window about WINDOW_MS long"""
    iters = {}
    for key, f in calls.items():
        _window(f, 2)
        iters[key] = min(400, max(3, int(WINDOW_MS * 1e3 / _window(f, 2)) + 1))
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(_window(f, iters[key]))
    return {k: (sorted(v)[len(v) // 2], f"{sorted(v)[len(v) // 2]:8.1f} ({min(v):8.1f} .. {max(v):8.1f})") for k, v in t.items()}


class Pool:
    """The caches of one (KV heads, batch, context): both kinds, one shuffled table"""

    def __init__(self, Hkv, B, L):
        g = torch.Generator(device="cuda").manual_seed(Hkv + B + L)
        nblk = L // BS
        self.Hkv, self.B, self.L = Hkv, B, L
        self.k, self.v = (torch.randn(B * nblk, BS, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
        self.bt = torch.randperm(B * nblk, device="cuda", generator=g).to(torch.int32).view(B, nblk)
        self.rows = self.bt.long()
        self.k8, self.v8 = self.k.to(torch.float8_e4m3fn), self.v.to(torch.float8_e4m3fn)
        self.ks, self.vs = (torch.rand(Hkv, device="cuda", generator=g) + 0.5 for _ in range(2))
        self.cl = torch.full((B,), L, device="cuda", dtype=torch.int32)

    def gathered(self, fp8, b=None):
        """K, V [B or 1, Hkv, L, 256] bf16 of the batch or of sequence b: the pages gathered, FP8 codes dequantised"""
        rows = self.rows if b is None else self.rows[b:b + 1]
        res = []
        for x, s in ((self.k8, self.ks), (self.v8, self.vs)) if fp8 else ((self.k, None), (self.v, None)):
            y = x[rows].view(rows.shape[0], self.L, self.Hkv, D)
            if fp8:
                y = (y.float() * s[None, None, :, None]).to(torch.bfloat16)
            res.append(y.permute(0, 2, 1, 3))
        return res


def leg(pool, n, fp8, window, rounds, lines, vary_nsplit=False):
    Hkv, B, L = pool.Hkv, pool.B, pool.L
    g = torch.Generator(device="cuda").manual_seed(n + 2 * fp8 + window)
    q = torch.randn(B * n, HQ, D, device="cuda", dtype=torch.bfloat16, generator=g)
    cu = torch.arange(0, B * n + 1, n, device="cuda", dtype=torch.int32)
    kc, vc, ks, vs = (pool.k8, pool.v8, pool.ks, pool.vs) if fp8 else (pool.k, pool.v, None, None)
    mask = None
    if n > 1 or window > 0:
        pos = L - n + torch.arange(n, device="cuda")
        j = torch.arange(L, device="cuda")
        mask = j[None, :] <= pos[:, None]
        if window > 0:
            mask &= pos[:, None] - j[None, :] < window

    def paged(nsplit=None):
        return paged_d256(q, kc, vc, pool.bt, pool.cl, cu, n, window_size=window, k_scale=ks, v_scale=vs, force_nsplit=nsplit)

    def dense(kv=None):
        out = []
        for b in range(B):
            k, v = pool.gathered(fp8, b) if kv is None else (kv[0][b:b + 1], kv[1][b:b + 1])
            out.append(aule.flash_attention(q[b * n:(b + 1) * n].permute(1, 0, 2)[None], k, v, causal="bottom-right", window_size=window)[0].permute(1, 0, 2))
        return torch.cat(out)

    def sdpa():
        k, v = pool.gathered(fp8)
        return F.scaled_dot_product_attention(q.view(B, n, HQ, D).permute(0, 2, 1, 3), k, v, attn_mask=mask, enable_gqa=True).permute(0, 2, 1, 3).reshape(B * n, HQ, D)

    held = [x.contiguous() for x in pool.gathered(fp8)]
    a, b_ = paged(), dense(held)
    torch.cuda.synchronize()
    vmax = float(held[1].float().abs().max())
    bound = 2 * (1e-3 + 2.0 ** -9 * vmax + 2.0 ** -8 * b_.float().abs())   # (both sides are 16-bit results)
    name = f"heads {HQ}/{Hkv} batch {B:2d} context {L:5d} tokens {n:4d} {'fp8 ' if fp8 else '16b '} window {window if window > 0 else 'none':>4}"
    if not bool(((a.float() - b_.float()).abs() <= bound).all()):
        raise SystemExit(f"{name}: the paged call and the gather + dense route disagree")
    rb, ns = plan(B, Hkv, n, L, window)
    nbytes = 2 * B * Hkv * D * (min(L, window + n) if window > 0 else L) * (1 if fp8 else 2)
    if vary_nsplit:
        forced = sorted({1, max(ns // 2, 1), ns, min(2 * ns, 64)})
        res = _alternated({k: (lambda k=k: paged(k)) for k in forced}, rounds)
        line = f"  {name}: plan {rb} x {ns:2d} x {Hkv} x {B:2d}   " + "   ".join(f"nsplit {k:2d}{'*' if k == ns else ' '} {res[k][1]} us" for k in forced)
    else:
        res = _alternated({"paged": paged, "gather+dense": dense, "dense": lambda: dense(held), "gather+sdpa": sdpa}, rounds)
        med = {k: v[0] for k, v in res.items()}
        line = (f"  {name}: plan {rb} x {ns:2d} x {Hkv} x {B:2d}   paged {res['paged'][1]} us   gather + dense {res['gather+dense'][1]} us   dense, gathered beforehand "
                f"{res['dense'][1]} us   gather + SDPA {res['gather+sdpa'][1]} us   gather + dense / paged {med['gather+dense'] / med['paged']:6.2f}x   dense / paged "
                f"{med['dense'] / med['paged']:6.2f}x   gather + SDPA / paged {med['gather+sdpa'] / med['paged']:6.2f}x   {nbytes / (med['paged'] * 1e-6) / 1e12:5.2f} TB/s of cache")
    _emit(line, lines)


def _emit(line, out):
    """to the terminal and, line by line, to --out FILE (a leg that ends the process leaves the legs before it on record)"""
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_d256 needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 3), _arg("--leg-timeout", 120)
    only = _arg("--heads", 0)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_paged_d256.py   (one MI355X; head_dim {D}, block_size {BS}, bf16 queries, shuffled block table; plan = row blocks x nsplit x KV heads x "
            f"batch workgroups; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call through the Python layer)")
    lines = None
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        lines = open(path, "w")
    _emit(head, lines)
    for Hkv in KV_HEADS:
        if only and Hkv != only:
            continue
        for B in BATCH:
            for L in CONTEXT:
                pool = Pool(Hkv, B, L)
                for fp8 in (False, True):
                    for n in TOKENS:
                        for window in WINDOWS:
                            signal.alarm(budget)
                            leg(pool, n, fp8, window, rounds, lines)
                            signal.alarm(0)
                    if L == 8192 and B == 1:      # one prompt chunk behind 8 K
                        signal.alarm(budget)
                        leg(pool, 2048, fp8, -1, rounds, lines)
                        signal.alarm(0)
                if L >= 8192 and B == 8:          # the plan's nsplit against forced 1 / half / double, two decode legs
                    signal.alarm(budget)
                    leg(pool, 1, False, -1, rounds, lines, vary_nsplit=True)
                    signal.alarm(0)
                del pool
                torch.cuda.empty_cache()
    if lines is not None:
        lines.close()


if __name__ == "__main__":
    main()
