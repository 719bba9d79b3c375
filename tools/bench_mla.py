#!/usr/bin/env python3
"""Paged MLA: aule.flash_attention_mla_paged (the latent cache read in place, once, for both products) against the only route a
user had before it -- gather the pages of every sequence into a contiguous latent [B, 1, L, 576] and call
torch.nn.functional.scaled_dot_product_attention with K = the gathered latent and V = its first 512 columns (a view: no copy) --
on the same tensors in the same process, alternated round by round, warm.  The heads of a token share the latent, so the SDPA
call folds them into the query axis (q [B, 1, n * heads, 576]: one "head", nothing expanded); with two tokens per sequence the
bottom-right rule is a boolean mask [n * heads, L].  The route is timed twice: with the gather (what a serving step pays) and with
the latent gathered beforehand (SDPA alone).

Shapes: bf16, block 64, shuffled block table; heads 16 (DeepSeek under TP 8) and 128 (TP 1); batch 1 / 8 / 64; context 1 K / 8 K /
32 K; one and two tokens per sequence.  Per leg: the launch plan (row blocks x nsplit x batch workgroups), the median over the
rounds and the spread (min .. max) of the three, the two ratios, the latent bytes of the batch (B L 1152) over the call's time and
its arithmetic (2 (576 + 512) flops per visible (row, key) pair) over its time.  Before a leg is timed the two routes are compared
(the forward bound of tests/util.py).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in this one
process and the first failure stops the run.  A timed window repeats its call until it holds about 40 ms of device time.
--out FILE also writes the table there.  --rounds N (default 5)."""
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

QK, VD, BS = 576, 512, 64
WINDOW_MS = 40
HEADS, BATCH, CONTEXT, TOKENS = (16, 128), (1, 8, 64), (1024, 8192, 32768), (1, 2)


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def plan(B, Hq, n, L):
    d = _capi.MlaPagedDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = _capi.DTYPE_BF16, B, Hq, QK, VD
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q, d.q_token_stride = BS, L // BS, B * n, n, Hq * QK
    d.cu_seqlens_q = 16   # (not read: non-null = ragged)
    out = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(d), out, 6) == 6
    return out[0], out[2]


def leg(Hq, B, L, n, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(Hq + B + L + n)
    dt = torch.bfloat16
    nblk = L // BS
    q = torch.randn(B * n, Hq, QK, device="cuda", dtype=dt, generator=g)
    kv = torch.randn(B * nblk, BS, QK, device="cuda", dtype=dt, generator=g)
    bt = torch.randperm(B * nblk, device="cuda", generator=g).to(torch.int32).view(B, nblk)
    cl = torch.full((B,), L, device="cuda", dtype=torch.int32)
    cu = torch.arange(0, B * n + 1, n, device="cuda", dtype=torch.int32)
    rows = bt.long()
    scale = QK ** -0.5
    mask = None
    if n > 1:
        pos = L - n + torch.arange(n * Hq, device="cuda") // Hq
        mask = (torch.arange(L, device="cuda")[None, :] <= pos[:, None]).view(1, 1, n * Hq, L)

    def paged():
        return aule.flash_attention_mla_paged(q, kv, bt, cl, cu, max_seqlen_q=n)

    def gather():
        return kv[rows].view(B, 1, L, QK)

    def sdpa(lat):
        return F.scaled_dot_product_attention(q.view(B, 1, n * Hq, QK), lat, lat[..., :VD], attn_mask=mask, scale=scale).view(B * n, Hq, VD)

    held = gather()
    a, b_ = paged(), sdpa(held)
    torch.cuda.synchronize()
    bound = 1e-3 + 2.0 ** -9 * float(kv[..., :VD].float().abs().max()) + 2.0 ** -8 * b_.float().abs()
    if not bool(((a.float() - b_.float()).abs() <= 2 * bound).all()):   # (both sides are 16-bit results)
        raise SystemExit(f"heads {Hq} batch {B} context {L} tokens {n}: the paged MLA and the gather route disagree")
    pairs = B * Hq * sum(L - n + i + 1 for i in range(n))
    flops, nbytes = 2.0 * (QK + VD) * pairs, B * L * QK * 2
    calls = {"mla": paged, "gather+sdpa": lambda: sdpa(gather()), "sdpa": lambda: sdpa(held)}

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
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(window(f, iters[key]))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    span = {k: f"{med[k]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})" for k, v in t.items()}
    rb, ns = plan(B, Hq, n, L)
    line = (f"  heads {Hq:3d} batch {B:2d} context {L:5d} tokens {n}: plan {rb} x {ns:2d} x {B:2d}   paged MLA {span['mla']} us   gather + SDPA {span['gather+sdpa']} us"
            f"   SDPA, latent gathered beforehand {span['sdpa']} us   with gather / MLA {med['gather+sdpa'] / med['mla']:6.2f}x   without gather / MLA "
            f"{med['sdpa'] / med['mla']:6.2f}x   {nbytes / (med['mla'] * 1e-6) / 1e12:5.2f} TB/s of latent   {flops / (med['mla'] * 1e-6) / 1e12:6.1f} TFLOP/s")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_mla.py   (one MI355X; latent 576 / 512, block_size {BS}, bf16, shuffled block table; plan = row blocks x nsplit x batch "
            f"workgroups; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for Hq in HEADS:
        for n in TOKENS:
            for B in BATCH:
                for L in CONTEXT:
                    signal.alarm(budget)
                    leg(Hq, B, L, n, rounds, lines)
                    signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
