#!/usr/bin/env python3
"""The MLA indexer: aule.mla_indexer_logits / aule.mla_indexer_topk / aule.mla_indexer against the torch route a caller had before
them, on the same tensors in the same process, alternated round by round, warm.

The torch route, as a serving loop would write it with no kernel of ours:
  logits  gather the sequence's key rows through the block table (an FP8 cache: gather codes and scales, dequantise to bf16), then
          per chunk of keys (so that nothing wider than [T, 64, chunk] exists) einsum -> relu -> times the weights -> sum over heads,
          and a causal mask (key j visible iff j <= p);
  top-k   torch.topk on the masked logits, a sort of the chosen positions, and the slot gather through the block table.
Before a leg is timed, our logits are compared with the torch route's (relative Frobenius error, both made from bf16 products), and
our lists with torch.topk + sort applied to OUR logits (equal as sets per token: random logits carry no ties).

Legs: bf16 and FP8 key caches, 64 index heads of width 128, block 64, topk 2048, shuffled block tables.  Decode: T = 1 / 8 / 64
sequences of one token at context 8 K / 32 K / 128 K.  Prefill: one 2048-token chunk at context 32 K (cu_seqlens_q, max_seqlen_q 2048).

Per leg: the logits launch plan (sequences x token groups x key chunks workgroups, keys per chunk), median (min .. max) us per call
through the Python layer for logits, top-k and both, ours and torch's, the three ratios (above 1: ours is faster; below 1 the leg is
marked LOSES), the achieved TFLOP/s of our logits (2 * visible (token, key) pairs * 64 * 128 flop) and the GB/s of visible logits our
top-k reads once (4 bytes each; it reads them up to five times).  Every leg runs under its own alarm (--leg-timeout seconds, default
120): a leg that hangs ends the process; the first failure stops the run.  --out FILE also writes the table there.  --rounds N
(default 5)."""
import ctypes
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402
from aule import _capi  # noqa: E402

H, D, BS, TOPK = 64, 128, 64, 2048
WINDOW_MS = 40
TOKENS, CONTEXT = (1, 8, 64), (8192, 32768, 131072)
PREFILL_CHUNK, PREFILL_CONTEXT = 2048, 32768
KEY_CHUNK = 4096   # keys per einsum of the torch route: [T, 64, 4096] fp32 at most 4 GB / 2048 tokens


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def plan(B, T, max_sq, mb):
    d = _capi.MlaIndexerLogitsDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.heads, d.head_dim, d.batch, d.num_blocks, d.block_size, d.max_blocks = _capi.DTYPE_BF16, H, D, B, 1, BS, mb
    d.total_tokens, d.max_seqlen_q, d.q_token_stride, d.logits_stride = T, max_sq, H * D, mb * BS
    d.cu_seqlens_q = 4096 if max_sq > 1 else None
    out = (ctypes.c_int32 * 5)()
    assert _capi.load().aule_hip_debug_mla_indexer_plan(ctypes.byref(d), out, 5) == 5
    return list(out)


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
    return {k: (sorted(v)[len(v) // 2], f"{sorted(v)[len(v) // 2]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})") for k, v in t.items()}


def leg(what, B, n, L, fp8, rounds, lines):
    """B sequences of n new tokens each at context L"""
    g = torch.Generator(device="cuda").manual_seed(B + n + L + fp8)
    dt = torch.bfloat16
    T, nblk = B * n, L // BS
    q = torch.randn(T, H, D, device="cuda", dtype=dt, generator=g)
    w = torch.randn(T, H, device="cuda", generator=g) * H ** -0.5
    kc = torch.randn(B * nblk, BS, D, device="cuda", dtype=dt, generator=g)
    bt = torch.randperm(B * nblk, device="cuda", generator=g).to(torch.int32).view(B, nblk)
    cl = torch.full((B,), L, device="cuda", dtype=torch.int32)
    cu = (torch.arange(B + 1, device="cuda", dtype=torch.int32) * n) if n > 1 else None
    ragged = dict(cu_seqlens_q=cu, max_seqlen_q=n) if n > 1 else {}
    cache, ks = (aule.quantize_indexer_cache_fp8(kc) if fp8 else (kc, None))
    del kc
    kw = dict(k_scale=ks) if fp8 else {}
    pos = (L - n + torch.arange(n, device="cuda")).repeat(B)          # p of every token
    cols = torch.arange(L, device="cuda")
    bt_long = bt.long()

    def ours_logits():
        return aule.mla_indexer_logits(q, w, cache, bt, cl, **ragged, **kw)

    def torch_logits():
        if fp8:
            keys = (cache[bt_long].to(dt) * ks[bt_long].to(dt)[..., None]).view(B, L, D)
        else:
            keys = cache[bt_long].view(B, L, D)
        out = torch.empty((B, n, L), device="cuda", dtype=torch.float32)
        qb, wb = q.view(B, n, H, D), w.view(B, n, H, 1)
        for k0 in range(0, L, KEY_CHUNK):
            s = torch.einsum("bnhd,bld->bnhl", qb, keys[:, k0:k0 + KEY_CHUNK])
            out[:, :, k0:k0 + KEY_CHUNK] = (torch.relu(s).float() * wb).sum(dim=2)
        return out.view(T, L).masked_fill_(cols[None, :] > pos[:, None], float("-inf"))

    mine = ours_logits()

    def ours_topk():
        return aule.mla_indexer_topk(mine, TOPK, bt, cl, BS, **ragged)

    def torch_topk():
        chosen = torch.topk(mine, TOPK, dim=-1).indices.sort(dim=-1).values
        blocks = torch.gather(bt_long.repeat_interleave(n, dim=0), 1, chosen // BS)
        return (blocks * BS + chosen % BS).to(torch.int32)

    def ours_both():
        return aule.mla_indexer(q, w, cache, bt, cl, TOPK, **ragged, **kw)

    def torch_both():
        lg = torch_logits()
        chosen = torch.topk(lg, TOPK, dim=-1).indices.sort(dim=-1).values
        blocks = torch.gather(bt_long.repeat_interleave(n, dim=0), 1, chosen // BS)
        return (blocks * BS + chosen % BS).to(torch.int32)

    theirs = torch_logits()
    torch.cuda.synchronize()
    fin = torch.isfinite(theirs)
    if not torch.equal(fin, torch.isfinite(mine)):
        raise SystemExit(f"{what}: the -inf marks of our logits and the torch route's differ")
    rel = float((mine[fin] - theirs[fin]).norm() / theirs[fin].norm())
    if not rel < 2e-2:
        raise SystemExit(f"{what}: our logits and the torch route's disagree (relative error {rel:.3g})")
    if not torch.equal(ours_topk(), torch_topk()):
        raise SystemExit(f"{what}: our lists and torch.topk + sort on the same logits disagree")
    del theirs, fin
    res = _alternated({"logits": ours_logits, "t.logits": torch_logits, "topk": ours_topk, "t.topk": torch_topk, "both": ours_both,
                       "t.both": torch_both}, rounds)
    med, span = {k: v[0] for k, v in res.items()}, {k: v[1] for k, v in res.items()}
    visible = int((pos + 1).sum())
    gt, groups, ck, chunks, grid = plan(B, T, n, nblk)
    ratios = [med["t." + k] / med[k] for k in ("logits", "topk", "both")]
    line = (f"  {what} {'fp8 ' if fp8 else 'bf16'}: plan {B:2d} x {groups:3d} x {chunks:4d} ({ck:6d} keys)   logits {span['logits']} us, torch "
            f"{span['t.logits']} us, {ratios[0]:7.2f}x   top-k {span['topk']} us, torch {span['t.topk']} us, {ratios[1]:6.2f}x   both {span['both']} us, torch "
            f"{span['t.both']} us, {ratios[2]:7.2f}x   {2.0 * visible * H * D / (med['logits'] * 1e-6) / 1e12:7.2f} TFLOP/s   "
            f"{visible * 4 / (med['topk'] * 1e-6) / 1e9:7.1f} GB/s of logits   (logits rel. err {rel:.1e})"
            + "".join(f"   LOSES on {k}" for k, r in zip(("logits", "top-k", "both"), ratios) if r < 1.0))
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_indexer needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_mla_indexer.py   (one MI355X; {H} index heads x {D}, block {BS}, topk {TOPK}, bf16 queries; plan = sequences x token groups x "
            f"key chunks workgroups; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included; "
            f"ratio = torch / ours)")
    print(head, flush=True)
    lines = [head]
    for fp8 in (False, True):
        for T in TOKENS:
            for L in CONTEXT:
                signal.alarm(budget)
                leg(f"decode  T {T:4d} context {L:6d}", T, 1, L, fp8, rounds, lines)
                signal.alarm(0)
                torch.cuda.empty_cache()
        signal.alarm(budget)
        leg(f"prefill T {PREFILL_CHUNK:4d} context {PREFILL_CONTEXT:6d}", 1, PREFILL_CHUNK, PREFILL_CONTEXT, fp8, rounds, lines)
        signal.alarm(0)
        torch.cuda.empty_cache()
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
