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

--fp8: the same 36 shapes with the 16-bit call NEXT TO aule.flash_attention_mla_paged_fp8 on the cache quantised with
aule.quantize_mla_cache_fp8 (the scale a device tensor), the two alternated round by round; the 16-bit kernel is the baseline of the
same build.  Before a leg is timed the FP8 call with kv_scale = 1 is compared bit for bit with the 16-bit call on the converted codes.
Per leg: both medians and spreads, 16-bit / FP8 (below 1: FP8 is slower) and the code bytes of the batch (B L 576) over the FP8 time.

--append: aule.mla_kv_append against the torch ops it replaces -- cos[pos] / sin[pos] and rope_raw for a rotated k_pe, cat, divide /
clamp / cast for an FP8 cache, index_copy_ -- T = 1 / 64 / 4096 / 65536 tokens, a 16-bit and an FP8 cache, with and without the
(interleaved) rotation, bf16, block 64, random slots and positions.  The two are compared bit for bit before they are timed.  Per
leg: medians and spreads, composed / fused, and from T = 4096 on the algorithmic bytes (T 576 (2 + cache element size)) over the time.

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

    res = _alternated(calls, rounds)
    med, span = {k: v[0] for k, v in res.items()}, {k: v[1] for k, v in res.items()}
    rb, ns = plan(B, Hq, n, L)
    line = (f"  heads {Hq:3d} batch {B:2d} context {L:5d} tokens {n}: plan {rb} x {ns:2d} x {B:2d}   paged MLA {span['mla']} us   gather + SDPA {span['gather+sdpa']} us"
            f"   SDPA, latent gathered beforehand {span['sdpa']} us   with gather / MLA {med['gather+sdpa'] / med['mla']:6.2f}x   without gather / MLA "
            f"{med['sdpa'] / med['mla']:6.2f}x   {nbytes / (med['mla'] * 1e-6) / 1e12:5.2f} TB/s of latent   {flops / (med['mla'] * 1e-6) / 1e12:6.1f} TFLOP/s")
    print(line, flush=True)
    lines.append(line)


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


def leg_fp8(Hq, B, L, n, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(Hq + B + L + n)
    dt = torch.bfloat16
    nblk = L // BS
    q = torch.randn(B * n, Hq, QK, device="cuda", dtype=dt, generator=g)
    kv = torch.randn(B * nblk, BS, QK, device="cuda", dtype=dt, generator=g)
    bt = torch.randperm(B * nblk, device="cuda", generator=g).to(torch.int32).view(B, nblk)
    cl = torch.full((B,), L, device="cuda", dtype=torch.int32)
    cu = torch.arange(0, B * n + 1, n, device="cuda", dtype=torch.int32)
    codes, ks = aule.quantize_mla_cache_fp8(kv)
    exact = codes.to(dt)
    a = aule.flash_attention_mla_paged_fp8(q, codes, bt, cl, cu, max_seqlen_q=n, scale=float(ks) * QK ** -0.5, return_lse=True)
    b_ = aule.flash_attention_mla_paged(q, exact, bt, cl, cu, max_seqlen_q=n, scale=float(ks) * QK ** -0.5, return_lse=True)
    torch.cuda.synchronize()
    if not (torch.equal(a[0].view(torch.int16), b_[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b_[1].view(torch.int32))):
        raise SystemExit(f"heads {Hq} batch {B} context {L} tokens {n}: the FP8 call and the 16-bit call on the converted codes differ")
    del exact, a, b_
    r = _alternated({"16": lambda: aule.flash_attention_mla_paged(q, kv, bt, cl, cu, max_seqlen_q=n),
                     "fp8": lambda: aule.flash_attention_mla_paged_fp8(q, codes, bt, cl, cu, max_seqlen_q=n, kv_scale=ks)}, rounds)
    rb, ns = plan(B, Hq, n, L)
    line = (f"  heads {Hq:3d} batch {B:2d} context {L:5d} tokens {n}: plan {rb} x {ns:2d} x {B:2d}   16-bit cache {r['16'][1]} us   FP8 cache {r['fp8'][1]} us"
            f"   16-bit / FP8 {r['16'][0] / r['fp8'][0]:5.2f}x   {B * L * QK / (r['fp8'][0] * 1e-6) / 1e12:5.2f} TB/s of codes")
    print(line, flush=True)
    lines.append(line)


def leg_append(T, fp8, rope, rounds, lines):
    from aule._torch import rope_raw
    g = torch.Generator(device="cuda").manual_seed(T + 2 * fp8 + rope)
    dt = torch.bfloat16
    nslots = (max(T, 1024) + BS - 1) // BS * BS * 2
    c = torch.randn(T, VD, device="cuda", dtype=dt, generator=g)
    r = torch.randn(T, QK - VD, device="cuda", dtype=dt, generator=g)
    slots = torch.randperm(nslots, device="cuda", generator=g)[:T]
    table_len = 8192
    ang = torch.rand(table_len, 32, device="cuda", generator=g) * 6.2831853
    cos, sin = torch.cos(ang), torch.sin(ang)
    pos = torch.randint(0, table_len, (T,), device="cuda", generator=g)
    ks = torch.tensor([6.0 / 448], device="cuda")
    cache = [torch.zeros(nslots // BS, BS, QK, device="cuda", dtype=torch.float8_e4m3fn if fp8 else dt) for _ in range(2)]
    kw = dict(kv_scale=ks) if fp8 else {}
    if rope:
        kw.update(cos=cos, sin=sin, positions=pos, rope_layout="interleaved")

    def fused():
        aule.mla_kv_append(c, r, cache[0], slots, **kw)

    def composed():
        rr = rope_raw(r.view(1, 1, T, QK - VD), cos[pos], sin[pos], layout="interleaved").view(T, QK - VD) if rope else r
        rows = torch.cat([c, rr], 1)
        if fp8:
            cache[1].view(torch.uint8).view(-1, QK).index_copy_(0, slots, (rows.float() / ks).clamp_(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))
        else:
            cache[1].view(-1, QK).index_copy_(0, slots, rows)

    fused(); composed()
    torch.cuda.synchronize()
    if not torch.equal(cache[0].view(torch.uint8), cache[1].view(torch.uint8)):
        raise SystemExit(f"T {T} fp8 {fp8} rope {rope}: the fused append and the composed one differ")
    t = _alternated({"fused": fused, "composed": composed}, rounds)
    line = (f"  T {T:6d} {'fp8' if fp8 else '16b'}  {'rope ' if rope else 'plain'}: fused {t['fused'][1]} us   composed {t['composed'][1]} us"
            f"   composed / fused {t['composed'][0] / t['fused'][0]:6.2f}x")
    if T >= 4096:
        nbytes = T * QK * (2 + (1 if fp8 else 2))
        line += f"   fused {nbytes / 1e6:6.1f} MB -> {nbytes / (t['fused'][0] * 1e-6) / 1e12:5.2f} TB/s"
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    if "--append" in sys.argv:
        head = (f"# tools/bench_mla.py --append   (one MI355X; latent rows 512 + 64, block_size {BS}, bf16 c_kv / k_pe, random slots and positions, interleaved "
                f"rotation; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
        print(head, flush=True)
        lines = [head]
        for T in (1, 64, 4096, 65536):
            for fp8 in (False, True):
                for rope in (False, True):
                    signal.alarm(budget)
                    leg_append(T, fp8, rope, rounds, lines)
                    signal.alarm(0)
        return _write(lines)
    head = (f"# tools/bench_mla.py{' --fp8' if '--fp8' in sys.argv else ''}   (one MI355X; latent 576 / 512, block_size {BS}, bf16, shuffled block table; plan = row blocks x nsplit x batch "
            f"workgroups; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for Hq in HEADS:
        for n in TOKENS:
            for B in BATCH:
                for L in CONTEXT:
                    signal.alarm(budget)
                    (leg_fp8 if "--fp8" in sys.argv else leg)(Hq, B, L, n, rounds, lines)
                    signal.alarm(0)
    _write(lines)


def _write(lines):
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
