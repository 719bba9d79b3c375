#!/usr/bin/env python3
"""Sparse MLA: aule.flash_attention_mla_sparse (every token reads the topk latent rows its list names, in place) against the two
routes a user had before it, on the same tensors in the same process, alternated round by round, warm:
  (a) aule.flash_attention_mla_paged (or _fp8) over the FULL context -- other arithmetic (every key instead of the listed ones), the
      bytes of the whole context;
  (b) a torch gather of the listed rows into [T, topk, 576] (an FP8 cache: the codes gathered, then dequantised) and
      torch.nn.functional.scaled_dot_product_attention with the heads of a token folded into the query axis.
Before a leg is timed the sparse call is compared with route (b) (the forward bound of tests/util.py, both sides 16-bit results).

Decode legs: bf16 and FP8 caches, topk 2048, heads 16 and 128, T = 1 / 8 / 64 sequences with one token each at context 8 K / 32 K /
128 K, block 64, shuffled block tables; the list of a token is a random draw of its own sequence's positions, turned into slots with
aule.paged_slot_mapping.  Prefill legs: a 2048-token chunk at the end of one contiguous [32768, 576] latent (the cache [L, 1, 576]),
token i listing 2048 random positions up to its own; route (a) is the causal paged call over the same latent read as blocks of 64.

Per leg: the launch plan (tokens x row blocks x nsplit workgroups), median (min .. max) us per call through the Python layer for the
three routes, the two ratios (above 1: the sparse call is faster) and the bytes of gathered latent rows (T topk 576 x element size)
over the sparse call's time.  Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the
process; the first failure stops the run.  --out FILE also writes the table there.  --rounds N (default 5).

Cap legs (T = 1, context 32 K, after the table): what the plan's "at most one split per two 64-entry tiles" costs where it binds.  The
same call through aule_hip_debug_mla_sparse_launch_nsplit (the C entry with the split count forced; descriptor and workspace made once,
so these figures hold no torch-layer cost and are lower than the table's) at nsplit 4 / 8 / 16 / 32: 16 is the plan's and 32 is one
tile per workgroup -- what the cap forbids (there are 32 tiles: more ranges would be empty).  Each result is first compared with the
entry's (bit for bit at the plan's nsplit, the forward bound elsewhere)."""
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

QK, VD, BS, TOPK = 576, 512, 64, 2048
WINDOW_MS = 40
HEADS, TOKENS, CONTEXT = (16, 128), (1, 8, 64), (8192, 32768, 131072)
PREFILL_CHUNK, PREFILL_LATENT = 2048, 32768


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def plan(T, Hq, topk):
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.heads_q, d.num_blocks, d.block_size, d.total_tokens, d.topk, d.q_token_stride = _capi.DTYPE_BF16, Hq, 1, 1, T, topk, Hq * QK
    out = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 6) == 6
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
    return {k: (sorted(v)[len(v) // 2], f"{sorted(v)[len(v) // 2]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})") for k, v in t.items()}


def _routes(q, kv, idx, fp8, dense):
    """the three calls on one problem; kv the 16-bit cache [nb, bs, 576], idx [T, topk] int32 valid slots, dense(cache, scale kw) route (a)"""
    T, Hq, _ = q.shape
    topk = idx.shape[1]
    scale = QK ** -0.5
    rows = idx.long()
    if fp8:
        cache, ks = aule.quantize_mla_cache_fp8(kv)
        kw = dict(kv_scale=ks)
        flat = cache.view(-1, QK)

        def gathered():
            return flat[rows].to(q.dtype) * ks.to(q.dtype)
    else:
        cache, kw = kv, {}
        flat = cache.view(-1, QK)

        def gathered():
            return flat[rows]

    def sparse():
        return aule.flash_attention_mla_sparse(q, cache, idx, **kw)

    def gather_sdpa():
        lat = gathered().view(T, 1, topk, QK)
        return F.scaled_dot_product_attention(q.view(T, 1, Hq, QK), lat, lat[..., :VD], scale=scale).view(T, Hq, VD)

    a, b_ = sparse(), gather_sdpa()
    torch.cuda.synchronize()
    vmax = float((flat[rows[0]].float() * (float(ks) if fp8 else 1.0))[..., :VD].abs().max())
    bound = 1e-3 + 2.0 ** -9 * vmax + 2.0 ** -8 * b_.float().abs()
    if not bool(((a.float() - b_.float()).abs() <= 2 * bound).all()):   # (both sides are 16-bit results)
        raise SystemExit("the sparse MLA and the gather route disagree")
    del a, b_
    return {"sparse": sparse, "dense": lambda: dense(cache, kw), "gather+sdpa": gather_sdpa}


def _report(what, T, Hq, fp8, res, lines):
    med, span = {k: v[0] for k, v in res.items()}, {k: v[1] for k, v in res.items()}
    rb, ns = plan(T, Hq, TOPK)
    nbytes = T * TOPK * QK * (1 if fp8 else 2)
    line = (f"  {what} {'fp8 ' if fp8 else 'bf16'} heads {Hq:3d}: plan {T:4d} x {rb} x {ns:2d}   sparse {span['sparse']} us   (a) dense, full context "
            f"{span['dense']} us   (b) gather + SDPA {span['gather+sdpa']} us   (a) / sparse {med['dense'] / med['sparse']:6.2f}x   (b) / sparse "
            f"{med['gather+sdpa'] / med['sparse']:6.2f}x   {nbytes / (med['sparse'] * 1e-6) / 1e12:5.2f} TB/s of listed rows")
    print(line, flush=True)
    lines.append(line)


def leg_decode(Hq, T, L, fp8, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(Hq + T + L + fp8)
    dt = torch.bfloat16
    nblk = L // BS
    q = torch.randn(T, Hq, QK, device="cuda", dtype=dt, generator=g)
    kv = torch.randn(T * nblk, BS, QK, device="cuda", dtype=dt, generator=g)
    bt = torch.randperm(T * nblk, device="cuda", generator=g).to(torch.int32).view(T, nblk)
    cl = torch.full((T,), L, device="cuda", dtype=torch.int32)
    pos = torch.stack([torch.randperm(L, device="cuda", generator=g)[:TOPK] for _ in range(T)])
    seq = torch.arange(T, device="cuda").repeat_interleave(TOPK)
    idx = aule.paged_slot_mapping(bt, pos.reshape(-1), BS, seq_ids=seq).to(torch.int32).view(T, TOPK).contiguous()

    def dense(cache, kw):
        return (aule.flash_attention_mla_paged_fp8 if fp8 else aule.flash_attention_mla_paged)(q, cache, bt, cl, **kw)

    res = _alternated(_routes(q, kv, idx, fp8, dense), rounds)
    _report(f"decode  T {T:2d} context {L:6d}", T, Hq, fp8, res, lines)


def leg_prefill(Hq, fp8, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(Hq + fp8)
    dt = torch.bfloat16
    T, L = PREFILL_CHUNK, PREFILL_LATENT
    q = torch.randn(T, Hq, QK, device="cuda", dtype=dt, generator=g)
    latent = torch.randn(L, QK, device="cuda", dtype=dt, generator=g)
    own = torch.arange(L - T, L, device="cuda")                      # token i sits at position L - T + i
    idx = (torch.rand(T, TOPK, device="cuda", generator=g) * (own[:, None] + 1)).long().clamp_(max=L - 1).to(torch.int32).contiguous()
    bt = torch.arange(L // BS, device="cuda", dtype=torch.int32).view(1, -1)
    cl = torch.tensor([L], device="cuda", dtype=torch.int32)
    cu = torch.tensor([0, T], device="cuda", dtype=torch.int32)

    def dense(cache, kw):
        return (aule.flash_attention_mla_paged_fp8 if fp8 else aule.flash_attention_mla_paged)(q, cache.view(L // BS, BS, QK), bt, cl, cu, max_seqlen_q=T, **kw)

    res = _alternated(_routes(q, latent.view(L, 1, QK), idx, fp8, dense), rounds)
    _report(f"prefill T {T} latent {L:6d}", T, Hq, fp8, res, lines)


def leg_cap(Hq, fp8, rounds, lines):
    T, L = 1, 32768
    g = torch.Generator(device="cuda").manual_seed(Hq + fp8 + 7)
    dt = torch.bfloat16
    q = torch.randn(T, Hq, QK, device="cuda", dtype=dt, generator=g)
    kv = torch.randn(L // BS, BS, QK, device="cuda", dtype=dt, generator=g)
    idx = torch.randperm(L, device="cuda", generator=g)[:TOPK].to(torch.int32).view(T, TOPK).contiguous()
    ks = None
    cache = kv
    if fp8:
        cache, ks = aule.quantize_mla_cache_fp8(kv)
    want = aule.flash_attention_mla_sparse(q, cache, idx, **(dict(kv_scale=ks) if fp8 else {}))
    out = torch.empty_like(want)
    ws = torch.empty(32 * T * Hq * 514 * 4 + 16, device="cuda", dtype=torch.uint8)
    lib = _capi.get_lib()
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads_q = _capi.DTYPE_BF16, int(fp8), Hq
    d.num_blocks, d.block_size, d.total_tokens, d.topk, d.q_token_stride = L // BS, BS, T, TOPK, Hq * QK
    d.device = torch.cuda.current_device()
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.kv_cache, d.indices, d.out = q.data_ptr(), cache.data_ptr(), idx.data_ptr(), out.data_ptr()
    d.kv_scale = ks.data_ptr() if fp8 else None
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    ref = ctypes.byref(d)
    rb, planned = plan(T, Hq, TOPK)
    vmax = float(kv[..., :VD].float().abs().max())
    bound = 1e-3 + 2.0 ** -9 * vmax + 2.0 ** -8 * want.float().abs()
    calls = {}
    for n in (4, 8, 16, 32):
        if lib.aule_hip_debug_mla_sparse_launch_nsplit(ref, n) != 0:
            raise SystemExit(f"cap leg: nsplit {n} refused: {lib.aule_get_error()}")
        torch.cuda.synchronize()
        same = torch.equal(out.view(torch.int16), want.view(torch.int16))
        if not (same if n == planned else bool(((out.float() - want.float()).abs() <= 2 * bound).all())):
            raise SystemExit(f"cap leg: nsplit {n} disagrees with the entry")
        calls[n] = (lambda n=n: lib.aule_hip_debug_mla_sparse_launch_nsplit(ref, n))
    res = _alternated(calls, rounds)
    tiles = (TOPK + 63) // 64
    line = (f"  cap     T  1 context {L:6d} {'fp8 ' if fp8 else 'bf16'} heads {Hq:3d}: the plan {T} x {rb} x {planned}   "
            + "   ".join(f"nsplit {n:2d} ({-(-tiles // n)} tile{'s' if tiles > n else ' '} each) {res[n][1]} us" for n in calls)
            + f"   the cap costs {res[planned][0] - res[32][0]:+5.1f} us ({res[planned][0] / res[32][0]:4.2f}x)")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_sparse needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    only_cap = "--cap-only" in sys.argv    # (the cap legs alone)
    head = (f"# tools/bench_mla_sparse.py   (one MI355X; latent 576 / 512, topk {TOPK}, bf16 queries; plan = tokens x row blocks x nsplit workgroups; "
            f"{rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for fp8 in (() if only_cap else (False, True)):
        for Hq in HEADS:
            for T in TOKENS:
                for L in CONTEXT:
                    signal.alarm(budget)
                    leg_decode(Hq, T, L, fp8, rounds, lines)
                    signal.alarm(0)
                    torch.cuda.empty_cache()
            signal.alarm(budget)
            leg_prefill(Hq, fp8, rounds, lines)
            signal.alarm(0)
            torch.cuda.empty_cache()
    lines.append("# the split cap at T = 1 (C entry with the split count forced, descriptor and workspace made once: no torch-layer cost)")
    print(lines[-1], flush=True)
    for fp8 in (False, True):
        for Hq in HEADS:
            signal.alarm(budget)
            leg_cap(Hq, fp8, rounds, lines)
            signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
