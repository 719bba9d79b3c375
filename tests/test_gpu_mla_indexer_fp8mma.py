"""The index logits with FP8 queries on the GPU (aule.mla_indexer_logits_fp8mma / aule_mla_indexer_logits_fp8mma_ex) against an fp64
statement of the contract.  EXACT data (codes in -3 .. 3, weights and scales powers of two: every partial sum is a multiple of 1/8 below
2^24) must equal the reference and the 16-bit-query call bit for bit.  RANDOM data: every element within 4 * gamma * B, gamma = (128 +
64 + 4) * 2^-24, B = k_scale * sum_h |w q_scale| sum_d |qc kc| (gamma * B bounds fp32 round-to-nearest accumulation; 4 is for the
matrix pipe's undocumented rounding); the largest err / (gamma * B) is printed.  The C entry writes into 0xFF bytes with logits_stride >
W and two rows of no sequence; cache rows and scales no token sees hold 0x7f codes and NaN; table entries past the used blocks are garbage."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu
GAMMA = (128 + 64 + 4) * 2.0 ** -24
NS, BASES = (1, 2, 8, 9, 17, 0, 2), (129, 31, 33, 127, 300, 40, None)   # new tokens and L - n per sequence; None: context_lens above W


def reference(q, w, kc, ks, bt, ctx, cu, W):
    """fp64: logits [T, W] (-inf where the key is not visible, NaN in rows of no sequence) and the bound B; w is weights * q_scale"""
    import torch
    bs, q, k, ks, w = kc.shape[1], q.float().double(), kc.view(-1, 128).float().double(), ks.view(-1).double(), w.double()
    out, bound = torch.full((len(q), W), float("nan"), dtype=torch.float64), torch.zeros(len(q), W, dtype=torch.float64)
    for b, L in enumerate(ctx.clamp(0, W).tolist()):
        s, e = (b, b + 1) if cu is None else (int(cu[b]), int(cu[b + 1]))
        for t in range(s, e):
            pos = L - e + t
            out[t] = float("-inf")
            if pos >= 0:
                j = torch.arange(pos + 1)
                rows = bt[b, j // bs].long() * bs + j % bs
                out[t, :pos + 1] = ks[rows] * (w[t][:, None] * (q[t] @ k[rows].T).clamp(min=0)).sum(0)
                bound[t, :pos + 1] = ks[rows] * (w[t].abs()[:, None] * (q[t].abs() @ k[rows].abs().T)).sum(0)
    return out, bound


@pytest.mark.parametrize("H,bs,exact,ragged", [(64, 64, True, True), (33, 48, True, True), (32, 64, True, True), (1, 48, True, True),
                                               (64, 48, True, False), (64, 64, False, True), (64, 48, False, True)])
def test_logits_against_fp64(H, bs, exact, ragged):
    import torch
    import aule
    from aule import _capi
    g = torch.Generator().manual_seed(7 * H + bs)
    ns = list(NS) if ragged else [1] * len(NS)
    mb = -(-(max(b for b in BASES if b) + max(ns)) // bs)
    W, B, T, msq = mb * bs, len(ns), sum(ns) + 2, max(ns)
    ctx = torch.tensor([W + 100 if base is None else base + n for n, base in zip(ns, BASES)], dtype=torch.int32)
    used = [-(-min(int(c), W) // bs) for c in ctx]
    nb = sum(used) + 3
    pool, seen = torch.randperm(nb, generator=g).int().tolist(), torch.zeros(nb * bs, dtype=torch.bool)
    bt = torch.tensor([[(2 ** 31 - 1, -2 ** 31, -7)[(b + i) % 3] for i in range(mb)] for b in range(B)], dtype=torch.int32)
    for b, u in enumerate(used):
        bt[b, :u] = torch.tensor([pool.pop() for _ in range(u)], dtype=torch.int32)
        j = torch.arange(min(int(ctx[b]), W) if ns[b] else 0)
        seen[bt[b, j // bs].long() * bs + j % bs] = True
    pick = lambda vals, *shape: torch.tensor(vals)[torch.randint(len(vals), shape, generator=g)]   # noqa: E731
    if exact:
        q, kc = (torch.randint(-3, 4, (n, m, 128), generator=g).float().to(torch.float8_e4m3fn) for n, m in ((T, H), (nb, bs)))
        w, qs, ks = pick([-2., -1., -.5, .5, 1., 2.], T, H), pick([.5, 1., 2.], T, H), pick([.5, 1., 2.], nb, bs)
    else:
        q, qs = aule.quantize_rows_fp8(torch.randn(T, H, 128, generator=g).to(torch.bfloat16))
        kc, ks = aule.quantize_indexer_cache_fp8(torch.randn(nb, bs, 128, generator=g).to(torch.bfloat16))
        w, qs = torch.randn(T, H, generator=g) / H ** 0.5, qs.reshape(T, H).contiguous()
    kc.view(torch.uint8).view(-1, 128)[~seen] = 0x7f
    ks.view(-1)[~seen] = float("nan")
    cu = torch.tensor([0] + torch.tensor(ns).cumsum(0).tolist(), dtype=torch.int32) if ragged else None
    want, bound = reference(q, w * qs, kc, ks, bt, ctx, cu, W)
    wide = torch.zeros(T, H * 128 + 64, dtype=torch.float8_e4m3fn)   # q is a slice of a wider tensor
    wide[:, :H * 128] = q.reshape(T, H * 128)
    q, w, qs, kc, ks, bt, ctx = (t.cuda() for t in (wide, w, qs, kc, ks, bt, ctx))
    q, cu = q[:, :H * 128].view(T, H, 128), cu.cuda() if ragged else None
    out = torch.full((T, W + 5), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    d = _capi.MlaIndexerLogitsFp8mmaDesc()
    d.struct_size, d.cache_dtype, d.heads, d.head_dim, d.batch, d.num_blocks, d.block_size, d.max_blocks = ctypes.sizeof(d), 1, H, 128, B, nb, bs, mb
    d.total_tokens, d.max_seqlen_q, d.device, d.q_token_stride, d.logits_stride = T, msq, -1, q.stride(0), W + 5
    for f, t in dict(q=q, weights=w, k_cache=kc, k_scale=ks, block_tables=bt, context_lens=ctx, q_scale=qs, cu_seqlens_q=cu, logits=out).items():
        setattr(d, f, t.data_ptr() if t is not None else None)
    torch.cuda.synchronize()
    assert _capi.get_lib().aule_mla_indexer_logits_fp8mma_ex(ctypes.byref(d)) == 0
    torch.cuda.synchronize()
    owned, bits = ~torch.isnan(want[:, 0]), out.cpu().view(torch.int32)
    assert bool((bits[:, W:] == -1).all()) and bool((bits[~owned] == -1).all()) and int((~owned).sum()) == 2
    got, want, bound = out.cpu()[owned][:, :W].double(), want[owned], bound[owned]
    fin = torch.isfinite(want)
    assert not bool(torch.isnan(got).any()) and torch.equal(torch.isneginf(got), ~fin) and bool(fin.any())
    n = T - 2 if ragged else B   # (the torch layer's plain decode is T == batch)
    call = lambda: aule.mla_indexer_logits_fp8mma(q[:n], w[:n], kc, ks, bt, ctx, cu, msq if ragged else None, q_scale=qs[:n])   # noqa: E731
    mine = call()
    assert torch.equal(mine.cpu().double(), got[:n]) and torch.equal(call(), mine)   # the torch layer, and a second run: the same bits
    if exact:
        twin = aule.mla_indexer_logits(q[:n].to(torch.bfloat16), (w * qs)[:n], kc, bt, ctx, cu, msq if ragged else None, k_scale=ks)
        assert torch.equal(got, want.float().double()) and torch.equal(mine.view(torch.int32), twin.view(torch.int32))
        return
    ratio = ((got - want).abs()[fin] / (GAMMA * bound[fin]).clamp(min=1e-300)).max().item()
    print("H %d bs %d: largest err / (gamma B) = %.4f" % (H, bs, ratio))
    assert bool(((got - want).abs()[fin] <= 4 * GAMMA * bound[fin]).all()), ratio
    # captured once, replayed after context_lens changed in place: the fresh result, on every replay
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        call()
        with torch.cuda.graph(graph, stream=stream):
            held = call()
    ctx.sub_(torch.tensor([0, 1, 0, 5, 40, 0, 0], dtype=torch.int32, device="cuda"))
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(held.view(torch.int32), call().view(torch.int32)) and not torch.equal(held.view(torch.int32), mine.view(torch.int32))
