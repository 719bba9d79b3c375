"""Sparse MLA over the per-128-scaled FP8 latent cache (656-byte rows) on the GPU: csrc/fa_fwd_mla_sparse_ds_gfx950.hip and
csrc/mla_kv_append_ds_gfx950.hip behind aule.flash_attention_mla_sparse / aule.mla_kv_append with a uint8 [.., 656] cache.

The judge is fp64 softmax attention over dequantize_mla_cache_fp8_ds(cache).double() rows gathered by the list (duplicates kept,
entries outside the cache skipped).  The bar is tests/test_gpu_mla_sparse.py's for the bf16 call -- util.fwd_tol("bf16", max |V|)
for out, 1e-3 for lse, -inf and zeros exactly where a token has no valid entry -- because the kernel multiplies the same bf16 image;
and, under the same plan, it equals the bf16 call over the dequantised cache bit for bit.  Neighbouring groups and rows of the cache
differ by 2^16 in scale, and every row that no valid entry names holds NaN bits in codes, scales and rotary part alike."""
import math

import numpy as np
import pytest

from util import assert_close, fwd_tol

pytestmark = pytest.mark.gpu

SCALE = 0.25 / math.sqrt(576)   # (the big groups hold values around 16: keeps the softmax from collapsing onto one key)


def make_cache(torch, aule, seed, nb, bs):
    """uint8 [nb, bs, 656] on the CPU: N(0, 1) times 2^4 or 2^-12, alternating with group + row, quantised by the library's rule"""
    S = nb * bs
    x = torch.randn(S, 576, generator=torch.Generator().manual_seed(seed))
    mag = torch.where((torch.arange(S)[:, None] + torch.arange(4)[None, :]) % 2 == 0, 16.0, 2.0 ** -12)
    x[:, :512] *= mag.repeat_interleave(128, dim=1)
    return aule.quantize_mla_cache_fp8_ds(x.view(nb, bs, 576))


def judge(kv, q, idx, S):
    """(out [T, Hq, 512], lse [T, Hq]) in fp64 from the dequantised rows kv [S, 576]"""
    T, Hq, _ = q.shape
    out, lse = np.zeros((T, Hq, 512)), np.full((T, Hq), -np.inf)
    for t in range(T):
        rows = kv[idx[t][(idx[t] >= 0) & (idx[t] < S)]]
        if len(rows):
            s = q[t] @ rows.T * SCALE
            p = np.exp(s - s.max(axis=-1, keepdims=True))
            lse[t] = s.max(axis=-1) + np.log(p.sum(axis=-1))
            out[t] = (p / p.sum(axis=-1, keepdims=True)) @ rows[:, :512]
    return out, lse


# (T, Hq, topk, block_size): one row block partly filled and a block boundary; one tile, a tile edge, several tiles with a split
@pytest.mark.parametrize("T,Hq,topk,bs", [(1, 1, 1, 1), (3, 16, 64, 16), (1, 65, 65, 64), (3, 128, 200, 16), (1, 16, 200, 1), (3, 65, 64, 64),
                                          (1, 128, 1, 16)])
def test_against_the_fp64_judge_and_the_bf16_call_bit_for_bit(T, Hq, topk, bs):
    import torch
    import aule
    nb = max(2, 160 // bs)
    S = nb * bs
    clean = make_cache(torch, aule, 7 * T + Hq + topk, nb, bs)
    # random slots (a shuffled pool), a slot listed twice, -1 padding, entries past the cache; the last of several tokens names nothing
    idx = torch.randint(0, S, (T, topk), generator=torch.Generator().manual_seed(Hq + topk), dtype=torch.int32)
    if topk >= 4:
        idx[:, 1], idx[:, topk // 2], idx[:, -1], idx[0, 2] = idx[:, 0], -1, S, -2 ** 31
    if T > 1:
        idx[-1] = -1
    named = torch.zeros(S, dtype=torch.bool)
    named[idx[(idx >= 0) & (idx < S)].long()] = True
    poisoned = clean.clone().view(S, 656)
    poisoned[~named] = 0xFF
    q = torch.randn(T, Hq, 576, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    deq = aule.dequantize_mla_cache_fp8_ds(clean)
    qd, idxd = q.cuda(), idx.cuda()
    out, lse = aule.flash_attention_mla_sparse(qd, poisoned.view(nb, bs, 656).cuda(), idxd, scale=SCALE, return_lse=True)
    only = aule.flash_attention_mla_sparse(qd, poisoned.view(nb, bs, 1, 656).cuda(), idxd, scale=SCALE)
    ref16 = aule.flash_attention_mla_sparse(qd, deq.cuda(), idxd, scale=SCALE, return_lse=True)
    torch.cuda.synchronize()
    kv = deq.double().view(S, 576).numpy()
    ref, lref = judge(kv, q.double().numpy(), idx.numpy(), S)
    got, glse = out.float().cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
    atol, rtol = fwd_tol("bf16", float(np.abs(kv[:, :512]).max()))
    none = ~np.isfinite(lref)
    lerr = float(np.abs(glse[~none] - lref[~none]).max()) if (~none).any() else 0.0
    print("max |out err| %.3g (atol %.3g + %.3g |ref|), max |lse err| %.3g, rows without a key %d" % (np.abs(got - ref).max(), atol, rtol, lerr, none.sum()))
    assert_close(got, ref, atol, rtol, "out")
    assert np.array_equal(np.isneginf(glse), none) and bool((got[none] == 0).all()) and lerr <= 1e-3
    assert torch.equal(only, out)                                            # return_lse both ways
    assert torch.equal(out, ref16[0]) and torch.equal(lse, ref16[1])         # the same image under the same plan


@pytest.mark.parametrize("rope", [None, "half", "interleaved"])
@pytest.mark.parametrize("T", [1, 5, 300])
def test_append_equals_the_torch_quantiser_byte_for_byte(T, rope):
    """the rows against quantize_mla_cache_fp8_ds of what the 16-bit append writes ([c_kv | rope(k_pe)], the rotation rounded once to
    bf16); inputs are strided slices of a wider projection; a group of zeros and groups whose amax is 448 * 2^n exactly"""
    import torch
    import aule
    bs = 16
    nb = (T + 7 + bs - 1) // bs
    S = nb * bs
    g = torch.Generator().manual_seed(T)
    proj = (torch.randn(T, 592, generator=g) * 3.0).to(torch.bfloat16)
    proj[0, 128:256] = 0
    proj[0, 256:384] = proj[0, 256:384].clamp(-40, 40)
    proj[0, 300] = 56.0          # 448 * 2^-3: amax / 448 is a power of two, the ceil must not step up
    proj[T - 1, 5] = -3584.0     # 448 * 2^3
    proj = proj.cuda()
    c_kv, k_pe = proj[:, :512], proj[:, 512:576]
    slots = torch.randperm(S, generator=g)[:T].cuda()
    if T > 2:
        slots[1] = -1
    kw = {}
    if rope:
        ang = torch.arange(64, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(32, dtype=torch.float32) / 32))[None, :]
        kw = dict(cos=ang.cos().cuda(), sin=ang.sin().cuda(), positions=torch.randint(0, 64, (T,), generator=g).cuda(), rope_layout=rope)
    cache = torch.full((nb, bs, 656), 0xA5, dtype=torch.uint8, device="cuda")
    rows16 = torch.zeros(nb, bs, 576, dtype=torch.bfloat16, device="cuda")
    aule.mla_kv_append(c_kv, k_pe, cache, slots, **kw)
    aule.mla_kv_append(c_kv, k_pe, rows16, slots, **kw)
    torch.cuda.synchronize()
    want = aule.quantize_mla_cache_fp8_ds(rows16.cpu()).view(S, 656)
    written = torch.zeros(S, dtype=torch.bool)
    written[slots[slots >= 0].cpu()] = True
    want[~written] = 0xA5        # unwritten slots, the skipped token's included, keep their bytes
    got = cache.cpu().view(S, 656)
    assert torch.equal(got, want), (got != want).nonzero()[:8]
    s0 = got[slots[0].item()][512:528].contiguous().view(torch.float32)
    assert s0[1] == 1.0 and s0[2] == 0.125 and got[slots[T - 1].item()][512:516].contiguous().view(torch.float32)[0] == 8.0


def test_graph_replay_of_append_and_attention_reads_the_current_list():
    """append + attention captured in one graph, replayed twice per list with the list changed in between: the eager result, bit for bit"""
    import torch
    import aule
    T, Hq, topk, nb, bs = 2, 16, 256, 20, 16
    S = nb * bs
    cache = make_cache(torch, aule, 5, nb, bs).cuda()
    g = torch.Generator().manual_seed(9)
    c_kv, k_pe = torch.randn(T, 512, generator=g).to(torch.bfloat16).cuda(), torch.randn(T, 64, generator=g).to(torch.bfloat16).cuda()
    slots = torch.tensor([3, S - 1], dtype=torch.int64).cuda()
    q = torch.randn(T, Hq, 576, generator=g).to(torch.bfloat16).cuda()
    idx = torch.randint(0, S, (T, topk), generator=g, dtype=torch.int32).cuda()
    idx[:, 0] = 3                # the appended row is among the keys

    def fn():
        aule.mla_kv_append(c_kv, k_pe, cache, slots)
        return aule.flash_attention_mla_sparse(q, cache, idx, scale=SCALE, return_lse=True)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = fn()
    for new in (idx.clone(), idx.flip(1).contiguous().clamp_(max=S // 2), torch.full_like(idx, -1)):
        idx.copy_(new)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        eager = fn()
        torch.cuda.synchronize()
        assert torch.equal(res[0], eager[0]) and torch.equal(res[1], eager[1])
    assert bool(torch.isneginf(res[1]).all()) and bool((res[0] == 0).all())
