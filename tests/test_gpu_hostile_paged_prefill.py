"""Hostile memory around the paged prefill (aule_attention_paged_prefill_ex), beside tests/test_gpu_hostile_memory.py and with its
helper (tests/hostile.py): the friendly problem against the same problem with NaN bits in every cache slot that no (table, length)
pair addresses, the unused table columns pointing at an all-NaN trap block, and out / lse / the guard bands filled with 0xFF.  The
rows the sequences own must be bit-identical in both runs, the rows they do not own must keep the fill pattern, guards and inputs
must be intact, and the hostile run's result must be right against the oracle."""
import ctypes

import numpy as np
import pytest

import hostile
from hostile import FRIENDLY, POISON, Arena, same_bits
from test_gpu_paged_prefill import Ragged, _judge
from util import torch_dtype

pytestmark = pytest.mark.gpu

# new tokens / lengths: no key at all; negative positions; a prefix and a tile boundary; no new tokens; a length that ends with its block
NS, LS = [1, 37, 70, 0, 3], [0, 20, 133, 50, 48]
CASES = [  # dtype, cache kind, Hq, Hkv, D, block size, window
    ("bf16", "16", 8, 2, 64, 16, -1),
    ("fp16", "fp8", 6, 2, 128, 24, 16),      # the general address path; 48: nothing stale in its last block, the next column trapped
    ("bf16", "16", 4, 1, 32, 128, -1),       # blocks larger than a tile
    ("fp16", "fp8", 8, 8, 64, 1, 300),
]


def _hostile_cache(p, dev, bt):
    """the device cache with one more block, NaN bits in every slot that (bt, clamped lengths) does not address"""
    nb, bs = dev.shape[:2]
    addressed = np.zeros((nb + 1, bs), dtype=bool)
    for b, _, _, L in p.sequences():
        j = np.arange(L)
        addressed[bt[b][j // bs], j % bs] = True
    assert not addressed[nb].any()
    bits = np.concatenate([dev, dev[:1]]).copy()
    bits[~addressed] = 0xFF if bits.dtype == np.uint8 else -1
    return bits


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-kv%s-H%dkv%d-D%d-bs%d-w%d" % c)
def test_paged_prefill(case, oracle_mod):
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    dtype, kind, Hq, Hkv, D, bs, window = case
    tdt = torch_dtype(dtype)
    p = Ragged(71, dtype, kind, Hq, Hkv, D, bs, NS, LS, lead=3, tail=5)
    fp8, B, T = p.fp8, p.B, p.T
    nb = p.kdev.shape[0]
    if fp8:
        kbits, vbits = p.kdev, p.vdev
    else:
        kbits, vbits = (torch.from_numpy(x).to(tdt).view(torch.int16).numpy() for x in (p.kdev, p.vdev))
    nblk = [(n + bs - 1) // bs for n in LS]
    trapped = p.bt.copy()
    for b in range(B):
        trapped[b, nblk[b]:] = nb                      # the trap block
    problems = {
        "friendly": (np.concatenate([kbits, kbits[1:2]]), np.concatenate([vbits, vbits[1:2]]), p.bt, FRIENDLY),
        "hostile": (_hostile_cache(p, kbits, trapped), _hostile_cache(p, vbits, trapped), trapped, POISON),
    }
    es, ces = 2, (1 if fp8 else 2)
    cache_bytes = (nb + 1) * bs * Hkv * D * ces
    regions = [("q", p.q.size * es, "in"), ("k_cache", cache_bytes, "in"), ("v_cache", cache_bytes, "in"),
               ("block_tables", p.bt.size * 4, "in"), ("context_lens", B * 4, "in"), ("cu_seqlens_q", (B + 1) * 4, "in")]
    if fp8:
        regions += [("k_scale", Hkv * 4, "in"), ("v_scale", Hkv * 4, "in")]
    regions += [("out", p.q.size * es, "out"), ("lse", T * Hq * 4, "out")]
    ar = Arena(torch, regions, max(D * es, Hkv * D * ces))
    d = _capi.PagedPrefillDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = hostile.DTYPE_CODE[dtype], 1 if fp8 else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, Hkv, D
    d.block_size, d.max_blocks = bs, p.bt.shape[1]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, p.max_sq, Hq * D
    d.scale, d.window_size, d.device = 0.0, window, torch.cuda.current_device()
    d.stream = torch.cuda.current_stream().cuda_stream
    for n, _, _ in regions:
        setattr(d, n, ar.ptr(n))
    failed = []

    def check(ok, what):
        if not ok:
            failed.append(what)
            print("FAILED:", what)

    own = torch.from_numpy(p.owned()).cuda()
    res = {}
    for name, (kc, vc, bt, pattern) in problems.items():
        orig = {"q": ar.upload("q", torch.from_numpy(p.q).to(tdt)), "k_cache": ar.upload("k_cache", kc), "v_cache": ar.upload("v_cache", vc),
                "block_tables": ar.upload("block_tables", bt.astype(np.int32)), "context_lens": ar.upload("context_lens", p.cl),
                "cu_seqlens_q": ar.upload("cu_seqlens_q", p.cu)}
        if fp8:
            orig["k_scale"] = ar.upload("k_scale", p.ks.astype(np.float32))
            orig["v_scale"] = ar.upload("v_scale", p.vs.astype(np.float32))
        ar.fill(pattern)
        _capi.check(lib.aule_attention_paged_prefill_ex(ctypes.byref(d)), "paged prefill")
        torch.cuda.synchronize()
        check(ar.guards_intact(), "%s: guard bytes written: %r" % (name, ar.damage()))
        for n, o in orig.items():
            check(ar.unchanged(n, o), "%s: input %s was written" % (name, n))
        out, lse = ar.view("out", tdt, (T, Hq, D)).clone(), ar.view("lse", torch.float32, (T, Hq)).clone()
        check(bool((out[~own].view(torch.uint8) == pattern).all()) and bool((lse[~own].view(torch.uint8) == pattern).all()),
              name + ": a row that belongs to no sequence was written")
        res[name] = (out, lse)
    check(same_bits(torch, res["hostile"][0][own], res["friendly"][0][own]), "out depends on cache slots / table columns / memory it does not own")
    check(same_bits(torch, res["hostile"][1][own], res["friendly"][1][own]), "lse depends on cache slots / table columns / memory it does not own")
    try:
        _judge(p, res["hostile"][0], res["hostile"][1], oracle_mod, window, "hostile paged prefill")
    except AssertionError as e:
        check(False, "oracle: %s" % e)
    assert not failed, "\n".join(failed)
