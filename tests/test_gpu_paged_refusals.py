"""What aule_attention_paged_decode_ex, aule_attention_paged_decode_fp8_ex and aule_attention_paged_query_ex refuse once the library is
initialised (without a device they answer -1 before they look at the descriptor, so tests/paged_sweep.py cannot ask them): every
single-field mutation of that sweep which the entry refuses, and the null-tensor and null-scale cases, is -3 with exactly the text the
entries had before their rules were stated once (the strings below are copied from aule_capi.cpp as it was then).  A refused call
launches nothing.  Before the refusals one good call per entry, at the smallest shape that crosses a block boundary, against the fp64
oracle under the bound of tests/test_gpu_paged_query.py."""
import ctypes

import numpy as np
import pytest

from test_gpu_paged_query import LSE_ATOL, Problem
from util import assert_close, fwd_tol

pytestmark = pytest.mark.gpu

B, HQ, HKV, D, BS, MAX_BLOCKS, CONTEXT = 1, 2, 1, 32, 16, 2, 17
ENTRIES = {  # entry -> (the _capi structure, the symbol, seq_q, the words before the reason)
    "decode": ("PagedDesc", "aule_attention_paged_decode_ex", 1, "Paged attention failed: "),
    "decode_fp8": ("PagedFp8Desc", "aule_attention_paged_decode_fp8_ex", 1, "Paged FP8 attention failed: "),
    "query": ("PagedQueryDesc", "aule_attention_paged_query_ex", 2, "Paged query attention failed: "),
}
STRUCT_SIZE = "bad descriptor (struct_size mismatch)"
DTYPE = {"decode": "dtype must be fp16 or bf16", "decode_fp8": "dtype (of q / out) must be fp16 or bf16", "query": "dtype (of q / out) must be fp16 or bf16"}
CACHE_DTYPE = "cache_dtype must be AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3"
HEAD_DIM = "head_dim %u unsupported (32, 64 or 128)"
HEADS = "heads_q (%u) must be divisible by heads_kv (%u)"
SEQ_Q = "seq_q %u unsupported (1 to 64 query tokens per sequence)"
BLOCKS = "bad block_size / max_blocks"
NULL_TENSOR = "null tensor pointer"
NULL_SCALE = "null scale pointer (k_scale and v_scale are [heads_kv] fp32 device arrays)"
SCALE_16 = "k_scale / v_scale apply to FP8 caches only; a 16-bit cache holds the values themselves"


def refusals(entry, fp8, size, a_pointer):
    """(field, value, reason) for every mutation the entry refuses; value None: a null pointer"""
    r = ([("struct_size", v, STRUCT_SIZE) for v in (0, size - 8, size + 8)] + [("dtype", v, DTYPE[entry]) for v in (-1, 0, 3)] +
         [("head_dim", v, HEAD_DIM % v) for v in (0, 48, 256)] + [("heads_kv", v, HEADS % (HQ, v)) for v in (0, 5)] +
         [("block_size", 0, BLOCKS)] + [("max_blocks", v, BLOCKS) for v in (0, 1 << 26, 1 << 28)] +
         [(f, None, NULL_TENSOR) for f in ("q", "k_cache", "v_cache", "block_tables", "context_lens", "out")])
    if entry == "query":
        r += [("cache_dtype", v, CACHE_DTYPE) for v in (2, -1)] + [("seq_q", v, SEQ_Q % v) for v in (0, 65)]
        r += [("cache_dtype", 0, SCALE_16)] if fp8 else [("cache_dtype", 1, NULL_SCALE), ("k_scale", a_pointer, SCALE_16), ("v_scale", a_pointer, SCALE_16)]
    if fp8:
        r += [("k_scale", None, NULL_SCALE), ("v_scale", None, NULL_SCALE)]
    return r


@pytest.mark.parametrize("entry,dtype,kind", [("decode", "bf16", "16"), ("decode_fp8", "fp16", "fp8"), ("query", "bf16", "16"), ("query", "fp16", "fp8")])
def test_good_call_then_every_refusal(entry, dtype, kind, oracle_mod):
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    cls, symbol, Sq, words = ENTRIES[entry]
    call = getattr(lib, symbol)
    p = Problem(53, dtype, kind, B, HQ, HKV, Sq, D, BS, [CONTEXT])
    p.bt = np.ascontiguousarray(p.bt[:, :MAX_BLOCKS])            # (the table without its spare columns: 17 keys cross into block 2 of 2)
    (q, kc, vc, bt, cl), scales = p.device(torch)
    if entry != "query":
        q = q[:, :, 0].contiguous()
    out = torch.empty_like(q)
    lse = torch.empty((B, HQ, Sq), device="cuda", dtype=torch.float32) if entry == "query" else None

    def desc():
        d = getattr(_capi, cls)()
        d.struct_size = ctypes.sizeof(d)
        d.dtype = {"fp16": 1, "bf16": 2}[dtype]
        d.batch, d.heads_q, d.heads_kv, d.head_dim, d.block_size, d.max_blocks = B, HQ, HKV, D, BS, MAX_BLOCKS
        d.scale, d.window_size, d.device = 0.0, -1, q.device.index or 0
        d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
        d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
        if entry == "query":
            d.seq_q, d.cache_dtype, d.lse = Sq, int(p.fp8), lse.data_ptr()
        if p.fp8:
            d.k_scale, d.v_scale = scales["k_scale"].data_ptr(), scales["v_scale"].data_ptr()
        return d

    assert call(ctypes.byref(desc())) == 0, _capi.last_error(lib)
    torch.cuda.synchronize()
    got, ref = out.float().cpu().numpy().reshape(B, HQ, Sq, D), p.judge(oracle_mod)
    atol, rtol = fwd_tol(dtype, p.vmax)
    print("%s %s %s: max |err| %.3g (atol %.3g)" % (entry, dtype, kind, np.abs(got - ref).max(), atol))
    assert_close(got, ref, atol, rtol, entry)
    if lse is not None:
        lerr = float(np.abs(lse.cpu().numpy().astype(np.float64) - p.lse_f64()).max())
        assert lerr <= LSE_ATOL, lerr

    size = ctypes.sizeof(getattr(_capi, cls))
    cases = refusals(entry, p.fp8, size, q.data_ptr())
    assert len(cases) >= 21
    for field, value, reason in cases:
        d = desc()
        setattr(d, field, value)
        assert call(ctypes.byref(d)) == -3, (field, value)
        assert _capi.last_error(lib) == words + reason, (field, value, _capi.last_error(lib))
    for field in ("batch", "heads_q"):                           # nothing to do: 0, whatever the pointers
        d = desc()
        setattr(d, field, 0)
        d.q = d.out = None
        assert call(ctypes.byref(d)) == 0, field
