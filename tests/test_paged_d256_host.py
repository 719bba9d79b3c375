"""Paged attention at head_dim 256 without a GPU: the additive C-ABI (symbols, layout, every answer the entries give before they need a
device), the launch plan's invariants over a grid of shapes, the torch layer's argument errors and a resource audit of the kernels."""
import ctypes
import itertools
import os
import re

import pytest

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

ENTRY, SIZE, HOOK, FORCE = ("aule_attention_paged_d256_ex", "aule_attention_paged_d256_workspace_size", "aule_hip_debug_paged_d256_plan",
                            "aule_hip_debug_paged_d256_launch_nsplit")
PTRS = ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "lse")
LAYOUT = dict(struct_size=0, dtype=4, cache_dtype=8, batch=12, heads_q=16, heads_kv=20, head_dim=24, block_size=28, max_blocks=32,
              total_tokens=36, max_seqlen_q=40, scale=44, window_size=48, device=52, q_token_stride=56, stream=64, q=72, k_cache=80,
              v_cache=88, block_tables=96, context_lens=104, cu_seqlens_q=112, out=120, lse=128, k_scale=136, v_scale=144, workspace=152,
              workspace_bytes=160)


def _fill(T=24, B=8, Hq=16, Hkv=8, bs=64, max_blocks=32, max_sq=3, window=-1, decode=False):
    """a well-formed descriptor with aligned dummy pointers: only ever handed to calls that answer before a launch"""
    d = _capi.PagedD256Desc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, _capi.KV_CACHE_SAME, B, Hq, Hkv, 256
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q, d.window_size = bs, max_blocks, T, max_sq, window
    d.q_token_stride = Hq * 256
    for n in PTRS:
        setattr(d, n, 4096)
    if decode:
        d.cu_seqlens_q = None
    return d


def _error(lib):
    return lib.aule_get_error().decode()


def _plan(lib, d):
    out = (ctypes.c_int32 * 6)()
    return lib.aule_hip_debug_paged_d256_plan(ctypes.byref(d), out, 6), list(out)


def test_symbols_and_layout_match_the_header():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name in (ENTRY, SIZE, HOOK, FORCE):
        assert re.search(r"\b%s\s*\(const aule_paged_d256_desc\*" % name, header) and hasattr(lib, name) and name in bound, name
    assert bound[SIZE][1] is ctypes.c_uint64
    assert "sizeof(aule_paged_d256_desc) = 168" in header and ctypes.sizeof(_capi.PagedD256Desc) == 168
    assert [n for n, _ in _capi.PagedD256Desc._fields_] == list(LAYOUT)
    assert all(getattr(_capi.PagedD256Desc, n).offset == off for n, off in LAYOUT.items())
    body = header.split("typedef struct aule_paged_d256_desc {")[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 25 and all(LAYOUT[n] == int(off) for n, off in quoted)
    assert "flash_attention_paged_d256" in aule.__all__ and callable(aule.flash_attention_paged_d256)


# (field, bad value, a piece of the reason): what the shape alone decides, and then what only a launch looks at
BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 152, "struct_size"), ("dtype", 0, "fp16 or bf16"), ("cache_dtype", 7, "cache_dtype"),
    ("head_dim", 128, "head_dim 128 unsupported by the head_dim 256 entry (256 only; 32, 64 and 128: aule_attention_paged_prefill_ex)"),
    ("head_dim", 192, "head_dim 192"), ("heads_kv", 3, "heads"), ("heads_kv", 0, "heads"),
    ("block_size", 0, "bad block_size"), ("max_blocks", 0, "bad block_size"), ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("q_token_stride", 16 * 256 - 8, "smaller than a token"), ("q_token_stride", 16 * 256 + 4, "must be a multiple of 8"),
    ("total_tokens", 1 << 30, "too large"), ("batch", 1 << 30, "too large"),
]
BAD_LAUNCH = [(n, None, "null tensor pointer") for n in ("q", "k_cache", "v_cache", "block_tables", "context_lens", "out")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("v_cache", 4097, "16-byte aligned"),
    ("k_scale", 4096, "FP8 caches only"), ("cache_dtype", _capi.KV_CACHE_FP8_E4M3, "null scale pointer"),
    ("workspace_bytes", 16, "workspace_bytes (16) is smaller than the plan's"), ("workspace", 4096 + 8, "workspace must be 16-byte aligned")]
_ids = lambda x: str(x).replace(" ", "_")[:40]   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_LAUNCH, ids=_ids)
def test_entries_refuse_each_bad_field_without_a_device(field, bad, needle):
    """-3 and a reason from both launches; 0 / -3 from the size query and the hook for a bad shape, their usual answer for a bad pointer"""
    lib = _capi.load()
    d = _fill(T=2, B=1, max_sq=2)   # 1 row block x 8 KV heads x 1 sequence: split, so the accepted size is not 0
    d.workspace, d.workspace_bytes = 4096, 1 << 40
    want = (lib.aule_attention_paged_d256_workspace_size(ctypes.byref(d)), _plan(lib, d))
    assert want[0] > 0 and want[1][0] == 6
    setattr(d, field, bad)
    for call in (lambda: lib.aule_attention_paged_d256_ex(ctypes.byref(d)), lambda: lib.aule_hip_debug_paged_d256_launch_nsplit(ctypes.byref(d), 2)):
        assert call() == -3
        assert needle in _error(lib) and _error(lib).startswith("Paged head_dim 256 attention failed: "), _error(lib)
    got = (lib.aule_attention_paged_d256_workspace_size(ctypes.byref(d)), _plan(lib, d))
    assert got == (want if (field, bad, needle) in BAD_LAUNCH else (0, (-3, [0] * 6)))


def test_null_descriptor_decode_rows_nsplit_and_nothing_to_do():
    lib = _capi.load()
    assert lib.aule_attention_paged_d256_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_paged_d256_workspace_size(None) == 0 and lib.aule_hip_debug_paged_d256_plan(None, None, 0) == -3
    assert lib.aule_hip_debug_paged_d256_launch_nsplit(ctypes.byref(_fill()), 0) == -3 and "nsplit (0) must be at least 1" in _error(lib)
    d = _fill(T=7, B=8, decode=True)   # plain decode (null offsets): sequence b owns row b, so the rows must be there
    assert lib.aule_attention_paged_d256_ex(ctypes.byref(d)) == -3 and "total_tokens < batch" in _error(lib) and _plan(lib, d)[0] == -3
    assert _plan(lib, _fill(T=9, B=8, decode=True))[0] == 6
    assert lib.aule_hip_debug_paged_d256_plan(ctypes.byref(_fill()), (ctypes.c_int32 * 6)(), 5) == -6   # the hook's capacity contract
    for field in ("total_tokens", "batch", "heads_q"):   # nothing to do: 0 with null pointers; a refused field is still refused
        d = _fill()
        setattr(d, field, 0)
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_paged_d256_ex(ctypes.byref(d)) == 0 and lib.aule_hip_debug_paged_d256_launch_nsplit(ctypes.byref(d), 3) == 0, field
        assert lib.aule_attention_paged_d256_workspace_size(ctypes.byref(d)) == 0 and _plan(lib, d)[0] == 0


def test_plan_invariants_over_a_grid_of_shapes():
    """(256 compute units: what the hook assumes without a device, and what an MI355X has)"""
    lib = _capi.load()
    split = single = 0
    for key in itertools.product((1, 3, 8, 64), ((16, 8), (16, 2), (8, 8)), (1, 5, 100), (128, 1024, 32768), (-1, 1024)):
        B, (Hq, Hkv), sq, cap, window = key
        T, g = B * sq + 3, Hq // Hkv
        d = _fill(T=T, B=B, Hq=Hq, Hkv=Hkv, bs=16, max_blocks=cap // 16, max_sq=sq, window=window)
        n, (rb, rows, nsplit, grid, lo, hi) = _plan(lib, d)
        assert n == 6 and rows == 64 and rb == -(-sq * g // 64), key
        keys = cap if window < 0 else min(cap, window + min(sq, -(-64 // g)))
        assert nsplit == max(1, min(-(-256 // (rb * Hkv * B)), 64, keys // 128)) and grid == rb * nsplit * Hkv * B, key
        ws = (lo & 0xffffffff) | (hi << 32)
        assert ws == (0 if nsplit == 1 else -(-nsplit * T * Hq * 258 * 4 // 16) * 16), key
        assert ws == lib.aule_attention_paged_d256_workspace_size(ctypes.byref(d)), key
        assert (n, [rb, rows, nsplit, grid, lo, hi]) == _plan(lib, d), key   # a function of the shape only
        split += nsplit > 1
        single += nsplit == 1
    assert split > 50 and single > 50
    # null offsets: one token per sequence whatever max_seqlen_q says; the block size enters through the capacity alone
    assert _plan(lib, _fill(T=8, B=8, Hq=128, Hkv=1, max_sq=4, decode=True)) == _plan(lib, _fill(T=8, B=8, Hq=128, Hkv=1, max_sq=1))
    assert _plan(lib, _fill(T=8, B=2, bs=24, max_blocks=86)) == _plan(lib, _fill(T=8, B=2, bs=8, max_blocks=258))


def test_argument_errors_are_value_errors_on_cpu_tensors():
    import torch
    T, B, Hq, Hkv, bs, nb = 6, 3, 4, 2, 16, 12
    q = torch.zeros(T, Hq, 256, dtype=torch.bfloat16)
    k = torch.zeros(nb, bs, Hkv, 256, dtype=torch.bfloat16)
    k8 = k.to(torch.float8_e4m3fn)
    bt, cl = torch.zeros(B, 4, dtype=torch.int32), torch.tensor([5, 9, 20], dtype=torch.int32)
    cu, one = torch.tensor([0, 2, 4, 6], dtype=torch.int32), torch.ones(Hkv)
    call = aule.flash_attention_paged_d256
    for args, kw, match in [
            ((q[..., :128], k[..., :128], k[..., :128], bt, cl, cu), {}, r"head_dim 256 only, got 128 \(head_dim 32, 64 and 128: flash_attention_paged_prefill\)"),
            ((q.float(), k.float(), k.float(), bt, cl, cu), {}, "fp16 or bf16"),
            ((q, k, k, bt, cl, cu), dict(k_scale=one, v_scale=one), "float8_e4m3fn caches only"),
            ((q, k8, k8, bt, cl, cu), dict(k_scale=one), "needs k_scale and v_scale"),
            ((q, k8, k8, bt, cl, cu), dict(k_scale=one, v_scale=torch.ones(3)), r"v_scale must be"),
            ((q, k[:, :0], k[:, :0], bt, cl, cu), {}, "block_size must be positive"),
            ((q, k, k, bt, cl[:2], cu), {}, r"block_tables must be \[batch, max_blocks\]"),
            ((q, k, k, bt, cl), {}, r"block_tables must be \[batch, max_blocks\]"),   # plain decode: q.shape[0] must be the batch
            ((q, k, k, bt, cl, cu[:3]), {}, r"cu_seqlens_q must be a \[batch \+ 1\]"),
            ((q, k, k, bt, cl, cu), dict(max_seqlen_q=0), "max_seqlen_q must be a positive int"),
            ((q[:3], k, k, bt, cl), dict(max_seqlen_q=2), "max_seqlen_q must be None or 1 without cu_seqlens_q")]:
        with pytest.raises(ValueError, match=match):
            call(*args, **kw)
    for args, kw in (((q, k, k, bt, cl, cu), dict(max_seqlen_q=2, return_lse=True)), ((q[:3], k8, k8, bt, cl), dict(k_scale=one, v_scale=one, window_size=8))):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):   # well-formed, on the CPU
            call(*args, **kw)


def test_kernels_neither_spill_nor_use_scratch(tmp_path):
    """{fp16, bf16} x {16-bit, FP8 cache} and both combines: no scratch, no spill, the LDS DESIGN.md 3.20 states (103 424 bytes)"""
    res = resource_report("fa_fwd_paged_d256_gfx950.hip", tmp_path)
    main = [n for n in res if "fa_fwd_paged_d256_kernel" in n]
    assert len(main) == 4 and sum("KvFp8" in n for n in main) == 2 and sum("Bf16Traits" in n for n in main) == 2, main
    assert len([n for n in res if "fa_paged_d256_combine_kernel" in n]) == 2 and len(res) == 6
    for n, r_ in res.items():
        assert r_.get("ScratchSize") == 0 and r_.get("VGPRs Spill") == 0 and r_.get("SGPRs Spill") == 0, (n, r_)
    assert all(res[n]["LDS Size"] == 103424 for n in main)
