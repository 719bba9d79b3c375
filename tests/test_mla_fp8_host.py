"""The FP8 latent cache of the paged MLA and the latent cache append, without a GPU: the additive C-ABI (symbols, the layouts of the
two new descriptors against the header and the static_asserts, every answer the entries give before they need a device, the
agreement of the FP8 size query with the 16-bit one), the argument errors and signatures of the torch layer, quantize_mla_cache_fp8
on the CPU, the build rule and a resource audit of the new kernels compiled with the Makefile's compiler and flags."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
FP8_ENTRY, FP8_SIZE, APPEND = "aule_attention_mla_paged_fp8_ex", "aule_attention_mla_paged_fp8_workspace_size", "aule_mla_kv_append_ex"
MLA_LAYOUT = dict(struct_size=0, dtype=4, batch=8, heads_q=12, qk_dim=16, v_dim=20, block_size=24, max_blocks=28, total_tokens=32,
                  max_seqlen_q=36, scale=40, device=44, q_token_stride=48, stream=56, q=64, kv_cache=72, block_tables=80, context_lens=88,
                  cu_seqlens_q=96, out=104, lse=112, workspace=120, workspace_bytes=128)
FP8_LAYOUT = dict(MLA_LAYOUT, kv_scale=136)
APPEND_LAYOUT = dict(struct_size=0, dtype=4, cache_dtype=8, rope_layout=12, total_tokens=16, num_blocks=20, block_size=24, table_len=28,
                     table_pitch=32, device=36, c_kv_token_stride=40, k_pe_token_stride=48, stream=56, c_kv=64, k_pe=72, kv_cache=80,
                     slot_mapping=88, kv_scale=96, cos=104, sin=112, positions=120)
FP8_PTRS = ("q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "lse", "kv_scale")
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _fill_fp8(T=24, B=8, Hq=16, bs=64, max_blocks=32, max_sq=3, dtype=2, cls=None):
    """a well-formed descriptor whose pointers are aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = (cls or _capi.MlaPagedFp8Desc)()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = dtype, B, Hq, 576, 512
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = bs, max_blocks, T, max_sq
    d.q_token_stride = Hq * 576
    for n in FP8_PTRS:
        if hasattr(d, n):
            setattr(d, n, 4096)
    return d


def _fill_append(T=5, fp8=False, rope=False):
    d = _capi.MlaKvAppendDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.rope_layout = 2, 1 if fp8 else 0, 0
    d.total_tokens, d.num_blocks, d.block_size = T, 4, 16
    d.c_kv_token_stride, d.k_pe_token_stride = 512, 64
    d.c_kv = d.k_pe = d.kv_cache = d.slot_mapping = 4096
    if fp8:
        d.kv_scale = 4096
    if rope:
        d.cos = d.sin = d.positions = 4096
        d.table_len = 100
    return d


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, desc in ((FP8_ENTRY, "aule_mla_paged_fp8_desc"), (FP8_SIZE, "aule_mla_paged_fp8_desc"), (APPEND, "aule_mla_kv_append_desc")):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, desc), header), name
        assert hasattr(lib, name) and name in bound, name
    assert bound[FP8_SIZE][1] is ctypes.c_uint64
    assert re.search(r"aule_hip_debug_mla_plan\s*\(const aule_mla_paged_desc\*", header)   # the plan hook keeps the 16-bit descriptor
    for name in ("flash_attention_mla_paged_fp8", "mla_kv_append", "quantize_mla_cache_fp8"):
        assert name in aule.__all__ and callable(getattr(aule, name)), name
    # the sentence about what is not built no longer lists the two
    comment = header.split("typedef struct aule_mla_paged_desc {")[0].rsplit("/* Paged MLA (additive)", 1)[1]
    not_built = comment.split("Not built:")[1].split("*/")[0]
    assert "FP8" not in not_built and "append" not in not_built and "sliding window" in not_built and "backward" in not_built and "192 / 128" in not_built


def test_signatures():
    sig = inspect.signature(aule.flash_attention_mla_paged_fp8)
    assert list(sig.parameters) == ["q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale", "return_lse", "kv_scale"]
    assert all(sig.parameters[n].default is None for n in ("cu_seqlens_q", "max_seqlen_q", "scale", "kv_scale")) and sig.parameters["return_lse"].default is False
    sig = inspect.signature(aule.mla_kv_append)
    assert list(sig.parameters) == ["c_kv", "k_pe", "kv_cache", "slot_mapping", "kv_scale", "cos", "sin", "positions", "rope_layout"]
    assert all(sig.parameters[n].default is None for n in ("kv_scale", "cos", "sin", "positions")) and sig.parameters["rope_layout"].default == "half"
    assert list(inspect.signature(aule.quantize_mla_cache_fp8).parameters) == ["kv_cache"]
    # the 16-bit call keeps its signature
    assert list(inspect.signature(aule.flash_attention_mla_paged).parameters) == ["q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q",
                                                                                  "max_seqlen_q", "scale", "return_lse"]


@pytest.mark.parametrize("struct,cls,layout,size", [("aule_mla_paged_fp8_desc", "MlaPagedFp8Desc", FP8_LAYOUT, 144),
                                                    ("aule_mla_kv_append_desc", "MlaKvAppendDesc", APPEND_LAYOUT, 128)], ids=["fp8", "append"])
def test_descriptor_layouts_match_the_header(struct, cls, layout, size):
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with static_asserts"""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    C = getattr(_capi, cls)
    assert "sizeof(%s) = %d" % (struct, size) in header and "sizeof(%s) == %d" % (struct, size) in capi
    assert ctypes.sizeof(C) == size
    assert [n for n, _ in C._fields_] == list(layout)
    for name, off in layout.items():
        assert getattr(C, name).offset == off, name
    body = header.split("typedef struct %s {" % struct)[1].split("}")[0]
    quoted = dict(re.findall(r"(\w+);\s*/\* offset (\d+)", body))
    assert set(quoted) == set(layout) - {"struct_size"}
    for name, off in quoted.items():
        assert layout[name] == int(off), name
    pinned = re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, capi)
    assert len(pinned) >= (1 if struct.endswith("fp8_desc") else 20)
    for name, off in pinned:
        assert layout[name] == int(off), name


def test_fp8_descriptor_is_the_16_bit_one_plus_kv_scale():
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert ctypes.sizeof(_capi.MlaPagedDesc) == 136 and "sizeof(aule_mla_paged_desc) == 136" in capi
    for name, _ in _capi.MlaPagedDesc._fields_:
        a, b = getattr(_capi.MlaPagedDesc, name), getattr(_capi.MlaPagedFp8Desc, name)
        assert (a.offset, a.size) == (b.offset, b.size) == (MLA_LAYOUT[name], a.size), name
    assert _capi.MlaPagedFp8Desc.kv_scale.offset == ctypes.sizeof(_capi.MlaPagedDesc)
    shared = set(re.findall(r"offsetof\(aule_mla_paged_fp8_desc, (\w+)\) == offsetof\(aule_mla_paged_desc, \1\)", capi))
    assert {"q", "kv_cache", "out", "lse", "workspace", "workspace_bytes", "q_token_stride", "stream"} <= shared
    assert "offsetof(aule_mla_paged_fp8_desc, kv_scale) == sizeof(aule_mla_paged_desc)" in capi


# (field, bad value, a piece of the reason)
FP8_BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 136, "struct_size"), ("struct_size", 152, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("qk_dim", 512, "qk_dim 512"), ("v_dim", 576, "v_dim 576"),
    ("block_size", 0, "bad block_size"), ("max_blocks", 0, "bad block_size"), ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("q_token_stride", 16 * 576 - 8, "q_token_stride (9208) is smaller than a token"),
    ("q_token_stride", 16 * 576 + 4, "q_token_stride (9220) must be a multiple of 8"),
    ("total_tokens", 1 << 30, "too large"), ("batch", 1 << 30, "too large"),
]
FP8_BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "kv_cache", "block_tables", "context_lens", "out")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("kv_cache", 4097, "16-byte aligned"),
    ("kv_scale", None, "null kv_scale"), ("kv_scale", 4096 + 2, "kv_scale must be 4-byte aligned")]


@pytest.mark.parametrize("field,bad,needle", FP8_BAD_SHAPE + FP8_BAD_POINTER, ids=_ids)
def test_fp8_launch_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason with the entry's own prefix, before the device is needed"""
    lib = _capi.load()
    d = _fill_fp8()
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Paged MLA FP8 attention failed: "), _error(lib)


def test_fp8_null_descriptor_and_a_16_bit_descriptor():
    lib = _capi.load()
    assert lib.aule_attention_mla_paged_fp8_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_mla_paged_fp8_workspace_size(None) == 0
    # each entry refuses the other kind's size
    d = _fill_fp8()
    assert lib.aule_attention_mla_paged_ex(ctypes.cast(ctypes.byref(d), ctypes.POINTER(_capi.MlaPagedDesc))) == -3
    assert _error(lib).startswith("Paged MLA attention failed: ") and "struct_size" in _error(lib)


@pytest.mark.parametrize("field,bad,needle", FP8_BAD_SHAPE, ids=_ids)
def test_fp8_size_query_refuses_what_the_launch_refuses(field, bad, needle):
    lib = _capi.load()
    d = _fill_fp8(T=2, B=1, max_sq=2)
    assert lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d)) > 0
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d)) == 0
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == -3


def test_fp8_size_query_equals_the_16_bit_one_and_reads_no_pointer():
    lib = _capi.load()
    seen = set()
    for B in (1, 3, 8, 64):
        for Hq in (5, 16, 128):
            for sq in (1, 3):
                for cap in (128, 2048, 131072):
                    kw = dict(T=B * sq + 3, B=B, Hq=Hq, bs=64, max_blocks=cap // 64, max_sq=sq)
                    d8, d16 = _fill_fp8(**kw), _fill_fp8(cls=_capi.MlaPagedDesc, **kw)
                    a = lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d8))
                    assert a == lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d16)), kw
                    for n in FP8_PTRS:
                        if n != "cu_seqlens_q":   # (null offsets are a statement about the problem: plain decode)
                            setattr(d8, n, None)
                    assert lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d8)) == a, kw
                    seen.add(a > 0)
    assert seen == {True, False}


def test_fp8_nothing_to_do_returns_zero_without_a_launch():
    lib = _capi.load()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill_fp8()
        setattr(d, field, 0)
        for n in FP8_PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == 0, field
        assert lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d)) == 0
        d.qk_dim = 512
        assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == -3


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entries_report_uninitialised_without_a_gpu():
    lib = _capi.load()
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(_fill_fp8())) == -1
    assert lib.aule_mla_kv_append_ex(ctypes.byref(_fill_append())) == -1
    assert lib.aule_mla_kv_append_ex(ctypes.byref(_fill_append(fp8=True, rope=True))) == -1


APPEND_BAD = [  # (fp8, rope, field, bad value, a piece of the reason)
    (False, False, "struct_size", 0, "struct_size"), (False, False, "struct_size", 168, "struct_size"),
    (False, False, "dtype", 0, "fp16 or bf16"), (False, False, "dtype", 3, "fp16 or bf16"),
    (False, False, "cache_dtype", 2, "cache_dtype must be"), (False, False, "cache_dtype", -1, "cache_dtype must be"),
    (False, False, "rope_layout", 2, "unknown rope_layout 2"), (False, True, "rope_layout", -1, "unknown rope_layout -1"),
    (False, False, "block_size", 0, "block_size must be positive"),
    (False, False, "c_kv_token_stride", 504, "c_kv_token_stride (504) is smaller than a row"),
    (False, False, "k_pe_token_stride", 0, "k_pe_token_stride (0) is smaller than a row"),
    (False, False, "c_kv_token_stride", 516, "multiples of 8"), (False, False, "k_pe_token_stride", 68, "multiples of 8"),
    (False, False, "cos", 4096, "RoPE group only partly given"), (False, False, "positions", 4096, "RoPE group only partly given"),
    (False, False, "table_len", 7, "RoPE group only partly given"), (False, True, "sin", None, "RoPE group only partly given"),
    (False, True, "table_len", 0, "RoPE group only partly given"),
    (False, True, "table_pitch", 16, "table_pitch must be 0 or a multiple of 4"), (False, True, "table_pitch", 34, "table_pitch must be 0 or a multiple of 4"),
    (False, False, "c_kv", None, "null tensor pointer"), (False, False, "k_pe", None, "null tensor pointer"),
    (False, False, "kv_cache", None, "null tensor pointer"), (False, False, "slot_mapping", None, "null tensor pointer"),
    (True, False, "kv_scale", None, "null kv_scale"), (False, False, "kv_scale", 4096, "kv_scale applies to an FP8 cache only"),
    (True, False, "kv_scale", 4098, "kv_scale must be 4-byte aligned"),
    (False, False, "c_kv", 4104, "16-byte aligned"), (False, False, "k_pe", 4098, "16-byte aligned"), (True, False, "kv_cache", 4104, "16-byte aligned"),
    (False, True, "cos", 4100, "16-byte aligned"), (False, True, "sin", 4104, "16-byte aligned"),
]


@pytest.mark.parametrize("fp8,rope,field,bad,needle", APPEND_BAD, ids=_ids)
def test_append_refuses_each_bad_field(fp8, rope, field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library)"""
    lib = _capi.load()
    d = _fill_append(fp8=fp8, rope=rope)
    setattr(d, field, bad)
    assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA KV append failed: "), _error(lib)


def test_append_null_descriptor_and_nothing_to_do():
    lib = _capi.load()
    assert lib.aule_mla_kv_append_ex(None) == -3 and "struct_size" in _error(lib)
    for fp8 in (False, True):
        d = _fill_append(T=0, fp8=fp8)
        d.c_kv = d.k_pe = d.kv_cache = d.slot_mapping = d.kv_scale = None
        assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == 0   # no token: 0 with null pointers, in any process
        d.rope_layout = 5
        assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == -3   # a refused field is still refused
    # table_pitch values the kernel takes: 0 (= 32) and multiples of 4 from 32 on pass the check (and then need the device)
    for pitch in (0, 32, 36, 64):
        d = _fill_append(T=0, rope=True)
        d.table_pitch = pitch
        assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == 0, pitch


def test_python_argument_errors_of_the_fp8_call():
    import torch
    T, B, Hq, bs, nb = 6, 3, 16, 16, 12
    q = torch.zeros(T, Hq, 576, dtype=torch.bfloat16)
    kv = torch.zeros(nb, bs, 576, dtype=torch.float8_e4m3fn)
    bt = torch.zeros(B, 4, dtype=torch.int32)
    cl = torch.tensor([5, 9, 20], dtype=torch.int32)
    cu = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    call = aule.flash_attention_mla_paged_fp8
    for bad in (torch.bfloat16, torch.float16, torch.float32, torch.float8_e4m3fnuz, torch.float8_e5m2, torch.uint8):
        with pytest.raises(ValueError, match="must be torch.float8_e4m3fn"):
            call(q, torch.zeros(nb, bs, 576).to(bad), bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q.float(), kv, bt, cl, cu)
    with pytest.raises(ValueError, match="latent width must be 576"):
        call(q, kv[..., :512], bt, cl, cu)
    with pytest.raises(ValueError, match="latent width must be 576"):
        call(q[..., :512], kv, bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,576\]"):
        call(q, kv.view(nb, bs, 2, 288), bt, cl, cu)
    for bad in (torch.ones(2), torch.ones(1, 1), torch.ones(3, 1)):
        with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
            call(q, kv, bt, cl, cu, kv_scale=bad)
    with pytest.raises(ValueError, match="block_size must be positive"):
        call(q, kv[:, :0], bt, cl, cu)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        call(q, kv, bt, cl[:2], cu)
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        call(q, kv, bt, cl, cu.long())
    with pytest.raises(ValueError, match="max_seqlen_q must be None or 1 without cu_seqlens_q"):
        call(q[:3], kv, bt, cl, max_seqlen_q=2)
    wide = torch.zeros(T, Hq * 576 + 4, dtype=torch.bfloat16)[:, :Hq * 576].view(T, Hq, 576)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        call(wide, kv, bt, cl, cu)
    # the 16-bit call still refuses a cache of another dtype, an FP8 one included
    with pytest.raises(ValueError, match="fp16 / bf16"):
        aule.flash_attention_mla_paged(q, kv, bt, cl, cu)
    # well-formed, on the CPU
    for ks in (None, 0.5, torch.tensor(0.5), torch.tensor([0.5])):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q, kv, bt, cl, cu, max_seqlen_q=2, return_lse=True, kv_scale=ks)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q[:3].to(torch.float16), kv.view(nb, bs, 1, 576), bt, cl, scale=192 ** -0.5)


def test_python_argument_errors_of_the_append():
    import torch
    T, nb, bs = 5, 4, 16
    c = torch.zeros(T, 512, dtype=torch.bfloat16)
    r = torch.zeros(T, 64, dtype=torch.bfloat16)
    kv = torch.zeros(nb, bs, 576, dtype=torch.bfloat16)
    kv8 = torch.zeros(nb, bs, 576, dtype=torch.float8_e4m3fn)
    slots = torch.arange(T)
    cos, sin, pos = torch.ones(100, 32), torch.zeros(100, 32), torch.arange(T)
    call = aule.mla_kv_append
    with pytest.raises(ValueError, match=r"expected c_kv \[T,512\]"):
        call(c[0], r, kv, slots)
    with pytest.raises(ValueError, match=r"expected c_kv \[T,512\]"):
        call(c, r.view(T, 2, 32), kv, slots)
    with pytest.raises(ValueError, match=r"expected c_kv \[T,512\]"):
        call(c, r, kv.view(nb, bs, 2, 288), slots)
    for a, b, k in ((c[:, :256], r, kv), (c, r[:, :32], kv), (c, r, kv[..., :512]), (r, c, kv)):
        with pytest.raises(ValueError, match="512 \\+ 64 = 576 wide"):
            call(a, b, k, slots)
    with pytest.raises(ValueError, match="c_kv has 5 tokens, k_pe 4"):
        call(c, r[:4], kv, slots)
    with pytest.raises(ValueError, match="share one of fp16 / bf16"):
        call(c, r.to(torch.float16), kv, slots)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(c.float(), r.float(), kv.float(), slots)
    for bad in (torch.float16, torch.float32, torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(ValueError, match="must be torch.float8_e4m3fn"):
            call(c, r, torch.zeros(nb, bs, 576).to(bad), slots)
    with pytest.raises(ValueError, match="kv_scale applies to a float8_e4m3fn cache only"):
        call(c, r, kv, slots, kv_scale=1.0)
    with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
        call(c, r, kv8, slots, kv_scale=torch.ones(2))
    with pytest.raises(ValueError, match="unknown rope_layout 'neox'"):
        call(c, r, kv, slots, rope_layout="neox")
    with pytest.raises(ValueError, match="kv_cache must be contiguous"):
        call(c, r, torch.zeros(nb, bs, 640, dtype=torch.bfloat16)[..., :576], slots)
    with pytest.raises(ValueError, match="block_size must be positive"):
        call(c, r, kv[:, :0], slots)
    with pytest.raises(ValueError, match="last dimension of c_kv must be contiguous"):
        call(torch.zeros(T, 1024, dtype=torch.bfloat16)[:, ::2], r, kv, slots)
    with pytest.raises(ValueError, match="k_pe: rows must be 16-byte aligned"):
        call(c, torch.zeros(T, 68, dtype=torch.bfloat16)[:, :64], kv, slots)
    with pytest.raises(ValueError, match="c_kv: rows must be 16-byte aligned"):
        call(torch.zeros(T, 580, dtype=torch.bfloat16)[:, 4:516], r, kv, slots)
    for bad in (slots[:4], slots.float(), slots.view(1, T), slots > 2):
        with pytest.raises(ValueError, match=r"slot_mapping must be an integer tensor of shape \[5\]"):
            call(c, r, kv, bad)
    with pytest.raises(ValueError, match="cos and sin are required"):
        call(c, r, kv, slots, cos=cos, positions=pos)
    with pytest.raises(ValueError, match="cos and sin are required"):
        call(c, r, kv, slots, sin=sin)
    with pytest.raises(ValueError, match="positions are required"):
        call(c, r, kv, slots, cos=cos, sin=sin)
    with pytest.raises(ValueError, match="cos and sin are required"):
        call(c, r, kv, slots, positions=pos)
    with pytest.raises(ValueError, match=r"positions must be an integer tensor of shape \[5\]"):
        call(c, r, kv, slots, cos=cos, sin=sin, positions=pos.float())
    with pytest.raises(ValueError, match=r"cos/sin must have shape \[..., 32\]"):
        call(c, r, kv, slots, cos=torch.ones(100, 64), sin=torch.ones(100, 64), positions=pos)
    # well-formed, on the CPU: both cache kinds, slices of one wider projection, the 3-d k_pe and the 4-d cache, both layouts
    fused = torch.zeros(T, 512 + 64 + 8, dtype=torch.bfloat16)
    for args, kw in (((c, r, kv, slots), {}), ((c, r, kv8, slots), dict(kv_scale=torch.tensor([0.25]))),
                     ((fused[:, :512], fused[:, 512:576], kv8, slots), dict(kv_scale=0.5, cos=cos, sin=sin, positions=pos, rope_layout="interleaved")),
                     ((c, r.view(T, 1, 64), kv.view(nb, bs, 1, 576), slots), dict(cos=cos, sin=sin, positions=pos))):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(*args, **kw)


def test_quantize_mla_cache_fp8_on_the_cpu():
    import torch
    g = torch.Generator().manual_seed(7)
    x = torch.randn(5, 16, 576, generator=g).to(torch.bfloat16)
    codes, scale = aule.quantize_mla_cache_fp8(x)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape and scale.shape == (1,) and scale.dtype == torch.float32
    assert float(scale) == float(x.float().abs().max() / 448)
    # round trip within half a code step: the spacing of e4m3 at |y| is 2^(max(floor(log2 |y|), -6) - 3)
    y = x.float() / scale
    step = torch.exp2(torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -6))) - 3)
    assert bool(((codes.float() - y).abs() <= step / 2).all())
    assert float(codes.float().abs().max()) == 448.0
    assert not bool(torch.isnan(codes.float()).any())
    # the 4-d spelling, and the formula of quantize_kv_cache_fp8 with one head
    c4, s4 = aule.quantize_mla_cache_fp8(x.view(5, 16, 1, 576))
    assert c4.shape == (5, 16, 1, 576) and torch.equal(c4.view(torch.uint8).view(5, 16, 576), codes.view(torch.uint8)) and torch.equal(s4, scale)
    ck, sk = aule.quantize_kv_cache_fp8(x.view(5, 16, 1, 576))
    assert torch.equal(ck.view(torch.uint8), c4.view(torch.uint8)) and torch.equal(sk, scale)
    # an all-zero cache: scale 1.0, codes 0
    codes, scale = aule.quantize_mla_cache_fp8(torch.zeros(2, 4, 576, dtype=torch.float16))
    assert float(scale) == 1.0 and bool((codes.view(torch.uint8) == 0).all())
    codes, scale = aule.quantize_mla_cache_fp8(torch.zeros(0, 4, 576, dtype=torch.float16))
    assert float(scale) == 1.0 and codes.shape == (0, 4, 576)
    # saturation instead of NaN: torch's cast of 465 is NaN, the helper's formula clamps first (a given scale: through the formula's pieces)
    assert bool(torch.isnan(torch.tensor([465.0]).to(torch.float8_e4m3fn).float()).all())
    big = torch.zeros(1, 2, 576)
    big[0, 0, 0], big[0, 1, 5] = 3.0e4, -3.0e4
    codes, scale = aule.quantize_mla_cache_fp8(big)
    assert sorted(codes.float().flatten().tolist())[0] == -448.0 and float(codes.float().max()) == 448.0
    with pytest.raises(ValueError, match="expected a latent cache"):
        aule.quantize_mla_cache_fp8(torch.zeros(2, 4, 512))
    with pytest.raises(ValueError, match="expected a latent cache"):
        aule.quantize_mla_cache_fp8(torch.zeros(2, 4, 2, 576))


def test_build_rule_names_the_new_sources():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    for src in ("fa_fwd_mla_paged_gfx950.hip", "fa_fwd_mla_paged_fp8_gfx950.hip", "mla_kv_append_gfx950.hip", "kv_append_gfx950.hip"):
        assert src in srcs and os.path.exists(os.path.join(CSRC, src)), src
    deps = {}
    for m in re.finditer(r"^((?:\$\(OBJDIR\)/\S+\.o ?)+): (.*)$", mk, re.M):
        for obj in m.group(1).split():
            deps.setdefault(obj, set()).update(m.group(2).split())
    for obj in ("fa_fwd_mla_paged_gfx950", "fa_fwd_mla_paged_fp8_gfx950"):
        assert {"fa_d256_common.h", "fa_paged_tile.h", "fa_mla_common.h"} <= deps["$(OBJDIR)/%s.o" % obj], obj
    for obj in ("kv_append_gfx950", "mla_kv_append_gfx950"):
        assert "kv_quant.h" in deps["$(OBJDIR)/%s.o" % obj], obj
    for h in ("fa_mla_common.h", "kv_quant.h"):
        assert os.path.exists(os.path.join(CSRC, h)), h
    # the quantiser is stated once
    for src in ("kv_append_gfx950.hip", "mla_kv_append_gfx950.hip"):
        text = open(os.path.join(CSRC, src)).read()
        assert '#include "kv_quant.h"' in text and "__builtin_amdgcn_cvt_pk_fp8_f32" not in text, src


def test_fp8_attention_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fp16 and bf16 of the FP8 attention kernel: no scratch, no VGPR or SGPR spill, the 16-bit kernel's 111 616 bytes of LDS; its name
    does not collide with the 16-bit kernel's, and the combine is not instantiated a second time"""
    res = resource_report("fa_fwd_mla_paged_fp8_gfx950.hip", tmp_path)
    assert not [n for n in res if "fa_fwd_mla_paged_kernel" in n or "fa_mla_combine_kernel" in n], list(res)
    ks = [n for n in res if "fa_mla_fp8_latent_kernel" in n]
    assert len(ks) == 2 and sum("Bf16Traits" in n for n in ks) == 1 and sum("F16Traits" in n for n in ks) == 1, ks
    for n in ks:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") == 111616, (n, r_)


def test_append_kernels_neither_spill_nor_use_scratch_nor_lds(tmp_path):
    """fp16 / bf16 x 16-bit / FP8 cache x no rotation / half / interleaved: twelve instances, no scratch, no spill, no LDS"""
    res = resource_report("mla_kv_append_gfx950.hip", tmp_path)
    ks = [n for n in res if "mla_kv_append_kernel" in n]
    assert len(ks) == 12, ks
    for n in ks:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size", 0) == 0, (n, r_)
