"""Variable-length packed batches without a GPU: the additive C-ABI (symbols, descriptor layouts, every answer the entries give before
they need a device, the workspace-size formula and its agreement with the launch), the argument errors of the torch layer, the build
rules (both files in the Makefile's source list, from which `make san` builds too; this file does not build the sanitizer library
itself -- tests/test_capi_sanitizers.py does, with the whole suite) and a resource audit of the kernels, compiled with the
Makefile's compiler and flags (no scratch, no spill, LDS below 45 KB)."""
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
FWD, BWD, SIZE = "aule_attention_varlen_forward_ex", "aule_attention_varlen_backward_ex", "aule_attention_varlen_backward_workspace_size"
FWD_PTRS = ("q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse")
BWD_PTRS = ("q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "dout", "dq", "dk", "dv", "workspace")

PROBLEM = dict(struct_size=0, dtype=4, batch=8, heads_q=12, heads_kv=16, head_dim=20, total_q=24, total_k=28, max_seqlen_q=32,
               max_seqlen_k=36, scale=40, causal=44, window_size=48, device=52, q_token_stride=56, k_token_stride=64, v_token_stride=72,
               stream=80, q=88, k=96, v=104, cu_seqlens_q=112, cu_seqlens_k=120)
FWD_LAYOUT = dict(PROBLEM, out=128, lse=136)
BWD_LAYOUT = dict(PROBLEM, out=128, lse=136, dout=144, dq=152, dk=160, dv=168, workspace=176, workspace_bytes=184)


def _ws_bytes(Tq, Hq):
    """delta [total_q, heads_q] fp32, on a 256-byte boundary"""
    return (Tq * Hq * 4 + 255) // 256 * 256


def _fill(kind="fwd", Tq=700, Tk=900, B=3, Hq=32, Hkv=8, D=128, max_sq=512, max_sk=640, dtype=2, causal=1, window=-1):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.VarlenDesc() if kind == "fwd" else _capi.VarlenBwdDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = dtype, B, Hq, Hkv, D
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = Tq, Tk, max_sq, max_sk
    d.causal, d.window_size = causal, window
    d.q_token_stride, d.k_token_stride, d.v_token_stride = Hq * D, Hkv * D, Hkv * D
    for n in (FWD_PTRS if kind == "fwd" else BWD_PTRS):
        setattr(d, n, 4096)
    if kind == "bwd":
        d.workspace_bytes = _ws_bytes(Tq, Hq)
    return d


def _entry(lib, kind):
    return lib.aule_attention_varlen_forward_ex if kind == "fwd" else lib.aule_attention_varlen_backward_ex


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, desc in ((FWD, "aule_varlen_desc"), (BWD, "aule_varlen_bwd_desc"), (SIZE, "aule_varlen_bwd_desc")):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, desc), header), name
        assert hasattr(lib, name) and name in bound, name
    assert bound[SIZE][1] is ctypes.c_uint64
    assert "flash_attention_varlen" in aule.__all__ and callable(aule.flash_attention_varlen)
    sig = inspect.signature(aule.flash_attention_varlen)
    assert list(sig.parameters) == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "causal", "scale",
                                    "window_size", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["max_seqlen_k"].default is None and p["causal"].default is True
    assert p["scale"].default is None and p["window_size"].default == -1 and p["return_lse"].default is False


@pytest.mark.parametrize("cls,struct,size,want", [(_capi.VarlenDesc, "aule_varlen_desc", 144, FWD_LAYOUT),
                                                 (_capi.VarlenBwdDesc, "aule_varlen_bwd_desc", 192, BWD_LAYOUT)], ids=["fwd", "bwd"])
def test_descriptor_layouts_match_the_header(cls, struct, size, want):
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(%s) = %d" % (struct, size) in header
    assert "sizeof(%s) == %d" % (struct, size) in capi
    assert ctypes.sizeof(cls) == size
    assert [n for n, _ in cls._fields_] == list(want)
    for name, off in want.items():
        assert getattr(cls, name).offset == off, name
    body = header.split("typedef struct %s {" % struct)[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 8
    for name, off in quoted:
        assert want[name] == int(off), name
    pinned = re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, capi)
    assert len(pinned) >= 8
    for name, off in pinned:
        assert want[name] == int(off), name
    # existing descriptors keep their sizes
    assert ctypes.sizeof(_capi.AttnDesc) == 112 and ctypes.sizeof(_capi.AttnBwdDesc) == 144 and ctypes.sizeof(_capi.PagedPrefillDesc) == 152


# (field, bad value, a piece of the reason) -- rules of the problem statement, both kinds
BAD_PROBLEM = [
    ("struct_size", 0, "struct_size"), ("struct_size", 8, "struct_size"), ("struct_size", 200, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"), ("dtype", -1, "fp16 or bf16"),
    ("head_dim", 256, "head_dim 256"), ("head_dim", 48, "head_dim 48"), ("head_dim", 0, "head_dim 0"),
    ("heads_kv", 5, "divisible"), ("heads_kv", 0, "divisible"),
    ("causal", 3, "unknown causal mode 3"), ("causal", -1, "unknown causal mode -1"),
    ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"), ("max_seqlen_k", 0, "max_seqlen_k must be at least 1"),
    ("q_token_stride", 32 * 128 - 8, "q_token_stride (4088) is smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", -4096, "smaller than a token"), ("q_token_stride", 32 * 128 + 4, "q_token_stride (4100) must be a multiple of 8"),
    ("k_token_stride", 8 * 128 - 8, "k_token_stride (1016) is smaller than a token"), ("k_token_stride", 8 * 128 + 2, "k_token_stride (1026) must be a multiple of 8"),
    ("v_token_stride", 0, "v_token_stride (0) is smaller than a token"), ("v_token_stride", 8 * 128 + 12, "v_token_stride (1036) must be a multiple of 8"),
    ("total_q", 1 << 30, "too large"), ("total_k", 1 << 30, "too large"), ("batch", 1 << 30, "too large"),
]
BAD_FWD = [
    ("q", None, "null tensor pointer"), ("k", None, "null tensor pointer"), ("v", None, "null tensor pointer"),
    ("out", None, "null tensor pointer"), ("cu_seqlens_q", None, "null cu_seqlens pointer"), ("cu_seqlens_k", None, "null cu_seqlens pointer"),
    ("q", 4096 + 8, "16-byte aligned"), ("k", 4097, "16-byte aligned"), ("v", 4096 + 4, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"),
]
BAD_BWD = BAD_FWD + [
    ("lse", None, "null tensor pointer"), ("dout", None, "null tensor pointer"), ("dq", None, "null tensor pointer"),
    ("dk", None, "null tensor pointer"), ("dv", None, "null tensor pointer"),
    ("dout", 4096 + 8, "16-byte aligned"), ("dq", 4096 + 8, "16-byte aligned"), ("dk", 4097, "16-byte aligned"), ("dv", 4096 + 2, "16-byte aligned"),
    ("workspace", 4096 + 8, "workspace must be 16-byte aligned"),
    ("workspace_bytes", _ws_bytes(700, 32) - 1, "workspace too small (89599 bytes, need 89600)"), ("workspace_bytes", 0, "workspace too small"),
]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD_PROBLEM + BAD_FWD, ids=_ids)
def test_forward_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library)."""
    lib = _capi.load()
    d = _fill("fwd")
    setattr(d, field, bad)
    assert lib.aule_attention_varlen_forward_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Variable-length attention failed: "), _error(lib)


@pytest.mark.parametrize("field,bad,needle", BAD_PROBLEM + BAD_BWD, ids=_ids)
def test_backward_refuses_each_bad_field(field, bad, needle):
    lib = _capi.load()
    d = _fill("bwd")
    setattr(d, field, bad)
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Variable-length backward failed: "), _error(lib)


@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_null_descriptor_and_packed_row_overflow(kind):
    lib = _capi.load()
    assert _entry(lib, kind)(None) == -3 and "struct_size" in _error(lib)
    # (total_q + 128) * (heads_q / heads_kv) must fit 32 bits: g = 8, the last total_q that fits and the first that does not
    last = 0x7fffffff // 8 - 128
    d = _fill(kind, Tq=last + 1, Hq=64, Hkv=8)
    assert _entry(lib, kind)(ctypes.byref(d)) == -3 and "32 bits" in _error(lib)
    if kind == "bwd":
        assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == 0
        d = _fill(kind, Tq=last, Hq=64, Hkv=8)
        assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == _ws_bytes(last, 64)


def test_nothing_to_do_returns_zero_without_a_launch():
    """forward: total_q = 0, batch = 0 or heads_q = 0; backward: batch = 0, heads_q = 0, or no query and no key row: 0, with null
    pointers, in any process.  A refused field is still refused."""
    lib = _capi.load()
    for kind, ptrs in (("fwd", FWD_PTRS), ("bwd", BWD_PTRS)):
        for fields in (("total_q",), ("batch",), ("heads_q",)):
            d = _fill(kind)
            for f in fields:
                setattr(d, f, 0)
            if kind == "bwd" and fields == ("total_q",):
                d.total_k = 0
            if fields == ("heads_q",):
                d.q_token_stride = 0
            for n in ptrs:
                setattr(d, n, None)
            assert _entry(lib, kind)(ctypes.byref(d)) == 0, (kind, fields)
            if kind == "bwd":
                d.workspace_bytes = 0
                assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == 0
        d = _fill(kind, Tq=0, Tk=0)
        d.head_dim = 256
        assert _entry(lib, kind)(ctypes.byref(d)) == -3
    # a backward without a query row still has the owned dk / dv rows to zero: it needs its key-side pointers and nothing else
    d = _fill("bwd", Tq=0)
    d.dk = None
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)
    # a forward without a key row writes zeros and -inf: k and v may be null, out may not
    d = _fill("fwd", Tk=0)
    d.k = d.v = None
    d.out = None
    assert lib.aule_attention_varlen_forward_ex(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entries_report_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_varlen_forward_ex(ctypes.byref(_fill("fwd"))) == -1
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(_fill("bwd"))) == -1
    d = _fill("bwd")
    d.workspace, d.workspace_bytes = None, 0     # no workspace: the library would allocate
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -1
    d = _fill("fwd", Tk=0)
    d.k = d.v = None
    assert lib.aule_attention_varlen_forward_ex(ctypes.byref(d)) == -1
    d = _fill("bwd", Tq=0)
    d.q = d.out = d.lse = d.dout = d.dq = d.workspace = None
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -1


@pytest.mark.parametrize("Tq,Hq,Hkv", [(1, 1, 1), (15, 4, 2), (16, 4, 4), (700, 32, 8), (33, 8, 1), (1 << 20, 64, 8)])
def test_workspace_size_is_delta(Tq, Hq, Hkv):
    """delta [total_q, heads_q] fp32 rounded up to 256 bytes, whatever the other fields say; no pointer is read"""
    lib = _capi.load()
    for D in (32, 64, 128):
        for causal in (0, 1, 2):
            d = _fill("bwd", Tq=Tq, Hq=Hq, Hkv=Hkv, D=D, causal=causal, window=17 if causal else -1)
            for n in BWD_PTRS:
                setattr(d, n, None)
            d.workspace_bytes = 0
            assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == _ws_bytes(Tq, Hq)
    assert lib.aule_attention_varlen_backward_workspace_size(None) == 0


@pytest.mark.parametrize("field,bad,needle", BAD_PROBLEM, ids=_ids)
def test_size_query_and_launch_give_the_same_verdict(field, bad, needle):
    """one checker: what the launch refuses on the problem statement the size query answers with 0, and the other way round"""
    lib = _capi.load()
    d = _fill("bwd")
    assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == _ws_bytes(700, 32)
    if not os.path.exists("/dev/kfd"):   # accepted: the device is the next thing it needs (with one, the dummy pointers must not be launched on)
        assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -1
    setattr(d, field, bad)
    assert lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d)) == 0
    assert lib.aule_attention_varlen_backward_ex(ctypes.byref(d)) == -3


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_varlen with CPU tensors: every rule is checked before a device is touched; a well-formed CPU
    call is an AuleError (no fallback)."""
    import torch
    Tq, Tk, Hq, Hkv, D = 10, 12, 8, 2, 64
    q = torch.zeros(Tq, Hq, D, dtype=torch.float16)
    k = torch.zeros(Tk, Hkv, D, dtype=torch.float16)
    cq = torch.tensor([0, 5, 10], dtype=torch.int32)
    ck = torch.tensor([0, 6, 12], dtype=torch.int32)
    call = aule.flash_attention_varlen
    # shapes
    with pytest.raises(ValueError, match=r"expected q \[total_q, heads_q, head_dim\]"):
        call(q.reshape(2, 5, Hq, D), k, k, cq, ck)
    with pytest.raises(ValueError, match=r"expected q \[total_q, heads_q, head_dim\]"):
        call(q, k, k[:4], cq, ck)
    with pytest.raises(ValueError, match=r"expected q \[total_q, heads_q, head_dim\]"):
        call(q, k[0], k[0], cq, ck)
    with pytest.raises(ValueError, match="head_dim mismatch"):
        call(q, k[..., :32], k[..., :32], cq, ck)
    with pytest.raises(ValueError, match="divisible"):
        call(q, torch.zeros(Tk, 3, D, dtype=torch.float16), torch.zeros(Tk, 3, D, dtype=torch.float16), cq, ck)
    # dtypes and head dims that are not built
    with pytest.raises(ValueError, match="not built"):
        call(q.float(), k.float(), k.float(), cq, ck)
    with pytest.raises(ValueError, match="share one dtype"):
        call(q, k.to(torch.bfloat16), k, cq, ck)
    with pytest.raises(ValueError, match="not built"):
        call(torch.zeros(Tq, Hq, 256, dtype=torch.float16), torch.zeros(Tk, Hkv, 256, dtype=torch.float16),
             torch.zeros(Tk, Hkv, 256, dtype=torch.float16), cq, ck)
    with pytest.raises(ValueError, match="not built"):
        call(torch.zeros(Tq, Hq, 136, dtype=torch.bfloat16), torch.zeros(Tk, Hkv, 136, dtype=torch.bfloat16),
             torch.zeros(Tk, Hkv, 136, dtype=torch.bfloat16), cq, ck)
    # offsets
    for bad in (cq.view(1, 3), [0, 5, 10], cq[:0]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] tensor"):
            call(q, k, k, bad, ck)
    with pytest.raises(ValueError, match=r"cu_seqlens_k must be a \[batch \+ 1\] tensor"):
        call(q, k, k, cq, None)
    with pytest.raises(ValueError, match=r"must both be \[batch \+ 1\]"):
        call(q, k, k, cq, ck[:2])
    for bad in (cq.long(), cq.float(), cq.to(torch.int16)):
        with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
            call(q, k, k, bad, ck)
        with pytest.raises(ValueError, match="cu_seqlens_k must be int32"):
            call(q, k, k, cq, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, k, k, cq, ck, max_seqlen_q=bad)
        with pytest.raises(ValueError, match="max_seqlen_k must be a positive int"):
            call(q, k, k, cq, ck, max_seqlen_k=bad)
    with pytest.raises(ValueError, match="causal must be"):
        call(q, k, k, cq, ck, causal="diagonal")
    # stride alignment: a token stride or a storage offset that is no multiple of 8 elements, in each of the three
    wide_q = torch.zeros(Tq, Hq * D + 4, dtype=torch.float16)[:, :Hq * D].view(Tq, Hq, D)
    wide_k = torch.zeros(Tk, Hkv * D + 4, dtype=torch.float16)[:, :Hkv * D].view(Tk, Hkv, D)
    shifted_k = torch.zeros(Tk * Hkv * D + 4, dtype=torch.float16)[4:].view(Tk, Hkv, D)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        call(wide_q, k, k, cq, ck)
    with pytest.raises(ValueError, match="k's token stride.*multiples of 8 elements"):
        call(q, wide_k, k, cq, ck)
    with pytest.raises(ValueError, match="v's token stride.*multiples of 8 elements"):
        call(q, k, wide_k, cq, ck)
    with pytest.raises(ValueError, match="k's token stride.*multiples of 8 elements"):
        call(q, shifted_k, k, cq, ck)
    # well-formed, on the CPU: the three slices of a fused projection included, and a head_dim that is padded
    fused = torch.zeros(Tq, Hq + 2 * Hkv, D, dtype=torch.float16)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], cq, cq, max_seqlen_q=5, max_seqlen_k=5)
    for causal in (False, True, "bottom-right"):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q, k, k, cq, ck, causal=causal, window_size=3, return_lse=True)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q[..., :40], k[..., :40], k[..., :40], cq, ck)


def test_build_rules_name_the_new_sources():
    """csrc/Makefile: both files in SRCS (so `make`, `make dbg` and `make san` compile them) with their header dependencies"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fa_fwd_varlen_gfx950.hip" in srcs and "fa_bwd_varlen_gfx950.hip" in srcs
    dep = re.search(r"^\$\(OBJDIR\)/fa_fwd_varlen_gfx950\.o \$\(OBJDIR\)/fa_bwd_varlen_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert {"fa_varlen_common.h", "fa_tile_attention.h", "fa_paged_tile.h", "fa_d256_common.h"} <= set(dep)
    for f in ("fa_varlen_common.h", "fa_tile_attention.h", "fa_fwd_varlen_gfx950.hip", "fa_bwd_varlen_gfx950.hip"):
        assert os.path.exists(os.path.join(CSRC, f))


@pytest.mark.parametrize("src,kernels", [("fa_fwd_varlen_gfx950.hip", {"fa_fwd_varlen_kernel": 6}),
                                         ("fa_bwd_varlen_gfx950.hip", {"fa_bwd_varlen_delta_kernel": 2, "fa_bwd_varlen_dq_kernel": 6,
                                                                       "fa_bwd_varlen_dkdv_kernel": 6})], ids=["fwd", "bwd"])
def test_varlen_kernels_neither_spill_nor_use_scratch(src, kernels, tmp_path):
    """fp16, bf16 x D 32, 64, 128 of every kernel: no scratch, no VGPR or SGPR spill, LDS below 45 KB (DESIGN.md 3.8 states the budget)"""
    res = resource_report(src, tmp_path)
    for name, count in kernels.items():
        ks = [n for n in res if name in n]
        assert len(ks) == count and sum("Bf16Traits" in n for n in ks) == count // 2, (name, ks)
        for n in ks:
            r_ = res[n]
            assert r_.get("ScratchSize") == 0, (n, r_)
            assert r_.get("VGPRs Spill") == 0, (n, r_)
            assert r_.get("SGPRs Spill") == 0, (n, r_)
            assert r_.get("LDS Size") < 45 * 1024, (n, r_)
