"""Attention sinks without a GPU: the six additive C-ABI symbols, the four descriptor layouts (each its twin field for field, the new
pointers appended), every answer the entries give before they need a device, the workspace-size rule of the backward, the three
Python signatures and the argument errors of the sink logits."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")

# entry -> (descriptor struct, ctypes class, result type)
ENTRIES = {
    "aule_attention_varlen_sink_forward_ex": ("aule_varlen_sink_desc", _capi.VarlenSinkDesc, ctypes.c_int32),
    "aule_attention_varlen_sink_backward_ex": ("aule_varlen_sink_bwd_desc", _capi.VarlenSinkBwdDesc, ctypes.c_int32),
    "aule_attention_varlen_sink_backward_workspace_size": ("aule_varlen_sink_bwd_desc", _capi.VarlenSinkBwdDesc, ctypes.c_uint64),
    "aule_attention_paged_prefill_sink_ex": ("aule_paged_prefill_sink_desc", _capi.PagedPrefillSinkDesc, ctypes.c_int32),
    "aule_attention_paged_query_sink_ex": ("aule_paged_query_sink_desc", _capi.PagedQuerySinkDesc, ctypes.c_int32),
    "aule_attention_paged_query_sink_workspace_size": ("aule_paged_query_sink_desc", _capi.PagedQuerySinkDesc, ctypes.c_uint64),
}

# kind -> (struct, class, size, twin struct, twin class, {appended field: offset})
LAYOUTS = {
    "varlen": ("aule_varlen_sink_desc", _capi.VarlenSinkDesc, 152, "aule_varlen_desc", _capi.VarlenDesc, {"sinks": 144}),
    "varlen_bwd": ("aule_varlen_sink_bwd_desc", _capi.VarlenSinkBwdDesc, 208, "aule_varlen_bwd_desc", _capi.VarlenBwdDesc,
                   {"sinks": 192, "dsinks": 200}),
    "prefill": ("aule_paged_prefill_sink_desc", _capi.PagedPrefillSinkDesc, 160, "aule_paged_prefill_desc", _capi.PagedPrefillDesc,
                {"sinks": 152}),
    "query": ("aule_paged_query_sink_desc", _capi.PagedQuerySinkDesc, 160, "aule_paged_query_desc", _capi.PagedQueryDesc, {"sinks": 152}),
}


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, (struct, cls, restype) in ENTRIES.items():
        assert re.search(r"\b%s\s*\(const %s\*" % (name, struct), header), name
        assert hasattr(lib, name) and name in bound, name
        assert bound[name][1] is restype and bound[name][2][0]._type_ is cls, name


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_descriptor_layouts_repeat_the_twin_and_append(kind):
    """size, field order, the twin's offsets through the whole prefix, the appended pointers; the same numbers in the header's text
    and in aule_capi.cpp's static_asserts"""
    struct, cls, size, twin_struct, twin, more = LAYOUTS[kind]
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(%s) = %d" % (struct, size) in header
    assert "sizeof(%s) == %d" % (struct, size) in capi
    assert ctypes.sizeof(cls) == size == ctypes.sizeof(twin) + 8 * len(more)
    names = [n for n, _ in cls._fields_]
    assert names == [n for n, _ in twin._fields_] + list(more)
    for n, t in twin._fields_:
        assert getattr(cls, n).offset == getattr(twin, n).offset and getattr(cls, n).size == getattr(twin, n).size, n
    for n, off in more.items():
        assert getattr(cls, n).offset == off, n
        assert "offsetof(%s, %s) == %d" % (struct, n, off) in capi, n
    assert "offsetof(%s, sinks) == sizeof(%s)" % (struct, twin_struct) in capi
    # the header: the same fields in the same order, and every offset it quotes
    body = header.split("typedef struct %s {" % struct)[1].split("} %s;" % struct)[0]
    declared = [n for line in re.sub(r"/\*.*?\*/", "", body).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert declared == names, declared
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 4 and set(more) <= {n for n, _ in quoted}
    for n, off in quoted:
        assert getattr(cls, n).offset == int(off), n
    # the twins keep their sizes
    assert [ctypes.sizeof(c) for c in (_capi.VarlenDesc, _capi.VarlenBwdDesc, _capi.PagedPrefillDesc, _capi.PagedQueryDesc)] == [144, 192, 152, 152]


# ---- well-formed descriptors whose pointers are aligned non-null dummies: only ever handed to calls that answer before a launch

def _varlen(kind, Tq=700, Tk=900, B=3, Hq=32, Hkv=8, D=128, max_sq=512, max_sk=640):
    d = _capi.VarlenSinkDesc() if kind == "varlen" else _capi.VarlenSinkBwdDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, B, Hq, Hkv, D
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = Tq, Tk, max_sq, max_sk
    d.causal, d.window_size = 1, -1
    d.q_token_stride, d.k_token_stride, d.v_token_stride = Hq * D, Hkv * D, Hkv * D
    ptrs = ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "sinks"]
    if kind == "varlen_bwd":
        ptrs += ["dout", "dq", "dk", "dv", "workspace", "dsinks"]
        d.workspace_bytes = _bwd_ws(Tq, Hq, B, max_sq)
    for n in ptrs:
        setattr(d, n, 4096)
    return d


def _paged(kind, B=3, Hq=8, Hkv=2, D=64, T=40):
    d = _capi.PagedPrefillSinkDesc() if kind == "prefill" else _capi.PagedQuerySinkDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, 0, B, Hq, Hkv, D
    d.block_size, d.max_blocks, d.window_size = 16, 8, -1
    ptrs = ["q", "k_cache", "v_cache", "block_tables", "context_lens", "out", "lse", "sinks"]
    if kind == "prefill":
        d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, 20, Hq * D
        ptrs.append("cu_seqlens_q")
    else:
        d.seq_q = 5
    for n in ptrs:
        setattr(d, n, 4096)
    return d


def _bwd_ws(Tq, Hq, B, max_sq):
    """delta [total_q, heads_q] fp32 on a 256-byte boundary, then the partials of the dsinks reduction:
    [batch][ceil(min(max_seqlen_q, total_q) / 256)][heads_q] fp32, on a 256-byte boundary too"""
    delta = (Tq * Hq * 4 + 255) // 256 * 256
    chunks = (min(max_sq, Tq) + 255) // 256
    return delta + (B * chunks * Hq * 4 + 255) // 256 * 256


FILL = {"varlen": _varlen, "varlen_bwd": _varlen, "prefill": _paged, "query": _paged}
LAUNCH = {"varlen": "aule_attention_varlen_sink_forward_ex", "varlen_bwd": "aule_attention_varlen_sink_backward_ex",
          "prefill": "aule_attention_paged_prefill_sink_ex", "query": "aule_attention_paged_query_sink_ex"}
PREFIX = {"varlen": "Variable-length sink attention failed: ", "varlen_bwd": "Variable-length sink backward failed: ",
          "prefill": "Paged prefill sink attention failed: ", "query": "Paged query sink attention failed: "}


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_null_sinks_and_wrong_sizes_are_refused_before_the_device(kind):
    """-3 with a reason, in a process that never called aule_init()"""
    lib = _capi.load()
    entry = getattr(lib, LAUNCH[kind])
    assert entry(None) == -3 and "struct_size" in _error(lib)
    d = FILL[kind](kind)
    d.sinks = None
    assert entry(ctypes.byref(d)) == -3
    assert _error(lib).startswith(PREFIX[kind]) and "null sinks pointer" in _error(lib), _error(lib)
    if kind == "varlen_bwd":
        d = FILL[kind](kind)
        d.dsinks = None
        assert entry(ctypes.byref(d)) == -3 and "null dsinks pointer" in _error(lib), _error(lib)
    twin_size = ctypes.sizeof(LAYOUTS[kind][4])
    for bad in (0, 8, twin_size, ctypes.sizeof(d) + 8):       # the twin's own size included: a sinkless descriptor is not read as one
        d = FILL[kind](kind)
        d.struct_size = bad
        assert entry(ctypes.byref(d)) == -3 and "struct_size" in _error(lib), (bad, _error(lib))
    # the twin's rules hold through the prefix: one of each family
    d = FILL[kind](kind)
    d.head_dim = 48
    assert entry(ctypes.byref(d)) == -3 and "head_dim 48" in _error(lib)
    d = FILL[kind](kind)
    d.heads_kv = 3
    assert entry(ctypes.byref(d)) == -3 and "divisible" in _error(lib)
    d = FILL[kind](kind)
    d.q = None
    assert entry(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_nothing_to_do_returns_zero_without_a_launch(kind):
    """the twin's rule, with every pointer null, in any process"""
    lib = _capi.load()
    entry = getattr(lib, LAUNCH[kind])
    empties = {"varlen": ("total_q", "batch", "heads_q"), "varlen_bwd": ("batch", "heads_q"), "prefill": ("total_tokens", "batch", "heads_q"),
               "query": ("batch", "heads_q")}[kind]
    for field in empties:
        d = FILL[kind](kind)
        setattr(d, field, 0)
        if field == "heads_q" and kind != "query":
            d.q_token_stride = 0
        for n, t in d._fields_:
            if t is ctypes.c_void_p and n != "stream":
                setattr(d, n, None)
        assert entry(ctypes.byref(d)) == 0, (kind, field, _error(lib))
    if kind == "varlen_bwd":
        d = _varlen(kind, Tq=0, Tk=0)
        d.sinks = d.dsinks = None
        assert entry(ctypes.byref(d)) == 0
        assert lib.aule_attention_varlen_sink_backward_workspace_size(ctypes.byref(d)) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_entries_report_uninitialised_without_a_gpu(kind):
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert getattr(lib, LAUNCH[kind])(ctypes.byref(FILL[kind](kind))) == -1


@pytest.mark.parametrize("Tq,Hq,B,max_sq", [(1, 1, 1, 1), (700, 32, 3, 512), (700, 32, 3, 5000), (257, 64, 2, 257), (4096 * 8, 64, 8, 4096)])
def test_backward_workspace_is_the_sinkless_backwards_plus_the_partials(Tq, Hq, B, max_sq):
    lib = _capi.load()
    d = _varlen("varlen_bwd", Tq=Tq, Hq=Hq, Hkv=1, B=B, max_sq=max_sq, D=64)
    for n, t in d._fields_:
        if t is ctypes.c_void_p:
            setattr(d, n, None)               # host logic only: no pointer is read
    d.workspace_bytes = 0
    twin = _capi.VarlenBwdDesc()
    ctypes.memmove(ctypes.byref(twin), ctypes.byref(d), ctypes.sizeof(twin))
    twin.struct_size = ctypes.sizeof(twin)
    base = int(lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(twin)))
    got = int(lib.aule_attention_varlen_sink_backward_workspace_size(ctypes.byref(d)))
    assert base == (Tq * Hq * 4 + 255) // 256 * 256 and got == _bwd_ws(Tq, Hq, B, max_sq) and got > base
    # a workspace that is given but one byte short is refused, the exact size is accepted (the next thing it needs is the device)
    d = _varlen("varlen_bwd", Tq=Tq, Hq=Hq, Hkv=1, B=B, max_sq=max_sq, D=64)
    d.workspace_bytes = got - 1
    assert lib.aule_attention_varlen_sink_backward_ex(ctypes.byref(d)) == -3 and "workspace too small" in _error(lib)
    assert lib.aule_attention_varlen_sink_backward_workspace_size(None) == 0
    d.head_dim = 48
    assert lib.aule_attention_varlen_sink_backward_workspace_size(ctypes.byref(d)) == 0


def test_query_workspace_is_the_sinkless_querys():
    lib = _capi.load()
    for B, Hq, Hkv, D, Sq, blocks in ((3, 8, 2, 64, 5, 8), (64, 64, 8, 64, 1, 512), (2, 4, 4, 128, 64, 40)):
        d = _paged("query", B=B, Hq=Hq, Hkv=Hkv, D=D)
        d.seq_q, d.max_blocks = Sq, blocks
        twin = _capi.PagedQueryDesc()
        ctypes.memmove(ctypes.byref(twin), ctypes.byref(d), ctypes.sizeof(twin))
        twin.struct_size = ctypes.sizeof(twin)
        want = int(lib.aule_attention_paged_query_workspace_size(ctypes.byref(twin)))
        assert want > 0 and int(lib.aule_attention_paged_query_sink_workspace_size(ctypes.byref(d))) == want
    d.seq_q = 65
    assert lib.aule_attention_paged_query_sink_workspace_size(ctypes.byref(d)) == 0
    assert lib.aule_attention_paged_query_sink_ex(ctypes.byref(d)) == -3 and "seq_q 65" in _error(lib)


def test_python_signatures_and_defaults():
    for name in ("flash_attention_varlen_sinks", "flash_attention_paged_prefill_sinks", "flash_attention_paged_query_sinks"):
        assert name in aule.__all__ and callable(getattr(aule, name)), name
    sig = inspect.signature(aule.flash_attention_varlen_sinks)
    assert list(sig.parameters) == ["q", "k", "v", "sinks", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "causal", "scale",
                                    "window_size", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["max_seqlen_k"].default is None and p["causal"].default is True
    assert p["scale"].default is None and p["window_size"].default == -1 and p["return_lse"].default is False
    sig = inspect.signature(aule.flash_attention_paged_prefill_sinks)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "sinks", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale",
                                    "window_size", "k_scale", "v_scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["scale"].default is None and p["window_size"].default == -1
    assert p["k_scale"].default is None and p["v_scale"].default is None and p["return_lse"].default is False
    sig = inspect.signature(aule.flash_attention_paged_query_sinks)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "sinks", "block_tables", "context_lens", "scale", "window_size", "k_scale",
                                    "v_scale", "return_lse"]
    p = sig.parameters
    assert p["scale"].default is None and p["window_size"].default == -1 and p["k_scale"].default is None
    assert p["v_scale"].default is None and p["return_lse"].default is False
    # the twins keep theirs
    assert "sinks" not in inspect.signature(aule.flash_attention_varlen).parameters
    assert "sinks" not in inspect.signature(aule.flash_attention_paged_prefill).parameters
    assert "sinks" not in inspect.signature(aule.flash_attention_paged_query).parameters


def test_sinks_argument_errors_are_value_errors_before_any_launch():
    """CPU tensors: wrong shape, dtype or device of sinks is a ValueError in all three calls; the twin's rules still come first; a
    well-formed CPU call is an AuleError (no fallback)."""
    import torch
    Hq, Hkv, D = 8, 2, 64
    q = torch.zeros(10, Hq, D, dtype=torch.float16)
    k = torch.zeros(12, Hkv, D, dtype=torch.float16)
    cq = torch.tensor([0, 5, 10], dtype=torch.int32)
    ck = torch.tensor([0, 6, 12], dtype=torch.int32)
    cache = torch.zeros(4, 16, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(2, 2, dtype=torch.int32)
    cl = torch.tensor([7, 9], dtype=torch.int32)
    q4 = torch.zeros(2, Hq, 3, D, dtype=torch.float16)
    good = torch.zeros(Hq)
    calls = {
        "varlen": lambda s: aule.flash_attention_varlen_sinks(q, k, k, s, cq, ck),
        "prefill": lambda s: aule.flash_attention_paged_prefill_sinks(q, cache, cache, s, bt, cl, cq),
        "query": lambda s: aule.flash_attention_paged_query_sinks(q4, cache, cache, s, bt, cl),
    }
    for name, call in calls.items():
        for bad in (torch.zeros(Hq + 1), torch.zeros(Hkv), torch.zeros(1, Hq), torch.zeros(()), [0.0] * Hq, None, 0.5):
            with pytest.raises(ValueError, match=r"sinks must be a \[heads_q\]"):
                call(bad)
        for bad in (good.double(), good.to(torch.bfloat16), good.to(torch.int32)):      # (q is fp16: bf16 is neither fp32 nor q's dtype)
            with pytest.raises(ValueError, match="sinks must be float32 or of q's dtype"):
                call(bad)
        with pytest.raises(ValueError, match="sinks must be on q's device"):
            call(torch.zeros(Hq, device="meta"))
        for ok in (good, good.half(), torch.full((Hq,), float("-inf"))):
            with pytest.raises(aule.AuleError, match="no CPU fallback"):
                call(ok)
    # the twin's own rules are still checked, and first
    with pytest.raises(ValueError, match="divisible"):
        aule.flash_attention_varlen_sinks(q, torch.zeros(12, 3, D, dtype=torch.float16), torch.zeros(12, 3, D, dtype=torch.float16), good, cq, ck)
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        aule.flash_attention_varlen_sinks(q, k, k, good, cq.long(), ck)
    with pytest.raises(ValueError, match="1 to 64 query tokens"):
        aule.flash_attention_paged_query_sinks(torch.zeros(2, Hq, 65, D, dtype=torch.float16), cache, cache, good, bt, cl)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\]"):
        aule.flash_attention_paged_prefill_sinks(q, cache, cache, good, bt, cl, cq[:2])


def test_build_rules_name_the_new_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fa_bwd_sinks_gfx950.hip" in srcs and os.path.exists(os.path.join(CSRC, "fa_bwd_sinks_gfx950.hip"))
    dep = re.search(r"^\$\(OBJDIR\)/fa_bwd_sinks_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert "fa_varlen_common.h" in dep
    src = open(os.path.join(CSRC, "fa_bwd_sinks_gfx950.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)          # a fixed summation order: no atomics in the code
