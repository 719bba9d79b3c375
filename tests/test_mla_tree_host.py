"""Tree masks over the latent cache without a GPU: the additive C-ABI (symbols, the descriptor's layout against its FP8 twin, every
answer the entry gives before it needs a device, the agreement of the size query with the twin's), the signature and argument errors
of the torch layer, the build rule, the new unit's text and a resource audit of its four kernels compiled with the Makefile's
compiler and flags against profiles/mla_tree_resources.txt."""
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
UNIT = "fa_fwd_mla_verify_gfx950.hip"
ENTRY, SIZE = "aule_attention_mla_paged_tree_ex", "aule_attention_mla_paged_tree_workspace_size"
PREFIX = "Paged MLA tree attention failed: "
NEW_FIELDS = dict(tree_mask=144, cache_dtype=152, reserved=156)
PTRS = ("q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "lse", "tree_mask")
FIGURES = ("VGPRs", "AGPRs", "ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size")
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _fill(T=24, B=8, Hq=16, bs=64, max_blocks=32, max_sq=3, dtype=2, fp8=False, cls=None):
    """a well-formed descriptor whose pointers are aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = (cls or _capi.MlaPagedTreeDesc)()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = dtype, B, Hq, 576, 512
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = bs, max_blocks, T, max_sq
    d.q_token_stride = Hq * 576
    for n in PTRS:
        if hasattr(d, n):
            setattr(d, n, 4096)
    if hasattr(d, "cache_dtype"):
        d.cache_dtype = int(fp8)
        if fp8:
            d.kv_scale = 4096
    return d


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, restype in ((ENTRY, ctypes.c_int32), (SIZE, ctypes.c_uint64)):
        assert re.search(r"\b%s\s*\(const aule_mla_paged_tree_desc\*" % name, header), name
        assert hasattr(lib, name) and name in bound, name
        assert bound[name][1] is restype and bound[name][2][0]._type_ is _capi.MlaPagedTreeDesc, name
    # the documents no longer list MLA trees as not built
    assert "the cascade and the MLA entries" not in header
    for f in (aule.flash_attention_paged_query_tree, aule.flash_attention_paged_prefill_tree):
        assert "flash_attention_mla_paged_tree" in f.__doc__ and "the cascade and the MLA entries" not in f.__doc__


def test_descriptor_layout_repeats_the_fp8_twin_and_appends_three_fields():
    """size 160, the twin's offsets and sizes through the whole prefix (so through offset 143), then tree_mask, cache_dtype and the
    padding; the same numbers in the header's text and in aule_capi.cpp's static_assert"""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    cls, twin = _capi.MlaPagedTreeDesc, _capi.MlaPagedFp8Desc
    assert "sizeof(aule_mla_paged_tree_desc) = 160" in header and "sizeof(aule_mla_paged_tree_desc) == 160" in capi
    assert ctypes.sizeof(cls) == 160 and ctypes.sizeof(twin) == 144
    assert [n for n, _ in cls._fields_] == [n for n, _ in twin._fields_] + list(NEW_FIELDS)
    for n, _ in twin._fields_:
        assert (getattr(cls, n).offset, getattr(cls, n).size) == (getattr(twin, n).offset, getattr(twin, n).size), n
    for n, off in NEW_FIELDS.items():
        assert getattr(cls, n).offset == off, n
        assert "offsetof(aule_mla_paged_tree_desc, %s) == %d" % (n, off) in capi, n
    assert cls.tree_mask.size == 8 and cls.cache_dtype.size == 4 and cls.kv_scale.offset == 136
    assert "offsetof(aule_mla_paged_tree_desc, tree_mask) == sizeof(aule_mla_paged_fp8_desc)" in capi
    # every field of the prefix is pinned against the twin
    same = set(re.findall(r"AULE_MLA_TREE_SAME\((\w+)\)", capi.split("#define AULE_MLA_TREE_SAME")[1].split("#undef AULE_MLA_TREE_SAME")[0]))
    assert same == {n for n, _ in twin._fields_} - {"struct_size"}
    # the header: the same fields in the same order, every offset it quotes, an int64 word type
    body = header.split("typedef struct aule_mla_paged_tree_desc {")[1].split("} aule_mla_paged_tree_desc;")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert [n for n, _ in quoted] == [n for n, _ in cls._fields_][1:]
    for n, off in quoted:
        assert getattr(cls, n).offset == int(off), n
    assert "const int64_t* tree_mask;" in body and "int32_t cache_dtype;" in body


# (field, bad value, a piece of the reason): the twin's table of bad fields
BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 136, "struct_size"), ("struct_size", 144, "struct_size"), ("struct_size", 168, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("qk_dim", 512, "qk_dim 512"), ("v_dim", 576, "v_dim 576"),
    ("block_size", 0, "bad block_size"), ("max_blocks", 0, "bad block_size"), ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("q_token_stride", 16 * 576 - 8, "q_token_stride (9208) is smaller than a token"),
    ("q_token_stride", 16 * 576 + 4, "q_token_stride (9220) must be a multiple of 8"),
    ("total_tokens", 1 << 30, "too large"), ("batch", 1 << 30, "too large"),
    ("cache_dtype", 2, "cache_dtype 2 must be"), ("cache_dtype", -1, "cache_dtype -1 must be"),
    ("cu_seqlens_q", None, "null cu_seqlens_q (a tree of one node per sequence is the decode call"),
]
BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "kv_cache", "block_tables", "context_lens", "out")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("kv_cache", 4097, "16-byte aligned"),
    ("tree_mask", None, "null tree_mask pointer"), ("tree_mask", 4096 + 4, "tree_mask must be 8-byte aligned"),
    ("kv_scale", 4096, "kv_scale applies to an FP8 cache only")]


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_POINTER, ids=_ids)
def test_launch_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason with the entry's own prefix, before the device is needed (so also in a process that never initialised the library)"""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith(PREFIX), _error(lib)


def test_fp8_scale_rules_and_a_null_descriptor():
    lib = _capi.load()
    d = _fill(fp8=True)
    d.kv_scale = None
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == -3 and "null kv_scale" in _error(lib)
    d.kv_scale = 4098
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == -3 and "kv_scale must be 4-byte aligned" in _error(lib)
    assert lib.aule_attention_mla_paged_tree_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_mla_paged_tree_workspace_size(None) == 0
    # each entry refuses the other kinds' sizes
    d = _fill()
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.cast(ctypes.byref(d), ctypes.POINTER(_capi.MlaPagedFp8Desc))) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_mla_paged_ex(ctypes.cast(ctypes.byref(d), ctypes.POINTER(_capi.MlaPagedDesc))) == -3 and "struct_size" in _error(lib)


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE, ids=_ids)
def test_size_query_refuses_what_the_launch_refuses_on_the_shape(field, bad, needle):
    lib = _capi.load()
    d = _fill(T=2, B=1, max_sq=2)
    assert lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d)) > 0
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d)) == 0
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == -3


def test_size_query_equals_the_twins_and_reads_no_pointer():
    lib = _capi.load()
    seen = set()
    for B in (1, 3, 8, 64):
        for Hq in (5, 16, 24, 128):
            for sq in (1, 5, 33, 64, 65):
                for cap in (128, 2048, 131072):
                    for fp8 in (False, True):
                        kw = dict(T=B * sq + 3, B=B, Hq=Hq, bs=64, max_blocks=cap // 64, max_sq=sq)
                        d, d16, d8 = _fill(fp8=fp8, **kw), _fill(cls=_capi.MlaPagedDesc, **kw), _fill(cls=_capi.MlaPagedFp8Desc, **kw)
                        a = lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d))
                        assert a == lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d16)), kw
                        assert a == lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d8)), kw
                        for n in PTRS + ("kv_scale", "workspace"):
                            if n != "cu_seqlens_q":   # (null offsets are a statement about the problem, and refused here)
                                setattr(d, n, None)
                        assert lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d)) == a, kw
                        seen.add(a > 0)
    assert seen == {True, False}


def test_nothing_to_do_returns_zero_without_a_launch():
    lib = _capi.load()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill()
        setattr(d, field, 0)
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == 0, field
        assert lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d)) == 0
        d.qk_dim = 512
        assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == -3       # a refused field is still refused


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(_fill())) == -1
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(_fill(fp8=True, T=2, B=1, max_sq=2))) == -1


def test_python_signature_and_defaults():
    assert "flash_attention_mla_paged_tree" in aule.__all__ and callable(aule.flash_attention_mla_paged_tree)
    sig = inspect.signature(aule.flash_attention_mla_paged_tree)
    assert list(sig.parameters) == ["q", "kv_cache", "tree_mask", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale",
                                    "return_lse", "kv_scale"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["scale"].default is None and p["kv_scale"].default is None and p["return_lse"].default is False
    assert p["cu_seqlens_q"].default is inspect.Parameter.empty and p["tree_mask"].default is inspect.Parameter.empty
    doc = " ".join(aule.flash_attention_mla_paged_tree.__doc__.split())
    for phrase in ("Out of scope", "more than 64 tree tokens", "cascade", "backward", "mla_indexer", "filter the lists"):
        assert phrase in doc, phrase
    # the twins keep their signatures
    assert "tree_mask" not in inspect.signature(aule.flash_attention_mla_paged).parameters
    assert "tree_mask" not in inspect.signature(aule.flash_attention_mla_paged_fp8).parameters


def test_python_argument_errors_are_value_errors_before_the_device():
    import torch
    T, B, Hq, bs, nb = 6, 3, 16, 16, 12
    q = torch.zeros(T, Hq, 576, dtype=torch.bfloat16)
    kv = torch.zeros(nb, bs, 576, dtype=torch.bfloat16)
    kv8 = kv.to(torch.float8_e4m3fn)
    words = torch.zeros(T, dtype=torch.int64)
    bt = torch.zeros(B, 4, dtype=torch.int32)
    cl = torch.tensor([5, 9, 20], dtype=torch.int32)
    cu = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    call = aule.flash_attention_mla_paged_tree
    for bad in (torch.zeros(T, 1, dtype=torch.int64), torch.zeros(T + 1, dtype=torch.int64), torch.zeros((), dtype=torch.int64), [0] * T, None, 7):
        with pytest.raises(ValueError, match=r"tree_mask must be a"):
            call(q, kv, bad, bt, cl, cu)
    for bad in (words.int(), words.double(), words.bool()):
        with pytest.raises(ValueError, match="tree_mask must be int64"):
            call(q, kv, bad, bt, cl, cu)
    with pytest.raises(ValueError, match="tree_mask must be contiguous"):
        call(q, kv, torch.zeros(2 * T, dtype=torch.int64)[::2], bt, cl, cu)
    with pytest.raises(ValueError, match="tree_mask must be on q's device"):
        call(q, kv, torch.zeros(T, dtype=torch.int64, device="meta"), bt, cl, cu)
    with pytest.raises(ValueError, match="cu_seqlens_q is required with tree_mask"):
        call(q[:3], kv, words[:3], bt, cl, None)
    with pytest.raises(ValueError, match="kv_scale applies to a float8_e4m3fn cache only"):
        call(q, kv, words, bt, cl, cu, kv_scale=0.5)
    with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
        call(q, kv8, words, bt, cl, cu, kv_scale=torch.ones(2))
    for bad in (torch.float16, torch.float32, torch.float8_e4m3fnuz, torch.float8_e5m2):
        with pytest.raises(ValueError, match="an FP8 latent cache must be torch.float8_e4m3fn"):
            call(q, torch.zeros(nb, bs, 576).to(bad), words, bt, cl, cu)
    with pytest.raises(ValueError, match="must be fp16 or bf16"):
        call(q.float(), kv.float(), words, bt, cl, cu)
    # the twin's own rules
    with pytest.raises(ValueError, match="latent width must be 576"):
        call(q[..., :512], kv, words, bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,576\]"):
        call(q[0], kv, words, bt, cl, cu)
    with pytest.raises(ValueError, match="block_size must be positive"):
        call(q, kv[:, :0], words, bt, cl, cu)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        call(q, kv, words, bt, cl[:2], cu)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\]"):
        call(q, kv, words, bt, cl, cu[:3])
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        call(q, kv, words, bt, cl, cu.long())
    with pytest.raises(ValueError, match="max_seqlen_q must be a positive int or None"):
        call(q, kv, words, bt, cl, cu, max_seqlen_q=0)
    wide = torch.zeros(T, Hq * 576 + 4, dtype=torch.bfloat16)[:, :Hq * 576].view(T, Hq, 576)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        call(wide, kv, words, bt, cl, cu)
    # well-formed, on the CPU: both cache kinds, the 4-d cache, every spelling of the scale
    for cache, kw in ((kv, {}), (kv.view(nb, bs, 1, 576), dict(scale=192 ** -0.5)), (kv8, {}), (kv8, dict(kv_scale=0.5)),
                      (kv8, dict(kv_scale=torch.tensor([0.5]), max_seqlen_q=2, return_lse=True))):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q, cache, words, bt, cl, cu, **kw)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, kv, torch.full((T,), -1, dtype=torch.int64), bt, cl, cu)


def test_build_rule_and_the_units_text():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert len(re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()) == 25        # (tests/test_tree_host.py pins that line)
    srcs = [w for line in re.findall(r"^SRCS [:+]= (.*)$", mk, re.M) for w in line.split()]
    assert UNIT in srcs and len(srcs) == len(set(srcs)) and os.path.exists(os.path.join(CSRC, UNIT))
    assert re.search(r"^SRCS \+= %s$" % re.escape(UNIT), mk, re.M)
    dep = re.search(r"^\$\(OBJDIR\)/fa_fwd_mla_verify_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert {"fa_d256_common.h", "fa_paged_tile.h", "fa_mla_common.h", "kv_quant.h"} <= set(dep)
    assert not [f for f in os.listdir(CSRC) if "tree" in f]
    # the body is stated once: the new unit instantiates it and holds no arithmetic of its own
    text = open(os.path.join(CSRC, UNIT)).read()
    assert '#include "fa_mla_common.h"' in text and "mla_paged_body<T, KV, false, true>" in text
    assert "mfma16" not in text and "fast_exp2(" not in text
    # the words are the last field of the kernels' parameter struct: every other instance keeps its argument offsets
    common = open(os.path.join(CSRC, "fa_mla_common.h")).read()
    fields = re.sub(r"//.*", "", common.split("struct MlaParams {")[1].split("};")[0])
    assert fields.split(";")[-2].strip() == "const long long* tree_mask = nullptr"
    assert common.count("fast_exp2(m - mu)") == 1


def _recorded():
    """{(kernel, dtype traits, cache kind): the six figures} of the `tree` lines of profiles/mla_tree_resources.txt"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "mla_tree_resources.txt")):
        f = line.split()
        if len(f) == 10 and f[0] == "tree":
            rows[(f[1], f[2], f[3])] = dict(zip(FIGURES, map(int, f[4:])))
    return rows


def test_resource_audit_of_the_four_instances(tmp_path):
    """fp16 / bf16 x 16-bit / e4m3fn cache under a name of their own: __launch_bounds__(256, 1), 111 616 bytes of LDS, no scratch, no
    spill, at most 256 + 256 registers, and the figures profiles/mla_tree_resources.txt records.  (The dense and the sparse instances
    at their recorded figures: tests/test_mla_sparse_host.py.)"""
    noted = _recorded()
    assert sorted(noted) == sorted(("fa_mla_verify_kernel", t, k) for t in ("Bf16Traits", "F16Traits") for k in ("Kv16", "KvFp8"))
    res = resource_report(UNIT, tmp_path)
    for other in ("fa_fwd_mla_paged_kernel", "fa_mla_fp8_latent_kernel", "fa_fwd_mla_sparse_kernel", "fa_mla_sparse_fp8_kernel", "fa_mla_combine_kernel"):
        assert not [n for n in res if other in n], other
    assert len(res) == 4, list(res)
    for (kernel, traits, kind), want in noted.items():
        ks = [n for n in res if kernel in n and "_%d%s" % (len(traits), traits) in n and "_%d%s" % (len(kind), kind) in n]
        assert len(ks) == 1, (kernel, traits, kind, list(res))
        got = {k: res[ks[0]].get(k) for k in FIGURES}
        print(kernel, traits, kind, got)
        assert got["ScratchSize"] == 0 and got["SGPRs Spill"] == 0 and got["VGPRs Spill"] == 0 and got["LDS Size"] == 111616, (ks[0], got)
        assert got["VGPRs"] <= 256 and got["AGPRs"] <= 256, (ks[0], got)
        assert got == want, (ks[0], got, want)       # the file reports what the compiler says
