"""The MLA indexer without a GPU: the additive C-ABI (symbols, both descriptors' layouts, every answer the two entries give before they
need a device, the agreement of the logits launch and its plan hook), the invariants of the launch plan over a sweep of shapes, the
argument errors of the torch layer, the build rule and a resource audit of the five kernel instances compiled with the Makefile's
compiler and flags (no scratch, no spill, the figures recorded in profiles/mla_indexer_resources.txt)."""
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
LOGITS, TOPK, HOOK = "aule_mla_indexer_logits_ex", "aule_mla_indexer_topk_ex", "aule_hip_debug_mla_indexer_plan"
L_PTRS = ("q", "weights", "k_cache", "block_tables", "context_lens", "cu_seqlens_q", "logits")
T_PTRS = ("logits", "block_tables", "context_lens", "cu_seqlens_q", "indices")
L_LAYOUT = dict(struct_size=0, dtype=4, cache_dtype=8, heads=12, head_dim=16, batch=20, num_blocks=24, block_size=28, max_blocks=32,
                total_tokens=36, max_seqlen_q=40, device=44, q_token_stride=48, logits_stride=56, stream=64, q=72, weights=80, k_cache=88,
                k_scale=96, block_tables=104, context_lens=112, cu_seqlens_q=120, logits=128)
T_LAYOUT = dict(struct_size=0, output=4, topk=8, batch=12, block_size=16, max_blocks=20, total_tokens=24, max_seqlen_q=28, device=32,
                reserved=36, logits_stride=40, stream=48, logits=56, block_tables=64, context_lens=72, cu_seqlens_q=80, indices=88)
FIGURES = ("VGPRs", "AGPRs", "ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size")
CUS = 256   # what the plan assumes without a device, and what an MI355X has


def _logits(T=8, H=64, B=2, nb=64, bs=64, mb=16, msq=4, dtype=2, fp8=False, ragged=True):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.MlaIndexerLogitsDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads, d.head_dim, d.batch = dtype, int(fp8), H, 128, B
    d.num_blocks, d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = nb, bs, mb, T, msq
    d.q_token_stride, d.logits_stride = H * 128, bs * mb
    for n in L_PTRS:
        setattr(d, n, 4096)
    if not ragged:
        d.cu_seqlens_q = None
    if fp8:
        d.k_scale = 4096
    return d


def _topk(T=8, B=2, bs=64, mb=16, msq=4, topk=2048, ragged=True):
    d = _capi.MlaIndexerTopkDesc()
    d.struct_size = ctypes.sizeof(d)
    d.output, d.topk, d.batch, d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = 0, topk, B, bs, mb, T, msq
    d.logits_stride = bs * mb
    for n in T_PTRS:
        setattr(d, n, 4096)
    if not ragged:
        d.cu_seqlens_q = None
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _plan(lib, d):
    out = (ctypes.c_int32 * 5)()
    n = lib.aule_hip_debug_mla_indexer_plan(ctypes.byref(d), out, 5)
    return n, list(out)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, desc in ((LOGITS, "aule_mla_indexer_logits_desc"), (TOPK, "aule_mla_indexer_topk_desc"), (HOOK, "aule_mla_indexer_logits_desc")):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, desc), header), name
        assert hasattr(lib, name) and name in bound, name
    assert "#define AULE_INDEXER_SLOTS 0" in header and "#define AULE_INDEXER_POSITIONS 1" in header
    assert (_capi.INDEXER_SLOTS, _capi.INDEXER_POSITIONS) == (0, 1)
    want = {"mla_indexer_logits": ["q", "weights", "k_cache", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "k_scale"],
            "mla_indexer_topk": ["logits", "topk", "block_tables", "context_lens", "block_size", "cu_seqlens_q", "max_seqlen_q", "output"],
            "mla_indexer": ["q", "weights", "k_cache", "block_tables", "context_lens", "topk", "cu_seqlens_q", "max_seqlen_q", "k_scale", "output",
                            "return_logits"],
            "quantize_indexer_cache_fp8": ["k_cache"]}
    for name, params in want.items():
        assert name in aule.__all__ and callable(getattr(aule, name)), name
        assert list(inspect.signature(getattr(aule, name)).parameters) == params, name
    sig = inspect.signature(aule.mla_indexer)
    assert sig.parameters["output"].default == "slots" and sig.parameters["return_logits"].default is False
    assert inspect.signature(aule.mla_indexer_topk).parameters["output"].default == "slots"
    # the docstring names what is out of scope and what the logits cost
    doc = " ".join(aule.mla_indexer_logits.__doc__.split())
    for what in ("FP8 queries", "streaming top-k", "append kernel", "H > 64", "backward", "T * W * 4 bytes", "1 GB"):
        assert what in doc, what
    # ... and the sparse entry points to its producer
    assert "aule.mla_indexer" in aule.flash_attention_mla_sparse.__doc__.split("Out of scope:")[1]


@pytest.mark.parametrize("cls,name,layout,size", [(_capi.MlaIndexerLogitsDesc, "aule_mla_indexer_logits_desc", L_LAYOUT, 136),
                                                  (_capi.MlaIndexerTopkDesc, "aule_mla_indexer_topk_desc", T_LAYOUT, 96)], ids=["logits", "topk"])
def test_descriptor_layouts_match_the_header(cls, name, layout, size):
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(%s) = %d" % (name, size) in header and "sizeof(%s) == %d" % (name, size) in capi
    assert ctypes.sizeof(cls) == size
    assert [n for n, _ in cls._fields_] == list(layout)
    for field, off in layout.items():
        assert getattr(cls, field).offset == off, field
    body = header.split("typedef struct %s {" % name)[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) == len(layout) - 1
    for field, off in quoted:
        assert layout[field] == int(off), field
    pinned = re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % name, capi)
    assert len(pinned) == len(layout) - 1
    for field, off in pinned:
        assert layout[field] == int(off), field
    assert ctypes.sizeof(_capi.MlaSparseDesc) == 120 and ctypes.sizeof(_capi.MlaPagedDesc) == 136   # the neighbours keep their sizes


# (field, bad value, a piece of the reason): what the shape alone decides -- the launch and the plan hook both refuse
L_BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 144, "struct_size"),
    ("dtype", 0, "dtype 0"), ("dtype", 3, "dtype 3"),
    ("cache_dtype", 2, "cache_dtype 2"), ("cache_dtype", -1, "cache_dtype -1"),
    ("heads", 0, "heads (0)"), ("heads", 65, "heads (65) must be in 1 .. 64"),
    ("head_dim", 64, "head_dim (64) must be 128"), ("head_dim", 576, "head_dim (576)"),
    ("num_blocks", 0, "num_blocks * block_size (0 * 64)"),
    ("block_size", 0, "block_size (0) and max_blocks (16)"), ("max_blocks", 0, "block_size (64) and max_blocks (0)"),
    ("max_blocks", 1 << 24, "block_size (64) and max_blocks (16777216)"),
    ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("q_token_stride", 64 * 128 - 8, "q_token_stride (8184) is smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", 64 * 128 + 4, "q_token_stride (8196) must be a multiple of 8"),
    ("logits_stride", 1023, "logits_stride (1023) is smaller than a row"), ("logits_stride", -1, "logits_stride (-1)"),
    ("batch", 1 << 30, "batch (1073741824) too large"), ("total_tokens", 1 << 30, "total_tokens (1073741824) too large"),
]
# ... and what only a launch looks at
L_BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "weights", "k_cache", "block_tables", "context_lens", "logits")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("k_cache", 4097, "16-byte aligned"), ("weights", 4098, "4-byte aligned"), ("logits", 4097, "4-byte aligned"),
    ("block_tables", 4098, "4-byte aligned"), ("context_lens", 4099, "4-byte aligned"), ("cu_seqlens_q", 4098, "4-byte aligned"),
    ("k_scale", 4096, "k_scale applies to an FP8 cache only")]
T_BAD = [
    ("struct_size", 0, "struct_size"), ("struct_size", 136, "struct_size"),
    ("output", 2, "output 2"), ("output", -1, "output -1"),
    ("topk", 0, "topk (0)"), ("topk", 65537, "topk (65537) must be in 1 .. 65536"), ("topk", -1, "topk (-1)"),
    ("reserved", 1, "reserved (1) must be 0"),
    ("block_size", 0, "block_size (0) and max_blocks (16)"), ("max_blocks", 0, "block_size (64) and max_blocks (0)"),
    ("max_blocks", 1 << 24, "block_size (64) and max_blocks (16777216)"),
    ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("logits_stride", 1023, "logits_stride (1023) is smaller than a row"),
    ("batch", 1 << 30, "batch (1073741824) too large"), ("total_tokens", 1 << 30, "total_tokens (1073741824) too large"),
] + [(n, None, "null tensor pointer") for n in ("logits", "block_tables", "context_lens", "indices")] + [
    ("logits", 4098, "4-byte aligned"), ("indices", 4097, "4-byte aligned"), ("block_tables", 4098, "4-byte aligned"),
    ("context_lens", 4099, "4-byte aligned"), ("cu_seqlens_q", 4098, "4-byte aligned")]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", L_BAD_SHAPE + L_BAD_POINTER, ids=_ids)
def test_logits_launch_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason naming the field, before the device is needed (so also in a process that never initialised the library)"""
    lib = _capi.load()
    d = _logits()
    setattr(d, field, bad)
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA indexer logits failed: "), _error(lib)


@pytest.mark.parametrize("field,bad,needle", T_BAD, ids=_ids)
def test_topk_launch_refuses_each_bad_field(field, bad, needle):
    lib = _capi.load()
    d = _topk()
    setattr(d, field, bad)
    assert lib.aule_mla_indexer_topk_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA indexer top-k failed: "), _error(lib)


def test_fp8_scale_rules_plain_decode_rule_and_null_descriptors():
    lib = _capi.load()
    d = _logits(fp8=True)
    d.k_scale = None
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3 and "null k_scale" in _error(lib)
    d.k_scale = 4098
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3 and "4-byte aligned" in _error(lib)
    # plain decode: sequence b owns row b
    d = _logits(T=3, B=4, ragged=False)
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3 and "total_tokens (3) < batch (4)" in _error(lib)
    assert _plan(lib, d)[0] == -3
    t = _topk(T=3, B=4, ragged=False)
    assert lib.aule_mla_indexer_topk_ex(ctypes.byref(t)) == -3 and "total_tokens (3) < batch (4)" in _error(lib)
    assert lib.aule_mla_indexer_logits_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_mla_indexer_topk_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_hip_debug_mla_indexer_plan(None, None, 0) == -3
    # grids past 2^31 - 1 workgroups
    d = _logits(T=(1 << 30) - 1, B=(1 << 30) - 1, msq=12, bs=1, mb=1)   # 3 token groups per sequence
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3 and "exceeds 2^31 - 1 workgroups" in _error(lib) and _plan(lib, d)[0] == -3
    t = _topk(T=(1 << 30) - 1, B=(1 << 30) - 1, msq=12, bs=1, mb=1)
    assert lib.aule_mla_indexer_topk_ex(ctypes.byref(t)) == -3 and "exceeds 2^31 - 1 workgroups" in _error(lib)


@pytest.mark.parametrize("field,bad,needle", L_BAD_SHAPE, ids=_ids)
def test_plan_hook_and_launch_give_the_same_verdict(field, bad, needle):
    """one checker: what the launch refuses on the shape the hook answers with -3"""
    lib = _capi.load()
    d = _logits()
    assert _plan(lib, d)[0] == 5
    setattr(d, field, bad)
    assert _plan(lib, d)[0] == -3
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3


@pytest.mark.parametrize("field,bad,needle", L_BAD_POINTER, ids=_ids)
def test_plan_hook_reads_no_pointer(field, bad, needle):
    """the pointer rules are the launch's alone: the hook answers a descriptor with bad or null pointers as it answers a good one (that
    cu_seqlens_q IS null states plain decode -- a fact of the shape, not a read)"""
    lib = _capi.load()
    for fp8 in (False, True):
        d = _logits(fp8=fp8)
        want = _plan(lib, d)
        assert want[0] == 5
        if field != "cu_seqlens_q" or bad is not None:
            setattr(d, field, bad)
        assert _plan(lib, d) == want
        for n in L_PTRS + ("k_scale",):
            if n != "cu_seqlens_q":
                setattr(d, n, None)
        assert _plan(lib, d) == want


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0 or batch = 0: 0 with null pointers, in any process; a refused field is still refused"""
    lib = _capi.load()
    for kw in (dict(T=0), dict(B=0)):
        d = _logits(**kw)
        for n in L_PTRS:
            setattr(d, n, None)
        assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == 0 and _plan(lib, d)[0] == 0
        d.heads = 65
        assert lib.aule_mla_indexer_logits_ex(ctypes.byref(d)) == -3 and _plan(lib, d)[0] == -3
        t = _topk(**kw)
        for n in T_PTRS:
            setattr(t, n, None)
        assert lib.aule_mla_indexer_topk_ex(ctypes.byref(t)) == 0
        t.topk = 0
        assert lib.aule_mla_indexer_topk_ex(ctypes.byref(t)) == -3


def test_plan_hook_capacity_contract():
    lib = _capi.load()
    d = _logits()
    out = (ctypes.c_int32 * 5)()
    assert lib.aule_hip_debug_mla_indexer_plan(ctypes.byref(d), None, 0) == -5
    assert lib.aule_hip_debug_mla_indexer_plan(ctypes.byref(d), out, 4) == -5 and list(out) == [0] * 5
    assert lib.aule_hip_debug_mla_indexer_plan(ctypes.byref(d), out, 5) == 5


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entries_report_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(_logits())) == -1
    assert lib.aule_mla_indexer_logits_ex(ctypes.byref(_logits(fp8=True, T=2, ragged=False))) == -1
    assert lib.aule_mla_indexer_topk_ex(ctypes.byref(_topk())) == -1
    t = _topk(T=2, ragged=False, topk=1)
    t.output = 1
    assert lib.aule_mla_indexer_topk_ex(ctypes.byref(t)) == -1


def test_plan_invariants_over_a_sweep():
    """every (token group, key chunk) is owned exactly once, the grid fits 31 bits, and the numbers are the rule's"""
    lib = _capi.load()
    split = whole = 0
    for B in (1, 2, 7, 64, 300):
        for msq in (1, 3, 4, 5, 64, 70, 2048):
            for bs, mb in ((1, 1), (1, 255), (16, 16), (48, 3), (64, 17), (64, 128), (64, 512), (64, 2048), (1, 70001)):
                W = bs * mb
                d = _logits(T=max(B, msq), B=B, bs=bs, mb=mb, msq=msq)
                n, (gt, groups, ck, chunks, grid) = _plan(lib, d)
                key = (B, msq, W)
                assert n == 5 and gt == 4 and groups == -(-msq // 4), key
                # the chunks tile [0, W): none empty, none missing, each a multiple of 128 keys
                assert ck % 128 == 0 and ck > 0 and chunks >= 1 and (chunks - 1) * ck < W <= chunks * ck, key
                assert grid == B * groups * chunks and 0 < grid <= 2 ** 31 - 1, key
                # the rule: a few workgroups per compute unit, at most one chunk per 128 keys
                units, base = -(-W // 128), B * groups
                want = max(1, min(-(-4 * CUS // base), units))
                per = -(-units // want)
                assert (ck, chunks) == (per * 128, -(-units // per)), key
                split += chunks > 1
                whole += chunks == 1
                # neither the cache kind nor the dtype changes the plan; plain decode is max_seqlen_q = 1
                assert _plan(lib, _logits(T=max(B, msq), B=B, bs=bs, mb=mb, msq=msq, fp8=True, dtype=1)) == (n, [gt, groups, ck, chunks, grid]), key
                dec = _plan(lib, _logits(T=max(B, msq), B=B, bs=bs, mb=mb, msq=msq, ragged=False))
                assert dec == _plan(lib, _logits(T=max(B, msq), B=B, bs=bs, mb=mb, msq=1)) and dec[1][1] == 1, key
    assert split > 50 and whole > 50
    # max_seqlen_q is cut at total_tokens: no sequence has more tokens than the batch
    assert _plan(lib, _logits(T=5, B=1, msq=4096))[1][1] == 2


def test_python_argument_errors_are_value_errors_before_the_device():
    import torch
    T, H, nb, bs, mb, B = 3, 4, 5, 16, 2, 3
    q = torch.zeros(T, H, 128, dtype=torch.bfloat16)
    w = torch.zeros(T, H)
    kc = torch.zeros(nb, bs, 128, dtype=torch.bfloat16)
    bt = torch.zeros(B, mb, dtype=torch.int32)
    cl = torch.zeros(B, dtype=torch.int32)
    cu = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
    lg = torch.zeros(T, mb * bs)
    logits, topk, both = aule.mla_indexer_logits, aule.mla_indexer_topk, aule.mla_indexer
    with pytest.raises(ValueError, match=r"expected q \[T,H,128\]"):
        logits(q[0], w, kc, bt, cl)
    with pytest.raises(ValueError, match="the index head width must be 128"):
        logits(q[..., :64], w, kc, bt, cl)
    with pytest.raises(ValueError, match="the index head width must be 128"):
        logits(q, w, torch.zeros(nb, bs, 576, dtype=torch.bfloat16), bt, cl)
    with pytest.raises(ValueError, match="q must be fp16 or bf16"):
        logits(q.float(), w, kc.float(), bt, cl)
    with pytest.raises(ValueError, match=r"1 \.\. 64 index heads, got 65"):
        logits(torch.zeros(T, 65, 128, dtype=torch.bfloat16), torch.zeros(T, 65), kc, bt, cl)
    with pytest.raises(ValueError, match="k_cache must have q's dtype"):
        logits(q, w, kc.half(), bt, cl)
    with pytest.raises(ValueError, match="k_cache must have q's dtype"):
        logits(q, w, kc.to(torch.float8_e4m3fnuz), bt, cl, k_scale=torch.ones(nb, bs))
    with pytest.raises(ValueError, match="a float8_e4m3fn k_cache needs k_scale"):
        logits(q, w, kc.to(torch.float8_e4m3fn), bt, cl)
    with pytest.raises(ValueError, match="k_scale applies to a float8_e4m3fn cache only"):
        logits(q, w, kc, bt, cl, k_scale=torch.ones(nb, bs))
    for bad in (torch.ones(nb), torch.ones(nb, bs, dtype=torch.float64), torch.ones(nb, 2 * bs)[:, ::2], 1.0):
        with pytest.raises(ValueError, match=r"k_scale must be a contiguous fp32 tensor \[num_blocks, block_size\] = \[5, 16\]"):
            logits(q, w, kc.to(torch.float8_e4m3fn), bt, cl, k_scale=bad)
    for bad in (w.double(), w[:, :3], torch.zeros(T, 2 * H)[:, ::2], w[:2]):
        with pytest.raises(ValueError, match=r"weights must be a contiguous fp32 tensor \[T, H\] = \[3, 4\]"):
            logits(q, bad, kc, bt, cl)
    with pytest.raises(ValueError, match="k_cache must be contiguous"):
        logits(q, w, torch.zeros(nb, 2 * bs, 128, dtype=torch.bfloat16)[:, ::2], bt, cl)
    with pytest.raises(ValueError, match=r"1 \.\. 2\^31 - 1 rows"):
        logits(q, w, kc[:0], bt, cl)
    for call in (lambda **kw: logits(q, w, kc, **kw), lambda **kw: topk(lg, 4, block_size=bs, **kw)):
        with pytest.raises(ValueError, match=r"block_tables must be an int32 tensor .*got torch\.int64"):
            call(block_tables=bt.long(), context_lens=cl)
        with pytest.raises(ValueError, match=r"context_lens must be an int32 tensor .*got torch\.int64"):
            call(block_tables=bt, context_lens=cl.long())
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be an int32 tensor .*got torch\.int64"):
            call(block_tables=bt, context_lens=cl, cu_seqlens_q=cu.long())
        with pytest.raises(ValueError, match="block_tables must be contiguous"):
            call(block_tables=torch.zeros(B, 2 * mb, dtype=torch.int32)[:, ::2], context_lens=cl)
        with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\] and context_lens \[batch\]"):
            call(block_tables=bt, context_lens=cl[:2])
        with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
            call(block_tables=bt[:2], context_lens=cl[:2])   # plain decode: the batch is T
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] = \[4\] tensor"):
            call(block_tables=bt, context_lens=cl, cu_seqlens_q=cu[:3])
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int or None"):
            call(block_tables=bt, context_lens=cl, cu_seqlens_q=cu, max_seqlen_q=0)
        with pytest.raises(ValueError, match="max_seqlen_q must be None or 1 without cu_seqlens_q"):
            call(block_tables=bt, context_lens=cl, max_seqlen_q=2)
    with pytest.raises(ValueError, match="no backward"):
        logits(q.clone().requires_grad_(True), w, kc, bt, cl)
    with pytest.raises(ValueError, match="no backward"):
        logits(q, w.clone().requires_grad_(True), kc, bt, cl)
    with pytest.raises(ValueError, match="no backward"):
        topk(lg.clone().requires_grad_(True), 4, bt, cl, bs)
    wide = torch.zeros(T, H * 128 + 4, dtype=torch.bfloat16)[:, :H * 128].view(T, H, 128)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        logits(wide, w, kc, bt, cl)
    # the top-k's own
    for bad in (0, 65537, -1, 2.0, True):
        with pytest.raises(ValueError, match=r"topk must be an int in 1 \.\. 65536"):
            topk(lg, bad, bt, cl, bs)
        with pytest.raises(ValueError, match=r"topk must be an int in 1 \.\. 65536"):
            both(q, w, kc, bt, cl, bad)
    with pytest.raises(ValueError, match="output must be 'slots' or 'positions', got 'slot'"):
        topk(lg, 4, bt, cl, bs, output="slot")
    with pytest.raises(ValueError, match="output must be 'slots' or 'positions'"):
        both(q, w, kc, bt, cl, 4, output=0)
    with pytest.raises(ValueError, match="logits must be an fp32"):
        topk(lg.double(), 4, bt, cl, bs)
    with pytest.raises(ValueError, match="logits must be an fp32"):
        topk(lg[0], 4, bt, cl, bs)
    with pytest.raises(ValueError, match=r"logits must have max_blocks \* block_size = 2 \* 16 = 32 columns, got 31"):
        topk(lg[:, :31], 4, bt, cl, bs)
    with pytest.raises(ValueError, match="the rows of logits must be contiguous"):
        topk(torch.zeros(T, 2 * mb * bs)[:, ::2], 4, bt, cl, bs)
    for bad in (0, -16, 16.0, True):
        with pytest.raises(ValueError, match="block_size must be a positive int"):
            topk(lg, 4, bt, cl, bad)
    # well-formed, on the CPU: both cache kinds, the 4-d cache, ragged and plain decode, a slice of a wider projection, a row stride
    codes, ks = aule.quantize_indexer_cache_fp8(kc)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        logits(q, w, kc, bt, cl)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        logits(q, w, codes.view(nb, bs, 1, 128), bt, cl, cu_seqlens_q=cu, max_seqlen_q=1, k_scale=ks)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        both(torch.zeros(T, H + 2, 128, dtype=torch.float16)[:, :H], w, kc.half(), bt, cl, 7, cu_seqlens_q=cu, return_logits=True)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        topk(torch.zeros(T, mb * bs + 5)[:, :mb * bs], 65536, bt, cl, bs, cu_seqlens_q=cu, output="positions")
    with torch.no_grad():
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            logits(q.clone().requires_grad_(True), w, kc, bt, cl)


def test_quantize_indexer_cache_fp8_per_row_scales():
    """torch ops only: the scale of a row is its amax / 448, an all-zero row gets 1, and scale * codes gives the row back within e4m3's step"""
    import torch
    g = torch.Generator().manual_seed(5)
    kc = torch.randn(3, 4, 128, generator=g).to(torch.bfloat16)
    kc[1, 2] = 0
    kc[2, 0] *= 1000
    codes, ks = aule.quantize_indexer_cache_fp8(kc)
    assert codes.dtype == torch.float8_e4m3fn and codes.shape == kc.shape and ks.dtype == torch.float32 and ks.shape == (3, 4) and ks.is_contiguous()
    amax = kc.float().abs().amax(dim=-1)
    want = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    assert torch.equal(ks, want) and float(ks[1, 2]) == 1.0
    assert bool((codes[1, 2].float() == 0).all()) and float(codes.float().abs().amax()) == 448.0
    back = codes.float() * ks[..., None]
    assert bool(((back - kc.float()).abs() <= amax[..., None] * 2.0 ** -4 + 1e-30).all())   # 3 mantissa bits: half a step of 2^-3 of the amax
    c4, k4 = aule.quantize_indexer_cache_fp8(kc.view(3, 4, 1, 128))
    assert torch.equal(c4.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(k4, ks)
    with pytest.raises(ValueError, match="expected an index key cache"):
        aule.quantize_indexer_cache_fp8(torch.zeros(3, 4, 576))


def test_build_rule_names_the_new_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    first = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fa_mla_indexer_gfx950.hip" not in first and len(first) == 25     # (tests/test_tree_host.py pins that line)
    later = re.findall(r"^SRCS \+= (.*)$", mk, re.M)
    assert "fa_mla_indexer_gfx950.hip" in later and all(len(line.split()) == 1 for line in later)   # one line per later source
    srcs = first + later
    assert len(srcs) == len(set(srcs)) and os.path.exists(os.path.join(CSRC, "fa_mla_indexer_gfx950.hip"))
    dep = re.search(r"^\$\(OBJDIR\)/fa_mla_indexer_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert "kv_quant.h" in dep
    text = open(os.path.join(CSRC, "fa_mla_indexer_gfx950.hip")).read()
    # the exact conversion of the codes is kv_quant.h's, stated once
    assert '#include "kv_quant.h"' in text and "cvt8<T>" in text and "__builtin_amdgcn_cvt_pk_f32_fp8" not in text
    assert "__builtin_amdgcn_cvt_pk_f32_fp8" in open(os.path.join(CSRC, "kv_quant.h")).read()
    assert "__builtin_amdgcn_cvt_pk_f32_fp8" not in open(os.path.join(CSRC, "fa_paged_tile.h")).read()
    # no atomics on global memory: the only atomic adds are the histogram's, in LDS
    assert set(re.findall(r"atomic\w*\(&(\w+)", text)) == {"hist"} and "__shared__ unsigned hist[256]" in text


def _recorded():
    """{kernel instance: the six figures} of the `indexer` lines of profiles/mla_indexer_resources.txt"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "mla_indexer_resources.txt")):
        f = line.split()
        if len(f) == 8 and f[0] == "indexer":
            rows[f[1]] = dict(zip(FIGURES, map(int, f[2:])))
    return rows


def test_resource_audit_no_scratch_no_spill_and_the_recorded_figures(tmp_path):
    """the four logits instances ({fp16, bf16} x {16-bit, FP8 cache}) and the top-k kernel: no scratch, no spill, at most 256 registers
    (two workgroups of the logits kernel per SIMD, and 1024 threads of the top-k fit a compute unit), and the six figures the
    compile gives are the recorded ones"""
    res = resource_report("fa_mla_indexer_gfx950.hip", tmp_path)
    noted = _recorded()
    names = {"logits.bf16.16": ("fa_mla_indexer_logits_kernel", "Bf16Traits", "Lb0"), "logits.bf16.fp8": ("fa_mla_indexer_logits_kernel", "Bf16Traits", "Lb1"),
             "logits.fp16.16": ("fa_mla_indexer_logits_kernel", "9F16Traits", "Lb0"), "logits.fp16.fp8": ("fa_mla_indexer_logits_kernel", "9F16Traits", "Lb1"),
             "topk": ("fa_mla_indexer_topk_kernel",)}
    assert sorted(noted) == sorted(names) and len(res) == len(names), (sorted(noted), sorted(res))
    for label, parts in names.items():
        ks = [n for n in res if all(p in n for p in parts)]
        assert len(ks) == 1, (label, list(res))
        got = {k: res[ks[0]].get(k) for k in FIGURES}
        print(label, got)
        assert got["ScratchSize"] == 0 and got["SGPRs Spill"] == 0 and got["VGPRs Spill"] == 0, (label, got)
        assert got["VGPRs"] + got["AGPRs"] <= 256, (label, got)
        if label == "topk":
            assert got["VGPRs"] + got["AGPRs"] <= 128 and got["LDS Size"] <= 2048, got   # 16 waves of one workgroup: 4 per SIMD
        else:
            assert got["LDS Size"] == 64 * 272 + (256 if label.endswith("fp8") else 0), (label, got)   # the K tile (+ its 64 row scales)
        assert got == noted[label], (label, got, noted[label])   # the file reports what the compiler says
