"""The paged cascade and the merge of attention states without a GPU: the additive C-ABI (symbols, descriptor layouts, the
answers the entries give before they need a device), the argument errors of the torch layer, the invariants of the
shared-prefix launch plan through its debug hook, and a resource audit of the new kernels (no scratch, no spill)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
PTRS = ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "prefix_block_table", "prefix_len")
MAX_SPLIT = 32


def _fill(T=700, B=3, Hq=32, Hkv=8, D=128, bs=16, max_blocks=64, prefix_blocks=128, max_sq=512, dtype=2, cache_dtype=0):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer
    before a launch"""
    d = _capi.PagedCascadeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = dtype, cache_dtype
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, Hkv, D
    d.block_size, d.max_blocks, d.max_prefix_blocks = bs, max_blocks, prefix_blocks
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, max_sq, Hq * D
    for n in PTRS:
        setattr(d, n, 4096)
    if cache_dtype == 1:
        d.k_scale = d.v_scale = 4096
    return d


def _merge(rows=5, heads=4, D=64, dtype=1):
    d = _capi.MergeStatesDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.rows, d.heads, d.head_dim = dtype, rows, heads, D
    for i, n in enumerate(("out_a", "lse_a", "out_b", "lse_b", "out", "lse")):
        setattr(d, n, (i + 1) << 20)     # apart: lse may not overlap lse_a / lse_b
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0] for s in _capi.SIGNATURES}
    for name, arg in (("aule_attention_paged_cascade_ex", "aule_paged_cascade_desc"), ("aule_attention_paged_cascade_workspace_size", "aule_paged_cascade_desc"),
                      ("aule_attention_merge_states_ex", "aule_merge_states_desc"), ("aule_hip_debug_shared_prefix_plan", "aule_paged_cascade_desc")):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, arg), header), name
        assert hasattr(lib, name) and name in bound, name
    for name in ("flash_attention_paged_cascade", "merge_attention_states"):
        assert name in aule.__all__ and callable(getattr(aule, name))
    sig = inspect.signature(aule.flash_attention_paged_cascade)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "prefix_block_table", "prefix_len", "block_tables", "context_lens", "cu_seqlens_q",
                                    "max_seqlen_q", "scale", "k_scale", "v_scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["scale"].default is None and p["return_lse"].default is False
    assert list(inspect.signature(aule.merge_attention_states).parameters) == ["out_a", "lse_a", "out_b", "lse_b"]


CASCADE_OFFSETS = dict(struct_size=0, dtype=4, cache_dtype=8, batch=12, heads_q=16, heads_kv=20, head_dim=24, block_size=28, max_blocks=32,
                       total_tokens=36, max_seqlen_q=40, scale=44, max_prefix_blocks=48, device=52, q_token_stride=56, stream=64, q=72, k_cache=80,
                       v_cache=88, block_tables=96, context_lens=104, cu_seqlens_q=112, out=120, lse=128, k_scale=136, v_scale=144,
                       prefix_block_table=152, prefix_len=160, workspace=168, workspace_bytes=176)
MERGE_OFFSETS = dict(struct_size=0, dtype=4, rows=8, heads=12, head_dim=16, device=20, stream=24, out_a=32, lse_a=40, out_b=48, lse_b=56, out=64, lse=72)


@pytest.mark.parametrize("struct,cls,size,want", [("aule_paged_cascade_desc", "PagedCascadeDesc", 184, CASCADE_OFFSETS),
                                                  ("aule_merge_states_desc", "MergeStatesDesc", 80, MERGE_OFFSETS)])
def test_descriptor_layouts_match_the_header(struct, cls, size, want):
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(%s) = %d" % (struct, size) in header and "sizeof(%s) == %d" % (struct, size) in capi
    D = getattr(_capi, cls)
    assert ctypes.sizeof(D) == size
    assert [n for n, _ in D._fields_] == list(want)
    for name, off in want.items():
        assert getattr(D, name).offset == off, name
    body = header.split("typedef struct %s" % struct)[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= len(want) - 8
    for name, off in quoted:
        assert want[name] == int(off), name
    pinned = re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % struct, capi)
    assert len(pinned) >= len(want) - 8
    for name, off in pinned:
        assert want[name] == int(off), name
    if struct == "aule_paged_cascade_desc":   # the prefill's fields without the window, plus the prefix and the workspace
        theirs = {n for n, _ in _capi.PagedPrefillDesc._fields_} - {"window_size"}
        assert theirs | {"prefix_block_table", "prefix_len", "max_prefix_blocks", "workspace", "workspace_bytes"} == set(want)


BAD_FIELDS = [
    ("struct_size", 0, "struct_size"), ("struct_size", 152, "struct_size"), ("struct_size", 192, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("cache_dtype", 2, "cache_dtype"), ("cache_dtype", -1, "cache_dtype"),
    ("head_dim", 256, "head_dim 256"), ("head_dim", 48, "head_dim 48"), ("head_dim", 0, "head_dim 0"),
    ("heads_kv", 5, "divisible"), ("heads_kv", 0, "divisible"),
    ("block_size", 0, "block_size"), ("max_blocks", 0, "max_blocks"), ("max_blocks", 1 << 26, "max_blocks"),
    ("max_prefix_blocks", 0, "max_prefix_blocks"), ("max_prefix_blocks", 1 << 26, "max_prefix_blocks"),
    ("max_seqlen_q", 0, "max_seqlen_q"),
    ("q_token_stride", 32 * 128 - 8, "smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", -4096, "smaller than a token"), ("q_token_stride", 32 * 128 + 4, "multiple of 8"),
    ("total_tokens", 1 << 30, "too large"),
    ("q", None, "null tensor pointer"), ("k_cache", None, "null tensor pointer"), ("v_cache", None, "null tensor pointer"),
    ("block_tables", None, "null tensor pointer"), ("context_lens", None, "null tensor pointer"),
    ("cu_seqlens_q", None, "null tensor pointer"), ("out", None, "null tensor pointer"),
    ("prefix_block_table", None, "null tensor pointer"), ("prefix_len", None, "null tensor pointer"),
    ("k_scale", 4096, "FP8 caches only"), ("v_scale", 4096, "FP8 caches only"),
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("k_cache", 4097, "16-byte aligned"), ("v_cache", 4100, "16-byte aligned"),
]


@pytest.mark.parametrize("field,bad,needle", BAD_FIELDS, ids=lambda x: str(x).replace(" ", "_"))
def test_cascade_entry_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library); a field the
    plan reads is refused by the workspace query (0) and the plan hook (-3) too."""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib), _error(lib)
    if needle not in ("null tensor pointer", "FP8 caches only", "16-byte aligned"):
        plan = (ctypes.c_int32 * 7)()
        assert lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d)) == 0
        assert lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(d), plan, 7) == -3


def test_cascade_entry_refuses_fp8_without_scales_and_null():
    lib = _capi.load()
    assert lib.aule_attention_paged_cascade_ex(None) == -3
    assert lib.aule_attention_paged_cascade_workspace_size(None) == 0
    assert lib.aule_hip_debug_shared_prefix_plan(None, None, 0) == -3
    for field in ("k_scale", "v_scale"):
        d = _fill(cache_dtype=1)
        setattr(d, field, None)
        assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == -3
        assert "scale pointer" in _error(lib)
    # the packed-row count must fit 32 bits: 2^29 tokens x 8 heads per KV head
    d = _fill(T=1 << 29, Hq=64, Hkv=8)
    d.q_token_stride = 64 * 128
    assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == -3
    assert "32 bits" in _error(lib)


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0, batch = 0 or heads_q = 0: 0, with null pointers, in any process; no workspace, no plan."""
    lib = _capi.load()
    plan = (ctypes.c_int32 * 7)()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill()
        setattr(d, field, 0)
        if field == "heads_q":
            d.q_token_stride = 0
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == 0, field
        assert lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d)) == 0
        assert lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(d), plan, 7) == 0
    d = _fill(T=0)
    d.head_dim = 256
    assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == -3
    m = _merge(rows=0)
    for n in ("out_a", "lse_a", "out_b", "lse_b", "out", "lse"):
        setattr(m, n, None)
    assert lib.aule_attention_merge_states_ex(ctypes.byref(m)) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entries_report_uninitialised_without_a_gpu():
    lib = _capi.load()
    for cache_dtype in (0, 1):
        assert lib.aule_attention_paged_cascade_ex(ctypes.byref(_fill(cache_dtype=cache_dtype))) == -1
    assert lib.aule_attention_merge_states_ex(ctypes.byref(_merge())) == -1


@pytest.mark.parametrize("field,bad,needle", [("struct_size", 72, "struct_size"), ("dtype", 0, "fp16 or bf16"), ("head_dim", 0, "head_dim 0"),
                                              ("head_dim", 36, "head_dim 36"), ("head_dim", 2048, "head_dim 2048"), ("rows", 1 << 31, "too large"),
                                              ("out_a", None, "null tensor pointer"), ("lse_b", None, "null tensor pointer"), ("lse", None, "null tensor pointer"),
                                              ("out_b", (3 << 20) + 8, "16-byte aligned"), ("out", (5 << 20) + 2, "16-byte aligned")],
                         ids=lambda x: str(x).replace(" ", "_"))
def test_merge_entry_refuses_each_bad_field(field, bad, needle):
    lib = _capi.load()
    d = _merge()
    setattr(d, field, bad)
    assert lib.aule_attention_merge_states_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib), _error(lib)
    assert lib.aule_attention_merge_states_ex(None) == -3


@pytest.mark.parametrize("D", [64, 40, 1024])
def test_merge_entry_refuses_an_lse_that_overlaps_an_input(D):
    """Only out may alias an input: every thread of a row reads lse_a and lse_b, so an lse inside either is refused, whatever
    head_dim; one that ends where an input begins is not (it then reports the missing device or initialisation, not -3)."""
    lib = _capi.load()
    nbytes = 5 * 4 * 4
    for which in ("lse_a", "lse_b"):
        for shift in (0, 4, nbytes - 4, -(nbytes - 4)):
            d = _merge(D=D)
            d.lse = getattr(d, which) + shift
            assert lib.aule_attention_merge_states_ex(ctypes.byref(d)) == -3, (which, shift)
            assert "must not overlap" in _error(lib), _error(lib)
    if not os.path.exists("/dev/kfd"):
        d = _merge(D=D)
        d.lse = d.lse_a + nbytes
        assert lib.aule_attention_merge_states_ex(ctypes.byref(d)) == -1


def _plan(lib, d):
    out = (ctypes.c_int32 * 7)()
    assert lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(d), out, 7) == 7
    row_blocks, tiles, nsplit, tps, grid, lo, hi = list(out)
    return row_blocks, tiles, nsplit, tps, grid, (lo & 0xffffffff) | (hi << 32)


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (6, 2), (4, 1), (8, 8)])
@pytest.mark.parametrize("T", [1, 64, 129, 4096, 100000])
def test_plan_invariants(T, Hq, Hkv):
    """Over (T, g, Hkv, capacity): the splits tile [0, capacity) in whole 64-key tiles exactly once, 1 <= nsplit <= the cap, the
    grid is row blocks x Hkv x nsplit, the workspace is the header's formula, a capacity of one tile gives one split."""
    lib = _capi.load()
    g = Hq // Hkv
    for bs, blocks in ((16, 1), (16, 4), (16, 5), (24, 3), (1, 200), (128, 1), (16, 512), (16, 2048), (16, 1 << 16), (7, 1000)):
        for D in (64, 128):
            d = _fill(T=T, Hq=Hq, Hkv=Hkv, D=D, bs=bs, prefix_blocks=blocks)
            d.q_token_stride = Hq * D
            row_blocks, tiles, nsplit, tps, grid, ws = _plan(lib, d)
            cap = bs * blocks
            assert row_blocks == (T * g + 127) // 128 and tiles == (cap + 63) // 64
            assert 1 <= nsplit <= MAX_SPLIT and tps >= 1
            # split k owns tiles [k tps, min((k + 1) tps, tiles)): each non-empty, together every tile once
            assert (nsplit - 1) * tps < tiles <= nsplit * tps
            assert grid == row_blocks * Hkv * nsplit
            if cap <= 64:
                assert nsplit == 1
            # the two ends of the rule, whatever the device: more items than any part has compute units are not split, and one
            # item is split as far as the bounds allow
            if row_blocks * Hkv >= 512:
                assert nsplit == 1
            if row_blocks * Hkv == 1:
                assert tps == -(-tiles // min(MAX_SPLIT, tiles))
            r16 = lambda x: (x + 15) // 16 * 16   # noqa: E731
            assert ws == r16(nsplit * T * Hq * (D + 2) * 4) + r16(T * Hq * 4)
            assert lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d)) == ws
    out = (ctypes.c_int32 * 7)()
    assert lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(_fill()), out, 3) == -7      # the capacity needed
    assert lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(_fill()), None, 0) == -7


def test_argument_errors_are_value_errors_before_any_launch():
    """Through the two Python functions with CPU tensors: every rule is checked before the library is loaded or a device
    touched; a well-formed CPU call is an AuleError (no fallback)."""
    import torch
    B, T, Hq, Hkv, D, bs = 2, 10, 8, 2, 64, 16
    q = torch.zeros(T, Hq, D, dtype=torch.float16)
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    pbt = torch.zeros(3, dtype=torch.int32)
    pl = torch.tensor([20], dtype=torch.int32)
    cl = torch.full((B,), 5, dtype=torch.int32)
    cu = torch.tensor([0, 5, 10], dtype=torch.int32)
    call = aule.flash_attention_paged_cascade
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,D\]"):
        call(q.reshape(B, 5, Hq, D), c16, c16, pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,D\]"):
        call(q, c16, c16[:2], pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="head_dim mismatch"):
        call(q, torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="divisible"):
        call(q, torch.zeros(4, bs, 3, D, dtype=torch.float16), torch.zeros(4, bs, 3, D, dtype=torch.float16), pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="same dtype"):
        call(q, c8, c16, pbt, pl, bt, cl, cu)
    co = torch.zeros(4, bs, Hkv, D).to(torch.float8_e5m2)
    with pytest.raises(ValueError, match=r"float8_e4m3fn only.*OCP"):
        call(q, co, co, pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="paged cascade runs in fp16 or bf16"):
        call(q.float(), c8, c8, pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q, c16.to(torch.bfloat16), c16.to(torch.bfloat16), pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        call(q, c16, c16, pbt, pl, bt, cl, cu, k_scale=0.5)
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        call(q, c8, c8, pbt, pl, bt, cl, cu, k_scale=torch.ones(Hkv + 1))
    with pytest.raises(ValueError, match="head_dim must be one of"):
        c256 = torch.zeros(4, bs, Hkv, 256, dtype=torch.float16)
        call(torch.zeros(T, Hq, 256, dtype=torch.float16), c256, c256, pbt, pl, bt, cl, cu)
    with pytest.raises(ValueError, match="block_size"):
        c0 = torch.zeros(4, 0, Hkv, D, dtype=torch.float16)
        call(q, c0, c0, pbt, pl, bt, cl, cu)
    for bad in (pbt[:0], pbt.view(1, 3), pbt.float(), [0, 1, 2]):
        with pytest.raises(ValueError, match="prefix_block_table must be"):
            call(q, c16, c16, bad, pl, bt, cl, cu)
    for bad in (pl.long(), torch.zeros(2, dtype=torch.int32), torch.tensor(20, dtype=torch.int32), 2.5, True, None, 1 << 31):
        with pytest.raises(ValueError, match="prefix_len must be"):
            call(q, c16, c16, pbt, bad, bt, cl, cu)
    for bad_bt, bad_cl in ((bt[0], cl), (bt, cl[:1]), (bt[:, :0], cl), (bt, cl.view(B, 1))):
        with pytest.raises(ValueError, match="block_tables must be"):
            call(q, c16, c16, pbt, pl, bad_bt, bad_cl, cu)
    for bad_cu in (cu[:2], cu.view(1, B + 1), [0, 5, 10]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] = \[3\] tensor"):
            call(q, c16, c16, pbt, pl, bt, cl, bad_cu)
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        call(q, c16, c16, pbt, pl, bt, cl, cu.long())
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, c16, c16, pbt, pl, bt, cl, cu, max_seqlen_q=bad)
    wide = torch.zeros(T, Hq * D + 4, dtype=torch.float16)
    with pytest.raises(ValueError, match="multiples of 8 elements"):
        call(wide[:, :Hq * D].view(T, Hq, D), c16, c16, pbt, pl, bt, cl, cu)
    with pytest.raises(TypeError):
        call(q, c16, c16, pbt, pl, bt, cl, cu, window_size=16)       # not built
    for ok_pl in (pl, 20, 0, -5):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q, c16, c16, pbt, ok_pl, bt, cl, cu, max_seqlen_q=5)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, c8, c8, pbt.long(), pl, bt, cl, cu, k_scale=0.5, v_scale=torch.ones(Hkv), return_lse=True)

    merge = aule.merge_attention_states
    o, l = torch.zeros(T, Hq, D, dtype=torch.bfloat16), torch.zeros(T, Hq)
    with pytest.raises(ValueError, match="four tensors"):
        merge(o, l, o, None)
    with pytest.raises(ValueError, match="one shape"):
        merge(o, l, o[:5], l)
    with pytest.raises(ValueError, match="one shape"):
        merge(o[0, 0], l[0, 0], o[0, 0], l[0, 0])
    with pytest.raises(ValueError, match="both be fp16 or both bf16"):
        merge(o, l, o.half(), l)
    with pytest.raises(ValueError, match="both be fp16 or both bf16"):
        merge(o.float(), l, o.float(), l)
    with pytest.raises(ValueError, match="without head_dim"):
        merge(o, l[:5], o, l)
    with pytest.raises(ValueError, match="without head_dim"):
        merge(o, l, o, l.unsqueeze(-1))
    with pytest.raises(ValueError, match="must be float32"):
        merge(o, l.double(), o, l)
    with pytest.raises(ValueError, match="multiple of 8"):
        merge(o[..., :36], l, o[..., :36], l)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        merge(o, l, o, l)


def test_new_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fa_fwd_paged_shared_prefix_kernel<T, D, KV> (fp16, bf16 x D 32, 64, 128 x the two cache kinds), fa_cascade_merge_kernel<T, D>
    and fa_merge_states_kernel<T>."""
    res = {}
    for stem in ("fa_fwd_paged_shared_prefix_gfx950", "fa_merge_states_gfx950"):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                            "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / (stem + ".o")), os.path.join(CSRC, stem + ".hip")],
                           capture_output=True, text=True, timeout=900, cwd=CSRC)
        assert r.returncode == 0, r.stderr[-3000:]
        cur = None
        for line in r.stderr.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = m.group(1)
                res[cur] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[bytes/block\]| \[waves/SIMD\])?: (\d+)", line)
            if m and cur is not None:
                res[cur][m.group(1)] = int(m.group(2))
    ks = [n for n in res if "fa_fwd_paged_shared_prefix_kernel" in n]
    assert len(ks) == 12 and sum("KvFp8" in n for n in ks) == 6 and sum("Kv16" in n for n in ks) == 6, ks
    assert sum("Bf16Traits" in n for n in ks) == 6 and sum("F16Traits" in n for n in ks) == 6
    cm = [n for n in res if "fa_cascade_merge_kernel" in n]
    ms = [n for n in res if "fa_merge_states_kernel" in n]
    assert len(cm) == 6 and len(ms) == 2, (cm, ms)
    assert len(res) == 20, sorted(res)
    for n, r_ in res.items():
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") <= 40 * 1024, (n, r_)
