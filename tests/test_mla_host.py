"""Paged MLA attention without a GPU: the additive C-ABI (symbols, the descriptor's layout, every answer the entry gives before it
needs a device, the agreement of the launch, the size query and the plan hook), the invariants of the launch plan over a sweep of
shapes, the argument errors of the torch layer, the build rule and a resource audit of the kernels compiled with the Makefile's
compiler and flags (no scratch, no spill, LDS within the 160 KiB of a compute unit)."""
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
ENTRY, SIZE, HOOK = "aule_attention_mla_paged_ex", "aule_attention_mla_paged_workspace_size", "aule_hip_debug_mla_plan"
PTRS = ("q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "lse")
LAYOUT = dict(struct_size=0, dtype=4, batch=8, heads_q=12, qk_dim=16, v_dim=20, block_size=24, max_blocks=28, total_tokens=32,
              max_seqlen_q=36, scale=40, device=44, q_token_stride=48, stream=56, q=64, kv_cache=72, block_tables=80, context_lens=88,
              cu_seqlens_q=96, out=104, lse=112, workspace=120, workspace_bytes=128)
MAX_SPLIT = 64   # include/aule.h: "at most 64"


def _fill(T=24, B=8, Hq=16, bs=64, max_blocks=32, max_sq=3, dtype=2, decode=False):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.MlaPagedDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = dtype, B, Hq, 576, 512
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = bs, max_blocks, T, max_sq
    d.q_token_stride = Hq * 576
    for n in PTRS:
        setattr(d, n, 4096)
    if decode:
        d.cu_seqlens_q = None
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _plan(lib, d):
    out = (ctypes.c_int32 * 6)()
    n = lib.aule_hip_debug_mla_plan(ctypes.byref(d), out, 6)
    return n, list(out)


def _ws_formula(nsplit, T, Hq):
    return (nsplit * T * Hq * 514 * 4 + 15) // 16 * 16 if nsplit > 1 else 0


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name in (ENTRY, SIZE, HOOK):
        assert re.search(r"\b%s\s*\(const aule_mla_paged_desc\*" % name, header), name
        assert hasattr(lib, name) and name in bound, name
    assert bound[SIZE][1] is ctypes.c_uint64
    assert "flash_attention_mla_paged" in aule.__all__ and callable(aule.flash_attention_mla_paged)
    sig = inspect.signature(aule.flash_attention_mla_paged)
    assert list(sig.parameters) == ["q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale", "return_lse"]
    assert all(sig.parameters[n].default is None for n in ("cu_seqlens_q", "max_seqlen_q", "scale")) and sig.parameters["return_lse"].default is False


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_mla_paged_desc) = 136" in header and "sizeof(aule_mla_paged_desc) == 136" in capi
    assert ctypes.sizeof(_capi.MlaPagedDesc) == 136
    assert [n for n, _ in _capi.MlaPagedDesc._fields_] == list(LAYOUT)
    for name, off in LAYOUT.items():
        assert getattr(_capi.MlaPagedDesc, name).offset == off, name
    body = header.split("typedef struct aule_mla_paged_desc {")[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 20
    for name, off in quoted:
        assert LAYOUT[name] == int(off), name
    pinned = re.findall(r"offsetof\(aule_mla_paged_desc, (\w+)\) == (\d+)", capi)
    assert len(pinned) >= 12
    for name, off in pinned:
        assert LAYOUT[name] == int(off), name
    assert ctypes.sizeof(_capi.PagedPrefillDesc) == 152 and ctypes.sizeof(_capi.PagedCascadeDesc) == 184   # the neighbours keep their sizes


# (field, bad value, a piece of the reason): what the shape alone decides -- the launch, the size query and the plan hook all refuse
BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 152, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("qk_dim", 512, "qk_dim 512"), ("qk_dim", 128, "qk_dim 128"), ("v_dim", 576, "v_dim 576"), ("v_dim", 128, "v_dim 128"),
    ("block_size", 0, "bad block_size"), ("max_blocks", 0, "bad block_size"), ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"),
    ("q_token_stride", 16 * 576 - 8, "q_token_stride (9208) is smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", 16 * 576 + 4, "q_token_stride (9220) must be a multiple of 8"),
    ("total_tokens", 1 << 30, "too large"), ("batch", 1 << 30, "too large"),
]
# ... and what only a launch looks at
BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "kv_cache", "block_tables", "context_lens", "out")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("kv_cache", 4097, "16-byte aligned")]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_POINTER, ids=_ids)
def test_launch_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library)."""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Paged MLA attention failed: "), _error(lib)


def test_null_descriptor_decode_rows_and_packed_row_overflow():
    lib = _capi.load()
    assert lib.aule_attention_mla_paged_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_mla_paged_workspace_size(None) == 0 and _plan(lib, _fill())[0] == 6
    assert lib.aule_hip_debug_mla_plan(None, None, 0) == -3
    # plain decode (null offsets): sequence b owns row b, so the rows must be there
    d = _fill(T=7, B=8, decode=True)
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3 and "total_tokens < batch" in _error(lib)
    assert lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)) == 0 and _plan(lib, d)[0] == -3
    d = _fill(T=9, B=8, decode=True)
    assert _plan(lib, d)[0] == 6
    # (total_tokens + 64) * heads_q must fit 32 bits
    last = 0x7fffffff // 128 - 64
    d = _fill(T=last + 1, B=1, Hq=128)
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3 and "32 bits" in _error(lib)
    assert _plan(lib, d)[0] == -3 and _plan(lib, _fill(T=last, B=1, Hq=128))[0] == 6


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE, ids=_ids)
def test_size_query_plan_hook_and_launch_give_the_same_verdict(field, bad, needle):
    """one checker: what the launch refuses on the shape the size query answers with 0 and the hook with -3"""
    lib = _capi.load()
    d = _fill(T=2, B=1, max_sq=2)   # 1 row block x 1 sequence: split, so the accepted size is not 0
    n, plan = _plan(lib, d)
    assert n == 6 and plan[2] >= 2
    assert lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)) == _ws_formula(plan[2], 2, 16) > 0
    setattr(d, field, bad)
    assert lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)) == 0
    assert _plan(lib, d)[0] == -3
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3


@pytest.mark.parametrize("field,bad,needle", BAD_POINTER, ids=_ids)
def test_size_query_and_plan_hook_read_no_pointer(field, bad, needle):
    """the pointer rules are the launch's alone: both host queries answer a descriptor with bad or null pointers as they answer a good one"""
    lib = _capi.load()
    d = _fill(T=2, B=1, max_sq=2)
    want = (lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)), _plan(lib, d))
    setattr(d, field, bad)
    assert (lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)), _plan(lib, d)) == want
    for n in PTRS[:4] + PTRS[5:]:
        setattr(d, n, None)
    assert (lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)), _plan(lib, d)) == want


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0, batch = 0 or heads_q = 0: 0 with null pointers, in any process; a refused field is still refused"""
    lib = _capi.load()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill()
        setattr(d, field, 0)
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == 0, field
        assert lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)) == 0
        assert _plan(lib, d)[0] == 0
        d.qk_dim = 512
        assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3


def test_plan_hook_capacity_contract():
    lib = _capi.load()
    d = _fill()
    out = (ctypes.c_int32 * 6)()
    assert lib.aule_hip_debug_mla_plan(ctypes.byref(d), None, 0) == -6
    assert lib.aule_hip_debug_mla_plan(ctypes.byref(d), out, 5) == -6 and list(out) == [0] * 6
    assert lib.aule_hip_debug_mla_plan(ctypes.byref(d), out, 6) == 6


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(_fill())) == -1
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(_fill(decode=True, T=8))) == -1
    d = _fill(T=2, B=1, max_sq=2)   # a split plan without a workspace: the library would allocate
    d.lse = None
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -1


def test_plan_invariants_over_a_sweep():
    """(256 compute units: what the hook assumes without a device, and what an MI355X has)"""
    lib = _capi.load()
    seen_split = seen_single = 0
    for B in (1, 2, 3, 7, 8, 16, 33, 64):
        for Hq in (1, 5, 16, 128):
            for sq in (1, 2, 3, 4):
                for cap in (64, 128, 512, 2048, 8192, 131072):
                    T = B * sq + 3
                    d = _fill(T=T, B=B, Hq=Hq, bs=64, max_blocks=cap // 64, max_sq=sq)
                    n, (rb, rows, nsplit, grid, lo, hi) = _plan(lib, d)
                    key = (B, Hq, sq, cap)
                    assert n == 6 and rows == 64, key
                    assert rb == (sq * Hq + 63) // 64, key
                    assert 1 <= nsplit <= MAX_SPLIT and grid == rb * nsplit * B, key
                    if rb * B >= 256:
                        assert nsplit == 1, key
                    # a split is worth a workgroup only with keys to read: at most one per two 64-key tiles of the capacity
                    assert nsplit == max(1, min(-(-256 // (rb * B)), MAX_SPLIT, cap // 128)), key
                    ws = (lo & 0xffffffff) | (hi << 32)
                    assert ws == _ws_formula(nsplit, T, Hq) == lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d)), key
                    seen_split += nsplit > 1
                    seen_single += nsplit == 1
    assert seen_split > 100 and seen_single > 100
    n, plan = _plan(lib, _fill(T=1, B=1, Hq=16, bs=64, max_blocks=32, decode=True))
    assert n == 6 and plan[2] >= 2   # batch 1, heads 16, capacity 2048
    n, plan = _plan(lib, _fill(T=300, B=300, Hq=16, bs=64, max_blocks=1, decode=True))
    assert n == 6 and plan[:4] == [1, 64, 1, 300] and plan[4:] == [0, 0]
    # null offsets: one token per sequence whatever max_seqlen_q says; the block size does not enter but through the capacity
    a = _plan(lib, _fill(T=8, B=8, Hq=128, max_sq=4, decode=True))
    assert a == _plan(lib, _fill(T=8, B=8, Hq=128, max_sq=1)) and a[1][0] == 2
    assert _plan(lib, _fill(T=8, B=2, bs=24, max_blocks=86)) == _plan(lib, _fill(T=8, B=2, bs=8, max_blocks=258))


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_mla_paged with CPU tensors: every rule is checked before a device is touched; a well-formed CPU
    call is an AuleError (no fallback)."""
    import torch
    T, B, Hq, bs, nb = 6, 3, 16, 16, 12
    q = torch.zeros(T, Hq, 576, dtype=torch.bfloat16)
    kv = torch.zeros(nb, bs, 576, dtype=torch.bfloat16)
    bt = torch.zeros(B, 4, dtype=torch.int32)
    cl = torch.tensor([5, 9, 20], dtype=torch.int32)
    cu = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    call = aule.flash_attention_mla_paged
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,576\]"):
        call(q[0], kv, bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,576\]"):
        call(q, kv.view(nb, bs, 2, 288), bt, cl, cu)
    with pytest.raises(ValueError, match="latent width must be 576"):
        call(q[..., :512], kv[..., :512], bt, cl, cu)
    with pytest.raises(ValueError, match="latent width must be 576"):
        call(q, kv[..., :512], bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 / bf16"):
        call(q.float(), kv.float(), bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 / bf16"):
        call(q, kv.to(torch.float16), bt, cl, cu)
    with pytest.raises(ValueError, match="block_size must be positive"):
        call(q, kv[:, :0], bt, cl, cu)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        call(q, kv, bt, cl[:2], cu)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        call(q, kv, bt[:, :0], cl, cu)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        call(q, kv, bt, cl)   # plain decode: q.shape[0] must be the batch
    for bad in (cu[:3], cu.view(1, 4), [0, 2, 4, 6]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\]"):
            call(q, kv, bt, cl, bad)
    for bad in (cu.long(), cu.float()):
        with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
            call(q, kv, bt, cl, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, kv, bt, cl, cu, max_seqlen_q=bad)
    with pytest.raises(ValueError, match="max_seqlen_q must be None or 1 without cu_seqlens_q"):
        call(q[:3], kv, bt, cl, max_seqlen_q=2)
    wide = torch.zeros(T, Hq * 576 + 4, dtype=torch.bfloat16)[:, :Hq * 576].view(T, Hq, 576)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        call(wide, kv, bt, cl, cu)
    # well-formed, on the CPU: ragged, plain decode, the 4-d cache, a slice of a wider projection
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, kv, bt, cl, cu, max_seqlen_q=2, return_lse=True)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q[:3], kv.view(nb, bs, 1, 576), bt, cl, scale=192 ** -0.5)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(torch.zeros(T, Hq + 2, 576, dtype=torch.bfloat16)[:, :Hq], kv, bt, cl, cu)


def test_build_rule_names_the_new_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fa_fwd_mla_paged_gfx950.hip" in srcs
    dep = re.search(r"^\$\(OBJDIR\)/fa_fwd_mla_paged_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert "fa_d256_common.h" in dep
    assert os.path.exists(os.path.join(CSRC, "fa_fwd_mla_paged_gfx950.hip"))


def test_mla_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fp16 and bf16 of the attention kernel and of the combine: no scratch, no VGPR or SGPR spill, LDS within a compute unit's 160 KiB
    (DESIGN.md 3.9 states the budget: 111 616 bytes)"""
    res = resource_report("fa_fwd_mla_paged_gfx950.hip", tmp_path)
    for name in ("fa_fwd_mla_paged_kernel", "fa_mla_combine_kernel"):
        ks = [n for n in res if name in n]
        assert len(ks) == 2 and sum("Bf16Traits" in n for n in ks) == 1, (name, ks)
        for n in ks:
            r_ = res[n]
            assert r_.get("ScratchSize") == 0, (n, r_)
            assert r_.get("VGPRs Spill") == 0, (n, r_)
            assert r_.get("SGPRs Spill") == 0, (n, r_)
            assert r_.get("LDS Size") <= 160 * 1024, (n, r_)
    assert all(res[n]["LDS Size"] == 111616 for n in res if "fa_fwd_mla_paged_kernel" in n)
