"""MLA prefill (the non-absorbed 192 / 128 form over a packed batch) without a GPU: the additive C-ABI (symbol, descriptor layout,
every answer the entry gives before it needs a device), the argument errors of the torch layer, the build rules (the file in the
Makefile's source list, from which `make dbg` and `make san` build too; this file builds no sanitizer library itself --
tests/test_capi_sanitizers.py does, with the whole suite) and a resource audit of the two kernels, compiled with the Makefile's
compiler and flags (no scratch, no spill, the LDS DESIGN.md 3.10 states)."""
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
ENTRY = "aule_attention_mla_prefill_ex"
PTRS = ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse")
LAYOUT = dict(struct_size=0, dtype=4, batch=8, heads=12, qk_dim=16, v_dim=20, total_q=24, total_k=28, max_seqlen_q=32, max_seqlen_k=36,
              scale=40, causal=44, device=48, reserved=52, q_token_stride=56, k_nope_token_stride=64, k_nope_head_stride=72,
              v_token_stride=80, v_head_stride=88, k_pe_token_stride=96, stream=104, q=112, k_nope=120, k_pe=128, v=136,
              cu_seqlens_q=144, cu_seqlens_k=152, out=160, lse=168)
SIZE = 176
LDS_BYTES = 46080   # 64 keys x (400 B of K + 320 B of V): the number DESIGN.md 3.10 states


def _fill(Tq=700, Tk=900, B=3, H=16, max_sq=512, max_sk=640, dtype=2, causal=1):
    """a well-formed descriptor -- k_nope and v the two halves of a [Tk, H, 256] tensor, k_pe columns 512.. of a [Tk, 576] one -- whose
    pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.MlaPrefillDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads, d.qk_dim, d.v_dim = dtype, B, H, 192, 128
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = Tq, Tk, max_sq, max_sk
    d.causal = causal
    d.q_token_stride = H * 192
    d.k_nope_token_stride = d.v_token_stride = H * 256
    d.k_nope_head_stride = d.v_head_stride = 256
    d.k_pe_token_stride = 576
    for n in PTRS:
        setattr(d, n, 4096)
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    assert re.search(r"\bint32_t %s\s*\(const aule_mla_prefill_desc\*" % ENTRY, header)
    assert hasattr(lib, ENTRY) and ENTRY in bound and bound[ENTRY][1] is ctypes.c_int32
    assert "flash_attention_mla_prefill" in aule.__all__ and callable(aule.flash_attention_mla_prefill)
    sig = inspect.signature(aule.flash_attention_mla_prefill)
    assert list(sig.parameters) == ["q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "causal",
                                    "scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["max_seqlen_k"].default is None and p["causal"].default is True
    assert p["scale"].default is None and p["return_lse"].default is False
    # the contract is stated at the descriptor, with what is not built
    comment = header.split("typedef struct aule_mla_prefill_desc {")[0].rsplit("/* MLA PREFILL (additive)", 1)[1]
    not_built = comment.split("Not built:")[1]
    for word in ("backward", "window", "GQA", "FP8", "rotation", "key-range splits"):
        assert word in not_built, word


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert"""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    cls = _capi.MlaPrefillDesc
    assert "sizeof(aule_mla_prefill_desc) = %d" % SIZE in header
    assert "sizeof(aule_mla_prefill_desc) == %d" % SIZE in capi
    assert ctypes.sizeof(cls) == SIZE
    assert [n for n, _ in cls._fields_] == list(LAYOUT)
    for name, off in LAYOUT.items():
        assert getattr(cls, name).offset == off, name
    body = header.split("typedef struct aule_mla_prefill_desc {")[1].split("}")[0]
    quoted = dict(re.findall(r"(\w+);\s*/\* offset (\d+)", body))
    assert set(quoted) == set(LAYOUT) - {"struct_size"}
    pinned = dict(re.findall(r"offsetof\(aule_mla_prefill_desc, (\w+)\) == (\d+)", capi))
    assert set(pinned) == set(LAYOUT) - {"struct_size"}
    for name in quoted:
        assert LAYOUT[name] == int(quoted[name]) == int(pinned[name]), name
    # existing descriptors keep their sizes
    assert ctypes.sizeof(_capi.VarlenDesc) == 144 and ctypes.sizeof(_capi.MlaPagedDesc) == 136 and ctypes.sizeof(_capi.MergeStatesDesc) == 80


# (field, bad value, a piece of the reason); H = 16: a q token is 3072 elements, a k_nope / v token (15 * 256 + 128) = 3968
BAD = [
    ("struct_size", 0, "struct_size"), ("struct_size", 8, "struct_size"), ("struct_size", 144, "struct_size"), ("struct_size", 184, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"), ("dtype", -1, "fp16 or bf16"),
    ("qk_dim", 256, "qk_dim 256 / v_dim 128 unsupported"), ("qk_dim", 0, "qk_dim 0"), ("v_dim", 192, "qk_dim 192 / v_dim 192 unsupported"),
    ("v_dim", 512, "v_dim 512"),
    ("causal", 3, "unknown causal mode 3"), ("causal", -1, "unknown causal mode -1"),
    ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"), ("max_seqlen_k", 0, "max_seqlen_k must be at least 1"),
    ("q_token_stride", 3072 - 8, "q_token_stride (3064) is smaller than a token, heads * 192 = 3072"), ("q_token_stride", 0, "q_token_stride (0) is smaller"),
    ("q_token_stride", -3072, "q_token_stride (-3072) is smaller"), ("q_token_stride", 3072 + 4, "q_token_stride (3076) must be a multiple of 8"),
    ("k_nope_head_stride", 120, "k_nope_head_stride (120) is smaller than a head = 128"), ("k_nope_head_stride", 132, "k_nope_head_stride (132) must be a multiple of 8"),
    ("k_nope_head_stride", -256, "k_nope_head_stride (-256) is smaller"), ("k_nope_head_stride", 1 << 30, "too large"),
    ("v_head_stride", 0, "v_head_stride (0) is smaller than a head = 128"), ("v_head_stride", 258, "v_head_stride (258) must be a multiple of 8"),
    ("v_head_stride", 1 << 31, "too large"),
    ("k_nope_token_stride", 3968 - 8, "k_nope_token_stride (3960) is smaller than a token, (heads - 1) * k_nope_head_stride + 128 = 3968"),
    ("k_nope_token_stride", 4096 + 2, "k_nope_token_stride (4098) must be a multiple of 8"), ("k_nope_token_stride", -8, "k_nope_token_stride (-8) is smaller"),
    ("v_token_stride", 0, "v_token_stride (0) is smaller than a token, (heads - 1) * v_head_stride + 128 = 3968"),
    ("v_token_stride", 4096 + 12, "v_token_stride (4108) must be a multiple of 8"),
    ("k_pe_token_stride", 56, "k_pe_token_stride (56) is smaller than a token = 64"), ("k_pe_token_stride", 68, "k_pe_token_stride (68) must be a multiple of 8"),
    ("k_pe_token_stride", 0, "k_pe_token_stride (0) is smaller"),
    ("total_q", 1 << 30, "too large"), ("total_k", 1 << 30, "too large"), ("batch", 1 << 30, "too large"), ("heads", 1 << 30, "too large"),
    ("q", None, "null tensor pointer"), ("k_nope", None, "null tensor pointer"), ("k_pe", None, "null tensor pointer"), ("v", None, "null tensor pointer"),
    ("out", None, "null tensor pointer"), ("cu_seqlens_q", None, "null cu_seqlens pointer"), ("cu_seqlens_k", None, "null cu_seqlens pointer"),
    ("q", 4096 + 8, "16-byte aligned"), ("k_nope", 4097, "16-byte aligned"), ("k_pe", 4096 + 4, "16-byte aligned"), ("v", 4096 + 2, "16-byte aligned"),
    ("out", 4096 + 8, "out must be 16-byte aligned"), ("lse", 4096 + 2, "lse must be 4-byte aligned"),
]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD, ids=_ids)
def test_entry_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library)"""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA prefill failed: "), _error(lib)


def test_null_descriptor_and_sizes_beyond_32_bits():
    lib = _capi.load()
    assert lib.aule_attention_mla_prefill_ex(None) == -3 and _error(lib) == "MLA prefill failed: bad descriptor (struct_size mismatch)"
    # ceil(max_seqlen_q / 128) * heads * batch workgroups must fit 31 bits: 2^23 blocks x 16 heads x 16 sequences = 2^31
    d = _fill(Tq=(1 << 30) - 1, max_sq=1 << 30, B=16)
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -3
    assert _error(lib).startswith("MLA prefill failed: ") and "2^31 - 1 workgroups" in _error(lib) and "32 bits" in _error(lib)


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_q = 0, batch = 0 or heads = 0: 0, with null pointers, in any process.  A refused field is still refused."""
    lib = _capi.load()
    for field in ("total_q", "batch", "heads"):
        d = _fill()
        setattr(d, field, 0)
        if field == "heads":
            d.q_token_stride = 0
            d.k_nope_token_stride = d.v_token_stride = 128
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == 0, field
        d.causal = 7
        assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -3, field
    # without a key row the call writes zeros and -inf: k_nope, k_pe and v may be null (so the descriptor is accepted, see below), out may not
    d = _fill(Tk=0)
    d.k_nope = d.k_pe = d.v = None
    d.out = None
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(_fill())) == -1
    for causal in (0, 2):
        assert lib.aule_attention_mla_prefill_ex(ctypes.byref(_fill(causal=causal, dtype=1))) == -1
    d = _fill()
    d.lse = None
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -1
    d = _fill(Tk=0)
    d.k_nope = d.k_pe = d.v = None
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -1
    d = _fill(H=1)   # one head: any head stride from 128 up, a token is 128 elements
    d.q_token_stride, d.k_nope_token_stride, d.v_token_stride, d.k_nope_head_stride, d.v_head_stride, d.k_pe_token_stride = 192, 128, 128, 128, 1 << 20, 64
    assert lib.aule_attention_mla_prefill_ex(ctypes.byref(d)) == -1


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_mla_prefill with CPU tensors: every rule is checked before a device is touched; a well-formed CPU
    call is an AuleError (no fallback)."""
    import torch
    Tq, Tk, H = 10, 12, 4
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)   # noqa: E731
    q, kn, kp, v = z(Tq, H, 192), z(Tk, H, 128), z(Tk, 64), z(Tk, H, 128)
    cq = torch.tensor([0, 5, 10], dtype=torch.int32)
    ck = torch.tensor([0, 6, 12], dtype=torch.int32)
    call = aule.flash_attention_mla_prefill
    # shapes
    for bad in ((q.reshape(2, 5, H, 192), kn, kp, v), (q, kn[0], kp, v), (q, kn, kp.reshape(Tk, 2, 32), v), (q, kn, kp, v[0]), (None, kn, kp, v)):
        with pytest.raises(ValueError, match=r"expected q \[total_q, heads, 192\]"):
            call(*bad, cq, ck)
    for bad in ((z(Tq, H, 256), kn, kp, v), (q, z(Tk, H, 192), kp, v), (q, kn, z(Tk, 128), v), (q, kn, kp, z(Tk, H, 192)), (q[..., :128], kn, kp, v)):
        with pytest.raises(ValueError, match="192 / 128 / 128 / 64 exactly"):
            call(*bad, cq, ck)
    with pytest.raises(ValueError, match="one heads count"):
        call(q, z(Tk, 1, 128), kp, z(Tk, 1, 128), cq, ck)
    with pytest.raises(ValueError, match="one heads count"):
        call(q, kn, kp, z(Tk, 2, 128), cq, ck)
    with pytest.raises(ValueError, match="one total_k"):
        call(q, kn, kp[:8], v, cq, ck)
    with pytest.raises(ValueError, match="one total_k"):
        call(q, kn, kp, v[:8], cq, ck)
    # dtypes
    with pytest.raises(ValueError, match="not built"):
        call(q.float(), kn.float(), kp.float(), v.float(), cq, ck)
    for i in range(1, 4):
        args = [q, kn, kp, v]
        args[i] = args[i].to(torch.bfloat16)
        with pytest.raises(ValueError, match="share one dtype"):
            call(*args, cq, ck)
    # offsets, maxima and the causal mode: the rules of flash_attention_varlen
    for bad in (cq.view(1, 3), [0, 5, 10], cq[:0]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] tensor"):
            call(q, kn, kp, v, bad, ck)
    with pytest.raises(ValueError, match=r"cu_seqlens_k must be a \[batch \+ 1\] tensor"):
        call(q, kn, kp, v, cq, None)
    with pytest.raises(ValueError, match=r"must both be \[batch \+ 1\]"):
        call(q, kn, kp, v, cq, ck[:2])
    for bad in (cq.long(), cq.float()):
        with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
            call(q, kn, kp, v, bad, ck)
        with pytest.raises(ValueError, match="cu_seqlens_k must be int32"):
            call(q, kn, kp, v, cq, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, kn, kp, v, cq, ck, max_seqlen_q=bad)
        with pytest.raises(ValueError, match="max_seqlen_k must be a positive int"):
            call(q, kn, kp, v, cq, ck, max_seqlen_k=bad)
    with pytest.raises(ValueError, match="causal must be"):
        call(q, kn, kp, v, cq, ck, causal="diagonal")
    # no autograd
    for i in range(4):
        args = [q, kn, kp, v]
        args[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(ValueError, match="no backward"):
            call(*args, cq, ck)
    # well-formed, on the CPU: plain, k_pe [T, 1, 64], the in-place slices, and tensors that would be copied
    kvb, down = z(Tk, H, 256), z(Tk, 576)
    for args in ((q, kn, kp, v), (q, kn, kp.view(Tk, 1, 64), v), (q, kvb[..., :128], down[:, 512:], kvb[..., 128:]),
                 (q.transpose(0, 1).contiguous().transpose(0, 1), kn, z(64, Tk).t(), z(Tk, H, 132)[..., :128])):
        for causal in (False, True, "bottom-right"):
            with pytest.raises(aule.AuleError, match="no CPU fallback"):
                call(*args, cq, ck, causal=causal, return_lse=True, max_seqlen_q=5, max_seqlen_k=6)
    with torch.no_grad():
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q.clone().requires_grad_(True), kn, kp, v, cq, ck)


def test_in_place_rule_of_the_wrapper():
    """which tensors the wrapper reads in place and which it copies, and the strides it states (host logic on CPU tensors)"""
    import torch
    from aule import _torch as at
    T, H = 6, 4
    kvb = torch.zeros(T, H, 256, dtype=torch.bfloat16)
    for half in (kvb[..., :128], kvb[..., 128:]):
        x, ts, hs = at._mla_prefill_rows(half, True)
        assert x.data_ptr() == half.data_ptr() and (ts, hs) == (H * 256, 256)
    down = torch.zeros(T, 576, dtype=torch.bfloat16)
    x, ts, hs = at._mla_prefill_rows(down[:, 512:].unsqueeze(1), False)
    assert x.data_ptr() == down[:, 512:].data_ptr() and (ts, hs) == (576, 64)
    wide_q = torch.zeros(T, H * 192 + 16, dtype=torch.bfloat16)[:, :H * 192].view(T, H, 192)
    x, ts, hs = at._mla_prefill_rows(wide_q, False)
    assert x.data_ptr() == wide_q.data_ptr() and (ts, hs) == (H * 192 + 16, 192)
    # copied: a head stride on q, strides or offsets that are no multiples of 8, an innermost stride other than 1
    q_heads = torch.zeros(T, H, 200, dtype=torch.bfloat16)[..., :192]
    odd_head = torch.zeros(T, H, 132, dtype=torch.bfloat16)[..., :128]
    odd_token = torch.zeros(T, H * 128 + 4, dtype=torch.bfloat16)[:, :H * 128].view(T, H, 128)
    shifted = torch.zeros(T * H * 128 + 4, dtype=torch.bfloat16)[4:].view(T, H, 128)
    inner = torch.zeros(T, 128, H, dtype=torch.bfloat16).transpose(1, 2)
    for bad, free, W in ((q_heads, False, 192), (odd_head, True, 128), (odd_token, True, 128), (shifted, True, 128), (inner, True, 128)):
        x, ts, hs = at._mla_prefill_rows(bad, free)
        assert x.is_contiguous() and x.data_ptr() != bad.data_ptr() and (ts, hs) == (H * W, W)
    # one token, one head: the strides of extent-1 axes are not read
    one = torch.zeros(1, 1, 128, dtype=torch.bfloat16).as_strided((1, 1, 128), (7, 3, 1))
    x, ts, hs = at._mla_prefill_rows(one, True)
    assert x.data_ptr() == one.data_ptr() and (ts, hs) == (128, 128)


def test_build_rules_name_the_new_source():
    """csrc/Makefile: the file in SRCS (so `make`, `make dbg` and `make san` compile it) with its header dependencies; the variable-
    length forward keeps its six kernels (the new instances live in a file of their own) and the new file reads no environment"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "fa_fwd_mla_prefill_gfx950.hip" in srcs
    dep = re.search(r"^\$\(OBJDIR\)/fa_fwd_mla_prefill_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert {"fa_mla_prefill_common.h", "fa_varlen_common.h", "fa_tile_attention.h", "fa_paged_tile.h", "fa_d256_common.h"} <= set(dep)
    src = open(os.path.join(CSRC, "fa_fwd_mla_prefill_gfx950.hip")).read()
    assert '#include "fa_mla_prefill_common.h"' in src and "getenv" not in src and "fa_switches.h" not in src
    assert '#include "fa_varlen_common.h"' in src and "query_block(" in src and "x.visible(" in src
    common = open(os.path.join(CSRC, "fa_mla_prefill_common.h")).read()      # the tile source the backward reads too
    assert "MlaKeyTiles kt(" in src and "struct MlaKeyTiles" in common and "RowTile<" in common and "getenv" not in common
    assert "mla_prefill" not in open(os.path.join(CSRC, "fa_fwd_varlen_gfx950.hip")).read()


def test_mla_prefill_kernels_neither_spill_nor_use_scratch(tmp_path):
    """exactly two kernels (fp16, bf16): no scratch, no VGPR or SGPR spill, LDS = 46 080 bytes (DESIGN.md 3.10 states the budget)"""
    res = resource_report("fa_fwd_mla_prefill_gfx950.hip", tmp_path)
    ks = [n for n in res if "fa_fwd_mla_prefill_kernel" in n]
    assert len(res) == 2 and len(ks) == 2 and sum("Bf16Traits" in n for n in ks) == 1 and sum("F16Traits" in n for n in ks) == 1, sorted(res)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("### 3.10")[1].split("\n### ")[0]
    assert "46 080" in section
    for n in ks:
        r_ = res[n]
        print(n, r_)
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") == LDS_BYTES < 64 * 1024, (n, r_)
