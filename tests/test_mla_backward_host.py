"""The MLA 192 / 128 backward (aule_attention_mla_prefill_backward_ex, aule.flash_attention_mla_varlen) without a GPU: the three new
C symbols and the Python entry, the descriptor layout (ctypes == header comments == static_asserts, the problem statement at the
forward descriptor's offsets), every answer the entry gives before it needs a device, the workspace-size query, the launch plan's
invariants through the debug hook, the argument errors of the torch layer, the build rules and a resource audit of the kernels
compiled with the Makefile's compiler and flags (no scratch, no spill, the LDS DESIGN.md 3.11 states).  This file builds no sanitizer
library; tests/test_capi_sanitizers.py does, with the whole suite."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

import aule
from aule import _capi
from test_mla_prefill_host import LAYOUT as FWD_LAYOUT
from util import resource_report

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
SRC = "fa_bwd_mla_prefill_gfx950.hip"
ENTRY = "aule_attention_mla_prefill_backward_ex"
SIZE_QUERY = "aule_attention_mla_prefill_backward_workspace_size"
HOOK = "aule_hip_debug_mla_prefill_backward_plan"
PREFIX = [n for n in FWD_LAYOUT if n not in ("out", "lse")]
OWN = dict(out=160, lse=168, dout=176, dq=184, dk_nope=192, dk_pe=200, dv=208, dk_nope_token_stride=216, dk_nope_head_stride=224,
           dv_token_stride=232, dv_head_stride=240, workspace=248, workspace_bytes=256)
SIZE = 264
PTRS = ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "dout", "dq", "dk_nope", "dk_pe", "dv")
PLAN = ("heads_per_chunk", "n_chunks", "max_chunks", "delta_grid", "dq_grid", "dkdv_grid", "reduce_grid", "reduce", "ws_lo", "ws_hi")
LDS_DQ, LDS_DKDV = 47104, 25856   # 64 keys x (464 B of K + 272 B of V); 32 rows x (464 B of Q + 336 B of dO) + 2 x 32 floats


def _fill(Tq=700, Tk=900, B=3, H=16, max_sq=512, max_sk=640, dtype=2, causal=1):
    """a well-formed descriptor -- k_nope / v and dk_nope / dv the halves of [Tk, H, 256] tensors, k_pe columns 512.. of a [Tk, 576] one
    -- whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.MlaPrefillBwdDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads, d.qk_dim, d.v_dim = dtype, B, H, 192, 128
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = Tq, Tk, max_sq, max_sk
    d.causal = causal
    d.q_token_stride = H * 192
    d.k_nope_token_stride = d.v_token_stride = d.dk_nope_token_stride = d.dv_token_stride = H * 256
    d.k_nope_head_stride = d.v_head_stride = d.dk_nope_head_stride = d.dv_head_stride = 256
    d.k_pe_token_stride = 576
    for n in PTRS:
        setattr(d, n, 4096)
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _plan(lib, d):
    out = (ctypes.c_int32 * 10)()
    n = lib.aule_hip_debug_mla_prefill_backward_plan(ctypes.byref(d), out, 10)
    if n <= 0:
        return n
    assert n == 10
    plan = dict(zip(PLAN, out))
    plan["ws_bytes"] = (plan["ws_lo"] & 0xffffffff) | (plan["ws_hi"] << 32)
    return plan


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    assert re.search(r"\bint32_t %s\s*\(const aule_mla_prefill_bwd_desc\*" % ENTRY, header)
    assert re.search(r"\buint64_t %s\s*\(const aule_mla_prefill_bwd_desc\*" % SIZE_QUERY, header)
    assert re.search(r"\bint32_t %s\s*\(const aule_mla_prefill_bwd_desc\* desc, int32_t\* out, int32_t cap\)" % HOOK, header)
    for name, res in ((ENTRY, ctypes.c_int32), (SIZE_QUERY, ctypes.c_uint64), (HOOK, ctypes.c_int32)):
        assert hasattr(lib, name) and name in bound and bound[name][1] is res, name
    assert "flash_attention_mla_varlen" in aule.__all__ and callable(aule.flash_attention_mla_varlen)
    sig = inspect.signature(aule.flash_attention_mla_varlen)
    assert list(sig.parameters) == ["q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k", "causal",
                                    "scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["max_seqlen_k"].default is None and p["causal"].default is True
    assert p["scale"].default is None and p["return_lse"].default is False
    assert sig == inspect.signature(aule.flash_attention_mla_prefill)
    # the forward descriptor's comment keeps the word and points at the new entry
    not_built = header.split("typedef struct aule_mla_prefill_desc {")[0].rsplit("/* MLA PREFILL (additive)", 1)[1].split("Not built:")[1]
    assert "backward" in not_built and ENTRY in not_built


def test_descriptor_layout_matches_the_header():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    cls = _capi.MlaPrefillBwdDesc
    assert "sizeof(aule_mla_prefill_bwd_desc) = %d" % SIZE in header
    assert "sizeof(aule_mla_prefill_bwd_desc) == %d" % SIZE in capi
    assert ctypes.sizeof(cls) == SIZE and ctypes.sizeof(_capi.MlaPrefillDesc) == 176
    assert "sizeof(aule_mla_prefill_desc) == 176" in capi
    assert [n for n, _ in cls._fields_] == PREFIX + list(OWN)
    for name in PREFIX:   # the problem statement, at the forward descriptor's offsets
        assert getattr(cls, name).offset == FWD_LAYOUT[name] == getattr(_capi.MlaPrefillDesc, name).offset, name
        if name != "struct_size":
            assert "AULE_MLA_PREFILL_SAME(%s)" % name in capi, name
    for name, off in OWN.items():
        assert getattr(cls, name).offset == off, name
    body = header.split("typedef struct aule_mla_prefill_bwd_desc {")[1].split("}")[0]
    quoted = dict(re.findall(r"(\w+);\s*/\* offset (\d+)", body))
    pinned = dict(re.findall(r"offsetof\(aule_mla_prefill_bwd_desc, (\w+)\) == (\d+)", capi))
    assert set(quoted) == set(pinned) == set(OWN)
    for name in OWN:
        assert OWN[name] == int(quoted[name]) == int(pinned[name]), name
    # the fields of the header's struct, in order
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body)) == PREFIX + list(OWN)


# (field, bad value, a piece of the reason); H = 16: a q token is 3072 elements, a k_nope / v / dk_nope / dv token (15 * 256 + 128) = 3968
BAD = [
    ("struct_size", 0, "struct_size"), ("struct_size", 176, "struct_size"), ("struct_size", 272, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("qk_dim", 256, "qk_dim 256 / v_dim 128 unsupported"), ("v_dim", 192, "qk_dim 192 / v_dim 192 unsupported"),
    ("causal", 3, "unknown causal mode 3"), ("causal", -1, "unknown causal mode -1"),
    ("max_seqlen_q", 0, "max_seqlen_q must be at least 1"), ("max_seqlen_k", 0, "max_seqlen_k must be at least 1"),
    ("q_token_stride", 3072 - 8, "q_token_stride (3064) is smaller than a token, heads * 192 = 3072"), ("q_token_stride", 3072 + 4, "q_token_stride (3076) must be a multiple of 8"),
    ("k_nope_head_stride", 120, "k_nope_head_stride (120) is smaller than a head = 128"), ("k_nope_head_stride", 1 << 30, "too large"),
    ("v_head_stride", 258, "v_head_stride (258) must be a multiple of 8"),
    ("k_nope_token_stride", 3968 - 8, "k_nope_token_stride (3960) is smaller than a token, (heads - 1) * k_nope_head_stride + 128 = 3968"),
    ("v_token_stride", 4096 + 12, "v_token_stride (4108) must be a multiple of 8"),
    ("k_pe_token_stride", 56, "k_pe_token_stride (56) is smaller than a token = 64"), ("k_pe_token_stride", 68, "k_pe_token_stride (68) must be a multiple of 8"),
    ("total_q", 1 << 30, "too large"), ("total_k", 1 << 30, "too large"), ("batch", 1 << 30, "too large"), ("heads", 1 << 30, "too large"),
    # the backward's own: output strides, pointers, workspace
    ("dk_nope_head_stride", 120, "dk_nope_head_stride (120) is smaller than a head = 128"), ("dk_nope_head_stride", 132, "dk_nope_head_stride (132) must be a multiple of 8"),
    ("dk_nope_head_stride", -256, "dk_nope_head_stride (-256) is smaller"), ("dk_nope_head_stride", 1 << 30, "too large"),
    ("dv_head_stride", 0, "dv_head_stride (0) is smaller than a head = 128"), ("dv_head_stride", 258, "dv_head_stride (258) must be a multiple of 8"),
    ("dv_head_stride", 1 << 31, "too large"),
    ("dk_nope_token_stride", 3968 - 8, "dk_nope_token_stride (3960) is smaller than a token, (heads - 1) * dk_nope_head_stride + 128 = 3968"),
    ("dk_nope_token_stride", 4096 + 2, "dk_nope_token_stride (4098) must be a multiple of 8"), ("dk_nope_token_stride", -8, "dk_nope_token_stride (-8) is smaller"),
    ("dv_token_stride", 0, "dv_token_stride (0) is smaller than a token, (heads - 1) * dv_head_stride + 128 = 3968"),
    ("dv_token_stride", 4096 + 12, "dv_token_stride (4108) must be a multiple of 8"),
    ("cu_seqlens_q", None, "null cu_seqlens pointer"), ("cu_seqlens_k", None, "null cu_seqlens pointer"),
    ("q", None, "null tensor pointer"), ("k_nope", None, "null tensor pointer"), ("k_pe", None, "null tensor pointer"), ("v", None, "null tensor pointer"),
    ("out", None, "null tensor pointer"), ("lse", None, "null tensor pointer"), ("dout", None, "null tensor pointer"), ("dq", None, "null tensor pointer"),
    ("dk_nope", None, "null tensor pointer"), ("dk_pe", None, "null tensor pointer"), ("dv", None, "null tensor pointer"),
    ("q", 4096 + 8, "16-byte aligned"), ("k_pe", 4096 + 4, "16-byte aligned"), ("out", 4096 + 8, "16-byte aligned"), ("dout", 4097, "16-byte aligned"),
    ("dq", 4096 + 2, "16-byte aligned"), ("dk_nope", 4096 + 8, "16-byte aligned"), ("dk_pe", 4096 + 4, "16-byte aligned"), ("dv", 4096 + 8, "16-byte aligned"),
    ("lse", 4096 + 2, "lse must be 4-byte aligned"), ("workspace", 4096 + 8, "workspace must be 16-byte aligned"),
]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD, ids=_ids)
def test_entry_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library); the size query
    answers 0 and the hook -3 for what it can see (neither reads a pointer)"""
    lib = _capi.load()
    d = _fill()
    d.workspace, d.workspace_bytes = 8192, 1 << 40
    setattr(d, field, bad)
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA prefill backward failed: "), _error(lib)
    if field not in PTRS + ("workspace",):
        assert lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)) == 0
        assert _plan(lib, d) == -3


def test_null_descriptor_workspace_too_small_and_sizes_beyond_32_bits():
    lib = _capi.load()
    assert lib.aule_attention_mla_prefill_backward_ex(None) == -3 and _error(lib) == "MLA prefill backward failed: bad descriptor (struct_size mismatch)"
    assert lib.aule_attention_mla_prefill_backward_workspace_size(None) == 0 and lib.aule_hip_debug_mla_prefill_backward_plan(None, None, 0) == -3
    d = _fill()
    need = int(lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)))
    assert need > 0
    d.workspace, d.workspace_bytes = 8192, need - 1
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3
    assert "workspace too small (%d bytes, need %d)" % (need - 1, need) in _error(lib)
    # ceil(max_seqlen_q / 128) * heads * batch workgroups must fit 31 bits: 2^23 blocks x 16 heads x 16 sequences = 2^31
    d = _fill(Tq=(1 << 30) - 1, max_sq=1 << 30, B=16)
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3
    assert "2^31 - 1 workgroups" in _error(lib) and "32 bits" in _error(lib)
    assert lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)) == 0 and _plan(lib, d) == -3
    # the capacity contract of the plan hook: the ints needed, negated
    d = _fill()
    out = (ctypes.c_int32 * 10)()
    assert lib.aule_hip_debug_mla_prefill_backward_plan(ctypes.byref(d), out, 9) == -10
    assert lib.aule_hip_debug_mla_prefill_backward_plan(ctypes.byref(d), None, 10) == -10
    assert lib.aule_hip_debug_mla_prefill_backward_plan(ctypes.byref(d), out, 10) == 10


def test_nothing_to_do_returns_zero_without_a_launch():
    """batch = 0, heads = 0, or total_q = 0 and total_k = 0: 0, with null pointers, in any process.  A refused field is still refused."""
    lib = _capi.load()
    for fields in (("batch",), ("heads",), ("total_q", "total_k")):
        d = _fill()
        for f in fields:
            setattr(d, f, 0)
        if fields == ("heads",):
            d.q_token_stride = 0
            d.k_nope_token_stride = d.v_token_stride = d.dk_nope_token_stride = d.dv_token_stride = 128
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == 0, fields
        assert lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)) == 0 and _plan(lib, d) == 0
        d.causal = 7
        assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3, fields
    # one empty side: the other side's pointers are required, this side's are not
    d = _fill(Tq=0)
    d.q = d.out = d.lse = d.dout = d.dq = None
    d.dk_pe = None
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)
    d = _fill(Tk=0)
    d.k_nope = d.k_pe = d.v = d.dk_nope = d.dk_pe = d.dv = None
    d.dq = None
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(_fill())) == -1
    d = _fill(causal=2, dtype=1)
    d.workspace, d.workspace_bytes = 8192, int(lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)))
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -1
    d = _fill(Tq=0)
    d.q = d.out = d.lse = d.dout = d.dq = None
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -1
    d = _fill(Tk=0)
    d.k_nope = d.k_pe = d.v = d.dk_nope = d.dk_pe = d.dv = None
    assert lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)) == -1


HEADS = (1, 2, 5, 16, 17, 128)
TOTALS = (1, 127, 128, 129, 1000, 4096, 65536)
BATCHES = (1, 2, 7, 64)


def test_plan_invariants_and_the_workspace_size():
    """over heads x total_k x batch (x two maxima x two total_q): the chunks tile the heads exactly with a possibly short last chunk,
    n_chunks and the workspace stay within the bound the plan states, the grids are the stated products and fit 31 bits, and the size
    query is delta rounded to 256 bytes plus n_chunks * total_k * 64 * 4 when the reduce runs"""
    lib = _capi.load()
    seen = set()
    for H in HEADS:
        for Tk in TOTALS:
            for B in BATCHES:
                for max_sk in (Tk, max(1, Tk // B)):
                    for Tq in (Tk, 0):
                        d = _fill(Tq=Tq, Tk=Tk, B=B, H=H, max_sq=max(1, min(Tq, 4096)), max_sk=max_sk)
                        d.q_token_stride = H * 192
                        d.k_nope_token_stride = d.v_token_stride = d.dk_nope_token_stride = d.dv_token_stride = H * 256
                        pl = _plan(lib, d)
                        case = (H, Tk, B, max_sk, Tq)
                        assert isinstance(pl, dict), case
                        hpc, nch = pl["heads_per_chunk"], pl["n_chunks"]
                        assert hpc >= 1 and 1 <= nch <= pl["max_chunks"] == 16 and nch <= H, (case, pl)
                        assert (nch - 1) * hpc < H <= nch * hpc, (case, pl)     # exact tiling, the last chunk 1 .. hpc heads
                        kblocks, qblocks = (min(max_sk, Tk) + 127) // 128, (min(d.max_seqlen_q, Tq) + 127) // 128 if Tq else 0
                        assert pl["dkdv_grid"] == kblocks * B * nch and pl["dq_grid"] == qblocks * H * B and pl["delta_grid"] == (Tq * H + 3) // 4, (case, pl)
                        assert pl["reduce"] == (1 if nch > 1 else 0) and pl["reduce_grid"] == (kblocks * B if nch > 1 else 0), (case, pl)
                        for g in ("delta_grid", "dq_grid", "dkdv_grid", "reduce_grid"):
                            assert 0 <= pl[g] < 2 ** 31, (case, pl)
                        delta = (Tq * H * 4 + 255) // 256 * 256
                        want = delta + (nch * Tk * 64 * 4 if pl["reduce"] else 0)
                        assert pl["ws_bytes"] == want <= delta + pl["max_chunks"] * Tk * 64 * 4, (case, pl)
                        assert int(lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d))) == want, case
                        seen.add((nch > 1, H % hpc != 0, hpc > 1))
    # both plans occur, and chunks of several heads with a short last one
    assert {s[0] for s in seen} == {False, True} and (True, True, True) in seen and (False, False, True) in seen, seen


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_mla_varlen with CPU tensors: the forward entry's list; a well-formed CPU call is an AuleError (no
    fallback), with and without requires_grad"""
    import torch
    Tq, Tk, H = 10, 12, 4
    z = lambda *s, dt=torch.float16: torch.zeros(*s, dtype=dt)   # noqa: E731
    q, kn, kp, v = z(Tq, H, 192), z(Tk, H, 128), z(Tk, 64), z(Tk, H, 128)
    cq = torch.tensor([0, 5, 10], dtype=torch.int32)
    ck = torch.tensor([0, 6, 12], dtype=torch.int32)
    call = aule.flash_attention_mla_varlen
    for bad in ((q.reshape(2, 5, H, 192), kn, kp, v), (q, kn[0], kp, v), (q, kn, kp.reshape(Tk, 2, 32), v), (q, kn, kp, v[0]), (None, kn, kp, v)):
        with pytest.raises(ValueError, match=r"expected q \[total_q, heads, 192\]"):
            call(*bad, cq, ck)
    for bad in ((z(Tq, H, 256), kn, kp, v), (q, z(Tk, H, 192), kp, v), (q, kn, z(Tk, 128), v), (q, kn, kp, z(Tk, H, 192)), (q[..., :128], kn, kp, v)):
        with pytest.raises(ValueError, match="192 / 128 / 128 / 64 exactly"):
            call(*bad, cq, ck)
    with pytest.raises(ValueError, match="one heads count"):
        call(q, z(Tk, 1, 128), kp, z(Tk, 1, 128), cq, ck)
    with pytest.raises(ValueError, match="one total_k"):
        call(q, kn, kp[:8], v, cq, ck)
    with pytest.raises(ValueError, match="not built"):
        call(q.float(), kn.float(), kp.float(), v.float(), cq, ck)
    for i in range(1, 4):
        args = [q, kn, kp, v]
        args[i] = args[i].to(torch.bfloat16)
        with pytest.raises(ValueError, match="share one dtype"):
            call(*args, cq, ck)
    for bad in (cq.view(1, 3), [0, 5, 10], cq[:0]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] tensor"):
            call(q, kn, kp, v, bad, ck)
    with pytest.raises(ValueError, match=r"must both be \[batch \+ 1\]"):
        call(q, kn, kp, v, cq, ck[:2])
    with pytest.raises(ValueError, match="cu_seqlens_k must be int32"):
        call(q, kn, kp, v, cq, ck.long())
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, kn, kp, v, cq, ck, max_seqlen_q=bad)
        with pytest.raises(ValueError, match="max_seqlen_k must be a positive int"):
            call(q, kn, kp, v, cq, ck, max_seqlen_k=bad)
    with pytest.raises(ValueError, match="causal must be"):
        call(q, kn, kp, v, cq, ck, causal="diagonal")
    # well-formed, on the CPU: no fallback, whether or not a gradient is asked for (the forward-only entry refuses the latter)
    kvb, down = z(Tk, H, 256), z(Tk, 576)
    for args in ((q, kn, kp, v), (q, kn, kp.view(Tk, 1, 64), v), (q, kvb[..., :128], down[:, 512:], kvb[..., 128:])):
        for causal in (False, True, "bottom-right"):
            with pytest.raises(aule.AuleError, match="no CPU fallback"):
                call(*args, cq, ck, causal=causal, return_lse=True, max_seqlen_q=5, max_seqlen_k=6)
    for i in range(4):
        args = [q, kn, kp, v]
        args[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(*args, cq, ck)
        with pytest.raises(ValueError, match="no backward"):
            aule.flash_attention_mla_prefill(*args, cq, ck)


def test_build_rules_name_the_new_source():
    """csrc/Makefile: the file in SRCS (so `make`, `make dbg` and `make san` compile it) with its header dependencies; the
    variable-length backward and the MLA prefill forward know nothing of it, and it reads no environment"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert SRC in srcs
    dep = re.search(r"^\$\(OBJDIR\)/fa_bwd_mla_prefill_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert {"fa_mla_prefill_common.h", "fa_varlen_common.h", "fa_tile_attention.h", "fa_paged_tile.h", "fa_d256_common.h"} <= set(dep)
    src = open(os.path.join(CSRC, SRC)).read()
    assert '#include "fa_mla_prefill_common.h"' in src and "getenv" not in src and "fa_switches.h" not in src
    body = open(os.path.join(CSRC, "fa_varlen_common.h")).read()
    assert '#include "fa_varlen_common.h"' in src and "ragged_dq_body<" in src and "seq_range(" in src and "RowTile<" in src
    assert "query_block(" in body[body.index("void ragged_dq_body("):]
    for text in (src, body, open(os.path.join(CSRC, "fa_mla_prefill_common.h")).read(), open(os.path.join(CSRC, "fa_tile_attention.h")).read()):
        assert "atomicAdd" not in text and "__hip_atomic" not in text
    assert "mla" not in open(os.path.join(CSRC, "fa_bwd_varlen_gfx950.hip")).read()
    assert "bwd" not in open(os.path.join(CSRC, "fa_fwd_mla_prefill_gfx950.hip")).read()


def test_mla_backward_kernels_neither_spill_nor_use_scratch(tmp_path):
    """eight kernels (delta, dQ, dK/dV, reduce; fp16 and bf16): no scratch, no VGPR or SGPR spill, the LDS DESIGN.md 3.11 states"""
    res = resource_report(SRC, tmp_path)
    kinds = {"fa_bwd_mla_delta_kernel": 0, "fa_bwd_mla_dq_kernel": LDS_DQ, "fa_bwd_mla_dkdv_kernel": LDS_DKDV, "fa_bwd_mla_dkpe_reduce_kernel": 0}
    assert len(res) == 8, sorted(res)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design.split("### 3.11")[1].split("\n### ")[0]
    assert "47 104" in section and "25 856" in section
    for kind, lds in kinds.items():
        ks = [n for n in res if kind in n]
        assert len(ks) == 2 and sum("Bf16Traits" in n for n in ks) == 1 and sum("F16Traits" in n for n in ks) == 1, (kind, sorted(res))
        for n in ks:
            r_ = res[n]
            print(n, r_)
            assert r_.get("ScratchSize") == 0, (n, r_)
            assert r_.get("VGPRs Spill") == 0, (n, r_)
            assert r_.get("SGPRs Spill") == 0, (n, r_)
            assert r_.get("LDS Size") == lds < 64 * 1024, (n, r_)
