"""The paged prefill (ragged per-sequence queries against the paged KV cache) without a GPU: the additive C-ABI (symbol,
descriptor layout, the answers the entry gives before it needs a device), the argument errors of the torch layer, and a
resource audit of the twelve kernel instances (no scratch, no VGPR or SGPR spill)."""
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
NAME = "aule_attention_paged_prefill_ex"
PTRS = ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out")


def _fill(T=700, B=3, Hq=32, Hkv=8, D=128, bs=16, max_blocks=64, max_sq=512, dtype=2, cache_dtype=0, window=-1):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer
    before a launch"""
    d = _capi.PagedPrefillDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = dtype, cache_dtype
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, Hkv, D
    d.block_size, d.max_blocks, d.window_size = bs, max_blocks, window
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, max_sq, Hq * D
    for n in PTRS:
        setattr(d, n, 4096)
    if cache_dtype == 1:
        d.k_scale = d.v_scale = 4096
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    assert re.search(r"\b%s\s*\(const aule_paged_prefill_desc\*" % NAME, header)
    assert hasattr(lib, NAME)
    assert NAME in {s[0] for s in _capi.SIGNATURES}
    assert "flash_attention_paged_prefill" in aule.__all__ and callable(aule.flash_attention_paged_prefill)
    sig = inspect.signature(aule.flash_attention_paged_prefill)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale",
                                    "window_size", "k_scale", "v_scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["scale"].default is None and p["window_size"].default == -1
    assert p["k_scale"].default is None and p["v_scale"].default is None and p["return_lse"].default is False


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    assert "sizeof(aule_paged_prefill_desc) = 152" in header
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_paged_prefill_desc) == 152" in capi
    D = _capi.PagedPrefillDesc
    assert ctypes.sizeof(D) == 152
    want = dict(struct_size=0, dtype=4, cache_dtype=8, batch=12, heads_q=16, heads_kv=20, head_dim=24, block_size=28, max_blocks=32,
                total_tokens=36, max_seqlen_q=40, scale=44, window_size=48, device=52, q_token_stride=56, stream=64, q=72, k_cache=80,
                v_cache=88, block_tables=96, context_lens=104, cu_seqlens_q=112, out=120, lse=128, k_scale=136, v_scale=144)
    assert [n for n, _ in D._fields_] == list(want)
    for name, off in want.items():
        assert getattr(D, name).offset == off, name
    body = header.split("typedef struct aule_paged_prefill_desc")[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 20
    for name, off in quoted:
        assert want[name] == int(off), name
    for name, off in re.findall(r"offsetof\(aule_paged_prefill_desc, (\w+)\) == (\d+)", capi):
        assert want[name] == int(off), name
    # the fields of the paged query's descriptor without seq_q and the workspace, plus the ragged ones
    theirs = {n for n, _ in _capi.PagedQueryDesc._fields_} - {"seq_q", "workspace", "workspace_bytes"}
    assert theirs | {"total_tokens", "max_seqlen_q", "q_token_stride", "cu_seqlens_q"} == set(want)


BAD_FIELDS = [
    ("struct_size", 0, "struct_size"), ("struct_size", 144, "struct_size"), ("struct_size", 160, "struct_size"),
    ("dtype", 0, "fp16 or bf16"), ("dtype", 3, "fp16 or bf16"),
    ("cache_dtype", 2, "cache_dtype"), ("cache_dtype", -1, "cache_dtype"),
    ("head_dim", 256, "head_dim 256"), ("head_dim", 48, "head_dim 48"), ("head_dim", 0, "head_dim 0"),
    ("heads_kv", 5, "divisible"), ("heads_kv", 0, "divisible"),
    ("block_size", 0, "block_size"), ("max_blocks", 0, "block_size"), ("max_blocks", 1 << 28, "block_size"),
    ("max_seqlen_q", 0, "max_seqlen_q"),
    ("q_token_stride", 32 * 128 - 8, "smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", -4096, "smaller than a token"), ("q_token_stride", 32 * 128 + 4, "multiple of 8"),
    ("total_tokens", 1 << 30, "too large"),
    ("q", None, "null tensor pointer"), ("k_cache", None, "null tensor pointer"), ("v_cache", None, "null tensor pointer"),
    ("block_tables", None, "null tensor pointer"), ("context_lens", None, "null tensor pointer"),
    ("cu_seqlens_q", None, "null tensor pointer"), ("out", None, "null tensor pointer"),
    ("k_scale", 4096, "FP8 caches only"), ("v_scale", 4096, "FP8 caches only"),
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("k_cache", 4097, "16-byte aligned"),
]


@pytest.mark.parametrize("field,bad,needle", BAD_FIELDS, ids=lambda x: str(x).replace(" ", "_"))
def test_entry_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason, before the device is needed (so also in a process that never initialised the library)."""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib), _error(lib)


def test_entry_refuses_fp8_without_scales_and_null():
    lib = _capi.load()
    assert lib.aule_attention_paged_prefill_ex(None) == -3
    for field in ("k_scale", "v_scale"):
        d = _fill(cache_dtype=1)
        setattr(d, field, None)
        assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == -3
        assert "scale pointer" in _error(lib)
    # the packed-row count must fit 32 bits: 2^29 tokens x 8 heads per KV head
    d = _fill(T=1 << 29, Hq=64, Hkv=8)
    d.q_token_stride = 64 * 128
    assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == -3
    assert "32 bits" in _error(lib)


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0, batch = 0 or heads_q = 0: 0, with null pointers, in any process."""
    lib = _capi.load()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill()
        setattr(d, field, 0)
        if field == "heads_q":
            d.q_token_stride = 0
        for n in PTRS:
            setattr(d, n, None)
        assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == 0, field
    # ... but a refused field is still refused
    d = _fill(T=0)
    d.head_dim = 256
    assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == -3


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    lib = _capi.load()
    for cache_dtype in (0, 1):
        assert lib.aule_attention_paged_prefill_ex(ctypes.byref(_fill(cache_dtype=cache_dtype))) == -1


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_paged_prefill with CPU tensors: every rule is checked before the library is loaded or a
    device touched; a well-formed CPU call is an AuleError (no fallback)."""
    import torch
    B, T, Hq, Hkv, D, bs = 2, 10, 8, 2, 64, 16
    q = torch.zeros(T, Hq, D, dtype=torch.float16)
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cl = torch.full((B,), 5, dtype=torch.int32)
    cu = torch.tensor([0, 5, 10], dtype=torch.int32)
    call = aule.flash_attention_paged_prefill
    # shapes
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,D\]"):
        call(q.reshape(B, 5, Hq, D), c16, c16, bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,D\]"):
        call(q, c16, c16[:2], bt, cl, cu)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,D\]"):
        call(q, c16[0], c16[0], bt, cl, cu)
    with pytest.raises(ValueError, match="head_dim mismatch"):
        call(q, torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), bt, cl, cu)
    # head ratio
    with pytest.raises(ValueError, match="divisible"):
        call(q, torch.zeros(4, bs, 3, D, dtype=torch.float16), torch.zeros(4, bs, 3, D, dtype=torch.float16), bt, cl, cu)
    # dtypes and cache kinds
    with pytest.raises(ValueError, match="same dtype"):
        call(q, c8, c16, bt, cl, cu)
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        co = torch.zeros(4, bs, Hkv, D).to(other)
        with pytest.raises(ValueError, match=r"float8_e4m3fn only.*OCP"):
            call(q, co, co, bt, cl, cu)
    with pytest.raises(ValueError, match="paged prefill runs in fp16 or bf16"):
        call(q.float(), c8, c8, bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q.float(), c16.float(), c16.float(), bt, cl, cu)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q, c16.to(torch.bfloat16), c16.to(torch.bfloat16), bt, cl, cu)
    # scales
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        call(q, c16, c16, bt, cl, cu, k_scale=0.5)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        call(q, c16, c16, bt, cl, cu, v_scale=torch.ones(Hkv))
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        call(q, c8, c8, bt, cl, cu, k_scale=torch.ones(Hkv + 1))
    with pytest.raises(ValueError, match=r"v_scale must be"):
        call(q, c8, c8, bt, cl, cu, v_scale=torch.ones(Hkv, 2))
    # head_dim
    with pytest.raises(ValueError, match="head_dim must be one of"):
        c256 = torch.zeros(4, bs, Hkv, 256, dtype=torch.float16)
        call(torch.zeros(T, Hq, 256, dtype=torch.float16), c256, c256, bt, cl, cu)
    with pytest.raises(ValueError, match="block_size"):
        c0 = torch.zeros(4, 0, Hkv, D, dtype=torch.float16)
        call(q, c0, c0, bt, cl, cu)
    # table, lengths, offsets
    for bad_bt, bad_cl in ((bt[0], cl), (bt, cl[:1]), (bt[:, :0], cl), (bt, cl.view(B, 1))):
        with pytest.raises(ValueError, match="block_tables must be"):
            call(q, c16, c16, bad_bt, bad_cl, cu)
    for bad_cu in (cu[:2], torch.zeros(B + 2, dtype=torch.int32), cu.view(1, B + 1), [0, 5, 10]):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\] = \[3\] tensor"):
            call(q, c16, c16, bt, cl, bad_cu)
    for bad_cu in (cu.long(), cu.float(), cu.to(torch.int16)):
        with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
            call(q, c16, c16, bt, cl, bad_cu)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
            call(q, c16, c16, bt, cl, cu, max_seqlen_q=bad)
    # stride alignment: a token stride or a storage offset that is no multiple of 8 elements
    wide = torch.zeros(T, Hq * D + 4, dtype=torch.float16)
    with pytest.raises(ValueError, match="multiples of 8 elements"):
        call(wide[:, :Hq * D].view(T, Hq, D), c16, c16, bt, cl, cu)
    shifted = torch.zeros(T * Hq * D + 4, dtype=torch.float16)[4:].view(T, Hq, D)
    with pytest.raises(ValueError, match="multiples of 8 elements"):
        call(shifted, c16, c16, bt, cl, cu)
    # well-formed, on the CPU: a slice of a fused projection included
    fused = torch.zeros(T, 3 * Hq * D, dtype=torch.float16)
    for ok in (q, fused[:, :Hq * D].view(T, Hq, D), fused[:, Hq * D:2 * Hq * D].view(T, Hq, D)):
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(ok, c16, c16, bt, cl, cu, max_seqlen_q=5)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, c8, c8, bt, cl, cu, k_scale=0.5, v_scale=torch.ones(Hkv), return_lse=True)


def test_prefill_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fa_fwd_paged_prefill_kernel<T, D, KV>: fp16, bf16 x D 32, 64, 128 x the two cache kinds."""
    src = os.path.join(CSRC, "fa_fwd_paged_prefill_gfx950.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "prefill.o"), src],
                       capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\]| \[bytes/block\]| \[waves/SIMD\])?: (\d+)", line)
        if m and cur is not None:
            res[cur][m.group(1)] = int(m.group(2))
    ks = [n for n in res if "fa_fwd_paged_prefill_kernel" in n]
    assert len(ks) == 12 and sum("KvFp8" in n for n in ks) == 6 and sum("Kv16" in n for n in ks) == 6, ks
    assert sum("Bf16Traits" in n for n in ks) == 6 and sum("F16Traits" in n for n in ks) == 6
    for n in ks:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") <= 40 * 1024, (n, r_)
