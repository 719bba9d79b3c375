"""Sparse MLA over the per-128-scaled FP8 latent cache (656-byte rows) without a GPU: the additive C-ABI, the argument errors of the
torch layer, the quantiser and its way back on the CPU, the build rule and the resource audit of the new kernels."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
SPARSE = dict(struct_size=0, dtype=4, reserved=8, heads_q=12, num_blocks=16, block_size=20, total_tokens=24, topk=28, scale=32, device=36,
              q_token_stride=40, stream=48, q=56, kv_cache=64, indices=72, out=80, lse=88, workspace=96, workspace_bytes=104)
APPEND = dict(struct_size=0, dtype=4, reserved=8, rope_layout=12, total_tokens=16, num_blocks=20, block_size=24, table_len=28,
              table_pitch=32, device=36, c_kv_token_stride=40, k_pe_token_stride=48, stream=56, c_kv=64, k_pe=72, kv_cache=80,
              slot_mapping=88, cos=96, sin=104, positions=112)
FIGURES = ("VGPRs", "AGPRs", "ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size")
NO_GPU = not os.path.exists("/dev/kfd")


def _fill(cls=_capi.MlaSparseDsDesc, T=2, Hq=16, topk=2048):
    """a well-formed descriptor of either kind with 16-byte aligned dummy pointers: only handed to calls that answer before a launch"""
    d = cls()
    d.struct_size, d.dtype, d.total_tokens, d.num_blocks, d.block_size = ctypes.sizeof(d), 2, T, 64, 64
    if cls is _capi.MlaKvAppendDsDesc:
        d.c_kv_token_stride, d.k_pe_token_stride, ptrs = 512, 64, ("c_kv", "k_pe", "kv_cache", "slot_mapping")
    else:
        d.heads_q, d.topk, d.q_token_stride, ptrs = Hq, topk, Hq * 576, ("q", "kv_cache", "indices", "out", "lse")
    for n in ptrs:
        setattr(d, n, 4096)
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _plan(fn, d):
    out = (ctypes.c_int32 * 6)()
    return fn(ctypes.byref(d), out, 6), list(out)


@pytest.mark.parametrize("name,cls,layout,size", [("aule_mla_sparse_ds_desc", _capi.MlaSparseDsDesc, SPARSE, 112),
                                                  ("aule_mla_kv_append_ds_desc", _capi.MlaKvAppendDsDesc, APPEND, 120)])
def test_symbols_and_descriptor_layouts(name, cls, layout, size):
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    lib, bound = ctypes.CDLL(_capi.find_library()), {s[0] for s in _capi.SIGNATURES}
    for sym in ("aule_attention_mla_sparse_ds_ex", "aule_attention_mla_sparse_ds_workspace_size", "aule_hip_debug_mla_sparse_ds_plan",
                "aule_mla_kv_append_ds_ex"):
        assert re.search(r"\b%s\s*\(const aule_mla_\w+_ds_desc\*" % sym, header) and hasattr(lib, sym) and sym in bound, sym
    assert "sizeof(%s) = %d" % (name, size) in header and "sizeof(%s) == %d" % (name, size) in capi and ctypes.sizeof(cls) == size
    assert [(n, getattr(cls, n).offset) for n, _ in cls._fields_] == list(layout.items())
    body = header.split("typedef struct %s {" % name)[1].split("}")[0]
    stated = {n: o for n, o in layout.items() if o}
    assert {n: int(o) for n, o in re.findall(r"(\w+);\s*/\* offset (\d+)", body)} == stated
    assert {n: int(o) for n, o in re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % name, capi)} == stated
    assert {"quantize_mla_cache_fp8_ds", "dequantize_mla_cache_fp8_ds"} <= set(aule.__all__)


BAD_SHAPE = [("struct_size", 120, "struct_size"), ("dtype", 1, "dtype 1 (of q / out) must be bf16"), ("reserved", 1, "reserved (1) must be 0"),
             ("heads_q", 0, "heads_q (0)"), ("topk", 0, "topk (0)"), ("topk", 65537, "topk (65537)"), ("num_blocks", 0, "num_blocks * block_size (0 * 64)"),
             ("total_tokens", -1, "total_tokens (-1)"), ("q_token_stride", 16 * 576 + 4, "must be a multiple of 8")]
BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "kv_cache", "indices", "out")] + [
    ("kv_cache", 4104, "16-byte aligned"), ("indices", 4098, "indices must be 4-byte aligned")]


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_POINTER, ids=lambda x: str(x).replace(" ", "_"))
def test_attention_entry_refuses_each_bad_field_and_the_queries_agree(field, bad, needle):
    """-3 and a reason before the device is needed; what the shape decides the size query answers with 0 and the hook with -3, and
    neither reads a pointer"""
    lib = _capi.load()
    d = _fill()
    query = lambda: (lib.aule_attention_mla_sparse_ds_workspace_size(ctypes.byref(d)), _plan(lib.aule_hip_debug_mla_sparse_ds_plan, d))   # noqa: E731
    want = query()
    assert want[0] > 0 and want[1][0] == 6
    setattr(d, field, bad)
    assert lib.aule_attention_mla_sparse_ds_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Sparse MLA attention (656-byte rows) failed: "), _error(lib)
    assert query() == (want if (field, bad, needle) in BAD_POINTER else (0, (-3, [0] * 6)))


@pytest.mark.parametrize("T,Hq,topk", [(1, 16, 2048), (3, 65, 200), (300, 128, 64), (2, 1, 65536)])
def test_plan_is_the_sparse_plan_and_minus_one_follows_without_a_device(T, Hq, topk):
    lib = _capi.load()
    d, twin = _fill(T=T, Hq=Hq, topk=topk), _fill(_capi.MlaSparseDesc, T, Hq, topk)
    n, plan = _plan(lib.aule_hip_debug_mla_sparse_ds_plan, d)
    assert (n, plan) == _plan(lib.aule_hip_debug_mla_sparse_plan, twin) and n == 6
    ws = lib.aule_attention_mla_sparse_ds_workspace_size(ctypes.byref(d))
    assert ws == (plan[5] << 32) | (plan[4] & 0xffffffff) == lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(twin))
    if ws:   # a caller workspace smaller than the plan's is refused
        d.workspace, d.workspace_bytes = 4096, ws - 16
        assert lib.aule_attention_mla_sparse_ds_ex(ctypes.byref(d)) == -3 and "smaller than the plan's %d" % ws in _error(lib)
        d.workspace_bytes = ws
    if NO_GPU:   # past every check: the device is needed (the pointers are dummies: never launched)
        assert lib.aule_attention_mla_sparse_ds_ex(ctypes.byref(d)) == -1
    assert lib.aule_attention_mla_sparse_ds_ex(None) == -3 and lib.aule_attention_mla_sparse_ds_ex(ctypes.byref(_fill(T=0))) == 0


@pytest.mark.parametrize("field,bad,needle", [
    ("struct_size", 128, "struct_size"), ("dtype", 1, "must be bf16"), ("reserved", 1, "reserved (1) must be 0"), ("rope_layout", 2, "rope_layout 2"),
    ("block_size", 0, "block_size must be positive"), ("c_kv_token_stride", 508, "c_kv_token_stride (508)"), ("k_pe_token_stride", 68, "multiples of 8"),
    ("table_len", 8, "RoPE group only partly given"), ("kv_cache", None, "null tensor pointer"), ("c_kv", 4100, "16-byte aligned")])
def test_append_entry_refuses_each_bad_field(field, bad, needle):
    lib, cls = _capi.load(), _capi.MlaKvAppendDsDesc
    d = _fill(cls)
    setattr(d, field, bad)
    assert lib.aule_mla_kv_append_ds_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("MLA KV append (656-byte rows) failed: "), _error(lib)
    assert lib.aule_mla_kv_append_ds_ex(ctypes.byref(_fill(cls, T=0))) == 0
    if NO_GPU:   # (the pointers are dummies: never launched)
        assert lib.aule_mla_kv_append_ds_ex(ctypes.byref(_fill(cls))) == -1


def test_python_argument_errors_are_value_errors_before_the_device():
    import torch
    q, idx = torch.zeros(3, 4, 576, dtype=torch.bfloat16), torch.zeros(3, 8, dtype=torch.int32)
    kv = torch.zeros(5, 16, 656, dtype=torch.uint8)
    c_kv, k_pe, slots = torch.zeros(3, 512, dtype=torch.bfloat16), torch.zeros(3, 64, dtype=torch.bfloat16), torch.arange(3)
    sparse, append = aule.flash_attention_mla_sparse, aule.mla_kv_append
    for call in (lambda c, **kw: sparse(q, c, idx, **kw), lambda c, **kw: append(c_kv, k_pe, c, slots, **kw)):
        with pytest.raises(ValueError, match=r"\[num_blocks, block_size, 656\].*got \(5, 16, 576\)"):
            call(kv[..., :576])
        with pytest.raises(ValueError, match="kv_scale must be None with a uint8"):
            call(kv, kv_scale=1.0)
        with pytest.raises(ValueError, match="kv_cache must be contiguous"):
            call(torch.zeros(5, 32, 656, dtype=torch.uint8)[:, ::2])
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(kv.view(5, 16, 1, 656))
    with pytest.raises(ValueError, match="q must be bf16 with a uint8"):
        sparse(q.half(), kv, idx)
    with pytest.raises(ValueError, match="c_kv and k_pe must be bf16 with a uint8"):
        append(c_kv.half(), k_pe.half(), kv, slots)


def test_quantiser_and_its_way_back_on_the_cpu():
    import torch
    x = torch.randn(6, 4, 576, generator=torch.Generator().manual_seed(1)) * torch.logspace(-6, 6, 24, base=2.0).view(6, 4, 1)
    x[0, 0, :128] = 0
    x[0, 1, :128] = x[0, 1, :128].clamp(-400, 400)
    x[0, 1, 7] = 448.0 * 4
    cache = aule.quantize_mla_cache_fp8_ds(x)
    assert cache.shape == (6, 4, 656) and cache.dtype == torch.uint8
    scale = cache[..., 512:528].contiguous().view(torch.float32)
    assert bool((torch.frexp(scale)[0] == 0.5).all())                                     # powers of two
    assert scale[0, 0, 0] == 1.0 and bool((cache[0, 0, :128] == 0).all())                 # a group of zeros
    assert scale[0, 1, 0] == 4.0 and cache[0, 1, 7] == 0x7E                               # amax = 448 * 2^2: scale 4, code 448
    xg = x[..., :512].reshape(6, 4, 4, 128)
    amax = xg.abs().amax(-1)
    assert bool(((amax <= 448 * scale) & (amax > 224 * scale) | (amax == 0)).all())       # the smallest power of two that fits
    deq = aule.dequantize_mla_cache_fp8_ds(cache, torch.float32)
    assert deq.shape == (6, 4, 576) and aule.dequantize_mla_cache_fp8_ds(cache).dtype == torch.bfloat16
    assert torch.equal(deq[..., 512:], x[..., 512:].to(torch.bfloat16).float())
    # e4m3 keeps 3 mantissa bits: a normal code is within 2^-4 relative, a subnormal one (|x / scale| < 2^-6) within half its step 2^-9
    bound = torch.maximum(xg.abs() * 2.0 ** -4, scale[..., None] * 2.0 ** -10)
    assert bool(((deq[..., :512].reshape(6, 4, 4, 128) - xg).abs() <= bound).all())
    # what was quantised once is a fixed point: the same keys, and the same bytes wherever the scale is kept (a group whose largest
    # code rounded down to 224 is re-coded at half the scale with doubled codes)
    again = aule.quantize_mla_cache_fp8_ds(deq)
    assert torch.equal(aule.dequantize_mla_cache_fp8_ds(again, torch.float32), deq)
    same = (scale == again[..., 512:528].contiguous().view(torch.float32)).repeat_interleave(128, dim=-1)
    assert bool((again[..., :512] == cache[..., :512])[same].all()) and same.float().mean() > 0.8


def test_build_rule_and_resource_audit(tmp_path):
    """the Makefile names the new sources and their headers; the kernels compile with its flags without scratch or spill at the figures
    recorded in profiles/mla_sparse_ds_resources.txt, the attention kernel at the sparse instances' LDS size"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [w for line in re.findall(r"^SRCS [:+]= (.*)$", mk, re.M) for w in line.split()]
    units = ("fa_fwd_mla_sparse_ds_gfx950", "mla_kv_append_ds_gfx950")
    dep = re.search(r"^\$\(OBJDIR\)/%s\.o \$\(OBJDIR\)/%s\.o: (.*)$" % units, mk, re.M).group(1).split()
    assert {"fa_mla_ds.h", "fa_mla_common.h", "fa_paged_tile.h", "kv_quant.h"} <= set(dep) and len(srcs) == len(set(srcs))
    text = open(os.path.join(CSRC, units[0] + ".hip")).read()
    assert "mla_paged_body<Bf16Traits, KvFp8Ds, true>" in text and "mfma16" not in text      # the tile step is not written a second time
    lines = [ln.split() for ln in open(os.path.join(ROOT, "profiles", "mla_sparse_ds_resources.txt"))]
    noted = {f[1]: dict(zip(FIGURES, map(int, f[2:]))) for f in lines if len(f) == 8 and f[0] == "ds"}
    got = {}
    for i, u in enumerate(units):
        assert u + ".hip" in srcs
        (tmp_path / str(i)).mkdir()
        got.update(resource_report(u + ".hip", tmp_path / str(i)))
    assert len(got) == len(noted) == 4
    for key, want in noted.items():
        (sym,) = [n for n in got if key in n]
        fig = {k: got[sym].get(k) for k in FIGURES}
        assert fig["ScratchSize"] == 0 and fig["SGPRs Spill"] == 0 and fig["VGPRs Spill"] == 0 and fig == want, (key, fig, want)
    assert noted["fa_fwd_mla_sparse_ds_kernel"]["LDS Size"] == 111616
