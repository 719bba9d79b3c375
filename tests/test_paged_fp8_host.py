"""FP8 (OCP e4m3fn) paged decode without a GPU: the additive C-ABI (symbols, descriptor layout, workspace query), the
quantisation helper on CPU tensors, the argument errors of the torch layer, and a resource audit of the compiled instances
of the wave-per-chunk kernel, FP8 and 16-bit (no scratch, no VGPR or SGPR spill)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
NEW = ("aule_attention_paged_decode_fp8_ex", "aule_attention_paged_decode_fp8_workspace_size")


def _fill(d, dtype, B, Hq, Hkv, D, bs, max_blocks, window=-1):
    d.struct_size = ctypes.sizeof(d)
    d.dtype = dtype
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, Hkv, D
    d.block_size, d.max_blocks, d.window_size = bs, max_blocks, window
    return d


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0] for s in _capi.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\s*\(const aule_paged_fp8_desc\*" % name, header), name
        assert hasattr(lib, name), name
        assert name in bound, name


def test_fp8_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    assert "sizeof(aule_paged_fp8_desc) = 136" in header
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_paged_fp8_desc) == 136" in capi
    D = _capi.PagedFp8Desc
    assert ctypes.sizeof(D) == 136
    assert D.stream.offset == 48 and D.workspace.offset == 104 and D.workspace_bytes.offset == 112
    assert D.k_scale.offset == 120 and D.v_scale.offset == 128
    # the common part is aule_paged_desc field for field, which stays at 120 bytes
    assert ctypes.sizeof(_capi.PagedDesc) == 120
    for name, _ in _capi.PagedDesc._fields_:
        assert getattr(D, name).offset == getattr(_capi.PagedDesc, name).offset, name


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("B,Hq,Hkv,D,bs,mb", [(8, 32, 8, 128, 16, 2048), (2, 32, 1, 64, 128, 40), (3, 8, 8, 32, 1, 700),
                                             (1, 64, 8, 128, 48, 417), (4, 16, 4, 64, 33, 152)])
def test_fp8_workspace_query_equals_the_16_bit_plan(dtype, B, Hq, Hkv, D, bs, mb):
    """The chunk rule (about 2048 waves whatever the bytes per key) is the 16-bit call's, so the partials are too."""
    lib = _capi.load()
    d8 = _fill(_capi.PagedFp8Desc(), dtype, B, Hq, Hkv, D, bs, mb)
    d16 = _fill(_capi.PagedDesc(), dtype, B, Hq, Hkv, D, bs, mb)
    want = lib.aule_attention_paged_decode_workspace_size(ctypes.byref(d16))
    assert want > 0
    assert lib.aule_attention_paged_decode_fp8_workspace_size(ctypes.byref(d8)) == want


def test_fp8_workspace_query_refuses_bad_descriptors():
    lib = _capi.load()
    d = _fill(_capi.PagedFp8Desc(), 2, 8, 32, 8, 128, 16, 64)
    assert lib.aule_attention_paged_decode_fp8_workspace_size(ctypes.byref(d)) > 0
    d.struct_size = 120   # an aule_paged_desc handed to the FP8 entry
    assert lib.aule_attention_paged_decode_fp8_workspace_size(ctypes.byref(d)) == 0
    assert lib.aule_attention_paged_decode_fp8_workspace_size(None) == 0
    for field, bad in (("dtype", 0), ("head_dim", 256), ("heads_kv", 5), ("block_size", 0), ("max_blocks", 0)):
        d = _fill(_capi.PagedFp8Desc(), 2, 8, 32, 8, 128, 16, 64)
        setattr(d, field, bad)
        assert lib.aule_attention_paged_decode_fp8_workspace_size(ctypes.byref(d)) == 0, field


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_fp8_entry_reports_uninitialised_without_a_gpu():
    lib = _capi.load()
    d = _fill(_capi.PagedFp8Desc(), 2, 8, 32, 8, 128, 16, 64)
    assert lib.aule_attention_paged_decode_fp8_ex(ctypes.byref(d)) == -1


# ---- the quantisation helper (plain torch, CPU) -------------------------------------------------------------------

def _cache(seed, shape, head_scales):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    return x * torch.tensor(head_scales, dtype=torch.float32).view(1, 1, -1, 1)


def test_helper_is_exported():
    assert "quantize_kv_cache_fp8" in aule.__all__ and callable(aule.quantize_kv_cache_fp8)


@pytest.mark.parametrize("seed", range(6))
def test_helper_round_trip_is_within_the_format_bound(seed):
    """scale * code is within 2^-4 |x| + scale 2^-10 of x: half an ulp of a 3-bit mantissa, plus half the smallest
    subnormal step 2^-9 (both properties of e4m3fn, not of this code)."""
    import torch
    hs = [1e-3, 0.1, 1.0, 30.0, 1e3]
    x = _cache(seed, (7, 16, len(hs), 64), hs)
    c, s = aule.quantize_kv_cache_fp8(x)
    assert c.dtype == torch.float8_e4m3fn and c.shape == x.shape
    assert s.dtype == torch.float32 and s.shape == (len(hs),)
    amax = x.abs().amax(dim=(0, 1, 3))
    assert torch.equal(s, amax / 448.0)
    deq = s.view(1, 1, -1, 1) * c.float()
    assert not torch.isnan(deq).any()
    err = (deq.double() - x.double()).abs()
    bound = 2.0 ** -4 * x.double().abs() + s.double().view(1, 1, -1, 1) * 2.0 ** -10
    print("worst err / bound: %.3f" % float((err / bound).max()))
    assert bool((err <= bound).all())


def test_helper_saturates_and_survives_an_all_zero_head():
    """torch's cast to float8_e4m3fn does not saturate (465.0 -> NaN): the helper clamps before it; a head of zeros gets
    scale 1.0 (not 0/0); 16-bit inputs are accepted."""
    import torch
    assert torch.isnan(torch.tensor(465.0).to(torch.float8_e4m3fn).float())   # the premise
    x = _cache(1, (3, 8, 3, 32), [1e6, 0.0, 5.0])
    x[0, 0, 0, 0] = 3e7    # far above 448 and far above the rest of its head
    c, s = aule.quantize_kv_cache_fp8(x)
    assert not torch.isnan(c.float()).any()
    assert float(s[1]) == 1.0 and bool((c.float()[:, :, 1] == 0).all())
    assert float(c.float()[0, 0, 0, 0]) == 448.0
    cb, sb = aule.quantize_kv_cache_fp8(x.to(torch.bfloat16))
    assert cb.dtype == torch.float8_e4m3fn and sb.dtype == torch.float32 and not torch.isnan(cb.float()).any()


def test_helper_per_tensor_scale_is_one_repeated_value():
    import torch
    x = _cache(2, (4, 16, 4, 32), [0.5, 1.0, 2.0, 8.0])
    c, s = aule.quantize_kv_cache_fp8(x, per_head=False)
    assert s.shape == (4,) and bool((s == s[0]).all())
    assert float(s[0]) == float(x.abs().max() / 448.0)
    z, sz = aule.quantize_kv_cache_fp8(torch.zeros(2, 4, 3, 32), per_head=False)
    assert bool((sz == 1.0).all()) and bool((z.float() == 0).all())


# ---- argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule._torch.paged_decode with CPU tensors: aule.flash_attention_paged_amd keeps its device check first
    (a CPU query is an AuleError there, as before), and paged_decode validates formats, dtypes and scale shapes before
    it loads the library or touches a device -- so these are reachable, and raised, without a GPU."""
    import torch
    from aule._torch import paged_decode
    B, Hq, Hkv, D, bs = 2, 8, 2, 64, 16
    q = torch.zeros(B, Hq, D, dtype=torch.float16)
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cl = torch.ones(B, dtype=torch.int32)
    with pytest.raises(ValueError, match="same dtype"):
        paged_decode(q, c8, c16, bt, cl)
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        co = torch.zeros(4, bs, Hkv, D).to(other)
        with pytest.raises(ValueError, match=r"float8_e4m3fn only.*OCP"):
            paged_decode(q, co, co, bt, cl)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        paged_decode(q, c16, c16, bt, cl, k_scale=0.5)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        paged_decode(q, c16, c16, bt, cl, v_scale=torch.ones(Hkv))
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        paged_decode(q, c8, c8, bt, cl, k_scale=torch.ones(Hkv + 1))
    with pytest.raises(ValueError, match=r"v_scale must be"):
        paged_decode(q, c8, c8, bt, cl, v_scale=torch.ones(Hkv, 2))
    with pytest.raises(ValueError, match="fp16 or bf16"):
        paged_decode(q.float(), c8, c8, bt, cl)
    with pytest.raises(ValueError, match="head_dim"):
        paged_decode(torch.zeros(B, Hq, 256, dtype=torch.float16), torch.zeros(4, bs, Hkv, 256).to(torch.float8_e4m3fn),
                     torch.zeros(4, bs, Hkv, 256).to(torch.float8_e4m3fn), bt, cl)


def test_every_finite_code_is_exact_in_both_16_bit_types():
    """What lets the kernel convert a code to the query's type without its scale and keep the 16-bit MFMAs."""
    import torch
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    finite = codes[~torch.isnan(codes)]
    assert finite.numel() == 254 and float(finite.abs().max()) == 448.0
    for dt in (torch.float16, torch.bfloat16):
        assert torch.equal(finite.to(dt).float(), finite)


# ---- resource audit -------------------------------------------------------------------------------------------------

def test_fp8_kernels_neither_spill_nor_use_scratch(tmp_path):
    src = os.path.join(CSRC, "fa_fwd_splitkv_gfx950.hip")
    out = tmp_path / "splitkv.o"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), src],
                       capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur is not None:
            res[cur][m.group(1)] = int(m.group(2))
    # fa_fwd_splitkv_kernel<T, D, KV, PAGED>: fp16, bf16 x D 32, 64, 128 per K/V source
    wave = [n for n in res if "fa_fwd_splitkv_kernel" in n]
    fp8 = [n for n in wave if "KvFp8" in n]
    assert len(fp8) == 6, fp8
    assert all("Lb1" in n for n in fp8), fp8                        # FP8 is a paged source
    kv16 = [n for n in wave if "Kv16" in n]
    assert len(kv16) == 12 and len(wave) == 18, wave                # contiguous and paged
    assert sum("Lb1" in n for n in kv16) == 6, kv16
    for n in fp8 + kv16:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
