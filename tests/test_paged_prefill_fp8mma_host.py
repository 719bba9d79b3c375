"""The paged prefill with FP8 matrix products without a GPU: the additive C entry (symbol, the answers it gives before it needs a
device), the argument errors of the torch layer, aule.quantize_rows_fp8 on the CPU, a resource audit of the four kernel instances
and the Makefile rule of the new source."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT
from test_paged_prefill_host import BAD_FIELDS, PTRS, _error, _fill

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
NAME = "aule_attention_paged_prefill_fp8mma_ex"
SOURCE = "fa_fwd_paged_prefill_fp8mma_gfx950.hip"
LDS_BYTES = {64: 10240, 128: 19456}   # K image 64 x (D + 16), V^T image D x 80


def _entry(lib):
    return getattr(lib, NAME)


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    assert re.search(r"\b%s\s*\(const aule_paged_prefill_desc\*" % NAME, header)
    assert hasattr(lib, NAME)
    assert NAME in {s[0] for s in _capi.SIGNATURES}
    for name in ("flash_attention_paged_prefill_fp8mma", "quantize_rows_fp8"):
        assert name in aule.__all__ and callable(getattr(aule, name))
    sig = inspect.signature(aule.flash_attention_paged_prefill_fp8mma)
    assert sig == inspect.signature(aule.flash_attention_paged_prefill)
    kernels = open(os.path.join(CSRC, "fa_kernels.h")).read()
    assert "int launch_paged_prefill_fp8mma(const PagedPrefillArgs& a, hipStream_t stream);" in kernels


# the twin's refusals, on an FP8 descriptor (the two about scales given with a 16-bit cache are the twin's alone: here a 16-bit cache is
# refused as such)
TWIN_FIELDS = [c for c in BAD_FIELDS if c[0] not in ("k_scale", "v_scale")]


@pytest.mark.parametrize("field,bad,needle", TWIN_FIELDS, ids=lambda x: str(x).replace(" ", "_"))
def test_entry_keeps_every_refusal_of_the_twin(field, bad, needle):
    lib = _capi.load()
    d = _fill(cache_dtype=1)
    setattr(d, field, bad)
    assert _entry(lib)(ctypes.byref(d)) == -3
    assert needle in _error(lib), _error(lib)
    assert "Paged prefill FP8-product attention failed" in _error(lib)


def test_entry_refusals_of_its_own():
    lib = _capi.load()
    assert _entry(lib)(None) == -3
    # a 16-bit cache, with or without scale pointers
    d = _fill(cache_dtype=0)
    assert _entry(lib)(ctypes.byref(d)) == -3
    assert "cache_dtype must be AULE_KV_CACHE_FP8_E4M3" in _error(lib) and "aule_attention_paged_prefill_ex" in _error(lib)
    d.k_scale = d.v_scale = 4096
    assert _entry(lib)(ctypes.byref(d)) == -3
    assert "FP8 caches only" in _error(lib)      # (the twin's checker runs first)
    # head_dim 32 is the twin's
    d = _fill(cache_dtype=1, D=32)
    assert _entry(lib)(ctypes.byref(d)) == -3
    assert "head_dim 32 unsupported by the FP8-product prefill" in _error(lib) and "aule_attention_paged_prefill_ex" in _error(lib)
    # null scales
    for field in ("k_scale", "v_scale"):
        d = _fill(cache_dtype=1)
        setattr(d, field, None)
        assert _entry(lib)(ctypes.byref(d)) == -3
        assert "null scale pointer" in _error(lib)
    # the packed-row count must fit 32 bits
    d = _fill(T=1 << 29, Hq=64, Hkv=8, cache_dtype=1)
    d.q_token_stride = 64 * 128
    assert _entry(lib)(ctypes.byref(d)) == -3
    assert "32 bits" in _error(lib)


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0, batch = 0 or heads_q = 0: 0, with null pointers, in any process; this entry's own rules still hold."""
    lib = _capi.load()
    for field in ("total_tokens", "batch", "heads_q"):
        d = _fill(cache_dtype=1)
        setattr(d, field, 0)
        if field == "heads_q":
            d.q_token_stride = 0
        for n in PTRS + ("k_scale", "v_scale"):
            setattr(d, n, None)
        assert _entry(lib)(ctypes.byref(d)) == 0, field
    for change in (dict(D=32), dict(cache_dtype=0), dict(D=256)):
        d = _fill(T=0, **{"cache_dtype": 1, **change})
        assert _entry(lib)(ctypes.byref(d)) == -3, change


def test_wrapper_value_errors_and_no_cpu_fallback():
    import torch
    B, T, Hq, Hkv, D, bs = 2, 10, 8, 2, 64, 16
    q = torch.zeros(T, Hq, D, dtype=torch.float16)
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cl = torch.tensor([5, 5], dtype=torch.int32)
    cu = torch.tensor([0, 5, 10], dtype=torch.int32)
    call = aule.flash_attention_paged_prefill_fp8mma
    one = torch.ones(Hkv)
    with pytest.raises(ValueError, match=r"caches must be float8_e4m3fn.*flash_attention_paged_prefill\)"):
        call(q, c16, c16, bt, cl, cu)
    for scales in (dict(), dict(k_scale=one), dict(v_scale=0.5)):
        with pytest.raises(ValueError, match=r"needs k_scale and v_scale.*flash_attention_paged_prefill "):
            call(q, c8, c8, bt, cl, cu, **scales)
    q32, c32 = torch.zeros(T, Hq, 32, dtype=torch.float16), torch.zeros(4, bs, Hkv, 32).to(torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=r"head_dim must be one of \(64, 128\).*got 32.*flash_attention_paged_prefill\)"):
        call(q32, c32, c32, bt, cl, cu, k_scale=one, v_scale=one)
    # the twin's rules through the same helpers
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        call(q, c8, c8, bt, cl, cu, k_scale=torch.ones(Hkv + 1), v_scale=one)
    with pytest.raises(ValueError, match="block_tables must be"):
        call(q, c8, c8, bt[0], cl, cu, k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        call(q, c8, c8, bt, cl, cu.long(), k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="max_seqlen_q must be a positive int"):
        call(q, c8, c8, bt, cl, cu, max_seqlen_q=0, k_scale=one, v_scale=one)
    with pytest.raises(ValueError, match="head_dim mismatch"):
        call(q32, c8, c8, bt, cl, cu, k_scale=one, v_scale=one)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, c8, c8, bt, cl, cu, max_seqlen_q=5, k_scale=0.5, v_scale=one, return_lse=True)


def test_quantize_rows_fp8_on_the_cpu():
    import torch
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        x = (3.0 * torch.randn(7, 5, 128, generator=g)).to(dtype)
        x[2, 3] = 0
        codes, scales = aule.quantize_rows_fp8(x)
        assert codes.dtype == torch.float8_e4m3fn and codes.shape == x.shape
        assert scales.dtype == torch.float32 and scales.shape == (7, 5, 1)
        amax = x.float().abs().amax(dim=-1, keepdim=True)
        want = amax / 448.0
        want[2, 3] = 1.0
        assert torch.equal(scales, want)
        assert torch.equal(codes.view(torch.uint8), (x.float() / scales).to(torch.float8_e4m3fn).view(torch.uint8))
        assert bool((codes[2, 3].view(torch.uint8) == 0).all())
        assert float(codes.float().abs().amax()) == 448.0
    # a row of e4m3 values whose amax is 448 * 2^k round-trips exactly
    every = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    every = every[torch.isfinite(every)]
    assert every.numel() == 254 and float(every.abs().amax()) == 448.0
    for k in (-9, -1, 0, 3, 11):
        row = every * 2.0 ** k
        codes, scales = aule.quantize_rows_fp8(row)
        assert float(scales) == 2.0 ** k
        assert torch.equal(codes.float() * scales, row)
    with pytest.raises(ValueError):
        aule.quantize_rows_fp8(torch.zeros(3, dtype=torch.int32))


def test_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fa_fwd_paged_prefill_fp8mma_kernel<T, D>: fp16, bf16 x D 64, 128; LDS exactly what DESIGN.md 3.17 states."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "fp8mma.o"), os.path.join(CSRC, SOURCE)],
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
    ks = [n for n in res if "fa_fwd_paged_prefill_fp8mma_kernel" in n]
    assert len(ks) == 4 and sum("Bf16Traits" in n for n in ks) == 2 and sum("F16Traits" in n for n in ks) == 2, ks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n in ks:
        r_ = res[n]
        D = 128 if "Li128E" in n else 64
        assert "Li%dE" % D in n
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") == LDS_BYTES[D], (n, r_)
        assert r_.get("Occupancy") >= 2, (n, r_)
        assert ("%d bytes" % LDS_BYTES[D]) in design


def test_makefile_rule_lists_the_headers_the_source_includes():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS \+= %s$" % re.escape(SOURCE), mk, re.M)
    obj = "$(OBJDIR)/" + SOURCE.replace(".hip", ".o")
    listed = set("fa_device.h fa_kernels.h fa_fwd_tile.h fa_fwd_plan.h fa_switches.h".split())   # the pattern rule's
    for line in mk.splitlines():
        if ":" in line and obj in line.split(":")[0].split():
            listed |= set(line.split(":", 1)[1].split())

    def includes(name, seen):
        for inc in re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
            if inc not in seen and inc != SOURCE:
                seen.add(inc)
                includes(inc, seen)
        return seen

    need = includes(SOURCE, set())
    assert {"fa_paged_tile.h", "fa_tile_attention.h", "fa_d256_common.h", "kv_quant.h"} <= need
    assert need <= listed, sorted(need - listed)
