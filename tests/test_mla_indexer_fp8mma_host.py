"""The index logits with FP8 queries without a GPU: the descriptor's layout and symbols, every answer the entry and its plan hook give
before they need a device, the torch layer's own ValueErrors, and the resource audit of csrc/fa_mla_indexer_fp8mma_gfx950.hip."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

NAME, ENTRY, HOOK = "aule_mla_indexer_logits_fp8mma_desc", "aule_mla_indexer_logits_fp8mma_ex", "aule_hip_debug_mla_indexer_fp8mma_plan"
PTRS = ("q", "weights", "k_cache", "k_scale", "block_tables", "context_lens", "cu_seqlens_q", "logits", "q_scale")
LAYOUT = dict(struct_size=0, reserved=4, cache_dtype=8, heads=12, head_dim=16, batch=20, num_blocks=24, block_size=28, max_blocks=32,
              total_tokens=36, max_seqlen_q=40, device=44, q_token_stride=48, logits_stride=56, stream=64, q=72, weights=80, k_cache=88,
              k_scale=96, block_tables=104, context_lens=112, cu_seqlens_q=120, logits=128, q_scale=136)
FIGURES = ("VGPRs", "AGPRs", "ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size")
BAD_SHAPE = [("struct_size", 136, "struct_size"), ("reserved", 2, "reserved (2) must be 0"), ("cache_dtype", 0, "cache_dtype 0 must be AULE_KV_CACHE_FP8_E4M3"),
             ("cache_dtype", 2, "cache_dtype 2"), ("heads", 0, "heads (0)"), ("heads", 65, "heads (65) must be in 1 .. 64"),
             ("head_dim", 64, "head_dim (64) must be 128"), ("q_token_stride", 64 * 128 - 16, "q_token_stride (8176) is smaller than a token"),
             ("q_token_stride", 64 * 128 + 8, "q_token_stride (8200) must be a multiple of 16"), ("logits_stride", 1023, "logits_stride (1023) is smaller than a row")]
BAD_POINTER = [("k_scale", None, "null k_scale"), ("q_scale", 4098, "4-byte aligned"), ("q", 4104, "16-byte aligned"), ("logits", None, "null tensor pointer")]


def test_layout_and_symbols():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(ROOT, "aule-attention_amd", "csrc", "aule_capi.cpp")).read()
    cls = _capi.MlaIndexerLogitsFp8mmaDesc
    assert "sizeof(%s) = 144" % NAME in header and "sizeof(%s) == 144" % NAME in capi and ctypes.sizeof(cls) == 144
    assert [(n, getattr(cls, n).offset) for n, _ in cls._fields_] == list(LAYOUT.items())
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", header.split("typedef struct %s {" % NAME)[1].split("}")[0])
    for found in (quoted, re.findall(r"offsetof\(%s, (\w+)\) == (\d+)" % NAME, capi)):
        assert {f: int(o) for f, o in found} == {f: o for f, o in LAYOUT.items() if f != "struct_size"}
    lib, bound = ctypes.CDLL(_capi.find_library()), {s[0] for s in _capi.SIGNATURES}
    for name in (ENTRY, HOOK):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, NAME), header) and hasattr(lib, name) and name in bound, name
    assert "mla_indexer_logits_fp8mma" in aule.__all__


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_POINTER, ids=lambda x: str(x).replace(" ", "_"))
def test_launch_and_hook_refusals(field, bad, needle):
    """-3 with a reason naming the field before the device is needed; the hook agrees on the shape and reads no pointer"""
    lib, d, out = _capi.load(), _capi.MlaIndexerLogitsFp8mmaDesc(), (ctypes.c_int32 * 5)()
    d.struct_size, d.cache_dtype, d.heads, d.head_dim, d.batch, d.num_blocks, d.block_size, d.max_blocks = ctypes.sizeof(d), 1, 64, 128, 2, 64, 64, 16
    d.total_tokens, d.max_seqlen_q, d.q_token_stride, d.logits_stride = 8, 4, 64 * 128, 1024
    for n in PTRS:
        setattr(d, n, 4096)
    plan = lambda: (getattr(lib, HOOK)(ctypes.byref(d), out, 5), list(out))   # noqa: E731
    good = plan()
    assert good == (5, [4, 1, 128, 8, 16])   # mla_indexer_plan's rule at 256 compute units: 2 sequences x 1 group, 1024 keys in 8 chunks
    setattr(d, field, bad)
    assert getattr(lib, ENTRY)(ctypes.byref(d)) == -3
    msg = lib.aule_get_error()
    msg = msg.decode() if isinstance(msg, bytes) else str(msg)
    assert needle in msg and msg.startswith("MLA indexer FP8-product logits failed: "), msg
    shape = (field, bad, needle) in BAD_SHAPE
    assert plan()[0] == (-3 if shape else 5) and plan()[1] == good[1]
    for n in PTRS:
        setattr(d, n, None)
    d.total_tokens = 0   # nothing to do: 0 with null pointers, a refused field still refused
    assert getattr(lib, ENTRY)(ctypes.byref(d)) == plan()[0] == (-3 if shape else 0)


def test_python_value_errors_before_the_device():
    import torch
    q, w = torch.zeros(3, 4, 128, dtype=torch.float8_e4m3fn), torch.zeros(3, 4)
    kc, ks = torch.zeros(5, 16, 128, dtype=torch.float8_e4m3fn), torch.ones(5, 16)
    bt, cl, call = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), aule.mla_indexer_logits_fp8mma
    for args, kw, err, match in (((q.to(torch.bfloat16), w, kc, ks), {}, ValueError, "needs torch.float8_e4m3fn queries"),
                                 ((q, w, kc.to(torch.bfloat16), ks), {}, ValueError, "needs a torch.float8_e4m3fn k_cache"),
                                 ((q, w, kc, None), {}, ValueError, "needs k_scale"),
                                 ((q, w, kc, ks), dict(q_scale=torch.ones(3, 4, 1)), ValueError, r"q_scale must be a contiguous fp32 tensor \[T, H\] = \[3, 4\]"),
                                 ((q, w.clone().requires_grad_(True), kc, ks), {}, ValueError, "no backward"),
                                 ((q, w, kc, ks), dict(q_scale=torch.ones(3, 4)), aule.AuleError, "no CPU fallback")):
        with pytest.raises(err, match=match):
            call(*args, bt, cl, **kw)


def test_resource_audit(tmp_path):
    """both instances (H <= 32, H > 32): no scratch, no spill, at most 256 registers, the LDS the header comment derives (128 keys x 144
    bytes + 128 row scales), and the figures the profile records"""
    res = resource_report("fa_mla_indexer_fp8mma_gfx950.hip", tmp_path)
    noted = {f[1]: dict(zip(FIGURES, map(int, f[2:]))) for f in map(str.split, open(os.path.join(ROOT, "profiles", "mla_indexer_fp8mma_resources.txt")))
             if len(f) == 8 and f[0] == "indexer"}
    assert len(res) == 2 and sorted(noted) == ["logits.fp8mma.h32", "logits.fp8mma.h64"]
    for label, tag in (("logits.fp8mma.h32", "Lb0"), ("logits.fp8mma.h64", "Lb1")):
        (name,) = [n for n in res if "fa_mla_indexer_logits_fp8mma_kernel" in n and tag in n]
        got = {k: res[name].get(k) for k in FIGURES}
        assert got["ScratchSize"] == got["SGPRs Spill"] == got["VGPRs Spill"] == 0 and got["VGPRs"] + got["AGPRs"] <= 256, (label, got)
        assert got["LDS Size"] == 128 * 144 + 128 * 4 and got == noted[label], (label, got, noted[label])
