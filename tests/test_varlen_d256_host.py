"""Variable-length attention at head_dim 256 without a GPU: the C entries' answers before they need a device, the argument errors of
aule.flash_attention_varlen_d256, and the compiler's resource report of the new kernels."""
import ctypes
import os
import re

import pytest

import util
from conftest import ROOT
from test_varlen_host import _error, _fill   # (a well-formed descriptor on aligned dummy pointers; the reason of the last refusal)

import aule
from aule import _capi

FWD, BWD, SIZE = ("aule_attention_varlen_d256_" + s for s in ("forward_ex", "backward_ex", "backward_workspace_size"))
PREFIX = {FWD: "Variable-length attention (head_dim 256) failed: ", BWD: "Variable-length backward (head_dim 256) failed: "}
WS = (700 * 32 * 4 + 255) // 256 * 256


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, desc in ((FWD, "aule_varlen_desc"), (BWD, "aule_varlen_bwd_desc"), (SIZE, "aule_varlen_bwd_desc")):
        assert re.search(r"\b%s\s*\(const %s\*" % (name, desc), header) and hasattr(lib, name) and name in bound, name
    assert bound[SIZE][1] is ctypes.c_uint64 and "flash_attention_varlen_d256" in aule.__all__


BAD = [("head_dim", 128, "head_dim 128 unsupported (256 alone"), ("head_dim", 0, "head_dim 0 unsupported"), ("dtype", 0, "fp16 or bf16"),
       ("heads_kv", 5, "divisible"), ("q_token_stride", 32 * 256 - 8, "q_token_stride (8184) is smaller than a token"),
       ("v_token_stride", 8 * 256 + 4, "v_token_stride (2052) must be a multiple of 8"), ("struct_size", 8, "struct_size")]
BAD_LAUNCH = {FWD: [("q", None, "null tensor pointer"), ("cu_seqlens_k", None, "null cu_seqlens pointer")],
              BWD: [("dk", None, "null tensor pointer"), ("workspace_bytes", WS - 1, "workspace too small (89599 bytes, need 89600)")]}


@pytest.mark.parametrize("entry,field,bad,needle", [(e,) + c for e in (FWD, BWD) for c in BAD + BAD_LAUNCH[e]])
def test_each_bad_field_is_refused_before_the_device_is_needed(entry, field, bad, needle):
    """-3 with a reason under the entry's own prefix; the size query gives the launch's verdict on the problem statement"""
    lib = _capi.load()
    d = _fill("fwd" if entry == FWD else "bwd", D=256)
    setattr(d, field, bad)
    assert getattr(lib, entry)(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith(PREFIX[entry]), _error(lib)
    if entry == BWD:
        assert getattr(lib, SIZE)(ctypes.byref(d)) == (0 if (field, bad, needle) in BAD else WS)


def test_nothing_to_do_returns_zero():
    lib = _capi.load()
    for entry, kind in ((FWD, "fwd"), (BWD, "bwd")):
        for none in (dict(B=0), dict(Hq=0), dict(Tq=0, Tk=0)):
            assert getattr(lib, entry)(ctypes.byref(_fill(kind, D=256, **none))) == 0, (entry, none)
    assert getattr(lib, SIZE)(ctypes.byref(_fill("bwd", D=256, B=0))) == 0 and getattr(lib, SIZE)(ctypes.byref(_fill("bwd", D=256))) == WS


def test_python_argument_errors_are_value_errors_before_any_launch():
    import torch
    Hq, Hkv, call = 4, 2, aule.flash_attention_varlen_d256
    q, k = torch.zeros(10, Hq, 256, dtype=torch.bfloat16), torch.zeros(12, Hkv, 256, dtype=torch.bfloat16)
    cq, ck = torch.tensor([0, 5, 10], dtype=torch.int32), torch.tensor([0, 6, 12], dtype=torch.int32)
    wide = torch.zeros(12, Hkv * 256 + 4, dtype=torch.bfloat16)[:, :Hkv * 256].view(12, Hkv, 256)
    fused = torch.zeros(10, Hq + 2 * Hkv, 256, dtype=torch.bfloat16)   # (well formed, its three slices read in place: refused for the device alone)
    for error, args, reason in ((ValueError, (q[..., :128], k[..., :128], k[..., :128], cq, ck), r"head_dim 256 alone, got 128: flash_attention_varlen\b"),
                                (ValueError, (q.float(), k.float(), k.float(), cq, ck), "not built for torch.float32"),
                                (ValueError, (q, k, k, cq.long(), ck), "cu_seqlens_q must be int32"),
                                (ValueError, (q, wide, k, cq, ck), "k's token stride.*multiples of 8 elements"),
                                (aule.AuleError, (fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:], cq, cq, 5, 5), "no CPU fallback")):
        with pytest.raises(error, match=reason):
            call(*args)


@pytest.mark.parametrize("src,kernels", [("fa_fwd_varlen_d256_gfx950.hip", ["fa_fwd_varlen_d256_kernel"]),
                                         ("fa_bwd_varlen_d256_gfx950.hip", ["fa_bwd_varlen_d256_dq_kernel", "fa_bwd_varlen_d256_dkdv_kernel"])])
def test_kernels_neither_spill_nor_use_scratch(src, kernels, tmp_path, monkeypatch):
    """fp16 and bf16 of every new kernel, with what the Makefile's rule for these two files adds: no scratch, no spill, LDS within 160 KB"""
    line = util.makefile_compile_line() + "-Xclang -target-feature -Xclang -packed-fp32-ops".split()
    monkeypatch.setattr(util, "makefile_compile_line", lambda: line)
    res = util.resource_report(src, tmp_path)
    for name in kernels:
        ks = {n: r for n, r in res.items() if name in n}
        assert len(ks) == 2 and sum("Bf16Traits" in n for n in ks) == 1, (name, list(ks))
        assert all(r.get(x) == 0 for r in ks.values() for x in ("ScratchSize", "VGPRs Spill", "SGPRs Spill")), ks
        assert all(r.get("LDS Size") <= 160 * 1024 for r in ks.values()), ks
