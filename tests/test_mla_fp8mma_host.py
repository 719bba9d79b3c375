"""The paged MLA with FP8 matrix products without a GPU: the wrapper's own two ValueErrors, the answers the C entry and
its size query give before they need a device (the twin's descriptor, checker and codes) and the bound symbols."""
import ctypes
import inspect

import pytest

from test_mla_fp8_host import _error, _fill_fp8

import aule
from aule import _capi

ENTRY, SIZE = "aule_attention_mla_paged_fp8mma_ex", "aule_attention_mla_paged_fp8mma_workspace_size"


def test_the_wrapper_own_errors_come_before_any_device_use():
    import torch
    q = torch.zeros(6, 16, 576, dtype=torch.bfloat16)
    kv = torch.zeros(12, 16, 576, dtype=torch.float8_e4m3fn)
    bt, cl = torch.zeros(3, 4, dtype=torch.int32), torch.tensor([5, 9, 20], dtype=torch.int32)
    cu = torch.tensor([0, 2, 4, 6], dtype=torch.int32)
    call = aule.flash_attention_mla_paged_fp8mma
    assert list(inspect.signature(call).parameters) == list(inspect.signature(aule.flash_attention_mla_paged_fp8).parameters)
    for bad in (torch.bfloat16, torch.float8_e4m3fnuz, torch.uint8):
        with pytest.raises(ValueError, match="needs a torch.float8_e4m3fn latent cache"):
            call(q, torch.zeros(12, 16, 576).to(bad), bt, cl, cu, kv_scale=1.0)
    with pytest.raises(ValueError, match="needs kv_scale"):
        call(q, kv, bt, cl, cu)
    # the twin's rules through the twin's helpers, then the device
    with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
        call(q, kv, bt, cl, cu, kv_scale=torch.ones(2))
    with pytest.raises(ValueError, match="cu_seqlens_q must be int32"):
        call(q, kv, bt, cl, cu.long(), kv_scale=0.5)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, kv, bt, cl, cu, max_seqlen_q=2, kv_scale=torch.tensor([0.5]))


def test_the_c_entry_answers_as_the_twin_before_the_device():
    lib = _capi.load()
    bound = {s[0]: s for s in _capi.SIGNATURES}
    assert ENTRY in bound and SIZE in bound and bound[SIZE][1] is ctypes.c_uint64 and hasattr(lib, ENTRY) and hasattr(lib, SIZE)
    entry, size = getattr(lib, ENTRY), getattr(lib, SIZE)
    assert entry(None) == -3 and "struct_size" in _error(lib) and size(None) == 0
    for field, bad in (("struct_size", 136), ("struct_size", 0), ("qk_dim", 512), ("kv_scale", None)):
        d = _fill_fp8()
        setattr(d, field, bad)
        assert entry(ctypes.byref(d)) == lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == -3, field
        assert _error(lib).startswith("Paged MLA FP8 attention failed: ")
        assert entry(ctypes.byref(d)) == -3 and _error(lib).startswith("Paged MLA FP8-product attention failed: "), _error(lib)
    # a 16-bit descriptor is refused by its size; the size query is the twin's number
    d16 = _fill_fp8(cls=_capi.MlaPagedDesc)
    assert entry(ctypes.cast(ctypes.byref(d16), ctypes.POINTER(_capi.MlaPagedFp8Desc))) == -3 and "struct_size" in _error(lib)
    assert size(ctypes.cast(ctypes.byref(d16), ctypes.POINTER(_capi.MlaPagedFp8Desc))) == 0
    d = _fill_fp8(T=2, B=1, max_sq=2)
    assert size(ctypes.byref(d)) == lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d)) > 0
    # nothing to do: 0 without a device, null pointers and all
    d = _fill_fp8()
    d.total_tokens = 0
    d.q = d.kv_cache = d.out = d.kv_scale = None
    assert entry(ctypes.byref(d)) == 0 and size(ctypes.byref(d)) == 0

