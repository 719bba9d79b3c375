"""The indexer's write side without a GPU: the additive C-ABI entry (symbol, binding, descriptor size, the bad-descriptor answers),
the two public names, every argument rule of the torch layer, and a resource audit of the kernel file (no scratch, no spill)."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

NAME = "aule_mla_indexer_rows_ex"
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def test_symbol_names_and_descriptor():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = _capi.load()
    assert hasattr(ctypes.CDLL(_capi.find_library()), NAME) and NAME in {s[0] for s in _capi.SIGNATURES}
    assert "sizeof(aule_mla_indexer_rows_desc) = %d" % ctypes.sizeof(_capi.MlaIndexerRowsDesc) in header
    assert _capi.MlaIndexerRowsDesc.positions.offset == 176 and _capi.MlaIndexerRowsDesc.x_token_stride.offset == 64
    for name in ("mla_indexer_k_append", "mla_indexer_q_rotate"):
        assert name in aule.__all__ and callable(getattr(aule, name)), name
    d = _capi.MlaIndexerRowsDesc()
    assert lib.aule_mla_indexer_rows_ex(None) == -3
    assert lib.aule_mla_indexer_rows_ex(ctypes.byref(d)) == -3 and b"descriptor" in lib.aule_get_error()   # struct_size 0
    d.struct_size = ctypes.sizeof(d) - 8
    assert lib.aule_mla_indexer_rows_ex(ctypes.byref(d)) == -3
    d.struct_size, d.dtype, d.heads = ctypes.sizeof(d), 2, 1
    assert lib.aule_mla_indexer_rows_ex(ctypes.byref(d)) == 0                                              # no tokens: nothing to do


def _k_call(**kw):
    """a well-formed key append on CPU tensors (it ends in AuleError); `kw` replaces arguments"""
    a = dict(k=torch.zeros(4, 128, dtype=BF), k_cache=torch.zeros(2, 8, 128, dtype=BF), slot_mapping=torch.arange(4))
    a.update(kw)
    return aule.mla_indexer_k_append(a.pop("k"), a.pop("k_cache"), a.pop("slot_mapping"), **a)


def _q_call(**kw):
    a = dict(q=torch.zeros(4, 3, 128, dtype=BF))
    a.update(kw)
    return aule.mla_indexer_q_rotate(a.pop("q"), **a)


ROPE = dict(cos=torch.ones(16, 32), sin=torch.zeros(16, 32), positions=torch.arange(4))
W = torch.ones(128)
K_BAD = {
    "width": dict(k=torch.zeros(4, 64, dtype=BF)),
    "cache width": dict(k_cache=torch.zeros(2, 8, 64, dtype=BF)),
    "mixed dtypes": dict(k_cache=torch.zeros(2, 8, 128, dtype=torch.float16)),
    "fp8 without k_scale": dict(k_cache=torch.zeros(2, 8, 128, dtype=F8)),
    "k_scale with 16-bit cache": dict(k_scale=torch.zeros(2, 8)),
    "k_scale shape": dict(k_cache=torch.zeros(2, 8, 128, dtype=F8), k_scale=torch.zeros(16)),
    "k_scale dtype": dict(k_cache=torch.zeros(2, 8, 128, dtype=F8), k_scale=torch.zeros(2, 8, dtype=torch.float16)),
    "non-contiguous cache": dict(k_cache=torch.zeros(2, 8, 256, dtype=BF)[:, :, :128]),
    "token stride": dict(k=torch.zeros(4, 132, dtype=BF)[:, :128]),
    "storage offset": dict(k=torch.zeros(4, 136, dtype=BF)[:, 4:132]),
    "cos alone": dict(cos=ROPE["cos"]),
    "no positions": dict(cos=ROPE["cos"], sin=ROPE["sin"]),
    "positions alone": dict(positions=ROPE["positions"]),
    "rope_layout": dict(rope_layout="neox"),
    "rope_offset": dict(rope_offset=32),
    "scale_format": dict(scale_format="e8m0"),
    "slot shape": dict(slot_mapping=torch.arange(5)),
    "slot dtype": dict(slot_mapping=torch.zeros(4)),
    "heads": dict(k=torch.zeros(4, 2, 128, dtype=BF)),
    "bias without weight": dict(norm_bias=W),
    "requires grad": dict(k=torch.zeros(4, 128, dtype=BF, requires_grad=True)),
}
Q_BAD = {
    "rank": dict(q=torch.zeros(4, 128, dtype=BF)),
    "width": dict(q=torch.zeros(4, 3, 64, dtype=BF)),
    "head stride": dict(q=torch.zeros(4, 3, 132, dtype=BF)[:, :, :128]),
    "out shape": dict(out=torch.zeros(4, 2, 128, dtype=BF)),
    "out dtype": dict(out=torch.zeros(4, 3, 128, dtype=torch.float16)),
    "out stride": dict(out=torch.zeros(4, 3, 132, dtype=BF)[:, :, :128]),
}


@pytest.mark.parametrize("call,bad", [(_k_call, K_BAD[n]) for n in K_BAD] + [(_q_call, Q_BAD[n]) for n in Q_BAD],
                         ids=["k: " + n for n in K_BAD] + ["q: " + n for n in Q_BAD])
def test_argument_rules_are_value_errors(call, bad):
    with pytest.raises(ValueError):
        call(**bad)


@pytest.mark.parametrize("call,kw", [(_k_call, dict(ROPE, norm_weight=W, norm_bias=W, rope_layout="interleaved", rope_offset=64)),
                                     (_k_call, dict(k_cache=torch.zeros(2, 8, 128, dtype=F8), k_scale=torch.zeros(2, 8), scale_format="ue8m0")),
                                     (_q_call, dict(ROPE, out=torch.zeros(4, 3, 128, dtype=BF)))])
def test_cpu_tensors_that_pass_the_rules_are_an_aule_error(call, kw):
    with pytest.raises(aule.AuleError):
        call(**kw)


def test_no_instance_uses_scratch_or_spills(tmp_path):
    res = resource_report("mla_indexer_append_gfx950.hip", tmp_path)
    assert len(res) == 48 and all("mla_indexer_rows_kernel" in k for k in res), sorted(res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (k, r)
