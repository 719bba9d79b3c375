"""Logit soft-capping at head_dim 256 without a GPU: the additive C-ABI (symbols, each descriptor its twin plus softcap, the refusal of a
bad cap before a device is needed, size queries equal to the twins'), the Python ValueErrors and the compiler's resource report of the
new kernel instances."""
import ctypes
import os
import re

import pytest

import util
from conftest import ROOT
from test_paged_d256_host import _fill as _fill_paged
from test_varlen_host import _error, _fill as _fill_varlen

import aule
from aule import _capi

V = "aule_attention_varlen_d256_softcap_"
P = "aule_attention_paged_d256_softcap_"
# entry: (descriptor, its twin, the twin's filled descriptor, the twin's entry, error prefix or None for a size query)
ENTRIES = {
    V + "forward_ex": (_capi.VarlenSoftcapDesc, _capi.VarlenDesc, lambda: _fill_varlen("fwd", D=256), "aule_attention_varlen_d256_forward_ex",
                       "Variable-length soft-cap attention (head_dim 256) failed: "),
    V + "backward_ex": (_capi.VarlenSoftcapBwdDesc, _capi.VarlenBwdDesc, lambda: _fill_varlen("bwd", D=256), "aule_attention_varlen_d256_backward_ex",
                        "Variable-length soft-cap backward (head_dim 256) failed: "),
    V + "backward_workspace_size": (_capi.VarlenSoftcapBwdDesc, _capi.VarlenBwdDesc, lambda: _fill_varlen("bwd", D=256),
                                    "aule_attention_varlen_d256_backward_workspace_size", None),
    P + "ex": (_capi.PagedD256SoftcapDesc, _capi.PagedD256Desc, lambda: _fill_paged(T=8, B=1, max_blocks=64), "aule_attention_paged_d256_ex",
               "Paged head_dim 256 soft-cap attention failed: "),
    P + "workspace_size": (_capi.PagedD256SoftcapDesc, _capi.PagedD256Desc, lambda: _fill_paged(T=8, B=1, max_blocks=64),
                           "aule_attention_paged_d256_workspace_size", None),
}


def _capped(entry, softcap):
    """the twin's well-formed descriptor (dummy pointers: only for calls that answer before a launch) as the capped kind"""
    cls, _, fill, _, _ = ENTRIES[entry]
    twin, d = fill(), cls()
    for n, _ in twin._fields_:
        setattr(d, n, getattr(twin, n))
    d.struct_size, d.softcap = ctypes.sizeof(d), softcap
    return d


def test_symbols_are_declared_exported_and_bound_and_descriptors_are_twins_plus_softcap():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    names = {_capi.VarlenSoftcapDesc: "aule_varlen_softcap_desc", _capi.VarlenSoftcapBwdDesc: "aule_varlen_softcap_bwd_desc",
             _capi.PagedD256SoftcapDesc: "aule_paged_d256_softcap_desc"}
    for entry, (cls, twin, _, _, prefix) in ENTRIES.items():
        assert re.search(r"\b%s\s*\(const %s\*" % (entry, names[cls]), header) and hasattr(lib, entry) and entry in bound, entry
        assert bound[entry][1] is (ctypes.c_uint64 if prefix is None else ctypes.c_int32)
        assert ctypes.sizeof(cls) == ctypes.sizeof(twin) + 8 and cls.softcap.offset == ctypes.sizeof(twin) and cls.softcap.size == 4
        assert all(getattr(cls, n).offset == getattr(twin, n).offset for n, _ in twin._fields_), entry
        assert "sizeof(%s) = %d" % (names[cls], ctypes.sizeof(cls)) in header
    assert {"flash_attention_varlen_d256_softcap", "flash_attention_paged_d256_softcap"} <= set(aule.__all__)


@pytest.mark.parametrize("softcap,needle", [(0.0, "softcap is 0: for attention without a cap call aule_attention_"), (-1.0, "softcap (-1) must be a finite value > 0"),
                                            (float("inf"), "softcap (inf) must be"), (float("nan"), "must be a finite value > 0")])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_a_bad_softcap_is_refused_before_a_device_is_needed(entry, softcap, needle):
    lib = _capi.load()
    prefix = ENTRIES[entry][4]
    got = getattr(lib, entry)(ctypes.byref(_capped(entry, softcap)))
    if prefix is None:
        assert got == 0   # (the size query of a descriptor the launch refuses)
    else:
        assert got == -3 and _error(lib).startswith(prefix) and needle in _error(lib), _error(lib)
        if softcap == 0.0:
            assert ENTRIES[entry][3] in _error(lib), "the message for 0 names the uncapped twin"


@pytest.mark.parametrize("entry", [V + "backward_workspace_size", P + "workspace_size"])
def test_size_queries_equal_the_twins(entry):
    lib = _capi.load()
    twin = getattr(lib, ENTRIES[entry][3])(ctypes.byref(ENTRIES[entry][2]()))
    assert twin > 0 and getattr(lib, entry)(ctypes.byref(_capped(entry, 50.0))) == twin
    d = _capped(entry, 50.0)
    d.struct_size -= 8   # the twin's size is not this kind's
    assert getattr(lib, entry)(ctypes.byref(d)) == 0


def test_python_argument_errors_are_value_errors_before_any_launch():
    import torch
    q, k = torch.zeros(10, 4, 256, dtype=torch.bfloat16), torch.zeros(12, 2, 256, dtype=torch.bfloat16)
    cq, ck = torch.tensor([0, 5, 10], dtype=torch.int32), torch.tensor([0, 6, 12], dtype=torch.int32)
    cache, bt, cl = torch.zeros(4, 16, 2, 256, dtype=torch.bfloat16), torch.zeros(10, 2, dtype=torch.int32), torch.ones(10, dtype=torch.int32)
    calls = {"flash_attention_varlen_d256": lambda s: aule.flash_attention_varlen_d256_softcap(q, k, k, s, cq, ck),
             "flash_attention_paged_d256": lambda s: aule.flash_attention_paged_d256_softcap(q, cache, cache, s, bt, cl)}
    for twin, call in calls.items():
        for bad, reason in ((0, r"softcap is 0: for attention without a cap call %s\b" % twin), (-1.0, "finite value > 0, got -1.0"),
                            (float("inf"), "finite value > 0"), (float("nan"), "finite value > 0"), (torch.tensor(50.0), "Python float"), (None, "Python float")):
            with pytest.raises(ValueError, match=reason):
                call(bad)
    with pytest.raises(ValueError, match="flash_attention_varlen_d256_softcap takes head_dim 256 alone, got 128"):
        aule.flash_attention_varlen_d256_softcap(q[..., :128], k[..., :128], k[..., :128], 50.0, cq, ck)


@pytest.mark.parametrize("src,kernels", [("fa_varlen_d256_softcap_gfx950.hip", {"fa_fwd_varlen_d256_cap_kernel": 2, "fa_bwd_varlen_d256_cap_dq_kernel": 2,
                                                                                "fa_bwd_varlen_d256_cap_dkdv_kernel": 2}),
                                         ("fa_fwd_paged_d256_softcap_gfx950.hip", {"fa_fwd_paged_d256_cap_kernel": 4})])
def test_new_kernels_neither_spill_nor_use_scratch(src, kernels, tmp_path, monkeypatch):
    """every instance (fp16 and bf16; 16-bit and FP8 cache for the paged one) with what the Makefile's rule for the d256 files adds: no
    scratch, no spill, LDS within 160 KB; and nothing else is instantiated in the new files (the combine kernel least of all)"""
    line = util.makefile_compile_line() + "-Xclang -target-feature -Xclang -packed-fp32-ops".split()
    monkeypatch.setattr(util, "makefile_compile_line", lambda: line)
    res = util.resource_report(src, tmp_path)
    assert len(res) == sum(kernels.values()), list(res)
    for name, count in kernels.items():
        ks = {n: r for n, r in res.items() if name in n}
        assert len(ks) == count and sum("Bf16Traits" in n for n in ks) == count // 2 and sum("KvFp8" in n for n in ks) in (0, count // 2), (name, list(ks))
        assert all(r.get(x) == 0 for r in ks.values() for x in ("ScratchSize", "VGPRs Spill", "SGPRs Spill")), ks
        assert all(r.get("LDS Size") <= 160 * 1024 for r in ks.values()), ks
