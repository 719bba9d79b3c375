"""Paged attention for short multi-token queries without a GPU: the additive C-ABI (symbols, descriptor layout, the
workspace query against an independent restatement of the launch plan, refused descriptors), the argument errors of the
torch layer, and a resource audit of the multi-query kernel instances (no scratch, no VGPR or SGPR spill)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
NEW = ("aule_attention_paged_query_ex", "aule_attention_paged_query_workspace_size")


def _fill(B, Hq, Hkv, Sq, D, bs, max_blocks, dtype=2, cache_dtype=0, window=-1):
    d = _capi.PagedQueryDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = dtype, cache_dtype
    d.batch, d.heads_q, d.heads_kv, d.head_dim, d.seq_q = B, Hq, Hkv, D, Sq
    d.block_size, d.max_blocks, d.window_size = bs, max_blocks, window
    return d


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0] for s in _capi.SIGNATURES}
    for name in NEW:
        assert re.search(r"\b%s\s*\(const aule_paged_query_desc\*" % name, header), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert "flash_attention_paged_query" in aule.__all__ and callable(aule.flash_attention_paged_query)


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    assert "sizeof(aule_paged_query_desc) = 152" in header
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_paged_query_desc) == 152" in capi
    D = _capi.PagedQueryDesc
    assert ctypes.sizeof(D) == 152
    assert D.stream.offset == 48 and D.workspace.offset == 104 and D.workspace_bytes.offset == 112
    assert D.k_scale.offset == 120 and D.v_scale.offset == 128
    assert D.lse.offset == 136 and D.seq_q.offset == 144 and D.cache_dtype.offset == 148
    for name, off in re.findall(r"(\w+);\s*/\* offset (\d+)", header.split("typedef struct aule_paged_query_desc")[1].split("}")[0]):
        assert getattr(D, name).offset == int(off), name
    # the FP8 decode descriptor is its prefix, field for field, and stays at 136 bytes
    assert ctypes.sizeof(_capi.PagedFp8Desc) == 136
    for name, _ in _capi.PagedFp8Desc._fields_:
        assert getattr(D, name).offset == getattr(_capi.PagedFp8Desc, name).offset, name


def _plan_bytes(B, Hq, Hkv, Sq, D, bs, max_blocks):
    """wave_chunk_plan (csrc/fa_fwd_splitkv_gfx950.hip) restated: 32-row tiles of the Hq / Hkv * Sq packed rows of a
    (batch, KV head) unit, the 32-key tiles shared out over about 2048 waves, four waves per workgroup; one fp32 partial
    row of D + 2 floats per wave and packed row."""
    nrt = -(-(Hq // Hkv * Sq) // 32)
    units = B * Hkv * nrt
    ntiles = -(-(max_blocks * bs) // 32)
    want_waves = -(-2048 // units)
    chunk = max(1, -(-ntiles // want_waves))
    nwaves = -(-ntiles // chunk)
    npart = -(-nwaves // 4) * 4
    return npart * units * 32 * (D + 2) * 4


SHAPES = [  # B, Hq, Hkv, Sq, D, block_size, max_blocks
    (8, 32, 8, 4, 128, 16, 2048), (8, 32, 8, 1, 128, 16, 2048), (2, 16, 2, 7, 64, 24, 90), (1, 4, 1, 64, 64, 128, 17),
    (3, 8, 8, 40, 32, 1, 700), (4, 32, 8, 5, 128, 16, 5), (1, 64, 8, 9, 128, 48, 417),
]


@pytest.mark.parametrize("cache_dtype", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d-H%dkv%d-Sq%d-D%d-bs%d-mb%d" % s)
def test_workspace_query_equals_the_plan(shape, cache_dtype):
    lib = _capi.load()
    for dtype in (1, 2):
        d = _fill(*shape, dtype=dtype, cache_dtype=cache_dtype)
        assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)) == _plan_bytes(*shape)


@pytest.mark.parametrize("B,Hq,Hkv,D,bs,mb", [(8, 32, 8, 128, 16, 2048), (2, 32, 1, 64, 128, 40), (3, 8, 8, 32, 1, 700)])
def test_one_token_plans_like_the_decode(B, Hq, Hkv, D, bs, mb):
    """seq_q = 1 is the decode bit for bit, which needs the decode's plan."""
    lib = _capi.load()
    d16 = _capi.PagedDesc()
    d16.struct_size = ctypes.sizeof(d16)
    d16.dtype = 2
    d16.batch, d16.heads_q, d16.heads_kv, d16.head_dim, d16.block_size, d16.max_blocks = B, Hq, Hkv, D, bs, mb
    want = lib.aule_attention_paged_decode_workspace_size(ctypes.byref(d16))
    assert want > 0
    for cache_dtype in (0, 1):
        d = _fill(B, Hq, Hkv, 1, D, bs, mb, cache_dtype=cache_dtype)
        assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)) == want


def test_workspace_query_refuses_bad_descriptors():
    lib = _capi.load()
    good = (8, 32, 8, 4, 128, 16, 64)
    assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(_fill(*good))) > 0
    assert lib.aule_attention_paged_query_workspace_size(None) == 0
    for field, bad in (("struct_size", 136), ("struct_size", 0), ("dtype", 0), ("dtype", 3), ("cache_dtype", 2), ("cache_dtype", -1),
                       ("head_dim", 256), ("head_dim", 48), ("heads_kv", 5), ("heads_kv", 0), ("seq_q", 0), ("seq_q", 65),
                       ("block_size", 0), ("max_blocks", 0)):
        d = _fill(*good)
        setattr(d, field, bad)
        assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)) == 0, (field, bad)
    d = _fill(*good)
    d.batch = 0          # nothing to do
    assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)) == 0
    d = _fill(*good)
    d.seq_q = 64         # the largest query
    assert lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)) == _plan_bytes(8, 32, 8, 64, 128, 16, 64)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    lib = _capi.load()
    assert lib.aule_attention_paged_query_ex(ctypes.byref(_fill(8, 32, 8, 4, 128, 16, 64))) == -1


def test_argument_errors_are_value_errors_before_any_launch():
    """Through aule.flash_attention_paged_query with CPU tensors: every rule is checked before the library is loaded or a
    device touched, so each is reachable, and raised, without a GPU; a well-formed CPU call is an AuleError (no fallback)."""
    import torch
    B, Hq, Hkv, Sq, D, bs = 2, 8, 2, 4, 64, 16
    q = torch.zeros(B, Hq, Sq, D, dtype=torch.float16)
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cl = torch.full((B,), Sq, dtype=torch.int32)
    call = aule.flash_attention_paged_query
    with pytest.raises(ValueError, match=r"expected q \[B,Hq,Sq,D\]"):
        call(q[:, :, 0], c16, c16, bt, cl)                      # the decode's 3-D query
    with pytest.raises(ValueError, match=r"expected q \[B,Hq,Sq,D\]"):
        call(q, c16, c16[:2], bt, cl)
    with pytest.raises(ValueError, match="head_dim mismatch"):
        call(q, torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), torch.zeros(4, bs, Hkv, 32, dtype=torch.float16), bt, cl)
    with pytest.raises(ValueError, match="divisible"):
        call(q, torch.zeros(4, bs, 3, D, dtype=torch.float16), torch.zeros(4, bs, 3, D, dtype=torch.float16), bt, cl)
    with pytest.raises(ValueError, match="1 to 64 query tokens"):
        call(torch.zeros(B, Hq, 65, D, dtype=torch.float16), c16, c16, bt, cl)
    with pytest.raises(ValueError, match="1 to 64 query tokens"):
        call(torch.zeros(B, Hq, 0, D, dtype=torch.float16), c16, c16, bt, cl)
    with pytest.raises(ValueError, match="same dtype"):
        call(q, c8, c16, bt, cl)
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        co = torch.zeros(4, bs, Hkv, D).to(other)
        with pytest.raises(ValueError, match=r"float8_e4m3fn only.*OCP"):
            call(q, co, co, bt, cl)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q.float(), c8, c8, bt, cl)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        call(q, c16.to(torch.bfloat16), c16.to(torch.bfloat16), bt, cl)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        call(q, c16, c16, bt, cl, k_scale=0.5)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        call(q, c16, c16, bt, cl, v_scale=torch.ones(Hkv))
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        call(q, c8, c8, bt, cl, k_scale=torch.ones(Hkv + 1))
    with pytest.raises(ValueError, match=r"v_scale must be"):
        call(q, c8, c8, bt, cl, v_scale=torch.ones(Hkv, 2))
    with pytest.raises(ValueError, match="head_dim must be one of"):
        c256 = torch.zeros(4, bs, Hkv, 256, dtype=torch.float16)
        call(torch.zeros(B, Hq, Sq, 256, dtype=torch.float16), c256, c256, bt, cl)
    with pytest.raises(ValueError, match="block_size"):
        c0 = torch.zeros(4, 0, Hkv, D, dtype=torch.float16)
        call(q, c0, c0, bt, cl)
    for bad_bt, bad_cl in ((bt[0], cl), (bt[:1], cl), (bt, cl[:1]), (bt[:, :0], cl), (bt, cl.view(B, 1))):
        with pytest.raises(ValueError, match="block_tables must be"):
            call(q, c16, c16, bad_bt, bad_cl)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, c16, c16, bt, cl)
    # the decode keeps the reference's rule
    with pytest.raises(ValueError, match="single query token"):
        aule._torch.paged_decode(q, c16, c16, bt, cl)


def test_query_kernels_neither_spill_nor_use_scratch(tmp_path):
    """fa_fwd_paged_query_kernel<T, D, KV>: fp16, bf16 x D 32, 64, 128 x the two paged sources; the D = 128 instances are
    the register-heavy ones (a 16-bit cache: one wave per SIMD, as the decode instance)."""
    src = os.path.join(CSRC, "fa_fwd_splitkv_gfx950.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "splitkv.o"), src],
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
    mq = [n for n in res if "fa_fwd_paged_query_kernel" in n]
    assert len(mq) == 12 and sum("KvFp8" in n for n in mq) == 6 and sum("Kv16" in n for n in mq) == 6, mq
    for n in mq:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
