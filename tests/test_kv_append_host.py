"""Paged KV cache append without a GPU: the slot arithmetic of aule.paged_slot_mapping against a Python loop, the argument
errors of aule.paged_kv_append (ValueErrors before any device use, AuleError for CPU tensors), the additive C-ABI
(symbol, descriptor layout, the uninitialised contract), the sanitizer build, and a resource audit of the compiled
kernel instances (no scratch, no spill, a true fp32 division, the hardware FP8 conversion, 16-byte accesses)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
NAME = "aule_kv_cache_append_ex"


# ---- paged_slot_mapping ---------------------------------------------------------------------------------------------

def _tables(rng, num_seqs, max_blocks):
    import torch
    perm = rng.permutation(num_seqs * max_blocks + 5)[:num_seqs * max_blocks]
    return torch.from_numpy(perm.reshape(num_seqs, max_blocks).astype(np.int32))


def _loop(bt, positions, bs, seq_ids=None):
    out = []
    for t, p in enumerate(positions):
        s = t if seq_ids is None else seq_ids[t]
        out.append(-1 if p < 0 else int(bt[s][p // bs]) * bs + p % bs)
    return out


def test_exports():
    for name in ("paged_kv_append", "paged_slot_mapping"):
        assert name in aule.__all__ and callable(getattr(aule, name)), name


@pytest.mark.parametrize("bs", [1, 8, 16, 48])
@pytest.mark.parametrize("pos_dtype", ["int32", "int64"])
def test_slot_mapping_decode_case(bs, pos_dtype):
    import torch
    rng = np.random.RandomState(bs)
    B, mb = 7, 9
    bt = _tables(rng, B, mb)
    pos = rng.randint(0, mb * bs, size=B)
    pos[2] = -1          # a padded sequence
    pos[5] = -40
    pos[0], pos[1] = 0, mb * bs - 1
    got = aule.paged_slot_mapping(bt, torch.from_numpy(pos).to(getattr(torch, pos_dtype)), bs)
    assert got.dtype == torch.int64 and got.shape == (B,)
    assert got.tolist() == _loop(bt.tolist(), pos.tolist(), bs)
    assert got[2] == -1 and got[5] == -1


@pytest.mark.parametrize("bs", [4, 16, 33])
def test_slot_mapping_prefill_with_seq_ids(bs):
    import torch
    rng = np.random.RandomState(100 + bs)
    B, mb = 4, 11
    bt = _tables(rng, B, mb).to(torch.int64)
    lens = [mb * bs, 1, 3 * bs + 2, bs]
    seq = np.concatenate([np.full(n, b) for b, n in enumerate(lens)])
    pos = np.concatenate([np.arange(n) for n in lens])
    pos[5] = -1
    order = rng.permutation(len(pos))           # tokens need not be sorted
    seq, pos = seq[order], pos[order]
    got = aule.paged_slot_mapping(bt, torch.from_numpy(pos), bs, seq_ids=torch.from_numpy(seq).to(torch.int32))
    assert got.tolist() == _loop(bt.tolist(), pos.tolist(), bs, seq.tolist())
    live = got[got >= 0]
    assert live.unique().numel() == live.numel()      # distinct (sequence, position) pairs -> distinct slots


def test_slot_mapping_argument_errors():
    import torch
    bt = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="block_size"):
        aule.paged_slot_mapping(bt, torch.zeros(2, dtype=torch.int64), 0)
    with pytest.raises(ValueError, match="seq_ids"):
        aule.paged_slot_mapping(bt, torch.zeros(5, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="shape of positions"):
        aule.paged_slot_mapping(bt, torch.zeros(5, dtype=torch.int64), 4, seq_ids=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="expected block_tables"):
        aule.paged_slot_mapping(bt[0], torch.zeros(2, dtype=torch.int64), 4)


# ---- argument errors of paged_kv_append -----------------------------------------------------------------------------

def _args(device, T=5, Hkv=2, D=64, nb=4, bs=8, dtype=None, cache_dtype=None):
    import torch
    dtype = dtype or torch.float16
    cache_dtype = cache_dtype or dtype
    k = torch.zeros(T, Hkv, D, dtype=dtype, device=device)
    v = torch.zeros(T, Hkv, D, dtype=dtype, device=device)
    kc = torch.zeros(nb, bs, Hkv, D, dtype=cache_dtype, device=device)
    vc = torch.zeros(nb, bs, Hkv, D, dtype=cache_dtype, device=device)
    slots = torch.zeros(T, dtype=torch.int64, device=device)
    return k, v, kc, vc, slots


@pytest.mark.parametrize("device", ["meta", "cpu"])
def test_argument_errors_are_value_errors_before_any_device_use(device):
    import torch
    f8 = torch.float8_e4m3fn
    k, v, kc, vc, sl = _args(device)
    T, Hkv, D = k.shape
    with pytest.raises(ValueError, match=r"expected key/value \[T,Hkv,D\]"):
        aule.paged_kv_append(k[0], v[0], kc, vc, sl)
    with pytest.raises(ValueError, match=r"expected key/value \[T,Hkv,D\]"):
        aule.paged_kv_append(k, v, kc[0], vc[0], sl)
    with pytest.raises(ValueError, match="key/value shape mismatch"):
        aule.paged_kv_append(k, v[:3], kc, vc, sl)
    with pytest.raises(ValueError, match="k_cache/v_cache shape mismatch"):
        aule.paged_kv_append(k, v, kc, vc[:2], sl)
    with pytest.raises(ValueError, match="head_dim mismatch: key=32, cache=64"):
        aule.paged_kv_append(k[..., :32], v[..., :32], kc, vc, sl)
    with pytest.raises(ValueError, match="heads_kv mismatch: key=1, cache=2"):
        aule.paged_kv_append(k[:, :1], v[:, :1], kc, vc, sl)
    with pytest.raises(ValueError, match="same dtype"):
        aule.paged_kv_append(k, v, kc, vc.to(f8), sl)
    for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
        co = kc.to(other)
        with pytest.raises(ValueError, match=r"float8_e4m3fn only.*OCP"):
            aule.paged_kv_append(k, v, co, co, sl)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        aule.paged_kv_append(k.float(), v.float(), kc.float(), vc.float(), sl)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        aule.paged_kv_append(k, v, kc.to(torch.bfloat16), vc.to(torch.bfloat16), sl)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        aule.paged_kv_append(k, v.to(torch.bfloat16), kc, vc, sl)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        aule.paged_kv_append(k, v, kc, vc, sl, k_scale=0.5)
    with pytest.raises(ValueError, match="float8_e4m3fn caches only"):
        aule.paged_kv_append(k, v, kc, vc, sl, v_scale=torch.ones(Hkv))
    with pytest.raises(ValueError, match=r"k_scale must be.*\[2\]"):
        aule.paged_kv_append(k, v, kc.to(f8), vc.to(f8), sl, k_scale=torch.ones(Hkv + 1))
    with pytest.raises(ValueError, match="v_scale must be"):
        aule.paged_kv_append(k, v, kc.to(f8), vc.to(f8), sl, v_scale=torch.ones(Hkv, 2))
    k256, v256, kc256, vc256, _ = _args(device, D=256)
    with pytest.raises(ValueError, match="head_dim must be one of"):
        aule.paged_kv_append(k256, v256, kc256, vc256, sl)
    wide_k, wide_v = _args(device, Hkv=2 * Hkv)[2:4]
    with pytest.raises(ValueError, match="must be contiguous"):
        aule.paged_kv_append(k, v, wide_k[:, :, ::2], wide_v[:, :, ::2], sl)
    k2 = torch.zeros(T, Hkv, 2 * D, dtype=k.dtype, device=device)
    with pytest.raises(ValueError, match="last dimension of key must be contiguous"):
        aule.paged_kv_append(k2[..., ::2], v, kc, vc, sl)
    with pytest.raises(ValueError, match="last dimension of value must be contiguous"):
        aule.paged_kv_append(k, k2[..., ::2], kc, vc, sl)
    with pytest.raises(ValueError, match="smaller than a row"):
        aule.paged_kv_append(k[:1].expand(T, Hkv, D), v, kc, vc, sl)
    with pytest.raises(ValueError, match="16-byte aligned"):
        aule.paged_kv_append(torch.zeros(T, Hkv, D + 4, dtype=k.dtype, device=device)[..., :D], v, kc, vc, sl)
    with pytest.raises(ValueError, match="slot_mapping must be an integer tensor"):
        aule.paged_kv_append(k, v, kc, vc, sl[:3])
    with pytest.raises(ValueError, match="slot_mapping must be an integer tensor"):
        aule.paged_kv_append(k, v, kc, vc, sl.float())
    cos = torch.ones(16, D // 2, device=device)
    sin = torch.zeros(16, D // 2, device=device)
    pos = torch.zeros(T, dtype=torch.int32, device=device)
    with pytest.raises(ValueError, match="cos and sin are required"):
        aule.paged_kv_append(k, v, kc, vc, sl, cos=cos, positions=pos)
    with pytest.raises(ValueError, match="cos and sin are required"):
        aule.paged_kv_append(k, v, kc, vc, sl, sin=sin, positions=pos)
    with pytest.raises(ValueError, match="cos and sin are required"):
        aule.paged_kv_append(k, v, kc, vc, sl, positions=pos)
    with pytest.raises(ValueError, match="positions are required"):
        aule.paged_kv_append(k, v, kc, vc, sl, cos=cos, sin=sin)
    with pytest.raises(ValueError, match="positions must be an integer tensor"):
        aule.paged_kv_append(k, v, kc, vc, sl, cos=cos, sin=sin, positions=pos[:2])
    with pytest.raises(ValueError, match=r"cos/sin must have shape \[\.\.\., 32\]"):
        aule.paged_kv_append(k, v, kc, vc, sl, cos=cos[:, :16], sin=sin[:, :16], positions=pos)


def test_cpu_tensors_raise_aule_error():
    """No fallback: well-formed CPU arguments are refused loudly, for both cache kinds and with the rotation."""
    import torch
    k, v, kc, vc, sl = _args("cpu")
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        aule.paged_kv_append(k, v, kc, vc, sl)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        aule.paged_kv_append(k, v, kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn), sl, k_scale=0.5,
                             cos=torch.ones(8, 32), sin=torch.zeros(8, 32), positions=torch.zeros(5, dtype=torch.int64))
    assert bool((kc == 0).all())


# ---- the C-ABI ------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    assert re.search(r"int32_t %s\s*\(const aule_kv_append_desc\*" % NAME, header)
    assert hasattr(ctypes.CDLL(_capi.find_library()), NAME)
    sig = {s[0]: s for s in _capi.SIGNATURES}[NAME]
    assert sig[1] is ctypes.c_int32 and sig[2] == [ctypes.POINTER(_capi.KvAppendDesc)]
    kernels = open(os.path.join(CSRC, "fa_kernels.h")).read()
    assert "launch_kv_append" in kernels
    assert "kv_append_gfx950.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    assert "sizeof(aule_kv_append_desc) = 168" in header
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_kv_append_desc) == 168" in capi
    D = _capi.KvAppendDesc
    assert ctypes.sizeof(D) == 168
    want = {"struct_size": 0, "dtype": 4, "cache_dtype": 8, "num_tokens": 12, "heads_kv": 16, "head_dim": 20, "num_blocks": 24,
            "block_size": 28, "key_token_stride": 32, "key_head_stride": 40, "value_token_stride": 48, "value_head_stride": 56,
            "table_len": 64, "table_pitch": 68, "device": 72, "reserved": 76, "stream": 80, "key": 88, "value": 96,
            "k_cache": 104, "v_cache": 112, "slot_mapping": 120, "k_scale": 128, "v_scale": 136, "cos": 144, "sin": 152,
            "positions": 160}
    assert [n for n, _ in D._fields_] == list(want)
    for name, off in want.items():
        assert getattr(D, name).offset == off, name
    # the field order of the C struct is the order of the binding
    body = re.search(r"typedef struct aule_kv_append_desc \{(.*?)\} aule_kv_append_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+);", body)
    assert names == list(want), names


def good_desc():
    d = _capi.KvAppendDesc()
    d.struct_size = ctypes.sizeof(_capi.KvAppendDesc)
    d.dtype, d.cache_dtype = 2, 0
    d.num_tokens, d.heads_kv, d.head_dim, d.num_blocks, d.block_size = 4, 2, 64, 8, 16
    d.key_token_stride = d.value_token_stride = 128
    d.key_head_stride = d.value_head_stride = 64
    d.device = -1
    d.key, d.value, d.k_cache, d.v_cache, d.slot_mapping = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    return d


BAD_FIELDS = [  # (field, value): every way the issue calls a descriptor bad
    ("struct_size", 160), ("struct_size", 0), ("dtype", 0), ("dtype", 3), ("cache_dtype", 2), ("head_dim", 96), ("head_dim", 256),
    ("head_dim", 33), ("heads_kv", 0), ("block_size", 0), ("key", None), ("value", None), ("k_cache", None), ("v_cache", None),
    ("slot_mapping", None), ("k_scale", 0x6000), ("v_scale", 0x6000), ("cos", 0x7000), ("sin", 0x7000), ("positions", 0x7000),
    ("table_len", 5), ("key_token_stride", 63), ("key_head_stride", 32), ("value_token_stride", 0), ("value_head_stride", -64),
    ("key_token_stride", 100), ("key", 0x1008),
]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_uninitialised_contract_without_a_gpu():
    """As the existing _ex calls: nothing is read before the library is initialised, so NULL, a good descriptor and every
    bad one report -1 here (on the GPU, tests/test_gpu_kv_append.py holds each of these to -3)."""
    lib = _capi.load()
    assert lib.aule_kv_cache_append_ex(None) in (-1, -3)
    assert lib.aule_kv_cache_append_ex(ctypes.byref(good_desc())) == -1
    assert b"not initialized" in lib.aule_get_error().lower()
    for field, bad in BAD_FIELDS:
        d = good_desc()
        setattr(d, field, bad)
        assert lib.aule_kv_cache_append_ex(ctypes.byref(d)) in (-1, -3), field


_SAN_CHILD = r'''
import ctypes, os, sys
sys.path.insert(0, os.path.join(%(root)r, "aule-attention_amd"))
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from aule import _capi
lib = _capi.load()
assert _capi.library_path().endswith("libaule_san.so"), _capi.library_path()
import test_kv_append_host as t
assert lib.aule_kv_cache_append_ex(None) in (-1, -3)
assert lib.aule_kv_cache_append_ex(ctypes.byref(_capi.KvAppendDesc())) in (-1, -3)
assert lib.aule_kv_cache_append_ex(ctypes.byref(t.good_desc())) == -1      # never initialised in this process
n = 0
for field, bad in t.BAD_FIELDS:
    d = t.good_desc()
    setattr(d, field, bad)
    assert lib.aule_kv_cache_append_ex(ctypes.byref(d)) in (-1, -3), field
    n += 1
if not os.path.exists("/dev/kfd"):
    assert lib.aule_init() == -1 and b"Failed to initialize backend" in lib.aule_get_error()
    assert lib.aule_kv_cache_append_ex(ctypes.byref(t.good_desc())) == -1
    assert lib.aule_attention_forward_ex(ctypes.byref(_capi.AttnDesc())) == -1
print("SANITIZED-OK", n)
'''


def test_sanitizer_build_and_its_no_gpu_contract():
    """`make san` builds with the new source in it, and the new entry point keeps the no-GPU contract under ASan + UBSan
    (the good descriptor's pointers are made up: they must never be read on the host)."""
    from test_capi_sanitizers import SAN_LIB, _asan_runtime, _sources_newer_than
    rt = _asan_runtime()
    if rt is None or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no clang ASan runtime / hipcc in this image")
    if not os.path.exists(SAN_LIB) or _sources_newer_than(SAN_LIB):
        r = subprocess.run(["make", "-C", CSRC, "san", "-j8"], capture_output=True, text=True, timeout=1500)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(SAN_LIB)
    env = dict(os.environ)
    env.update({"AULE_LIBRARY_PATH": SAN_LIB, "LD_PRELOAD": rt,
                "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1:abort_on_error=0:verify_asan_link_order=0",
                "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    env.pop("AULE_BACKEND", None)
    r = subprocess.run([sys.executable, "-c", _SAN_CHILD % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "SANITIZED-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


# ---- the compiled kernel --------------------------------------------------------------------------------------------

def test_kernel_instances_resources_and_instructions(tmp_path):
    """Eight instances (fp16 / bf16 x 16-bit / FP8 cache x plain / rotated): none spills or uses scratch; every global access
    is 16 bytes wide except the 8-byte code stores; the FP8 instances divide with the full v_div_scale / v_div_fmas /
    v_div_fixup sequence (correctly rounded -- a bare reciprocal multiply would differ at ties) and convert with
    v_cvt_pk_fp8_f32; no LDS."""
    src = os.path.join(CSRC, "kv_append_gfx950.hip")
    out = tmp_path / "kv_append.s"
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
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
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/(?:lane|block)\])?: (\d+)", line)
        if m and cur is not None:
            res[cur][m.group(1)] = int(m.group(2))
    kern = [n for n in res if "kv_append_kernel" in n]
    assert len(kern) == 8, kern
    for n in kern:
        assert res[n].get("ScratchSize") == 0 and res[n].get("VGPRs Spill") == 0 and res[n].get("SGPRs Spill") == 0, (n, res[n])
        assert res[n].get("LDS Size", 0) == 0, (n, res[n])
    asm = open(out).read()
    bodies = {}
    for n in kern:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(n), asm, flags=re.S | re.M)
        assert m, n
        bodies[n] = m.group(1)
    for n, body in bodies.items():
        fp8 = "Lb1ELb" in n                       # kv_append_kernel<E, FP8, ROPE>
        rope = n.endswith("Lb1EEEvNS0_14KvAppendParamsE")
        loads = re.findall(r"\b(global_load_\w+|flat_load_\w+|buffer_load_\w+)", body)
        stores = re.findall(r"\b(global_store_\w+|flat_store_\w+|buffer_store_\w+)", body)
        wide = [x for x in loads if x.endswith("dwordx4")]
        assert len(wide) == (8 if rope else 4), (n, loads)                  # K, V halves (+ 2 x 2 table quarters each of cos / sin)
        narrow = sorted(set(loads) - set(wide))
        assert all(x in ("global_load_dwordx2", "global_load_dword") for x in narrow), (n, narrow)   # slot, position, scales
        assert stores == ["global_store_dwordx2" if fp8 else "global_store_dwordx4"] * 4, (n, stores)
        assert ("v_cvt_pk_fp8_f32" in body) == fp8, n
        assert body.count("v_cvt_pk_fp8_f32") == (16 if fp8 else 0), n      # 32 codes, two per instruction
        assert (body.count("v_div_fixup_f32") == 32) == fp8 and ("v_div_scale_f32" in body) == fp8, n
        assert "ds_" not in body, n
