"""Sparse MLA attention without a GPU: the additive C-ABI (symbols, the descriptor's layout, every answer the entry gives before it
needs a device, the agreement of the launch, the size query and the plan hook), the invariants of the launch plan over a sweep of
shapes, the argument errors of the torch layer, the build rule and a resource audit of the kernels compiled with the Makefile's
compiler and flags: the four new instances without scratch or spill, the dense MLA instances at the figures recorded from the parent
commit in profiles/mla_sparse_resources.txt."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT
from util import resource_report

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
ENTRY, SIZE, HOOK = "aule_attention_mla_sparse_ex", "aule_attention_mla_sparse_workspace_size", "aule_hip_debug_mla_sparse_plan"
PTRS = ("q", "kv_cache", "indices", "out", "lse")
LAYOUT = dict(struct_size=0, dtype=4, cache_dtype=8, heads_q=12, num_blocks=16, block_size=20, total_tokens=24, topk=28, scale=32,
              device=36, q_token_stride=40, stream=48, q=56, kv_cache=64, indices=72, kv_scale=80, out=88, lse=96, workspace=104,
              workspace_bytes=112)
MAX_SPLIT = 64
FIGURES = ("VGPRs", "AGPRs", "ScratchSize", "SGPRs Spill", "VGPRs Spill", "LDS Size")


def _fill(T=8, Hq=16, topk=2048, nb=64, bs=64, dtype=2, fp8=False):
    """a well-formed descriptor whose pointers are 16-byte aligned non-null dummies: only ever handed to calls that answer before a launch"""
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads_q, d.num_blocks, d.block_size, d.total_tokens, d.topk = dtype, int(fp8), Hq, nb, bs, T, topk
    d.q_token_stride = Hq * 576
    for n in PTRS:
        setattr(d, n, 4096)
    if fp8:
        d.kv_scale = 4096
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def _plan(lib, d):
    out = (ctypes.c_int32 * 6)()
    n = lib.aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 6)
    return n, list(out)


def _ws_formula(nsplit, T, Hq):
    return (nsplit * T * Hq * 514 * 4 + 15) // 16 * 16 if nsplit > 1 else 0


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name in (ENTRY, SIZE, HOOK):
        assert re.search(r"\b%s\s*\(const aule_mla_sparse_desc\*" % name, header), name
        assert hasattr(lib, name) and name in bound, name
    assert bound[SIZE][1] is ctypes.c_uint64
    force = "aule_hip_debug_mla_sparse_launch_nsplit"   # the bench's debug launch
    assert re.search(r"\b%s\s*\(const aule_mla_sparse_desc\* desc, int32_t nsplit\)" % force, header) and hasattr(lib, force) and force in bound
    assert "flash_attention_mla_sparse" in aule.__all__ and callable(aule.flash_attention_mla_sparse)
    sig = inspect.signature(aule.flash_attention_mla_sparse)
    assert list(sig.parameters) == ["q", "kv_cache", "indices", "scale", "return_lse", "kv_scale"]
    assert sig.parameters["scale"].default is None and sig.parameters["kv_scale"].default is None and sig.parameters["return_lse"].default is False
    # the docstring's last line names what is out of scope
    last = " ".join(aule.flash_attention_mla_sparse.__doc__.split("Out of scope:")[1].split())
    for what in ("indexer", "causal rule", "Hq < 64", "block table", "backward", "sink logits or tree masks"):
        assert what in last, what
    assert "fuzz_serving" not in last      # (tools/fuzz_serving.py has the `sparse` kind)


def test_descriptor_layout_matches_the_header():
    """ctypes against the numbers include/aule.h states and aule_capi.cpp pins with a static_assert."""
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(aule_mla_sparse_desc) = 120" in header and "sizeof(aule_mla_sparse_desc) == 120" in capi
    assert ctypes.sizeof(_capi.MlaSparseDesc) == 120
    assert [n for n, _ in _capi.MlaSparseDesc._fields_] == list(LAYOUT)
    for name, off in LAYOUT.items():
        assert getattr(_capi.MlaSparseDesc, name).offset == off, name
    body = header.split("typedef struct aule_mla_sparse_desc {")[1].split("}")[0]
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) == len(LAYOUT) - 1
    for name, off in quoted:
        assert LAYOUT[name] == int(off), name
    pinned = re.findall(r"offsetof\(aule_mla_sparse_desc, (\w+)\) == (\d+)", capi)
    assert len(pinned) == len(LAYOUT) - 1
    for name, off in pinned:
        assert LAYOUT[name] == int(off), name
    assert ctypes.sizeof(_capi.MlaPagedDesc) == 136 and ctypes.sizeof(_capi.MlaPagedFp8Desc) == 144   # the neighbours keep their sizes


# (field, bad value, a piece of the reason): what the shape alone decides -- the launch, the size query and the plan hook all refuse
BAD_SHAPE = [
    ("struct_size", 0, "struct_size"), ("struct_size", 136, "struct_size"),
    ("dtype", 0, "dtype 0"), ("dtype", 3, "dtype 3"),
    ("cache_dtype", 2, "cache_dtype 2"), ("cache_dtype", -1, "cache_dtype -1"),
    ("heads_q", 0, "heads_q (0)"), ("heads_q", -4, "heads_q (-4)"),
    ("topk", 0, "topk (0)"), ("topk", 65537, "topk (65537)"), ("topk", -1, "topk (-1)"),
    ("num_blocks", 0, "num_blocks * block_size (0 * 64)"), ("block_size", 0, "num_blocks * block_size (64 * 0)"),
    ("block_size", 1 << 25, "num_blocks * block_size (64 * 33554432)"),
    ("total_tokens", -1, "total_tokens (-1)"),
    ("q_token_stride", 16 * 576 - 8, "q_token_stride (9208) is smaller than a token"), ("q_token_stride", 0, "smaller than a token"),
    ("q_token_stride", 16 * 576 + 4, "q_token_stride (9220) must be a multiple of 8"),
    ("total_tokens", 0x7fffffff // 16, "32 bits"),
]
# ... and what only a launch looks at
BAD_POINTER = [(n, None, "null tensor pointer") for n in ("q", "kv_cache", "indices", "out")] + [
    ("q", 4096 + 8, "16-byte aligned"), ("out", 4096 + 2, "16-byte aligned"), ("kv_cache", 4097, "16-byte aligned"),
    ("indices", 4098, "indices must be 4-byte aligned"), ("kv_scale", 4096, "kv_scale applies to an FP8 cache only")]
_ids = lambda x: str(x).replace(" ", "_")   # noqa: E731


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE + BAD_POINTER, ids=_ids)
def test_launch_refuses_each_bad_field(field, bad, needle):
    """-3 and a reason naming the field and its value, before the device is needed (so also in a process that never initialised the library)"""
    lib = _capi.load()
    d = _fill()
    setattr(d, field, bad)
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3
    assert needle in _error(lib) and _error(lib).startswith("Sparse MLA attention failed: "), _error(lib)


def test_fp8_scale_rules_and_the_workspace_rule():
    lib = _capi.load()
    d = _fill(fp8=True)
    d.kv_scale = None
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3 and "null kv_scale" in _error(lib)
    d.kv_scale = 4098
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3 and "kv_scale must be 4-byte aligned" in _error(lib)
    # a caller workspace smaller than the plan's, or misaligned, is refused: nothing is launched
    d = _fill(T=1)
    need = lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d))
    assert need == _ws_formula(_plan(lib, d)[1][2], 1, 16) > 0
    d.workspace, d.workspace_bytes = 4096, need - 16
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3
    assert "workspace_bytes (%d) is smaller than the plan's %d" % (need - 16, need) in _error(lib)
    d.workspace, d.workspace_bytes = 4096 + 8, need
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3 and "workspace must be 16-byte aligned" in _error(lib)
    # ... and neither host query looks at it
    assert lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)) == need and _plan(lib, d)[0] == 6


def test_forced_split_count_keeps_every_rule_of_the_entry():
    """aule_hip_debug_mla_sparse_launch_nsplit: the entry's checker with the plan of the forced count; nsplit < 1 is refused"""
    lib = _capi.load()
    force = lib.aule_hip_debug_mla_sparse_launch_nsplit
    for bad in (0, -1):
        assert force(ctypes.byref(_fill()), bad) == -3 and "nsplit (%d) must be at least 1" % bad in _error(lib)
    assert force(None, 4) == -3 and "struct_size" in _error(lib)
    d = _fill()
    d.topk = 0
    assert force(ctypes.byref(d), 4) == -3 and "topk (0)" in _error(lib)
    d = _fill(T=0)
    assert force(ctypes.byref(d), 4) == 0
    # a caller workspace is held to the forced count's size: T = 1, 16 heads, topk 2048 -- the plan says 16, 32 needs twice the bytes
    d = _fill(T=1)
    need = lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d))
    d.workspace, d.workspace_bytes = 4096, need
    assert force(ctypes.byref(d), 32) == -3 and "workspace_bytes (%d) is smaller than the plan's %d" % (need, _ws_formula(32, 1, 16)) in _error(lib)
    assert force(ctypes.byref(d), 64) == -3 and "the plan's %d" % _ws_formula(32, 1, 16) in _error(lib)   # (32 tiles: at most 32 ranges)
    if not os.path.exists("/dev/kfd"):
        assert force(ctypes.byref(d), 16) == -1 and force(ctypes.byref(d), 8) == -1   # past every check: the device is needed


def test_null_descriptor_and_packed_row_overflow():
    lib = _capi.load()
    assert lib.aule_attention_mla_sparse_ex(None) == -3 and "struct_size" in _error(lib)
    assert lib.aule_attention_mla_sparse_workspace_size(None) == 0 and _plan(lib, _fill())[0] == 6
    assert lib.aule_hip_debug_mla_sparse_plan(None, None, 0) == -3
    # (total_tokens + 64) * heads_q must fit 32 bits
    last = 0x7fffffff // 128 - 64
    d = _fill(T=last + 1, Hq=128)
    d.q_token_stride = 128 * 576
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3 and "32 bits" in _error(lib)
    assert _plan(lib, d)[0] == -3 and lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)) == 0
    d.total_tokens = last
    assert _plan(lib, d)[0] == 6


@pytest.mark.parametrize("field,bad,needle", BAD_SHAPE, ids=_ids)
def test_size_query_plan_hook_and_launch_give_the_same_verdict(field, bad, needle):
    """one checker: what the launch refuses on the shape the size query answers with 0 and the hook with -3"""
    lib = _capi.load()
    d = _fill(T=2)   # 2 tokens x 1 row block: split, so the accepted size is not 0
    n, plan = _plan(lib, d)
    assert n == 6 and plan[2] >= 2
    assert lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)) == _ws_formula(plan[2], 2, 16) > 0
    setattr(d, field, bad)
    assert lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)) == 0
    assert _plan(lib, d)[0] == -3
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3


@pytest.mark.parametrize("field,bad,needle", BAD_POINTER, ids=_ids)
def test_size_query_and_plan_hook_read_no_pointer(field, bad, needle):
    """the pointer rules are the launch's alone: both host queries answer a descriptor with bad or null pointers as they answer a good one"""
    lib = _capi.load()
    for fp8 in (False, True):
        d = _fill(T=2, fp8=fp8)
        want = (lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)), _plan(lib, d))
        assert want[0] > 0
        setattr(d, field, bad)
        assert (lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)), _plan(lib, d)) == want
        for n in PTRS + ("kv_scale", "workspace"):
            setattr(d, n, None)
        assert (lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)), _plan(lib, d)) == want


def test_nothing_to_do_returns_zero_without_a_launch():
    """total_tokens = 0: 0 with null pointers, in any process; a refused field is still refused"""
    lib = _capi.load()
    d = _fill(T=0)
    for n in PTRS:
        setattr(d, n, None)
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == 0
    assert lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)) == 0
    assert _plan(lib, d)[0] == 0
    d.topk = 0
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -3 and _plan(lib, d)[0] == -3


def test_plan_hook_capacity_contract():
    lib = _capi.load()
    d = _fill()
    out = (ctypes.c_int32 * 6)()
    assert lib.aule_hip_debug_mla_sparse_plan(ctypes.byref(d), None, 0) == -6
    assert lib.aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 5) == -6 and list(out) == [0] * 6
    assert lib.aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 6) == 6


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
def test_entry_reports_uninitialised_without_a_gpu():
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(_fill())) == -1
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(_fill(fp8=True, T=1))) == -1
    d = _fill(T=300, Hq=128)   # one split: no workspace
    d.q_token_stride, d.lse = 128 * 576, None
    assert lib.aule_attention_mla_sparse_ex(ctypes.byref(d)) == -1


def test_plan_invariants_over_a_sweep():
    """(256 compute units: what the hook assumes without a device, and what an MI355X has)"""
    lib = _capi.load()
    seen_split = seen_single = 0
    for T in (1, 2, 3, 8, 64, 255, 256, 257, 4096):
        for Hq in (1, 16, 63, 64, 65, 128):
            for topk in (1, 63, 64, 65, 127, 128, 129, 200, 512, 2048, 4097, 65536):
                d = _fill(T=T, Hq=Hq, topk=topk)
                d.q_token_stride = Hq * 576
                n, (rb, rows, nsplit, grid, lo, hi) = _plan(lib, d)
                key = (T, Hq, topk)
                tiles = (topk + 63) // 64
                assert n == 6 and rows == 64 and rb == (Hq + 63) // 64, key
                assert 1 <= nsplit <= min(MAX_SPLIT, max(1, tiles // 2)), key
                assert nsplit == max(1, min(-(-256 // (T * rb)), MAX_SPLIT, tiles // 2)), key
                assert grid == T * rb * nsplit, key
                ws = (hi << 32) | (lo & 0xffffffff)
                assert ws == _ws_formula(nsplit, T, Hq) == lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)), key
                # every tile belongs to exactly one split
                per = -(-tiles // nsplit)
                assert (nsplit - 1) * per < tiles or nsplit * per >= tiles, key
                seen_split += nsplit > 1
                seen_single += nsplit == 1
                # the cache kind does not change the plan
                d8 = _fill(T=T, Hq=Hq, topk=topk, fp8=True)
                assert _plan(lib, d8) == (n, [rb, rows, nsplit, grid, lo, hi]), key
    assert seen_split > 50 and seen_single > 50


def test_python_argument_errors_are_value_errors_before_the_device():
    import torch
    T, Hq, topk, nb, bs = 3, 4, 8, 5, 16
    q = torch.zeros(T, Hq, 576, dtype=torch.bfloat16)
    kv = torch.zeros(nb, bs, 576, dtype=torch.bfloat16)
    idx = torch.zeros(T, topk, dtype=torch.int32)
    call = aule.flash_attention_mla_sparse
    for bad in (idx.long(), idx.to(torch.int16), idx.to(torch.uint8)):
        with pytest.raises(ValueError, match=r"indices must be int32 .*got torch\.(int64|int16|uint8)"):
            call(q, kv, bad)
    with pytest.raises(ValueError, match="indices must be int32"):
        call(q, kv, idx.float())
    with pytest.raises(ValueError, match="kv_scale applies to a float8_e4m3fn cache only"):
        call(q, kv, idx, kv_scale=0.5)
    with pytest.raises(ValueError, match=r"topk .* must be in 1 \.\. 65536, got 0"):
        call(q, kv, idx[:, :0])
    with pytest.raises(ValueError, match=r"topk .* must be in 1 \.\. 65536, got 65537"):
        call(q, kv, torch.zeros(T, 65537, dtype=torch.int32))
    with pytest.raises(ValueError, match="the latent width must be 576"):
        call(q[..., :512], kv, idx)
    with pytest.raises(ValueError, match="the latent width must be 576"):
        call(q, kv[..., :512], idx)
    with pytest.raises(ValueError, match=r"expected q \[T,Hq,576\]"):
        call(q[0], kv, idx)
    with pytest.raises(ValueError, match=r"indices must be a \[3, topk\]"):
        call(q, kv, idx[:2])
    with pytest.raises(ValueError, match=r"indices must be a \[3, topk\]"):
        call(q, kv, idx.view(T, 2, 4))
    with pytest.raises(ValueError, match="an FP8 latent cache must be torch.float8_e4m3fn, got torch.float8_e4m3fnuz"):
        call(q, kv.to(torch.float8_e4m3fnuz), idx)
    with pytest.raises(ValueError, match="an FP8 latent cache must be torch.float8_e4m3fn, got torch.float16"):
        call(q, kv.half(), idx)
    with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
        call(q, kv.to(torch.float8_e4m3fn), idx, kv_scale=torch.ones(2))
    with pytest.raises(ValueError, match="kv_cache must be contiguous"):
        call(q, torch.zeros(nb, 2 * bs, 576, dtype=torch.bfloat16)[:, ::2], idx)
    with pytest.raises(ValueError, match="indices must be contiguous"):
        call(q, kv, torch.zeros(T, 2 * topk, dtype=torch.int32)[:, ::2])
    with pytest.raises(ValueError, match="1 .. 2\\^31 - 1 slots"):
        call(q, kv[:0], idx)
    with pytest.raises(ValueError, match="no backward"):
        call(q.clone().requires_grad_(True), kv, idx)
    with pytest.raises(ValueError, match="no backward"):
        call(q, kv.clone().requires_grad_(True), idx)
    with pytest.raises(ValueError, match="must be fp16 or bf16"):
        call(q.float(), kv.float(), idx)
    wide = torch.zeros(T, Hq * 576 + 4, dtype=torch.bfloat16)[:, :Hq * 576].view(T, Hq, 576)
    with pytest.raises(ValueError, match="q's token stride.*multiples of 8 elements"):
        call(wide, kv, idx)
    # well-formed, on the CPU: both cache kinds, the 4-d cache, [T, 1, topk] indices, a slice of a wider projection, an un-paged latent
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, kv, idx, return_lse=True)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(q, kv.view(nb, bs, 1, 576).to(torch.float8_e4m3fn), idx.view(T, 1, topk), kv_scale=torch.ones(1), scale=192 ** -0.5)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        call(torch.zeros(T, Hq + 2, 576, dtype=torch.bfloat16)[:, :Hq], kv.view(nb * bs, 1, 576), idx)
    with torch.no_grad():
        with pytest.raises(aule.AuleError, match="no CPU fallback"):
            call(q.clone().requires_grad_(True), kv, idx)


def test_build_rule_names_the_new_source():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = [w for line in re.findall(r"^SRCS [:+]= (.*)$", mk, re.M) for w in line.split()]
    assert "fa_fwd_mla_sparse_gfx950.hip" in srcs and len(srcs) == len(set(srcs)) and os.path.exists(os.path.join(CSRC, "fa_fwd_mla_sparse_gfx950.hip"))
    dep = re.search(r"^\$\(OBJDIR\)/fa_fwd_mla_sparse_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert {"fa_d256_common.h", "fa_paged_tile.h", "fa_mla_common.h"} <= set(dep)
    # the body is stated once: the new unit instantiates it, it does not copy it
    text = open(os.path.join(CSRC, "fa_fwd_mla_sparse_gfx950.hip")).read()
    assert '#include "fa_mla_common.h"' in text and "mla_paged_body<T, Kv16, true>" in text and "mfma16" not in text


def _recorded(kind):
    """{(kernel, traits): the six figures} of the `kind` lines of profiles/mla_sparse_resources.txt"""
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "mla_sparse_resources.txt")):
        f = line.split()
        if len(f) == 9 and f[0] == kind:
            rows[(f[1], f[2])] = dict(zip(FIGURES, map(int, f[3:])))
    return rows


def _figures(res, kernel, traits):
    ks = [n for n in res if kernel in n and "_%d%s" % (len(traits), traits) in n]
    assert len(ks) == 1, (kernel, traits, list(res))
    return {k: res[ks[0]].get(k) for k in FIGURES}


def test_resource_audit_new_instances_clean_and_dense_instances_unchanged(tmp_path):
    """the four new instances: __launch_bounds__(256, 1), 111 616 bytes of LDS, no scratch, no spill; the dense MLA instances: the six
    figures the parent commit's compile gave (recorded in profiles/mla_sparse_resources.txt), every one"""
    parent, sparse = _recorded("parent"), _recorded("sparse")
    assert len(parent) == 4 and len(sparse) == 4
    units = {}
    for i, src in enumerate(("fa_fwd_mla_paged_gfx950.hip", "fa_fwd_mla_paged_fp8_gfx950.hip", "fa_fwd_mla_sparse_gfx950.hip")):
        sub = tmp_path / str(i)
        sub.mkdir()
        units[src] = resource_report(src, sub)
    where = {"fa_fwd_mla_paged_kernel": "fa_fwd_mla_paged_gfx950.hip", "fa_mla_fp8_latent_kernel": "fa_fwd_mla_paged_fp8_gfx950.hip",
             "fa_fwd_mla_sparse_kernel": "fa_fwd_mla_sparse_gfx950.hip", "fa_mla_sparse_fp8_kernel": "fa_fwd_mla_paged_fp8_gfx950.hip"}
    for (kernel, traits), want in parent.items():
        got = _figures(units[where[kernel]], kernel, traits)
        print("dense ", kernel, traits, got)
        assert got == want, (kernel, traits, got, want)
    for (kernel, traits), noted in sparse.items():
        got = _figures(units[where[kernel]], kernel, traits)
        print("sparse", kernel, traits, got)
        assert got["ScratchSize"] == 0 and got["SGPRs Spill"] == 0 and got["VGPRs Spill"] == 0 and got["LDS Size"] == 111616, (kernel, traits, got)
        assert got["VGPRs"] <= 256 and got["AGPRs"] <= 256, (kernel, traits, got)
        assert got == noted, (kernel, traits, got, noted)   # the file reports what the compiler says
    # the new unit holds the 16-bit instances and nothing else of the MLA; the combine is not instantiated a second time
    assert sorted(n for n in units["fa_fwd_mla_sparse_gfx950.hip"]) == sorted(n for n in units["fa_fwd_mla_sparse_gfx950.hip"] if "fa_fwd_mla_sparse_kernel" in n)
    assert len(units["fa_fwd_mla_sparse_gfx950.hip"]) == 2
