"""Tree masks without a GPU: the three additive C-ABI symbols, the two descriptor layouts (each its twin field for field, tree_mask
appended), every answer the entries give before they need a device, the workspace-size rule, the Python signatures and argument
errors, tree_mask_from_parents against a brute-force ancestor walk, and the resource audit of the two kernel sources."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

import aule
from aule import _capi

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")

# entry -> (descriptor struct, ctypes class, result type)
ENTRIES = {
    "aule_attention_paged_query_tree_ex": ("aule_paged_query_tree_desc", _capi.PagedQueryTreeDesc, ctypes.c_int32),
    "aule_attention_paged_query_tree_workspace_size": ("aule_paged_query_tree_desc", _capi.PagedQueryTreeDesc, ctypes.c_uint64),
    "aule_attention_paged_prefill_tree_ex": ("aule_paged_prefill_tree_desc", _capi.PagedPrefillTreeDesc, ctypes.c_int32),
}

# kind -> (struct, class, size, twin struct, twin class)
LAYOUTS = {
    "prefill": ("aule_paged_prefill_tree_desc", _capi.PagedPrefillTreeDesc, 160, "aule_paged_prefill_desc", _capi.PagedPrefillDesc),
    "query": ("aule_paged_query_tree_desc", _capi.PagedQueryTreeDesc, 160, "aule_paged_query_desc", _capi.PagedQueryDesc),
}
LAUNCH = {"prefill": "aule_attention_paged_prefill_tree_ex", "query": "aule_attention_paged_query_tree_ex"}
PREFIX = {"prefill": "Paged prefill tree attention failed: ", "query": "Paged query tree attention failed: "}


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


def test_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    lib = ctypes.CDLL(_capi.find_library())
    bound = {s[0]: s for s in _capi.SIGNATURES}
    for name, (struct, cls, restype) in ENTRIES.items():
        assert re.search(r"\b%s\s*\(const %s\*" % (name, struct), header), name
        assert hasattr(lib, name) and name in bound, name
        assert bound[name][1] is restype and bound[name][2][0]._type_ is cls, name


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_descriptor_layouts_repeat_the_twin_and_append_tree_mask(kind):
    """size, field order, the twin's offsets through the whole prefix, tree_mask at the twin's sizeof; the same numbers in the
    header's text and in aule_capi.cpp's static_asserts"""
    struct, cls, size, twin_struct, twin = LAYOUTS[kind]
    header = open(os.path.join(ROOT, "include", "aule.h")).read()
    capi = open(os.path.join(CSRC, "aule_capi.cpp")).read()
    assert "sizeof(%s) = %d" % (struct, size) in header
    assert "sizeof(%s) == %d" % (struct, size) in capi
    assert ctypes.sizeof(cls) == size == ctypes.sizeof(twin) + 8
    names = [n for n, _ in cls._fields_]
    assert names == [n for n, _ in twin._fields_] + ["tree_mask"]
    for n, t in twin._fields_:
        assert getattr(cls, n).offset == getattr(twin, n).offset and getattr(cls, n).size == getattr(twin, n).size, n
    assert cls.tree_mask.offset == ctypes.sizeof(twin) == 152 and cls.tree_mask.size == 8
    assert "offsetof(%s, tree_mask) == 152" % struct in capi
    assert "offsetof(%s, tree_mask) == sizeof(%s)" % (struct, twin_struct) in capi
    # the header: the same fields in the same order, every offset it quotes, and an int64 word type
    body = header.split("typedef struct %s {" % struct)[1].split("} %s;" % struct)[0]
    declared = [n for line in re.sub(r"/\*.*?\*/", "", body).split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", line.strip())]
    assert declared == names, declared
    assert "const int64_t* tree_mask;" in body
    quoted = re.findall(r"(\w+);\s*/\* offset (\d+)", body)
    assert len(quoted) >= 4 and "tree_mask" in {n for n, _ in quoted}
    for n, off in quoted:
        assert getattr(cls, n).offset == int(off), n
    # the twins keep their sizes
    assert [ctypes.sizeof(c) for c in (_capi.PagedPrefillDesc, _capi.PagedQueryDesc)] == [152, 152]


# ---- well-formed descriptors whose pointers are aligned non-null dummies: only ever handed to calls that answer before a launch

def _paged(kind, B=3, Hq=8, Hkv=2, D=64, T=40):
    d = _capi.PagedPrefillTreeDesc() if kind == "prefill" else _capi.PagedQueryTreeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, 0, B, Hq, Hkv, D
    d.block_size, d.max_blocks, d.window_size = 16, 8, -1
    ptrs = ["q", "k_cache", "v_cache", "block_tables", "context_lens", "out", "lse", "tree_mask"]
    if kind == "prefill":
        d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, 20, Hq * D
        ptrs.append("cu_seqlens_q")
    else:
        d.seq_q = 5
    for n in ptrs:
        setattr(d, n, 4096)
    return d


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_null_mask_window_and_wrong_sizes_are_refused_before_the_device(kind):
    """-3 with a reason, in a process that never called aule_init()"""
    lib = _capi.load()
    entry = getattr(lib, LAUNCH[kind])
    assert entry(None) == -3 and "struct_size" in _error(lib)
    d = _paged(kind)
    d.tree_mask = None
    assert entry(ctypes.byref(d)) == -3
    assert _error(lib).startswith(PREFIX[kind]) and "null tree_mask pointer" in _error(lib), _error(lib)
    for w in (1, 16, 4096):
        d = _paged(kind)
        d.window_size = w
        assert entry(ctypes.byref(d)) == -3
        assert _error(lib).startswith(PREFIX[kind]) and "window is not defined over a tree" in _error(lib), _error(lib)
    twin_size = ctypes.sizeof(LAYOUTS[kind][4])
    for bad in (0, 8, twin_size, ctypes.sizeof(d) + 8):       # the twin's own size included: a descriptor without words is not read as one
        d = _paged(kind)
        d.struct_size = bad
        assert entry(ctypes.byref(d)) == -3 and "struct_size" in _error(lib), (bad, _error(lib))
    # the twin's rules hold through the prefix: one of each family
    d = _paged(kind)
    d.head_dim = 48
    assert entry(ctypes.byref(d)) == -3 and "head_dim 48" in _error(lib)
    d = _paged(kind)
    d.heads_kv = 3
    assert entry(ctypes.byref(d)) == -3 and "divisible" in _error(lib)
    d = _paged(kind)
    d.q = None
    assert entry(ctypes.byref(d)) == -3 and "null tensor pointer" in _error(lib)
    if kind == "query":
        d = _paged(kind)
        d.seq_q = 65
        assert entry(ctypes.byref(d)) == -3 and "seq_q 65" in _error(lib), _error(lib)
        assert lib.aule_attention_paged_query_tree_workspace_size(ctypes.byref(d)) == 0


@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_nothing_to_do_returns_zero_without_a_launch(kind):
    """the twin's rule, with every pointer null, in any process"""
    lib = _capi.load()
    entry = getattr(lib, LAUNCH[kind])
    for field in {"prefill": ("total_tokens", "batch", "heads_q"), "query": ("batch", "heads_q")}[kind]:
        d = _paged(kind)
        setattr(d, field, 0)
        if field == "heads_q" and kind != "query":
            d.q_token_stride = 0
        for n, t in d._fields_:
            if t is ctypes.c_void_p and n != "stream":
                setattr(d, n, None)
        assert entry(ctypes.byref(d)) == 0, (kind, field, _error(lib))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="needs a box WITHOUT a GPU")
@pytest.mark.parametrize("kind", sorted(LAYOUTS))
def test_entries_report_uninitialised_without_a_gpu(kind):
    """a descriptor that passes every check needs the device: -1 where there is none"""
    lib = _capi.load()
    assert getattr(lib, LAUNCH[kind])(ctypes.byref(_paged(kind))) == -1


def test_query_workspace_is_the_twins():
    lib = _capi.load()
    for B, Hq, Hkv, D, Sq, blocks in ((3, 8, 2, 64, 5, 8), (64, 64, 8, 64, 1, 512), (2, 4, 4, 128, 64, 40), (8, 32, 8, 128, 32, 514)):
        d = _paged("query", B=B, Hq=Hq, Hkv=Hkv, D=D)
        d.seq_q, d.max_blocks = Sq, blocks
        twin = _capi.PagedQueryDesc()
        ctypes.memmove(ctypes.byref(twin), ctypes.byref(d), ctypes.sizeof(twin))
        twin.struct_size = ctypes.sizeof(twin)
        want = int(lib.aule_attention_paged_query_workspace_size(ctypes.byref(twin)))
        assert want > 0 and int(lib.aule_attention_paged_query_tree_workspace_size(ctypes.byref(d))) == want
        for n, t in d._fields_:
            if t is ctypes.c_void_p:
                setattr(d, n, None)               # host logic only: no pointer is read
        assert int(lib.aule_attention_paged_query_tree_workspace_size(ctypes.byref(d))) == want
    assert lib.aule_attention_paged_query_tree_workspace_size(None) == 0


def test_python_signatures_and_defaults():
    for name in ("flash_attention_paged_query_tree", "flash_attention_paged_prefill_tree", "tree_mask_from_parents"):
        assert name in aule.__all__ and callable(getattr(aule, name)), name
    sig = inspect.signature(aule.flash_attention_paged_query_tree)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "tree_mask", "block_tables", "context_lens", "scale", "k_scale", "v_scale",
                                    "return_lse"]
    p = sig.parameters
    assert p["scale"].default is None and p["k_scale"].default is None and p["v_scale"].default is None and p["return_lse"].default is False
    sig = inspect.signature(aule.flash_attention_paged_prefill_tree)
    assert list(sig.parameters) == ["q", "k_cache", "v_cache", "tree_mask", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q",
                                    "scale", "k_scale", "v_scale", "return_lse"]
    p = sig.parameters
    assert p["max_seqlen_q"].default is None and p["scale"].default is None and p["k_scale"].default is None
    assert p["v_scale"].default is None and p["return_lse"].default is False
    assert list(inspect.signature(aule.tree_mask_from_parents).parameters) == ["parents"]
    # no window over a tree; the twins keep their signatures
    for f in (aule.flash_attention_paged_query_tree, aule.flash_attention_paged_prefill_tree):
        assert "window_size" not in inspect.signature(f).parameters and "sinks" not in inspect.signature(f).parameters
    assert list(inspect.signature(aule.flash_attention_paged_query).parameters) == [
        "q", "k_cache", "v_cache", "block_tables", "context_lens", "scale", "window_size", "k_scale", "v_scale", "return_lse"]
    assert list(inspect.signature(aule.flash_attention_paged_prefill).parameters) == [
        "q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "max_seqlen_q", "scale", "window_size", "k_scale", "v_scale",
        "return_lse"]
    for f in (aule.flash_attention_paged_query, aule.flash_attention_paged_prefill, aule.flash_attention_paged_query_sinks,
              aule.flash_attention_paged_prefill_sinks):
        assert "tree_mask" not in inspect.signature(f).parameters
    for f in (aule.flash_attention_paged_query_tree, aule.flash_attention_paged_prefill_tree):
        for phrase in ("Out of scope", "sliding windows", "sink logits", "cascade", "MLA", "head_dim 256", "more than", "backward"):
            assert phrase in f.__doc__, (f.__name__, phrase)


def test_tree_mask_argument_errors_are_value_errors_before_any_launch():
    """CPU tensors: wrong shape, dtype, device or layout of tree_mask is a ValueError in both calls; the twin's rules still come first;
    a well-formed CPU call is an AuleError (no fallback)."""
    import torch
    Hq, Hkv, D, B, Sq, T = 8, 2, 64, 2, 3, 10
    q = torch.zeros(T, Hq, D, dtype=torch.float16)
    cq = torch.tensor([0, 5, 10], dtype=torch.int32)
    cache = torch.zeros(4, 16, Hkv, D, dtype=torch.float16)
    bt = torch.zeros(B, 2, dtype=torch.int32)
    cl = torch.tensor([7, 9], dtype=torch.int32)
    q4 = torch.zeros(B, Hq, Sq, D, dtype=torch.float16)
    calls = {
        "prefill": (lambda m: aule.flash_attention_paged_prefill_tree(q, cache, cache, m, bt, cl, cq), (T,)),
        "query": (lambda m: aule.flash_attention_paged_query_tree(q4, cache, cache, m, bt, cl), (B, Sq)),
    }
    for name, (call, shape) in calls.items():
        good = torch.zeros(shape, dtype=torch.int64)
        for bad in (torch.zeros(shape + (1,), dtype=torch.int64), torch.zeros(shape[:-1] + (shape[-1] + 1,), dtype=torch.int64),
                    torch.zeros((), dtype=torch.int64), good.flatten()[:-1], [0] * shape[-1], None, 7):
            with pytest.raises(ValueError, match=r"tree_mask must be a"):
                call(bad)
        for bad in (good.int(), good.double(), good.bool(), good.to(torch.uint8)):
            with pytest.raises(ValueError, match="tree_mask must be int64"):
                call(bad)
        wide = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=torch.int64)[..., ::2]
        assert wide.shape == good.shape and not wide.is_contiguous()
        with pytest.raises(ValueError, match="tree_mask must be contiguous"):
            call(wide)
        with pytest.raises(ValueError, match="tree_mask must be on q's device"):
            call(torch.zeros(shape, dtype=torch.int64, device="meta"))
        for ok in (good, torch.full(shape, -1, dtype=torch.int64)):
            with pytest.raises(aule.AuleError, match="no CPU fallback"):
                call(ok)
    # the twin's own rules are still checked, and first
    with pytest.raises(ValueError, match="1 to 64 query tokens"):
        aule.flash_attention_paged_query_tree(torch.zeros(B, Hq, 65, D, dtype=torch.float16), cache, cache,
                                              torch.zeros(B, 65, dtype=torch.int64), bt, cl)
    with pytest.raises(ValueError, match=r"cu_seqlens_q must be a \[batch \+ 1\]"):
        aule.flash_attention_paged_prefill_tree(q, cache, cache, torch.zeros(T, dtype=torch.int64), bt, cl, cq[:2])


# ---- tree_mask_from_parents

def _ancestor_words(parents):
    """brute force: walk from every node to the context, as Python integers, then as signed 64-bit values"""
    words = []
    for i in range(len(parents)):
        w, j = 0, i
        while True:
            w |= 1 << j
            p = parents[j]
            if not 0 <= p < j:
                break
            j = p
        words.append(w - (1 << 64) if w >= 1 << 63 else w)
    return words


def test_tree_mask_from_parents_matches_an_ancestor_walk():
    import torch
    g = torch.Generator().manual_seed(20)
    top_bit = 0
    for n in (1, 2, 5, 31, 32, 33, 63, 64):
        for trial in range(12):
            i = torch.arange(n)
            # a valid parent below i, bent towards long paths in every other draw, with a few roots and out-of-range values
            par = (torch.rand(n, generator=g) * i).long() if trial % 2 else torch.maximum(i - 1 - torch.randint(0, 3, (n,), generator=g), i * 0)
            par = torch.where(torch.rand(n, generator=g) < 0.1, torch.randint(-5, n + 5, (n,), generator=g), par)
            got = aule.tree_mask_from_parents(par)
            assert got.dtype == torch.int64 and got.shape == (n,) and got.device == par.device
            assert got.tolist() == _ancestor_words(par.tolist()), (n, trial, par.tolist())
            top_bit += n == 64 and bool((got < 0).any())
            for dt in (torch.int32, torch.int16):
                assert torch.equal(aule.tree_mask_from_parents(par.to(dt)), got)
    assert top_bit >= 6                    # bit 63 is set in many draws at seq_q = 64
    # batched: each row its own tree
    rows = [torch.randint(-2, 40, (40,), generator=g) for _ in range(5)]
    got = aule.tree_mask_from_parents(torch.stack(rows))
    assert got.shape == (5, 40) and got.tolist() == [_ancestor_words(r.tolist()) for r in rows]


def test_tree_mask_from_parents_chain_star_and_out_of_range():
    import torch
    i = torch.arange(64)
    chain = aule.tree_mask_from_parents(i - 1)
    want = [(2 << k) - 1 for k in range(64)]
    assert chain.tolist() == [w - (1 << 64) if w >= 1 << 63 else w for w in want] and chain[63].item() == -1
    star = aule.tree_mask_from_parents(torch.zeros(64, dtype=torch.int64))       # every node a child of node 0 (node 0: of the context)
    assert star.tolist() == _ancestor_words([0] * 64) and star[0].item() == 1 and star[5].item() == (1 << 5) | 1
    assert star[63].item() == -(1 << 63) + 1
    # anything outside [0, i): a child of the context -- the self bit alone
    for par in ([-1] * 7, [7, 8, 9, 10, 11, 12, 13], [0, 1, 2, 3, 4, 5, 6], [-(1 << 40)] * 7, [1 << 40] * 7):
        assert aule.tree_mask_from_parents(torch.tensor(par)).tolist() == [1 << k for k in range(7)], par
    assert aule.tree_mask_from_parents(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    for bad in (torch.zeros(3), torch.zeros(2, 2, 2, dtype=torch.int64), torch.zeros(65, dtype=torch.int64), [0, 0], torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            aule.tree_mask_from_parents(bad)


# ---- the kernels

def _resource_usage(src, tmp_path):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "tree.o"), os.path.join(CSRC, src)],
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
    return res


@pytest.mark.parametrize("src,kernel,lds,twins", [
    ("fa_fwd_splitkv_gfx950.hip", "fa_fwd_paged_tree_kernel", 32 * 1024, {"fa_fwd_paged_query_kernel": 12, "fa_fwd_splitkv_kernel": 18}),
    ("fa_fwd_paged_prefill_gfx950.hip", "fa_fwd_paged_prefill_tree_kernel", 40 * 1024, {"fa_fwd_paged_prefill_kernel": 12})])
def test_tree_kernels_neither_spill_nor_use_scratch(src, kernel, lds, twins, tmp_path):
    """fp16, bf16 x D 32, 64, 128 x the two cache kinds, under a name of their own: the instance counts the existing audits pin
    (12 paged-query, 18 split-KV, 12 paged-prefill) are those of the other names"""
    res = _resource_usage(src, tmp_path)
    ks = [n for n in res if kernel in n]
    assert len(ks) == 12 and sum("KvFp8" in n for n in ks) == 6 and sum("Kv16" in n for n in ks) == 6, ks
    assert sum("Bf16Traits" in n for n in ks) == 6 and sum("F16Traits" in n for n in ks) == 6
    for d in (32, 64, 128):
        assert sum("ELi%dE" % d in n for n in ks) == 4, (d, ks)
    for n in ks:
        r_ = res[n]
        assert r_.get("ScratchSize") == 0, (n, r_)
        assert r_.get("VGPRs Spill") == 0, (n, r_)
        assert r_.get("SGPRs Spill") == 0, (n, r_)
        assert r_.get("LDS Size") <= lds, (n, r_)
    for twin, count in twins.items():
        assert not any(twin in n for n in ks) and sum(twin in n for n in res) == count, (twin, sum(twin in n for n in res))


def test_no_source_file_is_added_and_the_bodies_are_written_once():
    """SRCS is unchanged: the tree kernels live in the two existing sources.  The split-KV body is the include the object rule already
    names, now compiled three times; the prefill body stays in its .hip, which includes itself for each of its two kernels."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert len(srcs) == 25 and "fa_fwd_splitkv_gfx950.hip" in srcs and "fa_fwd_paged_prefill_gfx950.hip" in srcs
    assert not [f for f in os.listdir(CSRC) if "tree" in f]
    deps = re.search(r"^\$\(OBJDIR\)/fa_fwd_splitkv_gfx950\.o: (.*)$", mk, re.M).group(1).split()
    assert "fa_fwd_splitkv_body.inc" in deps
    split = open(os.path.join(CSRC, "fa_fwd_splitkv_gfx950.hip")).read()
    assert split.count('#include "fa_fwd_splitkv_body.inc"') == 3 and split.count("TREE = false") == 2 and split.count("TREE = true") == 1
    prefill = open(os.path.join(CSRC, "fa_fwd_paged_prefill_gfx950.hip")).read()
    assert prefill.count('#include "fa_fwd_paged_prefill_gfx950.hip"') == 2 and prefill.count("#ifdef AULE_PAGED_PREFILL_BODY") == 1
    assert prefill.count("constexpr bool TREE = false;") == 1 and prefill.count("constexpr bool TREE = true;") == 1
    assert prefill.count("fast_exp2(m - mu)") == 1          # (the softmax step is still written once: tests/test_tile_attention_host.py)
