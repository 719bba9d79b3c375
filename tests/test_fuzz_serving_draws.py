"""What the fixed-seed slices of tools/fuzz_serving.py draw (tests/test_gpu_fuzz_serving.py runs them on the GPU): a fixed-seed fuzz is
only as good as what its seeds happen to reach, so the seeds are chosen for the conditions below and this file keeps them chosen.  It calls
the pure draw_* functions only -- no GPU, no torch -- and, for the key-split counts, the two plan hooks of the library, which answer
from the shape alone.  The hooks size the splits by the device's compute units: 256 here, MI355X's count, which is also what the
library assumes where no device answers."""
import ctypes
import importlib.util
import os

import pytest

from conftest import ROOT

from aule import _capi

spec = importlib.util.spec_from_file_location("fuzz_serving", os.path.join(ROOT, "tools", "fuzz_serving.py"))
fz = importlib.util.module_from_spec(spec)
spec.loader.exec_module(fz)

KINDS = ("prefill", "cascade", "mla", "varlen")


def _draws(kind):
    n, seed = fz.SLICES[kind]
    return fz.draws(kind, n, seed)


def test_the_slices_are_the_sizes_the_suite_promises():
    assert {k: fz.SLICES[k][0] for k in KINDS} == dict(prefill=30, cascade=20, mla=20, varlen=20)


@pytest.mark.parametrize("kind", KINDS)
def test_every_kind_draws_both_dtypes_every_head_dim_and_the_same_list_twice(kind):
    cfgs = _draws(kind)
    assert cfgs == _draws(kind)
    assert {c["dtype"] for c in cfgs} == {"bf16", "fp16"}
    if kind == "varlen":
        assert {c["D"] for c in cfgs} >= {32, 64, 128}
    elif kind != "mla":      # (MLA has the one latent width)
        assert {c["D"] for c in cfgs} == {32, 64, 128}
    for c in cfgs:           # plain values only: a configuration can be printed and read back
        assert eval(repr(c), {}) == c


def _seqs(cfgs):
    return [(c, n, L) for c in cfgs for n, L in zip(c["ns"], c["Ls"])]


@pytest.mark.parametrize("kind", ["prefill", "cascade"])
def test_ragged_slices(kind):
    cfgs = _draws(kind)
    g = lambda c: c["Hq"] // c["Hkv"]   # noqa: E731
    assert {c["kind"] for c in cfgs} == {"16", "fp8"}
    bss = {c["bs"] for c in cfgs}
    assert any(b > 1 and b & (b - 1) == 0 for b in bss) and any(b & (b - 1) for b in bss) and 1 in bss and any(b > 64 for b in bss), bss
    seqs = _seqs(cfgs)
    assert sum(1 for _, n, L in seqs if L < n) >= 3 and sum(1 for _, n, L in seqs if L == 0) >= 2 and sum(1 for _, n, L in seqs if n == 0) >= 2
    assert sum(1 for c, n, L in seqs if n * g(c) > 128) >= 3            # more than one row block
    assert sum(1 for c, n, L in seqs if (n * g(c)) % 32) >= 3           # a ragged last wave
    if kind == "prefill":
        assert sum(1 for c in cfgs if c["window"] > 0) >= 5
    else:
        assert all(c["window"] == -1 for c in cfgs)
    assert sum(1 for c in cfgs if c["q_pad"]) >= 3 and sum(1 for c in cfgs if c["lead"]) >= 3 and sum(1 for c in cfgs if c["scale_mul"] is not None) >= 3
    assert sum(1 for c in cfgs if c["tail"]) >= 1 and sum(1 for c in cfgs if c["table_len"] is not None) >= 1 and {c["extra_cols"] for c in cfgs} == {0, 2}
    uniform = [c for c in cfgs if len(set(c["ns"])) == 1 and 1 <= c["ns"][0] <= 64]
    assert len(uniform) >= 2 and any(c["ns"][0] == 1 for c in uniform), [c["ns"] for c in uniform]
    hard = [c["hard"][0] for c in cfgs if c["hard"] is not None]
    assert len(hard) >= 4 and set(hard) == {"spike", "offset"}, hard
    assert all(c["kind"] == "16" for c in cfgs if c["hard"] is not None)
    for c in cfgs:      # every draw is a valid call with something to compute
        assert sum(c["ns"]) >= 1 and c["Hq"] <= 32 and all(L >= 0 for L in c["Ls"])
        if c["hard"] is not None and c["hard"][0] == "spike":
            _, _, b, i, head, where, j = c["hard"]
            p = c["Ls"][b] - c["ns"][b] + i
            assert p >= 0 and head < c["Hq"] and (j < c["P"] if where == "prefix" else j <= p and (c["window"] <= 0 or p - j < c["window"]))


def _prefix_splits(c):
    geo = fz.ragged_geometry(c)
    d = _capi.PagedCascadeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = {"fp16": 1, "bf16": 2}[c["dtype"]], 1 if c["kind"] == "fp8" else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = geo["B"], c["Hq"], c["Hkv"], c["D"]
    d.block_size, d.max_blocks, d.max_prefix_blocks = c["bs"], geo["max_blocks"], geo["prefix_blocks"]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = geo["T"], geo["max_sq"], c["Hq"] * c["D"] + c["q_pad"]
    for n in ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "prefix_block_table", "prefix_len"):
        setattr(d, n, 4096)      # (16-byte aligned non-null dummies: the hook answers before any launch)
    if c["kind"] == "fp8":
        d.k_scale = d.v_scale = 4096
    plan = (ctypes.c_int32 * 7)()
    assert _capi.load().aule_hip_debug_shared_prefix_plan(ctypes.byref(d), plan, 7) == 7, c
    return plan[2]


def test_cascade_slice_prefixes_and_key_splits():
    cfgs = _draws("cascade")
    Ps = [(c["P"], c["bs"]) for c in cfgs]
    assert any(P == 0 for P, _ in Ps) and any(P % 64 for P, _ in Ps) and any(P % bs for P, bs in Ps) and any(P > 128 for P, _ in Ps), Ps
    assert any(P > 0 and P % bs == 0 for P, bs in Ps), Ps      # the concatenated-table cross-check runs
    assert {c["prefix_room"] for c in cfgs} == {False, True}
    splits = [_prefix_splits(c) for c in cfgs]
    assert sum(1 for n in splits if n > 1) >= 3, splits
    # ... with a split that holds no key of the prefix: more than one split of a table far larger than P
    assert any(n > 1 and c["prefix_room"] and c["P"] <= 129 for n, c in zip(splits, cfgs)), splits
    spikes = {c["hard"][5] for c in cfgs if c["hard"] is not None and c["hard"][0] == "spike"}
    assert spikes == {"prefix", "own"}, spikes                 # a spiked key in the shared prefix and one among a sequence's own keys


def _mla_splits(c):
    geo = fz.mla_geometry(c)
    d = _capi.MlaPagedDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = {"fp16": 1, "bf16": 2}[c["dtype"]], geo["B"], c["Hq"], 576, 512
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = c["bs"], geo["max_blocks"], geo["T"], geo["max_sq"]
    d.q_token_stride = (c["Hq"] + c["q_pad"]) * 576
    for n in ("q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "lse"):
        setattr(d, n, 4096)
    if c["ns"] is None:
        d.cu_seqlens_q = None
    plan = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(d), plan, 6) == 6, c
    return plan[2]


def test_mla_slice():
    cfgs = _draws("mla")
    splits = [_mla_splits(c) for c in cfgs]
    assert sum(1 for n in splits if n > 1) >= 5 and sum(1 for n in splits if n == 1) >= 3, splits
    assert any(c["Hq"] > 64 for c in cfgs)                                       # two row blocks per token
    assert {c["ns"] is None for c in cfgs} == {False, True}                      # decode and ragged
    assert {c["cache"] for c in cfgs} == {"16", "fp8"} and {c["scale"] is None for c in cfgs} == {False, True}
    fp8 = [c for c in cfgs if c["cache"] == "fp8"]
    assert any(c["kv_scale"] is None for c in fp8) and any(c["kv_scale"] is not None for c in fp8)
    assert all(0.25 <= c["kv_scale"] <= 2.0 for c in fp8 if c["kv_scale"] is not None)
    assert sum(1 for c in cfgs if c["ns"] is not None for n, L in zip(c["ns"], c["Ls"]) if L < n) >= 2
    assert {c["roomy"] for c in cfgs} == {False, True} and any(c["q_pad"] for c in cfgs) and any(c["lead"] for c in cfgs) and any(c["tail"] for c in cfgs)
    bss = {c["bs"] for c in cfgs}
    assert 1 in bss and any(b & (b - 1) for b in bss) and any(b > 1 and b & (b - 1) == 0 for b in bss), bss
    hard = [c["hard"][0] for c in cfgs if c["hard"] is not None]
    assert len(hard) >= 4 and set(hard) == {"spike", "offset"}, hard
    assert all(c["cache"] == "16" for c in cfgs if c["hard"] is not None)
    for c in cfgs:
        toks = c["ns"] if c["ns"] is not None else [1] * len(c["Ls"])
        assert sum(toks) >= 1 and (c["ns"] is not None or c["lead"] == c["tail"] == 0)


def test_varlen_slice():
    cfgs = _draws("varlen")
    for mask in ("none", "top", "br"):
        assert sum(1 for c in cfgs if c["mask"] == mask) >= 3, mask
    assert sum(1 for c in cfgs if c["window"] > 0) >= 4
    assert sum(1 for c in cfgs if c["max_sq"] is not None or c["max_sk"] is not None) >= 1
    assert sum(1 for c in cfgs if c["mask"] == "br" for n, L in zip(c["ns"], c["ls"]) if L < n) >= 2
    padded = [c for c in cfgs if c["wrapper"]]
    assert len(padded) >= 2 and all(c["D"] in (40, 96) for c in padded) and all(c["D"] in (32, 64, 128) for c in cfgs if not c["wrapper"])
    assert sum(1 for c in cfgs if c["strided"]) >= 3
    assert sum(1 for c in cfgs if c["scale_mul"] is not None) >= 3 and any(c["lead"] != (0, 0) for c in cfgs) and any(c["tail"] != (0, 0) for c in cfgs)
    for c in cfgs:
        assert sum(c["ns"]) >= 1 and sum(c["ls"]) >= 1
        if c["max_sq"] is not None:
            assert 1 <= c["max_sq"] < max(c["ns"])
        if c["max_sk"] is not None:
            assert 1 <= c["max_sk"] < max(c["ls"])
