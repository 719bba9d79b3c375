"""The launch plans of the ragged serving entries, pinned: the integers of the four plan hooks (paged MLA, sparse MLA, MLA indexer,
shared prefix) and the answers of the four workspace-size entries over a sweep of shapes, recorded from the library as it was before
the split rule, the length cut and the block-size shift were each written once (tests/golden/ragged_plans.json), and required of the
library as it is.  Host logic only: no GPU (256 compute units, what the plans assume without a device and what an MI355X has).

    python tests/test_ragged_plans_host.py --write      records the sweep from the library AULE_LIBRARY_PATH names
"""
import ctypes
import itertools
import json
import os
import sys

from conftest import GOLDEN

from aule import _capi

PATH = os.path.join(GOLDEN, "ragged_plans.json")
TOKENS, HEADS, BATCH = (1, 2, 5, 64, 300, 4096), (1, 16, 128), (1, 3, 64)
BLOCK_SIZE, MAX_BLOCKS, TOPK = (1, 16, 24, 64), (1, 15, 4096), (1, 64, 129, 2048, 65536)
KV_HEADS = {1: 1, 16: 4, 128: 8}   # of the cascade, per heads_q


def _max_sq(T):
    return sorted({1, 5, T})


def _ptrs(d, names, ragged):
    for n in names:
        setattr(d, n, 4096)
    if not ragged:
        d.cu_seqlens_q = None


def _mla(cls, T, H, B, msq, bs, mb, ragged):
    d = cls()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = 2, B, H, 576, 512
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q, d.q_token_stride = bs, mb, T, msq, H * 576
    _ptrs(d, ("q", "kv_cache", "block_tables", "context_lens", "cu_seqlens_q", "out"), ragged)
    return d


def _sparse(T, H, topk, bs):
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads_q, d.num_blocks, d.block_size, d.total_tokens, d.topk = 2, 0, H, 64, bs, T, topk
    d.q_token_stride = H * 576
    _ptrs(d, ("q", "kv_cache", "indices", "out"), True)
    return d


def _indexer(T, H, B, msq, bs, mb, ragged):
    d = _capi.MlaIndexerLogitsDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads, d.head_dim, d.batch = 2, 0, H, 128, B
    d.num_blocks, d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = 64, bs, mb, T, msq
    d.q_token_stride, d.logits_stride = H * 128, bs * mb
    _ptrs(d, ("q", "weights", "k_cache", "block_tables", "context_lens", "cu_seqlens_q", "logits"), ragged)
    return d


def _cascade(T, H, B, msq, bs, mb):
    d = _capi.PagedCascadeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, 0, B, H, KV_HEADS[H], 128
    d.block_size, d.max_blocks, d.max_prefix_blocks = bs, mb, mb
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, msq, H * 128
    _ptrs(d, ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "prefix_block_table", "prefix_len"), True)
    return d


def _hook(fn, d, n):
    """[return code, the integers it wrote]"""
    out = (ctypes.c_int32 * n)()
    rc = int(fn(ctypes.byref(d), out, n))
    return [rc] + list(out)[:max(rc, 0)]


def sweep(lib):
    """every case as [arguments..., hook answer, workspace-size answer(s)], in a fixed order"""
    rec = {"mla": [], "sparse": [], "indexer": [], "cascade": []}
    for T, H, B, bs, mb, ragged in itertools.product(TOKENS, HEADS, BATCH, BLOCK_SIZE, MAX_BLOCKS, (1, 0)):
        for msq in _max_sq(T):
            d, d8 = (_mla(c, T, H, B, msq, bs, mb, ragged) for c in (_capi.MlaPagedDesc, _capi.MlaPagedFp8Desc))
            d8.kv_scale = 4096
            rec["mla"].append([T, H, B, msq, bs, mb, ragged, _hook(lib.aule_hip_debug_mla_plan, d, 6),
                               int(lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d))),
                               int(lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d8)))])
            rec["indexer"].append([T, H, B, msq, bs, mb, ragged, _hook(lib.aule_hip_debug_mla_indexer_plan, _indexer(T, min(H, 64), B, msq, bs, mb, ragged), 5)])   # (the indexer has at most 64 heads)
            if ragged:
                d = _cascade(T, H, B, msq, bs, mb)
                rec["cascade"].append([T, H, B, msq, bs, mb, _hook(lib.aule_hip_debug_shared_prefix_plan, d, 7),
                                       int(lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d)))])
    for T, H, topk, bs in itertools.product(TOKENS, HEADS, TOPK, BLOCK_SIZE):
        d = _sparse(T, H, topk, bs)
        rec["sparse"].append([T, H, topk, bs, _hook(lib.aule_hip_debug_mla_sparse_plan, d, 6), int(lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(d)))])
    return rec


NARGS = {"mla": 7, "indexer": 7, "cascade": 6, "sparse": 4}   # the leading entries of a case that state the shape


def _wrapped(items, width=500):
    """JSON items, comma-separated, in lines of about `width` characters"""
    lines, cur = [], ""
    for s in (json.dumps(x, separators=(",", ":")) for x in items):
        if cur and len(cur) + len(s) > width:
            lines.append(cur)
            cur = ""
        cur += s + ","
    return "\n".join(lines + [cur[:-1]])


def test_the_plans_are_the_recorded_ones():
    """the file holds, per kind, the distinct answers and which of them every case of the sweep gets, in the sweep's order"""
    want = json.load(open(PATH))
    have = sweep(_capi.load())
    assert sorted(have) == sorted(want) == sorted(NARGS)
    for kind in sorted(want):
        answers, which = want[kind]["answers"], want[kind]["which"]
        assert len(have[kind]) == len(which) > 0, kind
        for case, w in zip(have[kind], which):
            assert case[NARGS[kind]:] == answers[w], (kind, case, answers[w])
    # the sweep reaches both sides of every rule: single and split launches, refusals
    mla = [a[0] for a in want["mla"]["answers"]]
    assert {a[0] for a in mla} == {6, -3} and any(a[3] > 1 for a in mla if a[0] == 6) and any(a[3] == 1 for a in mla if a[0] == 6)
    assert any(a[0][3] > 1 for a in want["sparse"]["answers"]) and any(a[0][3] > 1 for a in want["cascade"]["answers"] if a[0][0] == 7)


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        rec, parts = sweep(_capi.load()), []
        for kind in sorted(rec):
            answers = []
            for case in rec[kind]:
                if case[NARGS[kind]:] not in answers:
                    answers.append(case[NARGS[kind]:])
            which = [answers.index(case[NARGS[kind]:]) for case in rec[kind]]
            parts.append('"%s": {"answers": [\n%s\n], "which": [\n%s\n]}' % (kind, _wrapped(answers), _wrapped(which)))
        with open(PATH, "w") as f:
            f.write("{\n" + ",\n".join(parts) + "\n}\n")
        print("wrote", PATH, os.path.getsize(PATH), "bytes from", _capi.library_path())
