#!/usr/bin/env python3
"""Randomised differential test of the serving and packing entry points, the companion of tools/fuzz_parity.py (which covers the dense
forward / backward, the paged DECODE, RoPE, split-KV and windows):

    prefill   flash_attention_paged_prefill, and on the same draw flash_attention_paged_query / flash_attention_paged_amd where they apply
    cascade   flash_attention_paged_cascade and merge_attention_states
    mla       flash_attention_mla_paged and flash_attention_mla_paged_fp8
    varlen    aule_attention_varlen_forward_ex / _backward_ex, and the Python wrapper for head dims that are padded
    sinks     flash_attention_varlen_sinks (forward and backward), _paged_prefill_sinks, _paged_query_sinks and the C entries behind them
    tree      flash_attention_paged_query_tree and flash_attention_paged_prefill_tree
    mlapf     aule_attention_mla_prefill_ex / _backward_ex (192 / 128) and flash_attention_mla_varlen
    sparse    aule_attention_mla_sparse_ex and flash_attention_mla_sparse
    indexer   aule_mla_indexer_logits_ex / _topk_ex, mla_indexer_logits / _topk / mla_indexer, and their lists through the sparse MLA
    fp8mma    aule_attention_paged_prefill_fp8mma_ex and flash_attention_paged_prefill_fp8mma

    python tools/fuzz_serving.py KIND [n=100] [seed=0]          deterministic per seed; prints every failing configuration
    python tools/fuzz_serving.py one KIND "<cfg as printed>" SEED    one printed configuration again

Each kind is a pure draw and a run.  draw_KIND(rng) -> cfg (a dict of plain values; no torch, no GPU, no library call) and
run_KIND(cfg, seed) -> (cfg, errs) calls the library.  Every drawn call is a VALID call: hostile offsets, stale lengths and refusals belong to
tests/test_gpu_hostile_*.py, the *_refusals tests and the *_host.py files.  The judges are those of the hand-written test files
(Ragged, Cascade, Problem's conventions, Case, Fp8Case, Packed / Run and their _judge functions; for the newer kinds Batch / Paged,
QueryProblem / PrefillProblem and the MLA backward's Packed / Run): the fp64 oracle on the same quantised inputs, -inf / zeros /
never-written rows exactly.

Every kind caps the cost of its judge (shrinking batch, then heads, then lengths) near 0.2 s of fp64 work per draw.

Hard data (prefill, cascade, mla; 16-bit caches; forward only): one draw in four has either one key replaced by m * (a query row that sees
it) -- m = 20, or 8 for MLA: a logit in the hundreds at a random place of the keys -- or a constant c in {2, 4} added to every key of
one KV head (MLA: to the 64 rotary columns), which moves all logits of a row alike.  `out` keeps fwd_tol; the LSE bound becomes
max(LSE_ATOL, 4 x the error a plain NumPy fp32 log-sum-exp of the same rows has against the fp64 judge): fp32 arithmetic error grows
with |S|, and the kernels take two hardware transcendental steps on top of fp32 sums.  The bound never looks at the kernel's result.
Gradients under a sharp softmax are out of scope (the varlen kind stays on Gaussian data and BWD_TOL).

sinks: one draw picks the entry (varlen / prefill / query) and everything else.  sinks[h] = cycle[(h + rot) % 5] with the cycle (-inf, -30,
0, ln(Lmax) + 0.5, ln(Lmax) + 6), Lmax the most keys a row of the draw sees; one draw in six passes them in q's dtype and the judge sees the
rounded values.  Bars: fwd_tol, LSE 1e-3, BWD_TOL; rows without a key out == 0 and lse == sinks[h] exactly; the prefill and varlen legs
run the C entries into 0xFF-filled buffers.  Relations: the -inf heads are the sinkless entry bit for bit; two runs give the same bits; a
uniform batch (n <= 64) agrees between the prefill and the query entry within 2 x fwd_tol.  dsinks is held to max(DSINKS_BAR[dtype],
4 x e_model): e_model = |dsinks_model - dsinks_ref| / max(1, max|dsinks_ref|), dsinks_model the fp64 reduction with O rounded to the storage
dtype before delta = rowsum(dO * O) is formed -- the term DESIGN.md 3.12 names as the dominant one; the bound is computed from the reference
alone (sinks_reference, no GPU) and never reads the kernel's result.

The gradient floor (sinks: dq, dk; mlapf: dq, dk_nope, dk_pe): the backward entries are given O in 16 bits and form delta from it, and on
rows of a few keys dS = P (dP - delta) cancels down to that rounding, which BWD_TOL does not cover (two draws of the 150-draw runs at seed 1
showed it).  So an element may miss the judge by max(BWD_TOL's bound, 4 x e) where e is the largest difference between the
fp64 gradient formula on the exact O and on O rounded to storage (test_gpu_sinks.grads_model, test_gpu_mla_backward.rounding_model; per
draw for the sinks, per sequence for MLA).  From the reference alone; the hand files pass no floor and keep plain BWD_TOL.

tree: the entry (query / prefill), both caches, page sizes 1 .. 128, scale, lead / tail rows and a strided q for the prefill.  The words of
a sequence are drawn by kind (a random tree, random words, random words with emptied rows, all ones, the chain) from the data seed;
behind the drawn sequences every draw carries one more, a probe -- emptied rows in front of at most one key of context -- so that on the
reference alone the judge under the words is far from the judge under the chain.  Relations: chain sequences and sequences of more than 64 tokens (whose words are
garbage, as those of unowned rows) equal the plain entry bit for bit; two runs give the same bits.

mlapf: heads 1 .. 32, three masks, scale, lead / tail rows on both axes, cuts by max_seqlen_*, the three memory layouts of
tests/test_gpu_mla_backward.py::Run, and one draw in five through flash_attention_mla_varlen with autograd on slices of wider projections.
Relations: two runs give the same bits in all six outputs; sequence 0 alone equals the same sequence in the batch bit for bit (dk_pe where
both launches cut the heads into the same chunks).

sparse: dtype, a 16-bit or FP8 latent cache, 1 .. 6 tokens, heads 1 .. 128, lists of 1 .. 2048 entries over caches of 5 .. 4096 slots (block
size 1, powers of two and others; the small caches make every longer list repeat slots), scale (a negative one included), a padded q, the
caller's workspace at exactly the queried size or the library's.  Per token a share of invalid entries (none, scattered, one whole 64-entry
tile, one whole key range of the launch, all; the values -1, S, INT32_MIN, INT32_MAX) and whether its list is drawn from a few slots.  Gaussian
data hides a single list entry once a list is long (one entry of 2048 moves `out` by half its bound; tests/test_fuzz_serving_draws.py keeps
that measured), so one draw in three is hard (16-bit caches): a SEAM PROBE -- on one token, heads 0 .. min(Hq, 16) - 1 each take one
list position from the seam set (0, 63, 64, topk - 1, the first and last entry of every key range of the launch -- the plan's, from
aule_hip_debug_mla_sparse_plan, or the forced count's -- the valid entries next to an invalid run, then random ones), and the slot named
there holds 8 sign(scale) q[t, h]: a logit near 190, so that losing or misreading that one entry moves that head by hundreds of bounds; one
probe head in two lists its slot a second time in another tile (the judge's lse rises by ln 2, out stays) -- or the mla kind's OFFSET on
the 64 rotary columns.  The draw names the probe token; the positions are resolved by the reference side (sparse_problem), which reads the
plan hook -- host logic, no GPU.  Checks: test_gpu_mla_sparse.check on the C entry's result inside the Arena (0xFF pre-fill, guards,
inputs unchanged, NaN bits in every cache row no valid entry names): fwd_tol, LSE_ATOL (hard draws: the bound above, from
sparse_lse_f32_gap), exact zeros / -inf.  Relations: the Python entry and a second run give the C entry's bits; a forced key-range count
(aule_hip_debug_mla_sparse_launch_nsplit) stays within the bounds and the planned count, forced, gives the entry's bits; about one draw in
eight lists the contiguous slots of a block table (at most 191 keys: both plans say one split) and equals flash_attention_mla_paged bit for
bit.

indexer: heads 1 .. 64, block sizes 1 .. 128, a decode or ragged batch (n_b 1 .. 70, contexts around 1 / 63 / 64 / 65 / 129 / 1100, L_b = 0,
n_b > L_b, rows of no sequence, a max_seqlen_q cut, table columns beyond the used blocks), a 16-bit cache or FP8 codes with unit or per-row
scales, a padded q and logits stride, four kinds of weights (randn / sqrt(H), one head carries all, all negative, one zero head).  Logits:
check_logits unchanged (every element within the derived bound, -inf past p, 0xFF elsewhere); the Python entry and a second run the same
bits; unit scales the 16-bit call on the converted codes.  Top-k: topk_contract exactly (check_topk: the C entry twice and the Python
entry), at the drawn topk and output, on four sources of logits: the kernel's own, the hand file's row kinds, `ladder` (a base value plus
0 .. 255 units in the last place, shuffled, with repeats: only the last radix pass separates them) and `bits` (random 32-bit patterns of
both signs with denormals, +-inf and NaN planted).  Selection against fp64: every selected key's fp64 logit is at least the k-th largest
fp64 logit minus the row's two largest per-element bounds.  One draw in four feeds the slot lists to flash_attention_mla_sparse over a
latent cache that shares the table and the block size, judged by the sparse judge on those lists, and compares aule.mla_indexer.

fp8mma: _draw_ragged's axes on the entry's domain (FP8 cache, D 64 / 128), from a stream of its own, plus one row of q rewritten: all
zero (the judge's lse is ln(visible keys)), one element 100 x the rest, or an fp16 row near 6e4.  One draw in three is hard: _draw_ragged's
spike (one key = 20 x a query row that sees it) or offset, planted in the dequantised keys, which are then quantised again with the head's
k_scale -- the judge reads what survives.  Bounds are the hand file's: lse within LSE_ATOL of the q-rounded judge (hard draws: max(LSE_ATOL,
4 x lse_f32_gap) of the q-rounded rows), out within atol + 2 E_P of it, the rms rule, exact zeros / -inf, unowned rows of the 0xFF-filled
out / lse untouched.  Two terms grow a bound, both from the reference alone, each held by tests/test_fuzz_serving_draws.py to the wider
term in at most a quarter of the slice.  The LSE bound of a row gains 2 E_acc, E_acc = D 2^-20 |scale| x the row's largest single product
|q_d k_jd| (fp8mma_acc_term): the FP8 matrix instruction adds the products of a step aligned to the largest and keeps about 20 bits below
its leading bit, so the kernel's scores -- and its lse, which the entry's docstring calls exact -- are off by up to 2^-12.4 of the
largest product at D = 128.  The first slice found it on the `big` and `near6e4` rows (1.4 .. 3.0e-3 and 0.9 .. 2.1 against LSE_ATOL); rows
that see ONE key, whose lse is the scaled dot product itself, showed where it comes from: nothing when a single product is non-zero,
2^-12.4 of the largest product otherwise, 500 times fp32's own spacing (profiles/fuzz_new_serving_kinds.txt).  On plain rows 2 E_acc is
below 4e-4.  And the out bound gains rtol |judge| with fwd_tol's rtol, the rounding of out to storage.  A row that sees one
key has E_P = 0 and returns that value row exactly (the hand file's test 2), which is up to half a unit in the last place from the fp64
value -- 2^-8.9 of 15.1 in bf16 where atol allows 2^-9 max|V| (draws #12 and #14 of the first slice, seed 12, found it); from the reference alone, and
tests/test_fuzz_serving_draws.py holds it to the wider term in at most a quarter of the slice.  Relations: the Python entry, a second run and sequence 0 alone give the same bits; flash_attention_paged_prefill on
the same cache agrees with the same q-rounded judge within fwd_tol plus the largest distance between the q-rounded and the unrounded judge
(out and lse each), which ties the twin's masks and clamps to this kernel's."""
import ast, contextlib, importlib, io, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "aule-attention_amd"), ROOT):
    if _p not in sys.path: sys.path.insert(0, _p)
import numpy as np

JUDGE_BUDGET = 1.0     # scales every kind's cost cap (1.0 ~ 0.2 s of fp64 work per draw on one core)


def _pick(rng, xs):
    return xs[int(rng.randint(len(xs)))]


def _smaller(xs, x):
    """the next smaller member of the sorted list xs (x itself when it is the smallest)"""
    lower = [y for y in xs if y < x]
    return lower[-1] if lower else x


# --------------------------------------------------------------------------------------------------------------- prefill / cascade: the draw
NS_RAGGED = [0, 1, 2, 3, 31, 32, 33, 43, 64, 65, 127, 128, 129, 200]
AHEAD = [1, 63, 64, 65, 300]
BLOCK_SIZES = [1, 2, 7, 16, 24, 32, 64, 100, 128, 256]
PREFIXES = [0, 1, 63, 64, 65, 129, 500]
PREFIX_ROOM = 2048     # keys the roomy prefix table addresses


def _ragged_cost(c, P=0):
    """~ flops of the per-row decode oracle: per token a gather of (P + L) keys and values, per head a dot product and a weighted sum,
    and some 2000 flops' worth of interpreter per (token, head)"""
    return sum(n * (c["Hq"] * 2000 + (c["Hq"] + 2 * c["Hkv"]) * (P + max(L, 0)) * c["D"]) for n, L in zip(c["ns"], c["Ls"]))


def _draw_ragged(rng, cascade):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    hard = int(rng.randint(4)) == 0
    c["kind"] = "16" if hard else _pick(rng, ["16", "fp8"])      # (hard data is for 16-bit caches: such a draw has one)
    c["D"] = _pick(rng, [32, 64, 128])
    c["Hkv"] = _pick(rng, [1, 2, 3, 8])
    g = _pick(rng, [x for x in (1, 2, 3, 4, 5, 8, 16) if x * c["Hkv"] <= 32])
    c["bs"] = _pick(rng, BLOCK_SIZES)
    B = int(rng.randint(1, 7))
    shape = int(rng.randint(8))       # one batch in eight is uniform, one in eight all decode: the siblings' problems
    if shape == 0:
        ns = [_pick(rng, [1, 2, 3, 31, 32, 33, 43, 64])] * B
    elif shape == 1:
        ns = [1] * B
    else:
        ns = [_pick(rng, NS_RAGGED) for _ in range(B)]
    if sum(ns) == 0:
        ns[0] = 1
    ds = []      # L_b - n_b, or None for L_b = 0
    for n in ns:
        how = int(rng.randint(4))
        ds.append(None if how == 0 or (how == 1 and n == 0) else -int(rng.randint(1, n + 1)) if how == 1 else 0 if how == 2 else _pick(rng, AHEAD))
    c["window"] = -1 if cascade else _pick(rng, [-1, -1, 1, 16, 64, 65, 300])
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])          # scale = scale_mul / sqrt(D)
    c["lead"], c["tail"] = _pick(rng, [0, 3]), _pick(rng, [0, 5])
    c["q_pad"] = _pick(rng, [8, 24, 64]) if int(rng.randint(3)) == 0 else 0     # q a slice of a projection that much wider per token
    c["extra_cols"] = _pick(rng, [0, 2])
    room = _pick(rng, [1, 64, 700]) if int(rng.randint(4)) == 0 else 0           # the table addresses that many keys more than any L_b
    if cascade:
        c["P"] = _pick(rng, PREFIXES)
        c["prefix_room"] = int(rng.randint(2)) == 1                              # the prefix table: ceil(P / bs) blocks, or PREFIX_ROOM keys
    # the judge's budget: batch, then heads, then lengths
    P = c.get("P", 0)
    lens = lambda: [0 if d is None else max(n + d, 0) for n, d in zip(ns, ds)]   # noqa: E731
    while True:
        c["Hq"], c["ns"], c["Ls"] = c["Hkv"] * g, list(ns), lens()
        if _ragged_cost(c, P) <= 4e7 * JUDGE_BUDGET:
            break
        if len(ns) > 1:
            ns.pop(); ds.pop()
            if sum(ns) == 0: ns[0] = 1
        elif g > 1: g = _smaller([1, 2, 3, 4, 5, 8, 16], g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller([1, 2, 3, 8], c["Hkv"])
        elif ds[0] is not None and ds[0] > 1: ds[0] = _smaller(AHEAD, ds[0])
        elif ns[0] > 1:
            ns[0] = _smaller(NS_RAGGED, ns[0])
            if ds[0] is not None and ds[0] < 0: ds[0] = max(ds[0], -ns[0])
        elif cascade and c["P"] > 0: c["P"] = P = _smaller(PREFIXES, c["P"])
        else: break
    c["table_len"] = max(c["Ls"]) + room if room else None
    # hard data, drawn against the final shapes
    c["hard"] = None
    if hard:
        live = [(b, i) for b, (n, L) in enumerate(zip(c["ns"], c["Ls"])) for i in range(n) if L - n + i >= 0]
        if int(rng.randint(2)) == 0 and live:
            b, i = _pick(rng, live)
            p = c["Ls"][b] - c["ns"][b] + i                                      # the token's position: it sees the keys lo .. p
            lo = max(0, p - c["window"] + 1) if c["window"] > 0 else 0
            in_prefix = cascade and c["P"] > 0 and int(rng.randint(2)) == 0
            j = int(rng.randint(c["P"])) if in_prefix else int(rng.randint(lo, p + 1))
            c["hard"] = ("spike", 20.0, b, i, int(rng.randint(c["Hq"])), "prefix" if in_prefix else "own", j)
        else:
            c["hard"] = ("offset", float(_pick(rng, [2, 4])), int(rng.randint(c["Hkv"])))
    return c


def draw_prefill(rng):
    return _draw_ragged(rng, False)


def draw_cascade(rng):
    return _draw_ragged(rng, True)


def ragged_geometry(c):
    """what the descriptors of a ragged draw hold beyond the cfg itself: total tokens, table columns, prefix-table blocks (pure)"""
    bs = c["bs"]
    table_lens = c["Ls"] if c["table_len"] is None else [c["table_len"]] * len(c["Ls"])
    cols = max(max((n + bs - 1) // bs for n in table_lens), 1) + c["extra_cols"]
    geo = dict(T=c["lead"] + sum(c["ns"]) + c["tail"], B=len(c["ns"]), max_blocks=cols, max_sq=max(max(c["ns"]), 1), table_lens=table_lens)
    if "P" in c:
        geo["prefix_blocks"] = (PREFIX_ROOM + bs - 1) // bs if c["prefix_room"] else max((c["P"] + bs - 1) // bs, 1)
    return geo


# ----------------------------------------------------------------------------------------------------------------------------- mla: the draw
MLA_LS = [0, 1, "n-1", 33, 63, 64, 65, 200, 700, 1500]
MLA_LENS = [0, 1, 2, 3, 7, 33, 63, 64, 65, 200, 700, 1500]
MLA_HEADS = [1, 5, 16, 24, 64, 128]
MLA_ROOM = 2048


def _mla_cost(c):
    toks = c["ns"] if c["ns"] is not None else [1] * len(c["Ls"])
    return sum(n * (c["Hq"] * (2000 + 2 * L * 576) + 2 * L * 576) for n, L in zip(toks, c["Ls"]))


def draw_mla(rng):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    hard = int(rng.randint(4)) == 0
    c["cache"] = "16" if hard else _pick(rng, ["16", "fp8"])
    c["kv_scale"] = (None if int(rng.randint(2)) == 0 else round(float(rng.uniform(0.25, 2.0)), 3)) if c["cache"] == "fp8" else None
    c["Hq"] = _pick(rng, MLA_HEADS)
    c["bs"] = _pick(rng, [1, 16, 24, 64, 100])
    B = int(rng.randint(1, 6))
    ragged = int(rng.randint(2)) == 1
    ns = [_pick(rng, [0, 1, 2, 3, 4, 8]) for _ in range(B)] if ragged else None
    if ragged and sum(ns) == 0:
        ns[0] = 1
    Ls = []
    for b in range(B):
        L = _pick(rng, MLA_LS)
        Ls.append(max((ns[b] if ragged else 1) - 1, 0) if L == "n-1" else L)
    c["roomy"] = int(rng.randint(2)) == 1                        # the table addresses MLA_ROOM keys per sequence instead of L_b
    c["scale"] = _pick(rng, [None, 192 ** -0.5])
    c["lead"], c["tail"] = (_pick(rng, [0, 2]), _pick(rng, [0, 3])) if ragged else (0, 0)
    c["q_pad"] = _pick(rng, [0, 8])
    c["extra_cols"] = _pick(rng, [0, 2])
    while True:
        c["ns"], c["Ls"] = (list(ns) if ragged else None), list(Ls)
        if _mla_cost(c) <= 1.2e8 * JUDGE_BUDGET:
            break
        if len(Ls) > 1:
            Ls.pop()
            if ragged:
                ns.pop()
                if sum(ns) == 0: ns[0] = 1
        elif c["Hq"] > 1: c["Hq"] = _smaller(MLA_HEADS, c["Hq"])
        elif Ls[0] > 1: Ls[0] = _smaller(MLA_LENS, Ls[0])
        else: break
    c["hard"] = None
    if hard:
        toks = c["ns"] if ragged else [1] * len(c["Ls"])
        live = [(b, i) for b, (n, L) in enumerate(zip(toks, c["Ls"])) for i in range(n) if L - n + i >= 0]
        if int(rng.randint(2)) == 0 and live:
            b, i = _pick(rng, live)
            c["hard"] = ("spike", 8.0, b, i, int(rng.randint(c["Hq"])), "own", int(rng.randint(c["Ls"][b] - toks[b] + i + 1)))
        else:
            c["hard"] = ("offset", float(_pick(rng, [2, 4])))
    return c


def mla_geometry(c):
    bs = c["bs"]
    toks = c["ns"] if c["ns"] is not None else [1] * len(c["Ls"])
    table_lens = [MLA_ROOM] * len(c["Ls"]) if c["roomy"] else c["Ls"]
    cols = max(max((n + bs - 1) // bs for n in table_lens), 1) + c["extra_cols"]
    return dict(T=c["lead"] + sum(toks) + c["tail"], B=len(c["Ls"]), max_blocks=cols, max_sq=max(toks), table_lens=table_lens)


# -------------------------------------------------------------------------------------------------------------------------- varlen: the draw
VARLEN_NS = [0, 1, 2, 31, 32, 33, 64, 100, 128, 129, 200, 257]
VARLEN_LS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 257, 400]


def _varlen_cost(c):
    """~ flops of np_fwd_f64 + np_bwd_f64: seven products of Hq n L D each per sequence"""
    cut = lambda x, m: x if m is None else min(x, m)   # noqa: E731
    return sum(7 * c["Hq"] * (cut(n, c["max_sq"]) * cut(L, c["max_sk"]) * c["D"] + 3000) for n, L in zip(c["ns"], c["ls"]))


def draw_varlen(rng):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    c["wrapper"] = int(rng.randint(5)) == 0                      # through aule.flash_attention_varlen at a head dim that is padded
    c["D"] = _pick(rng, [40, 96]) if c["wrapper"] else _pick(rng, [32, 64, 128])
    c["Hkv"] = _pick(rng, [1, 2, 3, 4])
    g = _pick(rng, [1, 2, 3, 4, 8])
    B = int(rng.randint(1, 7))
    ns, ls = [_pick(rng, VARLEN_NS) for _ in range(B)], [_pick(rng, VARLEN_LS) for _ in range(B)]
    c["mask"] = _pick(rng, ["none", "top", "br"])
    c["window"] = _pick(rng, [-1, -1, 1, 17, 64, 100, 200])
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])
    c["lead"], c["tail"] = (_pick(rng, [0, 3]), _pick(rng, [0, 2])), (_pick(rng, [0, 5]), _pick(rng, [0, 7]))
    c["strided"] = int(rng.randint(3)) == 0 and not c["wrapper"]
    cut = _pick(rng, ["q", "k"]) if int(rng.randint(5)) == 0 else None
    cut_to = _pick(rng, [1, 40, 100])
    c["max_sq"] = c["max_sk"] = None
    while True:
        if sum(ns) == 0: ns[0] = 1
        if sum(ls) == 0: ls[0] = 1
        c["Hq"], c["ns"], c["ls"] = c["Hkv"] * g, list(ns), list(ls)
        if _varlen_cost(c) <= 2.5e8 * JUDGE_BUDGET:
            break
        big = max(range(len(ns)), key=lambda b: ns[b] * ls[b])
        if len(ns) > 1: ns.pop(); ls.pop()
        elif g > 1: g = _smaller([1, 2, 3, 4, 8], g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller([1, 2, 3, 4], c["Hkv"])
        elif ls[big] >= ns[big] and ls[big] > 1: ls[big] = _smaller(VARLEN_LS, ls[big])
        elif ns[big] > 1: ns[big] = _smaller(VARLEN_NS, ns[big])
        else: break
    if cut == "q" and max(c["ns"]) > 1: c["max_sq"] = min(cut_to, max(c["ns"]) - 1)      # below the longest sequence: that one is cut
    if cut == "k" and max(c["ls"]) > 1: c["max_sk"] = min(cut_to, max(c["ls"]) - 1)
    return c


# --------------------------------------------------------------------------------------------------------------------------- sinks: the draw
GROUPS = [1, 2, 3, 4, 5, 8, 16]
SINK_SQ = [1, 2, 5, 13, 33, 64]
SINK_CTX = [0, 1, "Sq-1", 45, 257, 1000, 2048]
SINK_CTX_LENS = [0, 1, 4, 12, 32, 45, 63, 257, 1000, 2048]
MASK_CODE = {"none": 0, "top": 1, "br": 2}


def keys_per_row(n, L, code, window):
    """how many keys each of the n rows of a sequence with L keys sees under the rule of csrc/fa_fwd_varlen_gfx950.hip (pure)"""
    res = []
    for i in range(n):
        pos = i + (L - n if code == 2 else 0)
        hi = min(pos, L - 1) if code else L - 1
        lo = max(0, pos - window + 1) if window > 0 else 0
        res.append(max(0, hi - lo + 1))
    return res


def sinks_sequences(c):
    """[(n, L)] as the entry sees them (after the max_seqlen_q cut), and the mask code of the draw (pure)"""
    if c["entry"] == "query":
        return [(c["Sq"], L) for L in c["Ls"]], 2
    cut = c["max_sq"] if c["max_sq"] is not None else max(max(c["ns"]), 1)
    return [(min(n, cut), L) for n, L in zip(c["ns"], c["Ls"])], MASK_CODE[c["mask"]]


def sinks_row_keys(c):
    """the key counts of all owned rows of the draw (pure)"""
    seqs, code = sinks_sequences(c)
    return [k for n, L in seqs for k in keys_per_row(n, L, code, c["window"])]


def _sinks_cost(c):
    """~ flops of the torch fp64 reference: per sequence two products of Hq n L D and a softmax over Hq n L, the forward twice (with the
    sinks and with none) and for the varlen entry the autograd backward on top"""
    seqs, _ = sinks_sequences(c)
    passes = 5 if c["entry"] == "varlen" else 2
    return passes * sum(c["Hq"] * (n * L * (4 * c["D"] + 40) + 3000) for n, L in seqs)


def draw_sinks(rng):
    c = {}
    c["entry"] = _pick(rng, ["varlen", "prefill", "query"])
    varlen = c["entry"] == "varlen"
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    c["wrapper"] = int(rng.randint(5)) == 0 and varlen           # through aule.flash_attention_varlen_sinks at a head dim that is padded
    c["D"] = _pick(rng, [40, 96]) if c["wrapper"] else _pick(rng, [32, 64, 128])
    c["Hkv"] = _pick(rng, [1, 2, 3, 8])
    g = _pick(rng, [x for x in GROUPS if x * c["Hkv"] <= 32])
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])
    c["window"] = _pick(rng, [-1, -1, 1, 17, 64, 128, 300])
    cache, bs, cols = _pick(rng, ["16", "fp8"]), _pick(rng, BLOCK_SIZES), _pick(rng, [1, 3])
    c["cache"], c["bs"], c["extra_cols"] = (None, None, None) if varlen else (cache, bs, cols)
    mask = _pick(rng, ["none", "top", "br"])
    c["mask"] = mask if varlen else "br"
    lead, tail, q_pad = _pick(rng, [0, 3]), _pick(rng, [0, 5]), _pick(rng, [8, 24, 64]) if int(rng.randint(3)) == 0 else 0
    c["lead"], c["tail"] = (0, 0) if c["entry"] == "query" else (lead, tail)
    c["q_pad"] = q_pad if c["entry"] == "prefill" else 0
    c["sinks_in_q_dtype"] = int(rng.randint(6)) == 0             # sinks passed in q's dtype: the judge sees the rounded values
    rot = int(rng.randint(5))
    cut = int(rng.randint(5)) == 0 and varlen
    cut_to = _pick(rng, [1, 40, 100])
    c["Sq"] = c["max_sq"] = None
    B = int(rng.randint(1, 7))
    if varlen:
        ns, Ls = [_pick(rng, VARLEN_NS) for _ in range(B)], [_pick(rng, VARLEN_LS) for _ in range(B)]
    elif c["entry"] == "prefill":
        shape = int(rng.randint(8))       # one batch in eight is uniform, as _draw_ragged's: the paged query's problem
        ns = [_pick(rng, [1, 2, 3, 31, 32, 33, 43, 64])] * B if shape == 0 else [_pick(rng, NS_RAGGED) for _ in range(B)]
        Ls = []
        for n in ns:
            how = int(rng.randint(4))
            Ls.append(0 if how == 0 or (how == 1 and n == 0) else n - int(rng.randint(1, n + 1)) if how == 1 else n if how == 2 else n + _pick(rng, AHEAD))
    else:
        c["Sq"] = _pick(rng, SINK_SQ)
        ns = [c["Sq"]] * B
        Ls = [max(c["Sq"] - 1, 0) if L == "Sq-1" else L for L in (_pick(rng, SINK_CTX) for _ in range(B))]
    while True:      # the judge's budget: batch, then heads, then lengths; and some row sees a key
        if not any(n >= 1 and L >= 1 for n, L in zip(ns, Ls)):
            ns[0], Ls[0] = max(ns[0], 1), max(Ls[0], 1)
        c["Hq"], c["ns"], c["Ls"] = c["Hkv"] * g, list(ns), list(Ls)
        if _sinks_cost(c) <= 6e8 * JUDGE_BUDGET:
            break
        big = max(range(len(ns)), key=lambda b: ns[b] * Ls[b])
        if len(ns) > 1: ns.pop(); Ls.pop()
        elif g > 1: g = _smaller(GROUPS, g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller([1, 2, 3, 8], c["Hkv"])
        elif Ls[big] > 1: Ls[big] = _smaller(sorted(set(VARLEN_LS + SINK_CTX_LENS)), Ls[big])
        else: break
    if cut and max(c["ns"]) > 1: c["max_sq"] = min(cut_to, max(c["ns"]) - 1)             # below the longest sequence: that one is cut
    # head h takes entry (h + rot) % 5 of the cycle; with fewer than five heads some head must take entry 3, ln(Lmax) + 0.5
    c["rot"] = rot if c["Hq"] >= 5 else (3 - rot % c["Hq"]) % 5
    return c


def sinks_half_head(c):
    """the first head whose sink logit is ln(Lmax) + 0.5 (pure)"""
    return next(h for h in range(c["Hq"]) if (h + c["rot"]) % 5 == 3)


# ---------------------------------------------------------------------------------------------------------------------------- tree: the draw
TREE_BS = [1, 7, 16, 24, 32, 64, 100, 128]
TREE_SQ = [1, 2, 5, 13, 31, 32, 33, 63, 64]
TREE_CTX = ["Sq//2", "Sq", "Sq+1", 45, 100, 257, 1000]
TREE_NS = [0, 1, 7, 20, 33, 63, 64, 65, 100]
TREE_AHEAD = [0, 1, 49, 64, 77, 200]
WORD_KINDS = ["tree", "random", "emptied", "ones", "chain"]


def _tree_cost(c):
    """~ flops of the fp64 judge: two products of Hq n L D per sequence and a softmax"""
    return sum(c["Hq"] * (n * L * (4 * c["D"] + 40) + 3000) for n, L in zip(c["ns"], c["Ls"]))


def draw_tree(rng):
    c = {}
    c["entry"] = _pick(rng, ["query", "prefill"])
    query = c["entry"] == "query"
    c["dtype"], c["cache"] = _pick(rng, ["bf16", "fp16"]), _pick(rng, ["16", "fp8"])
    c["D"] = _pick(rng, [32, 64, 128])
    c["Hkv"] = _pick(rng, [1, 2, 3, 8])
    g = _pick(rng, [x for x in GROUPS if x * c["Hkv"] <= 32])
    c["bs"] = _pick(rng, TREE_BS)
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])
    c["extra_cols"] = _pick(rng, [0, 2])
    lead, tail, q_pad = _pick(rng, [0, 3]), _pick(rng, [0, 5]), _pick(rng, [8, 24, 64]) if int(rng.randint(3)) == 0 else 0
    c["lead"], c["tail"], c["q_pad"] = (0, 0, 0) if query else (lead, tail, q_pad)
    c["Sq"] = _pick(rng, TREE_SQ) if query else None
    B = int(rng.randint(1, 7))
    sym = lambda L: {"Sq//2": c["Sq"] // 2, "Sq": c["Sq"], "Sq+1": c["Sq"] + 1}.get(L, L)   # noqa: E731
    if query:
        ns = [c["Sq"]] * B
        Ls = [sym(_pick(rng, TREE_CTX)) for _ in range(B)]
    else:
        ns = [_pick(rng, TREE_NS) for _ in range(B)]
        Ls = []
        for n in ns:
            how = int(rng.randint(7))
            Ls.append(n - int(rng.randint(1, n + 1)) if how == 0 and n > 0 else n + TREE_AHEAD[max(how - 1, 0)])
    kinds = [_pick(rng, WORD_KINDS) for _ in range(B)]           # the words of a sequence: by kind, from the data seed
    # One more sequence behind the drawn ones, the draw's probe: words with emptied rows in front of at most one key of context, so that its
    # rows see few keys and the judge under the words is far from the judge under the chain whatever the drawn sequences hold.  The
    # budget below shrinks the drawn sequences only.
    if query:
        probe = (c["Sq"], sym(_pick(rng, TREE_CTX[:3])))
    else:
        n = _pick(rng, [7, 20, 33, 63, 64])
        probe = (n, n - int(rng.randint(1, n + 1)) if int(rng.randint(3)) == 0 else n + int(rng.randint(2)))
    while True:
        c["Hq"], c["ns"], c["Ls"], c["words"] = c["Hkv"] * g, ns + [probe[0]], Ls + [probe[1]], kinds + ["emptied"]
        if _tree_cost(c) <= 3e8 * JUDGE_BUDGET:
            break
        if len(ns) > 1: ns.pop(); Ls.pop(); kinds.pop()
        elif g > 1: g = _smaller(GROUPS, g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller([1, 2, 3, 8], c["Hkv"])
        elif Ls[0] - ns[0] > 1: Ls[0] = ns[0] + _smaller(TREE_AHEAD, Ls[0] - ns[0])
        else: break
    return c


def tree_geometry(c):
    """what the descriptors of a tree draw hold beyond the cfg (pure)"""
    cols = max(max((L + c["bs"] - 1) // c["bs"] for L in c["Ls"]), 1) + c["extra_cols"]
    return dict(T=c["lead"] + sum(c["ns"]) + c["tail"], B=len(c["ns"]), max_blocks=cols)


# --------------------------------------------------------------------------------------------------------------------------- mlapf: the draw
MLAPF_HEADS = [1, 2, 3, 5, 8, 16, 17, 32]
MLAPF_NS = [0, 1, 2, 31, 32, 33, 64, 127, 128, 129, 200, 257]
MLAPF_LS = VARLEN_LS


def _mlapf_sequences(c):
    cut = lambda x, m: x if m is None else min(x, m)   # noqa: E731
    return [(cut(n, c["max_sq"]), cut(L, c["max_sk"])) for n, L in zip(c["ns"], c["ls"])]


def _mlapf_cost(c):
    """~ flops of np_fwd_f64 + np_bwd_f64: seven products of H n L 192 each per sequence"""
    return sum(7 * c["H"] * (n * L * 192 + 3000) for n, L in _mlapf_sequences(c))


def draw_mlapf(rng):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    c["wrapper"] = int(rng.randint(5)) == 0                      # aule.flash_attention_mla_varlen with autograd on slices of the projections
    c["H"] = _pick(rng, MLAPF_HEADS)
    B = int(rng.randint(1, 7))
    ns, ls = [_pick(rng, MLAPF_NS) for _ in range(B)], [_pick(rng, MLAPF_LS) for _ in range(B)]
    c["mask"] = _pick(rng, ["none", "top", "br"])
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])          # scale = scale_mul / sqrt(192)
    c["lead"], c["tail"] = (_pick(rng, [0, 3]), _pick(rng, [0, 2])), (_pick(rng, [0, 5]), _pick(rng, [0, 7]))
    layout = _pick(rng, ["contiguous", "in_place", "wide"])
    c["layout"] = None if c["wrapper"] else layout
    cut = _pick(rng, ["q", "k"]) if int(rng.randint(5)) == 0 else None
    cut_to = _pick(rng, [1, 40, 100])
    c["max_sq"] = c["max_sk"] = None
    while True:
        if sum(ns) == 0: ns[0] = 1
        if sum(ls) == 0: ls[0] = 1
        c["ns"], c["ls"] = list(ns), list(ls)
        if _mlapf_cost(c) <= 2.5e8 * JUDGE_BUDGET:
            break
        big = max(range(len(ns)), key=lambda b: ns[b] * ls[b])
        if len(ns) > 1: ns.pop(); ls.pop()
        elif c["H"] > 1: c["H"] = _smaller(MLAPF_HEADS, c["H"])
        elif ls[big] >= ns[big] and ls[big] > 1: ls[big] = _smaller(MLAPF_LS, ls[big])
        elif ns[big] > 1: ns[big] = _smaller(MLAPF_NS, ns[big])
        else: break
    if cut == "q" and max(c["ns"]) > 1: c["max_sq"] = min(cut_to, max(c["ns"]) - 1)      # below the longest sequence: that one is cut
    if cut == "k" and max(c["ls"]) > 1: c["max_sk"] = min(cut_to, max(c["ls"]) - 1)
    return c


def mlapf_geometry(c):
    """the totals and maxima the descriptor of a draw holds (pure)"""
    return dict(B=len(c["ns"]), Tq=c["lead"][0] + sum(c["ns"]) + c["tail"][0], Tk=c["lead"][1] + sum(c["ls"]) + c["tail"][1],
                max_sq=c["max_sq"] if c["max_sq"] is not None else max(1, max(c["ns"])),
                max_sk=c["max_sk"] if c["max_sk"] is not None else max(1, max(c["ls"])))


# -------------------------------------------------------------------------------------------------------------------------- sparse: the draw
SPARSE_HEADS = [1, 2, 8, 16, 17, 63, 64, 65, 96, 127, 128]
SPARSE_TOPKS = [1, 2, 63, 64, 65, 127, 129, 200, 500, 2048]
# (block_size, num_blocks): caches so small that every longer list repeats slots, caches of a few hundred slots, one of 4096
SPARSE_CACHES = [(1, 5), (16, 2), (7, 3), (1, 300), (16, 19), (48, 7), (24, 11), (64, 64)]
SPARSE_INVALID = ["none", "none", "scattered", "scattered", "tile", "split", "all"]      # a token's share of invalid entries
SPARSE_DENSE_LS = {1: [191, 1, 64, 100], 16: [176, 1, 64, 100]}      # the contiguous-list draw: block size -> context lengths (the first: the capacity)


def _sparse_cost(c):
    """~ flops of the per-token judge: scores over 576 columns and P @ rows over 512 per (head, entry), the gather of the rows, and some
    2e5 flops' worth of interpreter per token"""
    return c["T"] * (c["Hq"] * c["topk"] * 2200 + c["topk"] * 576 * 4 + 200000)


def draw_sparse(rng):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    hard = int(rng.randint(3)) == 0
    dense = not hard and int(rng.randint(5)) == 0                 # (two draws in fifteen: the contiguous lists of a block table)
    c["cache"] = "16" if hard or dense else _pick(rng, ["16", "fp8"])
    T, Hq, topk = int(rng.randint(1, 7)), _pick(rng, SPARSE_HEADS), _pick(rng, SPARSE_TOPKS)
    c["bs"], c["nb"] = _pick(rng, SPARSE_CACHES)
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5, -1.0])    # scale = scale_mul / sqrt(576)
    c["q_pad"] = _pick(rng, [0, 0, 8, 24])                       # q a slice of a projection that many heads wider per token
    invalid = [_pick(rng, SPARSE_INVALID) for _ in range(6)]
    repeat = [int(rng.randint(3)) == 0 for _ in range(6)]
    c["force_nsplit"] = _pick(rng, [None, None, 1, 2, 3, 7])
    c["ws"] = _pick(rng, ["caller", "own"])                       # the caller's workspace at exactly the queried size, or the library's
    kind, probe, add, dense_bs = int(rng.randint(2)), int(rng.randint(6)), float(_pick(rng, [2, 4])), _pick(rng, [1, 16])
    dense_ls = [int(rng.randint(1, 4)) for _ in range(6)]
    c["dense"] = None
    if dense:
        # tests/test_gpu_mla_sparse.py::test_contiguous_lists_equal_the_paged_decode_bit_for_bit: token t lists the slots of positions
        # 0 .. L_t - 1 of sequence t, padded with -1 to a multiple of 64; at most 191 keys of table, so that both plans say one split
        ls = SPARSE_DENSE_LS[dense_bs]
        c["bs"], topk = dense_bs, 192
        c["force_nsplit"], invalid, repeat = None, ["none"] * 6, [False] * 6
    while True:      # the judge's budget: tokens, then heads, then the list
        c["T"], c["Hq"], c["topk"] = T, Hq, topk
        if _sparse_cost(c) <= 1e9 * JUDGE_BUDGET:
            break
        if T > 1: T -= 1
        elif Hq > 1: Hq = _smaller(SPARSE_HEADS, Hq)
        elif topk > 1: topk = _smaller(SPARSE_TOPKS, topk)
        else: break
    if dense:
        c["dense"] = [ls[0]] + [ls[i] for i in dense_ls[1:c["T"]]]
        c["nb"] = c["T"] * (ls[0] // c["bs"]) + 3
    c["invalid"], c["repeat"] = invalid[:c["T"]], repeat[:c["T"]]
    # hard data, against the final shapes: ("seam", the probe token) -- the positions come from the split plan, which the reference side
    # reads (sparse_problem) -- or ("offset", c)
    c["hard"] = None
    if hard:
        if kind == 0:
            t = probe % c["T"]
            c["hard"] = ("seam", t)
            if c["invalid"][t] in ("split", "all") or (c["invalid"][t] == "tile" and c["topk"] <= 64):
                c["invalid"][t] = "scattered"                     # (the probe token keeps valid entries at the seams)
        else:
            c["hard"] = ("offset", add)
    return c


# -------------------------------------------------------------------------------------------------------------------------- fp8mma: the draw
FP8MMA_QROWS = ["plain", "zero", "big", "near6e4"]      # one (token, head) row of q: as drawn, all zero, one element x 100, fp16 near 6e4


def _fp8mma_cost(c):
    """~ flops of tests/test_gpu_paged_prefill_fp8mma.py::_models: per sequence three einsum products of n L Hq D, the exponentials and the
    e4m3 rounding of n L Hq weights"""
    return sum(c["Hq"] * (n * max(L, 0) * (6 * c["D"] + 60) + 3000) for n, L in zip(c["ns"], c["Ls"]))


def draw_fp8mma(rng):
    """_draw_ragged's axes on the FP8-product entry's domain (an FP8 cache, D 64 / 128, no sinks), from a stream of its own"""
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    hard = int(rng.randint(3)) == 0
    c["D"] = _pick(rng, [64, 128])
    c["Hkv"] = _pick(rng, [1, 2, 3, 8])
    g = _pick(rng, [x for x in (1, 2, 3, 4, 5, 8, 16) if x * c["Hkv"] <= 32])
    c["bs"] = _pick(rng, BLOCK_SIZES)
    B = int(rng.randint(1, 7))
    shape = int(rng.randint(8))       # one batch in eight is uniform, one in eight all decode
    if shape == 0:
        ns = [_pick(rng, [1, 2, 3, 31, 32, 33, 43, 64])] * B
    elif shape == 1:
        ns = [1] * B
    else:
        ns = [_pick(rng, NS_RAGGED) for _ in range(B)]
    if sum(ns) == 0:
        ns[0] = 1
    ds = []      # L_b - n_b, or None for L_b = 0
    for n in ns:
        how = int(rng.randint(4))
        ds.append(None if how == 0 or (how == 1 and n == 0) else -int(rng.randint(1, n + 1)) if how == 1 else 0 if how == 2 else _pick(rng, AHEAD))
    c["window"] = _pick(rng, [-1, -1, 1, 16, 64, 65, 300])
    c["scale_mul"] = _pick(rng, [None, None, 0.5, 1.5])          # scale = scale_mul / sqrt(D)
    c["lead"], c["tail"] = _pick(rng, [0, 3]), _pick(rng, [0, 5])
    c["q_pad"] = _pick(rng, [8, 24, 64]) if int(rng.randint(3)) == 0 else 0
    c["extra_cols"] = _pick(rng, [0, 2])
    room = _pick(rng, [1, 64, 700]) if int(rng.randint(4)) == 0 else 0
    qrow = _pick(rng, FP8MMA_QROWS)
    lens = lambda: [0 if d is None else max(n + d, 0) for n, d in zip(ns, ds)]   # noqa: E731
    while True:      # the judge's budget: batch, then heads, then lengths
        c["Hq"], c["ns"], c["Ls"] = c["Hkv"] * g, list(ns), lens()
        if _fp8mma_cost(c) <= 1e8 * JUDGE_BUDGET:
            break
        if len(ns) > 1:
            ns.pop(); ds.pop()
            if sum(ns) == 0: ns[0] = 1
        elif g > 1: g = _smaller([1, 2, 3, 4, 5, 8, 16], g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller([1, 2, 3, 8], c["Hkv"])
        elif ds[0] is not None and ds[0] > 1: ds[0] = _smaller(AHEAD, ds[0])
        elif ns[0] > 1:
            ns[0] = _smaller(NS_RAGGED, ns[0])
            if ds[0] is not None and ds[0] < 0: ds[0] = max(ds[0], -ns[0])
        else: break
    c["table_len"] = max(c["Ls"]) + room if room else None
    # the q row and the hard data, against the final shapes: a token that sees a key
    live = [(b, i) for b, (n, L) in enumerate(zip(c["ns"], c["Ls"])) for i in range(n) if L - n + i >= 0]
    c["qrow"], c["hard"] = None, None
    spike = hard and int(rng.randint(2)) == 0 and bool(live)
    if qrow == "near6e4" and c["dtype"] != "fp16":
        qrow = "big"
    if qrow != "plain" and live and not spike:                   # (a spiked key is m x a plain row of q)
        b, i = _pick(rng, live)
        c["qrow"] = (qrow, b, i, int(rng.randint(c["Hq"])))
    if spike:
        b, i = _pick(rng, live)
        p = c["Ls"][b] - c["ns"][b] + i
        lo = max(0, p - c["window"] + 1) if c["window"] > 0 else 0
        c["hard"] = ("spike", 20.0, b, i, int(rng.randint(c["Hq"])), "own", int(rng.randint(lo, p + 1)))
    elif hard:
        c["hard"] = ("offset", float(_pick(rng, [2, 4])), int(rng.randint(c["Hkv"])))
    return c


# ------------------------------------------------------------------------------------------------------------------------- indexer: the draw
INDEXER_BS = [1, 2, 7, 16, 48, 64, 128]
INDEXER_NS = [1, 2, 3, 4, 5, 63, 64, 70]
INDEXER_CTX = [0, 1, 63, 64, 65, 129, 1100, "n-k"]      # "n-k": fewer keys than new tokens (p < 0 for the first rows)
INDEXER_CTX_LENS = [0, 1, 63, 64, 65, 129, 1100]
INDEXER_TOPKS = [1, 63, 64, 65, 200, 2048, "above"]     # "above": three more than the table is wide -- every visible key and the -1 tail
INDEXER_WEIGHTS = ["randn", "one", "negative", "zero"]  # randn / sqrt(H); one head carries all the weight; all negative; one zero head
INDEXER_SOURCES = ["own", "hand", "ladder", "bits"]     # the logits a top-k call is given (indexer_logit_sources)


def _indexer_rows(c):
    """[(n rows after the cut, L)] per sequence (pure)"""
    if c["ns"] is None:
        return [(1, L) for L in c["ctx"]]
    cut = c["max_sq"] if c["max_sq"] is not None else max(c["ns"])
    return [(min(n, cut), L) for n, L in zip(c["ns"], c["ctx"])]


def _indexer_cost(c):
    """~ flops of Problem.judge (two products of H x 128 per visible key of every row), of the exact top-k contract on four logit sources
    (a sort of the row), and of the sparse judge on the selected keys of a pipeline draw"""
    cost = 0
    for n, L in _indexer_rows(c):
        seen = sum(max(L - n + i + 1, 0) for i in range(n))
        cost += seen * (c["H"] * 512 + 400) + n * 20000
        if c["pipeline"] is not None:
            cost += n * c["pipeline"] * min(L, 2051) * 2200
    return cost


def draw_indexer(rng):
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "fp16"])
    c["H"] = int(rng.randint(1, 65))
    c["bs"] = _pick(rng, INDEXER_BS)
    c["fp8"] = _pick(rng, [None, "unit", "rows"])
    c["q_pad"] = _pick(rng, [0, 0, 8, 16])                       # q a slice of a projection that many heads wider per token
    c["pad"] = _pick(rng, [0, 3, 8])                             # logits_stride = the table's width + pad
    c["weights"] = _pick(rng, INDEXER_WEIGHTS)
    c["topk"] = _pick(rng, INDEXER_TOPKS)
    c["positions"] = int(rng.randint(2)) == 1                    # the list holds positions, else cache slots
    pipeline = int(rng.randint(4)) == 0
    lat_heads = _pick(rng, [2, 16])
    ragged = int(rng.randint(3)) > 0
    B = int(rng.randint(1, 6))
    ns = [_pick(rng, INDEXER_NS) for _ in range(B)]
    ctx = [_pick(rng, INDEXER_CTX) for _ in range(B)]
    below = [int(rng.randint(1, 71)) for _ in range(B)]
    extra_rows = _pick(rng, [0, 0, 2, 3])
    c["extra_rows"] = extra_rows if ragged else 0                 # (plain decode: the Python entries take one row per sequence)
    cut = int(rng.randint(5)) == 0
    room = _pick(rng, [0, 0, 1, 5])                              # table columns beyond the longest context: that many blocks
    if pipeline:
        c["positions"] = False
    c["pipeline"] = lat_heads if pipeline else None               # the heads of the latent attention the lists are fed to
    while True:      # the judge's budget: batch, then heads, then lengths
        toks = ns if ragged else [1] * len(ns)
        c["ns"] = list(ns) if ragged else None
        c["ctx"] = [max(n - min(k, n), 0) if L == "n-k" else L for n, L, k in zip(toks, ctx, below)]
        c["max_sq"] = None
        if _indexer_cost(c) <= 3e8 * JUDGE_BUDGET:
            break
        big = max(range(len(ns)), key=lambda b: toks[b] * (c["ctx"][b] + 1))
        if len(ns) > 1: ns.pop(); ctx.pop(); below.pop()
        elif c["H"] > 1: c["H"] = max(1, c["H"] // 2)
        elif ctx[big] != "n-k" and ctx[big] > 1: ctx[big] = _smaller(INDEXER_CTX_LENS, ctx[big])
        elif ns[big] > 1: ns[big] = _smaller(INDEXER_NS, ns[big])
        else: break
    if cut and ragged and max(c["ns"]) > 1:
        c["max_sq"] = max(1, max(c["ns"]) - _pick(rng, [1, 6]))  # below the longest sequence: its last rows belong to no sequence
    c["cap"] = max(max(c["ctx"]), 1) + room * c["bs"] if room else None
    return c


DRAW = dict(indexer=draw_indexer, prefill=draw_prefill, cascade=draw_cascade, mla=draw_mla, varlen=draw_varlen, sinks=draw_sinks, tree=draw_tree, mlapf=draw_mlapf,
            sparse=draw_sparse, fp8mma=draw_fp8mma)
# The fixed-seed slices of the suite: kind -> (draws, seed).  tests/test_gpu_fuzz_serving.py runs them, tests/test_fuzz_serving_draws.py
# asserts (without a GPU) that they reach what they are for; a seed is chosen so that the latter holds.
SLICES = dict(prefill=(30, 2), cascade=(20, 3), mla=(20, 5), varlen=(20, 4), sinks=(20, 24), tree=(20, 2), mlapf=(20, 4),
              sparse=(24, 25), fp8mma=(20, 128), indexer=(20, 1))


def draws(kind, n, seed):
    """the n configurations of `kind` at `seed` (pure: the same list on every call)"""
    rng = np.random.RandomState(seed)
    return [DRAW[kind](rng) for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------------------- the runs
def _mods(*names):
    import oracle
    oracle.build()
    return [oracle] + [importlib.import_module(n) for n in names]


def _checked(errs, fn, *args, **kw):
    """one of the test files' asserting judges: its AssertionError becomes an entry of errs, its printed line is swallowed"""
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return fn(*args, **kw)
    except AssertionError as e:
        errs.append(" ".join(str(e).split())[:300])
        return None


def _same(torch, a, b):
    """the same bits (NaN payloads and the sign of zero included)"""
    a, b = a.contiguous(), b.contiguous()
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.view(view), b.view(view)))


def _close(errs, what, got, want, atol, rtol):
    got, want = got.float().cpu().numpy().astype(np.float64), want.float().cpu().numpy().astype(np.float64)
    if got.size == 0: return
    if not np.isfinite(got).all(): errs.append(what + ": non-finite"); return
    e = np.abs(got - want)
    if (e > atol + rtol * np.abs(want)).any(): errs.append("%s: err %.3e (atol %.3e)" % (what, e.max(), atol))


def _lse_close(errs, torch, what, got, want, bound):
    if not torch.equal(torch.isneginf(got), torch.isneginf(want)): errs.append(what + ": -inf in different rows"); return
    fin = torch.isfinite(want)
    if bool(fin.any()) and float((got[fin] - want[fin]).abs().max()) > bound:
        errs.append("%s: lse err %.3e (bound %.3e)" % (what, float((got[fin] - want[fin]).abs().max()), bound))


def _harden_ragged(p, c, quantize, cas=None):
    """the draw's hard-data treatment, applied to the 16-bit pool in place (what the device sees and what the oracle sees)"""
    h = c["hard"]
    if h is None: return
    g = p.Hq // p.Hkv
    if h[0] == "spike":
        _, m, b, i, head, where, j = h
        blk = int(cas.pbt[j // p.bs]) if where == "prefix" else int(p.bt[b][j // p.bs])
        p.kdev[blk, j % p.bs, head // g] = quantize((m * p.q[int(p.cu[b]) + i, head]).astype(np.float32), p.dtype)
    else:
        _, add, hk = h
        p.kdev[:, :, hk] = quantize((p.kdev[:, :, hk] + add).astype(np.float32), p.dtype)
    p.K = p.kdev.astype(np.float64)
    p._ref = {}


def run_prefill(cfg, seed, stats=None):
    import torch
    import aule
    oracle, tp, tq, util = _mods("test_gpu_paged_prefill", "test_gpu_paged_query", "util")
    c, geo = cfg, ragged_geometry(cfg)
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p = tp.Ragged(seed, c["dtype"], c["kind"], c["Hq"], c["Hkv"], c["D"], c["bs"], c["ns"], c["Ls"], lead=c["lead"], tail=c["tail"],
                  table_lens=None if c["table_len"] is None else geo["table_lens"], extra_cols=c["extra_cols"])
    assert (p.T, p.bt.shape[1], p.max_sq) == (geo["T"], geo["max_blocks"], geo["max_sq"])
    _harden_ragged(p, c, util.quantize)
    W, scale = c["window"], None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"])
    lse_atol = tq.LSE_ATOL
    if c["hard"] is not None:
        stats["lse_f32_gap"] = p.lse_f32_gap(W, scale)
        lse_atol = max(lse_atol, 4.0 * stats["lse_f32_gap"])
    out, lse, intact = tp._run_capi(torch, p, window=W, scale=scale, q_pad=c["q_pad"])
    own = p.owned()
    if not intact: errs.append("wrote in front of or behind out / lse")
    if not tp._untouched(torch, out, lse, own): errs.append("a row of no sequence was written")
    res = _checked(errs, tp._judge, p, out, lse, oracle, W, "prefill", scale=scale, lse_atol=lse_atol)
    if res: stats["out"], stats["lse"] = res
    # the Python entry on the same tensors: the same launch
    o2, l2 = p.run(torch, W, scale=scale, q_pad=c["q_pad"])
    torch.cuda.synchronize()
    town = torch.from_numpy(own).cuda()
    if not (_same(torch, o2[town], out[town]) and _same(torch, l2[town], lse[town])): errs.append("Python entry != C entry")
    B, n, lead = geo["B"], c["ns"][0], c["lead"]
    if all(x == n for x in c["ns"]) and 1 <= n <= 64:
        # tests/test_gpu_paged_prefill.py::test_agrees_with_the_paged_query_on_a_uniform_batch: the same problem by another kernel
        (q, kc, vc, bt, cl, _), scales = p.device(torch)
        q4 = q[lead:lead + B * n].view(B, n, p.Hq, p.D).permute(0, 2, 1, 3).contiguous()
        want, wl = aule.flash_attention_paged_query(q4, kc, vc, bt, cl, scale=scale, window_size=W, return_lse=True, **scales)
        torch.cuda.synchronize()
        atol, rtol = util.fwd_tol(p.dtype, p.vmax)
        _close(errs, "prefill vs paged query", out[lead:lead + B * n], want.permute(0, 2, 1, 3).reshape(B * n, p.Hq, p.D), atol, rtol)
        _lse_close(errs, torch, "prefill vs paged query", lse[lead:lead + B * n], wl.permute(0, 2, 1).reshape(B * n, p.Hq), 2 * lse_atol)
        if n == 1:
            dec = aule.flash_attention_paged_amd(q4.squeeze(2), kc, vc, bt, cl, scale=scale, window_size=W, **scales)
            torch.cuda.synchronize()
            if not _same(torch, want.squeeze(2), dec): errs.append("paged_amd != paged_query(seq_q = 1) bit for bit")
            L = np.clip(p.cl.astype(np.int64), 0, p.bt.shape[1] * p.bs)
            ref = oracle.paged_decode_f64(p.q[lead:lead + B], p.K, p.V, p.bt, L, scale, W)
            _close(errs, "paged_amd vs oracle", dec, torch.from_numpy(ref), atol, rtol)
    return cfg, errs


def run_cascade(cfg, seed, stats=None):
    import torch
    import aule
    oracle, tp, tc, tq, util = _mods("test_gpu_paged_prefill", "test_gpu_paged_cascade", "test_gpu_paged_query", "util")
    c, geo = cfg, ragged_geometry(cfg)
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p = tp.Ragged(seed, c["dtype"], c["kind"], c["Hq"], c["Hkv"], c["D"], c["bs"], c["ns"], c["Ls"], lead=c["lead"], tail=c["tail"],
                  table_lens=None if c["table_len"] is None else geo["table_lens"], extra_cols=c["extra_cols"], pool=geo["prefix_blocks"])
    cas = tc.Cascade(p, seed + 1, blocks=geo["prefix_blocks"])
    assert (p.T, p.bt.shape[1], len(cas.pbt)) == (geo["T"], geo["max_blocks"], geo["prefix_blocks"]) and c["P"] <= cas.cap
    _harden_ragged(p, c, util.quantize, cas)
    P, bs, scale = c["P"], c["bs"], None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"])
    lse_atol = tq.LSE_ATOL
    if c["hard"] is not None:
        stats["lse_f32_gap"] = cas.lse_f32_gap(P, scale)
        lse_atol = max(lse_atol, 4.0 * stats["lse_f32_gap"])
    out, lse = cas.run(torch, P, scale=scale, hostile=False, q_pad=c["q_pad"])
    torch.cuda.synchronize()
    res = _checked(errs, tc._judge, cas, out, lse, oracle, P, "cascade", scale=scale, lse_atol=lse_atol)
    if res: stats["out"], stats["lse"] = res
    (q, kc, vc, bt, cl, cu), scales, pbt, _ = cas.device(torch, P, hostile=False, q_pad=c["q_pad"])
    kw = dict(scale=scale, return_lse=True, **scales)
    own_np = p.owned()
    seen = np.zeros(p.T, dtype=bool)      # the owned rows at own positions >= 0: the rows that see a key at all
    for b, s, n, L in p.sequences():
        seen[s + max(n - L, 0):s + n] = True
    own, live, dead = (torch.from_numpy(m).cuda() for m in (own_np, seen, own_np & ~seen))
    atol2, rtol2 = util.fwd_tol(p.dtype, p.vmax, sides=2)
    # the state over the own keys alone: the plain prefill
    oo, ol = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=p.max_sq, **kw)
    torch.cuda.synchronize()
    if P == 0 and not (_same(torch, out[own], oo[own]) and _same(torch, lse[own], ol[own])): errs.append("P = 0 is not the prefill bit for bit")
    if P > 0 and P % bs == 0:
        # the prefix blocks in front of every sequence's own: the prefill over the concatenated table is the same problem for every row at an
        # own position >= 0 (a row in front of its sequence's keys sees nothing in the cascade, but prefix keys in the concatenation)
        bt2 = torch.cat([pbt[:P // bs].unsqueeze(0).expand(p.B, -1), bt], dim=1).contiguous()
        co, cl_ = aule.flash_attention_paged_prefill(q, kc, vc, bt2, cl + P, cu, max_seqlen_q=p.max_sq, **kw)
        torch.cuda.synchronize()
        _close(errs, "cascade vs prefill over the concatenated table", out[live], co[live], atol2, rtol2)
        _lse_close(errs, torch, "cascade vs prefill over the concatenated table", lse[live], cl_[live], 2 * lse_atol)
    # the state over the prefix alone: every owned token as a sequence of its own with one token at position P - 1, which sees all P keys
    rows = np.flatnonzero(own_np)
    if rows.size:
        idx = torch.from_numpy(rows).cuda()
        N = rows.size
        po, pl = aule.flash_attention_paged_prefill(q[idx].contiguous(), kc, vc, pbt.unsqueeze(0).expand(N, -1).contiguous(),
                                                    torch.full((N,), P, dtype=torch.int32, device="cuda"),
                                                    torch.arange(N + 1, dtype=torch.int32, device="cuda"), max_seqlen_q=1, **kw)
        mo, ml = aule.merge_attention_states(po, pl, oo[idx].contiguous(), ol[idx].contiguous())
        torch.cuda.synchronize()
        lv, dd = live[idx], dead[idx]
        _close(errs, "merge(prefix state, own state) vs cascade", mo[lv], out[idx][lv], atol2, rtol2)
        _lse_close(errs, torch, "merge(prefix state, own state) vs cascade", ml[lv], lse[idx][lv], 2 * lse_atol)
        # the exact rules: a side that holds no key (-inf) leaves the other side's bits
        if P == 0 and not (_same(torch, mo, oo[idx]) and _same(torch, ml, ol[idx])): errs.append("merge with an empty prefix state changed the own state")
        if not bool(torch.isneginf(ol[idx][dd]).all()): errs.append("own state of a row in front of its keys is not -inf")
        if not (_same(torch, mo[dd], po[dd]) and _same(torch, ml[dd], pl[dd])): errs.append("merge with an empty own state changed the prefix state")
    return cfg, errs


def run_mla(cfg, seed, stats=None):
    import torch
    oracle, tm, t8, util = _mods("test_gpu_mla", "test_gpu_mla_fp8", "util")
    c, geo = cfg, mla_geometry(cfg)
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    kw = dict(ns=c["ns"], table_lens=geo["table_lens"] if c["roomy"] else None, extra_cols=c["extra_cols"], lead=c["lead"], tail=c["tail"], q_pad=c["q_pad"])
    fp8 = c["cache"] == "fp8"
    case = t8.Fp8Case(seed, c["dtype"], c["Hq"], c["bs"], c["Ls"], kv_scale=1.0 if c["kv_scale"] is None else c["kv_scale"], **kw) if fp8 else \
        tm.Case(seed, c["dtype"], c["Hq"], c["bs"], c["Ls"], **kw)
    assert (case.T, case.bt.shape[1], case.max_sq) == (geo["T"], geo["max_blocks"], geo["max_sq"])
    h = c["hard"]
    if h is not None:
        if h[0] == "spike":
            _, m, b, i, head, _, j = h
            case.kv[int(case.bt[b][j // case.bs]), j % case.bs] = util.quantize((m * case.q[int(case.starts[b]) + i, head]).astype(np.float32), c["dtype"])
        else:
            case.kv[..., tm.VD:] = util.quantize((case.kv[..., tm.VD:] + h[1]).astype(np.float32), c["dtype"])
        case.vmax = float(np.abs(case.kv[..., :tm.VD]).max())
        case._ref = {}
    scale, lse_atol = c["scale"], tm.LSE_ATOL
    if h is not None:
        stats["lse_f32_gap"] = case.lse_f32_gap(scale)
        lse_atol = max(lse_atol, 4.0 * stats["lse_f32_gap"])
    tensors = case.device(torch)
    if fp8:
        ks = None if c["kv_scale"] is None else torch.tensor([c["kv_scale"]], dtype=torch.float32, device="cuda")
        call = lambda: case.run(torch, scale, tensors, kv_scale=ks)   # noqa: E731
    else:
        call = lambda: case.run(torch, scale, tensors)   # noqa: E731
    out, lse = call()
    torch.cuda.synchronize()
    res = _checked(errs, tm._judge, case, out, lse, oracle, "mla", scale, lse_atol)
    if res: stats["out"], stats["lse"] = res
    own = torch.from_numpy(case.owned()).cuda()
    o2, l2 = call()
    torch.cuda.synchronize()
    if not (_same(torch, o2[own], out[own]) and _same(torch, l2[own], lse[own])): errs.append("two runs give different bits")
    if fp8:
        # the documented rule: kv_scale = 1 is the 16-bit call on the codes converted (exactly) to q's dtype
        a, al = case.run(torch, scale, tensors, kv_scale=1.0)
        w, wl = case.run16(torch, scale, tensors)
        torch.cuda.synchronize()
        if not (_same(torch, a[own], w[own]) and _same(torch, al[own], wl[own])): errs.append("fp8 with kv_scale = 1 != the 16-bit call on the converted codes")
    return cfg, errs


def run_varlen(cfg, seed, stats=None):
    import torch
    import aule
    oracle, tv, util = _mods("test_gpu_varlen", "util")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p = tv.Packed(seed, c["dtype"], c["Hq"], c["Hkv"], c["D"], c["ns"], c["ls"], lead=c["lead"], tail=c["tail"], max_sq=c["max_sq"], max_sk=c["max_sk"])
    causal = {"none": False, "top": True, "br": "bottom-right"}[c["mask"]]
    W, scale = c["window"], None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"])
    if not c["wrapper"]:
        res = tv.Run(torch, p, strided=c["strided"]).launch(causal, W, scale=scale).results()
        _checked(errs, tv._unowned_still_poisoned, torch, p, res)
    else:
        tdt = util.torch_dtype(c["dtype"])
        q, k, v = (torch.from_numpy(a).to("cuda", tdt).requires_grad_(True) for a in (p.q, p.k, p.v))
        cu_q, cu_k = (torch.from_numpy(tv._i32(x)).cuda() for x in (p.cu_q, p.cu_k))
        out, lse = aule.flash_attention_varlen(q, k, v, cu_q, cu_k, max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk, causal=causal, scale=scale,
                                               window_size=W, return_lse=True)
        dq, dk, dv = torch.autograd.grad(out, (q, k, v), torch.from_numpy(p.dout).to("cuda", tdt))
        torch.cuda.synchronize()
        res = dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv)
        oq, ok = (torch.from_numpy(~m).cuda() for m in p.owned())
        if bool(dq[oq].any()) or bool(dk[ok].any()) or bool(dv[ok].any()): errs.append("a gradient row of no sequence is not zero")
    worst = _checked(errs, tv._judge, p, res, oracle, causal, W, "varlen", scale=scale)
    if worst: stats.update(worst)
    return cfg, errs


# ------------------------------------------------------------------------------------------------------------------------------------ sinks
def sinks_problem(cfg, seed, device="cuda"):
    """(Batch, Paged or None) of tests/test_gpu_sinks.py for a draw; device="cpu": the reference side, which needs no GPU"""
    ts = importlib.import_module("test_gpu_sinks")
    c = cfg
    seqs, code = sinks_sequences(c)
    b = ts.Batch(seed, c["dtype"], c["Hq"], c["Hkv"], c["D"], code, c["window"], ns=[n for n, _ in seqs], ls=c["Ls"], ns_raw=c["ns"],
                 max_sq=c["max_sq"] if c["max_sq"] is not None else max(max(c["ns"]), 1), lead=c["lead"], tail=c["tail"],
                 scale=None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"]), rot=c["rot"],
                 sinks_dtype=c["dtype"] if c["sinks_in_q_dtype"] else None)
    assert sorted(k for _, n, _, L in b.seqs for k in keys_per_row(n, L, code, c["window"])) == sorted(sinks_row_keys(c)) and b.lmax == max(sinks_row_keys(c))
    if c["entry"] == "varlen":
        return b, None
    p = ts.Paged(b, c["cache"] == "fp8", bs=c["bs"], seed=seed + 1, extra_cols=c["extra_cols"], device=device)
    if p.fp8:
        b.vmax = float(p.v_ref.abs().max())
    return b, p


def sinks_reference(cfg, seed):
    """The reference side of a sinks draw; no GPU.  Returns (b, p, ref, plain, facts): ref with the draw's sinks (and the fp64 gradients for
    the varlen entry), plain with every sink -inf, and the facts the conditions of tests/test_fuzz_serving_draws.py read -- gap =
    max|out_ref(sinks) - out_ref(no sinks)| over the owned rows, tol = atol + rtol max|out_ref| of fwd_tol, weight = the sink weight of the
    ln(Lmax) + 0.5 head at a row with Lmax keys, and for the varlen entry e_model (the dsinks error of a backward that reads O rounded to
    storage, |model - ref| / max(1, max|ref|)), bar (DSINKS_BAR) and bound = max(bar, 4 e_model)"""
    import torch
    ts, util = importlib.import_module("test_gpu_sinks"), importlib.import_module("util")
    b, p = sinks_problem(cfg, seed, device="cpu")
    src = b if p is None else p
    ref = src.reference(grads=cfg["entry"] == "varlen")
    plain = src.reference(sinks=b.sinks.new_full(b.sinks.shape, ts.NINF))
    own = b.owned()
    atol, rtol = util.fwd_tol(b.dtype, b.vmax)
    nkeys = torch.zeros(b.Tq, dtype=torch.long)
    for sq, n, _, L in b.seqs:
        nkeys[sq:sq + n] = ts._visible(n, L, b.code, b.window).sum(dim=1)
    row = int(torch.where(own, nkeys, torch.full_like(nkeys, -1)).argmax())
    assert int(nkeys[row]) == b.lmax >= 1
    facts = dict(gap=float((ref["out"][own] - plain["out"][own]).abs().max()), tol=atol + rtol * float(ref["out"][own].abs().max()),
                 weight=float(ref["w"][row, sinks_half_head(cfg)]), blind=int((own[:, None] & ~ref["seen"]).sum()))
    if cfg["entry"] == "varlen":
        exact, model = ts.dsinks_model(b, ref)
        rds = ref["dsinks"]
        norm = max(1.0, float(rds.abs().max()))
        assert float((exact - rds).abs().max()) <= 1e-9 * norm, "the closed form of dsinks is not autograd's"
        facts["e_model"] = float((model - rds).abs().max()) / norm
        facts["bar"] = ts.DSINKS_BAR[b.dtype]
        facts["bound"] = max(facts["bar"], 4.0 * facts["e_model"])
        # dq and dk the same way: the fp64 gradient formula with delta from O rounded to storage, against the same formula on the exact O
        exact, model = ts.grads_model(b, ref)
        facts["grad_model"], facts["grad_rel"] = {}, {}
        for name, ex, mo in zip(("dq", "dk"), exact, model):
            gnorm = max(1.0, float(ref[name].abs().max()))
            assert float((ex - ref[name]).abs().max()) <= 1e-9 * gnorm, "the closed form of %s is not autograd's" % name
            facts["grad_model"][name] = float((mo - ex).abs().max())
            facts["grad_rel"][name] = facts["grad_model"][name] / gnorm
        facts["grad_binds"] = 4.0 * max(facts["grad_rel"].values()) > util.BWD_TOL[b.dtype][0]
    return b, p, ref, plain, facts


def run_sinks(cfg, seed, stats=None):
    import torch
    import aule
    _, ts, util, hostile = _mods("test_gpu_sinks", "util", "hostile")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    b, _, ref, _, facts = sinks_reference(c, seed)
    _, p = sinks_problem(c, seed)                         # (the same seeds: the same problem, its cache on the device)
    if p is not None and p.fp8:
        b.vmax = float(p.v_ref.abs().max())
    W, scale, causal = c["window"], b.scale_arg, {"none": False, "top": True, "br": "bottom-right"}[c["mask"]]
    own = b.owned().cuda()
    ninf = [h for h in range(b.Hq) if b.sinks[h] == ts.NINF]
    sinks_arg = b.sinks.to(b.tdt).cuda() if c["sinks_in_q_dtype"] else b.sinks.cuda()     # (b.sinks holds the rounded values then)
    atol, rtol = util.fwd_tol(b.dtype, b.vmax)

    def forward(what, out, lse, rows=None):
        res = _checked(errs, ts._check_forward, b, ref, out, lse, what, rows)
        if res: stats["out"], stats["lse"] = max(stats.get("out", 0.0), res[0]), max(stats.get("lse", 0.0), res[1])

    def minus_inf_heads(what, out, lse, plain, plain_lse, rows):
        for h in ninf:
            if not (_same(torch, out[rows][:, h], plain[rows][:, h]) and _same(torch, lse[rows][:, h], plain_lse[rows][:, h])):
                errs.append("%s: head %d with sink -inf is not the sinkless entry bit for bit" % (what, h)); break

    if c["entry"] == "varlen":
        q, k, v, _, cu_q, cu_k = ts._cuda(b)
        kw = dict(causal=causal, scale=scale, window_size=W)
        if not c["wrapper"]:
            # the C entries, forward and backward, into one arena of 0xFF and again into one of zeros
            dirty, _ = ts._raw_run(torch, b, hostile.POISON)
            clean, _ = ts._raw_run(torch, b, hostile.FRIENDLY)
            shapes = dict(out=(b.tdt, (b.Tq, b.Hq, b.D)), lse=(torch.float32, (b.Tq, b.Hq)), dq=(b.tdt, (b.Tq, b.Hq, b.D)),
                          dk=(b.tdt, (b.Tk, b.Hkv, b.D)), dv=(b.tdt, (b.Tk, b.Hkv, b.D)), dsinks=(torch.float32, (b.Hq,)))
            got, again = ({n: a.view(n, dt, shape) for n, (dt, shape) in shapes.items()} for a in (dirty, clean))
            if not (dirty.guards_intact() and clean.guards_intact()): errs.append("guard bytes written")
            own_k = torch.zeros(b.Tk, dtype=torch.bool)
            for _, _, sk, L in b.seqs:
                own_k[sk:sk + L] = True
            own_k = own_k.cuda()
            for n in shapes:
                rows = slice(None) if n == "dsinks" else own_k if n in ("dk", "dv") else own
                if not _same(torch, got[n][rows], again[n][rows]): errs.append("two runs give different bits in " + n)
                if n != "dsinks" and not bool((hostile.as_bytes(torch, got[n][~rows]) == hostile.POISON).all()):
                    errs.append(n + ": a row of no sequence was written")
            out, lse = got["out"], got["lse"]
            # the Python entry: the same launch; sinks in q's dtype convert exactly
            o2, l2 = aule.flash_attention_varlen_sinks(q, k, v, sinks_arg, cu_q, cu_k, b.max_sq, b.max_sk, return_lse=True, **kw)
            if not (_same(torch, o2[own], out[own]) and _same(torch, l2[own], lse[own])): errs.append("Python entry != C entry")
        else:
            sinks_arg = sinks_arg.clone()
            for t in (q, k, v, sinks_arg):
                t.requires_grad_(True)
            out, lse = aule.flash_attention_varlen_sinks(q, k, v, sinks_arg, cu_q, cu_k, b.max_sq, b.max_sk, return_lse=True, **kw)
            dout = torch.zeros_like(out)
            dout[own] = b.dout.cuda()[own]
            dq, dk, dv, ds = torch.autograd.grad(out, (q, k, v, sinks_arg), dout)
            o2, l2 = aule.flash_attention_varlen_sinks(q.detach(), k.detach(), v.detach(), sinks_arg.detach(), cu_q, cu_k, b.max_sq, b.max_sk,
                                                       return_lse=True, **kw)
            if not (_same(torch, o2[own], out.detach()[own]) and _same(torch, l2[own], lse[own])): errs.append("two runs give different bits")
            got = dict(dq=dq, dk=dk, dv=dv, dsinks=ds.float())
            out, q, k, v = out.detach(), q.detach(), k.detach(), v.detach()
            own_k = torch.zeros(b.Tk, dtype=torch.bool)
            for _, _, sk, L in b.seqs:
                own_k[sk:sk + L] = True
            own_k = own_k.cuda()
            if bool(dq[~own].any()) or bool(dk[~own_k].any()) or bool(dv[~own_k].any()): errs.append("a gradient row of no sequence is not zero")
        torch.cuda.synchronize()
        forward("varlen sinks", out, lse)
        plain, plain_lse = aule.flash_attention_varlen(q, k, v, cu_q, cu_k, b.max_sq, b.max_sk, return_lse=True, **kw)
        minus_inf_heads("varlen", out, lse, plain, plain_lse, own)
        for n in ("dq", "dk", "dv"):      # (the owned rows: the others hold the arena's 0xFF, or zeros from the wrapper)
            rows = own if n == "dq" else own_k
            res = _checked(errs, ts._check_grad, got[n][rows], ref[n][rows.cpu()], b.dtype, n, 4.0 * facts["grad_model"].get(n, 0.0))
            if res is not None: stats[n] = res
        stats["grad_model"] = max(facts["grad_rel"].values())
        rds = ref["dsinks"].numpy()
        ds = got["dsinks"].double().cpu().numpy()
        stats["dsinks"] = float(np.abs(ds - rds).max() / max(1.0, np.abs(rds).max())) if np.isfinite(ds).all() else float("inf")
        stats["dsinks_model"] = facts["e_model"]
        if not stats["dsinks"] <= facts["bound"]: errs.append("dsinks off by %.3e of max(1, max|ref|) (bound %.3e)" % (stats["dsinks"], facts["bound"]))
        if any(ds[h] != 0.0 or rds[h] != 0.0 for h in ninf): errs.append("dsinks of a head with sink -inf is not zero")
        return cfg, errs

    bt, cl = p.bt.cuda(), p.cl.cuda()
    B, Sq, Hq, D = len(b.seqs), c["Sq"], b.Hq, b.D
    kw = dict(scale=scale, window_size=W, return_lse=True, **p.scales)
    if c["entry"] == "prefill":
        cu = torch.tensor(b.cu_q, dtype=torch.int32, device="cuda")
        out, lse = ts._raw_prefill(torch, b, p, c["q_pad"])
        _checked(errs, ts._unowned_still_poisoned, torch, b, dict(out=out, lse=lse))
        forward("paged prefill sinks", out, lse)
        q = b.q.cuda()
        o2, l2 = aule.flash_attention_paged_prefill_sinks(q, p.kc, p.vc, sinks_arg, bt, cl, cu, max_seqlen_q=b.max_sq, **kw)
        if not (_same(torch, o2[own], out[own]) and _same(torch, l2[own], lse[own])): errs.append("Python entry != C entry")
        plain, plain_lse = aule.flash_attention_paged_prefill(q, p.kc, p.vc, bt, cl, cu, max_seqlen_q=b.max_sq, **kw)
        minus_inf_heads("prefill", out, lse, plain, plain_lse, own)
        n, lead = c["ns"][0], c["lead"]
        if all(x == n for x in c["ns"]) and 1 <= n <= 64:
            # the same problem by the other kernel (tests/test_gpu_tree.py::test_query_tree_and_prefill_tree_agree's relation)
            q4 = q[lead:lead + B * n].view(B, n, Hq, D).permute(0, 2, 1, 3).contiguous()
            want, wl = aule.flash_attention_paged_query_sinks(q4, p.kc, p.vc, sinks_arg, bt, cl, **kw)
            torch.cuda.synchronize()
            _close(errs, "prefill vs paged query", out[lead:lead + B * n], want.permute(0, 2, 1, 3).reshape(B * n, Hq, D), 2 * atol, 2 * rtol)
            _lse_close(errs, torch, "prefill vs paged query", lse[lead:lead + B * n], wl.permute(0, 2, 1).reshape(B * n, Hq), 2 * ts.LSE_ATOL)
    else:
        q4 = b.q.view(B, Sq, Hq, D).permute(0, 2, 1, 3).contiguous().cuda()      # [B, Hq, Sq, D]
        flat = lambda o: o.permute(0, 2, 1, 3).reshape(B * Sq, Hq, D)             # noqa: E731
        flat_lse = lambda x: x.permute(0, 2, 1).reshape(B * Sq, Hq)               # noqa: E731
        out, lse = aule.flash_attention_paged_query_sinks(q4, p.kc, p.vc, sinks_arg, bt, cl, **kw)
        o2, l2 = aule.flash_attention_paged_query_sinks(q4, p.kc, p.vc, sinks_arg, bt, cl, **kw)
        torch.cuda.synchronize()
        if not (_same(torch, o2, out) and _same(torch, l2, lse)): errs.append("two runs give different bits")
        forward("paged query sinks", flat(out), flat_lse(lse))
        plain, plain_lse = aule.flash_attention_paged_query(q4, p.kc, p.vc, bt, cl, **kw)
        minus_inf_heads("query", flat(out), flat_lse(lse), flat(plain), flat_lse(plain_lse), own)
        cu = (torch.arange(B + 1, dtype=torch.int32) * Sq).cuda()
        want, wl = aule.flash_attention_paged_prefill_sinks(b.q.cuda(), p.kc, p.vc, sinks_arg, bt, cl, cu, max_seqlen_q=Sq, **kw)
        torch.cuda.synchronize()
        _close(errs, "paged query vs prefill", flat(out), want, 2 * atol, 2 * rtol)
        _lse_close(errs, torch, "paged query vs prefill", flat_lse(lse), wl, 2 * ts.LSE_ATOL)
    torch.cuda.synchronize()
    return cfg, errs


# ------------------------------------------------------------------------------------------------------------------------------------- tree
def tree_problem(cfg, seed, device="cuda"):
    """(QueryProblem or PrefillProblem of tests/test_gpu_tree.py, words, [(start, n, kind)] per sequence) for a draw.  words: [B, Sq] or [T]
    int64 on `device`, per sequence of its kind from the data seed; garbage for a sequence of more than 64 tokens and for the rows of no
    sequence.  device="cpu": the judge's side, which needs no GPU"""
    import torch
    tt = importlib.import_module("test_gpu_tree")
    c, geo = cfg, tree_geometry(cfg)
    scale = None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"])
    g = torch.Generator().manual_seed(seed + 500)
    if c["entry"] == "query":
        p = tt.QueryProblem(torch, seed, c["dtype"], c["cache"], c["Hq"], c["Hkv"], c["Sq"], c["D"], c["bs"], c["Ls"], scale=scale,
                            extra_cols=c["extra_cols"], device=device)
        words = torch.stack([tt.words_of_kind(torch, g, kind, c["Sq"]) for kind in c["words"]])
        seqs = [(b, c["Sq"], kind) for b, kind in enumerate(c["words"])]
    else:
        p = tt.PrefillProblem(torch, seed, c["dtype"], c["cache"], Hq=c["Hq"], Hkv=c["Hkv"], D=c["D"], bs=c["bs"], tail=c["tail"],
                              nl=list(zip(c["ns"], c["Ls"])), lead=c["lead"], q_pad=c["q_pad"], scale=scale, extra_cols=c["extra_cols"], device=device)
        assert p.T == geo["T"]
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (p.T,), generator=g, dtype=torch.int64)
        seqs = []
        for b, (n, kind) in enumerate(zip(c["ns"], c["words"])):
            if 0 < n <= 64:
                words[p.starts[b]:p.starts[b] + n] = tt.words_of_kind(torch, g, kind, n)
            seqs.append((p.starts[b], n, kind if n <= 64 else "causal"))
    assert p.bt.shape == (geo["B"], geo["max_blocks"])
    return p, words.to(device), seqs


def tree_reference(cfg, seed):
    """The judge's side of a tree draw; no GPU.  Returns (ref, lref, facts): the judge under the words, and what the conditions of
    tests/test_fuzz_serving_draws.py read -- trees = the word tensors of the sequences that carry a tree other than the chain, gap = max|tree
    judge - chain judge| and tol = atol + rtol max|out_ref| of fwd_tol"""
    import torch
    util = importlib.import_module("util")
    p, words, seqs = tree_problem(cfg, seed, device="cpu")
    ref, lref = p.judge(torch, words)
    chain, _ = p.judge(torch, words, causal=True)
    atol, rtol = util.fwd_tol(p.dtype, p.vmax)
    trees = [words[s, :n] if cfg["entry"] == "query" else words[s:s + n] for s, n, kind in seqs if n > 0 and kind not in ("chain", "causal")]
    return ref, lref, dict(trees=trees, gap=float((ref - chain).abs().max()) if ref.numel() else 0.0,
                           tol=atol + rtol * (float(ref.abs().max()) if ref.numel() else 0.0))


def run_tree(cfg, seed, stats=None):
    import torch
    _, tt, util = _mods("test_gpu_tree", "util")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p, words, seqs = tree_problem(c, seed)
    ref, lref, _ = tree_reference(c, seed)
    ref, lref = ref.cuda(), lref.cuda()

    def compare(what, out, lse):
        _checked(errs, tt.compare, torch, out, lse, ref, lref, c["dtype"], p.vmax, what)
        if out.numel():
            stats["out"] = float((out.double() - ref).abs().max())
            fin = torch.isfinite(lref) & torch.isfinite(lse)
            stats["lse"] = float((lse.double()[fin] - lref[fin]).abs().max()) if bool(fin.any()) else 0.0

    if c["entry"] == "query":
        out, lse = p.run(words)
        o2, l2 = p.run(words)
        tout, tlse = p.twin()
        torch.cuda.synchronize()
        compare("query tree", out, lse)
        if not (_same(torch, out, o2) and _same(torch, lse, l2)): errs.append("two runs give different bits")
        for b, _, kind in seqs:
            if kind == "chain" and not (_same(torch, out[b], tout[b]) and _same(torch, lse[b], tlse[b])):
                errs.append("sequence %d: chain words are not the plain entry bit for bit" % b)
        return cfg, errs
    # the C entry into poisoned out / lse
    from aule import _capi
    import ctypes
    poison = torch.randn(p.T, p.Hq, p.D, generator=torch.Generator().manual_seed(1)).to(p.q.dtype).cuda()
    out, lse = poison.clone(), torch.full((p.T, p.Hq), 7.25, device="cuda")
    rc = _capi.get_lib().aule_attention_paged_prefill_tree_ex(ctypes.byref(tt.prefill_desc(torch, p, words, out, lse)))
    torch.cuda.synchronize()
    if rc != 0:
        raise RuntimeError("aule_attention_paged_prefill_tree_ex refused a valid call: %s" % tt._error(_capi.get_lib()))
    lo, hi = p.lead, p.lead + p.owned
    free = torch.ones(p.T, dtype=torch.bool, device="cuda")
    free[lo:hi] = False
    if not (torch.equal(out[free], poison[free]) and bool((lse[free] == 7.25).all())): errs.append("a row of no sequence was written")
    compare("prefill tree", out[lo:hi], lse[lo:hi])
    o2, l2 = p.run(words)
    tout, tlse = p.twin()
    torch.cuda.synchronize()
    if not (_same(torch, o2[lo:hi], out[lo:hi]) and _same(torch, l2[lo:hi], lse[lo:hi])): errs.append("two runs (the Python entry, the C entry) give different bits")
    for s, n, kind in seqs:
        if kind in ("chain", "causal") and not (_same(torch, out[s:s + n], tout[s:s + n]) and _same(torch, lse[s:s + n], tlse[s:s + n])):
            errs.append("the sequence at row %d (%s, n = %d) is not the plain entry bit for bit" % (s, kind, n))
    return cfg, errs


# ------------------------------------------------------------------------------------------------------------------------------------ mlapf
def mlapf_reference(cfg, seed):
    """The reference side of an mlapf draw; no GPU.  Returns (Packed, causal, scale, floors, facts): floors per sequence {name: 4 x the
    error of the fp64 gradient that reads O rounded to storage} (tests/test_gpu_mla_backward.py::rounding_model; 0 for dv), which a gradient
    element may miss the judge by whatever BWD_TOL says, and facts = dict(rel: the largest model error over sequences and gradients as a
    share of max(1, max|grad|), binds: 4 x rel exceeds BWD_TOL's atol, i.e. the model term is the wider one somewhere)"""
    tb, util = importlib.import_module("test_gpu_mla_backward"), importlib.import_module("util")
    c = cfg
    p = tb.Packed(seed, c["dtype"], c["H"], c["ns"], c["ls"], lead=c["lead"], tail=c["tail"], max_sq=c["max_sq"], max_sk=c["max_sk"])
    geo = mlapf_geometry(c)
    assert (p.B, p.Tq, p.Tk, p.max_sq, p.max_sk) == (geo["B"], geo["Tq"], geo["Tk"], geo["max_sq"], geo["max_sk"])
    causal = {"none": False, "top": True, "br": "bottom-right"}[c["mask"]]
    scale = None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(192.0)
    model = tb.rounding_model(p, causal, scale)
    floors = [{n: 4.0 * err[n] for n in tb.GRADS} for err, _ in model]
    rel = max(err[n] / norm[n] for err, norm in model for n in tb.GRADS)
    return p, causal, scale, floors, dict(rel=rel, binds=4.0 * rel > util.BWD_TOL[c["dtype"]][0])


def run_mlapf(cfg, seed, stats=None):
    import torch
    import aule
    oracle, tb, util = _mods("test_gpu_mla_backward", "util")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p, causal, scale, floors, facts = mlapf_reference(c, seed)
    stats["grad_model"] = facts["rel"]
    names = ("out", "lse") + tb.GRADS

    def wrapper():
        tdt = util.torch_dtype(c["dtype"])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
        q = up(p.q).requires_grad_(True)
        kvb = up(np.concatenate([p.kn, p.v], axis=2)).requires_grad_(True)
        down = torch.cat([torch.zeros(p.Tk, 512, dtype=tdt, device="cuda"), up(p.kp)], dim=1).requires_grad_(True)
        cu_q, cu_k = (torch.from_numpy(tb._i32(x)).cuda() for x in (p.cu_q, p.cu_k))
        out, lse = aule.flash_attention_mla_varlen(q, kvb[..., :tb.DN], down[:, 512:].unsqueeze(1), kvb[..., tb.DN:], cu_q, cu_k, max_seqlen_q=p.max_sq,
                                                   max_seqlen_k=p.max_sk, causal=causal, scale=scale, return_lse=True)
        (out.float() * up(p.dout).float()).sum().backward()
        torch.cuda.synchronize()
        oq, ok = (torch.from_numpy(~m).cuda() for m in (p.owned(), p.owned_k()))
        if bool(q.grad[oq].any()) or bool(kvb.grad[ok].any()) or bool(down.grad[ok].any()) or bool(down.grad[:, :512].any()):
            errs.append("a gradient outside the sequences' rows and slices is not zero")
        return dict(out=out.detach(), lse=lse, dq=q.grad, dk_nope=kvb.grad[..., :tb.DN], dk_pe=down.grad[:, 512:], dv=kvb.grad[..., tb.DN:])

    def direct(pp):
        run = tb.Run(torch, pp, in_place=c["layout"] == "in_place", wide=c["layout"] == "wide").launch(causal, scale=scale)
        return run, run.results()

    if c["wrapper"]:
        res, again = wrapper(), wrapper()
    else:
        run, res = direct(p)
        _checked(errs, tb._unowned_still_poisoned, torch, p, res, run)
        again = direct(p)[1]
    worst = _checked(errs, tb.fw._judge, p, res, oracle, causal, "mlapf", scale=scale)      # (the forward's judge, which tb._judge runs first)
    if worst: stats.update(worst)
    worst = _checked(errs, tb._judge, p, res, oracle, causal, "mlapf", scale=scale, forward=False, floors=floors)
    if worst: stats.update(worst)
    oq, ok = (torch.from_numpy(m).cuda() for m in (p.owned(), p.owned_k()))
    for n in names:
        rows = oq if n in ("out", "lse", "dq") else ok
        if not _same(torch, res[n][rows], again[n][rows]): errs.append("two runs give different bits in " + n)
    # sequence 0 alone: the same bits as in the batch (dk_pe where both runs cut the heads into the same chunks)
    sq, n, sk, L = p.sequences()[0]
    if not c["wrapper"] and n + L > 0 and p.B > 1:
        one_p = p.alone(0)
        one = direct(one_p)[1]
        same_chunks = tb._plan(torch, one_p, causal)["heads_per_chunk"] == tb._plan(torch, p, causal)["heads_per_chunk"]
        for name in names:
            a, e = (sq, sq + n) if name in ("out", "lse", "dq") else (sk, sk + L)
            if name == "dk_pe" and not same_chunks: continue
            if not _same(torch, one[name], res[name][a:e]): errs.append("sequence 0 alone differs from the same sequence in the batch in " + name)
    return cfg, errs


# ----------------------------------------------------------------------------------------------------------------------------------- sparse
def sparse_plan(cfg):
    """(planned nsplit, workspace bytes) of a sparse draw from aule_hip_debug_mla_sparse_plan: host logic over the shape, no GPU"""
    import ctypes
    from aule import _capi
    c = cfg
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads_q = {"fp16": 1, "bf16": 2}[c["dtype"]], int(c["cache"] == "fp8"), c["Hq"]
    d.num_blocks, d.block_size, d.total_tokens, d.topk = c["nb"], c["bs"], c["T"], c["topk"]
    d.q_token_stride = (c["Hq"] + c["q_pad"]) * 576
    out = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 6) == 6, c
    return out[2], (out[5] << 32) | (out[4] & 0xffffffff)


def sparse_ranges(topk, nsplit):
    """[(first entry, last entry)] of the key ranges that hold an entry: split k owns the 64-entry tiles [k ceil(tiles / nsplit), ...)
    (csrc/fa_fwd_mla_sparse_gfx950.hip); a forced count is clamped to the tiles as mla_sparse_plan clamps it"""
    tiles = (topk + 63) // 64
    nsplit = max(1, min(nsplit, 64, tiles))
    per = (tiles + nsplit - 1) // nsplit
    return [(k * per * 64, min((k + 1) * per * 64, topk) - 1) for k in range(nsplit) if k * per * 64 < topk]


def sparse_problem(cfg, seed):
    """(Problem of tests/test_gpu_mla_sparse.py, indices [T, topk] int32, info) of a draw; no GPU.  info: planned (the plan's nsplit),
    nsplit (the count the draw's launch runs: the forced one after its clamp, else the planned), ws_bytes, scale, bt (the block table of
    a contiguous-list draw) and probes [(head, position, slot, position of the second listing or None)] of a seam draw"""
    ts, util = importlib.import_module("test_gpu_mla_sparse"), importlib.import_module("util")
    c = cfg
    T, topk = c["T"], c["topk"]
    p = ts.Problem(seed, c["dtype"], T, c["Hq"], c["nb"], c["bs"], fp8=c["cache"] == "fp8", q_pad=c["q_pad"])
    rng, S = p.rng, p.S
    planned, ws_bytes = sparse_plan(c)
    ranges = sparse_ranges(topk, c["force_nsplit"] or planned)
    info = dict(planned=planned, nsplit=len(ranges), ws_bytes=ws_bytes, bt=None, probes=[], ranges=ranges,
                scale=None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(576.0))
    if c["dense"] is not None:
        mb = c["dense"][0] // c["bs"]
        info["bt"] = bt = np.stack([rng.permutation(c["nb"])[:mb] for _ in range(T)]).astype(np.int32)
        idx = np.full((T, topk), -1, dtype=np.int32)
        for t, L in enumerate(c["dense"]):
            j = np.arange(L)
            idx[t, :L] = bt[t, j // c["bs"]] * c["bs"] + j % c["bs"]
        return p, idx, info
    bad = np.array([-1, S, ts.I32_MIN, ts.I32_MAX], dtype=np.int64)
    hard = c["hard"]
    probe_t = hard[1] if hard is not None and hard[0] == "seam" else None
    nprobe = min(c["Hq"], 16, S - 1)
    spiked = rng.choice(S, size=nprobe, replace=False) if probe_t is not None else np.zeros(0, dtype=np.int64)
    idx = np.empty((T, topk), dtype=np.int64)
    dead = np.zeros((T, topk), dtype=bool)
    for t in range(T):
        pool = np.setdiff1d(np.arange(S), spiked) if t == probe_t else np.arange(S)
        if c["repeat"][t] and t != probe_t:
            pool = rng.choice(pool, size=max(1, min(len(pool), topk) // 3), replace=False)
        idx[t] = rng.choice(pool, size=topk, replace=topk > len(pool) or (c["repeat"][t] and t != probe_t))
        how = c["invalid"][t]
        if how == "scattered":
            dead[t] = rng.rand(topk) < 0.25
        elif how == "tile":
            k = int(rng.randint((topk + 63) // 64))
            dead[t, 64 * k:64 * k + 64] = True
        elif how == "split":      # one whole key range of the launch; a launch of one range: the second half of the tiles
            first, last = ranges[int(rng.randint(len(ranges)))] if len(ranges) > 1 else (((topk + 63) // 64 + 1) // 2 * 64, topk - 1)
            dead[t, first:last + 1] = True
        elif how == "all":
            dead[t] = True
    if probe_t is not None:
        t = probe_t
        if c["invalid"][t] == "scattered":      # (the list's, the first tile's and the key ranges' ends stay valid: a whole tile would not)
            dead[t, [s for s in [0, 63, 64, topk - 1] + [e for r in ranges for e in r] if s < topk]] = False
        live = np.flatnonzero(~dead[t])
        nprobe = min(nprobe, len(live))
        # the seam set, in this order and deduplicated: the list's and the first tile's ends, the ends of the key ranges (in a shuffled order,
        # so that over the draws every range is reached), the edges of the invalid runs, then random entries
        seams = [0, 63, 64, topk - 1]
        for k in rng.permutation(len(ranges)):
            seams += list(ranges[k])
        d = dead[t].astype(np.int8)
        seams += list(np.flatnonzero((d[:-1] == 0) & (d[1:] == 1))[:3]) + list(np.flatnonzero((d[:-1] == 1) & (d[1:] == 0))[:3] + 1)
        seams += list(rng.permutation(live))
        at = []
        for s in seams:
            if 0 <= s < topk and not dead[t, s] and int(s) not in at:
                at.append(int(s))
        at = at[:nprobe]
        taken = set(at)
        m = -8.0 if info["scale"] is not None and info["scale"] < 0 else 8.0      # (the spiked logit is +8 |q|^2 |scale| under either sign)
        flat = p.kv.reshape(S, ts.QK)
        for h, pos in enumerate(at):
            slot, twice = int(spiked[h]), None
            idx[t, pos] = slot
            flat[slot] = util.quantize((m * p.q[t, h]).astype(np.float32), c["dtype"])
            if h % 2 == 1:       # one probe head in two lists its slot once more, in another tile: lse rises by ln 2, out stays
                other = [int(s) for s in live if s // 64 != pos // 64 and int(s) not in taken]
                if other:
                    twice = other[int(rng.randint(len(other)))]
                    idx[t, twice] = slot
                    taken.add(twice)
            info["probes"].append((h, pos, slot, twice))
    elif hard is not None:
        p.kv[..., ts.VD:] = util.quantize((p.kv[..., ts.VD:] + hard[1]).astype(np.float32), c["dtype"])
    idx[dead] = bad[rng.randint(len(bad), size=int(dead.sum()))]
    p.vmax = float(np.abs(p.kv[..., :ts.VD]).max())
    return p, idx.astype(np.int32), info


def _sparse_alone(p, t):
    """the problem of token t alone (the hand file's construction: the same cache, one row of q)"""
    import copy
    one = copy.copy(p)
    one.q, one.T = p.q[t:t + 1], 1
    return one


def sparse_lse_f32_gap(p, idx, scale=None):
    """max |fp32 log-sum-exp - fp64 log-sum-exp| over the tokens with a valid entry: the error plain NumPy fp32 arithmetic has on these
    inputs (the hard-data LSE bound of this module follows 4 x this; it never sees a kernel's result)"""
    sc = np.float32(1.0 / math.sqrt(576.0) if scale is None else scale)
    flat = p.kv.reshape(p.S, 576).astype(np.float32)
    _, lref = p.judge(idx, scale)
    gap = 0.0
    for t in range(p.T):
        rows = flat[idx[t][p.valid(idx[t])]]
        if len(rows):
            s = p.q[t].astype(np.float32) @ rows.T * sc
            m = s.max(axis=-1, keepdims=True)
            lse = m[:, 0] + np.log(np.exp(s - m).sum(axis=-1, dtype=np.float32))
            gap = max(gap, float(np.abs(lse.astype(np.float64) - lref[t]).max()))
    return gap


def sparse_reference(cfg, seed):
    """The reference side of a sparse draw; no GPU.  Returns (p, idx, info, (out, lse), facts).  facts: valid = valid entries per token;
    probes = per probe head (units, dlse): the largest |judge without the spiked entry - judge| over the head's 512 outputs in units of
    fwd_tol's bound there, and for a slot listed twice lse(judge) - lse(judge without the second listing), else None; one_entry = on a
    plain draw, the same units for the last valid entry of the token with the most valid entries (None on a hard draw)"""
    util = importlib.import_module("util")
    p, idx, info = sparse_problem(cfg, seed)
    ref = p.judge(idx, info["scale"])
    atol, rtol = util.fwd_tol(p.dtype, p.vmax)
    valid = [int(p.valid(idx[t]).sum()) for t in range(p.T)]

    def without(t, pos, h=None):
        lean = idx[t:t + 1].copy()
        lean[0, pos] = -1
        o, l = _sparse_alone(p, t).judge(lean, info["scale"])
        hs = slice(None) if h is None else h
        return float((np.abs(o[0][hs] - ref[0][t][hs]) / (atol + rtol * np.abs(ref[0][t][hs]))).max()), l[0]

    facts = dict(valid=valid, probes=[], one_entry=None)
    if info["probes"]:
        t = cfg["hard"][1]
        for h, pos, _, twice in info["probes"]:
            if twice is None:
                facts["probes"].append((without(t, pos, h)[0], None))
            else:      # both listings away: the spike is gone; the second alone away: ln 2 less
                lean = idx[t:t + 1].copy()
                lean[0, [pos, twice]] = -1
                o, _ = _sparse_alone(p, t).judge(lean, info["scale"])
                units = float((np.abs(o[0][h] - ref[0][t][h]) / (atol + rtol * np.abs(ref[0][t][h]))).max())
                facts["probes"].append((units, float(ref[1][t][h] - without(t, twice, h)[1][h])))
    elif cfg["hard"] is None and max(valid) >= 1:
        t = int(np.argmax(valid))
        facts["one_entry"] = without(t, int(np.flatnonzero(p.valid(idx[t]))[-1]))[0]
    return p, idx, info, ref, facts


def run_sparse(cfg, seed, stats=None):
    import ctypes
    import torch
    import aule
    from aule import _capi
    _, ts, hostile = _mods("test_gpu_mla_sparse", "hostile")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p, idx, info, ref, _ = sparse_reference(c, seed)
    scale, T, topk, Hq = info["scale"], c["T"], c["topk"], c["Hq"]
    lse_atol = ts.LSE_ATOL
    if c["hard"] is not None:
        stats["lse_f32_gap"] = sparse_lse_f32_gap(p, idx, scale)
        lse_atol = max(lse_atol, 4.0 * stats["lse_f32_gap"])
    lib = _capi.get_lib()
    assert int(lib.aule_attention_mla_sparse_workspace_size(ctypes.byref(ts._desc(torch, p, T, topk)))) == info["ws_bytes"]
    assert ts.plan_of(torch, p, T, topk)[2] == info["planned"], "the device's plan is not the one the reference side read"
    run = ts.Launch(torch, p, idx, scale=scale, ws_bytes=info["ws_bytes"] if c["ws"] == "caller" else 0)
    got = _checked(errs, run.run)
    if got is None:
        return cfg, errs
    res = _checked(errs, ts.check, p, got, idx, "sparse", scale, ref, lse_atol)
    if res: stats["out"], stats["lse"] = res
    again = _checked(errs, run.run)
    if again is not None and not ts._same(torch, again, got): errs.append("two runs give different bits")
    if not ts._same(torch, run.python(), got): errs.append("Python entry != C entry")

    def forced(n):
        eff = max(1, min(n, 64, (topk + 63) // 64))      # (mla_sparse_plan's clamp: the workspace is sized for it, ranges without a tile included)
        ws = (eff * T * Hq * 514 * 4 + 15) // 16 * 16 if c["ws"] == "caller" and eff > 1 else 0
        f = ts.Launch(torch, p, idx, scale=scale, ws_bytes=ws)
        f.arena.fill(hostile.POISON)
        rc = lib.aule_hip_debug_mla_sparse_launch_nsplit(ctypes.byref(f.desc()), n)
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError("aule_hip_debug_mla_sparse_launch_nsplit(%d) refused a valid call: %s" % (n, lib.aule_get_error()))
        if not f.arena.guards_intact(): errs.append("forced nsplit %d: guard bytes written" % n)
        if not all(f.arena.unchanged(name, was) for name, was in f.inputs.items()): errs.append("forced nsplit %d: an input was written" % n)
        return f.out.clone(), f.lse.clone()

    if c["force_nsplit"] is not None:
        other = forced(c["force_nsplit"])
        res = _checked(errs, ts.check, p, other, idx, "sparse, forced nsplit %d" % c["force_nsplit"], scale, ref, lse_atol)
        if res: stats["out"], stats["lse"] = max(stats.get("out", 0.0), res[0]), max(stats.get("lse", 0.0), res[1])
        if not ts._same(torch, forced(info["planned"]), got): errs.append("the planned nsplit, forced, is not the entry bit for bit")
    if c["dense"] is not None:
        dd = _capi.MlaPagedDesc()
        dd.struct_size = ctypes.sizeof(dd)
        dd.dtype, dd.batch, dd.heads_q, dd.qk_dim, dd.v_dim = ts.DTYPE_CODE[c["dtype"]], T, Hq, 576, 512
        dd.block_size, dd.max_blocks, dd.total_tokens, dd.max_seqlen_q, dd.q_token_stride = c["bs"], info["bt"].shape[1], T, 1, (Hq + c["q_pad"]) * 576
        plan = (ctypes.c_int32 * 6)()
        assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(dd), plan, 6) == 6 and plan[2] == 1 and info["planned"] == 1
        want = aule.flash_attention_mla_paged(run.q, run.kv, torch.from_numpy(info["bt"]).cuda(), torch.tensor(c["dense"], dtype=torch.int32).cuda(),
                                              scale=scale, return_lse=True)
        torch.cuda.synchronize()
        if not ts._same(torch, got, want): errs.append("contiguous lists are not flash_attention_mla_paged bit for bit")
    return cfg, errs


# ----------------------------------------------------------------------------------------------------------------------------------- fp8mma
def _e4m3_codes(x):
    """e4m3fn codes (uint8) of an array, round to nearest even, saturating at +-448 as a cache writer does"""
    import torch
    return torch.from_numpy(np.clip(np.asarray(x, dtype=np.float32), -448.0, 448.0)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def fp8mma_problem(cfg, seed):
    """(Ragged of tests/test_gpu_paged_prefill.py over an FP8 cache, window, scale, the q row (row, head) or None, the spiked (row, head,
    block, slot, KV head) or None) of a draw; no GPU.  The q row is rewritten in the dtype; hard data is planted in the dequantised keys
    and those keys are quantised again with the head's k_scale, so the device's codes and the judge's K are what survives of it"""
    tp, tq, util = (importlib.import_module(n) for n in ("test_gpu_paged_prefill", "test_gpu_paged_query", "util"))
    c, geo = cfg, ragged_geometry(cfg)
    p = tp.Ragged(seed, c["dtype"], "fp8", c["Hq"], c["Hkv"], c["D"], c["bs"], c["ns"], c["Ls"], lead=c["lead"], tail=c["tail"],
                  table_lens=None if c["table_len"] is None else geo["table_lens"], extra_cols=c["extra_cols"])
    assert (p.T, p.bt.shape[1], p.max_sq) == (geo["T"], geo["max_blocks"], geo["max_sq"])
    g, qrow, spiked = p.Hq // p.Hkv, None, None
    if c["qrow"] is not None:
        kind, b, i, head = c["qrow"]
        row = int(p.cu[b]) + i
        x = p.q[row, head].copy()
        if kind == "zero":
            x[:] = 0.0
        elif kind == "big":
            x[int(np.abs(x).argmax())] *= 100.0
        else:      # fp16 near its largest finite value, the signs as drawn
            x = np.where(x < 0, -1.0, 1.0) * (60000.0 - 4000.0 * np.abs(x))
        p.q[row, head] = util.quantize(x.astype(np.float32), c["dtype"])
        qrow = (row, head)

    def requantise(sel, values):
        hk = sel[2]
        p.kdev[sel] = _e4m3_codes(values / p.ks[hk])
        p.K[sel] = tq._decode(p.kdev[sel]) * p.ks[hk]

    h = c["hard"]
    if h is not None and h[0] == "spike":
        _, m, b, i, head, _, j = h
        row, blk = int(p.cu[b]) + i, int(p.bt[b][j // p.bs])
        requantise((blk, j % p.bs, head // g), m * p.q[row, head].astype(np.float64))
        spiked = (row, head, blk, j % p.bs, head // g)
    elif h is not None:
        _, add, hk = h
        requantise((slice(None), slice(None), hk), p.K[:, :, hk] + add)
    p._ref = {}
    return p, c["window"], None if c["scale_mul"] is None else c["scale_mul"] / math.sqrt(c["D"]), qrow, spiked


def _fp8mma_rounded(p):
    """the problem with q replaced by what the kernel multiplies: codes * scales of aule.quantize_rows_fp8 (fp32 values)"""
    import copy
    import torch
    import aule
    codes, scales = aule.quantize_rows_fp8(torch.from_numpy(p.q))
    r = copy.copy(p)
    r.q, r._ref = (codes.float() * scales).numpy(), {}
    return r


def fp8mma_acc_term(p, window, scale):
    """E_acc [T, Hq]: per row, D 2^-20 |scale| x the largest single product |q_d k_jd| over the keys the row sees (q as the kernel
    multiplies it: p is _fp8mma_rounded's problem); 0 where a row sees no key and on the rows of no sequence.  The FP8 matrix instruction
    adds the products of a step aligned to the largest of them and keeps about 20 bits below its leading bit, so a score can be off by
    D times that unit (measured on rows that see ONE key, where lse is the scaled dot product itself: up to 2^-12.4 of the largest product
    at D = 128, and nothing when a single product is non-zero; profiles/fuzz_new_serving_kinds.txt), and a log-sum-exp moves by at most the
    largest error of its scores."""
    g = p.Hq // p.Hkv
    sc = abs(1.0 / math.sqrt(p.D) if scale is None else scale)
    term = np.zeros((p.T, p.Hq))
    for b, s, n, L in p.sequences():
        if n == 0 or L == 0:
            continue
        j = np.arange(L)
        k = np.abs(p.K[p.bt[b][j // p.bs], j % p.bs])                          # [L, Hkv, D]
        pos = L - n + np.arange(n)
        see = j[None, :] <= pos[:, None]
        if window > 0:
            see &= pos[:, None] - j[None, :] < window
        q = np.abs(p.q[s:s + n].astype(np.float64)).reshape(n, p.Hkv, g, p.D)
        for i in range(n):
            if see[i].any():
                term[s + i] = (q[i][None, :, :, :] * k[see[i]][:, :, None, :]).max(axis=(0, 3)).reshape(p.Hq)
    return p.D * 2.0 ** -20 * sc * term


def fp8mma_reference(cfg, seed):
    """The reference side of an fp8mma draw; no GPU.  Returns (p, window, scale, facts).  facts: lse_atol -- LSE_ATOL, or on a hard draw
    max(LSE_ATOL, 4 x lse_f32_gap) with lse_f32_gap the error of a NumPy fp32 log-sum-exp of the q-rounded rows against the fp64 judge;
    lse_binds -- that term is the wider one; lse_bound [T, Hq] -- lse_atol + 2 E_acc (fp8mma_acc_term), e_acc its largest value on an
    owned row and acc_binds -- 2 E_acc exceeds lse_atol on some owned row; out_rtol / round_binds -- fwd_tol's rtol, which joins the out bound as rtol |judge|, and
    whether that is the wider term of the draw; plain_lse_bound -- the bound of the plain entry's LSE against the q-rounded judge; q_gap / lse_q_gap -- the largest distance between the q-rounded and the unrounded judge in out
    / lse over the owned rows; zero_row -- (the judge's lse on the all-zero q row, ln(visible keys)) or None; spike_units -- on a spike draw
    the largest |judge with the spiked key's codes zeroed - judge| on the spiked row in units of atol + 2 E_P, else None"""
    f8, tq, util = (importlib.import_module(n) for n in ("test_gpu_paged_prefill_fp8mma", "test_gpu_paged_query", "util"))
    c = cfg
    p, W, scale, qrow, spiked = fp8mma_problem(c, seed)
    out_j, lse_j, out_p = f8._models(p, W, scale)
    out_u, lse_u, _ = f8._models(p, W, scale, rounded=False)
    own = p.owned()
    fin = own[:, None] & np.isfinite(lse_j)
    facts = dict(lse_atol=tq.LSE_ATOL, lse_binds=False, lse_f32_gap=0.0, zero_row=None, spike_units=None,
                 q_gap=float(np.abs(out_j - out_u)[own].max()) if own.any() else 0.0,
                 lse_q_gap=float(np.abs(lse_j[fin] - lse_u[fin]).max()) if fin.any() else 0.0)
    if c["hard"] is not None:
        facts["lse_f32_gap"] = _fp8mma_rounded(p).lse_f32_gap(W, scale)
        facts["lse_atol"] = max(tq.LSE_ATOL, 4.0 * facts["lse_f32_gap"])
        facts["lse_binds"] = 4.0 * facts["lse_f32_gap"] > tq.LSE_ATOL
    # the LSE bound per row: the scalar above + 2 E_acc, the accumulation of the FP8 matrix instruction (fp8mma_acc_term; the factor of E_P)
    e_acc = fp8mma_acc_term(_fp8mma_rounded(p), W, scale)
    facts["acc_binds"] = bool((2.0 * e_acc[own] > facts["lse_atol"]).any()) if own.any() else False
    facts["e_acc"] = float(e_acc[own].max()) if own.any() else 0.0
    facts["lse_bound"] = facts["lse_atol"] + 2.0 * e_acc
    atol, rtol = util.fwd_tol(p.dtype, p.vmax)
    e_p = float(np.abs(out_p - out_j)[own].max()) if own.any() else 0.0
    # the rounding of out to storage (fwd_tol's rtol |judge|) on top of atol + 2 E_P: the wider term where rows see so few keys that E_P ~ 0
    facts["out_rtol"], facts["round_binds"] = rtol, bool(own.any()) and rtol * float(np.abs(out_j[own]).max()) > atol + 2.0 * e_p
    # the plain entry's LSE: its own bound (fp32: LSE_ATOL, 4 x the fp32 gap of the unrounded rows, and 2^-21 of the largest |lse|, four
    # spacings of fp32 there) plus the distance between the two judges
    plain_gap = p.lse_f32_gap(W, scale)
    facts["plain_lse_bound"] = max(tq.LSE_ATOL, 4.0 * plain_gap, 2.0 ** -21 * (float(np.abs(lse_u[fin]).max()) if fin.any() else 0.0)) + facts["lse_q_gap"]
    if qrow is not None and c["qrow"][0] == "zero":
        _, b, i, _ = c["qrow"]
        pos = c["Ls"][b] - c["ns"][b] + i
        facts["zero_row"] = (float(lse_j[qrow]), math.log(min(pos + 1, W) if W > 0 else pos + 1))
    if spiked is not None:
        row, head, blk, slot, hk = spiked
        lean = _fp8mma_lean(p, blk, slot, hk, row, head)
        facts["spike_units"] = float(np.abs(f8._models(lean, W, scale)[0][row, head] - out_j[row, head]).max()) / (atol + 2.0 * e_p)
    return p, W, scale, facts


def _fp8mma_lean(p, blk, slot, hk, row, head):
    """the problem without one key, as q's row (row, head) sees it: the key becomes -1e4 x that row, whose weight is exp(-1e4 |q|^2 scale) = 0"""
    import copy
    lean = copy.copy(p)
    lean.K, lean._ref = p.K.copy(), {}
    lean.K[blk, slot, hk] = -1e4 * p.q[row, head]
    return lean


def run_fp8mma(cfg, seed, stats=None):
    import torch
    import aule
    _, tp, f8, util = _mods("test_gpu_paged_prefill", "test_gpu_paged_prefill_fp8mma", "util")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    p, W, scale, facts = fp8mma_reference(c, seed)
    lse_atol = facts["lse_atol"]
    if facts["lse_f32_gap"]: stats["lse_f32_gap"] = facts["lse_f32_gap"]
    out, lse, intact = tp._run_capi(torch, p, window=W, scale=scale, q_pad=c["q_pad"], entry="aule_attention_paged_prefill_fp8mma_ex")
    own = p.owned()
    if not intact: errs.append("wrote in front of or behind out / lse")
    if not tp._untouched(torch, out, lse, own): errs.append("a row of no sequence was written")
    res = _checked(errs, f8._judge, p, out, lse, W, "fp8mma", scale=scale, lse_atol=facts["lse_bound"], out_rtol=facts["out_rtol"])
    stats["e_acc"] = facts["e_acc"]
    if res: stats["out"], stats["lse"], stats["out_of_bound"] = res
    (q, kc, vc, bt, cl, cu), scales = p.device(torch, q_pad=c["q_pad"])
    kw = dict(scale=scale, window_size=W, return_lse=True, **scales)
    town = torch.from_numpy(own).cuda()
    for what in ("Python entry != C entry", "two runs give different bits"):
        o2, l2 = aule.flash_attention_paged_prefill_fp8mma(q, kc, vc, bt, cl, cu, max_seqlen_q=p.max_sq, **kw)
        torch.cuda.synchronize()
        if not (_same(torch, o2[town], out[town]) and _same(torch, l2[town], lse[town])): errs.append(what)
    # sequence 0 alone: rows are quantised independently and a workgroup serves one sequence
    s, e = int(p.cu[0]), int(p.cu[1])
    if e > s and p.B > 1:
        one = torch.tensor([0, e - s], dtype=torch.int32, device="cuda")
        a, al = aule.flash_attention_paged_prefill_fp8mma(q[s:e], kc, vc, bt[:1], cl[:1], one, **kw)
        torch.cuda.synchronize()
        if not (_same(torch, a, out[s:e]) and _same(torch, al, lse[s:e])): errs.append("sequence 0 alone differs from the same sequence in the batch")
    # the plain entry on the same cache, against the same q-rounded judge: its bound plus the distance between the two judges (from the
    # reference alone) -- the twin's masks and clamps are this kernel's
    to, tl = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=p.max_sq, **kw)
    torch.cuda.synchronize()
    out_j, lse_j, _ = f8._models(p, W, scale)
    atol, rtol = util.fwd_tol(p.dtype, p.vmax)
    _close(errs, "plain entry vs the q-rounded judge", to[town], torch.from_numpy(out_j[own]), atol + facts["q_gap"], rtol)
    _lse_close(errs, torch, "plain entry vs the q-rounded judge", tl[town].double().cpu(), torch.from_numpy(lse_j[own]), facts["plain_lse_bound"])
    return cfg, errs


# ---------------------------------------------------------------------------------------------------------------------------------- indexer
def indexer_problem(cfg, seed):
    """(Tables, Problem of tests/test_gpu_mla_indexer.py, topk) of a draw, the weights rewritten by the draw's kind; no GPU"""
    ti = importlib.import_module("test_gpu_mla_indexer")
    c = cfg
    tab = ti.Tables(seed, c["bs"], c["ctx"], ns=c["ns"], max_sq=c["max_sq"], cap=c["cap"], extra_rows=c["extra_rows"])
    p = ti.Problem(seed + 1, c["dtype"], c["H"], tab, fp8=c["fp8"], q_pad=c["q_pad"])
    h0 = seed % c["H"]
    if c["weights"] == "one":
        w = np.zeros_like(p.w)
        w[:, h0] = np.abs(p.w[:, h0]) * np.sqrt(c["H"]) + 0.5
        p.w = w
    elif c["weights"] == "negative":
        p.w = -np.abs(p.w)
    elif c["weights"] == "zero":
        p.w[:, h0] = 0.0
    return tab, p, min(tab.W + 3, 65536) if c["topk"] == "above" else c["topk"]


def indexer_logit_sources(cfg, seed, tab):
    """{name: float32 [T, W]} -- the logits the top-k kernel is given besides the logits kernel's own: "hand", the row kinds of the hand file
    rotating over the rows; "ladder", per row a base value plus 0 .. 255 units in the last place, shuffled and with repeats (only the last
    radix pass separates them); "bits", random 32-bit patterns of both signs with denormals, +-inf and NaN planted"""
    ti = importlib.import_module("test_gpu_mla_indexer")
    rng = np.random.RandomState(seed + 7)
    T, W = tab.T, tab.W
    hand = np.stack([ti.hand_made(rng, ti.ROW_KINDS[(r + seed) % len(ti.ROW_KINDS)], W) for r in range(T)])
    base = (rng.randn(T, 1) * np.exp(rng.uniform(-3, 3, size=(T, 1)))).astype(np.float32)
    base[base == 0] = 1.0
    ladder = ((base.view(np.int32) & ~0xff) + rng.randint(0, 256, size=(T, W)).astype(np.int32)).view(np.float32)      # (the upper 24 bits shared)
    bits = rng.randint(0, 2 ** 32, size=(T, W), dtype=np.uint64).astype(np.uint32)
    special = np.array([0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x00000001, 0x807fffff, 0x00000000, 0x80000000], dtype=np.uint32)
    plant = rng.rand(T, W) < 0.1
    bits[plant] = special[rng.randint(len(special), size=int(plant.sum()))]
    return dict(hand=hand, ladder=np.ascontiguousarray(ladder), bits=bits.view(np.float32))


def indexer_selection_slack(judge_row, topk):
    """(fp64 logits [p + 1], the floor a selected key's fp64 logit may not fall below): the fp64 value of the k-th largest, k = min(topk,
    p + 1), minus the row's two largest per-element bounds (a key is selected over another on logits that are each within its bound)"""
    pos, val, bound = judge_row
    k = min(topk, pos + 1)
    two = np.sort(bound)[-2:].sum()
    return val, np.sort(val)[-k] - two


def run_indexer(cfg, seed, stats=None):
    import torch
    import aule
    _, ti, ts = _mods("test_gpu_mla_indexer", "test_gpu_mla_sparse")
    c = cfg
    errs, stats = [], {} if stats is None else stats      # (stats: the caller's dict, filled with the maxima this draw measured)
    tab, p, topk = indexer_problem(c, seed)
    run = ti.LogitsLaunch(torch, p, pad=c["pad"])
    got = _checked(errs, run.run)
    if got is None:
        return cfg, errs
    worst = _checked(errs, ti.check_logits, p, got, "indexer")
    if worst is not None: stats["logits_of_bound"] = worst
    if not ti.same_owned(torch, p, got, run.python()): errs.append("logits: Python entry != C entry")
    again = _checked(errs, run.run)
    if again is not None and not ti.same_bits(torch, got, again): errs.append("logits: two runs give different bits")
    if c["fp8"] == "unit":
        as16 = _checked(errs, ti.LogitsLaunch(torch, p, as_codes=False, pad=c["pad"]).run)
        if as16 is not None and not ti.same_bits(torch, got, as16): errs.append("the FP8 call with unit scales != the 16-bit call on the converted codes")
    # top-k, judged exactly on four sources of logits (the rows of no sequence of the kernel's own logits hold 0xFF: NaN bits, never read)
    own = got.numpy()[:, :tab.W].copy()
    sources = dict(indexer_logit_sources(c, seed, tab), own=own)
    for name in INDEXER_SOURCES:
        _checked(errs, ti.check_topk, torch, tab, sources[name], topk, "top-k on %s logits" % name, pad=c["pad"], kinds=(c["positions"],))
    # the selection against fp64: every selected key's fp64 logit is at least the k-th largest fp64 logit minus the row's two largest bounds
    lists = ti.TopkLaunch(torch, tab, own, topk, c["pad"]).run(c["positions"]).numpy()
    judge = p.judge()
    short = 0.0
    for row, b, pos in tab.rows():
        if pos < 0:
            continue
        mine = lists[row][lists[row] >= 0].astype(np.int64)
        if not c["positions"]:
            back = np.full(tab.nb * tab.bs, -1, dtype=np.int64)
            back[tab.slots(b, pos + 1)] = np.arange(pos + 1)
            mine = back[mine]
        if len(mine) != min(topk, pos + 1) or (mine < 0).any() or (mine > pos).any():
            errs.append("row %d: the list does not hold min(topk, p + 1) visible keys" % row); break
        val, floor = indexer_selection_slack(judge[row], topk)
        short = max(short, float((floor - val[mine]).max()))
    stats["selection_short"] = max(short, 0.0)
    if short > 0.0: errs.append("a selected key's fp64 logit is %.3g below the k-th largest minus the two largest bounds" % short)
    if c["pipeline"] is not None:
        # the lists through the sparse MLA over a latent cache that shares the table and the block size, judged on those lists
        sp = ts.Problem(seed + 2, c["dtype"], tab.T, c["pipeline"], tab.nb, tab.bs)
        idx = lists.astype(np.int32)
        res = _checked(errs, lambda: ts.check(sp, ts.Launch(torch, sp, idx).run(), idx, "indexer lists through the sparse MLA"))
        if res: stats["out"], stats["lse"] = res
        dev = aule.mla_indexer(run.q, run.w, run.k, run.bt, run.cl, topk, cu_seqlens_q=run.cu, max_seqlen_q=tab.max_sq if tab.cu is not None else None,
                               k_scale=run.ks if run.fp8 else None) if tab.cu is not None or tab.T == tab.B else None
        if dev is not None:
            torch.cuda.synchronize()
            owned = sorted(r for r, _, _ in tab.rows())
            if not np.array_equal(dev.cpu().numpy()[owned], lists[owned]): errs.append("aule.mla_indexer != the two C entries")
    return cfg, errs


RUN = dict(indexer=run_indexer, prefill=run_prefill, cascade=run_cascade, mla=run_mla, varlen=run_varlen, sinks=run_sinks, tree=run_tree, mlapf=run_mlapf,
           sparse=run_sparse, fp8mma=run_fp8mma)
# data seed of draw i: SEED0[kind] + i
SEED0 = dict(prefill=31000, cascade=32000, mla=33000, varlen=34000, sinks=35000, tree=36000, mlapf=37000, sparse=38000, indexer=39000, fp8mma=40000)


def run_slice(kind, n, seed):
    """the n draws of `kind` at `seed`; returns (failures [(i, data seed, cfg, errs)], maxima {name: worst value})"""
    failures, worst = [], {}
    for i, cfg in enumerate(draws(kind, n, seed)):
        stats = {}
        try:
            _, errs = RUN[kind](cfg, SEED0[kind] + i, stats)
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001   (a refusal of a call that should be valid, or a device error: a finding, and the end of this run)
            errs = ["EXCEPTION %s: %s" % (type(e).__name__, " ".join(str(e).split())[:200])]
            failures.append((i, SEED0[kind] + i, cfg, errs))
            print("FAIL %s #%d seed=%d cfg=%r: %s -- the run stops here" % (kind, i, SEED0[kind] + i, cfg, errs[0]), flush=True)
            break
        for k, v in stats.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if errs:
            failures.append((i, SEED0[kind] + i, cfg, errs))
            print("FAIL %s #%d: python tools/fuzz_serving.py one %s \"%r\" %d : %s" % (kind, i, kind, cfg, SEED0[kind] + i, "; ".join(errs)), flush=True)
    return failures, worst


def _fmt(worst):
    return ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "one":
        stats = {}
        cfg, errs = RUN[a[1]](ast.literal_eval(a[2]), int(a[3]), stats)
        print("%s cfg=%r: %s  [%s]" % (a[1], cfg, "; ".join(errs) if errs else "clean", _fmt(stats)))
        sys.exit(1 if errs else 0)
    if not a or a[0] not in RUN:
        sys.exit(__doc__)
    kind, n, seed = a[0], int(a[1]) if len(a) > 1 else 100, int(a[2]) if len(a) > 2 else 0
    failures, worst = run_slice(kind, n, seed)
    print("%s: %d configurations, %d failing; maxima: %s" % (kind, n, len(failures), _fmt(worst)))
    sys.exit(1 if failures else 0)
