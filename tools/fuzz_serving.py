#!/usr/bin/env python3
"""Randomised differential test of the serving and packing entry points, the companion of tools/fuzz_parity.py (which covers the dense
forward / backward, the paged DECODE, RoPE, split-KV and windows):

    prefill   flash_attention_paged_prefill, and on the same draw flash_attention_paged_query / flash_attention_paged_amd where they apply
    cascade   flash_attention_paged_cascade and merge_attention_states
    mla       flash_attention_mla_paged and flash_attention_mla_paged_fp8
    varlen    aule_attention_varlen_forward_ex / _backward_ex, and the Python wrapper for head dims that are padded

    python tools/fuzz_serving.py KIND [n=100] [seed=0]          deterministic per seed; prints every failing configuration
    python tools/fuzz_serving.py one KIND "<cfg as printed>" SEED    one printed configuration again

Each kind is a pure draw and a run.  draw_KIND(rng) -> cfg (a dict of plain values; no torch, no GPU, no library call) and
run_KIND(cfg, seed) -> (cfg, errs) calls the library.  Every drawn call is a VALID call: hostile offsets, stale lengths and refusals belong to
tests/test_gpu_hostile_*.py, the *_refusals tests and the *_host.py files.  The judges are those of the hand-written test files
(Ragged, Cascade, Problem's conventions, Case, Fp8Case, Packed / Run and their _judge functions): the fp64 oracle on the same quantised
inputs, -inf / zeros / never-written rows exactly.

Every kind caps the cost of its judge (shrinking batch, then heads, then lengths) near 0.2 s of fp64 work per draw.

Hard data (prefill, cascade, mla; 16-bit caches; forward only): one draw in four has either one key replaced by m * (a query row that sees
it) -- m = 20, or 8 for MLA: a logit in the hundreds at a random place of the keys -- or a constant c in {2, 4} added to every key of
one KV head (MLA: to the 64 rotary columns), which moves all logits of a row alike.  `out` keeps fwd_tol; the LSE bound becomes
max(LSE_ATOL, 4 x the error a plain NumPy fp32 log-sum-exp of the same rows has against the fp64 judge): fp32 arithmetic error grows
with |S|, and the kernels take two hardware transcendental steps on top of fp32 sums.  The bound never looks at the kernel's result.
Gradients under a sharp softmax are out of scope (the varlen kind stays on Gaussian data and BWD_TOL)."""
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


DRAW = dict(prefill=draw_prefill, cascade=draw_cascade, mla=draw_mla, varlen=draw_varlen)
# The fixed-seed slices of the suite: kind -> (draws, seed).  tests/test_gpu_fuzz_serving.py runs them, tests/test_fuzz_serving_draws.py
# asserts (without a GPU) that they reach what they are for; a seed is chosen so that the latter holds.
SLICES = dict(prefill=(30, 2), cascade=(20, 3), mla=(20, 5), varlen=(20, 4))


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


RUN = dict(prefill=run_prefill, cascade=run_cascade, mla=run_mla, varlen=run_varlen)
SEED0 = dict(prefill=31000, cascade=32000, mla=33000, varlen=34000)      # data seed of draw i: SEED0[kind] + i


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
