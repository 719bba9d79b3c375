"""The MLA indexer on the GPU (csrc/fa_mla_indexer_gfx950.hip behind aule.mla_indexer_logits / mla_indexer_topk / mla_indexer and
aule_mla_indexer_logits_ex / aule_mla_indexer_topk_ex): index logits over a paged cache of index keys, and per-token top-k key lists.

LOGITS.  The judge is formed here: fp64 NumPy on the quantised inputs, I[t, s] = k_scale[s] * sum_h w[t, h] relu(q[t, h] . k[s]).  EVERY
written element is compared, with the per-element bound
    |err| <= (128 + H + 4) * 2^-23 * k_scale[s] * sum_h |w_h| sum_d |q_hd k_sd|
-- one unit in the last place per accumulated term (128 products per head in the matrix pipe, whose rounding mode is not assumed; H
terms of the head sum; the weight product, the scale and one spare), relu being 1-Lipschitz.  Invisible columns of an owned row are
-inf exactly, rows of no sequence keep their 0xFF bytes.  Every check prints the largest ratio of error to bound it reached.

TOP-K.  Judged exactly: indices equal the NumPy statement of the contract (a stable argsort over (-logit, position) of the visible
keys with NaN as -inf, the first min(topk, p + 1) in ascending position order, mapped to slots or left as positions, padded with -1)
applied to the logits the kernel was given.  (The 0xFF pre-fill of an int32 list reads -1, the pad value: that a row of no sequence
is never written shows in the logits checks and in the guard bands, not here.)

Every launch of a C entry runs inside a hostile.Arena with the outputs pre-filled with 0xFF (guard bands intact afterwards, inputs
unchanged); every cache row and every row scale that no token may read holds NaN bits."""
import ctypes

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from util import quantize, torch_dtype

pytestmark = pytest.mark.gpu

DTYPE_CODE = {"fp16": 1, "bf16": 2}
D = 128
POISON_I32 = -1   # four 0xFF bytes
BAD_BLOCKS = (2 ** 31 - 1, -2 ** 31, -7, 10 ** 9)   # table entries past a sequence's used blocks


def resolve(ctx, cu, T, W, max_sq):
    """[(L_b, s_b, n_b)]: the device-side clamps of aule_mla_paged_desc, stated in Python"""
    out = []
    for b in range(len(ctx)):
        L = min(max(int(ctx[b]), 0), W)
        if cu is None:
            s, e = b, b + 1
        else:
            s = min(max(int(cu[b]), 0), T)
            e = min(max(int(cu[b + 1]), s), T)
        out.append((L, s, min(e - s, max_sq if cu is not None else 1)))
    return out


class Tables:
    """A batch over a paged cache: context_lens as given (hostile values included), cu_seqlens_q (None: plain decode), a block table
    whose used blocks are a shuffle of the pool and whose other entries are poison.  full_table: every entry of those sequences is a
    real block (for lengths beyond the capacity, which clamp to it)."""

    def __init__(self, seed, bs, ctx, ns=None, max_sq=None, cap=None, extra_rows=0, full_table=(), cu=None):
        rng = np.random.RandomState(seed)
        self.bs, self.B = bs, len(ctx)
        self.ctx = np.asarray(ctx, dtype=np.int32)
        top = max([int(c) for b, c in enumerate(ctx) if b not in full_table] + [1])
        self.mb = -(-(cap if cap is not None else top) // bs)
        self.W = self.mb * bs
        if cu is not None:   # offsets as given (hostile values included) over extra_rows rows
            self.cu, self.T, self.max_sq = np.asarray(cu, dtype=np.int32), extra_rows, max_sq
        elif ns is None:
            self.cu, self.T, self.max_sq = None, self.B + extra_rows, 1
        else:
            self.cu = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
            self.T = int(self.cu[-1]) + extra_rows
            self.max_sq = max(ns) if max_sq is None else max_sq
        self.seqs = resolve(self.ctx, self.cu, self.T, self.W, self.max_sq)
        used = [self.mb if b in full_table else -(-L // bs) for b, (L, _, _) in enumerate(self.seqs)]
        self.nb = sum(used) + 3
        pool = rng.permutation(self.nb)
        self.table = np.empty((self.B, self.mb), dtype=np.int32)
        at = 0
        for b, u in enumerate(used):
            self.table[b, :u] = pool[at:at + u]
            self.table[b, u:] = [BAD_BLOCKS[(b + i) % len(BAD_BLOCKS)] for i in range(self.mb - u)]
            at += u

    def rows(self):
        """[(row, b, p)] of every row that belongs to a sequence"""
        return [(s + i, b, L - n + i) for b, (L, s, n) in enumerate(self.seqs) for i in range(n)]

    def slots(self, b, upto):
        """cache rows of positions 0 .. upto - 1 of sequence b"""
        j = np.arange(upto)
        return self.table[b, j // self.bs].astype(np.int64) * self.bs + j % self.bs

    def readable(self):
        """bool [nb * bs]: the cache rows some token sees"""
        seen = np.zeros(self.nb * self.bs, dtype=bool)
        for b, (L, s, n) in enumerate(self.seqs):
            if n > 0 and L > 0:
                seen[self.slots(b, L)] = True   # the last token sits at L - 1
        return seen


class Problem:
    """Seeded q [T, H, 128], weights [T, H] and key cache [nb, bs, 128] of N(0, 1), q and k quantised to `dtype` (float arrays
    holding the quantised values).  fp8: "unit" -- codes with every row scale 1; "rows" -- aule.quantize_indexer_cache_fp8's codes
    with random positive per-row scales; `k` is then the converted codes (what the judge multiplies) and `ks` the scales."""

    def __init__(self, seed, dtype, H, tab, fp8=None, q_pad=0):
        import torch
        import aule
        rng = np.random.RandomState(seed)
        self.dtype, self.H, self.tab, self.fp8, self.q_pad = dtype, H, tab, fp8, q_pad
        self.q = quantize(rng.randn(tab.T, H, D).astype(np.float32), dtype)
        self.w = (rng.randn(tab.T, H) / np.sqrt(H)).astype(np.float32)
        k = quantize(rng.randn(tab.nb, tab.bs, D).astype(np.float32), dtype)
        self.codes = None
        self.ks = np.ones((tab.nb, tab.bs), dtype=np.float32)
        if fp8:
            self.codes, _ = aule.quantize_indexer_cache_fp8(torch.from_numpy(k * (1.0 if fp8 == "rows" else 100.0)))
            k = self.codes.float().numpy()
            if fp8 == "rows":
                self.ks = np.exp(rng.uniform(-6, 3, size=(tab.nb, tab.bs))).astype(np.float32)
        self.k = k

    def cache(self, as_codes=None):
        """the cache as the device sees it (as_codes False: the converted codes as a 16-bit cache), every row no token sees NaN bits"""
        import torch
        tab = self.tab
        as_codes = bool(self.fp8) if as_codes is None else as_codes
        dead = torch.from_numpy(~tab.readable())
        if as_codes:
            c = self.codes.clone().view(torch.uint8).reshape(-1, D)
            c[dead] = 0x7F
            return c.view(torch.float8_e4m3fn).reshape(tab.nb, tab.bs, D)
        c = torch.from_numpy(self.k).to(torch_dtype(self.dtype)).reshape(-1, D).view(torch.int16)
        c[dead] = -1
        return c.view(torch_dtype(self.dtype)).reshape(tab.nb, tab.bs, D)

    def scales(self):
        import torch
        ks = torch.from_numpy(self.ks.copy()).reshape(-1).view(torch.int32)
        ks[torch.from_numpy(~self.tab.readable())] = -1
        return ks.view(torch.float32).reshape(self.tab.nb, self.tab.bs)

    def judge(self):
        """{row: (p, logits fp64 [p + 1], bound fp64 [p + 1])} for every owned row"""
        tab, flat = self.tab, self.k.reshape(-1, D).astype(np.float64)
        out = {}
        for row, b, p in tab.rows():
            if p < 0:
                out[row] = (p, np.zeros(0), np.zeros(0))
                continue
            at = tab.slots(b, p + 1)
            kk, sc = flat[at], self.ks.reshape(-1)[at].astype(np.float64)
            qq, ww = self.q[row].astype(np.float64), self.w[row].astype(np.float64)
            val = sc * (ww[:, None] * np.maximum(qq @ kk.T, 0.0)).sum(axis=0)
            mag = sc * (np.abs(ww)[:, None] * (np.abs(qq) @ np.abs(kk).T)).sum(axis=0)
            out[row] = (p, val, (D + self.H + 4) * 2.0 ** -23 * mag)
        return out


def check_logits(p, got, what):
    """every element of `got` [T, stride] (a CPU tensor): logits within the bound, -inf on the invisible columns of an owned row, 0xFF
    bytes everywhere else; prints and returns the largest error-to-bound ratio"""
    tab = p.tab
    g = got.numpy()
    raw = g.view(np.int32)
    owned = np.zeros(tab.T, dtype=bool)
    worst, seen = 0.0, 0
    for row, (pos, val, bound) in p.judge().items():
        assert not owned[row], "the case gives a row to two sequences"
        owned[row] = True
        vis = pos + 1 if pos >= 0 else 0
        x = g[row, :vis].astype(np.float64)
        assert np.isfinite(x).all(), (what, row)
        err = np.abs(x - val)
        bad = err > bound
        assert not bad.any(), "%s: row %d (p = %d): %d logits out of bound, worst |err| %.3g against %.3g at key %d" % (
            what, row, pos, int(bad.sum()), err[bad.argmax()], bound[bad.argmax()], int(bad.argmax()))
        if vis:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
            seen += vis
        assert np.isneginf(g[row, vis:tab.W]).all(), "%s: row %d: columns past p = %d must be -inf" % (what, row, pos)
        assert (raw[row, tab.W:] == POISON_I32).all(), "%s: row %d: the row's padding was written" % (what, row)
    assert (raw[~owned] == POISON_I32).all(), "%s: a row of no sequence was written" % what
    print("%s: %d logits, max |err| / bound %.3f; %d of %d rows owned" % (what, seen, worst, int(owned.sum()), tab.T))
    return worst


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


class LogitsLaunch:
    """One problem's tensors inside an Arena, aule_mla_indexer_logits_ex run on them.  Outputs and guards are 0xFF before every run;
    after it the guards are intact and the inputs unchanged.  as_codes False: an FP8 problem's converted codes as a 16-bit cache."""

    def __init__(self, torch, p, as_codes=None, pad=8):
        self.torch, self.p, tab = torch, p, p.tab
        self.fp8 = bool(p.fp8) if as_codes is None else as_codes
        dt = torch_dtype(p.dtype)
        q = torch.zeros((tab.T, p.H + p.q_pad, D), dtype=dt)
        q[:, :p.H] = torch.from_numpy(p.q).to(dt)
        cache = p.cache(self.fp8)
        self.stride = tab.W + pad
        cu = tab.cu if tab.cu is not None else np.zeros(1, dtype=np.int32)
        regions = [("q", q.numel() * 2, "in"), ("w", p.w.size * 4, "in"), ("k", cache.numel() * cache.element_size(), "in"),
                   ("ks", p.ks.size * 4, "in"), ("bt", tab.table.size * 4, "in"), ("cl", tab.B * 4, "in"), ("cu", cu.size * 4, "in"),
                   ("lg", tab.T * self.stride * 4, "out")]
        self.arena = a = Arena(torch, regions, D * 2)
        self.inputs = {"q": a.upload("q", q), "w": a.upload("w", p.w), "k": a.upload("k", cache), "ks": a.upload("ks", p.scales()),
                       "bt": a.upload("bt", tab.table), "cl": a.upload("cl", tab.ctx), "cu": a.upload("cu", cu)}
        self.q = a.view("q", dt, (tab.T, p.H + p.q_pad, D))[:, :p.H]
        self.w = a.view("w", torch.float32, (tab.T, p.H))
        self.k = a.view("k", cache.dtype, (tab.nb, tab.bs, D))
        self.ks = a.view("ks", torch.float32, (tab.nb, tab.bs))
        self.bt = a.view("bt", torch.int32, (tab.B, tab.mb))
        self.cl = a.view("cl", torch.int32, (tab.B,))
        self.cu = a.view("cu", torch.int32, (cu.size,)) if tab.cu is not None else None
        self.lg = a.view("lg", torch.float32, (tab.T, self.stride))

    def desc(self):
        from aule import _capi
        a, p, tab = self.arena, self.p, self.p.tab
        d = _capi.MlaIndexerLogitsDesc()
        d.struct_size = ctypes.sizeof(d)
        d.dtype, d.cache_dtype, d.heads, d.head_dim, d.batch = DTYPE_CODE[p.dtype], int(self.fp8), p.H, D, tab.B
        d.num_blocks, d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = tab.nb, tab.bs, tab.mb, tab.T, tab.max_sq
        d.q_token_stride, d.logits_stride = (p.H + p.q_pad) * D, self.stride
        d.device = self.torch.cuda.current_device()
        d.stream = ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        d.q, d.weights, d.k_cache, d.logits = a.ptr("q"), a.ptr("w"), a.ptr("k"), a.ptr("lg")
        d.k_scale = a.ptr("ks") if self.fp8 else None
        d.block_tables, d.context_lens = a.ptr("bt"), a.ptr("cl")
        d.cu_seqlens_q = a.ptr("cu") if tab.cu is not None else None
        return d

    def run(self):
        """the C entry; returns a CPU clone of logits [T, stride]"""
        from aule import _capi
        torch, a = self.torch, self.arena
        lib = _capi.get_lib()
        a.fill(POISON)
        rc = lib.aule_mla_indexer_logits_ex(ctypes.byref(self.desc()))
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.aule_get_error())
        assert a.guards_intact(), a.damage()
        for name, was in self.inputs.items():
            assert a.unchanged(name, was), name
        return self.lg.clone().cpu()

    def python(self):
        """the Python entry on the same tensors: [T, W] on the device"""
        import aule
        tab = self.p.tab
        rows = tab.T if tab.cu is not None else tab.B   # (plain decode: the Python entry takes one row per sequence)
        got = aule.mla_indexer_logits(self.q[:rows], self.w[:rows], self.k, self.bt, self.cl, cu_seqlens_q=self.cu,
                                      max_seqlen_q=tab.max_sq if tab.cu is not None else None, k_scale=self.ks if self.fp8 else None)
        self.torch.cuda.synchronize()
        return got


def same_owned(torch, p, a, b):
    """bit identity of two logits tensors on the rows that belong to a sequence (the others are never written)"""
    rows = torch.tensor(sorted(r for r, _, _ in p.tab.rows()), dtype=torch.long)
    W = p.tab.W
    return same_bits(torch, a.cpu()[rows][:, :W].contiguous(), b.cpu()[rows][:, :W].contiguous())


# --------------------------------------------------------------------------------------------------------------------- 1. logits: the shapes
HEADS = (1, 16, 33, 64)          # one row, half a head block, a second block of one row, two full
BLOCK_SIZES = (1, 16, 48, 64)    # 48: no power of two
CONTEXTS = (1, 63, 64, 65, 129, 1100)
# ragged: (n_b, context): decode-like, short verify, chunks of 64 and 70 tokens (16 and 18 token groups, the last of 70 with two
# tokens), a sequence without keys, and one with more new tokens than keys (p < 0 for its first 7)
RAGGED = ((1, 1100), (3, 65), (5, 129), (64, 64), (70, 1100), (2, 0), (70, 63), (1, 1))
KINDS = (("bf16", None, 0), ("fp16", None, 8), ("bf16", "rows", 16), ("fp16", "rows", 0))   # (dtype, fp8, q_pad) by case


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_logits_decode_over_the_seams(H, bs):
    """plain decode (cu_seqlens_q = NULL), one token per sequence at every context of the table, an empty sequence, and two rows of no
    sequence behind the batch"""
    import torch
    i = HEADS.index(H) + BLOCK_SIZES.index(bs)
    dtype, fp8, q_pad = KINDS[i % 4]
    tab = Tables(300 + 7 * H + bs, bs, CONTEXTS + (0,), extra_rows=2)
    p = Problem(400 + H + bs, dtype, H, tab, fp8=fp8, q_pad=q_pad)
    run = LogitsLaunch(torch, p)
    got = run.run()
    check_logits(p, got, "decode H=%d bs=%d %s%s" % (H, bs, dtype, " fp8" if fp8 else ""))
    assert same_owned(torch, p, got, run.python()), "the Python entry differs from the C entry"
    assert same_bits(torch, got, run.run()), "two runs differ"


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_logits_ragged_over_the_seams(H, bs):
    """one ragged batch with n_b = 1 / 3 / 5 / 64 / 70: groups of four tokens on a staged tile, single-token groups on the direct
    path, L_b = 0, n_b > L_b, and three rows of no sequence behind the batch"""
    import torch
    i = HEADS.index(H) + BLOCK_SIZES.index(bs) + 1
    dtype, fp8, q_pad = KINDS[i % 4]
    tab = Tables(500 + 7 * H + bs, bs, [c for _, c in RAGGED], ns=[n for n, _ in RAGGED], extra_rows=3)
    p = Problem(600 + H + bs, dtype, H, tab, fp8=fp8, q_pad=q_pad)
    run = LogitsLaunch(torch, p)
    got = run.run()
    check_logits(p, got, "ragged H=%d bs=%d %s%s" % (H, bs, dtype, " fp8" if fp8 else ""))
    assert same_owned(torch, p, got, run.python()), "the Python entry differs from the C entry"
    assert same_bits(torch, got, run.run()), "two runs differ"


def test_logits_hostile_lengths_and_a_cut_sequence():
    """context_lens far above the capacity clamp to it (those sequences own every block of their table row), a negative one is an
    empty sequence, and max_seqlen_q = 64 cuts the 70-token sequence: its last 6 rows belong to no sequence"""
    import torch
    ns, ctx = [70, 3, 2, 5], [2 ** 31 - 1, 700, -5, 100000]
    tab = Tables(71, 16, ctx, ns=ns, max_sq=64, cap=300, full_table=(0, 3))
    assert tab.W == 304 and [s[0] for s in tab.seqs] == [304, 304, 0, 304] and [s[2] for s in tab.seqs] == [64, 3, 2, 5]
    p = Problem(72, "bf16", 64, tab)
    run = LogitsLaunch(torch, p)
    got = run.run()
    check_logits(p, got, "hostile lengths")
    assert len(tab.rows()) == 64 + 3 + 2 + 5 and tab.T == 80
    assert same_owned(torch, p, got, run.python())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_logits_fp8_unit_scales_equal_the_16_bit_call_bit_for_bit(dtype):
    """with every row scale 1 the FP8 call equals the 16-bit call on the converted codes, bit for bit, in both paths of the kernel"""
    import torch
    tab = Tables(81, 48, [c for _, c in RAGGED], ns=[n for n, _ in RAGGED])
    p = Problem(82, dtype, 33, tab, fp8="unit")
    as8, as16 = LogitsLaunch(torch, p), LogitsLaunch(torch, p, as_codes=False)
    got8, got16 = as8.run(), as16.run()
    check_logits(p, got8, "fp8 unit scales " + dtype)
    assert same_bits(torch, got8, got16), "the FP8 call differs from the 16-bit call on the converted codes"


# ---------------------------------------------------------------------------------------------------------------------- 2. top-k: exact
def topk_contract(logits, tab, topk, positions):
    """the NumPy statement of the contract: int32 [T, topk], POISON_I32 on the rows of no sequence"""
    out = np.full((tab.T, topk), POISON_I32, dtype=np.int32)
    for row, b, p in tab.rows():
        out[row] = -1
        if p < 0:
            continue
        x = logits[row, :p + 1].astype(np.float64)
        x[np.isnan(x)] = -np.inf
        order = np.argsort(-x, kind="stable")          # logit descending (by value: -0 == +0), then position ascending
        sel = np.sort(order[:min(topk, p + 1)])
        out[row, :len(sel)] = sel if positions else tab.slots(b, p + 1)[sel]
    return out


def hand_made(rng, kind, W):
    """one row of hand-made logits"""
    if kind == "equal":
        return np.full(W, 0.75, dtype=np.float32)
    if kind == "ties":
        return rng.randint(0, 8, size=W).astype(np.float32)
    if kind == "zeros":   # +0 and -0 compare equal: position decides among them
        return np.where(rng.rand(W) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32) + (rng.rand(W) < 0.1) * np.float32(-1.0)
    if kind == "nans":
        x = rng.randn(W).astype(np.float32)
        x[rng.rand(W) < 0.3] = np.nan
        x[rng.rand(W) < 0.1] = -np.inf
        return x
    if kind == "ninf":    # visible -inf still counts as visible
        x = np.full(W, -np.inf, dtype=np.float32)
        x[rng.rand(W) < 0.2] = 1.0
        return x
    if kind == "up":
        return (np.arange(W, dtype=np.float64) / W - 0.5).astype(np.float32)
    if kind == "down":
        return (0.5 - np.arange(W, dtype=np.float64) / W).astype(np.float32)
    return (rng.randn(W) * np.exp(rng.uniform(-20, 20))).astype(np.float32)


ROW_KINDS = ("equal", "ties", "zeros", "nans", "ninf", "up", "down", "random")


class TopkLaunch:
    """logits, tables and the list inside an Arena, aule_mla_indexer_topk_ex run on them (outputs and guards 0xFF before every run)"""

    def __init__(self, torch, tab, logits, topk, pad=0):
        self.torch, self.tab, self.topk = torch, tab, topk
        self.stride = tab.W + pad
        lg = np.full((tab.T, self.stride), np.nan, dtype=np.float32)
        lg[:, :tab.W] = logits
        cu = tab.cu if tab.cu is not None else np.zeros(1, dtype=np.int32)
        regions = [("lg", lg.size * 4, "in"), ("bt", tab.table.size * 4, "in"), ("cl", tab.B * 4, "in"), ("cu", cu.size * 4, "in"),
                   ("idx", tab.T * topk * 4, "out")]
        self.arena = a = Arena(torch, regions, 1024)
        self.inputs = {"lg": a.upload("lg", lg), "bt": a.upload("bt", tab.table), "cl": a.upload("cl", tab.ctx), "cu": a.upload("cu", cu)}
        self.lg = a.view("lg", torch.float32, (tab.T, self.stride))[:, :tab.W]
        self.bt = a.view("bt", torch.int32, (tab.B, tab.mb))
        self.cl = a.view("cl", torch.int32, (tab.B,))
        self.cu = a.view("cu", torch.int32, (cu.size,)) if tab.cu is not None else None
        self.idx = a.view("idx", torch.int32, (tab.T, topk))

    def run(self, positions, fill=POISON):
        from aule import _capi
        torch, a, tab = self.torch, self.arena, self.tab
        lib = _capi.get_lib()
        d = _capi.MlaIndexerTopkDesc()
        d.struct_size = ctypes.sizeof(d)
        d.output, d.topk, d.batch, d.block_size, d.max_blocks = int(positions), self.topk, tab.B, tab.bs, tab.mb
        d.total_tokens, d.max_seqlen_q, d.logits_stride = tab.T, tab.max_sq, self.stride
        d.device = torch.cuda.current_device()
        d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        d.logits, d.block_tables, d.context_lens, d.indices = a.ptr("lg"), a.ptr("bt"), a.ptr("cl"), a.ptr("idx")
        d.cu_seqlens_q = a.ptr("cu") if tab.cu is not None else None
        a.fill(fill)
        rc = lib.aule_mla_indexer_topk_ex(ctypes.byref(d))
        torch.cuda.synchronize()
        assert rc == 0, (rc, lib.aule_get_error())
        assert a.guards_intact(), a.damage()
        for name, was in self.inputs.items():
            assert a.unchanged(name, was), name
        return self.idx.clone().cpu()

    def python(self, positions):
        import aule
        tab = self.tab
        got = aule.mla_indexer_topk(self.lg, self.topk, self.bt, self.cl, tab.bs, cu_seqlens_q=self.cu,
                                    max_seqlen_q=tab.max_sq if tab.cu is not None else None, output="positions" if positions else "slots")
        self.torch.cuda.synchronize()
        return got.cpu()


def check_topk(torch, tab, logits, topk, what, pad=0, kinds=(False, True)):
    run = TopkLaunch(torch, tab, logits, topk, pad)
    for positions in kinds:
        want = topk_contract(logits, tab, topk, positions)
        got = run.run(positions).numpy()
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s (%s): %d entries differ, first at row %d entry %d: got %d, contract %d" % (
            what, "positions" if positions else "slots", len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])
        assert np.array_equal(run.run(positions).numpy(), got), what + ": two runs differ"
        owned = sorted(r for r, _, _ in tab.rows())
        assert np.array_equal(run.python(positions).numpy()[owned], want[owned]), what + ": the Python entry"
    lens = [min(topk, max(p + 1, 0)) for _, _, p in tab.rows()]
    print("%s: %d rows exact, lists of %d .. %d entries of %d" % (what, len(lens), min(lens), max(lens), topk))


WIDTHS = (1, 255, 256, 257, 4096, 70001)
TOPKS = (1, 63, 64, 65, 2048, "above")   # "above": more than any row sees -- every visible key and the -1 tail


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("topk", TOPKS, ids=str)
def test_topk_hand_made_logits(W, topk):
    """eight decode rows, one per kind of hand-made logits, over a shuffled table of block size 1: the first four rows see all W keys,
    the others fewer (a whole number of 1024-chunks where there is one, one key more, about half, one key)"""
    import torch
    topk = min(W + 3, 65536) if topk == "above" else topk
    rng = np.random.RandomState(W + topk)
    ctx = [W, W, W, W, max(W // 1024 * 1024, 1), min(W // 1024 * 1024 + 1, W), max(W // 2, 1), 1]
    order = rng.permutation(8)
    tab = Tables(W + 17 * topk, 1, [ctx[i] for i in order], cap=W)
    logits = np.stack([hand_made(rng, ROW_KINDS[r], W) for r in range(8)])
    check_topk(torch, tab, logits, topk, "W=%d topk=%d" % (W, topk), kinds=((W + topk) % 2 == 1,))


@pytest.mark.parametrize("bs,mb", [(1, 300), (16, 19), (48, 7)])
def test_topk_block_sizes_both_outputs_and_a_ragged_batch(bs, mb):
    """slots through shuffled tables of block size 1 / 16 / 48 and raw positions, on a ragged batch: several tokens per sequence at
    different p, p < 0, an empty sequence, a cut sequence, rows of no sequence, a row stride wider than the table"""
    import torch
    W = bs * mb
    ns, ctx = [5, 3, 9, 2, 1], [W, 2, W // 2, 0, W + 1000]
    tab = Tables(900 + bs, bs, ctx, ns=ns, max_sq=7, cap=W, extra_rows=2, full_table=(4,))
    assert tab.W == W and tab.seqs[2][2] == 7 and tab.seqs[1] == (2, 5, 3) and tab.seqs[4][0] == W
    rng = np.random.RandomState(bs)
    logits = np.stack([hand_made(rng, ROW_KINDS[(r * 3 + 1) % 8], W) for r in range(tab.T)])
    for topk in (1, 16, 64, W // 2 + 1, W, W + 5):
        check_topk(torch, tab, logits, topk, "bs=%d topk=%d" % (bs, topk), pad=5)


def test_topk_hostile_offsets_and_lengths():
    """cu_seqlens_q = [-5, 2, 9, 3] (negative, past the end, decreasing) and context_lens = [-7, 1000, 5] over 6 rows of 2 blocks of 16:
    after the clamps sequence 0 owns rows 0 - 1 with no key (lists of -1), sequence 1 rows 2 - 4 with the table's 32 keys, sequence 2 no
    row, and row 5 belongs to nobody.  Both outputs against the contract; the list is pre-filled once with 0xFF and once with 0x00, so
    that row 5 shows the fill's bytes both times (-1 is also the pad value); guards intact and inputs unchanged in every run."""
    import torch
    from hostile import FRIENDLY
    tab = Tables(950, 16, [-7, 1000, 5], max_sq=3, cap=32, extra_rows=6, full_table=(1,), cu=[-5, 2, 9, 3])
    assert (tab.T, tab.B, tab.mb, tab.W) == (6, 3, 2, 32) and tab.seqs == [(0, 0, 2), (32, 2, 3), (5, 6, 0)]
    assert [(r, b, p) for r, b, p in tab.rows()] == [(0, 0, -2), (1, 0, -1), (2, 1, 29), (3, 1, 30), (4, 1, 31)]
    rng = np.random.RandomState(951)
    logits = np.stack([hand_made(rng, ROW_KINDS[(r * 3 + 1) % 8], tab.W) for r in range(tab.T)])
    run = TopkLaunch(torch, tab, logits, 4)
    for positions in (False, True):
        want = topk_contract(logits, tab, 4, positions)
        assert (want[:2] == -1).all() and (want[2:5] >= 0).all()
        for fill, word in ((POISON, -1), (FRIENDLY, 0)):
            got = run.run(positions, fill).numpy()
            assert np.array_equal(got[:5], want[:5]), (positions, got, want)
            assert (got[5] == word).all(), "row 5 belongs to no sequence and was written: %s" % got[5]


# ------------------------------------------------------------------------------------------------------------------------ 3. end to end
def _e2e(torch, seed, dtype, H, bs, ns, ctx, fp8=None):
    tab = Tables(seed, bs, ctx, ns=ns)
    p = Problem(seed + 1, dtype, H, tab, fp8=fp8)
    dev = dict(q=torch.from_numpy(p.q).to(torch_dtype(dtype)).cuda(), w=torch.from_numpy(p.w).cuda(), k=p.cache().cuda(),
               bt=_i32(torch, tab.table).cuda(), cl=_i32(torch, tab.ctx).cuda(), cu=_i32(torch, tab.cu).cuda(),
               ks=p.scales().cuda() if fp8 else None)
    return tab, p, dev


@pytest.mark.parametrize("fp8", [None, "rows"], ids=["16", "fp8"])
def test_indexer_end_to_end_threshold(fp8):
    """aule.mla_indexer on random inputs, 40 tokens over 3 sequences, context <= 600, topk 128: the indices are the contract applied
    to the returned logits, the logits are within the bound, and the smallest selected logit is >= the largest unselected visible one"""
    import torch
    import aule
    tab, p, dev = _e2e(torch, 1001, "bf16", 64, 16, [17, 20, 3], [600, 333, 90], fp8=fp8)
    assert tab.T == 40
    idx, logits = aule.mla_indexer(dev["q"], dev["w"], dev["k"], dev["bt"], dev["cl"], 128, cu_seqlens_q=dev["cu"], k_scale=dev["ks"],
                                   output="positions", return_logits=True)
    slots = aule.mla_indexer(dev["q"], dev["w"], dev["k"], dev["bt"], dev["cl"], 128, cu_seqlens_q=dev["cu"], max_seqlen_q=20, k_scale=dev["ks"])
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (40, 128) and tuple(logits.shape) == (40, tab.W) and logits.dtype == torch.float32
    lg = logits.cpu()
    worst = 0.0
    for row, (pos, val, bound) in p.judge().items():
        x = lg[row, :pos + 1].numpy().astype(np.float64)
        assert (np.abs(x - val) <= bound).all() and np.isneginf(lg[row, pos + 1:].numpy()).all(), row
        worst = max(worst, float((np.abs(x - val) / bound).max()))
    print("end to end: max |err| / bound %.3f" % worst)
    assert np.array_equal(idx.cpu().numpy(), topk_contract(lg.numpy(), tab, 128, True))
    assert np.array_equal(slots.cpu().numpy(), topk_contract(lg.numpy(), tab, 128, False))
    for row, b, pos in tab.rows():
        mine = idx[row].cpu().numpy()
        mine = mine[mine >= 0]
        assert len(mine) == min(128, pos + 1) and (np.diff(mine) > 0).all() and mine.max() <= pos
        x = lg[row, :pos + 1].numpy()
        rest = np.setdiff1d(np.arange(pos + 1), mine)
        if len(rest):
            assert x[mine].min() >= x[rest].max(), row


def _plan_ints(hook, d, n):
    out = (ctypes.c_int32 * n)()
    assert hook(ctypes.byref(d), out, n) == n
    return list(out)


def test_full_lists_through_sparse_mla_equal_paged_mla_bit_for_bit():
    """topk >= every context: the list of a token is every key it sees, ascending, as slots -- so the sparse MLA over the lists equals
    the paged MLA on the same ragged causal problem bit for bit (both plans say one split: checked through the two plan hooks).  This
    pins the slot convention against the consumer."""
    import torch
    import aule
    from aule import _capi
    Hq, topk, bs = 16, 127, 16
    tab, p, dev = _e2e(torch, 2001, "bf16", 32, bs, [9, 1, 14], [100, 57, 14])
    assert tab.W == 112 and tab.T == 24
    g = torch.Generator().manual_seed(7)
    ql = torch.randn(tab.T, Hq, 576, generator=g).to(torch.bfloat16).cuda()
    kv = torch.randn(tab.nb, bs, 576, generator=g).to(torch.bfloat16).cuda()
    # one split on both sides
    lib = _capi.load()
    dp = _capi.MlaPagedDesc()
    dp.struct_size = ctypes.sizeof(dp)
    dp.dtype, dp.batch, dp.heads_q, dp.qk_dim, dp.v_dim, dp.block_size, dp.max_blocks = 2, tab.B, Hq, 576, 512, bs, tab.mb
    dp.total_tokens, dp.max_seqlen_q, dp.q_token_stride, dp.cu_seqlens_q = tab.T, 14, Hq * 576, 4096
    dp.device = torch.cuda.current_device()
    ds = _capi.MlaSparseDesc()
    ds.struct_size = ctypes.sizeof(ds)
    ds.dtype, ds.heads_q, ds.num_blocks, ds.block_size, ds.total_tokens, ds.topk, ds.q_token_stride = 2, Hq, tab.nb, bs, tab.T, topk, Hq * 576
    ds.device = torch.cuda.current_device()
    assert _plan_ints(lib.aule_hip_debug_mla_plan, dp, 6)[2] == 1 and _plan_ints(lib.aule_hip_debug_mla_sparse_plan, ds, 6)[2] == 1
    idx = aule.mla_indexer(dev["q"], dev["w"], dev["k"], dev["bt"], dev["cl"], topk, cu_seqlens_q=dev["cu"], max_seqlen_q=14)
    torch.cuda.synchronize()
    for row, b, pos in tab.rows():
        want = np.full(topk, -1, dtype=np.int64)
        want[:pos + 1] = tab.slots(b, pos + 1)
        assert np.array_equal(idx[row].cpu().numpy(), want), row
    sparse = aule.flash_attention_mla_sparse(ql, kv, idx, return_lse=True)
    paged = aule.flash_attention_mla_paged(ql, kv, dev["bt"], dev["cl"], cu_seqlens_q=dev["cu"], max_seqlen_q=14, return_lse=True)
    torch.cuda.synchronize()
    assert same_bits(torch, sparse[0], paged[0]) and same_bits(torch, sparse[1], paged[1])
    assert bool(torch.isfinite(sparse[0].float()).all()) and float(sparse[0].float().abs().max()) > 0


def _capture(torch, fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def test_graph_capture_replays_with_the_current_tables_lengths_and_weights():
    """a torch.cuda.graph capture of aule.mla_indexer (no synchronisation, no host copy: the tables, lengths and weights are read by
    the kernels in place); after changing context_lens, the table and the weights IN PLACE a replay gives what an eager call gives"""
    import torch
    import aule
    tab, p, dev = _e2e(torch, 3001, "fp16", 64, 16, [1, 4, 2], [290, 150, 77])
    # every block of the pool holds finite keys here: the second set of tables reads other rows
    dev["k"] = torch.from_numpy(p.k).to(torch.float16).cuda()
    fn = lambda: aule.mla_indexer(dev["q"], dev["w"], dev["k"], dev["bt"], dev["cl"], 64, cu_seqlens_q=dev["cu"], max_seqlen_q=4,   # noqa: E731
                                  return_logits=True)
    eager = [t.clone() for t in fn()]
    g, out = _capture(torch, fn)
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(torch, out[0], eager[0]) and same_owned(torch, p, out[1], eager[1])
    # new lengths, another table (the real blocks in another order), other weights -- in place
    dev["cl"].copy_(_i32(torch, [160, 290, 33]).cuda())
    real = torch.from_numpy(np.random.RandomState(9).permutation(tab.nb)[:tab.mb].astype(np.int32)).cuda()
    dev["bt"].copy_(torch.stack([real, real.flip(0), real.roll(5)]))
    dev["w"].mul_(-0.5).add_(0.125)
    g.replay()
    torch.cuda.synchronize()
    again = fn()
    torch.cuda.synchronize()
    assert not same_bits(torch, again[0], eager[0])
    assert same_bits(torch, out[0], again[0]) and same_owned(torch, p, out[1], again[1])
    lg = again[1].cpu().numpy()
    tab.ctx, tab.table = dev["cl"].cpu().numpy(), dev["bt"].cpu().numpy()
    tab.seqs = resolve(tab.ctx, tab.cu, tab.T, tab.W, 4)
    assert np.array_equal(again[0].cpu().numpy(), topk_contract(lg, tab, 64, False))
