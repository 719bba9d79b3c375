"""Tree masks on the GPU: aule.flash_attention_paged_query_tree and aule.flash_attention_paged_prefill_tree (the
fa_fwd_paged_tree_kernel instances of csrc/fa_fwd_splitkv_gfx950.hip and the fa_fwd_paged_prefill_tree_kernel instances of
csrc/fa_fwd_paged_prefill_gfx950.hip) and their C entries.

The judge is written here: a torch float64 softmax over each sequence's keys with the boolean visibility matrix of the rule --
query i of a sequence with L keys and n new tokens sees key j < L iff j < L - n or bit j - (L - n) of its word is set; a query at a
negative position sees nothing.  The test lays the keys of a sequence out logically ([L, heads_kv, head_dim]) and scatters them into
shuffled pages itself, so the judge needs no gather; FP8 caches are dequantised exactly (scale[hk] * float(code) in float64).
Out is held to fwd_tol(dtype, max |V|) of tests/util.py, the LSE to the 1e-3 of tests/test_gpu_paged_query.py, and rows without a
key are compared exactly (zeros, -inf)."""
import ctypes
import math

import pytest

from util import fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

CODE_8 = 0x50      # e4m3fn code of 8.0 (tests/test_gpu_paged_fp8.py): the finite codes with |x| <= 8
LSE_ATOL = 1e-3    # tests/test_gpu_paged_query.py
KINDS = ["16", "fp8"]


# ---- masks: drawn on the CPU from a seed, so that what they cover can be checked without a GPU

def chain_words(torch, n):
    """(2 << i) - 1 as int64 (i = 63: all ones)"""
    return torch.tensor([((2 << i) - 1) - ((1 << 64) if i == 63 else 0) for i in range(n)], dtype=torch.int64)


def random_parents(torch, g, n):
    """a random tree: parent uniform in [-1, i) -- -1: a child of the context"""
    return (torch.rand(n, generator=g) * (torch.arange(n) + 1)).long() - 1


WORD_KINDS = ("tree", "random", "emptied", "ones", "chain")


def words_of_kind(torch, g, kind, Sq):
    """[Sq] int64 from the generator g: a random tree, uniform random words, random words with emptied rows, all ones, or the chain"""
    import aule
    kind = WORD_KINDS.index(kind) if isinstance(kind, str) else kind
    if kind == 0:
        return aule.tree_mask_from_parents(random_parents(torch, g, Sq))
    if kind == 3:
        return torch.full((Sq,), -1, dtype=torch.int64)
    if kind == 4:
        return chain_words(torch, Sq)
    w = torch.randint(-2 ** 63, 2 ** 63 - 1, (Sq,), generator=g, dtype=torch.int64)
    if kind == 2:
        w[torch.rand(Sq, generator=g) < 0.4] = 0
        w[Sq // 2] = 0
    return w


def draw_words(torch, seed, B, Sq):
    """[B, Sq] int64: sequence b takes pattern b % 4 -- a random tree, uniform random words, random words with emptied rows, all ones"""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([words_of_kind(torch, g, b % 4, Sq) for b in range(B)])


def words_are_not_trivial(seqs):
    """seqs: the word tensors of some sequences, [n] each.  Over their rows, in the n bits that count: at least a quarter differ from the
    chain word, at least one is empty, and -- where a sequence has more than one token -- at least one names a token behind its own"""
    rows = [(i, w & ((1 << len(s)) - 1)) for s in seqs for i, w in enumerate(s.tolist())]
    differ = sum(w != (2 << i) - 1 for i, w in rows)
    assert 4 * differ >= len(rows), (differ, len(rows))
    assert any(w == 0 for _, w in rows)
    assert all(len(s) <= 1 for s in seqs) or any(w >> (i + 1) for i, w in rows)


# ---- problems

def make_kv(torch, g, dtype, kind, lens, Hkv, D):
    """per sequence: what the cache holds ([L, Hkv, D]: 16-bit values or e4m3fn codes as uint8) for K and V, and the float64 K and V the
    judge sees; plus the FP8 scales (or None)"""
    dt = torch_dtype(dtype)
    dev, f64, scales = [], [], None
    if kind == "fp8":
        ks, vs = (torch.rand(Hkv, generator=g) * 1.75 + 0.25 for _ in range(2))
        scales = (ks, vs)
    for L in lens:
        if kind == "fp8":
            pair = [(torch.randint(0, CODE_8 + 1, (L, Hkv, D), generator=g) | (torch.randint(0, 2, (L, Hkv, D), generator=g) << 7)).to(torch.uint8)
                    for _ in range(2)]
            f64.append(tuple(c.view(torch.float8_e4m3fn).double() * s.double().view(1, -1, 1) for c, s in zip(pair, scales)))
        else:
            pair = [torch.randn(L, Hkv, D, generator=g).to(dt) for _ in range(2)]
            f64.append(tuple(x.double() for x in pair))
        dev.append(tuple(pair))
    return dev, f64, scales


def paginate(torch, g, dev, bs, shared=None, extra_cols=2):
    """scatter the sequences' rows into shuffled pages: (k_cache, v_cache, block_tables) on the CPU; unused table columns point at block 0,
    unused rows of a page hold finite junk"""
    nblk = [(k.shape[0] + bs - 1) // bs for k, _ in dev]
    num_blocks = sum(nblk) + 3
    proto = dev[0][0]
    if proto.dtype == torch.uint8:
        caches = [torch.randint(0, CODE_8 + 1, (num_blocks, bs) + tuple(proto.shape[1:]), generator=g).to(torch.uint8) for _ in range(2)]
    else:
        caches = [torch.randn((num_blocks, bs) + tuple(proto.shape[1:]), generator=g).to(proto.dtype) for _ in range(2)]
    bt = torch.zeros(len(dev), max(max(nblk), 1) + extra_cols, dtype=torch.int32)
    perm = torch.randperm(num_blocks, generator=g)
    used = 0
    for b, pair in enumerate(dev):
        blocks = perm[used:used + nblk[b]]
        used += nblk[b]
        bt[b, :nblk[b]] = blocks.int()
        for cache, x in zip(caches, pair):
            for i, blk in enumerate(blocks.tolist()):
                part = x[i * bs:(i + 1) * bs]
                cache[blk, :part.shape[0]] = part
    return caches[0], caches[1], bt


def to_device(torch, kc, vc, scales, device="cuda"):
    if kc.dtype == torch.uint8:
        kc, vc = kc.to(device).view(torch.float8_e4m3fn), vc.to(device).view(torch.float8_e4m3fn)
        return kc, vc, dict(k_scale=scales[0].float().to(device), v_scale=scales[1].float().to(device))
    return kc.to(device), vc.to(device), {}


def visibility(torch, L, n, words, causal=False):
    """[n, L] bool of the rule (words: [n] int64 on any device); causal: the twin's rule j <= L - n + i instead of the words"""
    j = torch.arange(L, device=words.device)
    i = torch.arange(n, device=words.device)
    pos = L - n + i
    if causal:
        return j[None, :] <= pos[:, None]
    bit = j - (L - n)
    is_set = ((words[:, None] >> bit.clamp(0, 63)[None, :]) & 1) != 0
    return ((bit < 0)[None, :] | is_set) & (pos >= 0)[:, None]


def judge(torch, q, K, V, vis, scale):
    """q [n, Hq, D], K / V [L, Hkv, D], all float64 on one device, vis [n, L] -> out [n, Hq, D], lse [n, Hq] (zeros and -inf for a row
    without a key)"""
    n, Hq, D = q.shape
    L, Hkv, _ = K.shape
    g = Hq // Hkv
    out = torch.zeros(n, Hq, D, dtype=torch.float64, device=q.device)
    lse = torch.full((n, Hq), -math.inf, dtype=torch.float64, device=q.device)
    if L == 0 or n == 0:
        return out, lse
    s = torch.einsum("nhgd,lhd->nhgl", q.view(n, Hkv, g, D), K) * scale
    s = s.masked_fill(~vis[:, None, None, :], -math.inf)
    some = vis.any(dim=1)
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    z = p.sum(dim=-1, keepdim=True)
    o = torch.einsum("nhgl,lhd->nhgd", p / torch.where(z > 0, z, torch.ones_like(z)), V).reshape(n, Hq, D)
    l = (m + torch.log(z)).reshape(n, Hq)
    out[some], lse[some] = o[some], l[some]
    return out, lse


def compare(torch, out, lse, ref, lref, dtype, vmax, what, factor=1.0, lse_atol=LSE_ATOL):
    """out within factor x fwd_tol, lse within lse_atol; rows without a key exactly zeros and -inf; prints the figures first"""
    atol, rtol = fwd_tol(dtype, vmax)
    atol, rtol = factor * atol, factor * rtol
    out, lse = out.double(), lse.double()
    none = torch.isneginf(lref)
    err = (out - ref).abs()
    over = float((err - (atol + rtol * ref.abs())).max())
    lerr = float((lse[~none] - lref[~none]).abs().max()) if bool((~none).any()) else 0.0
    print("%s: max |out err| %.3g (atol %.3g, worst margin %.3g), max |lse err| %.3g (bound %.3g), rows without a key %d"
          % (what, float(err.max()), atol, over, lerr, lse_atol, int(none.sum())))
    assert bool(torch.isfinite(out).all()) and not bool(torch.isnan(lse).any()), what
    assert over <= 0.0, (what, float(err.max()), atol)
    assert torch.equal(torch.isneginf(lse), none), "%s: lse must be -inf exactly where a row sees no key" % what
    assert bool((out[none] == 0).all()), "%s: a row that sees no key must be zeros" % what
    assert lerr <= lse_atol, (what, lerr)


class QueryProblem:
    """B sequences of Sq new tokens each; q [B, Hq, Sq, D].  scale: None for 1 / sqrt(D); device="cpu": the judge's side alone"""

    def __init__(self, torch, seed, dtype, kind, Hq, Hkv, Sq, D, bs, lens, scale=None, extra_cols=2, device="cuda"):
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.Sq, self.lens, self.D, self.scale = dtype, Sq, list(lens), D, scale
        dev, self.f64, scales = make_kv(torch, g, dtype, kind, lens, Hkv, D)
        kc, vc, bt = paginate(torch, g, dev, bs, extra_cols=extra_cols)
        self.kc, self.vc, self.scales = to_device(torch, kc, vc, scales, device)
        qs = 0.25 if kind == "fp8" else 1.0
        self.q = (qs * torch.randn(len(lens), Hq, Sq, D, generator=g)).to(torch_dtype(dtype)).to(device)
        self.bt, self.cl = bt.to(device), torch.tensor(lens, dtype=torch.int32).to(device)
        self.vmax = max(float(v.abs().max()) for _, v in self.f64 if v.numel()) if any(lens) else 1.0

    def run(self, words):
        import aule
        return aule.flash_attention_paged_query_tree(self.q, self.kc, self.vc, words, self.bt, self.cl, scale=self.scale, return_lse=True,
                                                     **self.scales)

    def twin(self):
        import aule
        return aule.flash_attention_paged_query(self.q, self.kc, self.vc, self.bt, self.cl, scale=self.scale, return_lse=True, **self.scales)

    def judge(self, torch, words, causal=False):
        """causal: the chain's rule for every sequence instead of its words"""
        outs, lses = [], []
        for b, L in enumerate(self.lens):
            K, V = (x.to(self.q.device) for x in self.f64[b])
            vis = visibility(torch, L, self.Sq, words[b], causal=causal)
            o, l = judge(torch, self.q[b].double().permute(1, 0, 2).contiguous(), K, V, vis,
                         1.0 / math.sqrt(self.D) if self.scale is None else self.scale)
            outs.append(o.permute(1, 0, 2))
            lses.append(l.permute(1, 0))
        return torch.stack(outs), torch.stack(lses)


def query_lens(Sq):
    """the new tokens straddle 32-key tiles and more than one wave's chunk; the last sequence has L < Sq"""
    return [45, 100, 257, 1000, Sq // 2]


QUERY_CASES = [   # dtype, cache kind, Hq, Hkv, Sq, D, block size
    ("bf16", "16", 8, 2, 13, 128, 16),      # Hq / Hkv = 4 x 13 tokens: 52 packed rows, the second 32-row tile crosses a head boundary
    ("fp16", "fp8", 8, 2, 13, 64, 24),      # ... the general address path, FP8
    ("fp16", "16", 4, 2, 1, 64, 16),        # the decode: one word bit
    ("bf16", "fp8", 4, 2, 5, 128, 16),
    ("bf16", "16", 4, 1, 33, 64, 24),       # words that use the high half; 132 rows
    ("fp16", "fp8", 2, 2, 33, 128, 16),
    ("fp16", "16", 4, 2, 64, 128, 24),      # bit 63
    ("bf16", "fp8", 2, 1, 64, 64, 16),
]


@pytest.mark.parametrize("case", QUERY_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_query_tree_against_the_judge(case):
    import torch
    dtype, kind, Hq, Hkv, Sq, D, bs = case
    p = QueryProblem(torch, 100 + Sq, dtype, kind, Hq, Hkv, Sq, D, bs, query_lens(Sq))
    words = draw_words(torch, 8 + Sq, len(p.lens), Sq)      # (seeds for which words_are_not_trivial holds: checked on the CPU)
    words_are_not_trivial(list(words))
    words = words.cuda()
    out, lse = p.run(words)
    ref, lref = p.judge(torch, words)
    compare(torch, out, lse, ref, lref, dtype, p.vmax, "query tree %s" % (case,))
    assert bool(torch.isneginf(lref).any())               # (the emptied rows and the rows at negative positions)
    # two runs of the same call agree bit for bit
    out2, lse2 = p.run(words)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


class PrefillProblem:
    """the mixed batch: per sequence (n new tokens, L keys); g = Hq / Hkv = 4, so 64 tokens span two 128-row blocks; `tail` rows of q
    that no sequence owns"""
    NL = [(100, 300), (64, 141), (7, 200), (1, 50), (0, 30), (20, 11)]   # L - n = 200, 77, 193, 49, 30, -9

    def __init__(self, torch, seed, dtype, kind, Hq=8, Hkv=2, D=64, bs=16, tail=5, nl=None, lead=0, q_pad=0, scale=None, extra_cols=2,
                 device="cuda"):
        """lead: rows of q in front of the first sequence (the owned rows are lead .. lead + owned); q_pad > 0: q is a slice of a projection
        that much wider per token whose other columns hold NaN bits; scale: None for 1 / sqrt(D); device="cpu": the judge's side alone"""
        g = torch.Generator().manual_seed(seed)
        self.nl = list(self.NL if nl is None else nl)
        self.dtype, self.D, self.Hq, self.scale, self.lead = dtype, D, Hq, scale, lead
        ns, lens = [n for n, _ in self.nl], [L for _, L in self.nl]
        dev, self.f64, scales = make_kv(torch, g, dtype, kind, lens, Hkv, D)
        kc, vc, bt = paginate(torch, g, dev, bs, extra_cols=extra_cols)
        self.kc, self.vc, self.scales = to_device(torch, kc, vc, scales, device)
        self.owned = sum(ns)
        self.T = lead + self.owned + tail
        qs = 0.25 if kind == "fp8" else 1.0
        self.q = (qs * torch.randn(self.T, Hq, D, generator=g)).to(torch_dtype(dtype)).to(device)
        if q_pad:
            wide = torch.full((self.T, Hq * D + q_pad), -1, dtype=torch.int16, device=device).view(self.q.dtype)
            wide[:, :Hq * D] = self.q.view(self.T, -1)
            self.q = wide[:, :Hq * D].view(self.T, Hq, D)
        self.starts = [lead + sum(ns[:b]) for b in range(len(ns) + 1)]
        self.bt, self.cl = bt.to(device), torch.tensor(lens, dtype=torch.int32).to(device)
        self.cu = torch.tensor(self.starts, dtype=torch.int32).to(device)
        self.max_n = max(max(ns), 1)
        self.vmax = max([float(v.abs().max()) for _, v in self.f64 if v.numel()] or [1.0])

    def words(self, torch, seed, chain=False):
        """[T] int64: garbage for the sequences with more than 64 tokens and for the tail; the others draw_words' patterns, or the chain"""
        g = torch.Generator().manual_seed(seed)
        w = torch.randint(-2 ** 63, 2 ** 63 - 1, (self.T,), generator=g, dtype=torch.int64)
        for b, (n, _) in enumerate(self.nl):
            if 0 < n <= 64:
                w[self.starts[b]:self.starts[b] + n] = chain_words(torch, n) if chain else draw_words(torch, seed + b, 4, n)[b % 3]
        return w

    def run(self, words):
        import aule
        return aule.flash_attention_paged_prefill_tree(self.q, self.kc, self.vc, words, self.bt, self.cl, self.cu, max_seqlen_q=self.max_n,
                                                       scale=self.scale, return_lse=True, **self.scales)

    def twin(self):
        import aule
        return aule.flash_attention_paged_prefill(self.q, self.kc, self.vc, self.bt, self.cl, self.cu, max_seqlen_q=self.max_n,
                                                  scale=self.scale, return_lse=True, **self.scales)

    def judge(self, torch, words, causal=False):
        """[owned, Hq, D], [owned, Hq]: a sequence with more than 64 tokens under the causal rule (causal: every sequence)"""
        outs, lses = [], []
        for b, (n, L) in enumerate(self.nl):
            K, V = (x.to(self.q.device) for x in self.f64[b])
            s = self.starts[b]
            vis = visibility(torch, L, n, words[s:s + n], causal=causal or n > 64)
            o, l = judge(torch, self.q[s:s + n].double(), K, V, vis, 1.0 / math.sqrt(self.D) if self.scale is None else self.scale)
            outs.append(o)
            lses.append(l)
        return torch.cat(outs), torch.cat(lses)


def prefill_desc(torch, p, words, out, lse):
    from aule import _capi
    d = _capi.PagedPrefillTreeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[p.q.dtype]
    d.cache_dtype = 1 if p.scales else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = p.bt.shape[0], p.Hq, p.kc.shape[2], p.D
    d.block_size, d.max_blocks = p.kc.shape[1], p.bt.shape[1]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = p.T, p.max_n, p.q.stride(0)
    d.scale, d.window_size, d.device = 0.0 if p.scale is None else p.scale, -1, p.q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = p.q.data_ptr(), p.kc.data_ptr(), p.vc.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.block_tables, d.context_lens, d.cu_seqlens_q = p.bt.data_ptr(), p.cl.data_ptr(), p.cu.data_ptr()
    d.tree_mask = words.data_ptr() if words is not None else None
    if p.scales:
        d.k_scale, d.v_scale = p.scales["k_scale"].data_ptr(), p.scales["v_scale"].data_ptr()
    return d


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


@pytest.mark.parametrize("kind", KINDS)
def test_prefill_tree_mixed_batch_against_the_judge_through_the_c_abi(kind):
    """aule_attention_paged_prefill_tree_ex with the descriptor filled by hand, into poisoned out / lse: n = 100 (causal, garbage words),
    64 (two blocks), 7, 1, 0 and one sequence with L < n; the rows no sequence owns keep their bits; the Python entry gives the same bits;
    the long sequence equals the plain entry bit for bit; refusals are -3 with their text."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    dtype = "bf16" if kind == "16" else "fp16"
    p = PrefillProblem(torch, 31, dtype, kind)
    assert all((L - n) % 64 for n, L in p.nl) and any(L < n <= 64 for n, L in p.nl)
    words = p.words(torch, 5)
    words_are_not_trivial([words[p.starts[b]:p.starts[b] + n] for b, (n, _) in enumerate(p.nl) if 0 < n <= 64])
    words = words.cuda()
    poison = torch.randn(p.T, p.Hq, p.D, generator=torch.Generator().manual_seed(1)).to(p.q.dtype).cuda()
    out, lse = poison.clone(), torch.full((p.T, p.Hq), 7.25, device="cuda")
    assert lib.aule_attention_paged_prefill_tree_ex(ctypes.byref(prefill_desc(torch, p, words, out, lse))) == 0, _error(lib)
    torch.cuda.synchronize()
    assert torch.equal(out[p.owned:], poison[p.owned:]) and bool((lse[p.owned:] == 7.25).all()), "rows that no sequence owns were written"
    ref, lref = p.judge(torch, words)
    compare(torch, out[:p.owned], lse[:p.owned], ref, lref, dtype, p.vmax, "prefill tree, %s cache" % kind)
    assert bool(torch.isneginf(lref).any())
    # the Python entry: the same launch
    o2, l2 = p.run(words)
    assert torch.equal(o2[:p.owned], out[:p.owned]) and torch.equal(l2[:p.owned], lse[:p.owned])
    # the sequence with more than 64 tokens: the plain entry's bits, whatever its words hold
    ot, lt = p.twin()
    n0 = p.nl[0][0]
    assert n0 > 64 and torch.equal(o2[:n0], ot[:n0]) and torch.equal(l2[:n0], lt[:n0])
    assert not torch.equal(o2[n0:p.owned], ot[n0:p.owned])              # (and the trees are not the chain)

    def refused(change, needle):
        d = prefill_desc(torch, p, words, out, None)
        change(d)
        assert lib.aule_attention_paged_prefill_tree_ex(ctypes.byref(d)) == -3
        assert "Paged prefill tree attention failed" in _error(lib) and needle in _error(lib), _error(lib)

    refused(lambda d: setattr(d, "tree_mask", None), "null tree_mask pointer")
    refused(lambda d: setattr(d, "window_size", 8), "window is not defined over a tree")
    refused(lambda d: setattr(d, "struct_size", 152), "struct_size")
    refused(lambda d: setattr(d, "head_dim", 256), "head_dim 256")
    refused(lambda d: setattr(d, "cu_seqlens_q", None), "null tensor pointer")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Sq", [13, 64])
def test_query_chain_words_are_the_twin_bit_for_bit(kind, Sq):
    import torch
    p = QueryProblem(torch, 200 + Sq, "bf16" if kind == "16" else "fp16", kind, 8, 2, Sq, 128, 16, query_lens(Sq) + [31, 32, 33, 2048])
    words = chain_words(torch, Sq).repeat(len(p.lens), 1).contiguous().cuda()
    out, lse = p.run(words)
    tout, tlse = p.twin()
    assert torch.equal(out, tout) and torch.equal(lse, tlse)
    assert bool(torch.isfinite(lse).any()) and bool(torch.isneginf(lse).any())
    # ... and a tree is not: the entry reads its words
    w2 = words.clone()
    w2[:, -1] = 1
    if Sq > 1:
        assert not torch.equal(p.run(w2)[0], tout)


@pytest.mark.parametrize("kind", KINDS)
def test_prefill_chain_words_are_the_twin_bit_for_bit(kind):
    """the mixed batch with chain words for every sequence: out and lse of flash_attention_paged_prefill over the owned rows"""
    import torch
    for dtype, D, bs in (("bf16", 64, 16), ("fp16", 128, 24)):
        p = PrefillProblem(torch, 33, dtype, kind, D=D, bs=bs)
        words = p.words(torch, 9, chain=True).cuda()
        out, lse = p.run(words)
        tout, tlse = p.twin()
        assert torch.equal(out[:p.owned], tout[:p.owned]) and torch.equal(lse[:p.owned], tlse[:p.owned]), (dtype, D, bs)
        assert bool(torch.isneginf(lse[:p.owned]).any())


@pytest.mark.parametrize("kind", KINDS)
def test_query_tree_and_prefill_tree_agree(kind):
    """the same uniform problem through the two kernels, each with its own rounding: within 2 x fwd_tol"""
    import torch
    import aule
    Sq, dtype = 13, "bf16"
    p = QueryProblem(torch, 300, dtype, kind, 8, 2, Sq, 128, 16, [45, 100, 257, 1000])
    words = draw_words(torch, 17, len(p.lens), Sq).cuda()
    out, lse = p.run(words)
    B, Hq, _, D = p.q.shape
    cu = (torch.arange(B + 1, dtype=torch.int32) * Sq).cuda()
    o2, l2 = aule.flash_attention_paged_prefill_tree(p.q.permute(0, 2, 1, 3).reshape(B * Sq, Hq, D).contiguous(), p.kc, p.vc, words.reshape(-1),
                                                     p.bt, p.cl, cu, max_seqlen_q=Sq, return_lse=True, **p.scales)
    o2, l2 = o2.view(B, Sq, Hq, D).permute(0, 2, 1, 3), l2.view(B, Sq, Hq).permute(0, 2, 1)
    compare(torch, out, lse, o2.double(), l2.double(), dtype, p.vmax, "query tree vs prefill tree, %s cache" % kind, factor=2.0)


def _paths(parents):
    """root-to-leaf paths of the tree, as lists of node indices"""
    n = len(parents)
    par = [p if 0 <= p < i else -1 for i, p in enumerate(parents)]
    leaves = [i for i in range(n) if i not in par]
    paths = []
    for leaf in leaves:
        path, j = [], leaf
        while j >= 0:
            path.append(j)
            j = par[j]
        paths.append(path[::-1])
    return paths


@pytest.mark.parametrize("kind", KINDS)
def test_every_path_of_a_tree_is_the_plain_query_on_that_path(kind):
    """the user-level meaning: for a random 16-node tree, the rows of every root-to-leaf path equal flash_attention_paged_query on a cache
    in which that path's tokens lie consecutively behind the context.  Two kernels' roundings: 2 x fwd_tol, LSE 2e-3."""
    import torch
    import aule
    n, C, Hq, Hkv, D, bs, dtype = 16, 83, 8, 2, 128, 16, "bf16"
    g = torch.Generator().manual_seed(41)
    parents = random_parents(torch, g, n)
    paths = _paths(parents.tolist())
    assert len(paths) >= 3 and max(len(x) for x in paths) >= 3 and len({len(x) for x in paths}) >= 2, paths
    words = aule.tree_mask_from_parents(parents)
    dev, f64, scales = make_kv(torch, g, dtype, kind, [C + n], Hkv, D)
    kc, vc, bt = paginate(torch, g, dev, bs)
    kc, vc, sc = to_device(torch, kc, vc, scales)
    q = ((0.25 if kind == "fp8" else 1.0) * torch.randn(1, Hq, n, D, generator=g)).to(torch_dtype(dtype)).cuda()
    out, lse = aule.flash_attention_paged_query_tree(q, kc, vc, words.view(1, n).cuda(), bt.cuda(), torch.tensor([C + n], dtype=torch.int32).cuda(),
                                                     return_lse=True, **sc)
    vmax = float(f64[0][1].abs().max())
    # one call per path length: the paths of that length as a batch, each with its own pages behind a copy of the context
    for length in sorted({len(x) for x in paths}):
        group = [x for x in paths if len(x) == length]
        rows = [torch.tensor(list(range(C)) + [C + j for j in path]) for path in group]
        pdev = [(dev[0][0][r], dev[0][1][r]) for r in rows]
        pk, pv, pbt = paginate(torch, g, pdev, bs)
        pk, pv, _ = to_device(torch, pk, pv, scales)
        idx = torch.tensor(group).cuda()                                          # [paths, length]
        pq = q[0][:, idx].permute(1, 0, 2, 3).contiguous()                        # [paths, Hq, length, D]
        po, pl = aule.flash_attention_paged_query(pq, pk, pv, pbt.cuda(), torch.full((len(group),), C + length, dtype=torch.int32).cuda(),
                                                  return_lse=True, **sc)
        got_o = out[0][:, idx].permute(1, 0, 2, 3)
        got_l = lse[0][:, idx].permute(1, 0, 2)
        compare(torch, got_o, got_l, po.double(), pl.double(), dtype, vmax, "paths of %d nodes, %s cache" % (length, kind), factor=2.0, lse_atol=2e-3)


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
        res = fn()
    return g, res


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_read_the_current_words(kind):
    """each entry captured once; tree_mask -- and for the prefill entry cu_seqlens_q -- overwritten between replays: every replay equals the
    eager call on the same contents bit for bit"""
    import torch
    Sq = 13
    p = QueryProblem(torch, 400, "fp16", kind, 8, 2, Sq, 64, 16, [45, 100, 257, 1000])
    words = draw_words(torch, 21, 4, Sq).cuda()
    g, (out, lse) = _capture(torch, lambda: p.run(words))
    for seed in (22, 23):
        new = draw_words(torch, seed, 4, Sq).cuda()
        want, want_lse = p.run(new)
        words.copy_(new)
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(lse, want_lse), seed
    assert not torch.equal(want, p.run(draw_words(torch, 21, 4, Sq).cuda())[0])

    pp = PrefillProblem(torch, 401, "fp16", kind, tail=40)
    w = pp.words(torch, 24).cuda()
    g, (out, lse) = _capture(torch, lambda: pp.run(w))
    ns = [n for n, _ in pp.nl]
    for seed, shift in ((25, 0), (26, 3), (27, 40)):
        # new words, and the sequences moved `shift` rows up the packed axis (the tail makes room)
        new = pp.words(torch, seed)
        new_cu = torch.tensor([s + shift for s in pp.starts], dtype=torch.int32).cuda()
        new = torch.cat([new[pp.owned:pp.owned + shift], new[:pp.owned], new[pp.owned + shift:]]).cuda() if shift else new.cuda()
        keep = pp.cu.clone()
        pp.cu.copy_(new_cu)
        want, want_lse = pp.run(new)
        torch.cuda.synchronize()
        w.copy_(new)
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        rows = slice(shift, shift + sum(ns))
        assert torch.equal(out[rows], want[rows]) and torch.equal(lse[rows], want_lse[rows]), (seed, shift)
        assert bool(torch.isfinite(lse[rows]).any())
        pp.cu.copy_(keep)


def _query_desc(torch, p, words, out, lse):
    from aule import _capi
    B, Hq, Sq, D = p.q.shape
    d = _capi.PagedQueryTreeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[p.q.dtype]
    d.cache_dtype = 1 if p.scales else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim, d.seq_q = B, Hq, p.kc.shape[2], D, Sq
    d.block_size, d.max_blocks = p.kc.shape[1], p.bt.shape[1]
    d.scale, d.window_size, d.device = 0.0, -1, p.q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = p.q.data_ptr(), p.kc.data_ptr(), p.vc.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.block_tables, d.context_lens = p.bt.data_ptr(), p.cl.data_ptr()
    d.tree_mask = words.data_ptr() if words is not None else None
    if p.scales:
        d.k_scale, d.v_scale = p.scales["k_scale"].data_ptr(), p.scales["v_scale"].data_ptr()
    return d


@pytest.mark.parametrize("kind", KINDS)
def test_query_tree_c_abi_directly(kind):
    """aule_attention_paged_query_tree_ex with a caller workspace of exactly the queried size and with none (equal results, nothing
    written past the buffer, right against the judge), with and without lse; -3 and an error text for what is refused."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    Sq, dtype = 6, "bf16"
    p = QueryProblem(torch, 500, dtype, kind, 16, 4, Sq, 128, 16, [900, 33, 2048])
    words = draw_words(torch, 29, 3, Sq).cuda()
    B, Hq = p.q.shape[:2]
    res = []
    for mode in ("exact", "none", "no-lse"):
        out = torch.empty_like(p.q)
        lse = torch.full((B, Hq, Sq), 7.0, device="cuda") if mode != "no-lse" else None
        d = _query_desc(torch, p, words, out, lse)
        need = int(lib.aule_attention_paged_query_tree_workspace_size(ctypes.byref(d)))
        assert need > 0
        buf = torch.full((need + 4096,), 0x5A, device="cuda", dtype=torch.uint8)
        if mode != "none":
            d.workspace, d.workspace_bytes = buf.data_ptr(), need
        assert lib.aule_attention_paged_query_tree_ex(ctypes.byref(d)) == 0, _error(lib)
        torch.cuda.synchronize()
        assert bool((buf[need:] == 0x5A).all()), "wrote past the workspace it was given"
        if mode != "none":
            assert not bool((buf[:need] == 0x5A).all()), "did not use the workspace it was given"
        res.append((out, lse))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[1][1])
    ref, lref = p.judge(torch, words)
    compare(torch, res[0][0], res[0][1], ref, lref, dtype, p.vmax, "query tree through the C-ABI, %s cache" % kind)

    def refused(change, needle):
        d = _query_desc(torch, p, words, torch.empty_like(p.q), None)
        change(d)
        assert lib.aule_attention_paged_query_tree_ex(ctypes.byref(d)) == -3
        assert "Paged query tree attention failed" in _error(lib) and needle in _error(lib), _error(lib)

    refused(lambda d: setattr(d, "tree_mask", None), "null tree_mask pointer")
    refused(lambda d: setattr(d, "window_size", 4), "window is not defined over a tree")
    refused(lambda d: setattr(d, "struct_size", 152), "struct_size")
    refused(lambda d: setattr(d, "seq_q", 65), "seq_q 65")
    refused(lambda d: setattr(d, "heads_kv", 5), "divisible")
    refused(lambda d: setattr(d, "q", None), "null tensor pointer")
