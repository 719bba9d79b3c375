"""Tree masks over the latent cache on the GPU (csrc/fa_fwd_mla_verify_gfx950.hip behind aule.flash_attention_mla_paged_tree /
aule_attention_mla_paged_tree_ex): the verify step of tree drafters for the MLA models, both cache kinds.

The judge is written here, as in tests/test_gpu_tree.py: a torch float64 softmax over each sequence's latent rows (keys: all 576
elements, values: the first 512) with the boolean visibility matrix of the rule -- context keys and the bits of the token's word for a
sequence with at most 64 new tokens, the causal rule for a longer one.  An FP8 cache is judged on kv_scale * float(code) exactly.  The
bounds are the project's own: fwd_tol(dtype, max |V|) for out (max |dequantised V| for FP8), LSE_ATOL = 1e-3 for lse, as
tests/test_gpu_mla.py and tests/test_gpu_mla_fp8.py hold the same arithmetic to; rows without a key are exactly zeros and -inf.
Every case checks on the CPU that its visibility differs from the causal chain's, and prints the maxima it achieved.

Shapes are the smallest at which the kernel takes each of its paths: 16 / 24 / 128 heads (four tokens per 64-row block, a block
boundary inside a token, a token over two blocks), n in {1, 5, 33, 64, 65}, L < n, the new tokens at a tile start, inside a tile and
across a tile boundary ((L - n) mod 64 in {0, 40, 63}), block sizes 16, 48 and 64 with shuffled tables, one launch and key-range
splits (asserted through aule_hip_debug_mla_plan), a split without a tile."""
import ctypes
import math

import pytest

from hostile import POISON, Arena
from test_gpu_tree import LSE_ATOL, _capture, _paths, chain_words, compare, random_parents, visibility
from util import fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

QK, VD = 576, 512
DTYPE_CODE = {"fp16": 1, "bf16": 2}
KINDS = ["16", "fp8"]
WORD_KINDS = ("tree", "random", "zeros", "ones", "self", "chain")


def words_of(torch, g, kind, n):
    """[n] int64 on the CPU: a random tree, uniform random bits, nothing, everything, the self bit alone, or the chain"""
    import aule
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    if n > 64:                               # (a chunk: the words are not read; all ones shows that)
        return torch.full((n,), -1, dtype=torch.int64)
    if kind == "tree":
        return aule.tree_mask_from_parents(random_parents(torch, g, n))
    if kind == "random":
        return torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
    if kind == "zeros":
        return torch.zeros(n, dtype=torch.int64)
    if kind == "ones":
        return torch.full((n,), -1, dtype=torch.int64)
    if kind == "self":
        return chain_words(torch, n) ^ torch.cat([torch.zeros(1, dtype=torch.int64), chain_words(torch, n)[:-1]])
    assert kind == "chain", kind
    return chain_words(torch, n)


def causal_vis(torch, L, n):
    """[n, L] bool of the twin's rule: j <= L - n + i"""
    return visibility(torch, L, n, torch.zeros(n, dtype=torch.int64), causal=True)


def visible(torch, L, n, words):
    """[n, L] bool of the rule: the words for n <= 64, the causal chain for a longer sequence"""
    return visibility(torch, L, n, words, causal=n > 64)


def judge(torch, q, lat, vis, scale):
    """q [n, Hq, 576], lat [L, 576] float64, vis [n, L] -> out [n, Hq, 512], lse [n, Hq] (zeros and -inf for a row without a key)"""
    n, Hq, _ = q.shape
    L = lat.shape[0]
    out = torch.zeros(n, Hq, VD, dtype=torch.float64, device=q.device)
    lse = torch.full((n, Hq), -math.inf, dtype=torch.float64, device=q.device)
    if L == 0 or n == 0:
        return out, lse
    s = torch.einsum("nhd,ld->nhl", q, lat) * scale
    s = s.masked_fill(~vis[:, None, :], -math.inf)
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    z = p.sum(dim=-1, keepdim=True)
    o = torch.einsum("nhl,lv->nhv", p / torch.where(z > 0, z, torch.ones_like(z)), lat[:, :VD])
    some = vis.any(dim=1)
    out[some], lse[some] = o[some], (m + torch.log(z)).squeeze(-1)[some]
    return out, lse


class Problem:
    """Seeded inputs of one case.  seqs: [(L, n, word kind)] -- L keys in the cache INCLUDING the n new tokens.  The latent rows are
    scattered into shuffled pages (`cap`: keys of table capacity, default the longest sequence's blocks); rows of a page behind a
    sequence and the pages no table names hold finite junk, or NaN (nan_junk).  lead / tail: rows of no sequence around the packed
    tokens.  latents: the sequences' rows [L, 576] (float) instead of drawn ones; q: the packed queries; kv_scale: an FP8 cache's scale
    (default: the largest |element| of the sequences / 448)."""

    def __init__(self, torch, seed, dtype, kind, Hq, bs, seqs, cap=None, lead=0, tail=0, latents=None, nan_junk=False, q=None, kv_scale=None):
        g = torch.Generator().manual_seed(seed)
        self.torch, self.dtype, self.kind, self.Hq, self.bs, self.seqs = torch, dtype, kind, Hq, bs, seqs
        dt = torch_dtype(dtype)
        self.B = len(seqs)
        self.Ls, self.ns = [s[0] for s in seqs], [s[1] for s in seqs]
        lat = latents if latents is not None else [torch.randn(L, QK, generator=g) for L in self.Ls]
        nblk = [(L + bs - 1) // bs for L in self.Ls]
        cols = max(max(nblk) if cap is None else (cap + bs - 1) // bs, 1)
        assert cols >= max(nblk)
        num_blocks = sum(nblk) + 3
        pages = torch.randn(num_blocks, bs, QK, generator=g)
        if nan_junk:
            pages.fill_(math.nan)
        bt = torch.zeros(self.B, cols, dtype=torch.int32)
        perm = torch.randperm(num_blocks, generator=g)
        used, rows = 0, []
        for b in range(self.B):
            blocks = perm[used:used + nblk[b]]
            used += nblk[b]
            bt[b, :nblk[b]] = blocks.int()
            j = torch.arange(self.Ls[b])
            rows.append(blocks[j // bs] * bs + j % bs if self.Ls[b] else j)
            pages.view(-1, QK)[rows[-1]] = lat[b].float()
        self.kv_scale = None
        if kind == "fp8":
            amax = max([float(x.abs().max()) for x in lat if x.numel()] + [1e-6])
            self.kv_scale = torch.tensor([amax / 448.0], dtype=torch.float32) if kv_scale is None else kv_scale
            cache = (pages / self.kv_scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
            exact = cache.double() * self.kv_scale.double()
        else:
            cache = pages.to(dt)
            exact = cache.double()
        self.f64 = [exact.view(-1, QK)[r] for r in rows]                      # what the judge sees: [L, 576] float64 per sequence
        self.vmax = max([float(x[:, :VD].abs().max()) for x in self.f64 if x.numel()] + [0.0])
        self.starts = [lead + sum(self.ns[:b]) for b in range(self.B + 1)]
        self.T = self.starts[-1] + tail
        self.max_sq = max(self.ns + [1])
        self.q = (torch.randn(self.T, Hq, QK, generator=g) if q is None else q).to(dt).cuda()
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (self.T,), generator=g, dtype=torch.int64)      # rows of no sequence: anything
        for b, (L, n, wk) in enumerate(seqs):
            words[self.starts[b]:self.starts[b] + n] = words_of(torch, g, wk, n)
        self.words_cpu = words
        self.words = words.cuda()
        self.kv, self.bt = cache.cuda(), bt.cuda()
        self.cl = torch.tensor(self.Ls, dtype=torch.int32).cuda()
        self.cu = torch.tensor(self.starts, dtype=torch.int32).cuda()
        self.kvs = self.kv_scale.cuda() if self.kv_scale is not None else None
        self.owned = torch.zeros(self.T, dtype=torch.bool)
        for b in range(self.B):
            self.owned[self.starts[b]:self.starts[b] + self.ns[b]] = True
        self.owned = self.owned.cuda()

    def vis(self, words=None):
        """the sequences' visibility matrices on the CPU (words: [T] int64, default the problem's own)"""
        words = self.words_cpu if words is None else words.cpu()
        return [visible(self.torch, L, n, words[s:s + n]) for (L, n, _), s in zip(self.seqs, self.starts)]

    def differs_from_the_chain(self, words=None):
        return any(bool((v != causal_vis(self.torch, L, n)).any()) for v, (L, n, _) in zip(self.vis(words), self.seqs))

    def rows_without_a_key(self, words=None):
        return sum(int((~v.any(dim=1)).sum()) for v in self.vis(words))

    def kw(self):
        return dict(kv_scale=self.kvs) if self.kind == "fp8" else {}

    def run(self, words=None, cl=None, cu=None, q=None, max_sq=None):
        import aule
        return aule.flash_attention_mla_paged_tree(self.q if q is None else q, self.kv, self.words if words is None else words, self.bt,
                                                   self.cl if cl is None else cl, self.cu if cu is None else cu,
                                                   max_seqlen_q=max_sq or self.max_sq, return_lse=True, **self.kw())

    def twin(self):
        import aule
        f = aule.flash_attention_mla_paged_fp8 if self.kind == "fp8" else aule.flash_attention_mla_paged
        return f(self.q, self.kv, self.bt, self.cl, self.cu, max_seqlen_q=self.max_sq, return_lse=True, **self.kw())

    def judge(self, words=None):
        """(out [T, Hq, 512], lse [T, Hq]) float64 on the GPU; rows of no sequence: zeros and -inf, never compared"""
        torch = self.torch
        ref = torch.zeros(self.T, self.Hq, VD, dtype=torch.float64, device="cuda")
        lref = torch.full((self.T, self.Hq), -math.inf, dtype=torch.float64, device="cuda")
        for b, v in enumerate(self.vis(words)):
            s, n = self.starts[b], self.ns[b]
            ref[s:s + n], lref[s:s + n] = judge(torch, self.q[s:s + n].double(), self.f64[b].cuda(), v.cuda(), 1.0 / math.sqrt(QK))
        return ref, lref

    def check(self, out, lse, what, words=None):
        ref, lref = self.judge(words)
        own = self.owned
        compare(self.torch, out[own], lse[own], ref[own], lref[own], self.dtype, self.vmax, what)

    def nsplit(self):
        """the plan of the call's shape, from the hook (it reads no pointer and answers for every kind)"""
        from aule import _capi
        d = _capi.MlaPagedDesc()
        d.struct_size = ctypes.sizeof(d)
        d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = DTYPE_CODE[self.dtype], self.B, self.Hq, QK, VD
        d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = self.bs, self.bt.shape[1], self.T, self.max_sq
        d.q_token_stride, d.cu_seqlens_q = self.Hq * QK, 4096
        plan = (ctypes.c_int32 * 6)()
        assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(d), plan, 6) == 6
        return plan[2]


def tree_desc(torch, p, tensors, out, lse, ws=None):
    """the C descriptor of p's call; tensors: (q, kv, bt, cl, cu, words, kv_scale or None)"""
    from aule import _capi
    q, kv, bt, cl, cu, words, kvs = tensors
    d = _capi.MlaPagedTreeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = DTYPE_CODE[p.dtype], p.B, p.Hq, QK, VD
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q, d.q_token_stride = p.bs, bt.shape[1], p.T, p.max_sq, q.stride(0)
    d.device = torch.cuda.current_device()
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.kv_cache, d.block_tables, d.context_lens, d.cu_seqlens_q = q.data_ptr(), kv.data_ptr(), bt.data_ptr(), cl.data_ptr(), cu.data_ptr()
    d.out, d.lse, d.tree_mask = out.data_ptr(), lse.data_ptr(), words.data_ptr()
    d.cache_dtype = 1 if p.kind == "fp8" else 0
    d.kv_scale = kvs.data_ptr() if kvs is not None else None
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    return d


def _poisoned(torch, p):
    out = torch.full((p.T, p.Hq, VD), -1, dtype=torch.int16, device="cuda").view(torch_dtype(p.dtype))
    lse = torch.full((p.T, p.Hq), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    return out, lse


def _error(lib):
    msg = lib.aule_get_error()
    return msg.decode() if isinstance(msg, bytes) else str(msg)


# ---- the judge over the shapes at which the kernel takes each path
# name: (heads, block size, [(L, n, words)], capacity in keys, key-range splits expected)
SHAPES = {
    # four tokens per row block; new tokens inside a tile (L - n = 40), at a tile start (64), L < n, across a tile's edge (63)
    "h16-bs16": (16, 16, [(45, 5, "tree"), (97, 33, "random"), (3, 5, "ones"), (64, 1, "self"), (1, 1, "zeros")], 112, False),
    # a token spans two row blocks; the full word; L - n = 63 and 40
    "h128-bs64": (128, 64, [(127, 64, "tree"), (104, 64, "random")], 128, False),
    # a block boundary inside a token; a block size that is no power of two; L - n = 64, 40, 63
    "h24-bs48": (24, 48, [(69, 5, "tree"), (73, 33, "zeros"), (96, 33, "random")], 96, False),
    # one sequence, 512 keys of capacity, four key ranges of which the new tokens lie in the last that owns a tile; the first are context
    "split-h16": (16, 64, [(300, 33, "tree")], 512, True),
    # so short that the last two of four ranges own no tile
    "split-short-h128": (128, 16, [(70, 5, "random")], 512, True),
    "split-h24-bs48": (24, 48, [(300, 64, "tree"), (167, 5, "self")], 528, True),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tree_against_the_judge(shape, dtype, kind):
    import torch
    Hq, bs, seqs, cap, split = SHAPES[shape]
    p = Problem(torch, 100 + sorted(SHAPES).index(shape), dtype, kind, Hq, bs, seqs, cap=cap)
    assert p.differs_from_the_chain()
    ns = p.nsplit()
    assert (ns > 1) == split, ns
    if shape == "split-h16":
        # four ranges of two tiles: keys 0 .. 255 are pure context, the new tokens (267 ..) lie in the third, the fourth owns no tile
        assert ns == 4 and p.Ls[0] - p.ns[0] >= 256
    if shape == "split-short-h128":
        assert ns == 4 and (p.Ls[0] + 63) // 64 == 2
    out, lse = p.run()
    torch.cuda.synchronize()
    assert out.shape == (p.T, Hq, VD) and out.dtype == torch_dtype(dtype) and lse.shape == (p.T, Hq) and lse.dtype == torch.float32
    p.check(out, lse, "tree %s %s %s cache, nsplit %d" % (shape, dtype, kind, ns))
    out2, lse2 = p.run()
    assert torch.equal(out2, out) and torch.equal(lse2, lse)


@pytest.mark.parametrize("kind", KINDS)
def test_mixed_batch_through_the_c_abi_into_poisoned_buffers(kind):
    """a tree, a decode, a 65-token chunk whose words are all ones (ignored: it stays causal) and an empty sequence in one call, through
    aule_attention_mla_paged_tree_ex; rows of no sequence keep their bytes"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Problem(torch, 200, "bf16", kind, 24, 16, [(45, 5, "tree"), (130, 1, "ones"), (150, 65, "ones"), (40, 0, "zeros")], lead=2, tail=3)
    assert p.differs_from_the_chain() and bool((p.words_cpu[p.starts[2]:p.starts[3]] == -1).all())
    chunk = p.vis()[2]
    assert torch.equal(chunk, causal_vis(torch, 150, 65)) and not bool(chunk.all())
    out, lse = _poisoned(torch, p)
    d = tree_desc(torch, p, (p.q, p.kv, p.bt, p.cl, p.cu, p.words, p.kvs), out, lse)
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == 0, _error(lib)
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16)[~p.owned] == -1).all()) and bool((lse.view(torch.int32)[~p.owned] == -1).all())
    p.check(out, lse, "mixed batch, %s cache, C entry" % kind)
    want, want_lse = p.run()
    assert torch.equal(out[p.owned], want[p.owned]) and torch.equal(lse[p.owned], want_lse[p.owned])
    # the size query is the twin's, and a caller workspace of that size is used
    assert lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d)) == 0 and p.nsplit() == 1

    def refused(change, needle):
        x = tree_desc(torch, p, (p.q, p.kv, p.bt, p.cl, p.cu, p.words, p.kvs), out, lse)
        change(x)
        assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(x)) == -3 and needle in _error(lib), _error(lib)

    refused(lambda x: setattr(x, "tree_mask", None), "null tree_mask")
    refused(lambda x: setattr(x, "cu_seqlens_q", None), "null cu_seqlens_q")
    refused(lambda x: setattr(x, "cache_dtype", 2), "cache_dtype 2")
    refused(lambda x: setattr(x, "tree_mask", p.words.data_ptr() + 4), "8-byte aligned")


@pytest.mark.parametrize("kind", KINDS)
def test_the_mask_decides(kind):
    """node 3 is a child of node 1 and must not see node 2, its parent's sibling, whose latent row is 100 x the others.  The rows that do
    not see node 2 are judged with max |V| of the keys they see; the twin's (causal) answer for node 3 misses that bound by orders of
    magnitude, so a kernel that ignored the word would too."""
    import torch
    import aule
    C, n, Hq = 40, 5, 16
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(C + n, QK, generator=g)
    lat[C + 2] *= 100.0
    words = aule.tree_mask_from_parents(torch.tensor([-1, 0, 0, 1, 2]))
    p = Problem(torch, 300, "bf16", kind, Hq, 16, [(C + n, n, "zeros")], latents=[lat])
    v = visible(torch, C + n, n, words)
    assert not bool(v[3, C + 2]) and bool(v[4, C + 2]) and bool(v[2, C + 2]) and bool(causal_vis(torch, C + n, n)[3, C + 2])
    out, lse = p.run(words.cuda())
    ref, lref = p.judge(words)
    rows = torch.tensor([0, 1, 3]).cuda()                       # the rows that do not see the large key
    small = torch.ones(C + n, dtype=torch.bool)
    small[C + 2] = False
    vmax = float(p.f64[0][small][:, :VD].abs().max())
    assert float(p.f64[0][C + 2, :VD].abs().max()) > 30 * vmax
    compare(torch, out[rows], lse[rows], ref[rows], lref[rows], "bf16", vmax, "decisive mask, %s cache" % kind)
    tw, _ = p.twin()
    atol, rtol = fwd_tol("bf16", vmax)
    miss = float(((tw[3].double() - ref[3]).abs() - (atol + rtol * ref[3].abs())).max())
    print("the causal twin misses node 3's bound by %.3g (atol %.3g)" % (miss, atol))
    assert miss > 100 * atol


# ---- exact properties

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["h24-bs48", "h128-bs64", "split-h16", "split-h24-bs48"])
def test_chain_words_are_the_twin_bit_for_bit(shape, kind):
    import torch
    Hq, bs, seqs, cap, split = SHAPES[shape]
    p = Problem(torch, 400, "fp16", kind, Hq, bs, [(L, n, "chain") for L, n, _ in seqs], cap=cap)
    assert (p.nsplit() > 1) == split and not p.differs_from_the_chain()
    out, lse = p.run()
    tw, tw_lse = p.twin()
    assert bool(torch.isfinite(lse).all())
    assert torch.equal(out, tw) and torch.equal(lse, tw_lse)


def test_fp8_with_scale_one_is_the_16_bit_call_on_the_codes_bit_for_bit():
    import torch
    import aule
    for shape in ("h16-bs16", "split-h16"):
        Hq, bs, seqs, cap, _ = SHAPES[shape]
        p = Problem(torch, 410, "bf16", "fp8", Hq, bs, seqs, cap=cap)
        one = torch.ones(1, dtype=torch.float32, device="cuda")
        a, al = aule.flash_attention_mla_paged_tree(p.q, p.kv, p.words, p.bt, p.cl, p.cu, max_seqlen_q=p.max_sq, return_lse=True, kv_scale=one)
        b, bl = aule.flash_attention_mla_paged_tree(p.q, p.kv.to(torch.bfloat16), p.words, p.bt, p.cl, p.cu, max_seqlen_q=p.max_sq, return_lse=True)
        assert torch.equal(a, b) and torch.equal(al, bl), shape
        none, _ = aule.flash_attention_mla_paged_tree(p.q, p.kv, p.words, p.bt, p.cl, p.cu, max_seqlen_q=p.max_sq, return_lse=True)
        assert torch.equal(none, a)                                       # kv_scale = None is 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_a_sequence_alone_equals_the_same_sequence_in_a_batch(kind):
    """one launch either way (capacity of two tiles): every sequence of the batch as a call of its own, bit for bit"""
    import torch
    import aule
    Hq, bs, seqs, cap, _ = SHAPES["h16-bs16"]
    p = Problem(torch, 420, "bf16", kind, Hq, bs, seqs, cap=cap)
    assert p.nsplit() == 1
    out, lse = p.run()
    for b, (L, n, _) in enumerate(seqs):
        s = p.starts[b]
        cu = torch.tensor([0, n], dtype=torch.int32).cuda()
        o, l = aule.flash_attention_mla_paged_tree(p.q[s:s + n], p.kv, p.words[s:s + n].clone(), p.bt[b:b + 1], p.cl[b:b + 1], cu, max_seqlen_q=n,
                                                   return_lse=True, **p.kw())
        assert torch.equal(o, out[s:s + n]) and torch.equal(l, lse[s:s + n]), b


# ---- cross-checks: two kernels' roundings get 2 x fwd_tol and 2e-3 on lse, as tests/test_gpu_tree.py allows there

@pytest.mark.parametrize("kind", KINDS)
def test_the_same_tree_as_key_lists_through_the_sparse_call(kind):
    import torch
    import aule
    Hq, bs, seqs, cap, _ = SHAPES["split-h24-bs48"]
    p = Problem(torch, 500, "bf16", kind, Hq, bs, seqs, cap=cap)
    out, lse = p.run()
    vis = p.vis()
    topk = max(int(v.sum(dim=1).max()) for v in vis)
    idx = torch.full((p.T, topk), -1, dtype=torch.int32)
    bt = p.bt.cpu()
    for b, v in enumerate(vis):
        for i in range(p.ns[b]):
            j = torch.nonzero(v[i]).flatten()
            idx[p.starts[b] + i, :j.numel()] = bt[b][j // bs] * bs + (j % bs).int()
    so, sl = aule.flash_attention_mla_sparse(p.q, p.kv, idx.cuda(), return_lse=True, **p.kw())
    compare(torch, out, lse, so.double(), sl.double(), "bf16", p.vmax, "tree vs sparse lists, %s cache" % kind, factor=2.0, lse_atol=2e-3)


@pytest.mark.parametrize("kind", KINDS)
def test_every_path_of_a_tree_is_the_chain_call_on_that_path(kind):
    """the user-level meaning: the rows of every root-to-leaf path equal the plain MLA call on a cache in which that path's tokens lie
    consecutively behind the context -- the route there was before this entry"""
    import torch
    import aule
    n, C, Hq, bs = 16, 83, 16, 16
    g = torch.Generator().manual_seed(41)
    parents = random_parents(torch, g, n)
    paths = _paths(parents.tolist())
    assert len(paths) >= 3 and max(len(x) for x in paths) >= 3, paths
    words = aule.tree_mask_from_parents(parents)
    lat = torch.randn(C + n, QK, generator=g)
    p = Problem(torch, 510, "bf16", kind, Hq, bs, [(C + n, n, "zeros")], latents=[lat])
    assert p.differs_from_the_chain(words)
    out, lse = p.run(words.cuda())
    rows = [list(range(C)) + [C + j for j in path] for path in paths]
    q = torch.cat([p.q[torch.tensor(path).cuda()] for path in paths]).float().cpu()
    pp = Problem(torch, 511, "bf16", kind, Hq, bs, [(len(r), len(path), "chain") for r, path in zip(rows, paths)],
                 latents=[lat[torch.tensor(r)] for r in rows], q=q, kv_scale=p.kv_scale)    # (the same scale: the same codes)
    po, pl = pp.twin()
    at = torch.tensor([j for path in paths for j in path]).cuda()
    compare(torch, out[at], lse[at], po.double(), pl.double(), "bf16", p.vmax, "%d paths, %s cache" % (len(paths), kind), factor=2.0, lse_atol=2e-3)


# ---- robustness

@pytest.mark.parametrize("kind", KINDS)
def test_nan_behind_the_lengths_and_in_unnamed_blocks_changes_nothing(kind):
    import torch
    Hq, bs, seqs, cap, _ = SHAPES["split-h24-bs48"]
    a = Problem(torch, 600, "fp16", kind, Hq, bs, seqs, cap=cap)
    b = Problem(torch, 600, "fp16", kind, Hq, bs, seqs, cap=cap, nan_junk=True)
    assert bool(torch.isnan(b.kv.float()).any()) and not bool(torch.isnan(a.kv.float()).any()) and torch.equal(a.bt, b.bt)
    out, lse = a.run()
    nout, nlse = b.run()
    assert bool(torch.isfinite(nout).all()) and torch.equal(nout, out) and torch.equal(nlse, lse)


@pytest.mark.parametrize("kind", KINDS)
def test_inside_an_arena_with_stale_lengths_and_offsets(kind):
    """every tensor of the call between guard bands of one allocation, outputs and workspace poisoned; context_lens beyond the table's
    capacity and a last offset beyond total_tokens are clamped: the call equals the one with the clamped values bit for bit, the guards
    stay intact and the inputs unchanged"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Problem(torch, 700, "bf16", kind, 24, 64, [(300, 33, "tree"), (130, 5, "random")], cap=512)
    cap = p.bt.shape[1] * p.bs
    clamped_cl = torch.tensor([cap, 130], dtype=torch.int32).cuda()
    want, want_lse = p.run(cl=clamped_cl)
    stale_cl = torch.tensor([cap + 1000, 130], dtype=torch.int32)
    stale_cu = torch.tensor([0, 33, p.T + 100], dtype=torch.int32)
    probe_out, probe_lse = _poisoned(torch, p)
    d0 = tree_desc(torch, p, (p.q, p.kv, p.bt, p.cl, p.cu, p.words, p.kvs), probe_out, probe_lse)
    size = int(lib.aule_attention_mla_paged_tree_workspace_size(ctypes.byref(d0)))
    assert size > 0 and p.nsplit() > 1
    host = dict(q=p.q.cpu(), kv=p.kv.cpu().view(torch.uint8) if kind == "fp8" else p.kv.cpu(), bt=p.bt.cpu(), cl=stale_cl, cu=stale_cu,
                words=p.words_cpu)
    if kind == "fp8":
        host["kvs"] = p.kv_scale
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in host.items()]
    regions += [("out", p.T * p.Hq * VD * 2, "out"), ("lse", p.T * p.Hq * 4, "out"), ("ws", size, "ws")]
    arena = Arena(torch, regions, QK * 2)
    kept = {k: arena.upload(k, v) for k, v in host.items()}
    arena.fill(POISON)
    dt = torch_dtype(p.dtype)
    tensors = (arena.view("q", dt, p.q.shape), arena.view("kv", p.kv.dtype, p.kv.shape), arena.view("bt", torch.int32, p.bt.shape),
               arena.view("cl", torch.int32, (2,)), arena.view("cu", torch.int32, (3,)), arena.view("words", torch.int64, (p.T,)),
               arena.view("kvs", torch.float32, (1,)) if kind == "fp8" else None)
    out, lse = arena.view("out", dt, (p.T, p.Hq, VD)), arena.view("lse", torch.float32, (p.T, p.Hq))
    d = tree_desc(torch, p, tensors, out, lse, arena.bytes("ws"))
    assert lib.aule_attention_mla_paged_tree_ex(ctypes.byref(d)) == 0, _error(lib)
    torch.cuda.synchronize()
    assert arena.guards_intact(), arena.damage()
    for k, v in kept.items():
        assert arena.unchanged(k, v), k
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_read_the_current_words_and_offsets(kind):
    """one capture on one stream (max_seqlen_q given: no synchronisation); the words and cu_seqlens_q overwritten in place between
    replays: every replay equals the eager call on the same contents bit for bit"""
    import torch
    p = Problem(torch, 800, "fp16", kind, 16, 64, [(300, 33, "tree"), (200, 5, "random")], cap=512, tail=12)
    assert p.nsplit() > 1
    words, cu = p.words.clone(), p.cu.clone()
    g, (out, lse) = _capture(torch, lambda: p.run(words, cu=cu))
    first = None
    for seed, shift in ((1, 0), (2, 3), (3, 12)):
        gen = torch.Generator().manual_seed(seed)
        new = torch.cat([torch.zeros(shift, dtype=torch.int64), words_of(torch, gen, "tree", 33), words_of(torch, gen, "random", 5),
                         torch.zeros(12 - shift, dtype=torch.int64)]).cuda()
        new_cu = (p.cu + shift).clone()
        want, want_lse = p.run(new, cu=new_cu)
        torch.cuda.synchronize()
        words.copy_(new)
        cu.copy_(new_cu)
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        rows = slice(shift, shift + 38)
        assert torch.equal(out[rows], want[rows]) and torch.equal(lse[rows], want_lse[rows]), (seed, shift)
        assert bool(torch.isfinite(lse[rows]).any())
        first = want[rows].clone() if first is None else first
    assert not torch.equal(first, want[rows])


# ---- a fixed-seed random slice

FUZZ_SEED, FUZZ_DRAWS = 5, 32


def fuzz_draws(torch):
    """[(dtype, kind, heads, block size, [(L, n, words)])]: drawn on the CPU from FUZZ_SEED alone"""
    g = torch.Generator().manual_seed(FUZZ_SEED)
    pick = lambda xs: xs[int(torch.randint(0, len(xs), (1,), generator=g))]   # noqa: E731
    draws = []
    for _ in range(FUZZ_DRAWS):
        seqs = []
        for _ in range(pick([1, 2, 3])):
            n = pick([1, 2, 5, 17, 31, 32, 33, 63, 64, 65])
            ctx = pick([0, 1, 40, 63, 64, 100, 191, 230])
            L = pick([n - 2, 3]) if pick(range(10)) == 0 else ctx + n           # (one in ten: fewer keys than new tokens)
            seqs.append((max(L, 0), n, pick(["tree", "tree", "random", "random", "zeros", "ones", "self"])))
        draws.append((pick(["bf16", "fp16"]), pick(KINDS), pick([8, 16, 24, 128]), pick([16, 48, 64]), seqs))
    return draws


def test_fixed_seed_random_slice():
    import torch
    rows = empty = 0
    problems = []
    for i, (dtype, kind, Hq, bs, seqs) in enumerate(fuzz_draws(torch)):
        p = Problem(torch, 900 + i, dtype, kind, Hq, bs, seqs, cap=max(L for L, _, _ in seqs) + pick_spare(i) * bs)
        rows += sum(p.ns)
        empty += p.rows_without_a_key()
        problems.append(p)
    print("fuzz: %d draws, %d rows, %d without a visible key" % (len(problems), rows, empty))
    assert 4 * empty <= rows, (empty, rows)                 # the bound is not met trivially
    assert sum(p.differs_from_the_chain() for p in problems) >= len(problems) * 3 // 4
    seen = set()
    for i, p in enumerate(problems):
        out, lse = p.run()
        seen.add(p.nsplit() > 1)
        p.check(out, lse, "fuzz %d: %s %s H%d bs%d %s" % (i, p.dtype, p.kind, p.Hq, p.bs, p.seqs))
    assert seen == {True, False}


def pick_spare(i):
    """spare table blocks of draw i: none, two, or enough for key-range splits"""
    return (0, 2, 8)[i % 3]
