"""The paged cascade on the GPU (csrc/fa_fwd_paged_shared_prefix_gfx950.hip, the paged prefill and
csrc/fa_merge_states_gfx950.hip behind aule.flash_attention_paged_cascade / aule_attention_paged_cascade_ex), and
aule.merge_attention_states.

The judge: `oracle.paged_decode_f64` on a block-size-1 view of the caches, one row per token, whose table is the P prefix
slots followed by the sequence's own slots and whose context is P + p + 1 for a token at own position p >= 0, 0 otherwise.
That serves any P, aligned to a block or not.  The output bound is fwd_tol(dtype, max |V|, sides=2): the state over the own
keys is rounded to 16 bits once before the merge rounds again -- the project's two-rounding rule; the LSE against an fp64
log-sum-exp formed here, within LSE_ATOL.  -inf must appear exactly where a row sees no key, zeros in those rows, no NaN.

The batch is the prefill's -- 1, 37, 130, 0 and 300 new tokens against 1, 37, 130, 50 and 371 own keys -- plus a sequence of
20 tokens with 8 own keys (tokens 0 .. 11 sit at negative positions).  Prefix lengths 0, 1, 63, 64, 65 and 200 on a table
whose capacity gives more than one key split, and 30 and 64 on a table of at most 64 keys where the block size allows (one
split): a tile edge, a partial last tile, splits that hold no key."""
import ctypes
import math

import numpy as np
import pytest

from hostile import POISON, Arena
from test_gpu_paged_prefill import INT32_MIN, Ragged
from test_gpu_paged_query import LSE_ATOL
from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

NS, LS = [1, 37, 130, 0, 300, 20], [1, 37, 130, 50, 371, 8]
BIG, SMALL = 200, 64       # keys the two prefix tables are sized for (BIG: plus two spare columns; SMALL: rounded down to blocks)


class Cascade:
    """A Ragged batch plus a prefix table into the same block pool (the prefix may share blocks with a sequence: they are only
    read).  `keys`: what the table is sized for; `spare` more columns follow.  `blocks`: the table's length itself."""

    def __init__(self, p, seed, keys=BIG, spare=2, blocks=None):
        self.p = p
        rng = np.random.RandomState(seed)
        nb = (keys + p.bs - 1) // p.bs + spare if spare else max(keys // p.bs, 1)   # spare = 0: at most `keys` keys where a block allows
        nb = nb if blocks is None else blocks
        assert nb <= p.kdev.shape[0]
        self.pbt = rng.permutation(p.kdev.shape[0])[:nb].astype(np.int32)
        self.cap = nb * p.bs
        self._ref = {}

    def clamp(self, P):
        return min(max(int(P), 0), self.cap)

    def table(self, P, hostile=True):
        """the prefix table; hostile: the columns past ceil(P / bs) hold INT32_MIN and huge values"""
        t = self.pbt.copy()
        if hostile:
            first = (self.clamp(P) + self.p.bs - 1) // self.p.bs
            t[first:] = [INT32_MIN if i % 2 == 0 else 2 ** 31 - 1 - i for i in range(len(t) - first)]
        return t

    def _slots(self, P, b, L):
        """the cache rows of the P prefix keys, then of sequence b's L own keys (a block-size-1 view of the pool)"""
        p, bs = self.p, self.p.bs
        j, jo = np.arange(P), np.arange(L)
        return np.concatenate([self.pbt[j // bs].astype(np.int64) * bs + j % bs, p.bt[b][jo // bs].astype(np.int64) * bs + jo % bs])

    def lse_rows(self, P, b, s, n, L, scale=None, ft=np.float64):
        """[n, Hq]: the log-sum-exp of the token rows s .. s + n - 1 over prefix plus own keys, -inf where a row sees none; formed in
        `ft` (float64: the judge; float32: what plain fp32 arithmetic leaves of the same rows)"""
        p = self.p
        g = p.Hq // p.Hkv
        scale = 1.0 / math.sqrt(p.D) if scale is None else scale
        pos = L - n + np.arange(n)
        ctx = np.where(pos >= 0, P + pos + 1, 0)
        rows = np.full((n, p.Hq), -np.inf)
        if P + L > 0:
            k = p.K.reshape(-1, 1, p.Hkv, p.D)[self._slots(P, b, L), 0].astype(ft)
            sc = np.einsum("nhgd,lhd->nhgl", p.q[s:s + n].astype(ft).reshape(n, p.Hkv, g, p.D), k) * ft(scale)
            see = np.arange(P + L)[None, :] < ctx[:, None]
            sc = np.where(see[:, None, None, :], sc, ft(-np.inf))
            m = sc.max(axis=-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                v = m + np.log(np.exp(sc - np.where(np.isfinite(m), m, ft(0.0))[..., None]).sum(axis=-1))
            rows = np.where(np.isfinite(m), v, -np.inf).reshape(n, p.Hq).astype(np.float64)
        return rows

    def reference(self, oracle_mod, P, scale=None, **kw):
        """(out [T, Hq, D] float32, lse [T, Hq] float64) on the owned rows; once per (P, scale, lengths)"""
        p, P = self.p, self.clamp(P)
        key = (P, scale, tuple((k, tuple(np.asarray(v).tolist()) if k != "max_sq" else v) for k, v in sorted(kw.items())))
        if key in self._ref:
            return self._ref[key]
        K1, V1 = (x.reshape(-1, 1, p.Hkv, p.D) for x in (p.K, p.V))
        out = np.zeros((p.T, p.Hq, p.D), dtype=np.float32)
        lse = np.full((p.T, p.Hq), np.nan)
        for b, s, n, L in p.sequences(**kw):
            if n == 0:
                continue
            slots = self._slots(P, b, L)
            pos = L - n + np.arange(n)
            ctx = np.where(pos >= 0, P + pos + 1, 0)
            if len(slots) == 0:
                slots = np.zeros(1, dtype=np.int64)
            out[s:s + n] = oracle_mod.paged_decode_f64(p.q[s:s + n], K1, V1, np.repeat(slots[None], n, axis=0), ctx, scale, -1)
            lse[s:s + n] = self.lse_rows(P, b, s, n, L, scale)
        self._ref[key] = (out, lse)
        return out, lse

    def lse_f32_gap(self, P, scale=None, **kw):
        """max |fp32 log-sum-exp - fp64 log-sum-exp| over the owned rows that see a key (Ragged.lse_f32_gap, with the prefix)"""
        gap, P = 0.0, self.clamp(P)
        for b, s, n, L in self.p.sequences(**kw):
            if n and P + L:
                a, r = self.lse_rows(P, b, s, n, L, scale, np.float32), self.lse_rows(P, b, s, n, L, scale)
                fin = np.isfinite(r)
                if fin.any():
                    gap = max(gap, float(np.abs(a[fin] - r[fin]).max()))
        return gap

    def device(self, torch, P, cu=None, cl=None, hostile=True, q_pad=0):
        args, scales = self.p.device(torch, cu, cl, q_pad)
        plen = P if torch.is_tensor(P) else torch.tensor([P], dtype=torch.int32, device="cuda")
        return args, scales, torch.from_numpy(self.table(int(plen[0]) if torch.is_tensor(P) else P, hostile)).cuda(), plen

    def run(self, torch, P, max_sq=None, cu=None, cl=None, scale=None, hostile=True, q_pad=0):
        import aule
        (q, kc, vc, bt, cl, cu), scales, pbt, plen = self.device(torch, P, cu, cl, hostile, q_pad)
        return aule.flash_attention_paged_cascade(q, kc, vc, pbt, plen, bt, cl, cu, max_seqlen_q=self.p.max_sq if max_sq is None else max_sq,
                                                  scale=scale, return_lse=True, **scales)


def _judge(c, out, lse, oracle_mod, P, what, scale=None, lse_atol=LSE_ATOL, **kw):
    """the owned rows of (out, lse) against the oracle; prints the measured maxima before it asserts and returns them"""
    p = c.p
    own = p.owned(**kw)
    ref, lref = c.reference(oracle_mod, P, scale, **kw)
    out, lse = out.float().cpu().numpy()[own], lse.cpu().numpy().astype(np.float64)[own]
    ref, lref = ref[own], lref[own]
    atol, rtol = fwd_tol(p.dtype, p.vmax, sides=2)
    none = np.isneginf(lref)
    lerr = float(np.abs(lse[~none] - lref[~none]).max()) if (~none).any() else 0.0
    print("%s: %d rows, max |out err| %.3g (atol %.3g), max |lse err| %.3g (bound %.3g), rows without a key %d"
          % (what, int(own.sum()), np.abs(out - ref).max() if own.any() else 0.0, atol, lerr, lse_atol, int(none.sum())))
    assert not np.isnan(lse).any() and not np.isnan(out).any(), what
    assert_close(out, ref, atol, rtol, what)
    assert np.array_equal(np.isneginf(lse), none), "%s: lse must be -inf exactly where a row sees no key" % what
    assert bool((out[none] == 0).all()), "%s: a row that sees no key must be zeros" % what
    assert lerr <= lse_atol, (what, lerr)
    return float(np.abs(out - ref).max()) if own.any() else 0.0, lerr


def _desc(torch, c, args, scales, pbt, plen, out, lse, max_sq, ws=None):
    from aule import _capi
    p = c.p
    q, kc, vc, bt, cl, cu = args
    d = _capi.PagedCascadeDesc()
    d.struct_size = ctypes.sizeof(_capi.PagedCascadeDesc)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    d.cache_dtype = 1 if scales else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = cl.shape[0], p.Hq, p.Hkv, p.D
    d.block_size, d.max_blocks, d.max_prefix_blocks = p.bs, bt.shape[1], pbt.shape[0]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = p.T, max_sq, p.Hq * p.D
    d.scale, d.device = 0.0, q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.block_tables, d.context_lens, d.cu_seqlens_q = bt.data_ptr(), cl.data_ptr(), cu.data_ptr()
    d.prefix_block_table, d.prefix_len = pbt.data_ptr(), plen.data_ptr()
    if scales:
        d.k_scale, d.v_scale = scales["k_scale"].data_ptr(), scales["v_scale"].data_ptr()
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    return d


def _nsplit(d):
    from aule import _capi
    plan = (ctypes.c_int32 * 7)()
    assert _capi.load().aule_hip_debug_shared_prefix_plan(ctypes.byref(d), plan, 7) == 7
    return plan[2]


SHAPES = [  # dtype, Hq, Hkv, D, block size
    ("bf16", 32, 8, 128, 16),     # GQA 32/8
    ("fp16", 32, 8, 128, 16),
    ("fp16", 6, 2, 64, 24),       # g = 3: a token's heads straddle waves and blocks; the divide
    ("bf16", 4, 1, 32, 128),      # MQA; blocks larger than a tile
    ("fp16", 8, 8, 128, 1),       # MHA; one key per block
    ("bf16", 6, 2, 64, 24),       # the D = 64 and D = 32 instances of the other query type
    ("fp16", 4, 1, 32, 128),
]
PREFIXES = [(0, BIG), (1, BIG), (63, BIG), (64, BIG), (65, BIG), (200, BIG), (30, SMALL), (64, SMALL)]
_problems = {}


def _problem(kind, dtype, Hq, Hkv, D, bs, keys=BIG):
    key = (kind, dtype, Hq, Hkv, D, bs, keys)
    if key not in _problems:
        base = (kind, dtype, Hq, Hkv, D, bs)
        if base not in _problems:
            _problems[base] = Ragged(71, dtype, kind, Hq, Hkv, D, bs, NS, LS)
        _problems[key] = Cascade(_problems[base], 72, keys, spare=2 if keys == BIG else 0)
    return _problems[key]


@pytest.mark.parametrize("prefix", PREFIXES, ids=lambda x: "P%d-table%d" % x)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-H%dkv%d-D%d-bs%d" % s)
@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_cascade_rows_and_lse_vs_oracle(kind, shape, prefix, oracle_mod):
    import torch
    P, keys = prefix
    c = _problem(kind, *shape, keys=keys)
    p = c.p
    out, lse = c.run(torch, P)
    torch.cuda.synchronize()
    assert out.shape == (p.T, p.Hq, p.D) and out.dtype == torch_dtype(p.dtype) and lse.shape == (p.T, p.Hq) and lse.dtype == torch.float32
    _judge(c, out, lse, oracle_mod, P, "paged cascade, P = %d" % P)
    # the key splits the case ran with
    args, scales, pbt, plen = c.device(torch, P)
    n = _nsplit(_desc(torch, c, args, scales, pbt, plen, out, lse, p.max_sq))
    assert n == 1 if c.cap <= 64 else n > 1, (n, c.cap)     # one tile: one split; else the 256 CUs want more than one
    # the sequence of 20 tokens with 8 own keys: tokens 0 .. 11 at negative positions, whatever the prefix holds
    lse = lse.cpu().numpy()
    s = int(p.cu[5])
    assert bool(np.isneginf(lse[s:s + 12]).all()) and bool(np.isfinite(lse[s + 12:s + 20]).all())
    assert bool((out[s:s + 12] == 0).all())


@pytest.mark.parametrize("kind", ["16", "fp8"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=lambda s: "%s-H%dkv%d-D%d-bs%d" % s)
def test_empty_prefix_is_the_paged_prefill_bit_for_bit(kind, shape):
    import torch
    import aule
    c = _problem(kind, *shape)
    (q, kc, vc, bt, cl, cu), scales, pbt, plen = c.device(torch, 0)
    got = aule.flash_attention_paged_cascade(q, kc, vc, pbt, plen, bt, cl, cu, max_seqlen_q=c.p.max_sq, return_lse=True, **scales)
    want = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=c.p.max_sq, return_lse=True, **scales)
    torch.cuda.synchronize()
    own = torch.from_numpy(c.p.owned()).cuda()
    assert torch.equal(got[0][own].view(torch.int16), want[0][own].view(torch.int16))
    assert torch.equal(got[1][own].view(torch.int32), want[1][own].view(torch.int32))
    only_out = aule.flash_attention_paged_cascade(q, kc, vc, pbt, 0, bt, cl, cu, max_seqlen_q=c.p.max_sq, **scales)   # a Python int; no lse
    torch.cuda.synchronize()
    assert torch.equal(only_out[own].view(torch.int16), want[0][own].view(torch.int16))


@pytest.mark.parametrize("hostile,like", [(-5, 0), (INT32_MIN, 0), (None, None)], ids=["minus5", "int32min", "capacity+1000"])
def test_hostile_prefix_len_behaves_as_its_clamp(hostile, like, oracle_mod):
    import torch
    c = _problem("16", *SHAPES[2])
    if hostile is None:
        hostile, like = c.cap + 1000, c.cap
    got = c.run(torch, hostile)
    want = c.run(torch, like)
    torch.cuda.synchronize()
    own = torch.from_numpy(c.p.owned()).cuda()
    assert torch.equal(got[0][own].view(torch.int16), want[0][own].view(torch.int16))
    assert torch.equal(got[1][own].view(torch.int32), want[1][own].view(torch.int32))
    _judge(c, got[0], got[1], oracle_mod, hostile, "prefix_len %d" % hostile)


def _arena_run(torch, c, P, nan_outside=False, cu=None, cl=None):
    """through the C entry with every tensor, the workspace included, inside one poisoned arena; returns (arena, inputs kept,
    out, lse).  cu, cl: in place of the problem's offsets and lengths"""
    from aule import _capi
    lib = _capi.get_lib()
    p = c.p
    q = p.q.copy()
    if nan_outside:
        q[~p.owned(cu=cu, cl=cl)] = np.nan
    cu, cl = (np.asarray(have if given is None else given, dtype=np.int32) for have, given in ((p.cu, cu), (p.cl, cl)))
    tensors = {"q": q, "bt": p.bt, "cl": cl, "cu": cu, "pbt": c.table(P), "plen": np.array([P], dtype=np.int32)}
    dt = torch_dtype(p.dtype)
    dev = {k: torch.from_numpy(v) for k, v in tensors.items()}
    dev["q"] = dev["q"].to(dt)
    dev["k"], dev["v"] = (torch.from_numpy(x) if p.fp8 else torch.from_numpy(x).to(dt) for x in (p.kdev, p.vdev))
    if p.fp8:
        dev["ks"], dev["vs"] = (torch.tensor(x, dtype=torch.float32) for x in (p.ks, p.vs))
    rows = p.T * p.Hq
    # the workspace size needs a descriptor: shape fields only
    d = _capi.PagedCascadeDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = {"fp16": 1, "bf16": 2}[p.dtype], 1 if p.fp8 else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = p.B, p.Hq, p.Hkv, p.D
    d.block_size, d.max_blocks, d.max_prefix_blocks = p.bs, p.bt.shape[1], len(c.pbt)
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = p.T, p.max_sq, p.Hq * p.D
    d.device = torch.cuda.current_device()
    ws_bytes = lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d))
    assert ws_bytes > 0
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in dev.items()]
    regions += [("out", rows * p.D * 2, "out"), ("lse", rows * 4, "out"), ("ws", ws_bytes, "ws")]
    a = Arena(torch, regions, p.D * 2)
    kept = {k: a.upload(k, v) for k, v in dev.items()}
    a.fill(POISON)
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out, d.lse = a.ptr("q"), a.ptr("k"), a.ptr("v"), a.ptr("out"), a.ptr("lse")
    d.block_tables, d.context_lens, d.cu_seqlens_q = a.ptr("bt"), a.ptr("cl"), a.ptr("cu")
    d.prefix_block_table, d.prefix_len = a.ptr("pbt"), a.ptr("plen")
    d.workspace, d.workspace_bytes = a.ptr("ws"), ws_bytes
    if p.fp8:
        d.k_scale, d.v_scale = a.ptr("ks"), a.ptr("vs")
    assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    return a, kept, a.view("out", dt, (p.T, p.Hq, p.D)), a.view("lse", torch.float32, (p.T, p.Hq))


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_inside_a_poisoned_arena_with_rows_of_no_sequence(kind, oracle_mod):
    """Five rows in front of the first sequence and 40 behind the last, their q rows NaN; every tensor and the workspace inside
    one arena of 0xFF: the guard bands stay intact, the inputs unchanged, the rows of no sequence keep their poison in out and
    lse, and the owned rows satisfy the oracle without a NaN -- a NaN partial of an unowned row does not travel."""
    import torch
    p = Ragged(73, "bf16", kind, 8, 2, 64, 16, [3, 0, 140, 1], [70, 9, 140, 200], lead=5, tail=40)
    c = Cascade(p, 74, keys=100)
    a, kept, out, lse = _arena_run(torch, c, 100, nan_outside=True)
    assert a.guards_intact(), a.damage()
    for name, was in kept.items():
        assert a.unchanged(name, was), name
    own = p.owned()
    assert own.sum() == 144 and not own[:5].any() and not own[-40:].any()
    free = torch.from_numpy(~own).cuda()
    assert bool((out.view(torch.int16)[free] == -1).all()) and bool((lse.view(torch.int32)[free] == -1).all())
    _judge(c, out, lse, oracle_mod, 100, "arena, lead 5, tail 40")


def test_hostile_offsets_and_lengths_inside_a_poisoned_arena(oracle_mod):
    """cu_seqlens_q negative, past the end and decreasing, context_lens negative, INT32_MIN and far beyond the table (every table entry a
    real block), through the shared-prefix pass, the prefill AND the merge kernel, which clamps for itself.  After the clamps sequence 0
    owns rows 0 .. 2 with no own key (negative positions: zeros and -inf, whatever the prefix holds), sequence 2 rows 3 .. 142 with the
    table's 208 keys, the others nothing; the 46 rows behind them belong to nobody and keep their poison, the guards stay intact."""
    import torch
    p = Ragged(76, "bf16", "16", 8, 2, 64, 16, [3, 0, 140, 1], [70, 9, 140, 200], tail=45, table_lens=[208] * 4, extra_cols=0)
    c = Cascade(p, 77, keys=100)
    cu, cl = [-5, 3, 3, p.T + 7, 20], [-7, 9, 100000, INT32_MIN]
    assert p.T == 189 and p.sequences(cu=cu, cl=cl) == [(0, 0, 3, 0), (1, 3, 0, 9), (2, 3, 140, 208), (3, 189, 0, 0)]
    a, kept, out, lse = _arena_run(torch, c, 100, nan_outside=True, cu=cu, cl=cl)
    assert a.guards_intact(), a.damage()
    for name, was in kept.items():
        assert a.unchanged(name, was), name
    own = p.owned(cu=cu, cl=cl)
    assert own.sum() == 143 and own[:143].all()
    free = torch.from_numpy(~own).cuda()
    assert bool((out.view(torch.int16)[free] == -1).all()) and bool((lse.view(torch.int32)[free] == -1).all())
    assert bool((out[:3] == 0).all()) and bool(torch.isneginf(lse[:3]).all())
    _judge(c, out, lse, oracle_mod, 100, "arena, hostile offsets and lengths", cu=cu, cl=cl)


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_capture_replays_with_the_current_lengths(kind):
    """torch.cuda.graph: no allocation node and no synchronisation in the captured call; after prefix_len, context_lens and
    cu_seqlens_q are overwritten in place a replay equals a fresh eager call on the new contents."""
    import torch
    import aule
    ns, Ls = [200, 5, 1, 94], [300, 37, 500, 94]
    p = Ragged(75, "fp16", kind, 32, 8, 128, 16, ns, Ls, table_lens=[512] * 4)
    c = Cascade(p, 76, keys=400)
    (q, kc, vc, bt, cl, cu), scales, pbt, plen = c.device(torch, 333, hostile=False)
    fn = lambda: aule.flash_attention_paged_cascade(q, kc, vc, pbt, plen, bt, cl, cu, max_seqlen_q=256, return_lse=True, **scales)   # noqa: E731
    eager, eager_lse = fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, lse = fn()
    out.zero_(); lse.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
    for new_p, new_cu, new_cl in ((64, [0, 17, 17, 273, 300], [17, 400, 512, 10]), (0, [0, 100, 200, 250, 300], [100, 100, 50, 50]),
                                  (400, [0, 1, 2, 3, 4], [1, 2, 3, 4])):
        plen.fill_(new_p)
        cu.copy_(torch.tensor(new_cu, device="cuda", dtype=torch.int32))
        cl.copy_(torch.tensor(new_cl, device="cuda", dtype=torch.int32))
        want, want_lse = fn()
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        own = torch.zeros(p.T, dtype=torch.bool, device="cuda")
        own[:new_cu[-1]] = True
        assert not torch.equal(want, eager)
        assert torch.equal(out[own], want[own]) and torch.equal(lse[own], want_lse[own]), new_p


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_c_entry_with_a_caller_workspace_equals_the_python_path(kind):
    """... bit for bit, with and without an lse buffer; a workspace that is too small falls back to the stream's allocator."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    c = _problem(kind, *SHAPES[0])
    p = c.p
    want, want_lse = c.run(torch, 200)
    args, scales, pbt, plen = c.device(torch, 200)
    own = torch.from_numpy(p.owned()).cuda()
    d0 = _desc(torch, c, args, scales, pbt, plen, want, None, p.max_sq)
    size = lib.aule_attention_paged_cascade_workspace_size(ctypes.byref(d0))
    assert size > 0
    for ws_bytes, with_lse in ((size, True), (size, False), (64, True)):
        out = torch.full((p.T, p.Hq, p.D), -1, dtype=torch.int16, device="cuda").view(torch_dtype(p.dtype))
        lse = torch.full((p.T, p.Hq), -1, dtype=torch.int32, device="cuda").view(torch.float32)
        ws = torch.full((ws_bytes,), POISON, dtype=torch.uint8, device="cuda")
        d = _desc(torch, c, args, scales, pbt, plen, out, lse if with_lse else None, p.max_sq, ws)
        assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert torch.equal(out[own].view(torch.int16), want[own].view(torch.int16))
        if with_lse:
            assert torch.equal(lse[own].view(torch.int32), want_lse[own].view(torch.int32))
        else:
            assert bool((lse.view(torch.int32) == -1).all())


def test_c_abi_refusals_on_the_device():
    """-3 and a reason for what the checker refuses, with real device pointers in every other field."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    c = _problem("fp8", *SHAPES[2])
    args, scales, pbt, plen = c.device(torch, 65)
    out = torch.empty((c.p.T, c.p.Hq, c.p.D), device="cuda", dtype=torch_dtype(c.p.dtype))

    def refused(change, needle):
        d = _desc(torch, c, args, scales, pbt, plen, out, None, c.p.max_sq)
        change(d)
        assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg

    refused(lambda d: setattr(d, "struct_size", 152), "struct_size")
    refused(lambda d: setattr(d, "head_dim", 256), "head_dim 256")
    refused(lambda d: setattr(d, "max_seqlen_q", 0), "max_seqlen_q")
    refused(lambda d: setattr(d, "max_prefix_blocks", 0), "max_prefix_blocks")
    refused(lambda d: setattr(d, "q_token_stride", 6 * 64 + 4), "multiple of 8")
    refused(lambda d: setattr(d, "prefix_len", None), "null tensor pointer")
    refused(lambda d: setattr(d, "prefix_block_table", None), "null tensor pointer")
    refused(lambda d: setattr(d, "k_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "q", args[0].data_ptr() + 2), "16-byte aligned")
    d = _desc(torch, c, args, scales, pbt, plen, out, None, c.p.max_sq)
    d.total_tokens = 0
    assert lib.aule_attention_paged_cascade_ex(ctypes.byref(d)) == 0


# ---------------------------------------------------------------------------------------------------------------- merge_attention_states
def _states(dtype, N=37, H=6, D=64, seed=77):
    """seeded states; rows 0 .. 2 of head 0: a has no key, b has no key, neither has"""
    rng = np.random.RandomState(seed)
    oa, ob = (quantize(rng.randn(N, H, D).astype(np.float32), dtype) for _ in range(2))
    la, lb = (3.0 * rng.randn(N, H)).astype(np.float32), (3.0 * rng.randn(N, H)).astype(np.float32)
    la[0, 0] = lb[1, 0] = la[2, 0] = lb[2, 0] = -np.inf
    return oa, la, ob, lb


@pytest.mark.parametrize("dtype,D", [("bf16", 64), ("fp16", 128), ("fp16", 40)])
def test_merge_states_vs_fp64_and_its_exact_rules(dtype, D):
    import torch
    import aule
    from aule import _capi
    oa, la, ob, lb = _states(dtype, D=D)
    dt = torch_dtype(dtype)
    toa, tob = (torch.from_numpy(x).to("cuda", dt) for x in (oa, ob))
    tla, tlb = (torch.from_numpy(x).cuda() for x in (la, lb))
    out, lse = aule.merge_attention_states(toa, tla, tob, tlb)
    rev, rev_lse = aule.merge_attention_states(tob, tlb, toa, tla)
    torch.cuda.synchronize()
    assert out.shape == toa.shape and out.dtype == dt and lse.shape == tla.shape and lse.dtype == torch.float32
    # either order, the same bits
    assert torch.equal(out.view(torch.int16), rev.view(torch.int16)) and torch.equal(lse.view(torch.int32), rev_lse.view(torch.int32))
    # the fp64 formula
    with np.errstate(invalid="ignore", divide="ignore"):
        M = np.maximum(la, lb).astype(np.float64)
        Ms = np.where(np.isfinite(M), M, 0.0)
        wa, wb = np.exp(la - Ms), np.exp(lb - Ms)
        ref = np.where((wa + wb)[..., None] > 0, (wa[..., None] * oa + wb[..., None] * ob) / np.where(wa + wb > 0, wa + wb, 1.0)[..., None], 0.0)
        lref = np.where(wa + wb > 0, Ms + np.log(wa + wb), -np.inf)
    atol, rtol = fwd_tol(dtype, max(np.abs(oa).max(), np.abs(ob).max()))
    got, glse = out.float().cpu().numpy(), lse.cpu().numpy().astype(np.float64)
    fin = np.isfinite(lref)
    print("merge: max |out err| %.3g (atol %.3g), max |lse err| %.3g" % (np.abs(got - ref).max(), atol, np.abs(glse[fin] - lref[fin]).max()))
    assert_close(got, ref, atol, rtol, "merge_attention_states")
    assert np.array_equal(np.isneginf(glse), ~fin) and float(np.abs(glse[fin] - lref[fin]).max()) <= LSE_ATOL
    # the -inf rules, bit for bit
    assert torch.equal(out[0, 0].view(torch.int16), tob[0, 0].view(torch.int16)) and torch.equal(lse[0, 0], tlb[0, 0])
    assert torch.equal(out[1, 0].view(torch.int16), toa[1, 0].view(torch.int16)) and torch.equal(lse[1, 0], tla[1, 0])
    assert bool((out[2, 0].view(torch.int16) == 0).all()) and bool(torch.isneginf(lse[2, 0]))
    # out aliases an input, through the C entry
    lib = _capi.get_lib()
    for alias in ("a", "b"):
        xa, xb = toa.clone(), tob.clone()
        lo = torch.empty_like(tla)
        d = _capi.MergeStatesDesc()
        d.struct_size = ctypes.sizeof(d)
        d.dtype, d.rows, d.heads, d.head_dim = {"fp16": 1, "bf16": 2}[dtype], oa.shape[0], oa.shape[1], D
        d.device = torch.cuda.current_device()
        d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        d.out_a, d.lse_a, d.out_b, d.lse_b = xa.data_ptr(), tla.data_ptr(), xb.data_ptr(), tlb.data_ptr()
        d.out, d.lse = (xa if alias == "a" else xb).data_ptr(), lo.data_ptr()
        assert lib.aule_attention_merge_states_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert torch.equal((xa if alias == "a" else xb).view(torch.int16), out.view(torch.int16)) and torch.equal(lo.view(torch.int32), lse.view(torch.int32))
        assert torch.equal((xb if alias == "a" else xa), (tob if alias == "a" else toa))
        # ... but lse may not: at D = 40 a row's threads straddle waves, and every one of them reads both inputs
        d.out, d.lse = out.data_ptr(), (tla if alias == "a" else tlb).data_ptr()
        before = (tla if alias == "a" else tlb).clone()
        assert lib.aule_attention_merge_states_ex(ctypes.byref(d)) == -3 and b"must not overlap" in lib.aule_get_error()
        torch.cuda.synchronize()
        assert torch.equal((tla if alias == "a" else tlb).view(torch.int32), before.view(torch.int32))
