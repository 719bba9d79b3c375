"""The paged prefill on the GPU (csrc/fa_fwd_paged_prefill_gfx950.hip behind aule.flash_attention_paged_prefill /
aule_attention_paged_prefill_ex): ragged per-sequence queries, packed along the first axis of q, against the paged KV cache.

The judge is the one of tests/test_gpu_paged_query.py: row s_b + i of the call is `oracle.paged_decode_f64` on that query row
with the context max(L_b - n_b + 1 + i, 0) and the same window (FP8: on the dequantised caches in float64), under the
project's forward bound fwd_tol(dtype, max |V|); the LSE against an fp64 log-sum-exp formed here, within LSE_ATOL = 1e-3 -- the
sibling's bound, for the sibling's reason: fp32 sums of unrounded weights and two hardware transcendental steps.  -inf must
appear exactly where a row sees no key, zeros in those rows, and no NaN anywhere.

Shapes are the smallest that reach each path: a block is 128 packed rows (token-major, g = Hq / Hkv heads per token), a
wave 32 of them, a key tile 64 keys; block sizes 1, 16 (shift), 24 (divide) and 128 (larger than a tile)."""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_paged_query import CODE_8, LSE_ATOL, _decode, _table
from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

INT32_MIN = -(2 ** 31)


class Ragged:
    """Seeded inputs of one ragged batch: sequence b has ns[b] new tokens and Ls[b] keys.  cu_seqlens_q starts at `lead`
    and q has `tail` rows behind the last sequence.  The table is sized for table_lens (default: Ls); the block pool holds at
    least `pool` blocks (default: what the tables need, plus 3)."""

    def __init__(self, seed, dtype, kind, Hq, Hkv, D, bs, ns, Ls, lead=0, tail=0, table_lens=None, extra_cols=2, pool=None):
        rng = np.random.RandomState(seed)
        self.dtype, self.fp8, self.bs, self.B = dtype, kind == "fp8", bs, len(ns)
        self.Hq, self.Hkv, self.D = Hq, Hkv, D
        table_lens = [max(int(x), 0) for x in (Ls if table_lens is None else table_lens)]
        num_blocks = max(sum((n + bs - 1) // bs for n in table_lens) + 3, pool or 0)
        shape = (num_blocks, bs, Hkv, D)
        self.cu = (lead + np.concatenate([[0], np.cumsum(ns)])).astype(np.int32)
        self.T = int(self.cu[-1]) + tail
        if self.fp8:
            self.q = quantize(0.25 * rng.randn(self.T, Hq, D).astype(np.float32), dtype)
            self.kdev, self.vdev = ((rng.randint(0, CODE_8 + 1, size=shape) | (rng.randint(0, 2, size=shape) << 7)).astype(np.uint8)
                                    for _ in range(2))
            self.ks, self.vs = rng.uniform(0.25, 2.0, Hkv), rng.uniform(0.25, 2.0, Hkv)
            self.K = _decode(self.kdev) * self.ks.reshape(1, 1, -1, 1)
            self.V = _decode(self.vdev) * self.vs.reshape(1, 1, -1, 1)
        else:
            self.q = quantize(rng.randn(self.T, Hq, D).astype(np.float32), dtype)
            self.kdev, self.vdev = (quantize(rng.randn(*shape).astype(np.float32), dtype) for _ in range(2))
            self.ks = self.vs = None
            self.K, self.V = self.kdev.astype(np.float64), self.vdev.astype(np.float64)
        self.bt = _table(rng, self.B, bs, table_lens, num_blocks, extra_cols)
        self.cl = np.array(Ls, dtype=np.int32)
        self.vmax = float(np.abs(self.V).max())
        self.max_sq = max(max(ns), 1)
        self._ref = {}

    # ---- what the kernel is defined to do with (cu, cl): the clamps of include/aule.h
    def sequences(self, cu=None, cl=None, max_sq=None):
        """[(b, s, n, L)] after the device's clamps"""
        cu = self.cu if cu is None else np.asarray(cu)
        cl = self.cl if cl is None else np.asarray(cl)
        max_sq = self.max_sq if max_sq is None else max_sq
        cap = self.bt.shape[1] * self.bs
        res = []
        for b in range(len(cl)):
            L = min(max(int(cl[b]), 0), cap)
            s = min(max(int(cu[b]), 0), self.T)
            e = min(max(int(cu[b + 1]), s), self.T)
            res.append((b, s, min(e - s, max_sq), L))
        return res

    def owned(self, **kw):
        """bool [T]: the rows that belong to a sequence"""
        m = np.zeros(self.T, dtype=bool)
        for _, s, n, _ in self.sequences(**kw):
            m[s:s + n] = True
        return m

    def lse_rows(self, b, s, n, L, window=-1, scale=None, ft=np.float64):
        """[n, Hq]: ln sum_j exp(scale q_i . k_j) over the keys the token rows s .. s + n - 1 of sequence b see, -inf where a row sees
        none; formed in `ft` -- float64: the judge; float32: what plain fp32 arithmetic leaves of the same rows"""
        g = self.Hq // self.Hkv
        scale = 1.0 / math.sqrt(self.D) if scale is None else scale
        rows = np.full((n, self.Hq), -np.inf)
        if L > 0:
            j = np.arange(L)
            k = self.K[self.bt[b][j // self.bs], j % self.bs].astype(ft)               # [L, Hkv, D]
            sc = np.einsum("nhgd,lhd->nhgl", self.q[s:s + n].astype(ft).reshape(n, self.Hkv, g, self.D), k) * ft(scale)
            p = L - n + np.arange(n)
            see = j[None, :] <= p[:, None]
            if window > 0:
                see &= p[:, None] - j[None, :] < window
            sc = np.where(see[:, None, None, :], sc, ft(-np.inf))
            m = sc.max(axis=-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                v = m + np.log(np.exp(sc - np.where(np.isfinite(m), m, ft(0.0))[..., None]).sum(axis=-1))
            rows = np.where(np.isfinite(m), v, -np.inf).reshape(n, self.Hq).astype(np.float64)
        return rows

    def reference(self, oracle_mod, window=-1, scale=None, **kw):
        """(out [T, Hq, D] float32, lse [T, Hq] float64) on the owned rows, zeros / +inf markers elsewhere; computed once per
        (window, scale, lengths) and shared"""
        key = (window, scale, tuple((k, tuple(np.asarray(v).tolist()) if k != "max_sq" else v) for k, v in sorted(kw.items())))
        if key in self._ref:
            return self._ref[key]
        out = np.zeros((self.T, self.Hq, self.D), dtype=np.float32)
        lse = np.full((self.T, self.Hq), np.nan)
        for b, s, n, L in self.sequences(**kw):
            if n == 0:
                continue
            ctx = np.maximum(L - n + 1 + np.arange(n), 0)
            out[s:s + n] = oracle_mod.paged_decode_f64(self.q[s:s + n], self.K, self.V, np.repeat(self.bt[b:b + 1], n, axis=0), ctx, scale, window)
            lse[s:s + n] = self.lse_rows(b, s, n, L, window, scale)
        self._ref[key] = (out, lse)
        return out, lse

    def lse_f32_gap(self, window=-1, scale=None, **kw):
        """max |fp32 log-sum-exp - fp64 log-sum-exp| over the owned rows that see a key: the error plain NumPy fp32 arithmetic has on
        these inputs (what an LSE bound may follow when the logits are large)"""
        gap = 0.0
        for b, s, n, L in self.sequences(**kw):
            if n and L:
                a, r = self.lse_rows(b, s, n, L, window, scale, np.float32), self.lse_rows(b, s, n, L, window, scale)
                fin = np.isfinite(r)
                if fin.any():
                    gap = max(gap, float(np.abs(a[fin] - r[fin]).max()))
        return gap

    # ---- the device side
    def device(self, torch, cu=None, cl=None, q_pad=0):
        """q_pad > 0: q is a slice of a [T, Hq D + q_pad] projection whose other columns hold NaN bits"""
        dt = torch_dtype(self.dtype)
        if self.fp8:
            kc, vc = (torch.from_numpy(x).cuda().view(torch.float8_e4m3fn) for x in (self.kdev, self.vdev))
            scales = dict(k_scale=torch.tensor(self.ks, dtype=torch.float32, device="cuda"),
                          v_scale=torch.tensor(self.vs, dtype=torch.float32, device="cuda"))
        else:
            kc, vc = (torch.from_numpy(x).to("cuda", dt) for x in (self.kdev, self.vdev))
            scales = {}
        cu = torch.from_numpy(np.asarray(self.cu if cu is None else cu, dtype=np.int32)).cuda()
        cl = torch.from_numpy(np.asarray(self.cl if cl is None else cl, dtype=np.int32)).cuda()
        q = torch.from_numpy(self.q).to("cuda", dt)
        if q_pad:
            wide = torch.full((self.T, self.Hq * self.D + q_pad), -1, dtype=torch.int16, device="cuda").view(dt)
            wide[:, :self.Hq * self.D] = q.view(self.T, -1)
            q = wide[:, :self.Hq * self.D].view(self.T, self.Hq, self.D)
        return (q, kc, vc, torch.from_numpy(self.bt).cuda(), cl, cu), scales

    def run(self, torch, window=-1, max_sq=None, cu=None, cl=None, scale=None, q_pad=0):
        import aule
        args, scales = self.device(torch, cu, cl, q_pad)
        return aule.flash_attention_paged_prefill(*args, max_seqlen_q=self.max_sq if max_sq is None else max_sq, scale=scale, window_size=window,
                                                  return_lse=True, **scales)


def _judge(p, out, lse, oracle_mod, window, what, scale=None, lse_atol=LSE_ATOL, **kw):
    """the owned rows of (out, lse) against the oracle; prints the measured maxima before it asserts and returns them"""
    own = p.owned(**kw)
    ref, lref = p.reference(oracle_mod, window, scale, **kw)
    out, lse = out.float().cpu().numpy()[own], lse.cpu().numpy().astype(np.float64)[own]
    ref, lref = ref[own], lref[own]
    atol, rtol = fwd_tol(p.dtype, p.vmax)
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


# The ragged batch of every shape: new tokens 1, 37, 130, 0, 300 against lengths
#   0    the sequence has no key at all (zeros, -inf)
#   20   shorter than its 37 tokens: tokens 0 .. 16 sit at negative positions
#   130  no prefix (L = n), and the last tokens cross the tile boundary at key 128
#   50   a sequence without new tokens: nothing of it is computed or written
#   371  a 71-key prefix; 371 = 5 tiles + 51 keys, 23 blocks of 16 + 3 keys, 15 of 24 + 11, 2 of 128 + 115
# Windows: with the 71-key prefix, block 0 of the long sequence holds positions 71 .. 102 (g = 4), 71 .. 113 (g = 3), 71 .. 198
# (g = 1): the lower edges p - W + 1 of its first and last row fall in different 64-key tiles for W = 16 (55 | 87 ..), for W = 300 in
# the last block (.. 63 | 64 ..: positions 359 .. 370 at g = 4), and for W = 1 in block 1 (103 .. 134 at g = 4).
NS, LS = [1, 37, 130, 0, 300], [0, 20, 130, 50, 371]
SHAPES = [  # dtype, Hq, Hkv, D, block size, window
    ("bf16", 32, 8, 128, 16, -1),     # GQA 32/8
    ("fp16", 32, 8, 128, 16, 16),
    ("fp16", 6, 2, 64, 24, -1),       # g = 3: a token's heads straddle waves and blocks; the divide
    ("bf16", 6, 2, 64, 1, 300),       # one key per block
    ("bf16", 4, 1, 32, 128, -1),      # MQA; blocks larger than a tile
    ("fp16", 4, 1, 32, 16, 1),
    ("fp16", 8, 8, 128, 24, -1),      # MHA: a block is 128 tokens
    ("bf16", 8, 8, 128, 128, 300),
]
CASES = [(kind,) + s for kind in ("16", "fp8") for s in SHAPES]
_problems = {}


def _problem(kind, dtype, Hq, Hkv, D, bs):
    key = (kind, dtype, Hq, Hkv, D, bs)
    if key not in _problems:
        _problems[key] = Ragged(61, dtype, kind, Hq, Hkv, D, bs, NS, LS)
    return _problems[key]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "kv%s-%s-H%dkv%d-D%d-bs%d-w%d" % c)
def test_ragged_rows_and_lse_vs_oracle(case, oracle_mod):
    import torch
    kind, dtype, Hq, Hkv, D, bs, window = case
    p = _problem(kind, dtype, Hq, Hkv, D, bs)
    out, lse = p.run(torch, window)
    torch.cuda.synchronize()
    assert out.shape == (p.T, Hq, D) and out.dtype == torch_dtype(dtype) and lse.shape == (p.T, Hq) and lse.dtype == torch.float32
    _judge(p, out, lse, oracle_mod, window, "paged prefill")
    lse = lse.cpu().numpy()
    assert bool(np.isneginf(lse[0]).all())                          # L = 0
    assert bool(np.isneginf(lse[1:1 + 17]).all()) and bool(np.isfinite(lse[1 + 17:38]).all())    # positions -17 .. -1, then 0 .. 19


def _desc(torch, p, args, scales, out, lse, max_sq, window=-1, q_stride=None, scale=0.0):
    from aule import _capi
    q, kc, vc, bt, cl, cu = args
    d = _capi.PagedPrefillDesc()
    d.struct_size = ctypes.sizeof(_capi.PagedPrefillDesc)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    d.cache_dtype = 1 if scales else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = cl.shape[0], p.Hq, p.Hkv, p.D
    d.block_size, d.max_blocks = p.bs, bt.shape[1]
    d.total_tokens, d.max_seqlen_q = p.T, max_sq
    d.q_token_stride = p.Hq * p.D if q_stride is None else q_stride
    d.scale, d.window_size, d.device = scale, window, q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.block_tables, d.context_lens, d.cu_seqlens_q = bt.data_ptr(), cl.data_ptr(), cu.data_ptr()
    if scales:
        d.k_scale, d.v_scale = scales["k_scale"].data_ptr(), scales["v_scale"].data_ptr()
    return d


PAD = 64   # rows of 0xFF in front of and behind out / lse


def _run_capi(torch, p, max_sq=None, window=-1, cu=None, cl=None, with_lse=True, scale=None, q_pad=0, entry="aule_attention_paged_prefill_ex"):
    """through the C-ABI into 0xFF-filled buffers with PAD rows of margin on both sides; returns (out, lse, margins intact).  (entry: the
    FP8-product twin takes the same descriptor)"""
    from aule import _capi
    lib = _capi.get_lib()
    args, scales = p.device(torch, cu, cl, q_pad)
    big_o = torch.full((p.T + 2 * PAD, p.Hq, p.D), -1, dtype=torch.int16, device="cuda")
    big_l = torch.full((p.T + 2 * PAD, p.Hq), -1, dtype=torch.int32, device="cuda")
    out, lse = big_o[PAD:PAD + p.T], big_l[PAD:PAD + p.T]
    d = _desc(torch, p, args, scales, out, lse if with_lse else None, p.max_sq if max_sq is None else max_sq, window,
              args[0].stride(0) if q_pad else None, 0.0 if scale is None else scale)
    assert getattr(lib, entry)(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    intact = all(bool((t[:PAD] == -1).all()) and bool((t[PAD + p.T:] == -1).all()) for t in (big_o, big_l))
    return out.view(torch_dtype(p.dtype)), lse.view(torch.float32), intact


def _untouched(torch, out, lse, own):
    """every row outside the sequences still holds the 0xFF it was filled with"""
    free = torch.from_numpy(~own).cuda()
    return bool((out.view(torch.int16)[free] == -1).all()) and bool((lse.view(torch.int32)[free] == -1).all())


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_rows_outside_the_sequences_are_never_written(kind, oracle_mod):
    """cu_seqlens_q[0] = 5 and a tail of 40 rows padded for graph capture; out / lse pre-filled with 0xFF.  Then the same batch
    with max_seqlen_q far above every n_b -- a grid of mostly idle workgroups -- bit for bit; and without lse."""
    import torch
    p = Ragged(62, "bf16", kind, 8, 2, 64, 16, [3, 0, 140, 1], [70, 9, 140, 200], lead=5, tail=40)
    out, lse, intact = _run_capi(torch, p)
    own = p.owned()
    assert own.sum() == 144 and not own[:5].any() and not own[-40:].any()
    assert intact and _untouched(torch, out, lse, own)
    _judge(p, out, lse, oracle_mod, -1, "lead 5, tail 40")
    out2, lse2, intact2 = _run_capi(torch, p, max_sq=5000)      # (cut to T = 189 by the entry: 6 blocks per unit against 5)
    assert intact2 and torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(lse2.view(torch.int32), lse.view(torch.int32))
    out3, lse3, intact3 = _run_capi(torch, p, with_lse=False)
    assert intact3 and torch.equal(out3.view(torch.int16), out.view(torch.int16)) and bool((lse3.view(torch.int32) == -1).all())
    # max_seqlen_q below a sequence's count cuts that sequence: its first 100 rows, at positions L - 100 + i
    out4, lse4, intact4 = _run_capi(torch, p, max_sq=100)
    own4 = p.owned(max_sq=100)
    assert own4.sum() == 104 and intact4 and _untouched(torch, out4, lse4, own4)
    _judge(p, out4, lse4, oracle_mod, -1, "max_seqlen_q 100 < 140", max_sq=100)


def test_hostile_context_lens_are_clamped(oracle_mod):
    """Above what the table addresses, negative, INT32_MIN: clamped on the device to [0, max_blocks * block_size]."""
    import torch
    bs, cols = 16, 6
    p = Ragged(63, "fp16", "16", 8, 2, 128, bs, [40, 7, 3, 20], [cols * bs] * 4, extra_cols=0)
    assert p.bt.shape[1] == cols
    full = _run_capi(torch, p)
    hostile_cl = [cols * bs + 1000, 2 ** 31 - 1, -5, INT32_MIN]
    got = _run_capi(torch, p, cl=hostile_cl)
    assert full[2] and got[2]
    own = p.owned()
    assert _untouched(torch, got[0], got[1], own)
    _judge(p, got[0], got[1], oracle_mod, -1, "hostile context_lens", cl=hostile_cl)
    for b, s, n, L in p.sequences(cl=hostile_cl):
        if b < 2:      # clamped to the capacity: the rows of the full-length run, bit for bit
            assert L == cols * bs
            assert torch.equal(got[0][s:s + n], full[0][s:s + n]) and torch.equal(got[1][s:s + n], full[1][s:s + n])
        else:          # clamped to 0
            assert L == 0 and bool((got[0][s:s + n] == 0).all()) and bool(torch.isneginf(got[1][s:s + n]).all())


@pytest.mark.parametrize("name,cu", [("decreasing", [0, 40, 70, 60, 50]), ("beyond-T", [0, 40, 70, 1000, 2 ** 31 - 1]),
                                     ("negative", [INT32_MIN, 40, 70, 70, -3])])
def test_hostile_cu_seqlens_stay_inside_the_buffers(name, cu, oracle_mod):
    """Offsets are clamped on the device: s = clamp(cu[b], 0, T), e = clamp(cu[b + 1], s, T).  Nothing outside out / lse is
    written, rows no clamped sequence owns keep their 0xFF, and the well-formed sequences 0 and 1 give the rows they give in
    a well-formed batch, bit for bit.  Every address stays inside the allocations by the clamps."""
    import torch
    p = Ragged(64, "bf16", "16", 6, 2, 64, 16, [40, 30, 20, 10], [100, 30, 64, 33])
    assert p.T == 100
    good = _run_capi(torch, p)
    got = _run_capi(torch, p, cu=cu)
    assert good[2] and got[2], "wrote outside out / lse"
    seqs = p.sequences(cu=cu)
    assert [(s, n) for _, s, n, _ in seqs] == {"decreasing": [(0, 40), (40, 30), (70, 0), (60, 0)], "beyond-T": [(0, 40), (40, 30), (70, 30), (100, 0)],
                                                "negative": [(0, 40), (40, 30), (70, 0), (70, 0)]}[name]
    assert _untouched(torch, got[0], got[1], p.owned(cu=cu))
    assert torch.equal(got[0][:70], good[0][:70]) and torch.equal(got[1][:70], good[1][:70])
    _judge(p, got[0], got[1], oracle_mod, -1, "hostile cu_seqlens_q: " + name, cu=cu)


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_sequences_do_not_depend_on_their_place_in_the_batch(kind):
    """Permuting the sequences of a batch (with their tables and lengths) gives the same per-sequence rows bit for bit; so
    does a sequence alone."""
    import torch
    import aule
    p = Ragged(65, "fp16", kind, 6, 2, 64, 24, [1, 37, 130, 0, 50], [300, 20, 130, 50, 99])
    (q, kc, vc, bt, cl, cu), scales = p.device(torch)
    base, base_lse = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=130, return_lse=True, **scales)
    rows = [(int(p.cu[b]), int(p.cu[b + 1])) for b in range(p.B)]
    order = [3, 2, 4, 0, 1]
    idx = torch.tensor(order, device="cuda")
    qp = torch.cat([q[rows[b][0]:rows[b][1]] for b in order])
    cup = torch.tensor(np.concatenate([[0], np.cumsum([NSb for NSb in (rows[b][1] - rows[b][0] for b in order)])]), dtype=torch.int32, device="cuda")
    perm, perm_lse = aule.flash_attention_paged_prefill(qp, kc, vc, bt[idx], cl[idx], cup, max_seqlen_q=130, return_lse=True, **scales)
    torch.cuda.synchronize()
    for i, b in enumerate(order):
        s, e = rows[b]
        ps = int(cup[i])
        assert torch.equal(perm[ps:ps + e - s], base[s:e]) and torch.equal(perm_lse[ps:ps + e - s], base_lse[s:e]), b
    for b in (1, 2, 4):
        s, e = rows[b]
        one = torch.tensor([0, e - s], dtype=torch.int32, device="cuda")
        alone, alone_lse = aule.flash_attention_paged_prefill(q[s:e], kc, vc, bt[b:b + 1], cl[b:b + 1], one, return_lse=True, **scales)
        torch.cuda.synchronize()
        assert torch.equal(alone, base[s:e]) and torch.equal(alone_lse, base_lse[s:e]), b


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_chunked_prompt_equals_the_prompt_in_one_call(kind, oracle_mod):
    """A 300-token prompt at block size 16: in one call, and as chunks of 100 with L = 100, 200, 300.  Each satisfies the
    oracle bound, and they agree within fwd_tol."""
    import torch
    import aule
    p = Ragged(66, "bf16", kind, 8, 2, 128, 16, [300], [300])
    whole, whole_lse = p.run(torch)
    torch.cuda.synchronize()
    _judge(p, whole, whole_lse, oracle_mod, -1, "prompt in one call")
    (q, kc, vc, bt, _, _), scales = p.device(torch)
    parts, parts_lse = [], []
    for c in range(3):
        cl = torch.tensor([100 * (c + 1)], dtype=torch.int32, device="cuda")
        cu = torch.tensor([0, 100], dtype=torch.int32, device="cuda")
        o, l = aule.flash_attention_paged_prefill(q[100 * c:100 * (c + 1)], kc, vc, bt, cl, cu, max_seqlen_q=100, return_lse=True, **scales)
        parts.append(o); parts_lse.append(l)
    torch.cuda.synchronize()
    chunked, chunked_lse = torch.cat(parts), torch.cat(parts_lse)
    _judge(p, chunked, chunked_lse, oracle_mod, -1, "prompt in chunks of 100")
    atol, rtol = fwd_tol("bf16", p.vmax)
    print("chunked vs whole: %.3g (atol %.3g)" % (float((chunked.float() - whole.float()).abs().max()), atol))
    assert_close(chunked.float().cpu().numpy(), whole.float().cpu().numpy(), atol, rtol, "chunked vs whole")


@pytest.mark.parametrize("dtype,kind,window", [("bf16", "16", -1), ("fp16", "fp8", 100)])
def test_agrees_with_the_paged_query_on_a_uniform_batch(dtype, kind, window):
    """Five tokens per sequence: the same problem as flash_attention_paged_query's, by another kernel -- within fwd_tol."""
    import torch
    import aule
    B, Hq, Hkv, D = 3, 32, 8, 128
    p = Ragged(67, dtype, kind, Hq, Hkv, D, 16, [5] * B, [2000, 37, 3])
    (q, kc, vc, bt, cl, cu), scales = p.device(torch)
    got, got_lse = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=5, window_size=window, return_lse=True, **scales)
    q4 = q.view(B, 5, Hq, D).permute(0, 2, 1, 3).contiguous()
    want, want_lse = aule.flash_attention_paged_query(q4, kc, vc, bt, cl, window_size=window, return_lse=True, **scales)
    torch.cuda.synchronize()
    want, want_lse = want.permute(0, 2, 1, 3).reshape(B * 5, Hq, D), want_lse.permute(0, 2, 1).reshape(B * 5, Hq)
    atol, rtol = fwd_tol(dtype, p.vmax)
    print("prefill vs paged query: %.3g (atol %.3g)" % (float((got.float() - want.float()).abs().max()), atol))
    assert_close(got.float().cpu().numpy(), want.float().cpu().numpy(), atol, rtol, "prefill vs paged query")
    assert torch.equal(torch.isneginf(got_lse), torch.isneginf(want_lse))
    fin = torch.isfinite(want_lse)
    assert float((got_lse[fin] - want_lse[fin]).abs().max()) <= 2 * LSE_ATOL      # each within LSE_ATOL of the fp64 value


def test_fused_projection_slice_is_read_in_place(oracle_mod):
    """q as a slice of a [T, 3 Hq D] projection: the token stride is passed on, nothing is copied, same bits."""
    import torch
    import aule
    p = Ragged(68, "fp16", "16", 8, 2, 64, 16, [33, 2], [100, 64])
    (q, kc, vc, bt, cl, cu), _ = p.device(torch)
    fused = torch.randn(p.T, 3 * 8 * 64, device="cuda", dtype=torch.float16)
    fused[:, 512:1024] = q.view(p.T, 512)
    qs = fused[:, 512:1024].view(p.T, 8, 64)
    assert qs.data_ptr() == fused.data_ptr() + 1024 and not qs.is_contiguous()
    got = aule.flash_attention_paged_prefill(qs, kc, vc, bt, cl, cu, max_seqlen_q=33, return_lse=True)
    want = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=33, return_lse=True)
    auto = aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu)       # max_seqlen_q read from cu_seqlens_q
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(auto, want[0])
    _judge(p, got[0], got[1], oracle_mod, -1, "strided q")


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_capture_replays_with_the_current_lengths(kind):
    """torch.cuda.graph: no allocation and no synchronisation in the captured call (max_seqlen_q is passed); a replay is
    bit-identical to eager, and after cu_seqlens_q / context_lens are overwritten in place with another ragged batch under
    the same max_seqlen_q, the replay equals the eager call on the new contents.  Both batches cover all T rows."""
    import torch
    import aule
    ns, Ls = [200, 5, 1, 94], [700, 37, 2047, 94]
    p = Ragged(69, "fp16", kind, 32, 8, 128, 16, ns, Ls, table_lens=[2048] * 4)
    (q, kc, vc, bt, cl, cu), scales = p.device(torch)
    fn = lambda: aule.flash_attention_paged_prefill(q, kc, vc, bt, cl, cu, max_seqlen_q=256, return_lse=True, **scales)   # noqa: E731
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
    for _ in range(2):
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(lse, eager_lse)
    cu.copy_(torch.tensor([0, 17, 17, 273, 300], device="cuda", dtype=torch.int32))
    cl.copy_(torch.tensor([17, 900, 2048, 10], device="cuda", dtype=torch.int32))
    want, want_lse = fn()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(want, eager)
    assert torch.equal(out, want) and torch.equal(lse, want_lse)


def test_c_abi_refusals_on_the_device():
    """-3 and a reason for what the checker refuses, with real device pointers in every other field."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Ragged(70, "bf16", "fp8", 8, 2, 64, 16, [9, 3], [40, 3])
    args, scales = p.device(torch)
    out = torch.empty((p.T, 8, 64), device="cuda", dtype=torch.bfloat16)

    def refused(change, needle):
        d = _desc(torch, p, args, scales, out, None, 9)
        change(d)
        assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg

    refused(lambda d: setattr(d, "struct_size", 144), "struct_size")
    refused(lambda d: setattr(d, "head_dim", 256), "head_dim 256")
    refused(lambda d: setattr(d, "max_seqlen_q", 0), "max_seqlen_q")
    refused(lambda d: setattr(d, "q_token_stride", 8 * 64 + 4), "multiple of 8")
    refused(lambda d: setattr(d, "cu_seqlens_q", None), "null tensor pointer")
    refused(lambda d: setattr(d, "k_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "q", args[0].data_ptr() + 2), "16-byte aligned")
    d = _desc(torch, p, args, scales, out, None, 9)
    d.total_tokens = 0
    assert lib.aule_attention_paged_prefill_ex(ctypes.byref(d)) == 0
