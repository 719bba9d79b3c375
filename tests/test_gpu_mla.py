"""Paged MLA attention on the GPU (csrc/fa_fwd_mla_paged_gfx950.hip behind aule.flash_attention_mla_paged /
aule_attention_mla_paged_ex): one latent cache [num_blocks, block_size, 576], keys = its rows, values = their first 512 elements.

The judge is the fp64 oracle of the paged DECODE, one query token at a time, as tests/test_gpu_paged_query.py does: token i of
sequence b is `paged_decode_f64` with the latent cache reshaped to [nb, bs, 1, 576] as both K and V, the context length
max(L_b - n_b + 1 + i, 0), and [..., :512] of its result -- the definition of the call, with no oracle of its own.  Bounds are the
project's: fwd_tol(dtype, max |V|) for the output and LSE_ATOL = 1e-3 against an fp64 log-sum-exp formed here.  Inputs are N(0, 1)
quantised to the dtype.  Every check prints the maxima it achieved."""
import ctypes
import math

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from test_gpu_paged_query import _table
from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

LSE_ATOL = 1e-3
QK, VD = 576, 512
DTYPE_CODE = {"fp16": 1, "bf16": 2}


class Case:
    """Seeded inputs of one case.  ns = None: plain decode (sequence b owns row b); else ns[b] new tokens of sequence b, packed behind
    `lead` rows that belong to no sequence.  `tail` more such rows at the end; q_pad > 0: q is a slice of a wider projection."""

    def __init__(self, seed, dtype, Hq, bs, Ls, ns=None, table_lens=None, extra_cols=2, lead=0, tail=0, q_pad=0):
        rng = np.random.RandomState(seed)
        self.dtype, self.Hq, self.bs, self.B, self.ns, self.q_pad = dtype, Hq, bs, len(Ls), ns, q_pad
        self.toks = [1] * self.B if ns is None else list(ns)
        assert ns is not None or lead == 0
        self.T = lead + sum(self.toks) + tail
        self.starts = lead + np.concatenate([[0], np.cumsum(self.toks)]).astype(np.int32)
        self.cu = None if ns is None else self.starts.copy()
        self.max_sq = max(self.toks)
        table_lens = list(Ls) if table_lens is None else table_lens
        num_blocks = sum((n + bs - 1) // bs for n in table_lens) + 3
        self.q = quantize(rng.randn(self.T, Hq, QK).astype(np.float32), dtype)
        self.kv = quantize(rng.randn(num_blocks, bs, QK).astype(np.float32), dtype)
        self.bt = _table(rng, self.B, bs, table_lens, num_blocks, extra_cols)
        self.cl = np.array(Ls, dtype=np.int32)
        self.vmax = float(np.abs(self.kv[..., :VD]).max())
        self._ref = {}

    def owned(self):
        own = np.zeros(self.T, dtype=bool)
        for b in range(self.B):
            own[self.starts[b]:self.starts[b] + self.toks[b]] = True
        return own

    def device(self, torch):
        dt = torch_dtype(self.dtype)
        q = torch.from_numpy(self.q).to("cuda", dt)
        if self.q_pad:
            wide = torch.zeros((self.T, self.Hq + self.q_pad, QK), device="cuda", dtype=dt)
            wide[:, :self.Hq] = q
            q = wide[:, :self.Hq]
        cu = None if self.cu is None else torch.from_numpy(self.cu).cuda()
        return q, torch.from_numpy(self.kv).to("cuda", dt), torch.from_numpy(self.bt).cuda(), torch.from_numpy(self.cl).cuda(), cu

    def run(self, torch, scale=None, tensors=None):
        import aule
        q, kv, bt, cl, cu = tensors or self.device(torch)
        return aule.flash_attention_mla_paged(q, kv, bt, cl, cu, max_seqlen_q=None if cu is None else self.max_sq, scale=scale, return_lse=True)

    def lse_row(self, b, r, n, sc, ft=np.float64):
        """[Hq]: the log-sum-exp of query row r over the first n > 0 keys of sequence b at the scale sc, formed in `ft` (float64: the
        judge; float32: what plain fp32 arithmetic leaves of the same row)"""
        j = np.arange(n)
        s = self.q[r].astype(ft) @ self.kv[self.bt[b][j // self.bs], j % self.bs].astype(ft).T * ft(sc)
        m = s.max(axis=-1)
        return (m + np.log(np.exp(s - m[:, None]).sum(axis=-1))).astype(np.float64)

    def _rows(self):
        """[(i, sequences with a token i, their q rows, the keys those rows see)]"""
        L = np.clip(self.cl.astype(np.int64), 0, self.bt.shape[1] * self.bs)
        for i in range(self.max_sq):
            sel = [b for b in range(self.B) if self.toks[b] > i]
            yield sel, [int(self.starts[b]) + i for b in sel], [max(int(L[b]) - self.toks[b] + 1 + i, 0) for b in sel]

    def reference(self, oracle_mod, scale=None):
        """(out [T, Hq, 512] from the decode oracle, lse [T, Hq] float64) of the owned rows; computed once per scale"""
        if scale in self._ref:
            return self._ref[scale]
        K4 = self.kv.astype(np.float64)[:, :, None, :]
        ref = np.zeros((self.T, self.Hq, VD))
        lref = np.full((self.T, self.Hq), -np.inf)
        sc = 1.0 / math.sqrt(QK) if scale is None else scale
        for sel, rows, ctx in self._rows():
            ref[rows] = oracle_mod.paged_decode_f64(self.q[rows], K4, K4, self.bt[sel], ctx, scale)[..., :VD]
            for b, r, n in zip(sel, rows, ctx):
                if n > 0:
                    lref[r] = self.lse_row(b, r, n, sc)
        self._ref[scale] = (ref, lref)
        return self._ref[scale]

    def lse_f32_gap(self, scale=None):
        """max |fp32 log-sum-exp - fp64 log-sum-exp| over the owned rows that see a key: the error plain NumPy fp32 arithmetic has on
        these inputs (what an LSE bound may follow when the logits are large)"""
        sc = 1.0 / math.sqrt(QK) if scale is None else scale
        return max([float(np.abs(self.lse_row(b, r, n, sc, np.float32) - self.lse_row(b, r, n, sc)).max())
                    for sel, rows, ctx in self._rows() for b, r, n in zip(sel, rows, ctx) if n > 0] or [0.0])


def _judge(c, out, lse, oracle_mod, what, scale=None, lse_atol=LSE_ATOL):
    """the owned rows against the judge; returns the two measured maxima"""
    own = c.owned()
    out, lse = out.float().cpu().numpy()[own], lse.cpu().numpy().astype(np.float64)[own]
    ref, lref = (x[own] for x in c.reference(oracle_mod, scale))
    atol, rtol = fwd_tol(c.dtype, c.vmax)
    none = ~np.isfinite(lref)
    lerr = float(np.abs(lse[~none] - lref[~none]).max()) if (~none).any() else 0.0
    oerr = float(np.abs(out - ref).max())
    print("%s: max |out err| %.3g (atol %.3g), max |lse err| %.3g (bound %.3g), rows without a key %d of %d"
          % (what, oerr, atol, lerr, lse_atol, int(none.sum()), none.size))
    assert_close(out, ref, atol, rtol, what)
    assert np.array_equal(np.isneginf(lse), none), "%s: lse must be -inf exactly where a row sees no key" % what
    assert not np.isnan(lse).any()
    assert bool((out[none] == 0).all()), "%s: a row that sees no key must be zeros" % what
    assert lerr <= lse_atol, (what, lerr)
    return oerr, lerr


def _desc(torch, c, tensors, out, lse, ws=None, T=None):
    from aule import _capi
    q, kv, bt, cl, cu = tensors
    d = _capi.MlaPagedDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.qk_dim, d.v_dim = DTYPE_CODE[c.dtype], c.B, c.Hq, QK, VD
    d.block_size, d.max_blocks = c.bs, bt.shape[1]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = c.T if T is None else T, c.max_sq, q.stride(0)
    d.device = torch.cuda.current_device()
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.kv_cache, d.block_tables, d.context_lens = q.data_ptr(), kv.data_ptr(), bt.data_ptr(), cl.data_ptr()
    d.cu_seqlens_q = cu.data_ptr() if cu is not None else None
    d.out, d.lse = out.data_ptr(), lse.data_ptr() if lse is not None else None
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    return d


def _nsplit(d):
    from aule import _capi
    plan = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(d), plan, 6) == 6
    return plan[2]


def _poisoned(torch, c, T=None):
    T = c.T if T is None else T
    out = torch.full((T, c.Hq, VD), -1, dtype=torch.int16, device="cuda").view(torch_dtype(c.dtype))
    lse = torch.full((T, c.Hq), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    return out, lse


def _c_call(torch, c, tensors, out, lse, ws=None, T=None):
    from aule import _capi
    lib = _capi.get_lib()
    d = _desc(torch, c, tensors, out, lse, ws, T)
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    return d


# ------------------------------------------------------------------------------------------------------------------- decode, null offsets
DECODE = [  # dtype, heads, block size, lengths, spare table columns, scale, splits expected
    ("bf16", 16, 16, [1, 33, 200], 2, None, True),          # a quarter-filled row block; 15 x 16 keys of capacity: two key ranges
    ("fp16", 128, 16, [1, 33, 200], 0, None, True),         # two row blocks per sequence
    ("bf16", 5, 16, [1, 33, 200], 2, 192 ** -0.5, True),    # rows that are no multiple of anything; the DeepSeek scale
    ("fp16", 128, 64, [63, 64, 65], 0, None, False),        # around a tile's and a block's edge; two 64-key tiles of capacity: one launch
    ("bf16", 16, 64, [63, 64, 65], 2, None, True),          # ... and split
    ("fp16", 16, 24, [1, 33, 200], 2, None, True),          # the general address path
]


@pytest.mark.parametrize("dtype,Hq,bs,Ls,extra,scale,split", DECODE, ids=lambda x: str(x).replace(" ", ""))
def test_decode_vs_the_decode_oracle(dtype, Hq, bs, Ls, extra, scale, split, oracle_mod):
    import torch
    c = Case(11, dtype, Hq, bs, Ls, extra_cols=extra)
    tensors = c.device(torch)
    out, lse = c.run(torch, scale, tensors)
    torch.cuda.synchronize()
    assert out.shape == (3, Hq, VD) and out.dtype == torch_dtype(dtype) and lse.shape == (3, Hq) and lse.dtype == torch.float32
    assert (_nsplit(_desc(torch, c, tensors, out, lse)) > 1) == split
    _judge(c, out, lse, oracle_mod, "decode %s H%d bs%d %s" % (dtype, Hq, bs, Ls), scale)
    # the 4-d spelling of the cache is the same call
    q, kv, bt, cl, _ = tensors
    out4, lse4 = c.run(torch, scale, (q, kv.view(kv.shape[0], bs, 1, QK), bt, cl, None))
    assert same_bits(torch, out4, out) and same_bits(torch, lse4, lse)


# ---------------------------------------------------------------------------------------------------------------------------------- ragged
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ragged_rows_straddle_tokens(dtype, oracle_mod):
    """heads 24 with n_b = {3, 1, 2}: 72 rows of the first sequence are a full block and a block of 8, and a block holds tokens at
    different positions; lengths {70, 1, 40}"""
    import torch
    c = Case(21, dtype, 24, 16, [70, 1, 40], ns=[3, 1, 2])
    out, lse = c.run(torch)
    torch.cuda.synchronize()
    _judge(c, out, lse, oracle_mod, "ragged %s H24 n{3,1,2}" % dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ragged_negative_positions_empty_sequence_and_strided_q(dtype, oracle_mod):
    """a sequence with n_b > L_b (its first tokens sit at negative positions: zeros and -inf), one with L_b = 0, q a slice of a wider
    projection, rows in front of and behind the sequences"""
    import torch
    c = Case(22, dtype, 24, 16, [70, 2, 0, 40], ns=[3, 4, 2, 2], lead=2, tail=3, q_pad=8)
    tensors = c.device(torch)
    assert tensors[0].stride(0) == (24 + 8) * QK
    out, lse = c.run(torch, None, tensors)
    torch.cuda.synchronize()
    _judge(c, out, lse, oracle_mod, "ragged %s strided, n > L, L = 0" % dtype)
    _, lref = c.reference(oracle_mod)
    assert np.isneginf(lref[2 + 3:2 + 3 + 2]).all() and np.isfinite(lref[2 + 3 + 2:2 + 3 + 4]).all() and np.isneginf(lref[9:11]).all()
    # the same bits from contiguous queries
    q = tensors[0].contiguous()
    out2, lse2 = c.run(torch, None, (q,) + tensors[1:])
    own = torch.from_numpy(c.owned()).cuda()
    assert same_bits(torch, out2[own], out[own]) and same_bits(torch, lse2[own], lse[own])


# ---------------------------------------------------------------------------------------------------------------------------------- splits
@pytest.mark.parametrize("dtype,L", [("bf16", 1500), ("fp16", 1500), ("bf16", 40), ("fp16", 0)])
def test_key_ranges_of_one_sequence(dtype, L, oracle_mod):
    """batch 1, heads 16, capacity 2048: the plan splits the keys; at length 40 all splits but the first are empty, at length 0 all are.
    Two runs give the same bits."""
    import torch
    c = Case(31, dtype, 16, 64, [L], table_lens=[2048], extra_cols=0)
    tensors = c.device(torch)
    assert tensors[2].shape == (1, 32)
    out, lse = c.run(torch, None, tensors)
    torch.cuda.synchronize()
    ns = _nsplit(_desc(torch, c, tensors, out, lse))
    print("nsplit", ns)
    assert ns >= 2
    _judge(c, out, lse, oracle_mod, "split x%d %s L=%d" % (ns, dtype, L))
    out2, lse2 = c.run(torch, None, tensors)
    assert same_bits(torch, out2, out) and same_bits(torch, lse2, lse)


def test_wide_batch_takes_one_launch(oracle_mod):
    """300 sequences x 16 heads at length 64: more row blocks than compute units, nsplit = 1"""
    import torch
    rng = np.random.RandomState(5)
    c = Case(32, "bf16", 16, 64, [int(x) for x in rng.randint(1, 65, size=300)], table_lens=[64] * 300, extra_cols=0)
    c.cl[:3] = 64
    tensors = c.device(torch)
    out, lse = c.run(torch, None, tensors)
    torch.cuda.synchronize()
    assert _nsplit(_desc(torch, c, tensors, out, lse)) == 1
    _judge(c, out, lse, oracle_mod, "decode B300 H16")


# ------------------------------------------------------------------------------------------------------- rows never written, clamps
def test_unowned_rows_keep_their_bytes_and_lengths_are_clamped(oracle_mod):
    import torch
    c = Case(41, "bf16", 24, 16, [70, 1, 40], ns=[3, 1, 2], lead=1, tail=4)
    tensors = c.device(torch)
    own = torch.from_numpy(c.owned()).cuda()
    out, lse = _poisoned(torch, c)
    _c_call(torch, c, tensors, out, lse)
    assert bool((out.view(torch.int16)[~own] == -1).all()) and bool((lse.view(torch.int32)[~own] == -1).all())
    _judge(c, out, lse, oracle_mod, "C entry, lead 1, tail 4")
    want, want_lse = c.run(torch, None, tensors)
    assert same_bits(torch, out[own], want[own]) and same_bits(torch, lse[own], want_lse[own])
    # plain decode with total_tokens padded past the batch
    cd = Case(42, "fp16", 16, 16, [1, 33, 200], tail=5)
    td = cd.device(torch)
    out, lse = _poisoned(torch, cd)
    _c_call(torch, cd, td, out, lse)
    assert bool((out.view(torch.int16)[3:] == -1).all()) and bool((lse.view(torch.int32)[3:] == -1).all())
    _judge(cd, out, lse, oracle_mod, "C entry, decode, tail 5")
    # context_lens above the table's capacity: the clamped call, bit for bit
    cap = tensors[2].shape[1] * c.bs
    big = tensors[3].clone()
    big[0] = cap + 1000
    at_cap = tensors[3].clone()
    at_cap[0] = cap
    a, al = c.run(torch, None, tensors[:3] + (big,) + tensors[4:])
    b, bl = c.run(torch, None, tensors[:3] + (at_cap,) + tensors[4:])
    assert same_bits(torch, a[own], b[own]) and same_bits(torch, al[own], bl[own]) and not same_bits(torch, a[own], want[own])
    neg = tensors[3].clone()
    neg[0] = -7
    a, al = c.run(torch, None, tensors[:3] + (neg,) + tensors[4:])
    assert bool((a[1:4] == 0).all()) and bool(torch.isneginf(al[1:4]).all())


def test_hostile_offsets_write_nothing_outside_out():
    """cu_seqlens_q pointing past total_tokens, backwards and below zero: out / lse are [T] rows inside larger poisoned buffers, and
    nothing but those T rows changes"""
    import torch
    c = Case(43, "bf16", 24, 16, [70, 1, 40], ns=[3, 1, 2])
    q, kv, bt, cl, cu = c.device(torch)
    for hostile in ([0, 4, c.T + 5, c.T + 100], [-5, 2, 1, 2 ** 31 - 1], [c.T + 1, c.T + 2, c.T + 3, c.T + 4]):
        big_out, big_lse = _poisoned(torch, c, c.T + 8)
        cu.copy_(torch.tensor(hostile, dtype=torch.int32, device="cuda"))
        _c_call(torch, c, (q, kv, bt, cl, cu), big_out[4:4 + c.T], big_lse[4:4 + c.T])
        for x in (big_out.view(torch.int16), big_lse.view(torch.int32)):
            assert bool((x[:4] == -1).all()) and bool((x[4 + c.T:] == -1).all()), hostile


def test_poisoned_workspace_does_not_change_a_split_result():
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    c = Case(31, "bf16", 16, 64, [1500], table_lens=[2048], extra_cols=0)
    tensors = c.device(torch)
    want, want_lse = c.run(torch, None, tensors)
    out, lse = _poisoned(torch, c)
    size = lib.aule_attention_mla_paged_workspace_size(ctypes.byref(_desc(torch, c, tensors, out, lse)))
    assert size > 0
    for nbytes, with_lse in ((size, True), (size, False), (64, True)):   # (64: too small, the library allocates on the stream)
        out, lse = _poisoned(torch, c)
        ws = torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")
        _c_call(torch, c, tensors, out, lse if with_lse else None, ws)
        assert same_bits(torch, out, want)
        assert same_bits(torch, lse, want_lse) if with_lse else bool((lse.view(torch.int32) == -1).all())


# ------------------------------------------------------------------------------------------------------------------------ hostile memory
@pytest.mark.parametrize("which", ["decode", "ragged-split"])
def test_inside_an_arena(which, oracle_mod):
    """every tensor of the call between guard bands of one allocation, outputs and workspace poisoned: the guards stay intact, the
    inputs unchanged, and the owned rows equal the plain call's bits"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    if which == "decode":
        c = Case(51, "fp16", 16, 16, [1, 33, 150], extra_cols=0, tail=2)   # three tiles of capacity: one launch
    else:
        c = Case(52, "bf16", 24, 64, [700, 3, 129], ns=[3, 1, 2], table_lens=[1024] * 3, extra_cols=0, lead=1, tail=2)
    plain = c.device(torch)
    own = torch.from_numpy(c.owned()).cuda()
    if which == "decode":   # (the Python call takes no padded rows with null offsets: the first B rows are the sequences')
        want, want_lse = (x[own] for x in _poisoned(torch, c))
        want[:], want_lse[:] = c.run(torch, None, (plain[0][:c.B],) + plain[1:])
    else:
        want, want_lse = (x[own] for x in c.run(torch, None, plain))
    probe_out, probe_lse = _poisoned(torch, c)
    d0 = _desc(torch, c, plain, probe_out, probe_lse)
    size = int(lib.aule_attention_mla_paged_workspace_size(ctypes.byref(d0)))
    assert (size > 0) == (which == "ragged-split") and (_nsplit(d0) > 1) == (which == "ragged-split")
    dt = torch_dtype(c.dtype)
    host = dict(q=torch.from_numpy(c.q).to(dt), kv=torch.from_numpy(c.kv).to(dt), bt=torch.from_numpy(c.bt), cl=torch.from_numpy(c.cl))
    if c.cu is not None:
        host["cu"] = torch.from_numpy(c.cu)
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in host.items()]
    regions += [("out", c.T * c.Hq * VD * 2, "out"), ("lse", c.T * c.Hq * 4, "out"), ("ws", max(size, 16), "ws")]
    arena = Arena(torch, regions, QK * 2)
    kept = {k: arena.upload(k, v) for k, v in host.items()}
    arena.fill(POISON)
    q = arena.view("q", dt, (c.T, c.Hq, QK))
    tensors = (q, arena.view("kv", dt, c.kv.shape), arena.view("bt", torch.int32, c.bt.shape), arena.view("cl", torch.int32, c.cl.shape),
               arena.view("cu", torch.int32, c.cu.shape) if c.cu is not None else None)
    out, lse = arena.view("out", dt, (c.T, c.Hq, VD)), arena.view("lse", torch.float32, (c.T, c.Hq))
    _c_call(torch, c, tensors, out, lse, arena.bytes("ws") if size else None)
    assert arena.guards_intact(), arena.damage()
    for k, v in kept.items():
        assert arena.unchanged(k, v), k
    assert same_bits(torch, out[own], want) and same_bits(torch, lse[own], want_lse)
    assert bool((out.view(torch.int16)[~own] == -1).all()) and bool((lse.view(torch.int32)[~own] == -1).all())
    _judge(c, out, lse, oracle_mod, "arena, " + which)


# ------------------------------------------------------------------------------------------------------------------------------------ graph
def test_capture_replays_with_the_current_lengths():
    """torch.cuda.graph of one split call (workspace from torch's allocator, max_seqlen_q given: no synchronisation): after
    context_lens is overwritten in place a replay equals a fresh eager call on the new contents"""
    import torch
    import aule
    c = Case(61, "bf16", 16, 64, [1500, 700], ns=[2, 1], table_lens=[2048, 2048], extra_cols=0)
    q, kv, bt, cl, cu = c.device(torch)
    fn = lambda: aule.flash_attention_mla_paged(q, kv, bt, cl, cu, max_seqlen_q=2, return_lse=True)   # noqa: E731
    eager, eager_lse = fn()
    torch.cuda.synchronize()
    assert _nsplit(_desc(torch, c, (q, kv, bt, cl, cu), eager, eager_lse)) >= 2
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
    assert same_bits(torch, out, eager) and same_bits(torch, lse, eager_lse)
    for new_cl in ([40, 2048], [0, 1], [2000, 333]):
        cl.copy_(torch.tensor(new_cl, device="cuda", dtype=torch.int32))
        want, want_lse = fn()
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert not same_bits(torch, want, eager)
        assert same_bits(torch, out, want) and same_bits(torch, lse, want_lse), new_cl


# -------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_the_device():
    import torch
    import aule
    from aule import _capi
    lib = _capi.get_lib()
    c = Case(71, "bf16", 16, 16, [1, 33, 200])
    q, kv, bt, cl, _ = c.device(torch)
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        aule.flash_attention_mla_paged(q.cpu(), kv.cpu(), bt.cpu(), cl.cpu())
    with pytest.raises(ValueError, match="latent width must be 576"):
        aule.flash_attention_mla_paged(q[..., :512].contiguous(), kv[..., :512].contiguous(), bt, cl)
    with pytest.raises(ValueError, match=r"block_tables must be \[batch, max_blocks\]"):
        aule.flash_attention_mla_paged(q[:2], kv, bt, cl)
    out, lse = _poisoned(torch, c)

    def refused(change, needle):
        d = _desc(torch, c, (q, kv, bt, cl, None), out, lse)
        change(d)
        assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg

    refused(lambda d: setattr(d, "qk_dim", 512), "qk_dim 512")
    refused(lambda d: setattr(d, "v_dim", 576), "v_dim 576")
    refused(lambda d: setattr(d, "total_tokens", 2), "total_tokens < batch")
    refused(lambda d: setattr(d, "q", q.data_ptr() + 2), "16-byte aligned")
    refused(lambda d: setattr(d, "kv_cache", None), "null tensor pointer")
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == -1).all())
    d = _desc(torch, c, (q, kv, bt, cl, None), out, lse)
    d.heads_q = 0
    assert lib.aule_attention_mla_paged_ex(ctypes.byref(d)) == 0
