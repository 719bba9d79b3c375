"""Paged attention for short multi-token queries on the GPU (the fa_fwd_paged_query_kernel instances of
csrc/fa_fwd_splitkv_gfx950.hip behind aule.flash_attention_paged_query / aule_attention_paged_query_ex).

The judge is the fp64 oracle of the paged DECODE, one query row at a time: row i of the call is `paged_decode_f64` on
q[:, :, i] with the context lengths L - Sq + 1 + i (clamped at 0) and the same window -- the definition of the call, with no
oracle of its own.  Bounds are the project's forward bound fwd_tol(dtype, max |V|), as tests/test_gpu_paged.py and
tests/test_gpu_paged_fp8.py use it (FP8 caches: the oracle sees the dequantised caches, scale[hk] * float(code) in float64).
The LSE is judged against an fp64 log-sum-exp formed here from the gathered keys."""
import ctypes
import math

import numpy as np
import pytest

from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

CODE_8 = 0x50   # e4m3fn code of 8.0 (tests/test_gpu_paged_fp8.py): magnitudes 0 .. CODE_8 are the finite codes with |x| <= 8
LSE_ATOL = 1e-3


def _decode(codes_u8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(codes_u8)).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)


def _table(rng, B, bs, lens, num_blocks, extra_cols=2):
    """shuffled block table; the unused columns point at block 0"""
    nblk = [(n + bs - 1) // bs for n in lens]
    bt = np.zeros((B, max(max(nblk), 1) + extra_cols), dtype=np.int32)
    perm = rng.permutation(num_blocks)
    used = 0
    for b in range(B):
        bt[b, :nblk[b]] = perm[used:used + nblk[b]]
        used += nblk[b]
    return bt


class Problem:
    """Seeded inputs of one case: what the device sees (q, caches or codes + scales, table, lengths) and the float64 caches
    the oracle sees."""

    def __init__(self, seed, dtype, kind, B, Hq, Hkv, Sq, D, bs, lens, table_lens=None):
        rng = np.random.RandomState(seed)
        self.dtype, self.fp8, self.Sq, self.bs = dtype, kind == "fp8", Sq, bs
        table_lens = list(lens) if table_lens is None else table_lens
        num_blocks = sum((n + bs - 1) // bs for n in table_lens) + 3
        shape = (num_blocks, bs, Hkv, D)
        if self.fp8:
            self.q = quantize(0.25 * rng.randn(B, Hq, Sq, D).astype(np.float32), dtype)
            self.kdev, self.vdev = ((rng.randint(0, CODE_8 + 1, size=shape) | (rng.randint(0, 2, size=shape) << 7)).astype(np.uint8)
                                    for _ in range(2))
            self.ks, self.vs = rng.uniform(0.25, 2.0, Hkv), rng.uniform(0.25, 2.0, Hkv)
            self.K = _decode(self.kdev) * self.ks.reshape(1, 1, -1, 1)
            self.V = _decode(self.vdev) * self.vs.reshape(1, 1, -1, 1)
        else:
            self.q = quantize(rng.randn(B, Hq, Sq, D).astype(np.float32), dtype)
            self.kdev, self.vdev = (quantize(rng.randn(*shape).astype(np.float32), dtype) for _ in range(2))
            self.ks = self.vs = None
            self.K, self.V = self.kdev.astype(np.float64), self.vdev.astype(np.float64)
        self.bt = _table(rng, B, bs, table_lens, num_blocks)
        self.cl = np.array(lens, dtype=np.int32)
        self.vmax = float(np.abs(self.V).max())

    def device(self, torch):
        dt = torch_dtype(self.dtype)
        if self.fp8:
            kc, vc = (torch.from_numpy(x).cuda().view(torch.float8_e4m3fn) for x in (self.kdev, self.vdev))
            scales = dict(k_scale=torch.tensor(self.ks, dtype=torch.float32, device="cuda"),
                          v_scale=torch.tensor(self.vs, dtype=torch.float32, device="cuda"))
        else:
            kc, vc = (torch.from_numpy(x).to("cuda", dt) for x in (self.kdev, self.vdev))
            scales = {}
        return (torch.from_numpy(self.q).to("cuda", dt), kc, vc, torch.from_numpy(self.bt).cuda(), torch.from_numpy(self.cl).cuda()), scales

    def run(self, torch, window=-1, scale=None, return_lse=True):
        import aule
        args, scales = self.device(torch)
        return aule.flash_attention_paged_query(*args, scale=scale, window_size=window, return_lse=return_lse, **scales)

    def clamped_lens(self):
        return np.clip(self.cl.astype(np.int64), 0, self.bt.shape[1] * self.bs)

    def judge(self, oracle_mod, window=-1, scale=None):
        """[B, Hq, Sq, D]: row i = the decode oracle on q[:, :, i] with L - Sq + 1 + i keys"""
        L = self.clamped_lens()
        rows = [oracle_mod.paged_decode_f64(self.q[:, :, i], self.K, self.V, self.bt, np.maximum(L - self.Sq + 1 + i, 0), scale, window)
                for i in range(self.Sq)]
        return np.stack(rows, axis=2)

    def lse_f64(self, window=-1, scale=None):
        """[B, Hq, Sq] float64: ln sum_j exp(scale q_i . k_j) over the keys row i sees; -inf where it sees none"""
        B, Hq, Sq, D = self.q.shape
        Hkv = self.K.shape[2]
        scale = 1.0 / math.sqrt(D) if scale is None else scale
        L = self.clamped_lens()
        out = np.full((B, Hq, Sq), -np.inf)
        for b in range(B):
            n = int(L[b])
            if n == 0:
                continue
            j = np.arange(n)
            k = self.K[self.bt[b][j // self.bs], j % self.bs]                                    # [n, Hkv, D]
            s = np.einsum("hgid,nhd->hgin", self.q[b].astype(np.float64).reshape(Hkv, Hq // Hkv, Sq, D), k) * scale
            p = n - Sq + np.arange(Sq)
            see = j[None, :] <= p[:, None]
            if window > 0:
                see &= p[:, None] - j[None, :] < window
            s = np.where(see[None, None], s, -np.inf)
            m = s.max(axis=-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                lse = m + np.log(np.exp(s - np.where(np.isfinite(m), m, 0.0)[..., None]).sum(axis=-1))
            out[b] = np.where(np.isfinite(m), lse, -np.inf).reshape(Hq, Sq)
        return out


def _check(p, torch, oracle_mod, window, what):
    """output against the judge, LSE against the fp64 log-sum-exp; returns the two measured maxima"""
    out, lse = p.run(torch, window)
    torch.cuda.synchronize()
    out, lse = out.float().cpu().numpy(), lse.cpu().numpy().astype(np.float64)
    ref, lref = p.judge(oracle_mod, window), p.lse_f64(window)
    atol, rtol = fwd_tol(p.dtype, p.vmax)
    none = ~np.isfinite(lref)
    lerr = float(np.abs(lse[~none] - lref[~none]).max()) if (~none).any() else 0.0
    print("%s: max |out err| %.3g (atol %.3g), max |lse err| %.3g (bound %.3g), rows without a key %d"
          % (what, np.abs(out - ref).max(), atol, lerr, LSE_ATOL, int(none.sum())))
    assert_close(out, ref, atol, rtol, what)
    assert np.array_equal(np.isneginf(lse), none), "%s: lse must be -inf exactly where a row sees no key" % what
    assert not np.isnan(lse).any()
    assert bool((out[none] == 0).all()), "%s: a row that sees no key must be zeros" % what
    assert lerr <= LSE_ATOL, (what, lerr)
    return out, lse


CASES = [  # dtype, cache kind, B, Hq, Hkv, Sq, D, block_size, context lens, window
    ("bf16", "16", 2, 32, 8, 5, 128, 16, [2000, 37], -1),      # GQA 32/8 x 5 tokens: 20 packed rows in one tile
    ("fp16", "16", 2, 16, 2, 7, 64, 24, [1500, 100], -1),      # GQA 16/2 x 7: 56 rows in two tiles; the general address path
    ("bf16", "16", 1, 4, 1, 64, 64, 128, [1100], -1),          # MQA 4/1 x 64: 256 rows, a tile is half a head; blocks larger than a tile
    ("fp16", "16", 2, 8, 8, 3, 32, 1, [300, 2], -1),           # one token per block; a sequence shorter than the query (position < 0)
    ("fp16", "16", 2, 8, 4, 40, 128, 16, [2050, 1999], 1),     # windows: the lower edge of query 0 and of query 39 lie in different tiles
    ("bf16", "16", 2, 8, 4, 40, 128, 16, [2050, 1999], 16),
    ("fp16", "16", 2, 8, 4, 40, 128, 16, [2050, 1999], 300),
    ("bf16", "16", 3, 16, 4, 4, 64, 128, [2048, 129, 3], 300),
    ("bf16", "fp8", 2, 32, 8, 5, 128, 16, [2000, 37], -1),
    ("fp16", "fp8", 2, 16, 2, 7, 64, 24, [1500, 100], 16),
    ("bf16", "fp8", 1, 4, 1, 64, 32, 128, [1100], 300),
    ("fp16", "fp8", 2, 8, 8, 3, 128, 1, [300, 2], 1),
    ("bf16", "fp8", 2, 8, 4, 40, 64, 16, [2050, 1999], 300),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}-B{c[2]}-H{c[3]}kv{c[4]}-Sq{c[5]}-D{c[6]}-bs{c[7]}-w{c[9]}")
def test_rows_and_lse_vs_oracle(case, oracle_mod):
    """LSE: bound 1e-3 for inputs of unit scale -- fp32 sums of unrounded weights and two hardware transcendental steps leave
    errors of some 1e-5; the measured maximum of every case is printed (pytest -s) and has not been recorded here yet."""
    import torch
    dtype, kind, B, Hq, Hkv, Sq, D, bs, lens, window = case
    p = Problem(41, dtype, kind, B, Hq, Hkv, Sq, D, bs, lens)
    _check(p, torch, oracle_mod, window, "paged query")


@pytest.mark.parametrize("kind,window", [("16", -1), ("fp8", -1), ("16", 100), ("fp8", 100)])
def test_one_token_is_bit_identical_to_the_decode(kind, window):
    import torch
    import aule
    p = Problem(42, "bf16", kind, 4, 32, 8, 1, 128, 16, [1000, 37, 0, 1])
    (q, kc, vc, bt, cl), scales = p.device(torch)
    got = aule.flash_attention_paged_query(q, kc, vc, bt, cl, window_size=window, **scales)
    want = aule.flash_attention_paged_amd(q.squeeze(2), kc, vc, bt, cl, window_size=window, **scales)
    torch.cuda.synchronize()
    assert got.shape == (4, 32, 1, 128)
    assert torch.equal(got.squeeze(2), want)
    p = Problem(43, "fp16", kind, 2, 8, 2, 1, 64, 24, [700, 25])    # the general address path
    (q, kc, vc, bt, cl), scales = p.device(torch)
    got = aule.flash_attention_paged_query(q, kc, vc, bt, cl, window_size=window, **scales)
    want = aule.flash_attention_paged_amd(q.squeeze(2), kc, vc, bt, cl, window_size=window, **scales)
    torch.cuda.synchronize()
    assert torch.equal(got.squeeze(2), want)


@pytest.mark.parametrize("kind", ["16", "fp8"])
@pytest.mark.parametrize("lens", [[70], [70, 33, 5, 0]], ids=["L70", "L70-33-5-0"])
def test_fully_masked_tiles(lens, kind, oracle_mod):
    """Sq = 40 against 70 keys, one 32-key tile per wave: query 0 (position 30) sees nothing of tiles 1 and 2, so the waves
    of those tiles hold rows whose running maximum never leaves -inf.  With lengths 33, 5 and 0 some queries sit at negative
    positions: zeros, lse = -inf, and nothing in the whole output is a NaN or an infinity."""
    import torch
    B = len(lens)
    p = Problem(44, "fp16", kind, B, 2, 2, 40, 64, 16, lens, table_lens=[70] * B)
    out, lse = _check(p, torch, oracle_mod, -1, "fully masked tiles")
    assert np.isfinite(out).all()
    for b, n in enumerate(lens):
        dead = max(0, 40 - n)                     # queries at negative positions
        assert bool((out[b, :, :dead] == 0).all()) and bool(np.isneginf(lse[b, :, :dead]).all())
        assert bool(np.isfinite(lse[b, :, dead:]).all())
        if dead < 40:
            assert bool((out[b, :, dead:] != 0).any())


def test_context_len_beyond_the_block_table_is_clamped():
    """As the decode: a stale length is clamped on the device to what the table addresses (the query positions follow the
    clamped length); the table and the lengths may be CPU tensors."""
    import torch
    import aule
    torch.manual_seed(9)
    B, Hq, Hkv, Sq, D, bs, nb = 2, 8, 2, 6, 128, 16, 6
    q = torch.randn(B, Hq, Sq, D, device="cuda", dtype=torch.float16)
    kc = torch.randn(B * nb, bs, Hkv, D, device="cuda", dtype=torch.float16)
    vc = torch.randn_like(kc)
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)            # CPU on purpose
    full = torch.tensor([nb * bs, nb * bs], dtype=torch.int32)
    over = torch.tensor([nb * bs + 1000, 2 ** 30], dtype=torch.int32)
    ref, lref = aule.flash_attention_paged_query(q, kc, vc, bt, full, return_lse=True)
    got, lgot = aule.flash_attention_paged_query(q, kc, vc, bt, over, return_lse=True)
    neg = aule.flash_attention_paged_query(q, kc, vc, bt, torch.tensor([-5, -(2 ** 31)], dtype=torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(got, ref) and torch.equal(lgot, lref)
    assert bool((neg == 0).all())


@pytest.mark.parametrize("dtype,kind,window", [("bf16", "16", -1), ("fp16", "16", 100), ("bf16", "fp8", -1)])
def test_agrees_with_the_contiguous_bottom_right_forward(dtype, kind, window):
    """Equal lengths: the gathered K / V [B, Hkv, L, D] under flash_attention(causal="bottom-right") is the same problem,
    run by the tiled kernels.  Power-of-two FP8 scales, so the 16-bit expansion of the cache is exact."""
    import torch
    import aule
    B, Hq, Hkv, Sq, D, bs, n = 2, 16, 4, 12, 128, 16, 1000
    p = Problem(45, dtype, kind, B, Hq, Hkv, Sq, D, bs, [n] * B)
    if p.fp8:
        p.ks, p.vs = np.array([0.5, 2.0, 0.25, 1.0]), np.array([4.0, 0.125, 1.0, 0.5])
        p.K = _decode(p.kdev) * p.ks.reshape(1, 1, -1, 1)
        p.V = _decode(p.vdev) * p.vs.reshape(1, 1, -1, 1)
        p.vmax = float(np.abs(p.V).max())
    got = p.run(torch, window, return_lse=False)
    j = np.arange(n)
    dt = torch_dtype(dtype)
    K = torch.from_numpy(np.stack([p.K[p.bt[b][j // bs], j % bs] for b in range(B)])).to(dt).permute(0, 2, 1, 3).contiguous().cuda()
    V = torch.from_numpy(np.stack([p.V[p.bt[b][j // bs], j % bs] for b in range(B)])).to(dt).permute(0, 2, 1, 3).contiguous().cuda()
    assert np.array_equal(K.double().cpu().numpy(), np.stack([p.K[p.bt[b][j // bs], j % bs] for b in range(B)]).transpose(0, 2, 1, 3))
    dense = aule.flash_attention(torch.from_numpy(p.q).to("cuda", dt), K, V, causal="bottom-right", window_size=window)
    torch.cuda.synchronize()
    atol, rtol = fwd_tol(dtype, p.vmax)
    print("paged query vs contiguous: %.3g (atol %.3g)" % (float((got.float() - dense.float()).abs().max()), atol))
    assert_close(got.float().cpu().numpy(), dense.float().cpu().numpy(), atol, rtol, "paged query vs contiguous bottom-right")


def _capture(torch, fn, steps=3):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.graph(g):
        for _ in range(steps):
            outs.append(fn())
    return g, outs


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_capture_replays_bit_identical(kind):
    """As tests/test_gpu_graph.py does for the paged decode: no allocation and no synchronisation in the captured call."""
    import torch
    import aule
    p = Problem(46, "fp16", kind, 4, 32, 8, 4, 128, 16, [2048, 1000, 37, 2047])
    (q, kc, vc, bt, cl), scales = p.device(torch)
    fn = lambda: aule.flash_attention_paged_query(q, kc, vc, bt, cl, return_lse=True, **scales)   # noqa: E731
    eager, eager_lse = fn()
    torch.cuda.synchronize()
    g, outs = _capture(torch, fn)
    for _ in range(2):
        for o, l in outs:
            o.zero_(); l.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, eager) and torch.equal(l, eager_lse) for o, l in outs)
    # new lengths in the captured buffer: the replay reads them on the device
    cl.copy_(torch.tensor([5, 2048, 900, 0], device="cuda", dtype=torch.int32))
    want, want_lse = fn()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(outs[-1][0], want) and torch.equal(outs[-1][1], want_lse)


def _desc(torch, q, kc, vc, bt, cl, out, lse, scales):
    from aule import _capi
    B, Hq, Sq, D = q.shape
    d = _capi.PagedQueryDesc()
    d.struct_size = ctypes.sizeof(_capi.PagedQueryDesc)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    d.cache_dtype = 1 if scales else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim, d.seq_q = B, Hq, kc.shape[2], D, Sq
    d.block_size, d.max_blocks = kc.shape[1], bt.shape[1]
    d.scale, d.window_size, d.device = 0.0, -1, q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
    if scales:
        d.k_scale, d.v_scale = scales["k_scale"].data_ptr(), scales["v_scale"].data_ptr()
    return d


@pytest.mark.parametrize("kind", ["16", "fp8"])
def test_c_abi_directly(kind, oracle_mod):
    """aule_attention_paged_query_ex with a caller workspace of exactly the queried size and with none (equal results,
    nothing written past the buffer, right against the judge), with and without lse; -3 and an error text for what the
    descriptor checker refuses."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Problem(47, "bf16", kind, 3, 16, 4, 6, 128, 16, [900, 33, 2048])
    (q, kc, vc, bt, cl), scales = p.device(torch)
    B, Hq, Sq, _ = q.shape
    res = []
    for mode in ("exact", "none", "no-lse"):
        out = torch.empty_like(q)
        lse = torch.full((B, Hq, Sq), 7.0, device="cuda") if mode != "no-lse" else None
        d = _desc(torch, q, kc, vc, bt, cl, out, lse, scales)
        need = int(lib.aule_attention_paged_query_workspace_size(ctypes.byref(d)))
        assert need > 0
        buf = torch.full((need + 4096,), 0x5A, device="cuda", dtype=torch.uint8)
        if mode != "none":
            d.workspace, d.workspace_bytes = buf.data_ptr(), need
        assert lib.aule_attention_paged_query_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert bool((buf[need:] == 0x5A).all()), "wrote past the workspace it was given"
        if mode != "none":
            assert not bool((buf[:need] == 0x5A).all()), "did not use the workspace it was given"
        res.append((out, lse))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[1][1])
    atol, rtol = fwd_tol("bf16", p.vmax)
    assert_close(res[0][0].float().cpu().numpy(), p.judge(oracle_mod), atol, rtol, "paged query through the C-ABI")
    lerr = float(np.abs(res[0][1].cpu().numpy().astype(np.float64) - p.lse_f64()).max())
    assert lerr <= LSE_ATOL, lerr

    def refused(change, needle):
        d = _desc(torch, q, kc, vc, bt, cl, torch.empty_like(q), None, scales)
        change(d)
        assert lib.aule_attention_paged_query_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg

    refused(lambda d: setattr(d, "struct_size", 136), "struct_size")
    refused(lambda d: setattr(d, "dtype", 0), "fp16 or bf16")
    refused(lambda d: setattr(d, "cache_dtype", 2), "cache_dtype")
    refused(lambda d: setattr(d, "head_dim", 256), "head_dim 256")
    refused(lambda d: setattr(d, "heads_kv", 5), "divisible")
    refused(lambda d: setattr(d, "seq_q", 0), "seq_q 0")
    refused(lambda d: setattr(d, "seq_q", 65), "seq_q 65")
    refused(lambda d: setattr(d, "block_size", 0), "block_size")
    refused(lambda d: setattr(d, "max_blocks", 0), "block_size")
    refused(lambda d: setattr(d, "q", None), "null tensor pointer")
    refused(lambda d: setattr(d, "context_lens", None), "null tensor pointer")
    if scales:
        refused(lambda d: setattr(d, "k_scale", None), "scale pointer")
        refused(lambda d: setattr(d, "v_scale", None), "scale pointer")
    else:
        refused(lambda d: setattr(d, "k_scale", q.data_ptr()), "FP8 caches only")
