"""Attention sinks on the GPU: aule.flash_attention_varlen_sinks / _paged_prefill_sinks / _paged_query_sinks and the C entries behind them.

Judge: written here, torch fp64 on the CPU over the quantised inputs, per sequence and head -- the masked logits under the visibility
rule of csrc/fa_fwd_varlen_gfx950.hip restated in _visible (the paged entries are its bottom-right case), the sink column
concatenated, the softmax, the column dropped, times V; torch.autograd gives dq, dk, dv and dsinks.  It never goes through the library.
Bounds: out util.fwd_tol(dtype, max|V|), lse 1e-3 (the sinkless twins' bars), dq / dk / dv util.BWD_TOL as
tests/test_gpu_varlen.py::_check_grad applies it.  Rows that see no key: out == 0 and lse == sinks[h] exactly.

Sink logits per head cycle through -inf, -30, 0, ln(Lmax) + 0.5 and ln(Lmax) + 6, Lmax the largest number of keys a row of the case
sees (with N(0, 1) logits the fourth puts about half of the mass on the sink there, the fifth nearly all).  Two conditions are asserted
on the reference alone, so that a kernel that ignores the sinks cannot pass: the sink weight of the ln(Lmax) + 0.5 head at the row
with most keys lies in [0.2, 0.8], and max|out_ref(sinks) - out_ref(no sinks)| exceeds 20 x the forward tolerance.

dsinks: |got - ref| / max(1, max|ref|) against the fp64 reference, measured over the sixteen cases of test_backward_against_the_reference
on an MI355X (DESIGN.md 4 has the table): fp16 7.8e-5 .. 3.6e-4, bf16 3.9e-4 .. 2.0e-3 and one case at 4.0e-3 (heads 4 / 2, D = 128,
bottom-right, window 17: rows of at most 17 keys, so O is large and its bf16 rounding, which delta = rowsum(dO * O) inherits, is
2^-9 |O| sqrt(128) per row; over 241 owned rows that is the 0.03 observed on a gradient of 8.4).  The bar is 4 x the worst measured value
and never above BWD_TOL[dtype]'s atol: fp16 1.43e-3; bf16 4 x 4.0e-3 would be 1.6e-2, so the bar is the cap, 5e-3, which the worst
case meets with 20 % to spare and the other seven with a factor of 2.5 or more.  The inputs are seeded and the kernels are bit-reproducible,
so the figures do not move from run to run; a wrong reduction misses by O(1)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import hostile
from hostile import FRIENDLY, POISON, Arena
from util import BWD_TOL, fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

LSE_ATOL = 1e-3
CODE = {False: 0, True: 1, "bottom-right": 2}
NINF = float("-inf")
# query / key lengths: one row; 70 rows against 200 keys (four 64-key tiles, L > n); 130 = 130 (two 128-row blocks at g = 1, nine at
# g = 8); 40 rows against 25 keys (L < n: under bottom-right the first 15 rows see no key).  The third sequence arrives 140 long and is
# cut to max_seqlen_q = 130: its last 10 rows belong to nobody, as do 3 rows in front of the batch and 5 behind it.
NS_RAW, NS, LS = (1, 70, 140, 40), (1, 70, 130, 40), (1, 200, 130, 25)
MAX_SQ, MAX_SK, LEAD, TAIL = 130, 200, 3, 5
HEADS = [(8, 1, 64), (4, 2, 128)]
# |got - ref| / max(1, max|ref|) of dsinks, worst over the cases of test_backward_against_the_reference, per dtype (MI355X)
DSINKS_MEASURED = {"bf16": 4.016e-3, "fp16": 3.559e-4}
DSINKS_BAR = {dt: min(4 * m, BWD_TOL[dt][0]) for dt, m in DSINKS_MEASURED.items()}
assert all(DSINKS_MEASURED[dt] < DSINKS_BAR[dt] <= BWD_TOL[dt][0] for dt in DSINKS_BAR)


def _visible(n, L, code, window):
    """[n, L] bool: query i sits at pos = i (code 0, 1) or i + L - n (code 2); key j is visible iff (!code || j <= pos) and, with a
    window W > 0, pos - j < W"""
    import torch
    i = torch.arange(n)[:, None]
    j = torch.arange(L)[None, :]
    pos = i + (L - n if code == 2 else 0)
    vis = torch.ones(n, L, dtype=torch.bool)
    if code:
        vis &= j <= pos
    if window > 0:
        vis &= pos - j < window
    return vis


def _sink_values(Hq, lmax, rot=0):
    """head h takes entry (h + rot) % 5 of the cycle"""
    cycle = [NINF, -30.0, 0.0, math.log(lmax) + 0.5, math.log(lmax) + 6.0]
    return [cycle[(h + rot) % 5] for h in range(Hq)]


def _ref_seq(q, k, v, sinks, code, window, scale):
    """q [n, Hq, D], k / v [L, Hkv, D], sinks [Hq], all fp64 -> out [n, Hq, D] (differentiable), lse [n, Hq], sink weight [n, Hq]"""
    import torch
    n, Hq, _ = q.shape
    L, Hkv, _ = k.shape
    g = Hq // Hkv
    kk, vv = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    s = torch.einsum("nhd,lhd->hnl", q, kk) * scale
    s = s.masked_fill(~_visible(n, L, code, window)[None], NINF)
    z = torch.cat([s, sinks[:, None, None].expand(Hq, n, 1)], dim=-1)
    m = z.detach().amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(z - m)
    den = e.sum(dim=-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    out = torch.einsum("hnl,lhd->nhd", p[..., :L], vv)
    with torch.no_grad():
        lse = torch.where(den > 0, m + torch.log(den), torch.full_like(den, NINF))[..., 0].T
    return out, lse, p[..., L].detach().T


class Batch:
    """A packed batch: quantised inputs as fp64 CPU tensors, the owned ranges after the clamps, the sink logits.
    scale: None for 1 / sqrt(D) (scale_arg is what a call is given); rot: the cycle of sink logits starts that many entries in;
    sinks_dtype: the logits rounded to that storage dtype, which is what the judge then sees."""

    def __init__(self, seed, dtype, Hq, Hkv, D, code, window, ns=NS, ls=LS, ns_raw=NS_RAW, max_sq=MAX_SQ, lead=LEAD, tail=TAIL, scale=None,
                 rot=0, sinks_dtype=None):
        import torch
        gen = torch.Generator().manual_seed(seed)
        self.dtype, self.tdt, self.Hq, self.Hkv, self.D, self.code, self.window = dtype, torch_dtype(dtype), Hq, Hkv, D, code, window
        self.scale_arg, self.scale = scale, 1.0 / math.sqrt(D) if scale is None else scale
        self.cu_q = [lead + int(x) for x in np.concatenate([[0], np.cumsum(ns_raw)])]
        self.cu_k = [2 + int(x) for x in np.concatenate([[0], np.cumsum(ls)])]
        self.Tq, self.Tk = self.cu_q[-1] + tail, self.cu_k[-1] + 4
        self.max_sq, self.max_sk = max_sq, max(max(ls), 1)
        self.seqs = [(self.cu_q[b], min(ns_raw[b], max_sq), self.cu_k[b], ls[b]) for b in range(len(ns))]
        assert [s[1] for s in self.seqs] == list(ns)
        rnd = lambda *shape: torch.randn(*shape, generator=gen).to(self.tdt)   # noqa: E731
        self.q, self.k, self.v, self.dout = rnd(self.Tq, Hq, D), rnd(self.Tk, Hkv, D), rnd(self.Tk, Hkv, D), rnd(self.Tq, Hq, D)
        self.lmax = max(int(_visible(n, L, code, window).sum(dim=1).max()) if n and L else 0 for _, n, _, L in self.seqs)
        self.sinks = torch.tensor(_sink_values(Hq, max(self.lmax, 1), rot), dtype=torch.float32)
        if sinks_dtype is not None:
            self.sinks = self.sinks.to(torch_dtype(sinks_dtype)).float()
        self.vmax = float(self.v.float().abs().max())

    def owned(self):
        import torch
        o = torch.zeros(self.Tq, dtype=torch.bool)
        for sq, n, _, _ in self.seqs:
            o[sq:sq + n] = True
        return o

    def reference(self, sinks=None, grads=False, k=None, v=None):
        """out [Tq, Hq, D], lse, sink weight [Tq, Hq] (zeros / nan in unowned rows), seen [Tq, Hq] bool (the row sees a key), and with
        grads the fp64 dq, dk, dv, dsinks of sum(out * dout) over the owned rows"""
        import torch
        q = self.q.double().requires_grad_(grads)
        k = (self.k if k is None else k).double().requires_grad_(grads)
        v = (self.v if v is None else v).double().requires_grad_(grads)
        s = (self.sinks if sinks is None else sinks).double().requires_grad_(grads)
        out = torch.zeros(self.Tq, self.Hq, self.D, dtype=torch.float64)
        lse = torch.full((self.Tq, self.Hq), float("nan"), dtype=torch.float64)
        w = torch.zeros(self.Tq, self.Hq, dtype=torch.float64)
        seen = torch.zeros(self.Tq, self.Hq, dtype=torch.bool)
        pieces = []
        for sq, n, sk, L in self.seqs:
            o, l_, w_ = _ref_seq(q[sq:sq + n], k[sk:sk + L], v[sk:sk + L], s, self.code, self.window, self.scale)
            pieces.append((sq, n, o))
            out[sq:sq + n], lse[sq:sq + n], w[sq:sq + n] = o.detach(), l_, w_
            seen[sq:sq + n] = _visible(n, L, self.code, self.window).any(dim=1)[:, None]
        res = dict(out=out, lse=lse, w=w, seen=seen)
        if grads:
            loss = sum((o * self.dout[sq:sq + n].double()).sum() for sq, n, o in pieces)
            loss.backward()
            res.update(dq=q.grad, dk=k.grad, dv=v.grad, dsinks=s.grad)
        return res


@functools.lru_cache(maxsize=None)
def _batch(dtype, Hq, Hkv, D, causal, window, seed=11):
    return Batch(seed, dtype, Hq, Hkv, D, CODE[causal], window)


@functools.lru_cache(maxsize=None)
def _reference(dtype, Hq, Hkv, D, causal, window, grads=False):
    """computed once per case and shared; the tests do not write to it"""
    b = _batch(dtype, Hq, Hkv, D, causal, window)
    ref = b.reference(grads=grads)
    _sinks_matter(b, ref, b.reference(sinks=b.sinks.new_full(b.sinks.shape, NINF))["out"])
    return ref


def _sinks_matter(b, ref, plain_out, rows=None):
    """the two conditions on the reference alone"""
    import torch
    own = b.owned() if rows is None else rows
    atol, rtol = fwd_tol(b.dtype, b.vmax)
    nkeys = torch.zeros(b.Tq, dtype=torch.long)
    for sq, n, _, L in b.seqs:
        nkeys[sq:sq + n] = _visible(n, L, b.code, b.window).sum(dim=1)
    row = int(torch.where(own, nkeys, torch.full_like(nkeys, -1)).argmax())
    assert int(nkeys[row]) == b.lmax
    w = float(ref["w"][row, 3])
    assert 0.2 <= w <= 0.8, ("sink weight of the ln(Lmax) + 0.5 head at the row with most keys", w)
    gap = float((ref["out"][own] - plain_out[own]).abs().max())
    assert gap > 20 * (atol + rtol * float(ref["out"][own].abs().max())), gap


def _check_forward(b, ref, out, lse, what, rows=None):
    """owned rows against the reference; the rows that see no key exactly"""
    import torch
    own = b.owned() if rows is None else rows
    out, lse = out.detach().double().cpu(), lse.detach().double().cpu()
    atol, rtol = fwd_tol(b.dtype, b.vmax)
    err = (out[own] - ref["out"][own]).abs()
    assert torch.isfinite(out[own]).all(), what
    assert bool((err <= atol + rtol * ref["out"][own].abs()).all()), "%s: out off by %.3e" % (what, float(err.max()))
    fin = torch.isfinite(ref["lse"]) & own[:, None]
    lerr = (lse[fin] - ref["lse"][fin]).abs()
    assert bool((lerr <= LSE_ATOL).all()), "%s: lse off by %.3e" % (what, float(lerr.max()))
    blind = own[:, None] & ~ref["seen"]
    assert bool((out[blind] == 0).all()), what + ": a row without a key must be zero"
    want = b.sinks.double()[None, :].expand(b.Tq, b.Hq)
    assert torch.equal(lse[blind], want[blind]), what + ": lse of a row without a key must be sinks[h] exactly"
    print("%s: max|out err| %.3e (atol %.2e), max|lse err| %.3e, %d rows x heads without a key"
          % (what, float(err.max()), atol, float(lerr.max()) if lerr.numel() else 0.0, int(blind.sum())))
    return float(err.max()) if err.numel() else 0.0, float(lerr.max()) if lerr.numel() else 0.0


def _check_grad(got, ref, dtype, what, floor=0.0):
    """tests/test_gpu_varlen.py::_check_grad (floor: as there, 0 in this file)"""
    atol, rtol = BWD_TOL[dtype]
    ref = ref.numpy()
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    got = got.detach().double().cpu().numpy()
    assert np.isfinite(got).all(), what + ": non-finite gradient"
    err = np.abs(got - ref)
    bad = err > np.maximum(atol * scale + rtol * np.abs(ref), floor)
    assert not bad.any(), "%s: %d elements out of bound, max err %.3e (max|grad| %.3g)" % (what, int(bad.sum()), err.max(), scale)
    return float(err.max() / scale) if ref.size else 0.0


def _cuda(b):
    import torch
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device="cuda")   # noqa: E731
    return b.q.cuda(), b.k.cuda(), b.v.cuda(), b.sinks.cuda(), i32(b.cu_q), i32(b.cu_k)


VARLEN_CASES = [(dt, Hq, Hkv, D, causal, window) for (Hq, Hkv, D) in HEADS for dt in ("bf16", "fp16")
                for causal in (True, "bottom-right", False) for window in (-1, 17)]
_id = lambda c: "-".join(str(x) for x in c)   # noqa: E731


# ---- 1. forward against the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", VARLEN_CASES, ids=_id)
def test_varlen_forward_against_the_reference(case):
    import torch
    import aule
    dt, Hq, Hkv, D, causal, window = case
    b, ref = _batch(*case), _reference(*case)
    q, k, v, sinks, cu_q, cu_k = _cuda(b)
    out, lse = aule.flash_attention_varlen_sinks(q, k, v, sinks, cu_q, cu_k, b.max_sq, b.max_sk, causal=causal, window_size=window, return_lse=True)
    plain, plain_lse = aule.flash_attention_varlen(q, k, v, cu_q, cu_k, b.max_sq, b.max_sk, causal=causal, window_size=window, return_lse=True)
    torch.cuda.synchronize()
    _check_forward(b, ref, out, lse, "varlen " + _id(case))
    # 2b. with mixed sinks the -inf heads equal the sinkless entry bit for bit
    own = b.owned().cuda()
    for h in (h for h in range(Hq) if b.sinks[h] == NINF):
        assert torch.equal(out[own][:, h], plain[own][:, h]) and torch.equal(lse[own][:, h], plain_lse[own][:, h]), h
    assert not torch.equal(out[own][:, 3], plain[own][:, 3])


def test_varlen_forward_padded_head_dim():
    """D = 40 runs zero-padded to 64 through the public wrapper, sinks untouched by the padding"""
    import torch
    import aule
    b = Batch(5, "bf16", 4, 2, 40, 2, -1)
    ref = b.reference()
    _sinks_matter(b, ref, b.reference(sinks=b.sinks.new_full(b.sinks.shape, NINF))["out"])
    q, k, v, sinks, cu_q, cu_k = _cuda(b)
    out, lse = aule.flash_attention_varlen_sinks(q, k, v, sinks.to(torch.bfloat16), cu_q, cu_k, b.max_sq, b.max_sk, causal="bottom-right", return_lse=True)
    torch.cuda.synchronize()
    assert out.shape == (b.Tq, 4, 40)
    b.sinks = b.sinks.to(torch.bfloat16).float()          # (what the call was given)
    _check_forward(b, b.reference(), out, lse, "varlen D = 40, bf16 sinks")


class Paged:
    """the sequences of a Batch behind a paged cache: block size `bs`, the blocks handed out in a shuffled order, 16-bit or FP8 (per-head
    scales: aule.quantize_kv_cache_fp8 on the CPU; the reference reads the dequantised values).  device="cpu": the reference side alone"""

    def __init__(self, b, fp8, bs=16, seed=3, extra_cols=1, device="cuda"):
        import torch
        import aule
        self.b, self.fp8 = b, fp8
        nblk = [-(-L // bs) for _, _, _, L in b.seqs]
        self.bs, self.max_blocks = bs, max(nblk) + extra_cols
        order = torch.randperm(sum(nblk) + 2, generator=torch.Generator().manual_seed(seed)).tolist()
        kc = torch.zeros(len(order), bs, b.Hkv, b.D, dtype=b.tdt)
        vc = torch.zeros_like(kc)
        self.bt = torch.zeros((len(b.seqs), self.max_blocks), dtype=torch.int32)      # (entries past a sequence's blocks: a valid block)
        for i, (_, _, sk, L) in enumerate(b.seqs):
            for j in range(nblk[i]):
                blk = order.pop()
                self.bt[i, j] = blk
                rows = min(bs, L - j * bs)
                kc[blk, :rows], vc[blk, :rows] = b.k[sk + j * bs:sk + j * bs + rows], b.v[sk + j * bs:sk + j * bs + rows]
        self.cl = torch.tensor([L for _, _, _, L in b.seqs], dtype=torch.int32)
        self.scales = {}
        self.k_ref = self.v_ref = None
        if fp8:
            kc, ks = aule.quantize_kv_cache_fp8(kc)
            vc, vs = aule.quantize_kv_cache_fp8(vc)
            self.scales = dict(k_scale=ks.to(device), v_scale=vs.to(device))
            kd, vd = kc.float() * ks.view(1, 1, -1, 1), vc.float() * vs.view(1, 1, -1, 1)
            self.k_ref, self.v_ref = torch.zeros(b.Tk, b.Hkv, b.D), torch.zeros(b.Tk, b.Hkv, b.D)
            for i, (_, _, sk, L) in enumerate(b.seqs):
                for j in range(nblk[i]):
                    rows = min(bs, L - j * bs)
                    self.k_ref[sk + j * bs:sk + j * bs + rows] = kd[self.bt[i, j], :rows]
                    self.v_ref[sk + j * bs:sk + j * bs + rows] = vd[self.bt[i, j], :rows]
        self.kc, self.vc = kc.to(device), vc.to(device)

    def reference(self, **kw):
        return self.b.reference(k=self.k_ref, v=self.v_ref, **kw)


def _raw_prefill(torch, b, p, q_pad=0):
    """aule_attention_paged_prefill_sink_ex on the Batch b behind the Paged p, into out / lse pre-filled with 0xFF; q_pad > 0: q is a slice
    of a projection that much wider per token whose other columns hold NaN bits.  Returns (out, lse) over all Tq rows."""
    from aule import _capi
    lib = _capi.get_lib()
    w = b.Hq * b.D
    wide = torch.full((b.Tq, w + q_pad), -1, dtype=torch.int16, device="cuda").view(b.tdt)
    wide[:, :w] = b.q.cuda().view(b.Tq, w)
    out = torch.full((b.Tq, b.Hq, b.D), -1, dtype=torch.int16, device="cuda").view(b.tdt)
    lse = torch.full((b.Tq, b.Hq), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    bt, cl, cu, sinks = p.bt.cuda(), p.cl.cuda(), torch.tensor(b.cu_q, dtype=torch.int32, device="cuda"), b.sinks.cuda()
    d = _capi.PagedPrefillSinkDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = hostile.DTYPE_CODE[b.dtype], 1 if p.fp8 else 0
    d.batch, d.heads_q, d.heads_kv, d.head_dim = len(b.seqs), b.Hq, b.Hkv, b.D
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = p.bs, p.max_blocks, b.Tq, b.max_sq
    d.scale, d.window_size, d.device = 0.0 if b.scale_arg is None else b.scale_arg, b.window, torch.cuda.current_device()
    d.q_token_stride = w + q_pad
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out, d.lse = wide.data_ptr(), p.kc.data_ptr(), p.vc.data_ptr(), out.data_ptr(), lse.data_ptr()
    d.block_tables, d.context_lens, d.cu_seqlens_q, d.sinks = bt.data_ptr(), cl.data_ptr(), cu.data_ptr(), sinks.data_ptr()
    if p.fp8:
        d.k_scale, d.v_scale = p.scales["k_scale"].data_ptr(), p.scales["v_scale"].data_ptr()
    _capi.check(lib.aule_attention_paged_prefill_sink_ex(ctypes.byref(d)), "paged prefill sink")
    torch.cuda.synchronize()
    return out, lse


def _unowned_still_poisoned(torch, b, tensors):
    """the rows of no sequence still hold the 0xFF they were filled with"""
    free = ~b.owned().cuda()
    for name, t in tensors.items():
        assert bool((hostile.as_bytes(torch, t[free]) == POISON).all()), name + ": a row that belongs to no sequence was written"


def dsinks_model(b, ref):
    """(exact, model) [Hq] fp64 from the reference alone: dsinks[h] = -sum over the owned rows of w[row, h] * delta[row, h], w the sink
    weight and delta = rowsum(dO * O) -- with O in fp64, which is autograd's dsinks, and with O rounded to the storage dtype first, which is
    what a backward that reads the stored O computes (the dominant term of the kernel's error)"""
    own = b.owned()
    dout, w = b.dout.double()[own], ref["w"][own]
    exact = -(w * (dout * ref["out"][own]).sum(dim=-1)).sum(dim=0)
    model = -(w * (dout * ref["out"][own].to(b.tdt).double()).sum(dim=-1)).sum(dim=0)
    return exact, model


def grads_model(b, ref):
    """(dq, dk) fp64 from the reference alone: the gradient formula dS = P (dP - delta), dq = scale dS K, dk = scale dS^T Q with
    delta = rowsum(dO * O) taken from O rounded to the storage dtype, which is what the backward entry is given (dv = P^T dO does not read
    delta).  With the unrounded O the same formula is autograd's gradient, so both are returned: ((dq, dk) exact, (dq, dk) model)."""
    import torch

    def run(rounded):
        dq, dk = torch.zeros_like(ref["dq"]), torch.zeros_like(ref["dk"])
        g = b.Hq // b.Hkv
        for sq, n, sk, L in b.seqs:
            if n == 0 or L == 0:
                continue
            q, do = b.q[sq:sq + n].double(), b.dout[sq:sq + n].double()
            kk, vv = (x[sk:sk + L].double().repeat_interleave(g, dim=1) for x in (b.k, b.v))
            s = torch.einsum("nhd,lhd->hnl", q, kk) * b.scale
            vis = _visible(n, L, b.code, b.window)[None] & torch.isfinite(ref["lse"][sq:sq + n].T)[..., None]
            P = torch.where(vis, torch.exp(s - ref["lse"][sq:sq + n].T[..., None]), torch.zeros_like(s))
            O = ref["out"][sq:sq + n]
            delta = (do * (O.to(b.tdt).double() if rounded else O)).sum(dim=-1).T[..., None]
            dS = P * (torch.einsum("nhd,lhd->hnl", do, vv) - delta)
            dq[sq:sq + n] = torch.einsum("hnl,lhd->nhd", dS, kk) * b.scale
            dk[sk:sk + L] = (torch.einsum("hnl,nhd->lhd", dS, q) * b.scale).view(L, b.Hkv, g, b.D).sum(dim=2)
        return dq, dk
    return run(False), run(True)


PREFILL_CASES = [(dt, Hq, Hkv, D, window, fp8) for (Hq, Hkv, D) in HEADS for dt in ("bf16", "fp16") for window in (-1, 17) for fp8 in (False, True)]


@pytest.mark.parametrize("case", PREFILL_CASES, ids=_id)
def test_paged_prefill_forward_against_the_reference(case):
    """the bottom-right rule per sequence; 16-bit and FP8 caches (k_scale in the scores, not in the sink)"""
    import torch
    import aule
    dt, Hq, Hkv, D, window, fp8 = case
    b = _batch(dt, Hq, Hkv, D, "bottom-right", window)
    p = Paged(b, fp8)
    ref = p.reference() if fp8 else _reference(dt, Hq, Hkv, D, "bottom-right", window)
    if fp8:
        b.vmax, keep = float(p.v_ref.abs().max()), b.vmax
        _sinks_matter(b, ref, p.reference(sinks=b.sinks.new_full(b.sinks.shape, NINF))["out"])
    q, _, _, sinks, cu_q, _ = _cuda(b)
    args = (p.bt.cuda(), p.cl.cuda(), cu_q)
    out, lse = aule.flash_attention_paged_prefill_sinks(q, p.kc, p.vc, sinks, *args, max_seqlen_q=b.max_sq, window_size=window, return_lse=True, **p.scales)
    plain, plain_lse = aule.flash_attention_paged_prefill(q, p.kc, p.vc, *args, max_seqlen_q=b.max_sq, window_size=window, return_lse=True, **p.scales)
    torch.cuda.synchronize()
    try:
        _check_forward(b, ref, out, lse, "paged prefill " + _id(case))
    finally:
        if fp8:
            b.vmax = keep
    own = b.owned().cuda()
    for h in (h for h in range(Hq) if b.sinks[h] == NINF):
        assert torch.equal(out[own][:, h], plain[own][:, h]) and torch.equal(lse[own][:, h], plain_lse[own][:, h]), h


QUERY_CASES = [(dt, Hq, Hkv, D, window, fp8, Sq) for (Hq, Hkv, D) in HEADS for (dt, window) in (("bf16", -1), ("fp16", 17))
               for fp8 in (False, True) for Sq in (1, 5, 64)]


@pytest.mark.parametrize("case", QUERY_CASES, ids=_id)
def test_paged_query_forward_against_the_reference(case):
    """seq_q = 1 (the decode), 5 and 64 tokens at the end of contexts of 1, 200, 130 and 3 keys (shorter than seq_q: rows at negative
    positions see no key); the 16-bit cache merges through the workgroup-per-row combine, the FP8 cache through the wave-per-row one"""
    import torch
    import aule
    dt, Hq, Hkv, D, window, fp8, Sq = case
    ls = (1, 200, 130, 3)
    b = Batch(17, dt, Hq, Hkv, D, 2, window, ns=(Sq,) * 4, ls=ls, ns_raw=(Sq,) * 4, max_sq=Sq, lead=0, tail=0)
    p = Paged(b, fp8)
    ref = p.reference()
    if fp8:
        b.vmax = float(p.v_ref.abs().max())
    _sinks_matter(b, ref, p.reference(sinks=b.sinks.new_full(b.sinks.shape, NINF))["out"])
    q = b.q.view(4, Sq, Hq, D).permute(0, 2, 1, 3).contiguous().cuda()      # [B, Hq, Sq, D]
    bt, cl, sinks = p.bt.cuda(), p.cl.cuda(), b.sinks.cuda()
    out, lse = aule.flash_attention_paged_query_sinks(q, p.kc, p.vc, sinks, bt, cl, window_size=window, return_lse=True, **p.scales)
    plain, plain_lse = aule.flash_attention_paged_query(q, p.kc, p.vc, bt, cl, window_size=window, return_lse=True, **p.scales)
    torch.cuda.synchronize()
    flat = lambda o: o.permute(0, 2, 1, 3).reshape(4 * Sq, Hq, D)   # noqa: E731
    flat_lse = lambda x: x.permute(0, 2, 1).reshape(4 * Sq, Hq)     # noqa: E731
    _check_forward(b, ref, flat(out), flat_lse(lse), "paged query " + _id(case))
    for h in (h for h in range(Hq) if b.sinks[h] == NINF):
        assert torch.equal(out[:, h], plain[:, h]) and torch.equal(lse[:, h], plain_lse[:, h]), h


# ---- 2. exactness: sinks all -inf is the sinkless entry, bit for bit ----------------------------------------------------------------

@pytest.mark.parametrize("dt,Hq,Hkv,D", [("bf16", 8, 1, 64), ("fp16", 4, 2, 128)])
def test_all_minus_inf_sinks_equal_the_sinkless_entries_bit_for_bit(dt, Hq, Hkv, D):
    """out and lse, the rows without a key included (0 and -inf), for all three entries and both caches"""
    import torch
    import aule
    none = torch.full((Hq,), NINF, device="cuda")
    for causal, window in ((True, -1), ("bottom-right", 17), (False, -1)):
        b = _batch(dt, Hq, Hkv, D, causal, window)
        q, k, v, _, cu_q, cu_k = _cuda(b)
        own = b.owned().cuda()
        got = aule.flash_attention_varlen_sinks(q, k, v, none, cu_q, cu_k, b.max_sq, b.max_sk, causal=causal, window_size=window, return_lse=True)
        want = aule.flash_attention_varlen(q, k, v, cu_q, cu_k, b.max_sq, b.max_sk, causal=causal, window_size=window, return_lse=True)
        assert torch.equal(got[0][own], want[0][own]) and torch.equal(got[1][own], want[1][own]), (causal, window)
        if causal == "bottom-right":
            assert bool(torch.isinf(want[1][own]).any())       # the case has rows without a key
    b = _batch(dt, Hq, Hkv, D, "bottom-right", -1)
    q, _, _, _, cu_q, _ = _cuda(b)
    own = b.owned().cuda()
    for fp8 in (False, True):
        p = Paged(b, fp8)
        args = (p.bt.cuda(), p.cl.cuda(), cu_q)
        got = aule.flash_attention_paged_prefill_sinks(q, p.kc, p.vc, none, *args, max_seqlen_q=b.max_sq, return_lse=True, **p.scales)
        want = aule.flash_attention_paged_prefill(q, p.kc, p.vc, *args, max_seqlen_q=b.max_sq, return_lse=True, **p.scales)
        assert torch.equal(got[0][own], want[0][own]) and torch.equal(got[1][own], want[1][own]), fp8
        assert bool(torch.isinf(want[1][own]).any())
        for Sq in (1, 5, 64):
            qq = torch.randn(4, Hq, Sq, D, generator=torch.Generator().manual_seed(Sq)).to(b.tdt).cuda()
            got = aule.flash_attention_paged_query_sinks(qq, p.kc, p.vc, none, args[0], args[1], return_lse=True, **p.scales)
            want = aule.flash_attention_paged_query(qq, p.kc, p.vc, args[0], args[1], return_lse=True, **p.scales)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (fp8, Sq)
    torch.cuda.synchronize()


# ---- 3. backward (varlen) -------------------------------------------------------------------------------------------------------------

BWD_CASES = [(dt, Hq, Hkv, D, causal, window) for (dt, Hq, Hkv, D) in (("bf16", 8, 1, 64), ("fp16", 4, 2, 128), ("fp16", 8, 1, 64), ("bf16", 4, 2, 128))
             for (causal, window) in ((True, -1), ("bottom-right", 17), (False, -1), ("bottom-right", -1))]


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_backward_against_the_reference(case):
    """dq, dk, dv from the sinkless kernels given the sink-inclusive lse, dsinks from the reduction; two runs agree bit for bit in all
    four; the -inf heads get dsinks == 0 exactly"""
    import torch
    import aule
    dt, Hq, Hkv, D, causal, window = case
    b, ref = _batch(*case), _reference(*case, grads=True)
    runs = []
    for _ in range(2):
        q, k, v, sinks, cu_q, cu_k = _cuda(b)
        for t in (q, k, v, sinks):
            t.requires_grad_(True)
        out = aule.flash_attention_varlen_sinks(q, k, v, sinks, cu_q, cu_k, b.max_sq, b.max_sk, causal=causal, window_size=window)
        dout = torch.zeros_like(out)
        own = b.owned().cuda()
        dout[own] = b.dout.cuda()[own]
        out.backward(dout)
        runs.append((q.grad, k.grad, v.grad, sinks.grad))
    torch.cuda.synchronize()
    for a, c, name in zip(runs[0], runs[1], ("dq", "dk", "dv", "dsinks")):
        assert hostile.same_bits(torch, a, c), name + ": two runs differ"
    dq, dk, dv, ds = runs[0]
    worst = {n: _check_grad(g, ref[n], dt, "%s %s" % (n, _id(case))) for n, g in (("dq", dq), ("dk", dk), ("dv", dv))}
    assert ds.dtype == torch.float32 and ds.shape == (Hq,)
    rds = ref["dsinks"].numpy()
    rel = float(np.abs(ds.double().cpu().numpy() - rds).max() / max(1.0, np.abs(rds).max()))
    print("backward %s: dq %.3e dk %.3e dv %.3e of max(1, max|grad|); dsinks %.3e of max(1, max|ref| = %.3g), bar %.3e"
          % (_id(case), worst["dq"], worst["dk"], worst["dv"], rel, np.abs(rds).max(), DSINKS_BAR[dt]))
    assert np.abs(rds).max() > 0.5, "the reference gradient of the sinks is not trivial"
    assert torch.isfinite(ds).all() and rel <= DSINKS_BAR[dt], rel
    for h in range(Hq):
        if b.sinks[h] == NINF:
            assert float(ds[h]) == 0.0 and rds[h] == 0.0


def test_autograd_returns_the_parameters_dtype():
    """sinks as a bf16 nn.Parameter: the wrapper converts with .float(), so the gradient comes back in bf16"""
    import torch
    import aule
    b = _batch("bf16", 8, 1, 64, True, -1)
    q, k, v, sinks, cu_q, cu_k = _cuda(b)
    param = torch.nn.Parameter(sinks.clamp_min(-30.0).to(torch.bfloat16))
    out = aule.flash_attention_varlen_sinks(q, k, v, param, cu_q, cu_k, b.max_sq, b.max_sk)
    own = b.owned().cuda()
    out[own].float().square().sum().backward()
    torch.cuda.synchronize()
    assert param.grad is not None and param.grad.dtype == torch.bfloat16 and param.grad.shape == (8,)
    assert torch.isfinite(param.grad).all() and float(param.grad.abs().max()) > 0
    assert q.grad is None                                  # only the sinks asked for a gradient


# ---- 4. unowned rows and hostile memory ---------------------------------------------------------------------------------------------------

def _raw_run(torch, b, pattern):
    """forward and backward through the raw C entries on one arena filled with `pattern` (guards, outputs, workspace); returns the arena,
    the uploaded input bytes and the outputs"""
    from aule import _capi
    lib = _capi.get_lib()
    e = 2
    nq, nk = b.Tq * b.Hq * b.D * e, b.Tk * b.Hkv * b.D * e
    d = _capi.VarlenSinkBwdDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = hostile.DTYPE_CODE[b.dtype], len(b.seqs), b.Hq, b.Hkv, b.D
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = b.Tq, b.Tk, b.max_sq, b.max_sk
    d.causal, d.window_size, d.device = b.code, b.window, torch.cuda.current_device()
    d.scale = 0.0 if b.scale_arg is None else b.scale_arg
    d.q_token_stride, d.k_token_stride, d.v_token_stride = b.Hq * b.D, b.Hkv * b.D, b.Hkv * b.D
    ws = int(lib.aule_attention_varlen_sink_backward_workspace_size(ctypes.byref(d)))
    assert ws > (b.Tq * b.Hq * 4 + 255) // 256 * 256
    regions = [("q", nq, "in"), ("k", nk, "in"), ("v", nk, "in"), ("dout", nq, "in"), ("cu_q", 4 * len(b.cu_q), "in"), ("cu_k", 4 * len(b.cu_k), "in"),
               ("sinks", 4 * b.Hq, "in"), ("out", nq, "out"), ("lse", 4 * b.Tq * b.Hq, "out"), ("dq", nq, "out"), ("dk", nk, "out"), ("dv", nk, "out"),
               ("dsinks", 4 * b.Hq, "out"), ("ws", ws, "ws")]
    a = Arena(torch, regions, b.D * e)
    a.fill(pattern)
    dout = torch.zeros_like(b.dout)
    dout[b.owned()] = b.dout[b.owned()]
    ins = {n: a.upload(n, x) for n, x in (("q", b.q), ("k", b.k), ("v", b.v), ("dout", dout), ("cu_q", torch.tensor(b.cu_q, dtype=torch.int32)),
                                          ("cu_k", torch.tensor(b.cu_k, dtype=torch.int32)), ("sinks", b.sinks))}
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k, d.v, d.cu_seqlens_q, d.cu_seqlens_k = a.ptr("q"), a.ptr("k"), a.ptr("v"), a.ptr("cu_q"), a.ptr("cu_k")
    f = _capi.VarlenSinkDesc()
    ctypes.memmove(ctypes.byref(f), ctypes.byref(d), ctypes.sizeof(_capi.VarlenDesc))
    f.struct_size = ctypes.sizeof(f)
    f.out, f.lse, f.sinks = a.ptr("out"), a.ptr("lse"), a.ptr("sinks")
    _capi.check(lib.aule_attention_varlen_sink_forward_ex(ctypes.byref(f)), "sink forward")
    d.out, d.lse, d.dout, d.dq, d.dk, d.dv = a.ptr("out"), a.ptr("lse"), a.ptr("dout"), a.ptr("dq"), a.ptr("dk"), a.ptr("dv")
    d.workspace, d.workspace_bytes, d.sinks, d.dsinks = a.ptr("ws"), ws, a.ptr("sinks"), a.ptr("dsinks")
    _capi.check(lib.aule_attention_varlen_sink_backward_ex(ctypes.byref(d)), "sink backward")
    torch.cuda.synchronize()
    return a, ins


@pytest.mark.parametrize("dt,Hq,Hkv,D,causal,window", [("bf16", 8, 1, 64, "bottom-right", -1), ("fp16", 4, 2, 128, True, 17)])
def test_unowned_rows_and_hostile_memory(dt, Hq, Hkv, D, causal, window):
    """One arena per run, guard bands around every tensor.  Friendly run: everything that is not an input starts as zeros.  Hostile run:
    it starts as 0xFF -- NaN in out, lse, the delta workspace and the partials, in the rows no sequence owns and all around sinks and
    dsinks.  dsinks is finite and the friendly run's bit for bit (the reduction walks owned rows only); exactly heads_q floats of it are
    written and of sinks read (the bands around them are intact, the result does not depend on them); the unowned rows of out and lse
    keep their poison; no input and no guard is touched."""
    import torch
    b = _batch(dt, Hq, Hkv, D, causal, window)
    ref = _reference(dt, Hq, Hkv, D, causal, window, grads=True)
    clean, _ = _raw_run(torch, b, FRIENDLY)
    dirty, ins = _raw_run(torch, b, POISON)
    for a in (clean, dirty):
        assert a.guards_intact(), a.damage()
    for n, original in ins.items():
        assert dirty.unchanged(n, original), n
    ds_clean, ds_dirty = clean.view("dsinks", torch.float32, (Hq,)), dirty.view("dsinks", torch.float32, (Hq,))
    assert torch.isfinite(ds_dirty).all() and hostile.same_bits(torch, ds_clean, ds_dirty)
    rds = ref["dsinks"].numpy()
    assert np.abs(ds_dirty.double().cpu().numpy() - rds).max() / max(1.0, np.abs(rds).max()) <= DSINKS_BAR[dt]
    own = b.owned().cuda()
    for name, dtype, shape in (("out", b.tdt, (b.Tq, Hq, D)), ("lse", torch.float32, (b.Tq, Hq)), ("dq", b.tdt, (b.Tq, Hq, D))):
        c, x = clean.view(name, dtype, shape), dirty.view(name, dtype, shape)
        assert hostile.same_bits(torch, c[own], x[own]), name
        assert bool((hostile.as_bytes(torch, x[~own]) == POISON).all()), name + ": an unowned row was written"
        assert bool((hostile.as_bytes(torch, c[~own]) == FRIENDLY).all()), name + ": an unowned row was written"
    _check_forward(b, ref, dirty.view("out", b.tdt, (b.Tq, Hq, D)), dirty.view("lse", torch.float32, (b.Tq, Hq)), "hostile " + dt)


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------------------

def test_capture_replays_with_the_current_sinks():
    """the kernel reads sinks on every launch and nothing copies it to the host: a captured paged-prefill sink call, replayed after
    sinks was overwritten in place, equals a fresh call with the new values bit for bit"""
    import torch
    import aule
    b = _batch("bf16", 8, 1, 64, "bottom-right", -1)
    p = Paged(b, False)
    q, _, _, sinks, cu_q, _ = _cuda(b)
    bt, cl = p.bt.cuda(), p.cl.cuda()
    fn = lambda: aule.flash_attention_paged_prefill_sinks(q, p.kc, p.vc, sinks, bt, cl, cu_q, max_seqlen_q=b.max_sq, return_lse=True)   # noqa: E731
    own = b.owned().cuda()
    eager, eager_lse = (t.clone() for t in fn())
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
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[own], eager[own]) and torch.equal(lse[own], eager_lse[own])
    sinks.copy_(torch.tensor([1.5, NINF, 4.0, -2.0, 0.25, 9.0, NINF, 3.0], device="cuda"))
    want, want_lse = fn()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(want[own], eager[own])
    assert torch.equal(out[own], want[own]) and torch.equal(lse[own], want_lse[own])
