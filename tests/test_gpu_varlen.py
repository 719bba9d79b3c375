"""Variable-length packed batches on the GPU: aule_attention_varlen_forward_ex / _backward_ex and aule.flash_attention_varlen.

Judge: per sequence, oracle.np_fwd_f64 / np_bwd_f64 on the quantised inputs of that sequence reshaped to [1, H, S, D], with the same
causal code and window.  The sequence bounds come from the clamp rule of include/aule.h restated here (_clamp); the rows of a
sequence that see no key (a prefix under the bottom-right rule with L < n, a suffix under a window with L < n, everything with
L = 0) are checked directly against the rule -- out = 0, lse = -inf, dq = 0 exactly -- and the oracle judges the remaining rows, whose
own visibility mask is asserted equal to the rule's.  Bounds: util.fwd_tol(dtype, max|V|), LSE within 1e-3, util.BWD_TOL scaled by
max(1, max|grad|) as tests/test_gpu_d256.py::_check_grad; the achieved maxima are printed.  Every launch goes to buffers pre-filled
with 0xFF, and the rows no sequence owns must still hold it afterwards."""
import ctypes

import numpy as np
import pytest

import hostile
from hostile import POISON, Arena, same_bits
from util import BWD_TOL, assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

LSE_ATOL = 1e-3
CODE = {False: 0, True: 1, "bottom-right": 2}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
# query and key lengths that cross the 32-row wave, the 128-row block (32 tokens at g = 4), the 64-key tile and the 128-key block,
# paired so that L < n, L > n, L = n, n = 0 and L = 0 all occur
NS = [0, 1, 31, 33, 129, 200, 200, 1]
LS = [63, 0, 257, 1, 130, 65, 257, 1]


def _clamp(cu, b, total, cap):
    s = min(max(int(cu[b]), 0), total)
    e = min(max(int(cu[b + 1]), s), total)
    return s, min(e - s, cap)


def _visible(n, L, code, window):
    """[n, L] bool: the rule of include/aule.h"""
    i = np.arange(n)[:, None]
    j = np.arange(L)[None, :]
    pos = i + (L - n if code == 2 else 0)
    vis = np.ones((n, L), dtype=bool)
    if code:
        vis &= j <= pos
    if window > 0:
        vis &= pos - j < window
    return vis


class Packed:
    """A packed batch: q / dout [Tq, Hq, D], k / v [Tk, Hkv, D] (quantised fp32 arrays), offsets and maxima as the entry reads them."""

    def __init__(self, seed, dtype, Hq, Hkv, D, ns, ls, lead=(0, 0), tail=(0, 0), max_sq=None, max_sk=None, cu_q=None, cu_k=None,
                 Tq=None, Tk=None):
        rng = np.random.RandomState(seed)
        self.dtype, self.Hq, self.Hkv, self.D = dtype, Hq, Hkv, D
        self.cu_q = np.asarray(cu_q if cu_q is not None else lead[0] + np.concatenate([[0], np.cumsum(ns)]), dtype=np.int64)
        self.cu_k = np.asarray(cu_k if cu_k is not None else lead[1] + np.concatenate([[0], np.cumsum(ls)]), dtype=np.int64)
        self.B = len(self.cu_q) - 1
        self.Tq = Tq if Tq is not None else int(self.cu_q[-1]) + tail[0]
        self.Tk = Tk if Tk is not None else int(self.cu_k[-1]) + tail[1]
        self.q = quantize(rng.randn(self.Tq, Hq, D), dtype)
        self.k = quantize(rng.randn(self.Tk, Hkv, D), dtype)
        self.v = quantize(rng.randn(self.Tk, Hkv, D), dtype)
        self.dout = quantize(rng.randn(self.Tq, Hq, D), dtype)
        self.max_sq = max_sq if max_sq is not None else max(1, max(ns))
        self.max_sk = max_sk if max_sk is not None else max(1, max(ls))

    def sequences(self):
        """[(s_q, n, s_k, L)] after the clamps"""
        out = []
        for b in range(self.B):
            sq, n = _clamp(self.cu_q, b, self.Tq, min(self.max_sq, self.Tq))
            sk, L = _clamp(self.cu_k, b, self.Tk, min(self.max_sk, self.Tk))
            out.append((sq, n, sk, L))
        return out

    def owned(self):
        oq, ok = np.zeros(self.Tq, dtype=bool), np.zeros(self.Tk, dtype=bool)
        for sq, n, sk, L in self.sequences():
            assert not oq[sq:sq + n].any() and not ok[sk:sk + L].any(), "the test's sequences overlap"
            oq[sq:sq + n] = True
            ok[sk:sk + L] = True
        return oq, ok

    def alone(self, b):
        """sequence b as a batch of its own (the arrays sliced, offsets from 0)"""
        sq, n, sk, L = self.sequences()[b]
        p = Packed.__new__(Packed)
        p.dtype, p.Hq, p.Hkv, p.D, p.B = self.dtype, self.Hq, self.Hkv, self.D, 1
        p.q, p.dout, p.k, p.v = self.q[sq:sq + n], self.dout[sq:sq + n], self.k[sk:sk + L], self.v[sk:sk + L]
        p.cu_q, p.cu_k, p.Tq, p.Tk = np.array([0, n]), np.array([0, L]), n, L
        p.max_sq, p.max_sk = max(n, 1), max(L, 1)
        return p


def _i32(a):
    return np.clip(np.asarray(a, dtype=np.int64), I32_MIN, I32_MAX).astype(np.int32)


def _launch(torch, lib, p, ptr, causal, window, ws_bytes, backward=True, strides=None, scale=0.0):
    """forward, then backward, on the pointers in `ptr` (name -> address); strides: the token strides of q, k, v in elements (None: contiguous)"""
    from aule import _capi
    code = CODE[causal]

    def problem(d):
        d.struct_size = ctypes.sizeof(d)
        d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = hostile.DTYPE_CODE[p.dtype], p.B, p.Hq, p.Hkv, p.D
        d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = p.Tq, p.Tk, p.max_sq, p.max_sk
        d.scale, d.causal, d.window_size, d.device = scale, code, window, torch.cuda.current_device()
        d.q_token_stride, d.k_token_stride, d.v_token_stride = strides or (p.Hq * p.D, p.Hkv * p.D, p.Hkv * p.D)
        d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for n in ("q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse"):
            setattr(d, n, ptr[n])
        return d

    _capi.check(lib.aule_attention_varlen_forward_ex(ctypes.byref(problem(_capi.VarlenDesc()))), "varlen forward")
    if backward:
        d = problem(_capi.VarlenBwdDesc())
        assert int(lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d))) == ws_bytes
        for n in ("dout", "dq", "dk", "dv"):
            setattr(d, n, ptr[n])
        d.workspace, d.workspace_bytes = ptr["workspace"], ws_bytes
        _capi.check(lib.aule_attention_varlen_backward_ex(ctypes.byref(d)), "varlen backward")


def _ws_bytes(p):
    return (p.Tq * p.Hq * 4 + 255) // 256 * 256


class Run:
    """the batch on the device, outputs and workspace pre-filled with 0xFF; launch() runs forward and backward into them.
    strided: q, k and v with three DIFFERENT token strides -- q and k rows in buffers of their own, 16 and 8 elements wider than a
    token, v the second half of a [Tk, 2 Hkv, D] tensor -- and NaN bits in every element between the rows."""

    def __init__(self, torch, p, strided=False):
        tdt = torch_dtype(p.dtype)
        self.torch, self.p, self.strides = torch, p, None
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
        self.q, self.k, self.v, self.dout = up(p.q), up(p.k), up(p.v), up(p.dout)
        if strided:
            wq, wk, wv = p.Hq * p.D + 16, p.Hkv * p.D + 8, 2 * p.Hkv * p.D
            self.strides = (wq, wk, wv)
            nan = lambda rows, width: torch.full((rows, width * 2), POISON, dtype=torch.uint8, device="cuda").view(tdt)   # noqa: E731
            bq, bk, bv = nan(p.Tq, wq), nan(p.Tk, wk), nan(p.Tk, wv)
            bq[:, :p.Hq * p.D] = self.q.reshape(p.Tq, -1)
            bk[:, :p.Hkv * p.D] = self.k.reshape(p.Tk, -1)
            bv[:, p.Hkv * p.D:] = self.v.reshape(p.Tk, -1)
            self.q, self.k, self.v = bq, bk, bv[:, p.Hkv * p.D:]     # (data_ptr() of the slice: the first v row)
        self.cu_q, self.cu_k = (torch.from_numpy(_i32(c)).cuda() for c in (p.cu_q, p.cu_k))
        poison = lambda shape, dt: torch.full(shape, POISON, dtype=torch.uint8, device="cuda").view(dt)   # noqa: E731
        self.out, self.dq = (poison((p.Tq, p.Hq, p.D * 2), tdt) for _ in range(2))
        self.dk, self.dv = (poison((p.Tk, p.Hkv, p.D * 2), tdt) for _ in range(2))
        self.lse = poison((p.Tq, p.Hq * 4), torch.float32)
        self.ws = torch.full((max(_ws_bytes(p), 16),), POISON, dtype=torch.uint8, device="cuda")

    def launch(self, causal, window, backward=True, scale=None):
        from aule import _capi
        names = ("q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "dout", "dq", "dk", "dv")
        tensors = (self.q, self.k, self.v, self.cu_q, self.cu_k, self.out, self.lse, self.dout, self.dq, self.dk, self.dv)
        ptr = {n: t.data_ptr() for n, t in zip(names, tensors)}
        ptr["workspace"] = self.ws.data_ptr()
        _launch(self.torch, _capi.get_lib(), self.p, ptr, causal, window, _ws_bytes(self.p), backward, self.strides, 0.0 if scale is None else scale)
        return self

    def results(self):
        self.torch.cuda.synchronize()
        return {n: getattr(self, n) for n in ("out", "lse", "dq", "dk", "dv")}


def _check_grad(got, ref, dtype, what, floor=0.0):
    """tests/test_gpu_d256.py::_check_grad; floor: an absolute error allowed whatever the element (the randomised draws pass 4 x the
    error of the fp64 gradient that reads O rounded to storage; 0 everywhere else)"""
    atol, rtol = BWD_TOL[dtype]
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), what + ": non-finite gradient"
    err = np.abs(got - ref)
    bad = err > np.maximum(atol * scale + rtol * np.abs(ref), floor)
    assert not bad.any(), "%s: %d elements out of bound, max err %.3e (max|grad| %.3g)" % (what, int(bad.sum()), err.max(), scale)
    return float(err.max() / scale) if ref.size else 0.0


def _np(t):
    return t.detach().float().cpu().numpy()


def _judge(p, res, oracle, causal, window, what, backward=True, scale=None):
    """res: name -> tensor (out, lse, dq, dk, dv over the whole packed axes).  Checks every owned row; prints the maxima and returns them."""
    code = CODE[causal]
    out, lse = _np(res["out"]), _np(res["lse"])
    if backward:
        dq, dk, dv = _np(res["dq"]), _np(res["dk"]), _np(res["dv"])
    worst = dict(out=0.0, lse=0.0, dq=0.0, dk=0.0, dv=0.0)
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        tag = "%s seq %d (n %d, L %d)" % (what, b, n, L)
        vis = _visible(n, L, code, window)
        seen = vis.any(axis=1)
        rows = np.flatnonzero(seen)
        a, e = (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)
        assert seen[a:e].all(), "the rows that see a key are one range"
        blind = np.r_[sq:sq + a, sq + e:sq + n]
        assert (out[blind] == 0).all() and (lse[blind] == -np.inf).all(), tag + ": a row without a visible key must be zeros and -inf"
        if backward:
            assert (dq[blind] == 0).all(), tag + ": dq of a row without a visible key must be zero"
        if e == a:
            if backward:
                assert (dk[sk:sk + L] == 0).all() and (dv[sk:sk + L] == 0).all(), tag + ": no query sees these keys, dk = dv = 0"
            continue
        # the rows a .. e - 1 against all L keys: the oracle's own mask must be the rule's
        sub = causal if not (code == 2 and L <= e - a) else True
        assert np.array_equal(oracle._vis_mask(e - a, L, sub, window), vis[a:e]), tag + ": the judge's sub-problem is another problem"
        t = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2))[None]   # noqa: E731
        qs, ks, vs, ds = t(p.q[sq + a:sq + e]), t(p.k[sk:sk + L]), t(p.v[sk:sk + L]), t(p.dout[sq + a:sq + e])
        ro, rl = oracle.np_fwd_f64(qs, ks, vs, causal=sub, scale=scale, window=window)
        atol, rtol = fwd_tol(p.dtype, np.abs(vs).max())
        got = out[sq + a:sq + e].transpose(1, 0, 2)[None]
        assert_close(got, ro, atol, rtol, tag + " out")
        assert_close(lse[sq + a:sq + e].T[None], rl, LSE_ATOL, 0.0, tag + " lse")
        worst["out"] = max(worst["out"], float(np.abs(got - ro).max()))
        worst["lse"] = max(worst["lse"], float(np.abs(lse[sq + a:sq + e].T[None] - rl).max()))
        if backward:
            rq, rk, rv = oracle.np_bwd_f64(qs, ks, vs, ds, causal=sub, scale=scale, window=window)
            worst["dq"] = max(worst["dq"], _check_grad(dq[sq + a:sq + e].transpose(1, 0, 2)[None], rq, p.dtype, tag + " dq"))
            worst["dk"] = max(worst["dk"], _check_grad(dk[sk:sk + L].transpose(1, 0, 2)[None], rk, p.dtype, tag + " dk"))
            worst["dv"] = max(worst["dv"], _check_grad(dv[sk:sk + L].transpose(1, 0, 2)[None], rv, p.dtype, tag + " dv"))
    print("%s: max|err| out %.3e lse %.3e; of max(1, max|grad|): dq %.2e dk %.2e dv %.2e"
          % (what, worst["out"], worst["lse"], worst["dq"], worst["dk"], worst["dv"]))
    return worst


def _unowned_still_poisoned(torch, p, res):
    oq, ok = (torch.from_numpy(~m).cuda() for m in p.owned())
    for n, mask in (("out", oq), ("lse", oq), ("dq", oq), ("dk", ok), ("dv", ok)):
        rows = res[n][mask]
        assert bool((rows.reshape(-1).view(torch.uint8) == POISON).all()), n + ": a row that belongs to no sequence was written"


# dtype, Hq, Hkv, D, causal, window: every (dtype, D), g = 1, 4, 8 (MQA) and 3 heads without grouping, the three causal modes, windows 1, 17, 100
CASES = [
    ("bf16", 8, 2, 128, True, -1),
    ("fp16", 8, 2, 64, False, -1),
    ("bf16", 8, 1, 32, "bottom-right", -1),
    ("fp16", 2, 2, 128, "bottom-right", 17),
    ("bf16", 4, 1, 64, True, 1),
    ("fp16", 8, 1, 32, False, 100),
    ("bf16", 2, 2, 32, True, 100),
    ("fp16", 4, 1, 128, False, 17),
    ("bf16", 8, 1, 128, "bottom-right", 100),
    ("fp16", 3, 3, 64, True, -1),
    ("bf16", 4, 4, 64, "bottom-right", 1),
    ("fp16", 8, 2, 32, True, 17),
]
_case_id = lambda c: "%s-H%dkv%d-D%d-%s-w%d" % (c[0], c[1], c[2], c[3], {False: "full", True: "causal", "bottom-right": "br"}[c[4]], c[5])   # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_forward_and_backward_against_the_oracle(case, oracle_mod):
    """the mixed batch with a lead offset (cu[0] = 3 / 2) and tail rows behind the last sequence (5 / 7)"""
    import torch
    dtype, Hq, Hkv, D, causal, window = case
    p = Packed(11, dtype, Hq, Hkv, D, NS, LS, lead=(3, 2), tail=(5, 7))
    res = Run(torch, p).launch(causal, window).results()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, window, _case_id(case))


@pytest.mark.parametrize("case", [CASES[8], CASES[11], CASES[5]], ids=_case_id)
def test_a_sequence_alone_is_bit_identical_to_the_same_sequence_in_the_batch(case):
    import torch
    dtype, Hq, Hkv, D, causal, window = case
    p = Packed(12, dtype, Hq, Hkv, D, NS, LS, lead=(3, 2), tail=(5, 7))
    batch = Run(torch, p).launch(causal, window).results()
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        if n + L == 0:
            continue
        one = Run(torch, p.alone(b)).launch(causal, window).results()
        for name in ("out", "lse", "dq"):
            assert same_bits(torch, one[name], batch[name][sq:sq + n]), "seq %d: %s differs between alone and in the batch" % (b, name)
        for name in ("dk", "dv"):
            assert same_bits(torch, one[name], batch[name][sk:sk + L]), "seq %d: %s differs between alone and in the batch" % (b, name)


@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5]], ids=_case_id)
def test_three_different_token_strides_through_the_c_entry(case):
    """q, k and v each with a token stride of its own (a kernel that read one tensor with another's stride would read the NaN bits
    between the rows): every output bit-identical to the contiguous run"""
    import torch
    dtype, Hq, Hkv, D, causal, window = case
    p = Packed(20, dtype, Hq, Hkv, D, NS, LS, lead=(3, 2), tail=(5, 7))
    want = Run(torch, p).launch(causal, window).results()
    got = Run(torch, p, strided=True).launch(causal, window).results()
    for name in want:
        assert same_bits(torch, got[name], want[name]), name + " depends on the token strides"


@pytest.mark.parametrize("dtype,Hq,Hkv,D,causal", [("bf16", 8, 2, 128, True), ("fp16", 4, 1, 64, "bottom-right"), ("bf16", 2, 2, 32, False)])
def test_a_window_that_masks_nothing_equals_no_window(dtype, Hq, Hkv, D, causal):
    """window_size = INT32_MAX ("effectively off"), and the largest window the kernels still run with (one below
    min(max_seqlen_q, total_q) + min(max_seqlen_k, total_k)): forward and backward bit-identical to window_size = -1, with L < n and
    L > n under every causal mode (bottom-right with L < n puts rows at negative positions)"""
    import torch
    p = Packed(21, dtype, Hq, Hkv, D, NS, LS, lead=(3, 2), tail=(5, 7))
    want = Run(torch, p).launch(causal, -1).results()
    assert bool(want["dk"][torch.from_numpy(p.owned()[1]).cuda()].any())
    for window in (I32_MAX, min(p.max_sq, p.Tq) + min(p.max_sk, p.Tk) - 1, 2 ** 30):
        got = Run(torch, p).launch(causal, window).results()
        for name in want:
            assert same_bits(torch, got[name], want[name]), "%s differs from the no-window result at window_size = %d" % (name, window)


@pytest.mark.parametrize("causal,window", [(True, -1), ("bottom-right", 17), (False, -1)])
def test_max_seqlen_cuts_a_sequence_to_its_first_tokens(causal, window, oracle_mod):
    """max_seqlen_q = 40 and max_seqlen_k = 70 below the longest sequences: n and L are cut, the rows behind the cut are not written"""
    import torch
    p = Packed(13, "bf16", 8, 2, 64, NS, LS, lead=(1, 0), tail=(2, 3), max_sq=40, max_sk=70)
    assert [s[1] for s in p.sequences()] == [0, 1, 31, 33, 40, 40, 40, 1] and [s[3] for s in p.sequences()] == [63, 0, 70, 1, 70, 65, 70, 1]
    res = Run(torch, p).launch(causal, window).results()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, window, "max_seqlen cut")


@pytest.mark.parametrize("dtype,Hq,Hkv,D,n,L,causal,window", [("bf16", 4, 2, 64, 160, 160, True, -1), ("fp16", 8, 1, 128, 70, 200, "bottom-right", -1),
                                                            ("bf16", 4, 4, 32, 97, 97, False, 50)])
def test_equal_lengths_agree_with_the_dense_entry(dtype, Hq, Hkv, D, n, L, causal, window):
    """aule.flash_attention on the transposed tensors: two 16-bit results of the same problem (fwd_tol with sides = 2; gradients
    within BWD_TOL scaled by max(1, max|grad|))"""
    import torch
    import aule
    B = 3
    p = Packed(14, dtype, Hq, Hkv, D, [n] * B, [L] * B)
    res = Run(torch, p).launch(causal, window).results()
    tdt = torch_dtype(dtype)
    dense = lambda a, S, H: torch.from_numpy(a).to("cuda", tdt).reshape(B, S, H, D).transpose(1, 2).contiguous().requires_grad_(True)   # noqa: E731
    q, k, v = dense(p.q, n, Hq), dense(p.k, L, Hkv), dense(p.v, L, Hkv)
    out = aule.flash_attention(q, k, v, causal=causal, window_size=window)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dense(p.dout, n, Hq).detach())
    torch.cuda.synchronize()
    packed = lambda x: _np(x.transpose(1, 2).reshape(-1, x.shape[1], D))   # noqa: E731
    atol, rtol = fwd_tol(dtype, np.abs(p.v).max(), sides=2)
    assert_close(_np(res["out"]), packed(out), atol, rtol, "out against the dense entry")
    print("max|out - dense| %.3e" % np.abs(_np(res["out"]) - packed(out)).max())
    for name, ref in (("dq", dq), ("dk", dk), ("dv", dv)):
        print("%s against the dense entry: %.2e of max(1, max|grad|)" % (name, _check_grad(_np(res[name]), packed(ref).astype(np.float64), dtype, name)))


@pytest.mark.parametrize("dtype,Hq,Hkv,D,causal,window", [("bf16", 8, 2, 64, True, -1), ("fp16", 4, 1, 128, "bottom-right", 17), ("bf16", 4, 2, 40, True, -1)])
def test_autograd_through_the_wrapper_on_a_fused_projection(dtype, Hq, Hkv, D, causal, window, oracle_mod):
    """q, k, v are the three strided slices of one [T, Hq + 2 Hkv, D] tensor (read in place at D = 64 / 128, zero-padded to 64 at D = 40);
    torch.autograd.grad through aule.flash_attention_varlen against the judge, the maxima read from the offsets (the one
    synchronisation) and passed; the gradient is zero in the rows no sequence owns."""
    import torch
    import aule
    ns = [0, 1, 31, 33, 129, 70]
    p = Packed(15, dtype, Hq, Hkv, D, ns, ns, lead=(3, 3), tail=(5, 5))
    tdt = torch_dtype(dtype)
    fused = torch.from_numpy(np.concatenate([p.q, p.k, p.v], axis=1)).to("cuda", tdt).requires_grad_(True)
    q, k, v = fused[:, :Hq], fused[:, Hq:Hq + Hkv], fused[:, Hq + Hkv:]
    cu = torch.from_numpy(_i32(p.cu_q)).cuda()
    dout = torch.from_numpy(p.dout).to("cuda", tdt)
    for maxima in ({}, dict(max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk)):
        out, lse = aule.flash_attention_varlen(q, k, v, cu, cu, causal=causal, window_size=window, return_lse=True, **maxima)
        assert out.shape == (p.Tq, Hq, D) and lse.shape == (p.Tq, Hq) and not lse.requires_grad
        (g,) = torch.autograd.grad(out, fused, dout)
        torch.cuda.synchronize()
        oq, _ = p.owned()
        assert not g[torch.from_numpy(~oq).cuda()].any(), "the gradient of a row no sequence owns must be zero"
        res = dict(out=out, lse=lse, dq=g[:, :Hq], dk=g[:, Hq:Hq + Hkv], dv=g[:, Hq + Hkv:])
        _judge(p, res, oracle_mod, causal, window, "autograd %s D%d" % (dtype, D))
    with torch.no_grad():
        plain = aule.flash_attention_varlen(q, k, v, cu, cu, causal=causal, window_size=window, **maxima)
    torch.cuda.synchronize()
    own = torch.from_numpy(oq).cuda()
    assert same_bits(torch, plain[own], out.detach()[own])


def test_capture_replays_with_the_current_offsets():
    """forward and backward captured with both maxima and the workspace passed: no allocation, no synchronisation; a replay equals
    eager bit for bit, and after the offsets are overwritten in place the replay equals an eager call on the new contents"""
    import torch
    p = Packed(16, "bf16", 8, 2, 128, [100, 7, 60, 33], [100, 200, 3, 97], max_sq=128, max_sk=256)
    assert p.Tq == 200 and p.Tk == 400
    names = ("out", "lse", "dq", "dk", "dv")

    def eager(cu_q, cu_k):
        x = Packed.__new__(Packed)
        x.__dict__.update(p.__dict__)
        x.cu_q, x.cu_k = np.asarray(cu_q), np.asarray(cu_k)
        return {n: t.clone() for n, t in Run(torch, x).launch(True, -1).results().items()}

    want = eager(p.cu_q, p.cu_k)
    run = Run(torch, p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run.launch(True, -1)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.launch(True, -1)
    for n in names:
        getattr(run, n).view(torch.uint8).fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    for n in names:
        assert same_bits(torch, getattr(run, n), want[n]), n + ": replay differs from eager"
    new_q, new_k = [0, 128, 128, 150, 200], [0, 40, 296, 300, 400]
    want2 = eager(new_q, new_k)
    assert not same_bits(torch, want2["out"], want["out"])
    run.cu_q.copy_(torch.tensor(new_q, dtype=torch.int32, device="cuda"))
    run.cu_k.copy_(torch.tensor(new_k, dtype=torch.int32, device="cuda"))
    for n in names:
        getattr(run, n).view(torch.uint8).fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    for n in names:
        assert same_bits(torch, getattr(run, n), want2[n]), n + ": replay does not see the current offsets"


@pytest.mark.parametrize("dtype,Hq,Hkv,D,causal,window", [("bf16", 8, 2, 128, True, -1), ("fp16", 4, 1, 64, "bottom-right", 17), ("bf16", 2, 2, 32, False, -1)])
def test_hostile_memory_and_hostile_offsets(dtype, Hq, Hkv, D, causal, window, oracle_mod):
    """Every tensor carved from one arena, outputs, workspace and guard bands 0xFF; offsets negative, decreasing, beyond the totals,
    INT32_MIN and INT32_MAX.  After the clamps (max_seqlen_q = 40, max_seqlen_k = 64) the sequences own q rows [0, 30), [30, 70),
    [95, 120) and k rows [0, 50), [50, 114), [115, 150): exactly those are written and right, inputs and guards are intact."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    cu_q = [I32_MIN, 30, I32_MAX, 100, 95, 130, -3]
    cu_k = [-9, 50, I32_MAX, 140, 115, 200, I32_MIN]
    p = Packed(17, dtype, Hq, Hkv, D, None, None, max_sq=40, max_sk=64, cu_q=cu_q, cu_k=cu_k, Tq=120, Tk=150)
    assert [(s, n, sk, L) for s, n, sk, L in p.sequences() if n + L] == [(0, 30, 0, 50), (30, 40, 50, 64), (95, 25, 115, 35)]
    tdt = torch_dtype(dtype)
    qb, kb = p.Tq * Hq * D * 2, p.Tk * Hkv * D * 2
    ws_bytes = _ws_bytes(p)
    regions = [("q", qb, "in"), ("k", kb, "in"), ("v", kb, "in"), ("dout", qb, "in"), ("cu_seqlens_q", (p.B + 1) * 4, "in"),
               ("cu_seqlens_k", (p.B + 1) * 4, "in"), ("out", qb, "out"), ("lse", p.Tq * Hq * 4, "out"), ("dq", qb, "out"),
               ("dk", kb, "out"), ("dv", kb, "out"), ("workspace", ws_bytes, "ws")]
    ar = Arena(torch, regions, Hq * D * 2)
    orig = {n: ar.upload(n, torch.from_numpy(a).to(tdt)) for n, a in (("q", p.q), ("k", p.k), ("v", p.v), ("dout", p.dout))}
    orig["cu_seqlens_q"] = ar.upload("cu_seqlens_q", _i32(cu_q))
    orig["cu_seqlens_k"] = ar.upload("cu_seqlens_k", _i32(cu_k))
    ar.fill(POISON)
    _launch(torch, lib, p, {n: ar.ptr(n) for n, _, _ in regions}, causal, window, ws_bytes)
    torch.cuda.synchronize()
    assert ar.guards_intact(), "guard bytes written: %r" % (ar.damage(),)
    for n, o in orig.items():
        assert ar.unchanged(n, o), "input %s was written" % n
    res = dict(out=ar.view("out", tdt, (p.Tq, Hq, D)), lse=ar.view("lse", torch.float32, (p.Tq, Hq)), dq=ar.view("dq", tdt, (p.Tq, Hq, D)),
               dk=ar.view("dk", tdt, (p.Tk, Hkv, D)), dv=ar.view("dv", tdt, (p.Tk, Hkv, D)))
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, window, "hostile %s D%d" % (dtype, D))


def test_no_key_row_and_no_query_row(oracle_mod):
    """total_k = 0 with total_q > 0: zeros and -inf in the owned rows (k and v null); a backward with total_q = 0 zeroes the owned dk / dv rows"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Packed(18, "fp16", 4, 2, 64, [5, 40], [0, 0], tail=(3, 0))
    run = Run(torch, p)
    ptr = dict(q=run.q.data_ptr(), k=None, v=None, cu_seqlens_q=run.cu_q.data_ptr(), cu_seqlens_k=run.cu_k.data_ptr(), out=run.out.data_ptr(),
               lse=run.lse.data_ptr(), dout=run.dout.data_ptr(), dq=run.dq.data_ptr(), dk=None, dv=None, workspace=run.ws.data_ptr())
    _launch(torch, lib, p, ptr, True, -1, _ws_bytes(p))
    res = run.results()
    assert not res["out"][:45].any() and bool((res["lse"][:45] == -float("inf")).all()) and not res["dq"][:45].any()
    assert bool((res["out"][45:].view(torch.uint8) == POISON).all()) and bool((res["dq"][45:].view(torch.uint8) == POISON).all())
    p = Packed(19, "bf16", 4, 2, 32, [0, 0], [70, 130], lead=(0, 2), tail=(0, 3))
    run = Run(torch, p)
    ptr = dict(q=None, k=run.k.data_ptr(), v=run.v.data_ptr(), cu_seqlens_q=run.cu_q.data_ptr(), cu_seqlens_k=run.cu_k.data_ptr(), out=None,
               lse=None, dout=None, dq=None, dk=run.dk.data_ptr(), dv=run.dv.data_ptr(), workspace=None)
    d = _capi.VarlenBwdDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = 2, 2, 4, 2, 32
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k, d.causal = 0, p.Tk, 1, 130, 1
    d.q_token_stride, d.k_token_stride, d.v_token_stride = 128, 64, 64
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, a in ptr.items():
        setattr(d, n, a)
    assert int(lib.aule_attention_varlen_backward_workspace_size(ctypes.byref(d))) == 0
    _capi.check(lib.aule_attention_varlen_backward_ex(ctypes.byref(d)), "varlen backward without a query")
    torch.cuda.synchronize()
    for g in (run.dk, run.dv):
        assert not g[2:202].any() and bool((g[:2].view(torch.uint8) == POISON).all()) and bool((g[202:].view(torch.uint8) == POISON).all())
