"""MLA prefill on the GPU: aule_attention_mla_prefill_ex and aule.flash_attention_mla_prefill (the non-absorbed 192 / 128 form over a
variable-length packed batch).

Judge: per sequence, oracle.np_fwd_f64 on the quantised inputs of that sequence reshaped to [1, H, S, D], with K = [k_nope | k_pe]
(k_pe repeated for every head; the oracle takes a value width that differs from the key width) and the same causal code.  The
sequence bounds come from the clamp rule of include/aule.h restated here (_clamp, as tests/test_gpu_varlen.py); the rows of a sequence
that see no key (a prefix under the bottom-right rule with L < n, everything with L = 0) are checked directly against the rule --
out = 0, lse = -inf exactly -- and the oracle judges the remaining rows, whose own visibility mask is asserted equal to the rule's.
Bounds: util.fwd_tol(dtype, max|V|) for every row of out (the rows that see fewer than util.MANY_KEYS keys through
util.assert_close_rows, which applies and prints that bound for them) and LSE within 1e-3; the achieved maxima are printed before
they are judged.  (The rule of assert_close_rows for rows with MANY_KEYS keys or more -- no u max|V| term -- is the one of the
full-size configurations: at 64 .. 260 keys of Gaussian data the rounding of P to bf16 alone is about u max|V| / sqrt(keys) = 1.1e-3
and 2 of 42 240 elements of a sequence of 129 tokens sit at 1.23e-3, above its 1.14e-3; it is not asserted here.)  Every launch
through the C entry goes to buffers pre-filled with 0xFF, and the rows no sequence owns must still hold it afterwards."""
import ctypes

import numpy as np
import pytest

import hostile
from hostile import POISON, Arena, same_bits
from util import MANY_KEYS, assert_close, assert_close_rows, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

LSE_ATOL = 1e-3
CODE = {False: 0, True: 1, "bottom-right": 2}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
DQ, DN, DR, DV = 192, 128, 64, 128
# the lengths of tests/test_gpu_varlen.py -- they cross the 32-row wave, the 128-row block and the 64-key tile, paired so that L < n,
# L > n, L = n, n = 0 and L = 0 all occur -- and one sequence of 1100 tokens: nine ranks of one sequence, eighteen tiles
NS = [0, 1, 31, 33, 129, 200, 200, 1]
LS = [63, 0, 257, 1, 130, 65, 257, 1]
LONG = 1100


def _clamp(cu, b, total, cap):
    s = min(max(int(cu[b]), 0), total)
    e = min(max(int(cu[b + 1]), s), total)
    return s, min(e - s, cap)


def _visible(n, L, code):
    """[n, L] bool: the rule of include/aule.h"""
    i = np.arange(n)[:, None]
    j = np.arange(L)[None, :]
    pos = i + (L - n if code == 2 else 0)
    return (j <= pos) if code else np.ones((n, L), dtype=bool)


def _i32(a):
    return np.clip(np.asarray(a, dtype=np.int64), I32_MIN, I32_MAX).astype(np.int32)


class Packed:
    """A packed batch: q [Tq, H, 192], k_nope / v [Tk, H, 128], k_pe [Tk, 64] (quantised fp32 arrays), offsets and maxima as the entry
    reads them."""

    def __init__(self, seed, dtype, H, ns, ls, lead=(0, 0), tail=(0, 0), max_sq=None, max_sk=None, cu_q=None, cu_k=None, Tq=None, Tk=None,
                 zero_rope=False):
        rng = np.random.RandomState(seed)
        self.dtype, self.H = dtype, H
        self.cu_q = np.asarray(cu_q if cu_q is not None else lead[0] + np.concatenate([[0], np.cumsum(ns)]), dtype=np.int64)
        self.cu_k = np.asarray(cu_k if cu_k is not None else lead[1] + np.concatenate([[0], np.cumsum(ls)]), dtype=np.int64)
        self.B = len(self.cu_q) - 1
        self.Tq = Tq if Tq is not None else int(self.cu_q[-1]) + tail[0]
        self.Tk = Tk if Tk is not None else int(self.cu_k[-1]) + tail[1]
        self.q = quantize(rng.randn(self.Tq, H, DQ), dtype)
        self.kn = quantize(rng.randn(self.Tk, H, DN), dtype)
        self.kp = quantize(rng.randn(self.Tk, DR), dtype)
        self.v = quantize(rng.randn(self.Tk, H, DV), dtype)
        if zero_rope:
            self.q[..., DN:] = 0
            self.kp[:] = 0
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
        oq = np.zeros(self.Tq, dtype=bool)
        for sq, n, _, _ in self.sequences():
            assert not oq[sq:sq + n].any(), "the test's sequences overlap"
            oq[sq:sq + n] = True
        return oq

    def alone(self, b):
        """sequence b as a batch of its own (the arrays sliced, offsets from 0)"""
        sq, n, sk, L = self.sequences()[b]
        p = Packed.__new__(Packed)
        p.dtype, p.H, p.B = self.dtype, self.H, 1
        p.q, p.kn, p.kp, p.v = self.q[sq:sq + n], self.kn[sk:sk + L], self.kp[sk:sk + L], self.v[sk:sk + L]
        p.cu_q, p.cu_k, p.Tq, p.Tk = np.array([0, n]), np.array([0, L]), n, L
        p.max_sq, p.max_sk = max(n, 1), max(L, 1)
        return p

    def with_offsets(self, cu_q, cu_k):
        p = Packed.__new__(Packed)
        p.__dict__.update(self.__dict__)
        p.cu_q, p.cu_k = np.asarray(cu_q), np.asarray(cu_k)
        return p


def _launch(torch, p, ptr, causal, strides=None, scale=0.0):
    """the C entry on the pointers in `ptr` (name -> address); strides: name -> elements (None: contiguous)"""
    from aule import _capi
    s = strides or dict(q_token_stride=p.H * DQ, k_nope_token_stride=p.H * DN, k_nope_head_stride=DN, v_token_stride=p.H * DV,
                        v_head_stride=DV, k_pe_token_stride=DR)
    d = _capi.MlaPrefillDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads, d.qk_dim, d.v_dim = hostile.DTYPE_CODE[p.dtype], p.B, p.H, DQ, DV
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = p.Tq, p.Tk, p.max_sq, p.max_sk
    d.scale, d.causal, d.device = scale, CODE[causal], torch.cuda.current_device()
    for n, x in s.items():
        setattr(d, n, x)
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse"):
        setattr(d, n, ptr[n])
    _capi.check(_capi.get_lib().aule_attention_mla_prefill_ex(ctypes.byref(d)), "MLA prefill")


class Run:
    """the batch on the device, out and lse pre-filled with 0xFF; launch() runs the C entry into them.
    in_place: k_nope and v the two halves of one [Tk, H, 256] tensor, k_pe columns 512.. of a [Tk, 576] tensor, q in a buffer 16
    elements wider than a token -- NaN bits in every element between the rows."""

    def __init__(self, torch, p, in_place=False):
        tdt = torch_dtype(p.dtype)
        self.torch, self.p, self.strides = torch, p, None
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
        self.q, self.kn, self.kp, self.v = up(p.q), up(p.kn), up(p.kp), up(p.v)
        if in_place:
            nan = lambda *shape: torch.full(shape[:-1] + (shape[-1] * 2,), POISON, dtype=torch.uint8, device="cuda").view(tdt)   # noqa: E731
            wq = p.H * DQ + 16
            bq, kvb, down = nan(p.Tq, wq), nan(p.Tk, p.H, DN + DV), nan(p.Tk, 512 + DR)
            bq[:, :p.H * DQ] = self.q.reshape(p.Tq, -1)
            kvb[..., :DN] = self.kn
            kvb[..., DN:] = self.v
            down[:, 512:] = self.kp
            self.hold = (bq, kvb, down)
            self.q, self.kn, self.v, self.kp = bq, kvb[..., :DN], kvb[..., DN:], down[:, 512:]   # (data_ptr() of a slice: its first element)
            self.strides = dict(q_token_stride=wq, k_nope_token_stride=p.H * (DN + DV), k_nope_head_stride=DN + DV,
                                v_token_stride=p.H * (DN + DV), v_head_stride=DN + DV, k_pe_token_stride=512 + DR)
        self.cu_q, self.cu_k = (torch.from_numpy(_i32(c)).cuda() for c in (p.cu_q, p.cu_k))
        poison = lambda shape, dt: torch.full(shape, POISON, dtype=torch.uint8, device="cuda").view(dt)   # noqa: E731
        self.out = poison((p.Tq, p.H, DV * 2), tdt)
        self.lse = poison((p.Tq, p.H * 4), torch.float32)

    def launch(self, causal, scale=None):
        names = ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse")
        tensors = (self.q, self.kn, self.kp, self.v, self.cu_q, self.cu_k, self.out, self.lse)
        ptr = {n: (t.data_ptr() if t.numel() else None) for n, t in zip(names, tensors)}
        _launch(self.torch, self.p, ptr, causal, self.strides, 0.0 if scale is None else scale)
        return self

    def results(self):
        self.torch.cuda.synchronize()
        return dict(out=self.out, lse=self.lse)


def _np(t):
    return t.detach().float().cpu().numpy()


def _judge(p, res, oracle, causal, what, scale=None, sides=1):
    """res: name -> tensor (out, lse over the whole packed axis).  Checks every owned row; prints the maxima and returns them.
    sides = 2: the result went through two roundings to 16 bits (a merge): fwd_tol(dtype, max|V|, sides=2) for every row."""
    code = CODE[causal]
    out, lse = _np(res["out"]), _np(res["lse"])
    worst = dict(out=0.0, lse=0.0)
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        tag = "%s seq %d (n %d, L %d)" % (what, b, n, L)
        vis = _visible(n, L, code)
        seen = vis.any(axis=1)
        rows = np.flatnonzero(seen)
        a, e = (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)
        assert seen[a:e].all(), "the rows that see a key are one range"
        blind = np.r_[sq:sq + a, sq + e:sq + n]
        assert (out[blind] == 0).all() and (lse[blind] == -np.inf).all(), tag + ": a row without a visible key must be zeros and -inf"
        if e == a:
            continue
        # the rows a .. e - 1 against all L keys: the oracle's own mask must be the rule's
        sub = causal if not (code == 2 and L <= e - a) else True
        assert np.array_equal(oracle._vis_mask(e - a, L, sub, -1), vis[a:e]), tag + ": the judge's sub-problem is another problem"
        t = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2))[None]   # noqa: E731
        key = np.concatenate([p.kn[sk:sk + L], np.repeat(p.kp[sk:sk + L, None, :], p.H, axis=1)], axis=2)
        qs, ks, vs = t(p.q[sq + a:sq + e]), t(key), t(p.v[sk:sk + L])
        ro, rl = oracle.np_fwd_f64(qs, ks, vs, causal=sub, scale=scale)
        got = out[sq + a:sq + e].transpose(1, 0, 2)[None]
        got_lse = lse[sq + a:sq + e].T[None]
        worst["out"] = max(worst["out"], float(np.abs(got - ro).max()))
        worst["lse"] = max(worst["lse"], float(np.abs(got_lse - rl).max()))
        print("%s: max|out err| %.3e  max|lse err| %.3e" % (tag, float(np.abs(got - ro).max()), float(np.abs(got_lse - rl).max())))
        vmax = np.abs(vs).max()
        atol, rtol = fwd_tol(p.dtype, vmax, sides=sides)
        assert_close(got, ro, atol, rtol, tag + " out")
        few = np.tile(vis[a:e].sum(axis=1), p.H) < MANY_KEYS
        if sides == 1 and few.any():
            assert_close_rows(got.reshape(-1, DV)[few], ro.reshape(-1, DV)[few], np.zeros(int(few.sum())), p.dtype, vmax, tag + " out")
        assert_close(got_lse, rl, LSE_ATOL, 0.0, tag + " lse")
    print("%s: max|err| out %.3e [fwd_tol %s] lse %.3e [%.0e]" % (what, worst["out"], "%.2e + %.2e |ref|" % fwd_tol(p.dtype, np.abs(p.v).max(), sides),
                                                                   worst["lse"], LSE_ATOL))
    return worst


def _unowned_still_poisoned(torch, p, res):
    free = torch.from_numpy(~p.owned()).cuda()
    for n in ("out", "lse"):
        rows = res[n][free]
        assert bool((rows.reshape(-1).view(torch.uint8) == POISON).all()), n + ": a row that belongs to no sequence was written"


def _mixed(seed, dtype, H, **kw):
    """the mixed batch and the long sequence, with a lead offset (cu[0] = 3 / 2) and tail rows behind the last sequence (5 / 7)"""
    return Packed(seed, dtype, H, NS + [LONG], LS + [LONG], lead=(3, 2), tail=(5, 7), **kw)


def _cid(c):
    if isinstance(c, bool) or c == "bottom-right":
        return {False: "full", True: "causal", "bottom-right": "br"}[c]
    return "H%d" % c if isinstance(c, int) else str(c)


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", True, 2), ("bf16", False, 1), ("fp16", False, 5),
                                            ("bf16", "bottom-right", 2), ("fp16", "bottom-right", 1)], ids=_cid)
def test_parity_against_the_oracle(dtype, causal, H, oracle_mod):
    import torch
    p = _mixed(31, dtype, H)
    res = Run(torch, p).launch(causal).results()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, "parity %s H%d %s" % (dtype, H, _cid(causal)))


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2), ("bf16", False, 1)], ids=_cid)
def test_tensors_read_in_place_give_the_same_bits(dtype, causal, H):
    """k_nope and v the halves of a [Tk, H, 256] tensor, k_pe columns 512.. of a [Tk, 576] tensor, q with a wider token stride (a kernel
    that read one tensor with another's stride would read the NaN bits between the rows): bit-identical to the contiguous run"""
    import torch
    p = _mixed(32, dtype, H)
    want = Run(torch, p).launch(causal).results()
    got = Run(torch, p, in_place=True).launch(causal).results()
    assert bool(torch.isfinite(want["out"][torch.from_numpy(p.owned()).cuda()].float()).all())
    for name in want:
        assert same_bits(torch, got[name], want[name]), name + " depends on the strides"


@pytest.mark.parametrize("dtype,causal,H", [("bf16", "bottom-right", 2), ("fp16", True, 5)], ids=_cid)
def test_a_sequence_alone_is_bit_identical_to_the_same_sequence_in_the_batch(dtype, causal, H):
    import torch
    p = _mixed(33, dtype, H)
    batch = Run(torch, p).launch(causal).results()
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        if n == 0:
            continue
        one = Run(torch, p.alone(b)).launch(causal).results()
        for name in ("out", "lse"):
            assert same_bits(torch, one[name], batch[name][sq:sq + n]), "seq %d: %s differs between alone and in the batch" % (b, name)


@pytest.mark.parametrize("causal", [True, "bottom-right", False], ids=_cid)
def test_max_seqlen_cuts_a_sequence_to_its_first_tokens(causal, oracle_mod):
    """max_seqlen_q = 40 and max_seqlen_k = 70 below the longest sequences: n and L are cut, the rows behind the cut are not written"""
    import torch
    p = Packed(34, "bf16", 2, NS, LS, lead=(1, 0), tail=(2, 3), max_sq=40, max_sk=70)
    assert [s[1] for s in p.sequences()] == [0, 1, 31, 33, 40, 40, 40, 1] and [s[3] for s in p.sequences()] == [63, 0, 70, 1, 70, 65, 70, 1]
    res = Run(torch, p).launch(causal).results()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, "max_seqlen cut " + _cid(causal))


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2), ("bf16", False, 1)], ids=_cid)
def test_hostile_memory_and_hostile_offsets(dtype, causal, H, oracle_mod):
    """Every tensor carved from one arena, outputs and guard bands 0xFF; offsets negative, decreasing, beyond the totals, INT32_MIN and
    INT32_MAX: hostile, and defined by the clamps.  After them (max_seqlen_q = 40, max_seqlen_k = 64) the sequences own q rows [0, 30),
    [30, 70), [95, 120) and k rows [0, 50), [50, 114), [115, 150): exactly those query rows are written and right, inputs and guards
    are intact."""
    import torch
    cu_q = [I32_MIN, 30, I32_MAX, 100, 95, 130, -3]
    cu_k = [-9, 50, I32_MAX, 140, 115, 200, I32_MIN]
    p = Packed(35, dtype, H, None, None, max_sq=40, max_sk=64, cu_q=cu_q, cu_k=cu_k, Tq=120, Tk=150)
    assert [(s, n, sk, L) for s, n, sk, L in p.sequences() if n + L] == [(0, 30, 0, 50), (30, 40, 50, 64), (95, 25, 115, 35)]
    tdt = torch_dtype(dtype)
    regions = [("q", p.Tq * H * DQ * 2, "in"), ("k_nope", p.Tk * H * DN * 2, "in"), ("k_pe", p.Tk * DR * 2, "in"), ("v", p.Tk * H * DV * 2, "in"),
               ("cu_seqlens_q", (p.B + 1) * 4, "in"), ("cu_seqlens_k", (p.B + 1) * 4, "in"), ("out", p.Tq * H * DV * 2, "out"),
               ("lse", p.Tq * H * 4, "out")]
    ar = Arena(torch, regions, H * DQ * 2)
    orig = {n: ar.upload(n, torch.from_numpy(a).to(tdt)) for n, a in (("q", p.q), ("k_nope", p.kn), ("k_pe", p.kp), ("v", p.v))}
    orig["cu_seqlens_q"] = ar.upload("cu_seqlens_q", _i32(cu_q))
    orig["cu_seqlens_k"] = ar.upload("cu_seqlens_k", _i32(cu_k))
    ar.fill(POISON)
    _launch(torch, p, {n: ar.ptr(n) for n, _, _ in regions}, causal)
    torch.cuda.synchronize()
    assert ar.guards_intact(), "guard bytes written: %r" % (ar.damage(),)
    for n, o in orig.items():
        assert ar.unchanged(n, o), "input %s was written" % n
    res = dict(out=ar.view("out", tdt, (p.Tq, H, DV)), lse=ar.view("lse", torch.float32, (p.Tq, H)))
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, "hostile %s H%d" % (dtype, H))


def test_no_key_row():
    """total_k = 0 with total_q > 0: zeros and -inf in the owned rows, with k_nope, k_pe and v null"""
    import torch
    p = Packed(36, "fp16", 2, [5, 140], [0, 0], tail=(3, 0))
    res = Run(torch, p).launch(True).results()
    assert not res["out"][:145].any() and bool((res["lse"][:145] == -float("inf")).all())
    assert bool((res["out"][145:].view(torch.uint8) == POISON).all()) and bool((res["lse"][145:].view(torch.uint8) == POISON).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_key_chunks_merged_equal_one_call(dtype, oracle_mod):
    """non-causal attention over keys [0, L1) and [L1, L) of every sequence as two calls with return_lse=True, merged by
    aule.merge_attention_states: the oracle over all L keys, two roundings to 16 bits (fwd_tol with sides = 2).  One sequence has
    an empty second chunk (its merge returns the first state)."""
    import torch
    import aule
    H, ns, ls, cut = 2, [33, 129, 70], [257, 130, 65], [100, 64, 65]
    p = Packed(37, dtype, H, ns, ls)
    tdt = torch_dtype(dtype)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    cu_q = torch.from_numpy(_i32(p.cu_q)).cuda()
    states = []
    for part in (0, 1):
        idx = np.concatenate([np.arange(s + (c if part else 0), s + (L if part else c)) for s, L, c in zip(p.cu_k[:-1], ls, cut)]).astype(np.int64)
        lens = [(L - c) if part else c for L, c in zip(ls, cut)]
        cu_k = torch.from_numpy(_i32(np.concatenate([[0], np.cumsum(lens)]))).cuda()
        out, lse = aule.flash_attention_mla_prefill(up(p.q), up(p.kn[idx]), up(p.kp[idx]), up(p.v[idx]), cu_q, cu_k, max_seqlen_q=max(ns),
                                                    max_seqlen_k=max(max(lens), 1), causal=False, return_lse=True)
        assert out.shape == (p.Tq, H, DV) and lse.shape == (p.Tq, H) and lse.dtype == torch.float32
        states += [out, lse]
    assert bool((states[3][-70:] == -float("inf")).all()) and not states[2][-70:].any()
    out, lse = aule.merge_attention_states(*states)
    torch.cuda.synchronize()
    assert same_bits(torch, out[-70:], states[0][-70:])
    _judge(p, dict(out=out, lse=lse), oracle_mod, False, "merge %s" % dtype, sides=2)


@pytest.mark.parametrize("dtype,causal", [("bf16", True), ("fp16", "bottom-right")], ids=_cid)
def test_zero_rope_agrees_with_the_varlen_forward_at_128(dtype, causal, oracle_mod):
    """k_pe = 0 and q[..., 128:] = 0: the same problem as aule.flash_attention_varlen at D = 128 under the same explicit scale.  Two
    16-bit results of one problem: fwd_tol with sides = 2; each side is also judged against the oracle alone."""
    import torch
    import aule
    H, scale = 2, 0.11
    p = Packed(38, dtype, H, NS, LS, lead=(3, 2), tail=(5, 7), zero_rope=True)
    got = Run(torch, p).launch(causal, scale=scale).results()
    _judge(p, got, oracle_mod, causal, "zero rope, MLA prefill %s" % dtype, scale=scale)
    tdt = torch_dtype(dtype)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    cu_q, cu_k = (torch.from_numpy(_i32(c)).cuda() for c in (p.cu_q, p.cu_k))
    out, lse = aule.flash_attention_varlen(up(p.q[..., :DN]), up(p.kn), up(p.v), cu_q, cu_k, max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk,
                                           causal=causal, scale=scale, return_lse=True)
    torch.cuda.synchronize()
    _judge(p, dict(out=out, lse=lse), oracle_mod, causal, "zero rope, varlen D128 %s" % dtype, scale=scale)
    own = torch.from_numpy(p.owned()).cuda()
    a, b = _np(got["out"][own]), _np(out[own])
    atol, rtol = fwd_tol(dtype, np.abs(p.v).max(), sides=2)
    print("zero rope %s: max|MLA prefill - varlen| out %.3e, bit-identical: out %s lse %s"
          % (dtype, np.abs(a - b).max(), same_bits(torch, got["out"][own], out[own]), same_bits(torch, got["lse"][own], lse[own])))
    assert_close(a, b, atol, rtol, "MLA prefill against the varlen forward")
    la, lb = _np(got["lse"][own]), _np(lse[own])
    fin = np.isfinite(lb)
    assert np.array_equal(np.isfinite(la), fin) and np.abs(la[fin] - lb[fin]).max() <= 2 * LSE_ATOL


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2)], ids=_cid)
def test_python_entry_equals_the_c_entry(dtype, causal, H):
    """contiguous tensors and the in-place slices through aule.flash_attention_mla_prefill: the owned rows bit-identical to the C
    entry's; return_lse=False returns one tensor; the maxima read from the offsets (the one synchronisation) give the same bits"""
    import torch
    import aule
    p = _mixed(39, dtype, H)
    want = Run(torch, p).launch(causal).results()
    own = torch.from_numpy(p.owned()).cuda()
    for in_place in (False, True):
        run = Run(torch, p, in_place=in_place)
        q = run.q[:, :H * DQ].view(p.Tq, H, DQ) if in_place else run.q
        assert (q.data_ptr() == run.q.data_ptr()) and (not in_place or not q.is_contiguous())
        for maxima in (dict(max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk), {}):
            out, lse = aule.flash_attention_mla_prefill(q, run.kn, run.kp if not in_place else run.kp.unsqueeze(1), run.v, run.cu_q, run.cu_k,
                                                        causal=causal, return_lse=True, **maxima)
            torch.cuda.synchronize()
            assert out.shape == (p.Tq, H, DV) and out.dtype == torch_dtype(dtype) and lse.shape == (p.Tq, H)
            assert same_bits(torch, out[own], want["out"][own]) and same_bits(torch, lse[own], want["lse"][own]), (in_place, maxima)
    only = aule.flash_attention_mla_prefill(q, run.kn, run.kp, run.v, run.cu_q, run.cu_k, max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk, causal=causal)
    torch.cuda.synchronize()
    assert torch.is_tensor(only) and same_bits(torch, only[own], want["out"][own])
    with pytest.raises(ValueError, match="no backward"):
        aule.flash_attention_mla_prefill(q.clone().requires_grad_(True), run.kn, run.kp, run.v, run.cu_q, run.cu_k, max_seqlen_q=p.max_sq,
                                         max_seqlen_k=p.max_sk)


def test_capture_replays_with_the_current_offsets():
    """captured with both maxima passed: one launch on one stream, no allocation, no synchronisation; a replay equals eager bit for
    bit, and after the offsets are overwritten in place the replay equals an eager call on the new contents"""
    import torch
    p = Packed(40, "bf16", 2, [100, 7, 60, 33], [100, 200, 3, 97], max_sq=128, max_sk=256)
    assert p.Tq == 200 and p.Tk == 400
    names = ("out", "lse")

    def eager(cu_q, cu_k):
        return {n: t.clone() for n, t in Run(torch, p.with_offsets(cu_q, cu_k)).launch(True).results().items()}

    want = eager(p.cu_q, p.cu_k)
    run = Run(torch, p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run.launch(True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run.launch(True)
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
