"""MLA 192 / 128 backward on the GPU: aule_attention_mla_prefill_backward_ex and aule.flash_attention_mla_varlen.

Judge: per sequence, oracle.np_fwd_f64 / np_bwd_f64 on the quantised inputs of that sequence with K = [k_nope | k_pe broadcast over the
heads]; v and dout enter the judge zero-padded from 128 to 192 columns (its fold of dv over grouped heads assumes one width; the pad
changes no product and its dv columns come back exactly zero); the k_pe gradient is the judge's dk[..., 128:] summed over the heads.
The forward half (out, lse) is judged by tests/test_gpu_mla_prefill.py::_judge: util.fwd_tol and LSE within 1e-3.  Gradients: util.BWD_TOL scaled by max(1, max|grad|), tests/test_gpu_varlen.py::_check_grad itself -- for dk_pe too, which is
accumulated in fp32 over the heads and rounded once.  A query row without a visible key has dq = 0 exactly, a key no query sees has
dk_nope = dv = dk_pe = 0 exactly.  Shapes: the mixed batch of the variable-length suite (at most 257 tokens; L < n, L > n, L = n,
n = 0 and L = 0 all present) with a lead offset and tail rows.  Everything the library writes goes to buffers pre-filled with 0xFF:
rows no sequence owns, and the elements between the strided dk_nope / dv rows, must still hold it afterwards.  The achieved maxima
are printed."""
import ctypes

import numpy as np
import pytest

import hostile
import test_gpu_mla_prefill as fw          # helpers only: Packed, the clamp and visibility rules, the forward's judge
from hostile import POISON, Arena, same_bits
from test_gpu_varlen import _check_grad
from util import quantize, torch_dtype

pytestmark = pytest.mark.gpu

CODE = fw.CODE
DQ, DN, DR, DV = 192, 128, 64, 128
NS, LS = fw.NS, fw.LS
I32_MIN, I32_MAX = fw.I32_MIN, fw.I32_MAX
_i32, _np, _cid = fw._i32, fw._np, fw._cid
PLAN = ("heads_per_chunk", "n_chunks", "max_chunks", "delta_grid", "dq_grid", "dkdv_grid", "reduce_grid", "reduce", "ws_lo", "ws_hi")


class Packed(fw.Packed):
    """tests/test_gpu_mla_prefill.py::Packed and dout [Tq, H, 128]"""

    def __init__(self, seed, dtype, H, ns, ls, **kw):
        super().__init__(seed, dtype, H, ns, ls, **kw)
        self.dout = quantize(np.random.RandomState(seed + 1000).randn(self.Tq, H, DV), dtype)

    def owned_k(self):
        ok = np.zeros(self.Tk, dtype=bool)
        for _, _, sk, L in self.sequences():
            assert not ok[sk:sk + L].any(), "the test's sequences overlap"
            ok[sk:sk + L] = True
        return ok

    def alone(self, b):
        sq, n, _, _ = self.sequences()[b]
        p = super().alone(b)
        p.__class__ = Packed
        p.dout = self.dout[sq:sq + n]
        return p

    def with_offsets(self, cu_q, cu_k):
        p = super().with_offsets(cu_q, cu_k)
        p.__class__ = Packed
        return p


def _mixed(seed, dtype, H, **kw):
    """the mixed batch with a lead offset (cu[0] = 3 / 2) and tail rows behind the last sequence (5 / 7)"""
    return Packed(seed, dtype, H, NS, LS, lead=(3, 2), tail=(5, 7), **kw)


def _problem(torch, d, p, causal, strides, scale=0.0):
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads, d.qk_dim, d.v_dim = hostile.DTYPE_CODE[p.dtype], p.B, p.H, DQ, DV
    d.total_q, d.total_k, d.max_seqlen_q, d.max_seqlen_k = p.Tq, p.Tk, p.max_sq, p.max_sk
    d.scale, d.causal, d.device = scale, CODE[causal], torch.cuda.current_device()
    s = dict(q_token_stride=p.H * DQ, k_nope_token_stride=p.H * DN, k_nope_head_stride=DN, v_token_stride=p.H * DV, v_head_stride=DV,
             k_pe_token_stride=DR)
    s.update(strides or {})
    for n, x in s.items():
        if hasattr(d, n):
            setattr(d, n, x)
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return d


def _bwd_desc(torch, p, causal, strides=None, scale=0.0):
    from aule import _capi
    s = dict(dk_nope_token_stride=p.H * DN, dk_nope_head_stride=DN, dv_token_stride=p.H * DV, dv_head_stride=DV)
    s.update(strides or {})
    return _problem(torch, _capi.MlaPrefillBwdDesc(), p, causal, s, scale)


def _plan(torch, p, causal=True, strides=None):
    """the launch plan of the call (host logic: no pointer is read)"""
    from aule import _capi
    out = (ctypes.c_int32 * 10)()
    d = _bwd_desc(torch, p, causal, strides)
    n = _capi.get_lib().aule_hip_debug_mla_prefill_backward_plan(ctypes.byref(d), out, 10)
    assert n in (0, 10), n
    plan = dict(zip(PLAN, out)) if n else dict.fromkeys(PLAN, 0)
    plan["ws_bytes"] = (plan["ws_lo"] & 0xffffffff) | (plan["ws_hi"] << 32)
    return plan


def _ws_bytes(torch, p, causal=True):
    from aule import _capi
    n = int(_capi.get_lib().aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(_bwd_desc(torch, p, causal))))
    assert n == _plan(torch, p, causal)["ws_bytes"]
    return n


def _launch(torch, p, ptr, causal, strides=None, scale=0.0, backward=True, ws_bytes=None):
    """forward, then backward, through the C entries on the pointers in `ptr` (name -> address)"""
    from aule import _capi
    lib = _capi.get_lib()
    d = _problem(torch, _capi.MlaPrefillDesc(), p, causal, strides, scale)
    for n in ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse"):
        setattr(d, n, ptr[n])
    _capi.check(lib.aule_attention_mla_prefill_ex(ctypes.byref(d)), "MLA prefill")
    if backward:
        d = _bwd_desc(torch, p, causal, strides, scale)
        for n in ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "dout", "dq", "dk_nope", "dk_pe", "dv"):
            setattr(d, n, ptr[n])
        d.workspace, d.workspace_bytes = ptr["workspace"], _ws_bytes(torch, p, causal) if ws_bytes is None else ws_bytes
        _capi.check(lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)), "MLA prefill backward")


GAP = 8   # elements between dk_nope and dv, and behind dv, of a head of the wide gradient buffer


class Run:
    """the batch on the device; out, lse, the gradients and the workspace pre-filled with 0xFF; launch() runs forward and backward.
    in_place: tests/test_gpu_mla_prefill.py::Run's inputs (k_nope and v the halves of a [Tk, H, 256] tensor, k_pe columns 512.. of a
    [Tk, 576] one, q 16 elements wider than a token, NaN bits between the rows) and dk_nope / dv the halves of one [Tk, H, 256] buffer.
    wide: dk_nope and dv in one [Tk, H, 272] buffer, 8 elements behind each that the library must not write."""

    def __init__(self, torch, p, in_place=False, wide=False):
        tdt = torch_dtype(p.dtype)
        base = fw.Run(torch, p, in_place=in_place)
        self.torch, self.p, self.base = torch, p, base
        self.strides = dict(base.strides or {})
        self.dout = torch.from_numpy(np.ascontiguousarray(p.dout)).to("cuda", tdt)
        poison = lambda shape, dt=tdt: torch.full(shape[:-1] + (shape[-1] * torch.empty((), dtype=dt).element_size(),), POISON,   # noqa: E731
                                                  dtype=torch.uint8, device="cuda").view(dt)
        self.out, self.lse = base.out, base.lse
        self.dq = poison((p.Tq, p.H, DQ))
        self.dk_pe = poison((p.Tk, DR))
        if in_place or wide:
            W = DN + DV + (2 * GAP if wide else 0)
            self.dkv = poison((p.Tk, p.H, W))
            self.dk_nope, self.dv = self.dkv[..., :DN], self.dkv[..., DN + (GAP if wide else 0):][..., :DV]
            self.strides.update(dk_nope_token_stride=p.H * W, dk_nope_head_stride=W, dv_token_stride=p.H * W, dv_head_stride=W)
        else:
            self.dkv = None
            self.dk_nope, self.dv = poison((p.Tk, p.H, DN)), poison((p.Tk, p.H, DV))
        self.ws = torch.full((max(_ws_bytes(torch, p), 16),), POISON, dtype=torch.uint8, device="cuda")

    def launch(self, causal, scale=None, backward=True):
        b = self.base
        names = ("q", "k_nope", "k_pe", "v", "cu_seqlens_q", "cu_seqlens_k", "out", "lse", "dout", "dq", "dk_nope", "dk_pe", "dv")
        tensors = (b.q, b.kn, b.kp, b.v, b.cu_q, b.cu_k, self.out, self.lse, self.dout, self.dq, self.dk_nope, self.dk_pe, self.dv)
        ptr = {n: (t.data_ptr() if t.numel() else None) for n, t in zip(names, tensors)}
        ptr["workspace"] = self.ws.data_ptr()
        _launch(self.torch, self.p, ptr, causal, self.strides, 0.0 if scale is None else scale, backward)
        return self

    def results(self):
        self.torch.cuda.synchronize()
        return {n: getattr(self, n) for n in ("out", "lse", "dq", "dk_nope", "dk_pe", "dv")}


GRADS = ("dq", "dk_nope", "dk_pe", "dv")


def rounding_model(p, causal, scale=None):
    """per sequence {name: max |g_model - g|} for dq, dk_nope, dk_pe, and {name: max(1, max|g|)}: g the fp64 gradient formula
    dS = P (dP - delta) and g_model the same with delta = rowsum(dO * O) taken from O rounded to the storage dtype, which is what the backward
    entry is given (dv = P^T dO does not read delta).  NumPy on the quantised inputs alone: no GPU, no library call."""
    code, res = CODE[causal], []
    scale = DQ ** -0.5 if scale is None else scale
    for sq, n, sk, L in p.sequences():
        err, norm = dict.fromkeys(GRADS, 0.0), dict.fromkeys(GRADS, 1.0)
        if n and L:
            q, do, v = (x.astype(np.float64) for x in (p.q[sq:sq + n], p.dout[sq:sq + n], p.v[sk:sk + L]))
            key = np.concatenate([p.kn[sk:sk + L], np.repeat(p.kp[sk:sk + L, None, :], p.H, axis=1)], axis=2).astype(np.float64)
            s = np.where(fw._visible(n, L, code)[None], np.einsum("nhd,lhd->hnl", q, key) * scale, -np.inf)
            m = s.max(axis=-1, keepdims=True)
            e = np.exp(s - np.where(np.isfinite(m), m, 0.0))
            den = e.sum(axis=-1, keepdims=True)
            P = e / np.where(den > 0, den, 1.0)
            O, dP = np.einsum("hnl,lhd->nhd", P, v), np.einsum("nhd,lhd->hnl", do, v)
            g = []
            for Ouse in (O, quantize(O, p.dtype).astype(np.float64)):
                dS = P * (dP - (do * Ouse).sum(axis=-1).T[..., None])
                dk = np.einsum("hnl,nhd->lhd", dS, q) * scale
                g.append(dict(dq=np.einsum("hnl,lhd->nhd", dS, key) * scale, dk_nope=dk[..., :DN], dk_pe=dk[..., DN:].sum(axis=1)))
            for name in g[0]:
                err[name] = float(np.abs(g[1][name] - g[0][name]).max())
                norm[name] = max(1.0, float(np.abs(g[0][name]).max()))
        res.append((err, norm))
    return res


def _judge(p, res, oracle, causal, what, scale=None, forward=True, floors=None):
    """res: name -> tensor over the whole packed axes.  Checks every owned row; prints the maxima and returns them.
    floors: per sequence {name: absolute error allowed whatever the element} (the randomised draws: 4 x rounding_model's error)"""
    code = CODE[causal]
    if forward:
        fw._judge(p, res, oracle, causal, what, scale=scale)
    dq, dkn, dkp, dv = (_np(res[n]) for n in GRADS)
    worst = dict.fromkeys(GRADS, 0.0)
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        tag = "%s seq %d (n %d, L %d)" % (what, b, n, L)
        vis = fw._visible(n, L, code)
        seen = vis.any(axis=1)
        rows = np.flatnonzero(seen)
        a, e = (int(rows[0]), int(rows[-1]) + 1) if rows.size else (0, 0)
        assert seen[a:e].all(), "the rows that see a key are one range"
        blind = np.r_[sq:sq + a, sq + e:sq + n]
        assert (dq[blind] == 0).all(), tag + ": dq of a row without a visible key must be zero"
        unseen = sk + np.flatnonzero(~vis.any(axis=0))
        assert (dkn[unseen] == 0).all() and (dv[unseen] == 0).all() and (dkp[unseen] == 0).all(), tag + ": a key no query sees has zero gradients"
        if e == a:
            continue
        sub = causal if not (code == 2 and L <= e - a) else True
        assert np.array_equal(oracle._vis_mask(e - a, L, sub, -1), vis[a:e]), tag + ": the judge's sub-problem is another problem"
        t = lambda x: np.ascontiguousarray(x.transpose(1, 0, 2))[None]   # noqa: E731
        key = np.concatenate([p.kn[sk:sk + L], np.repeat(p.kp[sk:sk + L, None, :], p.H, axis=1)], axis=2)
        # (np_bwd_f64 folds dv's heads with the key width: v and dout go in zero-padded from 128 to 192 columns, which changes no
        # product -- the pad of dv comes back exactly zero)
        wide = lambda x: np.concatenate([x, np.zeros(x.shape[:-1] + (DQ - DV,), dtype=x.dtype)], axis=-1)   # noqa: E731
        rq, rk, rv = oracle.np_bwd_f64(t(p.q[sq + a:sq + e]), t(key), t(wide(p.v[sk:sk + L])), t(wide(p.dout[sq + a:sq + e])), causal=sub, scale=scale)
        assert not rv[..., DV:].any()
        rv = rv[..., :DV]
        fl = floors[b] if floors is not None else dict.fromkeys(GRADS, 0.0)
        worst["dq"] = max(worst["dq"], _check_grad(dq[sq + a:sq + e].transpose(1, 0, 2)[None], rq, p.dtype, tag + " dq", fl["dq"]))
        worst["dk_nope"] = max(worst["dk_nope"], _check_grad(dkn[sk:sk + L].transpose(1, 0, 2)[None], rk[..., :DN], p.dtype, tag + " dk_nope", fl["dk_nope"]))
        worst["dv"] = max(worst["dv"], _check_grad(dv[sk:sk + L].transpose(1, 0, 2)[None], rv, p.dtype, tag + " dv"))
        worst["dk_pe"] = max(worst["dk_pe"], _check_grad(dkp[sk:sk + L], rk[0, :, :, DN:].sum(axis=0), p.dtype, tag + " dk_pe", fl["dk_pe"]))
    print("%s: of max(1, max|grad|): dq %.2e dk_nope %.2e dk_pe %.2e dv %.2e" % (what, worst["dq"], worst["dk_nope"], worst["dk_pe"], worst["dv"]))
    return worst


def _all_poison(torch, t):
    return bool((t.reshape(-1).view(torch.uint8) == POISON).all())


def _unowned_still_poisoned(torch, p, res, run=None):
    fq, fk = torch.from_numpy(~p.owned()).cuda(), torch.from_numpy(~p.owned_k()).cuda()
    for n, mask in (("out", fq), ("lse", fq), ("dq", fq), ("dk_nope", fk), ("dk_pe", fk), ("dv", fk)):
        assert _all_poison(torch, res[n][mask].contiguous()), n + ": a row that belongs to no sequence was written"
    if run is not None and run.dkv is not None and run.dkv.shape[2] > DN + DV:
        assert _all_poison(torch, run.dkv[..., DN:DN + GAP].contiguous()) and _all_poison(torch, run.dkv[..., DN + GAP + DV:].contiguous()), \
            "an element between the strided dk_nope / dv rows was written"


# both dtypes x the three causal modes x heads 1, 2, 5, and 17 heads: more heads than the chunk bound, so heads_per_chunk = 2 and the
# last chunk holds one head
H_SHORT = 17
PARITY = [(dt, c, H) for dt in ("bf16", "fp16") for c in (True, False, "bottom-right") for H in (1, 2, 5)] + [("bf16", True, H_SHORT), ("fp16", "bottom-right", H_SHORT)]


def test_the_parity_cases_take_both_plans():
    """host logic on the device's CU count: one head writes dk_pe from the dK/dV kernel, more heads go through the reduce, and the
    17-head cases run chunks of two heads with a short last chunk"""
    import torch
    plans = {H: _plan(torch, _mixed(50, "bf16", H)) for H in sorted({c[2] for c in PARITY})}
    print(plans)
    assert any(pl["n_chunks"] == 1 and not pl["reduce"] and pl["reduce_grid"] == 0 for pl in plans.values()), "no case writes dk_pe directly"
    assert any(pl["n_chunks"] >= 2 and pl["reduce"] and pl["reduce_grid"] > 0 for pl in plans.values()), "no case runs the reduce"
    pl = plans[H_SHORT]
    assert pl["n_chunks"] >= 2 and pl["heads_per_chunk"] >= 2 and H_SHORT % pl["heads_per_chunk"] != 0, pl
    for H, pl in plans.items():
        assert (pl["n_chunks"] - 1) * pl["heads_per_chunk"] < H <= pl["n_chunks"] * pl["heads_per_chunk"] and pl["n_chunks"] <= pl["max_chunks"]


@pytest.mark.parametrize("dtype,causal,H", PARITY, ids=_cid)
def test_parity_against_the_oracle(dtype, causal, H, oracle_mod):
    import torch
    p = _mixed(51, dtype, H)
    run = Run(torch, p, wide=True).launch(causal)
    res = run.results()
    _unowned_still_poisoned(torch, p, res, run)
    _judge(p, res, oracle_mod, causal, "parity %s H%d %s" % (dtype, H, _cid(causal)))


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", False, 1)], ids=_cid)
def test_zero_dout_gives_zero_gradients_and_two_runs_agree(dtype, causal, H):
    import torch
    p = _mixed(52, dtype, H)
    first = {n: t.clone() for n, t in Run(torch, p).launch(causal).results().items()}
    again = Run(torch, p).launch(causal).results()
    for n in first:
        assert same_bits(torch, first[n], again[n]), n + ": two runs of the same call differ"
    oq, ok = torch.from_numpy(p.owned()).cuda(), torch.from_numpy(p.owned_k()).cuda()
    assert bool(first["dk_pe"][ok].any()) and bool(first["dq"][oq].any())
    p.dout[:] = 0
    res = Run(torch, p).launch(causal).results()
    for n, own in (("dq", oq), ("dk_nope", ok), ("dk_pe", ok), ("dv", ok)):
        assert not bool(res[n][own].any()), n + " must be exactly zero for dout = 0"


@pytest.mark.parametrize("dtype,causal", [("bf16", True), ("fp16", "bottom-right")], ids=_cid)
def test_zero_rope_agrees_with_the_varlen_backward_at_128(dtype, causal):
    """k_pe = 0 and q[..., 128:] = 0: dq[..., 128:] and dk_pe are exactly zero, and dq[..., :128], dk_nope, dv are the gradients of
    aule.flash_attention_varlen at D = 128 under the same explicit scale: two 16-bit results, within BWD_TOL"""
    import torch
    import aule
    H, scale = 2, 0.11
    p = _mixed(53, dtype, H, zero_rope=True)
    res = Run(torch, p).launch(causal, scale=scale).results()
    oq, ok = torch.from_numpy(p.owned()).cuda(), torch.from_numpy(p.owned_k()).cuda()
    assert not bool(res["dq"][oq][..., DN:].any()) and not bool(res["dk_pe"][ok].any())
    tdt = torch_dtype(dtype)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt).requires_grad_(True)   # noqa: E731
    q, k, v = up(p.q[..., :DN]), up(p.kn), up(p.v)
    cu_q, cu_k = (torch.from_numpy(_i32(c)).cuda() for c in (p.cu_q, p.cu_k))
    out = aule.flash_attention_varlen(q, k, v, cu_q, cu_k, max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk, causal=causal, scale=scale)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), up(p.dout).detach())
    torch.cuda.synchronize()
    for name, got, ref, own in (("dq", res["dq"][..., :DN], dq, oq), ("dk_nope", res["dk_nope"], dk, ok), ("dv", res["dv"], dv, ok)):
        print("zero rope %s %s against the varlen backward: %.2e of max(1, max|grad|)"
              % (dtype, name, _check_grad(_np(got[own]), _np(ref[own]).astype(np.float64), dtype, name)))


@pytest.mark.parametrize("dtype,causal,H", [("bf16", "bottom-right", 2), ("fp16", True, 5)], ids=_cid)
def test_a_sequence_alone_is_bit_identical_to_the_same_sequence_in_the_batch(dtype, causal, H):
    """dq, dk_nope and dv always; dk_pe when both runs cut the heads into the same chunks (the hook says)"""
    import torch
    p = _mixed(54, dtype, H)
    batch = Run(torch, p).launch(causal).results()
    hpc = _plan(torch, p, causal)["heads_per_chunk"]
    compared = 0
    for b, (sq, n, sk, L) in enumerate(p.sequences()):
        if n + L == 0:
            continue
        one_p = p.alone(b)
        one = Run(torch, one_p).launch(causal).results()
        assert same_bits(torch, one["dq"], batch["dq"][sq:sq + n]), "seq %d: dq differs between alone and in the batch" % b
        for name in ("dk_nope", "dv"):
            assert same_bits(torch, one[name], batch[name][sk:sk + L]), "seq %d: %s differs between alone and in the batch" % (b, name)
        if L and _plan(torch, one_p, causal)["heads_per_chunk"] == hpc:
            compared += 1
            assert same_bits(torch, one["dk_pe"], batch["dk_pe"][sk:sk + L]), "seq %d: dk_pe differs between alone and in the batch" % b
    print("dk_pe compared for %d sequences (%d heads per chunk in the batch)" % (compared, hpc))
    assert compared > 0


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2), ("bf16", False, 1)], ids=_cid)
def test_tensors_read_and_written_in_place_give_the_same_bits(dtype, causal, H):
    import torch
    p = _mixed(55, dtype, H)
    want = Run(torch, p).launch(causal).results()
    run = Run(torch, p, in_place=True).launch(causal)
    got = run.results()
    assert run.dkv.shape == (p.Tk, H, DN + DV) and got["dk_nope"].data_ptr() == run.dkv.data_ptr()
    for name in want:
        assert same_bits(torch, got[name].contiguous(), want[name]), name + " depends on the strides"


@pytest.mark.parametrize("causal", [True, "bottom-right", False], ids=_cid)
def test_max_seqlen_cuts_a_sequence_to_its_first_tokens(causal, oracle_mod):
    """max_seqlen_q = 40 and max_seqlen_k = 70 below the longest sequences: n and L are cut, the rows behind the cut are not written"""
    import torch
    p = Packed(56, "bf16", 2, NS, LS, lead=(1, 0), tail=(2, 3), max_sq=40, max_sk=70)
    assert [s[1] for s in p.sequences()] == [0, 1, 31, 33, 40, 40, 40, 1] and [s[3] for s in p.sequences()] == [63, 0, 70, 1, 70, 65, 70, 1]
    res = Run(torch, p).launch(causal).results()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, "max_seqlen cut " + _cid(causal))


def test_no_key_row_and_no_query_row():
    """total_k = 0 with total_q > 0 zeroes the owned dq rows (the key-side pointers null); total_q = 0 with total_k > 0 zeroes the owned
    key rows (the query-side pointers null) -- with one chunk (dk_pe from the dK/dV kernel) and with more (through the reduce)"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Packed(57, "fp16", 4, [5, 40], [0, 0], tail=(3, 0))
    run = Run(torch, p).launch(True)
    res = run.results()
    assert not res["dq"][:45].any() and _all_poison(torch, res["dq"][45:])
    for H in (1, 5):
        p = Packed(58, "bf16", H, [0, 0], [70, 130], lead=(0, 2), tail=(0, 3))
        run = Run(torch, p)
        d = _bwd_desc(torch, p, True)
        b = run.base
        d.k_nope, d.k_pe, d.v, d.cu_seqlens_q, d.cu_seqlens_k = b.kn.data_ptr(), b.kp.data_ptr(), b.v.data_ptr(), b.cu_q.data_ptr(), b.cu_k.data_ptr()
        d.dk_nope, d.dk_pe, d.dv = run.dk_nope.data_ptr(), run.dk_pe.data_ptr(), run.dv.data_ptr()
        need = int(lib.aule_attention_mla_prefill_backward_workspace_size(ctypes.byref(d)))
        assert need == (0 if H == 1 else _plan(torch, p)["n_chunks"] * p.Tk * DR * 4)
        d.workspace, d.workspace_bytes = (run.ws.data_ptr(), need) if need else (None, 0)
        _capi.check(lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)), "MLA prefill backward without a query")
        torch.cuda.synchronize()
        for g in (run.dk_nope, run.dk_pe, run.dv):
            assert not g[2:202].any() and _all_poison(torch, g[:2]) and _all_poison(torch, g[202:])


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2)], ids=_cid)
def test_autograd_on_the_slices_of_the_projections(dtype, causal, H, oracle_mod):
    """aule.flash_attention_mla_varlen on k_nope / v = the halves of a fused kv_b output and k_pe = columns 512.. of a down-projection
    (given as [T, 1, 64]); loss.backward() against the judge through the slices; out and lse bit-identical to
    aule.flash_attention_mla_prefill, which still refuses inputs that require grad"""
    import torch
    import aule
    ns = [0, 1, 31, 33, 129, 70]
    p = Packed(59, dtype, H, ns, ns, lead=(3, 3), tail=(5, 5))
    tdt = torch_dtype(dtype)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731
    q = up(p.q).requires_grad_(True)
    kvb = up(np.concatenate([p.kn, p.v], axis=2)).requires_grad_(True)
    down = torch.cat([torch.zeros(p.Tk, 512, dtype=tdt, device="cuda"), up(p.kp)], dim=1).requires_grad_(True)
    cu = torch.from_numpy(_i32(p.cu_q)).cuda()
    dout = up(p.dout)
    args = (q, kvb[..., :DN], down[:, 512:].unsqueeze(1), kvb[..., DN:], cu, cu)
    for maxima in ({}, dict(max_seqlen_q=p.max_sq, max_seqlen_k=p.max_sk)):
        q.grad = kvb.grad = down.grad = None
        out, lse = aule.flash_attention_mla_varlen(*args, causal=causal, return_lse=True, **maxima)
        assert out.shape == (p.Tq, H, DV) and lse.shape == (p.Tq, H) and not lse.requires_grad and out.requires_grad
        (out.float() * dout.float()).sum().backward()
        torch.cuda.synchronize()
        oq, ok = p.owned(), p.owned_k()
        assert not q.grad[torch.from_numpy(~oq).cuda()].any() and not kvb.grad[torch.from_numpy(~ok).cuda()].any(), "a row no sequence owns has zero gradient"
        assert not down.grad[:, :512].any() and not down.grad[torch.from_numpy(~ok).cuda()].any()
        res = dict(out=out, lse=lse, dq=q.grad, dk_nope=kvb.grad[..., :DN], dk_pe=down.grad[:, 512:], dv=kvb.grad[..., DN:])
        _judge(p, res, oracle_mod, causal, "autograd %s H%d" % (dtype, H))
    with torch.no_grad():
        plain, plain_lse = aule.flash_attention_mla_prefill(*args, causal=causal, return_lse=True, **maxima)
        same, same_lse = aule.flash_attention_mla_varlen(*args, causal=causal, return_lse=True, **maxima)
    torch.cuda.synchronize()
    own = torch.from_numpy(oq).cuda()
    for a, b in ((plain, out.detach()), (plain_lse, lse), (same, plain), (same_lse, plain_lse)):
        assert same_bits(torch, a[own], b[own])
    with pytest.raises(ValueError, match="no backward"):
        aule.flash_attention_mla_prefill(*args, causal=causal, **maxima)


def test_capture_replays_with_the_current_offsets():
    """forward and backward captured with both maxima and the workspace passed: no allocation, no synchronisation; a replay equals
    eager bit for bit, and after the offsets are overwritten in place the replay equals an eager call on the new contents"""
    import torch
    p = Packed(60, "bf16", 5, [100, 7, 60, 33], [100, 200, 3, 97], max_sq=128, max_sk=256)
    assert p.Tq == 200 and p.Tk == 400 and _plan(torch, p)["reduce"] == 1
    names = ("out", "lse") + GRADS

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
    assert not same_bits(torch, want2["dq"], want["dq"])
    run.base.cu_q.copy_(torch.tensor(new_q, dtype=torch.int32, device="cuda"))
    run.base.cu_k.copy_(torch.tensor(new_k, dtype=torch.int32, device="cuda"))
    for n in names:
        getattr(run, n).view(torch.uint8).fill_(POISON)
    g.replay()
    torch.cuda.synchronize()
    for n in names:
        assert same_bits(torch, getattr(run, n), want2[n]), n + ": replay does not see the current offsets"


@pytest.mark.parametrize("dtype,causal,H", [("bf16", True, 5), ("fp16", "bottom-right", 2), ("bf16", False, 1)], ids=_cid)
def test_hostile_memory_and_hostile_offsets(dtype, causal, H, oracle_mod):
    """Every tensor carved from one arena, outputs, workspace and guard bands 0xFF; offsets negative, decreasing, beyond the totals,
    INT32_MIN and INT32_MAX.  After the clamps (max_seqlen_q = 40, max_seqlen_k = 64) the sequences own q rows [0, 30), [30, 70),
    [95, 120) and k rows [0, 50), [50, 114), [115, 150): exactly those are written and right, inputs and guards are intact.  Then the
    same launch with OVERLAPPING sequences (a doubly owned row has no specified value): guards and inputs intact, the rows outside
    every sequence still poisoned, the uniquely owned rows finite."""
    import torch
    cu_q = [I32_MIN, 30, I32_MAX, 100, 95, 130, -3]
    cu_k = [-9, 50, I32_MAX, 140, 115, 200, I32_MIN]
    p = Packed(61, dtype, H, None, None, max_sq=40, max_sk=64, cu_q=cu_q, cu_k=cu_k, Tq=120, Tk=150)
    assert [(s, n, sk, L) for s, n, sk, L in p.sequences() if n + L] == [(0, 30, 0, 50), (30, 40, 50, 64), (95, 25, 115, 35)]
    tdt = torch_dtype(dtype)
    ws_bytes = _ws_bytes(torch, p, causal)
    regions = [("q", p.Tq * H * DQ * 2, "in"), ("k_nope", p.Tk * H * DN * 2, "in"), ("k_pe", p.Tk * DR * 2, "in"), ("v", p.Tk * H * DV * 2, "in"),
               ("dout", p.Tq * H * DV * 2, "in"), ("cu_seqlens_q", (p.B + 1) * 4, "in"), ("cu_seqlens_k", (p.B + 1) * 4, "in"),
               ("out", p.Tq * H * DV * 2, "out"), ("lse", p.Tq * H * 4, "out"), ("dq", p.Tq * H * DQ * 2, "out"), ("dk_nope", p.Tk * H * DN * 2, "out"),
               ("dk_pe", p.Tk * DR * 2, "out"), ("dv", p.Tk * H * DV * 2, "out"), ("workspace", max(ws_bytes, 16), "ws")]
    ar = Arena(torch, regions, H * DQ * 2)
    orig = {n: ar.upload(n, torch.from_numpy(a).to(tdt)) for n, a in (("q", p.q), ("k_nope", p.kn), ("k_pe", p.kp), ("v", p.v), ("dout", p.dout))}
    orig["cu_seqlens_q"] = ar.upload("cu_seqlens_q", _i32(cu_q))
    orig["cu_seqlens_k"] = ar.upload("cu_seqlens_k", _i32(cu_k))
    views = lambda: dict(out=ar.view("out", tdt, (p.Tq, H, DV)), lse=ar.view("lse", torch.float32, (p.Tq, H)), dq=ar.view("dq", tdt, (p.Tq, H, DQ)),   # noqa: E731
                         dk_nope=ar.view("dk_nope", tdt, (p.Tk, H, DN)), dk_pe=ar.view("dk_pe", tdt, (p.Tk, DR)), dv=ar.view("dv", tdt, (p.Tk, H, DV)))
    ar.fill(POISON)
    _launch(torch, p, {n: ar.ptr(n) for n, _, _ in regions}, causal, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    assert ar.guards_intact(), "guard bytes written: %r" % (ar.damage(),)
    for n, o in orig.items():
        assert ar.unchanged(n, o), "input %s was written" % n
    res = views()
    _unowned_still_poisoned(torch, p, res)
    _judge(p, res, oracle_mod, causal, "hostile %s H%d" % (dtype, H))
    # overlapping: q rows [0, 30) and [20, 60), k rows [0, 50) and [40, 104); rows 20 .. 29 and 40 .. 49 are doubly owned
    cu_q2, cu_k2 = [0, 30, 20, 60, 60, 60, 60], [0, 50, 40, 104, 104, 104, 104]
    orig["cu_seqlens_q"] = ar.upload("cu_seqlens_q", _i32(cu_q2))
    orig["cu_seqlens_k"] = ar.upload("cu_seqlens_k", _i32(cu_k2))
    ar.fill(POISON)
    _launch(torch, p, {n: ar.ptr(n) for n, _, _ in regions}, causal, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    assert ar.guards_intact(), "guard bytes written: %r" % (ar.damage(),)
    for n, o in orig.items():
        assert ar.unchanged(n, o), "input %s was written" % n
    res = views()
    assert _all_poison(torch, res["dq"][60:]) and _all_poison(torch, res["out"][60:])
    for n in ("dk_nope", "dk_pe", "dv"):
        assert _all_poison(torch, res[n][104:]), n
    assert bool(torch.isfinite(res["dq"][:20].float()).all()) and bool(torch.isfinite(res["dq"][30:60].float()).all())
    for n in ("dk_nope", "dk_pe", "dv"):
        assert bool(torch.isfinite(res[n][:40].float()).all()) and bool(torch.isfinite(res[n][50:104].float()).all()), n
