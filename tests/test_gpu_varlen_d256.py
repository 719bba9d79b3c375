"""aule.flash_attention_varlen_d256 and its C entries on the GPU against a plain fp64 NumPy attention per sequence and head.  Bounds:
util.fwd_tol for out, 1e-3 for lse, util.BWD_TOL scaled by max(1, max|grad|) for the gradients; every element is compared."""
from types import SimpleNamespace

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from test_gpu_varlen import CODE, I32_MAX, I32_MIN, _clamp, _launch
from util import BWD_TOL, assert_close, fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

D = 256
# query lengths [70, 1, 0, 129] against key lengths [200, 65, 63, 129]: two 128-row blocks at g = 2, a one-row block, an empty sequence
# in the middle, key tails of 8, 1 and 63 in a 64-key tile, a second dK/dV block of 1 and 72 keys, L < n and L > n
CQ, CK = [0, 70, 71, 71, 200], [0, 200, 265, 328, 457]
NAMES = ("out", "lse", "dq", "dk", "dv")
ENTRIES = ["aule_attention_varlen_d256_" + s for s in ("forward_ex", "backward_ex", "backward_workspace_size")]


def judge(q, k, v, do, cu_q, cu_k, causal, window, max_sq=I32_MAX, max_sk=I32_MAX):
    """fp64 out, lse, dq, dk, dv of every (sequence, head); NaN in the rows that no sequence owns"""
    (Tq, Hq, _), (Tk, Hkv, _) = q.shape, k.shape
    g, scale = Hq // Hkv, D ** -0.5
    r = {n: np.full(s, np.nan) for n, s in zip(NAMES, (q.shape, (Tq, Hq), q.shape, k.shape, k.shape))}
    for b in range(len(cu_q) - 1):   # (_clamp: offsets clamped to the totals, lengths to the maxima)
        (sq, n), (sk, L) = _clamp(cu_q, b, Tq, max_sq), _clamp(cu_k, b, Tk, max_sk)
        Q, K = slice(sq, sq + n), slice(sk, sk + L)
        r["dk"][K] = r["dv"][K] = 0.0
        pos = np.arange(n)[:, None] + (L - n if CODE[causal] == 2 else 0)
        j = np.arange(L)[None, :]
        vis = ((j <= pos) | (CODE[causal] == 0)) & ((pos - j < window) | (window <= 0))
        for h in range(Hq):
            qs, ks, vs, ds = q[Q, h], k[K, h // g], v[K, h // g], do[Q, h]
            s = np.where(vis, qs @ ks.T * scale, -np.inf)
            m = np.where(vis.any(1), s.max(1, initial=-np.inf), 0.0)
            p = np.exp(s - m[:, None])
            l = np.where(vis.any(1), p.sum(1), 1.0)
            p = p / l[:, None]
            o = r["out"][Q, h] = p @ vs
            r["lse"][Q, h] = np.where(vis.any(1), m + np.log(l), -np.inf)
            dsc = p * (ds @ vs.T - (ds * o).sum(1)[:, None])
            r["dq"][Q, h] = dsc @ ks * scale
            r["dk"][K, h // g] += dsc.T @ qs * scale
            r["dv"][K, h // g] += p.T @ ds
    return r


def make(seed, dtype, Hq, Hkv, Tq, Tk):
    """q, k, v as in-place slices of one fused [Tk + 11, Hq + 2 Hkv, 256] projection (a leaf) and dout; then the fp64 values of the four"""
    import torch
    rng = np.random.RandomState(seed)
    x, do = (torch.from_numpy(rng.randn(*s).astype(np.float32)).to("cuda", torch_dtype(dtype)) for s in ((Tk + 11, Hq + 2 * Hkv, D), (Tq, Hq, D)))
    x.requires_grad_(True)
    dev = [x[:Tq, :Hq], x[:Tk, Hq:Hq + Hkv], x[:Tk, Hq + Hkv:], do]
    return dev, [t.detach().double().cpu().numpy() for t in dev]


def run(q, k, v, do, cu_q, cu_k, causal, window, **kw):
    import torch
    import aule
    cu = [torch.tensor(a, dtype=torch.int32, device="cuda") for a in (cu_q, cu_k)]
    out, lse = aule.flash_attention_varlen_d256(q, k, v, *cu, causal=causal, window_size=window, return_lse=True, **kw)
    dq, dk, dv, gx = torch.autograd.grad(out, (q, k, v, q._base), do)
    return dict(out=out.detach(), lse=lse, dq=dq, dk=dk, dv=dv, gx=gx)


def check(got, ref, dtype, vmax, what, sides=1):
    """every element of every row that the reference owns (is not NaN) within the project's bounds"""
    for n, r in ref.items():
        rows = ~np.isnan(r).reshape(len(r), -1).all(1)
        a, r = got[n].double().cpu().numpy()[rows], r[rows]
        a, r = (np.where(np.isneginf(x), -1e30, x) for x in (a, r))   # (lse of a row without a key: -inf in both, or far out of tolerance)
        atol, rtol = fwd_tol(dtype, vmax, sides) if n == "out" else (1e-3, 0.0) if n == "lse" else BWD_TOL[dtype]
        if n in ("dq", "dk", "dv"):
            atol *= max(1.0, float(np.abs(r).max(initial=0.0)))
        assert_close(a, r, atol, rtol, "%s %s" % (what, n))


@pytest.mark.parametrize("heads", [(4, 2), (3, 1), (2, 2)], ids=lambda h: "H%dkv%d" % h)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("window", [-1, 17, 100])
@pytest.mark.parametrize("causal", [False, True, "bottom-right"])
def test_block_and_tile_boundaries_in_place_through_autograd(causal, window, dtype, heads):
    dev, host = make(1, dtype, heads[0], heads[1], 200, 457)
    got = run(*dev, CQ, CK, causal, window)
    check(got, judge(*host, CQ, CK, causal, window), dtype, np.abs(host[2]).max(), "%s w%d" % (causal, window))
    assert not got["gx"][457:].any() and not got["gx"][200:, :heads[0]].any(), "gradient of rows outside every sequence"


def test_bit_identities_and_cuts():
    """two runs agree; a sequence alone gives the bits it gives in the batch; a window that masks nothing is no window; the cuts cut"""
    import torch
    dev, host = make(3, "fp16", 4, 2, 200, 457)
    batch, again, wide, plain = (run(*dev, CQ, CK, "bottom-right", w) for w in (100, 100, 329, -1))   # (329 = longest n + longest L: masks nothing)
    (a, e), (ka, ke) = CQ[3:], CK[3:]   # the last sequence, 129 x 129 from unaligned offsets: three query blocks, two key blocks
    alone = run(dev[0][a:e], dev[1][ka:ke], dev[2][ka:ke], dev[3][a:e], [0, e - a], [0, ke - ka], "bottom-right", 100)
    for n in NAMES:
        lo, hi = (ka, ke) if n in ("dk", "dv") else (a, e)
        assert same_bits(torch, alone[n], batch[n][lo:hi]), "the sequence alone: " + n
        assert same_bits(torch, batch[n], again[n]) and same_bits(torch, plain[n], wide[n]), n
    got = run(*dev, CQ, CK, True, 17, max_seqlen_q=50, max_seqlen_k=100)
    check(got, judge(*host, CQ, CK, True, 17, 50, 100), "fp16", np.abs(host[2]).max(), "cut")
    assert not got["dq"][50:70].any() and not got["dk"][100:200].any(), "rows past the cut carry a gradient"


@pytest.mark.parametrize("causal,window", [(True, -1), ("bottom-right", 17)])
def test_hostile_memory_hostile_offsets_and_capture(causal, window):
    """bf16 tensors of one allocation between NaN guard bands, outputs and workspace NaN-filled, through the C entries.  After the clamps and
    the cuts (100 queries, 150 keys) the sequences own q rows [0, 171) and k rows [0, 150), [200, 300); the last has no key.  Then a capture."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    Hq, Hkv, Tq, Tk = 4, 2, 200, 300
    cu_q, cu_k = [I32_MIN, 70, 71, 71, I32_MAX], [-9, 200, 265, 1000, I32_MAX]
    dev, host = make(5, "bf16", Hq, Hkv, Tq, Tk)
    qb, kb, ws = Tq * Hq * D * 2, Tk * Hkv * D * 2, (Tq * Hq * 4 + 255) // 256 * 256
    sizes = dict(q=qb, k=kb, v=kb, dout=qb, cu_seqlens_q=20, cu_seqlens_k=20, out=qb, lse=Tq * Hq * 4, dq=qb, dk=kb, dv=kb, workspace=ws)
    ar = Arena(torch, [(n, b, "in" if i < 6 else "out") for i, (n, b) in enumerate(sizes.items())], D * 2)
    orig = {n: ar.upload(n, x) for n, x in zip(sizes, [x.detach() for x in dev] + [np.array(cu_q, np.int32), np.array(cu_k, np.int32)])}
    ar.fill(POISON)
    shapes = dict(out=(Tq, Hq, D), lse=(Tq, Hq), dq=(Tq, Hq, D), dk=(Tk, Hkv, D), dv=(Tk, Hkv, D))
    res = {n: ar.view(n, torch.float32 if n == "lse" else torch.bfloat16, s) for n, s in shapes.items()}
    # tests/test_gpu_varlen.py's launch (forward, then backward, on these addresses), given the head_dim 256 entries under the names it calls
    lib256 = SimpleNamespace(**{n.replace("_d256", ""): getattr(lib, n) for n in ENTRIES})
    p = SimpleNamespace(dtype="bf16", B=4, Hq=Hq, Hkv=Hkv, D=D, Tq=Tq, Tk=Tk, max_sq=100, max_sk=150)
    args = (torch, lib256, p, {n: ar.ptr(n) for n in sizes}, causal, window, ws)
    _launch(*args)
    torch.cuda.synchronize()
    assert ar.guards_intact(), "guard bytes written: %r" % (ar.damage(),)
    assert all(ar.unchanged(n, o) for n, o in orig.items()), "an input was written"
    for n in NAMES:
        free = res[n][150:200] if n in ("dk", "dv") else res[n][171:]
        assert bool((free.contiguous().view(torch.uint8) == POISON).all()), n + ": a row of no sequence was written"
    check(res, judge(*host, cu_q, cu_k, causal, window, 100, 150), "bf16", np.abs(host[2]).max(), "hostile")
    first = res["out"].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # (the eager call above was the warm-up)
        _launch(*args)
    for n, cu in (("cu_seqlens_q", [0, 100, 100, 150, 200]), ("cu_seqlens_k", [0, 40, 190, 200, 300])):
        ar.view(n, torch.int32, (5,)).copy_(torch.tensor(cu, dtype=torch.int32))
    _launch(*args)
    torch.cuda.synchronize()
    now = {n: t.clone() for n, t in res.items()}
    assert not same_bits(torch, now["out"], first), "the new offsets must change the result"
    for _ in range(2):   # (several replays over NaN-filled outputs: each must equal the eager result)
        ar.fill(POISON)
        g.replay()
        torch.cuda.synchronize()
        for n in NAMES:
            assert same_bits(torch, res[n], now[n]), n + ": replay differs from eager"


@pytest.mark.parametrize("heads,causal", [((4, 2), True), ((3, 1), False)])
def test_equal_lengths_agree_with_the_dense_entry(heads, causal):
    import aule
    (Hq, Hkv), S = heads, 192
    dev, host = make(6, "bf16", Hq, Hkv, 2 * S, 2 * S)
    got = run(*dev, [0, S, 2 * S], [0, S, 2 * S], causal, -1)
    q, k, v = (x.detach().reshape(2, S, -1, D).transpose(1, 2).contiguous().requires_grad_(True) for x in dev[:3])
    out = aule.flash_attention(q, k, v, causal=causal)
    out.backward(dev[3].view(2, S, Hq, D).transpose(1, 2))
    flat = {n: x.transpose(1, 2).reshape(2 * S, -1, D).double().cpu().numpy() for n, x in dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad).items()}
    check(got, flat, "bf16", np.abs(host[2]).max(), "dense", sides=2)
