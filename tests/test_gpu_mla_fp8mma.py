"""The paged MLA with FP8 matrix products (aule.flash_attention_mla_paged_fp8mma, csrc/fa_fwd_mla_paged_fp8mma_gfx950.hip; DESIGN.md
3.19) on the GPU, on the twin's cases (tests/test_gpu_mla.py, test_gpu_mla_fp8.py) and against the two fp64 models of
tests/test_gpu_paged_prefill_fp8mma.py restated for the latent cache:
  the q-rounded judge   fp64 attention over kv_scale * codes with q replaced by codes * scales of aule.quantize_rows_fp8;
  the P model           the same with exp(s - rowmax) 2^8 rounded to e4m3 before the PV product.
lse is held to LSE_ATOL against the judge; out to fwd_tol's atol + 2 E_P, E_P = max |P model - judge|, and its rms error to
2 rms(P model - judge) + atol: bounds that come from the references alone."""
import ctypes
import math

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from test_gpu_mla import LSE_ATOL, QK, VD, _desc, _nsplit, _poisoned
from test_gpu_mla_fp8 import NAN_CODE, Fp8Case, _desc8
from util import fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

CASES = {  # id: (constructor arguments, scale)
    "bf16-H16-split": ((11, "bf16", 16, 16, [1, 33, 200]), dict(extra_cols=2), None),
    "fp16-H128-bs64": ((12, "fp16", 128, 64, [1, 64, 65, 130]), dict(extra_cols=0), None),
    "bf16-H5-bs24": ((13, "bf16", 5, 24, [1, 33, 200]), dict(extra_cols=2), 192 ** -0.5),
    "fp16-H24-ragged": ((14, "fp16", 24, 16, [70, 1, 40]), dict(ns=[3, 1, 2]), None),
    "bf16-H16-strided": ((15, "bf16", 16, 16, [70, 2, 0, 40]), dict(ns=[3, 4, 2, 2], lead=2, tail=3, q_pad=8), None),
}
_cases = {}


def _case(name):
    if name not in _cases:
        args, kw, scale = CASES[name]
        _cases[name] = (Fp8Case(*args, **kw), scale)
    return _cases[name]


def _run(torch, c, scale=None, tensors=None, codes=None):
    import aule
    q, kv, bt, cl, cu = tensors or c.device(torch)
    return aule.flash_attention_mla_paged_fp8mma(q, kv if codes is None else codes, bt, cl, cu, max_seqlen_q=None if cu is None else c.max_sq,
                                                 scale=scale, return_lse=True, kv_scale=c.kv_scale.cuda())


def _models(c, scale):
    """(judge out [T, Hq, 512], judge lse [T, Hq], P-model out) in fp64: zeros / -inf where a row sees no key; once per case"""
    import torch
    import aule
    if "fp8mma" not in c._ref:
        codes, scales = aule.quantize_rows_fp8(torch.from_numpy(c.q))
        qh = (codes.float() * scales).numpy().astype(np.float64)
        e4m3 = lambda x: torch.from_numpy(x.astype(np.float32)).to(torch.float8_e4m3fn).float().numpy().astype(np.float64)   # noqa: E731
        sc = 1.0 / math.sqrt(QK) if scale is None else scale
        out_j, out_p, lse_j = np.zeros((c.T, c.Hq, VD)), np.zeros((c.T, c.Hq, VD)), np.full((c.T, c.Hq), -np.inf)
        for sel, rows, ctx in c._rows():
            for b, r, n in zip(sel, rows, ctx):
                if n > 0:
                    j = np.arange(n)
                    k = c.kv[c.bt[b][j // c.bs], j % c.bs]
                    s = qh[r] @ k.T * sc
                    m = s.max(axis=-1, keepdims=True)
                    w = np.exp(s - m)
                    den = w.sum(axis=-1, keepdims=True)
                    out_j[r], out_p[r] = w @ k[:, :VD] / den, e4m3(w * 256.0) @ k[:, :VD] / (256.0 * den)
                    lse_j[r] = (m + np.log(den))[:, 0]
        c._ref["fp8mma"] = (out_j, lse_j, out_p)
    return c._ref["fp8mma"]


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_lse_vs_the_models(name):
    """Test 1.  The measured maxima are printed; DESIGN.md section 4 quotes them."""
    import torch
    c, scale = _case(name)
    tensors = c.device(torch)
    out, lse = _poisoned(torch, c)
    got = _run(torch, c, scale, tensors)
    torch.cuda.synchronize()
    d = _desc8(torch, c, tensors, out, lse, c.kv_scale.cuda())
    d.scale = scale or 0.0   # (0: the library's 1 / sqrt(576))
    if name == "bf16-H16-split":
        assert _nsplit(_desc(torch, c, tensors, out, lse)) > 1      # (the plan hook takes the 16-bit descriptor)
    # unowned rows keep their poison: the C entry on poisoned buffers, which must also give the wrapper's bits
    from aule import _capi
    assert _capi.get_lib().aule_attention_mla_paged_fp8mma_ex(ctypes.byref(d)) == 0, _capi.get_lib().aule_get_error()
    torch.cuda.synchronize()
    own = c.owned()
    dev_own = torch.from_numpy(own).cuda()
    assert bool((out.view(torch.int16)[~dev_own] == -1).all()) and bool((lse.view(torch.int32)[~dev_own] == -1).all())
    assert same_bits(torch, out[dev_own], got[0][dev_own]) and same_bits(torch, lse[dev_own], got[1][dev_own])
    out_j, lse_j, out_p = (x[own] for x in _models(c, scale))
    out, lse = out.float().cpu().numpy().astype(np.float64)[own], lse.cpu().numpy().astype(np.float64)[own]
    atol = fwd_tol(c.dtype, c.vmax)[0]
    none = np.isneginf(lse_j)
    lerr = float(np.abs(lse[~none] - lse_j[~none]).max())
    e_p, err = float(np.abs(out_p - out_j).max()), float(np.abs(out - out_j).max())
    rms = lambda x: float(np.sqrt(np.mean(np.square(x))))   # noqa: E731
    rms_p, rms_k = rms(out_p - out_j), rms(out - out_j)
    print("fp8mma mla %s: |lse err| %.3g (bound %.3g); max |out - judge| %.4g, E_P %.4g (bound atol %.3g + 2 E_P); rms %.4g, model rms %.4g; "
          "rows without a key %d" % (name, lerr, LSE_ATOL, err, e_p, atol, rms_k, rms_p, int(none.sum())))
    assert not np.isnan(lse).any() and not np.isnan(out).any()
    assert np.array_equal(np.isneginf(lse), none), "lse must be -inf exactly where a row sees no key"
    assert bool((out[none] == 0).all()), "a row that sees no key must be zeros"
    assert lerr <= LSE_ATOL
    assert err <= atol + 2.0 * e_p
    assert rms_k <= 2.0 * rms_p + atol
    if name == "bf16-H16-strided":
        assert none.sum() == (2 + 2) * c.Hq   # n > L: two tokens at negative positions; L = 0: two more


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("Hq", [16, 128])
def test_one_visible_key_gives_that_value_row_exactly(dtype, Hq):
    """Test 2.  L = n: token 0 sees key 0 alone, p = 2^8 and l = 2^8 exactly, so its rows are code(row 0)[:512] * kv_scale -- formed in fp32,
    rounded once to the dtype -- bit for bit (the sign of a zero aside).  Pins the column order of the value image."""
    import torch
    c = Fp8Case(16, dtype, Hq, 16, [3, 1], ns=[3, 1])
    out, _ = _run(torch, c)
    torch.cuda.synchronize()
    for b in range(c.B):
        row = c.codes[int(c.bt[b][0]), 0, :VD].float() * c.kv_scale          # fp32
        want = row.to(torch_dtype(dtype)).expand(Hq, VD)
        want = torch.where(want == 0, torch.zeros_like(want), want)
        got = out[int(c.starts[b])].cpu()
        got = torch.where(got == 0, torch.zeros_like(got), got)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (b, int((got != want).sum()))
        assert int((want != 0).sum()) > Hq * VD // 2


@pytest.mark.parametrize("name,split", [("bf16-H16-split", True), ("fp16-H24-ragged", False)])
def test_nan_codes_where_nothing_may_be_read(name, split):
    """Test 3.  Code 0x7F in every cache row that is no live key (the blocks no table names, the slots past L): the results equal the run
    with zeros there bit for bit."""
    import torch
    c, scale = _case(name)
    tensors = c.device(torch)
    live = torch.from_numpy(c.live_slots()).view(-1, 1)
    flat = c.codes.view(torch.uint8).view(-1, QK)
    runs = []
    for fill in (0, NAN_CODE):
        codes = torch.where(live, flat, torch.full_like(flat, fill)).view(c.codes.shape).view(torch.float8_e4m3fn).cuda()
        runs.append(_run(torch, c, scale, tensors, codes=codes))
    torch.cuda.synchronize()
    assert (_nsplit(_desc(torch, c, tensors, runs[0][0], runs[0][1])) > 1) == split
    own = torch.from_numpy(c.owned()).cuda()
    assert not bool(torch.isnan(runs[1][0][own].float()).any()) and not bool(torch.isnan(runs[1][1][own]).any())
    assert same_bits(torch, runs[0][0][own], runs[1][0][own]) and same_bits(torch, runs[0][1][own], runs[1][1][own])


@pytest.mark.parametrize("cu", [None, [1, 5, 100, 200], [5, 3, 4, 2], [-5, 2, 1, 2 ** 31 - 1]], ids=["sane", "past-T", "backwards", "negative"])
def test_c_entry_inside_an_arena(cu):
    """Test 4.  Every tensor between guard bands, outputs and workspace poisoned, hostile offsets: the guards intact, the inputs unchanged,
    nothing outside the owned rows written, two runs the same bits; with sane offsets the owned rows equal the Python call's."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    c = Fp8Case(52, "bf16", 24, 64, [700, 3, 129], ns=[3, 1, 2], table_lens=[1024] * 3, extra_cols=0, lead=1, tail=2)
    offs = c.cu if cu is None else np.array(cu, dtype=np.int32)
    own = np.zeros(c.T, dtype=bool)
    for b in range(c.B):   # the contract's clamps
        s = min(max(int(offs[b]), 0), c.T)
        e = min(max(int(offs[b + 1]), s), c.T)
        own[s:s + min(e - s, c.max_sq)] = True
    own = torch.from_numpy(own).cuda()
    dt = torch_dtype(c.dtype)
    host = dict(q=torch.from_numpy(c.q).to(dt), kv=c.codes.view(torch.uint8), bt=torch.from_numpy(c.bt), cl=torch.from_numpy(c.cl), ks=c.kv_scale,
                cu=torch.from_numpy(offs))
    probe = _desc8(torch, c, c.device(torch), *_poisoned(torch, c), c.kv_scale.cuda())
    size = int(lib.aule_attention_mla_paged_fp8mma_workspace_size(ctypes.byref(probe)))
    assert size > 0 and size == lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(probe))
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in host.items()]
    regions += [("out", c.T * c.Hq * VD * 2, "out"), ("lse", c.T * c.Hq * 4, "out"), ("ws", size, "ws")]
    arena = Arena(torch, regions, QK * 2)
    kept = {k: arena.upload(k, v) for k, v in host.items()}
    tensors = (arena.view("q", dt, (c.T, c.Hq, QK)), arena.view("kv", torch.float8_e4m3fn, tuple(c.codes.shape)),
               arena.view("bt", torch.int32, c.bt.shape), arena.view("cl", torch.int32, c.cl.shape), arena.view("cu", torch.int32, offs.shape))
    out, lse = arena.view("out", dt, (c.T, c.Hq, VD)), arena.view("lse", torch.float32, (c.T, c.Hq))
    d = _desc8(torch, c, tensors, out, lse, arena.view("ks", torch.float32, (1,)), arena.bytes("ws"))
    runs = []
    for _ in range(2):
        arena.fill(POISON)
        assert lib.aule_attention_mla_paged_fp8mma_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert arena.guards_intact(), arena.damage()
        for k, v in kept.items():
            assert arena.unchanged(k, v), k
        assert bool((out.view(torch.int16)[~own] == -1).all()) and bool((lse.view(torch.int32)[~own] == -1).all())
        runs.append((out.clone(), lse.clone()))
    assert same_bits(torch, runs[0][0], runs[1][0]) and same_bits(torch, runs[0][1], runs[1][1])
    if cu is None:
        want, want_lse = _run(torch, c)
        assert same_bits(torch, out[own], want[own]) and same_bits(torch, lse[own], want_lse[own])


def test_capture_replays_with_the_current_lengths():
    """Test 5.  One torch.cuda.graph of a split call; context_lens overwritten in place: a replay equals a fresh eager call."""
    import torch
    import aule
    c = Fp8Case(61, "bf16", 16, 64, [1500, 700], ns=[2, 1], table_lens=[2048, 2048], extra_cols=0)
    q, kv, bt, cl, cu = c.device(torch)
    ks = c.kv_scale.cuda()
    fn = lambda: aule.flash_attention_mla_paged_fp8mma(q, kv, bt, cl, cu, max_seqlen_q=2, return_lse=True, kv_scale=ks)   # noqa: E731
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
    for new_cl in ([1500, 700], [40, 2048], [0, 1], [2000, 333]):
        cl.copy_(torch.tensor(new_cl, device="cuda", dtype=torch.int32))
        want, want_lse = fn()
        out.zero_(); lse.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(torch, out, want) and same_bits(torch, lse, want_lse), new_cl
    assert not same_bits(torch, want, eager)
