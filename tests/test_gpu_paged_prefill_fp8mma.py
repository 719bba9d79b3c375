"""The paged prefill with FP8 matrix products (aule.flash_attention_paged_prefill_fp8mma, csrc/fa_fwd_paged_prefill_fp8mma_gfx950.hip)
on the GPU, on the twin's ragged batch (tests/test_gpu_paged_prefill.py) and against two fp64 models of its arithmetic:
  the q-rounded judge   fp64 attention over the dequantised caches with q replaced by codes * scales of aule.quantize_rows_fp8;
  the P model           the same with p = exp(s - rowmax) 2^8 rounded to e4m3 before the PV product (final max, one pass).
The LSE never sees the rounding of P, so it is held to the twin's bound against the judge; the output is held to the fwd tolerance
plus twice the P model's own distance from the judge (the kernel rounds P against the running max of 64-key tiles, the model against
the final max: the same error law in another realisation)."""
import ctypes
import math

import numpy as np
import pytest

import hostile
from hostile import POISON, Arena
from test_gpu_paged_prefill import INT32_MIN, LS, NS, Ragged, _desc
from test_gpu_paged_query import LSE_ATOL, _decode
from util import fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

SHAPES = [  # dtype, Hq, Hkv, D, block size, window
    ("bf16", 32, 8, 128, 16, -1),
    ("fp16", 32, 8, 128, 16, 16),
    ("fp16", 6, 2, 64, 24, -1),
    ("bf16", 6, 2, 64, 1, 300),
    ("fp16", 8, 8, 128, 24, -1),
    ("bf16", 8, 8, 128, 128, 300),
]
_problems = {}


def _problem(dtype, Hq, Hkv, D, bs):
    key = (dtype, Hq, Hkv, D, bs)
    if key not in _problems:
        _problems[key] = Ragged(61, dtype, "fp8", Hq, Hkv, D, bs, NS, LS)
    return _problems[key]


def _e4m3(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).float().numpy().astype(np.float64)


def _models(p, window=-1, scale=None, rounded=True, **kw):
    """(judge out [T, Hq, D], judge lse [T, Hq], P-model out) in fp64 on the owned rows (zeros / -inf where a row sees no key; rows of no
    sequence: zeros and NaN); computed once per (window, scale, lengths) and kept on the problem.  rounded=False (tools/fuzz_serving.py):
    the same three with q as it is, not its e4m3 codes"""
    import torch
    import aule
    key = ("fp8mma", window, scale, rounded, tuple((k, tuple(np.asarray(v).tolist()) if k != "max_sq" else v) for k, v in sorted(kw.items())))
    if key in p._ref:
        return p._ref[key]
    codes, scales = aule.quantize_rows_fp8(torch.from_numpy(p.q))
    qh = (codes.float() * scales).numpy().astype(np.float64) if rounded else p.q.astype(np.float64)
    g, scale = p.Hq // p.Hkv, 1.0 / math.sqrt(p.D) if scale is None else scale
    out_j = np.zeros((p.T, p.Hq, p.D))
    out_p = np.zeros((p.T, p.Hq, p.D))
    lse_j = np.full((p.T, p.Hq), np.nan)
    for b, s, n, L in p.sequences(**kw):
        if n == 0:
            continue
        lse_j[s:s + n] = -np.inf
        if L == 0:
            continue
        j = np.arange(L)
        k, v = p.K[p.bt[b][j // p.bs], j % p.bs], p.V[p.bt[b][j // p.bs], j % p.bs]      # [L, Hkv, D]
        sc = np.einsum("nhgd,lhd->nhgl", qh[s:s + n].reshape(n, p.Hkv, g, p.D), k) * scale
        pos = L - n + np.arange(n)
        see = j[None, :] <= pos[:, None]
        if window > 0:
            see &= pos[:, None] - j[None, :] < window
        sc = np.where(see[:, None, None, :], sc, -np.inf)
        m = sc.max(axis=-1)
        any_key = np.isfinite(m)
        w = np.exp(sc - np.where(any_key, m, 0.0)[..., None])
        den = w.sum(axis=-1)
        safe = np.where(any_key, den, 1.0)[..., None]
        out_j[s:s + n] = (np.einsum("nhgl,lhd->nhgd", w, v) / safe).reshape(n, p.Hq, p.D)
        out_p[s:s + n] = (np.einsum("nhgl,lhd->nhgd", _e4m3(w * 256.0), v) / (256.0 * safe)).reshape(n, p.Hq, p.D)
        with np.errstate(divide="ignore"):
            lse_j[s:s + n] = np.where(any_key, m + np.log(np.where(any_key, den, 1.0)), -np.inf).reshape(n, p.Hq)
    p._ref[key] = (out_j, lse_j, out_p)
    return p._ref[key]


def _rms(x):
    return float(np.sqrt(np.mean(np.square(x)))) if x.size else 0.0


def _judge(p, out, lse, window, what, scale=None, lse_atol=LSE_ATOL, out_rtol=0.0, **kw):
    """test 1's rules on the owned rows; prints the measured figures before it asserts and returns (max |out - judge|, max |lse err|, the
    largest |out - judge| as a share of its bound).  (scale, lse_atol, out_rtol: tools/fuzz_serving.py's draws, whose rows of one or two
    keys have E_P = 0 and are left with the rounding of out to storage alone, fwd_tol's rtol |judge|; every test of this file keeps the
    defaults.)"""
    own = p.owned(**kw)
    out_j, lse_j, out_p = (x[own] for x in _models(p, window, scale, **kw))
    out, lse = out.float().cpu().numpy().astype(np.float64)[own], lse.cpu().numpy().astype(np.float64)[own]
    atol = fwd_tol(p.dtype, p.vmax)[0]
    none = np.isneginf(lse_j)
    lerr = float(np.abs(lse[~none] - lse_j[~none]).max()) if (~none).any() else 0.0
    lse_bound = np.broadcast_to(np.asarray(lse_atol, dtype=np.float64), (p.T, p.Hq))[own]      # (a scalar, or a bound per row [T, Hq])
    lse_atol = float(lse_bound.max()) if lse_bound.size else 0.0
    e_p, err = float(np.abs(out_p - out_j).max()), float(np.abs(out - out_j).max())
    rms_p, rms_k = _rms(out_p - out_j), _rms(out - out_j)
    print("%s: %d rows, |lse err| %.3g (bound %.3g); max |out - judge| %.4g, E_P %.4g, ratio %.3f (bound atol %.3g + 2 E_P); "
          "rms %.4g, model rms %.4g, ratio %.3f; rows without a key %d"
          % (what, int(own.sum()), lerr, lse_atol, err, e_p, err / e_p if e_p else 0.0, atol, rms_k, rms_p, rms_k / rms_p if rms_p else 0.0,
             int(none.sum())))
    assert not np.isnan(lse).any() and not np.isnan(out).any(), what
    assert np.array_equal(np.isneginf(lse), none), "%s: lse must be -inf exactly where a row sees no key" % what
    assert bool((out[none] == 0).all()), "%s: a row that sees no key must be zeros" % what
    assert bool((np.abs(lse[~none] - lse_j[~none]) <= lse_bound[~none]).all()), (what, lerr, lse_atol)
    share = float((np.abs(out - out_j) / (atol + out_rtol * np.abs(out_j) + 2.0 * e_p)).max()) if out.size else 0.0
    assert share <= 1.0, (what, err, atol, e_p, share)
    assert rms_k <= 2.0 * rms_p + atol, (what, rms_k, rms_p, atol)
    return err, lerr, share


def _run(torch, p, window=-1, max_sq=None, cu=None, cl=None, caches=None):
    import aule
    (q, kc, vc, bt, cl, cu), scales = p.device(torch, cu, cl)
    if caches is not None:
        kc, vc = (torch.from_numpy(x).cuda().view(torch.float8_e4m3fn) for x in caches)
    return aule.flash_attention_paged_prefill_fp8mma(q, kc, vc, bt, cl, cu, max_seqlen_q=p.max_sq if max_sq is None else max_sq,
                                                     window_size=window, return_lse=True, **scales)


@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%s-H%dkv%d-D%d-bs%d-w%d" % c)
def test_rows_and_lse_vs_the_models(case):
    """Test 1.  Measured on MI355X (max ratio, rms ratio against the P model), in SHAPES' order: DESIGN.md section 4."""
    import torch
    dtype, Hq, Hkv, D, bs, window = case
    p = _problem(dtype, Hq, Hkv, D, bs)
    out, lse = _run(torch, p, window)
    torch.cuda.synchronize()
    assert out.shape == (p.T, Hq, D) and out.dtype == torch_dtype(dtype) and lse.shape == (p.T, Hq) and lse.dtype == torch.float32
    _judge(p, out, lse, window, "fp8mma prefill")
    lse = lse.cpu().numpy()
    assert bool(np.isneginf(lse[0]).all())                          # L = 0
    assert bool(np.isneginf(lse[1:1 + 17]).all()) and bool(np.isfinite(lse[1 + 17:38]).all())    # positions -17 .. -1, then 0 .. 19


@pytest.mark.parametrize("dtype,Hq,Hkv,D,bs", [("fp16", 8, 2, 128, 16), ("bf16", 8, 2, 128, 24), ("bf16", 6, 2, 64, 16), ("fp16", 6, 2, 64, 24)])
def test_one_visible_key_gives_that_value_row_exactly(dtype, Hq, Hkv, D, bs):
    """Test 2.  window_size = 1: p = 2^8 and l = 2^8 exactly, so a row at position pos >= 0 is code(V[pos]) * v_scale[hk] -- formed in fp32
    as the kernel forms it (the one rounding before storage; the code has 4 significant bits, the scale 24) -- rounded to the dtype, bit for
    bit (the sign of a zero aside); a row at a negative position is zeros.  Pins the key and column order of the V image."""
    import torch
    p = _problem(dtype, Hq, Hkv, D, bs)
    out, lse = _run(torch, p, 1)
    torch.cuda.synchronize()
    g = Hq // Hkv
    vcode = torch.from_numpy(_decode(p.vdev).astype(np.float32))                # [blocks, bs, Hkv, D]
    vs = torch.tensor(p.vs, dtype=torch.float32).reshape(1, Hkv, 1)
    want = torch.zeros((p.T, Hq, D), dtype=torch_dtype(dtype))
    for b, s, n, L in p.sequences():
        for i in range(n):
            pos = L - n + i
            if pos >= 0:
                row = vcode[int(p.bt[b][pos // bs]), pos % bs] * vs[0]                 # [Hkv, D] fp32
                want[s + i] = row.repeat_interleave(g, dim=0).to(torch_dtype(dtype))
    own = torch.from_numpy(p.owned())
    got = out.cpu()
    # bit for bit, with the expected zeros normalised to +0: a code -0 gives -0 in `want` and +0 from an accumulator that starts at +0
    want = torch.where(want == 0, torch.zeros_like(want), want)
    assert torch.equal(got[own].view(torch.int16), want[own].view(torch.int16)), int((got[own].view(torch.int16) != want[own].view(torch.int16)).sum())
    assert int((want[own] != 0).sum()) > own.sum() * Hq * D // 2


@pytest.mark.parametrize("dtype,Hq,Hkv,D,bs", [("fp16", 6, 2, 64, 24), ("bf16", 8, 2, 128, 16)])
def test_a_sequence_alone_equals_the_sequence_in_the_batch(dtype, Hq, Hkv, D, bs):
    """Test 3.  Rows are quantised independently and a workgroup serves one sequence: out and lse bit for bit."""
    import torch
    import aule
    p = Ragged(65, dtype, "fp8", Hq, Hkv, D, bs, [1, 37, 130, 0, 50], [300, 20, 130, 50, 99])
    (q, kc, vc, bt, cl, cu), scales = p.device(torch)
    base, base_lse = aule.flash_attention_paged_prefill_fp8mma(q, kc, vc, bt, cl, cu, max_seqlen_q=130, return_lse=True, **scales)
    for b in (0, 1, 2, 4):
        s, e = int(p.cu[b]), int(p.cu[b + 1])
        one = torch.tensor([0, e - s], dtype=torch.int32, device="cuda")
        alone, alone_lse = aule.flash_attention_paged_prefill_fp8mma(q[s:e], kc, vc, bt[b:b + 1], cl[b:b + 1], one, return_lse=True, **scales)
        torch.cuda.synchronize()
        assert torch.equal(alone, base[s:e]) and torch.equal(alone_lse, base_lse[s:e]), b


@pytest.mark.parametrize("dtype,Hq,Hkv,D,bs", [("bf16", 6, 2, 64, 24), ("fp16", 8, 2, 128, 16)])
def test_nan_codes_where_nothing_may_be_read(dtype, Hq, Hkv, D, bs):
    """Test 4.  Code 0x7F (NaN) in every pool block no table names and in the rows of a sequence's last block past L: the results equal
    the run with zeros there, bit for bit."""
    import torch
    p = Ragged(66, dtype, "fp8", Hq, Hkv, D, bs, NS, LS, pool=80)
    addressed = np.zeros(p.kdev.shape[:2], dtype=bool)
    for b, _, _, L in p.sequences():
        j = np.arange(L)
        addressed[p.bt[b][j // bs], j % bs] = True
    assert (~addressed).sum() > 20 * bs
    runs = []
    for fill in (0x00, 0x7F):
        caches = []
        for dev in (p.kdev, p.vdev):
            x = dev.copy()
            x[~addressed] = fill
            caches.append(x)
        runs.append(_run(torch, p, caches=caches))
    torch.cuda.synchronize()
    own = torch.from_numpy(p.owned()).cuda()
    assert not bool(torch.isnan(runs[1][0][own]).any())
    assert torch.equal(runs[0][0][own].view(torch.int16), runs[1][0][own].view(torch.int16))
    assert torch.equal(runs[0][1][own].view(torch.int32), runs[1][1][own].view(torch.int32))


HOSTILE = [  # name, (dtype, Hq, Hkv, D, bs), ns, Ls, extra table columns, hostile context_lens, hostile cu_seqlens_q
    ("as-given", ("bf16", 6, 2, 64, 16), [40, 30, 20, 10], [100, 30, 64, 33], 2, None, None),
    ("context_lens", ("fp16", 8, 2, 128, 16), [40, 7, 3, 20], [96] * 4, 0, [96 + 1000, 2 ** 31 - 1, -5, INT32_MIN], None),
    ("cu-decreasing", ("bf16", 6, 2, 64, 16), [40, 30, 20, 10], [100, 30, 64, 33], 2, None, [0, 40, 70, 60, 50]),
    ("cu-beyond-T", ("bf16", 6, 2, 64, 16), [40, 30, 20, 10], [100, 30, 64, 33], 2, None, [0, 40, 70, 1000, 2 ** 31 - 1]),
    ("cu-negative", ("fp16", 8, 2, 128, 24), [40, 30, 20, 10], [100, 30, 64, 33], 2, None, [INT32_MIN, 40, 70, 70, -3]),
]


@pytest.mark.parametrize("case", HOSTILE, ids=lambda c: c[0])
def test_unowned_rows_and_hostile_lengths(case):
    """Test 5.  out / lse and the guard bands hold 0xFF (tests/hostile.py's arena), context_lens / cu_seqlens_q take the twin's hostile
    values: no byte outside the owned rows changes, no input is written, and the owned rows pass test 1's rules."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    name, (dtype, Hq, Hkv, D, bs), ns, Ls, extra, cl, cu = case
    p = Ragged(64, dtype, "fp8", Hq, Hkv, D, bs, ns, Ls, tail=3, extra_cols=extra)
    tdt, B, T = torch_dtype(dtype), p.B, p.T
    kw = {k: v for k, v in (("cl", cl), ("cu", cu)) if v is not None}
    cache_bytes = p.kdev.size
    regions = [("q", p.q.size * 2, "in"), ("k_cache", cache_bytes, "in"), ("v_cache", cache_bytes, "in"),
               ("block_tables", p.bt.size * 4, "in"), ("context_lens", B * 4, "in"), ("cu_seqlens_q", (B + 1) * 4, "in"),
               ("k_scale", Hkv * 4, "in"), ("v_scale", Hkv * 4, "in"), ("out", p.q.size * 2, "out"), ("lse", T * Hq * 4, "out")]
    ar = Arena(torch, regions, max(D * 2, Hkv * D))
    d = _capi.PagedPrefillDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype = hostile.DTYPE_CODE[dtype], 1
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, Hkv, D
    d.block_size, d.max_blocks = bs, p.bt.shape[1]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, p.max_sq, Hq * D
    d.scale, d.window_size, d.device = 0.0, -1, torch.cuda.current_device()
    d.stream = torch.cuda.current_stream().cuda_stream
    for n, _, _ in regions:
        setattr(d, n, ar.ptr(n))
    orig = {"q": ar.upload("q", torch.from_numpy(p.q).to(tdt)), "k_cache": ar.upload("k_cache", p.kdev), "v_cache": ar.upload("v_cache", p.vdev),
            "block_tables": ar.upload("block_tables", p.bt.astype(np.int32)),
            "context_lens": ar.upload("context_lens", np.asarray(p.cl if cl is None else cl, dtype=np.int32)),
            "cu_seqlens_q": ar.upload("cu_seqlens_q", np.asarray(p.cu if cu is None else cu, dtype=np.int32)),
            "k_scale": ar.upload("k_scale", p.ks.astype(np.float32)), "v_scale": ar.upload("v_scale", p.vs.astype(np.float32))}
    ar.fill(POISON)
    _capi.check(lib.aule_attention_paged_prefill_fp8mma_ex(ctypes.byref(d)), "paged prefill fp8mma")
    torch.cuda.synchronize()
    assert ar.guards_intact(), ar.damage()
    for n, o in orig.items():
        assert ar.unchanged(n, o), "input %s was written" % n
    out, lse = ar.view("out", tdt, (T, Hq, D)).clone(), ar.view("lse", torch.float32, (T, Hq)).clone()
    own = p.owned(**kw)
    free = torch.from_numpy(~own).cuda()
    assert bool((out[free].view(torch.uint8) == POISON).all()) and bool((lse[free].view(torch.uint8) == POISON).all()), "an unowned row was written"
    _judge(p, out, lse, -1, "hostile " + name, **kw)


def test_capture_replays_with_the_current_lengths():
    """Test 6.  Capture once, overwrite the lengths and offsets on the device, replay: the eager call on the new values bit for bit."""
    import torch
    import aule
    ns, Ls = [200, 5, 1, 94], [700, 37, 2047, 94]
    p = Ragged(69, "fp16", "fp8", 32, 8, 128, 16, ns, Ls, table_lens=[2048] * 4)
    (q, kc, vc, bt, cl, cu), scales = p.device(torch)
    fn = lambda: aule.flash_attention_paged_prefill_fp8mma(q, kc, vc, bt, cl, cu, max_seqlen_q=256, return_lse=True, **scales)   # noqa: E731
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
    cu.copy_(torch.tensor([0, 17, 17, 273, 300], device="cuda", dtype=torch.int32))
    cl.copy_(torch.tensor([17, 900, 2048, 10], device="cuda", dtype=torch.int32))
    want, want_lse = fn()
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(want, eager)
    assert torch.equal(out, want) and torch.equal(lse, want_lse)


def test_c_entry_on_the_device():
    """Test 7.  The descriptor path gives the wrapper's bits; what the entry refuses on a live device leaves out untouched."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    p = Ragged(70, "bf16", "fp8", 8, 2, 64, 16, [9, 3, 70], [40, 3, 200])
    args, scales = p.device(torch)
    want, want_lse = _run(torch, p, 16)
    out = torch.full((p.T, 8, 64), -1, device="cuda", dtype=torch.int16).view(torch.bfloat16)
    lse = torch.full((p.T, 8), -1, device="cuda", dtype=torch.int32).view(torch.float32)
    d = _desc(torch, p, args, scales, out, lse, p.max_sq, 16)
    assert lib.aule_attention_paged_prefill_fp8mma_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16)) and torch.equal(lse.view(torch.int32), want_lse.view(torch.int32))

    kc16 = torch.zeros(args[1].shape, device="cuda", dtype=torch.bfloat16)

    def refused(change, needle):
        out.view(torch.int16).fill_(-1)
        d = _desc(torch, p, args, scales, out, None, p.max_sq)
        change(d)
        assert lib.aule_attention_paged_prefill_fp8mma_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg
        torch.cuda.synchronize()
        assert bool((out.view(torch.int16) == -1).all()), needle

    def to_16_bit(d):
        d.cache_dtype, d.k_scale, d.v_scale = 0, None, None
        d.k_cache = d.v_cache = kc16.data_ptr()

    refused(to_16_bit, "cache_dtype must be AULE_KV_CACHE_FP8_E4M3")
    refused(lambda d: (setattr(d, "head_dim", 32), setattr(d, "q_token_stride", 8 * 32)), "head_dim 32")
    refused(lambda d: setattr(d, "k_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "v_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "struct_size", 144), "struct_size")
    refused(lambda d: setattr(d, "cu_seqlens_q", None), "null tensor pointer")
    d = _desc(torch, p, args, scales, out, None, p.max_sq)
    d.total_tokens = 0
    assert lib.aule_attention_paged_prefill_fp8mma_ex(ctypes.byref(d)) == 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == -1).all())
