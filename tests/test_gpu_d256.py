"""GPU parity of head_dim 256 (fa_fwd_d256_gfx950.hip, fa_bwd_d256_gfx950.hip) and of the head sizes padded to it (160, 192).

Judges: the fp64 oracle (fwd_f64 / bwd_f64 on small shapes, fwd_rows_f64 / bwd_head_f64 at full size).  Bounds: the existing ones
of tests/util.py -- assert_close_rows / fwd_tol and LSE_TOL for the forward, BWD_TOL for the gradients (as test_gpu_bwd.py).
Random shapes at the kernels' tile seams, hard data and the other padded sizes: the d256 and pad kinds of tools/fuzz_parity.py
(tests/test_gpu_fuzz.py).
"""
import ctypes
import math

import numpy as np
import pytest

from util import BWD_TOL, LSE_TOL, assert_close, assert_close_rows, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

ROUTE_D256 = 9          # aule_hip_debug_forward_route
BWD_BIT_D256 = 128      # aule_hip_debug_last_backward_route


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def oracle_mod():
    import oracle
    return oracle


def _lib():
    from aule import _capi
    lib = _capi.load()
    lib.aule_hip_debug_forward_route.restype = ctypes.c_int32
    lib.aule_hip_debug_forward_route.argtypes = [ctypes.POINTER(_capi.AttnDesc)]
    lib.aule_hip_debug_last_backward_route.restype = ctypes.c_int32
    return lib


def _fwd_route(dtype, B, Hq, Hkv, Sq, Sk, causal, window, scale):
    from aule import _capi
    from aule import _torch as at
    d = _capi.AttnDesc()
    d.struct_size = ctypes.sizeof(_capi.AttnDesc)
    d.dtype = {"fp32": 0, "fp16": 1, "bf16": 2}[dtype]
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, Sq, Sk, 256
    d.causal, d.window_size = at.causal_code(causal), window
    d.scale = 0.0 if scale is None else scale
    return _lib().aule_hip_debug_forward_route(ctypes.byref(d))


def _inputs(seed, B, Hq, Hkv, Sq, Sk, D, dtype):
    rng = np.random.RandomState(seed)
    q = quantize(rng.randn(B, Hq, Sq, D).astype(np.float32), dtype)
    k = quantize(rng.randn(B, Hkv, Sk, D).astype(np.float32), dtype)
    v = quantize(rng.randn(B, Hkv, Sk, D).astype(np.float32), dtype)
    do = quantize(rng.randn(B, Hq, Sq, D).astype(np.float32), dtype)
    return q, k, v, do


def _nkeys(Sq, Sk, causal, window):
    """keys each query row sees (the oracle's mask)"""
    from aule import _torch as at
    code = at.causal_code(causal)
    coff = Sk - Sq if code == 2 else 0
    pos = np.arange(Sq) + coff
    hi = np.minimum(Sk, pos + 1) if code else np.full(Sq, Sk)
    lo = np.maximum(0, pos - window + 1) if window > 0 else np.zeros(Sq, dtype=np.int64)
    return np.maximum(0, hi - lo)


def _dev(torch, a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(dtype))


# dtype, B, Hq, Hkv, Sq, Sk, causal, window, scale
FWD_CASES = [
    ("bf16", 1, 4, 4, 257, 257, False, -1, None),
    ("bf16", 1, 4, 1, 65, 1025, True, -1, None),                 # MQA, top-left causal, Sk > Sq
    ("fp16", 1, 4, 2, 1000, 1025, "bottom-right", -1, -0.2),      # negative scale
    ("bf16", 1, 32, 8, 65, 5000, "bottom-right", -1, 0.0),        # scale 0 at this layer: uniform weights
    ("bf16", 1, 2, 2, 1, 1, False, -1, None),
    ("fp16", 2, 8, 2, 1, 5000, False, -1, None),                  # decode rows, GQA
    ("fp16", 1, 4, 4, 257, 257, True, 7, None),
    ("bf16", 1, 4, 2, 1000, 1025, True, 100, None),
    ("bf16", 1, 4, 2, 257, 1025, False, 256, None),
    ("fp16", 1, 2, 2, 1000, 1000, False, 1000, 0.0),
    ("bf16", 1, 4, 4, 1000, 63, False, 7, None),                  # rows past key 69 see nothing: O = 0, LSE = -inf
    ("bf16", 1, 32, 8, 257, 1025, True, -1, -0.2),
    ("fp16", 1, 8, 1, 65, 63, False, -1, None),
    ("bf16", 2, 4, 4, 1000, 1000, True, 256, None),
    ("fp16", 1, 4, 4, 65, 5000, "bottom-right", 1000, None),
    ("bf16", 1, 2, 2, 1000, 5000, False, -1, None),
    ("fp32", 1, 2, 2, 257, 257, True, -1, None),
    ("fp32", 1, 4, 1, 65, 1025, "bottom-right", 100, -0.2),
    ("fp32", 1, 2, 2, 1, 63, False, -1, 0.0),                     # scale 0: uniform weights
    ("fp32", 1, 2, 2, 1000, 1025, True, 7, None),
]


def _fwd(torch, case, seed=0):
    from aule import _torch as at
    dtype, B, Hq, Hkv, Sq, Sk, causal, W, scale = case
    q, k, v, _ = _inputs(seed, B, Hq, Hkv, Sq, Sk, 256, dtype)
    sc = 1.0 / 16.0 if scale is None else scale
    out, lse = at.fwd_raw(_dev(torch, q, dtype), _dev(torch, k, dtype), _dev(torch, v, dtype), at.causal_code(causal), sc,
                          want_lse=True, window=W)
    torch.cuda.synchronize()
    return (q, k, v), out.float().cpu().numpy(), lse.cpu().numpy()


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_forward_and_lse(torch_cuda, oracle_mod, case):
    dtype, B, Hq, Hkv, Sq, Sk, causal, W, scale = case
    (q, k, v), out, lse = _fwd(torch_cuda, case)
    ref, ref_lse = oracle_mod.fwd_f64(q, k, v, causal, scale, W)
    nk = np.tile(_nkeys(Sq, Sk, causal, W), B * Hq)
    # (the bound of the window and negative-scale tests: one rounding of P to the storage dtype per visible key)
    atol, rtol = fwd_tol(dtype, np.abs(v).max())
    assert_close(out, ref, atol, rtol, "O")
    empty = nk == 0
    got_l, ref_l = lse.reshape(-1), ref_lse.reshape(-1)
    assert np.isneginf(ref_l[empty]).all() and np.isneginf(got_l[empty]).all()
    assert_close(got_l[~empty], ref_l[~empty], LSE_TOL[dtype], LSE_TOL[dtype], "LSE")
    if dtype != "fp32":
        assert _fwd_route(dtype, B, Hq, Hkv, Sq, Sk, causal, W, scale) == ROUTE_D256


_PREFIX = {}


def _prefix_problem(torch, dtype):
    """B1 H2 kv1 Sq = Sk = 300, top-left causal: the inputs on the device and the long call's (out, lse), computed once per dtype"""
    from aule import _torch as at
    if dtype not in _PREFIX:
        q, k, v, _ = _inputs(8, 1, 2, 1, 300, 300, 256, dtype)
        t = tuple(_dev(torch, x, dtype) for x in (q, k, v))
        out, lse = at.fwd_raw(*t, 1, 1.0 / 16.0, want_lse=True)
        torch.cuda.synchronize()
        _PREFIX[dtype] = (t, out, lse)
    return _PREFIX[dtype]


@pytest.mark.parametrize("n", [65, 128, 129])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_top_left_causal_prefix_is_the_short_call_bit_for_bit(torch_cuda, dtype, n):
    """Under the top-left rule rows 0 .. n - 1 see keys 0 .. n - 1 only, so the first n rows of the 300 x 300 call are the call on the first
    n rows and keys.  The long call walks more key tiles for those rows' query block (kend follows the block's last row: fa_fwd_d256_gfx950.hip),
    every one of them fully masked for these rows: a masked tile leaves m, l and O as they are (alpha = exp2(0) = 1, every weight
    exp2(-inf) = 0), so the bits agree -- n = 65: the ragged second key tile; 128: a whole query block; 129: one row of the second block,
    whose long call runs four key tiles against three."""
    from aule import _torch as at
    torch = torch_cuda
    (tq, tk, tv), out, lse = _prefix_problem(torch, dtype)
    o, l = at.fwd_raw(tq[:, :, :n].contiguous(), tk[:, :, :n].contiguous(), tv[:, :, :n].contiguous(), 1, 1.0 / 16.0, want_lse=True)
    torch.cuda.synchronize()
    view = torch.int32 if dtype == "fp32" else torch.int16
    assert torch.equal(o.view(view), out[:, :, :n].contiguous().view(view))
    assert torch.equal(l.view(torch.int32), lse[:, :, :n].contiguous().view(torch.int32))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_online_softmax_rescale_is_exercised_at_d256(torch_cuda, oracle_mod, dtype):
    """The twin of test_gpu_fwd.py::test_online_softmax_rescale_is_exercised: a key in the LAST 64-key tile of row 295 (key 290 of 300)
    whose logit (24 in natural units) towers over the row's, so that the running maximum jumps after O and l were accumulated, and a key
    with a large negative logit; causal and not.  On the reference alone the spike moves row 295 by more than 20 x the tolerance."""
    from aule import _torch as at
    rng = np.random.RandomState(5)
    q = rng.randn(1, 2, 300, 256).astype(np.float32) * 0.5
    k = rng.randn(1, 2, 300, 256).astype(np.float32) * 0.5
    v = rng.randn(1, 2, 300, 256).astype(np.float32)
    plain = quantize(k.copy(), dtype)      # (a copy: for fp32 the round trip hands the same memory back)
    k[:, :, 290, :] = 6.0 * q[:, :, 295, :]
    k[:, :, 100, :] = -4.0 * q[:, :, 120, :]
    q, k, v = (quantize(x, dtype) for x in (q, k, v))
    atol, rtol = fwd_tol(dtype, np.abs(v).max())
    for causal in (True, False):
        case = (dtype, 1, 2, 2, 300, 300, causal, -1, None)
        out, lse = at.fwd_raw(*(_dev(torch_cuda, x, dtype) for x in (q, k, v)), at.causal_code(causal), 1.0 / 16.0, want_lse=True)
        torch_cuda.cuda.synchronize()
        ref, ref_lse = oracle_mod.fwd_f64(q, k, v, causal, None)
        without, _ = oracle_mod.fwd_f64(q, plain, v, causal, None)
        assert (np.abs(without[:, :, 295] - ref[:, :, 295]) > 20 * (atol + rtol * np.abs(ref[:, :, 295]))).any()
        assert_close(out.float().cpu().numpy(), ref, atol, rtol, "spike %s causal=%s" % (dtype, causal))
        assert_close(lse.cpu().numpy(), ref_lse, LSE_TOL[dtype] * 4, 1e-5, "spike lse")
        if dtype != "fp32":
            assert _fwd_route(*case) == ROUTE_D256


def _check_grad(got, ref, dtype, what):
    atol, rtol = BWD_TOL[dtype]
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    print("%s: max|err| %.3e = %.2e of max|grad| %.3g" % (what, err.max(), err.max() / scale, scale))
    bad = err > atol * scale + rtol * np.abs(ref)
    assert not bad.any(), "%s: %d elements out of bound, max err %.3e" % (what, int(bad.sum()), err.max())


BWD_CASES = [
    ("bf16", 1, 4, 4, 257, 257, False, -1, None),
    ("bf16", 1, 4, 1, 65, 1025, True, -1, None),
    ("fp16", 1, 4, 2, 1000, 1025, "bottom-right", -1, -0.2),
    ("bf16", 1, 2, 2, 1, 1, False, -1, None),
    ("fp16", 1, 4, 4, 257, 257, True, 7, None),
    ("bf16", 1, 4, 2, 1000, 1025, True, 100, None),
    ("bf16", 1, 4, 2, 257, 1025, False, 256, None),
    ("bf16", 1, 4, 4, 1000, 63, False, 7, None),
    ("fp16", 1, 8, 1, 65, 63, False, -1, None),
    ("fp16", 1, 4, 4, 65, 1000, "bottom-right", 100, 0.0),
    ("fp32", 1, 2, 2, 257, 257, True, -1, None),
    ("fp32", 1, 4, 1, 65, 1025, "bottom-right", 100, -0.2),
]


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_backward(torch_cuda, oracle_mod, case):
    from aule import _torch as at
    torch = torch_cuda
    dtype, B, Hq, Hkv, Sq, Sk, causal, W, scale = case
    q, k, v, do = _inputs(1, B, Hq, Hkv, Sq, Sk, 256, dtype)
    sc = 1.0 / 16.0 if scale is None else scale
    code = at.causal_code(causal)
    tq, tk, tv, tdo = (_dev(torch, x, dtype) for x in (q, k, v, do))
    out, lse = at.fwd_raw(tq, tk, tv, code, sc, want_lse=True, window=W)
    dq, dk, dv = at.bwd_raw(tq, tk, tv, out, tdo, lse, code, sc, window=W)
    torch.cuda.synchronize()
    assert _lib().aule_hip_debug_last_backward_route() & BWD_BIT_D256
    rq, rk, rv = oracle_mod.bwd_f64(q, k, v, do, causal, sc, W)
    for name, g, r in (("dQ", dq, rq), ("dK", dk, rk), ("dV", dv, rv)):
        _check_grad(g.float().cpu().numpy(), r, dtype, name)


@pytest.mark.parametrize("D,dtype,causal", [(160, "fp16", False), (192, "bf16", True)])
def test_padded_head_sizes_with_autograd(torch_cuda, oracle_mod, D, dtype, causal):
    import aule
    torch = torch_cuda
    B, Hq, Hkv, Sq, Sk = 1, 4, 2, 300, 333
    q, k, v, do = _inputs(2, B, Hq, Hkv, Sq, Sk, D, dtype)
    tq, tk, tv = (_dev(torch, x, dtype).requires_grad_(True) for x in (q, k, v))
    out = aule.flash_attention(tq, tk, tv, causal=causal)
    assert out.shape == (B, Hq, Sq, D)
    out.backward(_dev(torch, do, dtype))
    torch.cuda.synchronize()
    assert _lib().aule_hip_debug_last_backward_route() & BWD_BIT_D256
    ref, _ = oracle_mod.fwd_f64(q, k, v, causal)
    atol, rtol = fwd_tol(dtype, np.abs(v).max())
    assert_close(out.detach().float().cpu().numpy(), ref, atol, rtol, "O")
    rq, rk, rv = oracle_mod.bwd_f64(q, k, v, do, causal)
    for name, g, r in (("dQ", tq.grad, rq), ("dK", tk.grad, rk), ("dV", tv.grad, rv)):
        assert g.shape == r.shape
        _check_grad(g.float().cpu().numpy(), r, dtype, name)


def test_full_size_causal_bf16(torch_cuda, oracle_mod):
    """B4 H16 S4096 D256 bf16 causal: the FLOPs of the C2 headline (B4 H32 S4096 D128)."""
    import aule
    torch = torch_cuda
    B, H, S, D = 4, 16, 4096, 256
    g = torch.Generator(device="cuda").manual_seed(3)
    tq, tk, tv, tdo = (torch.randn(B, H, S, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4))
    for t in (tq, tk, tv):
        t.requires_grad_(True)
    out = aule.flash_attention(tq, tk, tv, causal=True)
    out.backward(tdo)
    torch.cuda.synchronize()
    q, k, v, do = (t.detach().float().cpu().numpy() for t in (tq, tk, tv, tdo))
    rng = np.random.RandomState(4)
    rows = np.sort(rng.choice(B * H * S, 256, replace=False)).astype(np.int64)
    ref, ref_lse = oracle_mod.fwd_rows_f64(q, k, v, rows, True)
    got = out.detach().float().cpu().numpy().reshape(-1, D)[rows]
    assert_close_rows(got, ref, (rows % S) + 1, "bf16", np.abs(v).max(), "O rows")
    for head in ((0, 5), (3, 15)):
        b, h = head
        rq, rk, rv = oracle_mod.bwd_head_f64(q, k, v, do, head=head, causal=True)
        _check_grad(tq.grad[b, h:h + 1].float().cpu().numpy(), rq, "bf16", "dQ %s" % (head,))
        _check_grad(tk.grad[b, h].float().cpu().numpy(), rk, "bf16", "dK %s" % (head,))
        _check_grad(tv.grad[b, h].float().cpu().numpy(), rv, "bf16", "dV %s" % (head,))


def test_sdpa_shim_runs_the_hip_path(torch_cuda, oracle_mod, monkeypatch):
    import aule
    torch = torch_cuda

    def refuse(*a, **kw):
        raise AssertionError("the SDPA shim fell back to PyTorch at head_dim 256")

    monkeypatch.setattr(aule, "_original_sdpa", refuse)
    q, k, v, _ = _inputs(5, 1, 8, 2, 200, 200, 256, "bf16")
    out = aule.scaled_dot_product_attention(_dev(torch, q, "bf16"), _dev(torch, k, "bf16"), _dev(torch, v, "bf16"),
                                            is_causal=True, enable_gqa=True)
    torch.cuda.synchronize()
    ref, _ = oracle_mod.fwd_f64(q, k, v, True)
    atol, rtol = fwd_tol("bf16", np.abs(v).max())
    assert_close(out.float().cpu().numpy(), ref, atol, rtol, "SDPA shim")


def test_numpy_input(torch_cuda, oracle_mod):
    import aule
    q, k, v, _ = _inputs(6, 1, 2, 2, 130, 130, 256, "fp32")
    out = aule.flash_attention(q, k, v, causal=True)
    assert isinstance(out, np.ndarray) and out.shape == q.shape
    ref, _ = oracle_mod.fwd_f64(q, k, v, True)
    assert_close(out, ref, 1e-5, 1e-5, "NumPy D=256")


def test_graph_capture_replays_eager(torch_cuda):
    import aule
    torch = torch_cuda
    q, k, v, _ = _inputs(7, 1, 8, 2, 300, 700, 256, "bf16")
    tq, tk, tv = (_dev(torch, x, "bf16") for x in (q, k, v))
    with torch.no_grad():
        eager = aule.flash_attention(tq, tk, tv, causal=True).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            aule.flash_attention(tq, tk, tv, causal=True)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = aule.flash_attention(tq, tk, tv, causal=True)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_ex_validation_refuses_other_sizes(torch_cuda):
    from aule import _torch as at
    from aule._capi import AuleError
    torch = torch_cuda
    for D in (129, 192, 257):
        x = torch.zeros(1, 1, 8, D, device="cuda", dtype=torch.bfloat16)
        with pytest.raises(AuleError, match="pad to the next size"):
            at.fwd_raw(x, x, x, 0, 0.1, want_lse=False)
