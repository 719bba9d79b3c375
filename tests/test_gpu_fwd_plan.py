"""The forward's launch plan and its launch are the same thing: for one small shape per route, what aule_attention_forward_ex ran
(aule_hip_debug_last_forward_route, stored by the launcher from the plan it executes) is what aule_hip_debug_forward_route answers
for the same descriptor without a device (csrc/fa_fwd_plan.h), it is the route the case is named for, and the result is right.
Also: the plan's workspace size is what the launch uses (a caller buffer one byte short is not taken; one of exactly the size is)."""
import ctypes
import os

import numpy as np
import pytest

from util import LSE_TOL, assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

# (route, dtype, B, Hq, Hkv, Sq, Sk, D, causal)
ROUTE_CASES = [
    (0, "fp32", 1, 2, 2, 64, 64, 32, 0),
    (1, "bf16", 1, 2, 2, 128, 128, 32, 1),
    (4, "bf16", 32, 1, 1, 1, 8192, 128, 0),        # 134 MB of K+V: the streaming corner of the wave-per-chunk kernel
    (5, "fp16", 1, 8, 2, 16, 2048, 64, 0),
    (7, "bf16", 1, 8, 8, 4096, 4096, 128, 1),
    (8, "fp16", 1, 4, 4, 512, 512, 64, 1),
    (9, "bf16", 1, 2, 2, 128, 128, 256, 0),
    (0, "fp32", 1, 2, 2, 128, 128, 256, 0),        # fp32 at head_dim 256: route 0 by the plan's statement, run by the head_dim 256 file
]
DTYPE_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}


@pytest.fixture(scope="module")
def env():
    import torch
    from aule import _capi
    for var in os.environ:   # (the default dispatch; the switches are read once per process)
        assert not var.startswith(("AULE_HIP_FWD_", "AULE_HIP_W4_")) and var != "AULE_HIP_F32_SPLIT", var
    return torch, _capi, _capi.get_lib()


def _desc(torch, _capi, q, k, v, out, lse, dtype, causal):
    B, Hq, Sq, D = q.shape
    d = _capi.AttnDesc()
    d.struct_size = ctypes.sizeof(_capi.AttnDesc)
    d.dtype = DTYPE_CODE[dtype]
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, k.shape[1], Sq, k.shape[2], D
    d.scale, d.causal, d.window_size, d.device = D ** -0.5, causal, -1, torch.cuda.current_device()
    d.stream = torch.cuda.current_stream().cuda_stream
    d.q, d.k, d.v, d.out, d.lse = (t.data_ptr() for t in (q, k, v, out, lse))
    return d


def _problem(torch, case):
    route, dtype, B, Hq, Hkv, Sq, Sk, D, causal = case
    rng = np.random.RandomState(1000 + route + D)
    qn, kn, vn = (quantize(rng.randn(*s).astype(np.float32), dtype) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D)))
    q, k, v = (torch.from_numpy(x).to("cuda", torch_dtype(dtype)) for x in (qn, kn, vn))
    return qn, kn, vn, q, k, v, torch.empty_like(q), torch.empty((B, Hq, Sq), device="cuda", dtype=torch.float32)


@pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: "route%d-%s-D%d" % (c[0], c[1], c[7]))
def test_the_launch_runs_what_the_plan_says(case, env, oracle_mod):
    torch, _capi, lib = env
    route, dtype, B, Hq, Hkv, Sq, Sk, D, causal = case
    qn, kn, vn, q, k, v, out, lse = _problem(torch, case)
    d = _desc(torch, _capi, q, k, v, out, lse, dtype, causal)
    planned = int(lib.aule_hip_debug_forward_route(ctypes.byref(d)))
    buf = (ctypes.c_int32 * 16)()
    assert lib.aule_hip_debug_forward_plan(ctypes.byref(d), buf, 16) >= 3 and buf[0] == planned
    assert (buf[1] & 0xFFFFFFFF) | (buf[2] << 32) == lib.aule_attention_forward_workspace_size(ctypes.byref(d))
    _capi.check(lib.aule_attention_forward_ex(ctypes.byref(d)), "aule_attention_forward_ex")
    torch.cuda.synchronize()
    ran = int(lib.aule_hip_debug_last_forward_route())
    print(case, "planned", planned, "ran", ran, "plan", list(buf[:12]))
    assert ran == planned == route, (case, planned, ran)
    ref, ref_lse = oracle_mod.fwd_f64(qn, kn, vn, bool(causal), None)
    atol, rtol = fwd_tol(dtype, np.abs(vn).max())
    assert_close(out.float().cpu().numpy(), ref, atol, rtol, "out")
    assert_close(lse.cpu().numpy(), ref_lse, LSE_TOL[dtype], 1e-5, "lse")


def test_fused_rotation_runs_route_8(env, oracle_mod):
    torch, _capi, lib = env
    from aule import _torch as at
    case = (8, "fp16", 1, 4, 4, 512, 512, 64, 1)
    qn, kn, vn, q, k, v, _, _ = _problem(torch, case)
    cos, sin = oracle_mod.rope_tables(512, 64)
    tc, ts = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in (cos, sin))
    kr = at.rope_raw(k, tc, ts, "half", False, 0)
    fused, lse = at.fwd_raw(q, kr, v, 1, 64 ** -0.5, want_lse=True, q_rope=(tc, ts, 0))
    torch.cuda.synchronize()
    assert lib.aule_hip_debug_last_forward_route() == 8
    two_pass, _ = at.fwd_raw(at.rope_raw(q, tc, ts, "half", False, 0), kr, v, 1, 64 ** -0.5, want_lse=True)
    assert torch.equal(fused, two_pass)
    qo, ko = (quantize(oracle_mod.rope_f64(x, cos, sin, "half"), "fp16") for x in (qn, kn))
    ref, ref_lse = oracle_mod.fwd_f64(qo, ko, vn, True, None)
    atol, rtol = fwd_tol("fp16", np.abs(vn).max())
    assert_close(fused.float().cpu().numpy(), ref, atol, rtol, "out")
    assert_close(lse.cpu().numpy(), ref_lse, LSE_TOL["fp16"], 1e-5, "lse")


def test_a_workspace_one_byte_short_is_not_taken(env):
    """Route 5 with a caller buffer of ws_bytes - 1: the launch allocates stream-ordered instead, leaves the buffer alone, and the
    result equals the one computed in a buffer of exactly ws_bytes (which is written, and nothing behind it)."""
    torch, _capi, lib = env
    case = (5, "fp16", 1, 8, 2, 16, 2048, 64, 0)
    _, _, _, q, k, v, _, _ = _problem(torch, case)
    res = []
    for short in (0, 1):
        out, lse = torch.empty_like(q), torch.empty((1, 8, 16), device="cuda", dtype=torch.float32)
        d = _desc(torch, _capi, q, k, v, out, lse, "fp16", 0)
        need = int(lib.aule_attention_forward_workspace_size(ctypes.byref(d)))
        assert need > 0
        ws = torch.full((need + 4096,), 0x5A, device="cuda", dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), need - short
        _capi.check(lib.aule_attention_forward_ex(ctypes.byref(d)), "aule_attention_forward_ex")
        torch.cuda.synchronize()
        assert lib.aule_hip_debug_last_forward_route() == 5
        assert bool((ws[need:] == 0x5A).all()), "wrote past the workspace it was given"
        assert bool((ws[:need] == 0x5A).all()) == bool(short), "the caller's buffer: used when it is large enough, untouched when not"
        res.append((out, lse))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_paged_decode_in_a_workspace_of_the_queried_size(fp8, env):
    """B2 Hq4 Hkv1 D64 block 16: the output is bitwise the same with a caller workspace of exactly the queried size and with none."""
    torch, _capi, lib = env
    B, Hq, Hkv, D, bs, max_blocks = 2, 4, 1, 64, 16, 24
    gen = torch.Generator(device="cuda").manual_seed(11)
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16, generator=gen)
    if fp8:   # e4m3fn codes without the NaN patterns (0x7f, 0xff)
        kc, vc = ((torch.randint(0, 0x78, (B * max_blocks, bs, Hkv, D), device="cuda", generator=gen)
                   + 128 * torch.randint(0, 2, (B * max_blocks, bs, Hkv, D), device="cuda", generator=gen)).to(torch.uint8) for _ in range(2))
    else:
        kc, vc = (torch.randn(B * max_blocks, bs, Hkv, D, device="cuda", dtype=torch.bfloat16, generator=gen) for _ in range(2))
    bt = torch.randperm(B * max_blocks, device="cuda", generator=gen).to(torch.int32).reshape(B, max_blocks).contiguous()
    cl = torch.tensor([max_blocks * bs - 5, 33], device="cuda", dtype=torch.int32)
    ks, vs = torch.tensor([0.7], device="cuda"), torch.tensor([1.6], device="cuda")
    res = []
    for mine in (True, False):
        out = torch.empty_like(q)
        d = _capi.PagedFp8Desc() if fp8 else _capi.PagedDesc()
        d.struct_size = ctypes.sizeof(d)
        d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim, d.block_size, d.max_blocks = 2, B, Hq, Hkv, D, bs, max_blocks
        d.scale, d.window_size, d.device = 0.0, -1, torch.cuda.current_device()
        d.stream = torch.cuda.current_stream().cuda_stream
        d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
        d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
        if fp8:
            d.k_scale, d.v_scale = ks.data_ptr(), vs.data_ptr()
        size = lib.aule_attention_paged_decode_fp8_workspace_size if fp8 else lib.aule_attention_paged_decode_workspace_size
        need = int(size(ctypes.byref(d)))
        assert need > 0
        ws = torch.full((need + 4096,), 0x5A, device="cuda", dtype=torch.uint8)
        if mine:
            d.workspace, d.workspace_bytes = ws.data_ptr(), need
        run = lib.aule_attention_paged_decode_fp8_ex if fp8 else lib.aule_attention_paged_decode_ex
        _capi.check(run(ctypes.byref(d)), "paged decode")
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0x5A).all()), "wrote past the workspace it was given"
        assert bool((ws[:need] == 0x5A).all()) == (not mine)
        assert bool(torch.isfinite(out.float()).all())
        res.append(out)
    assert torch.equal(res[0], res[1])
