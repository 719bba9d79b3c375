"""GPU tests of the legacy C-ABI through ctypes (run with -m gpu): the call sequences
of the reference's ctypes consumers (python/aule/vulkan.py, tests/test_paged_python.py:
31-118, tests/benchmark_mi300x.py:75-153) with numerics checked against the oracle."""
import ctypes

import numpy as np
import pytest

from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    from aule.hip import Aule
    a = Aule()
    yield a
    a.close()


def test_init_idempotent_and_info(A):
    lib = A._lib
    assert lib.aule_init() == 0 and lib.aule_init() == 0          # src/lib.zig:60-63
    assert lib.aule_get_backend_name() == b"HIP/ROCm"
    assert lib.aule_get_vendor() == 1 and lib.aule_get_gpu_vendor() == 1
    assert lib.aule_is_amd_optimized() == 1 and lib.aule_has_fp16() == 1
    assert lib.aule_get_subgroup_size() == 64 and lib.aule_supports_backward() == 1
    assert lib.aule_set_shader_variant(0) == 0 and lib.aule_get_shader_variant() == 0
    assert lib.aule_has_shader_variant(0) == 1 and lib.aule_has_shader_variant(2) == 0
    assert lib.aule_set_shader_variant(3) == -2
    assert len(A.device_name) > 0
    buf = ctypes.create_string_buffer(4)
    assert lib.aule_get_device_name(buf, 4) == 3 and len(buf.value) == 3   # truncated to len-1


def test_handle_lifecycle_and_errors(A):
    lib = A._lib
    lib.aule_tensor_clear_all()
    assert lib.aule_tensor_count() == 0 and lib.aule_tensor_max() == 1024
    h = lib.aule_tensor_create(1, 2, 3, 4)
    assert h == 1 and lib.aule_tensor_size(h) == 24 and lib.aule_tensor_count() == 1
    data = np.arange(24, dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.aule_tensor_upload(h, data.ctypes.data_as(fp), 24) == 0
    assert lib.aule_tensor_upload(h, data.ctypes.data_as(fp), 23) == -3      # size mismatch
    assert b"size mismatch" in lib.aule_get_error()
    back = np.zeros(24, np.float32)
    assert lib.aule_tensor_download(h, back.ctypes.data_as(fp), 24) == 0
    assert np.array_equal(back, data)                                          # padded pitch is invisible
    u = np.zeros(24, np.uint32)
    assert lib.aule_tensor_download_u32(h, u.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 24) == 0
    assert np.array_equal(u.view(np.float32), data)
    assert lib.aule_tensor_upload(0, data.ctypes.data_as(fp), 24) == -1
    assert lib.aule_tensor_upload(7, data.ctypes.data_as(fp), 24) == -1
    h2 = lib.aule_tensor_create_u32(1, 1, 1, 8)
    assert h2 == 2
    lib.aule_tensor_destroy(h)
    assert lib.aule_tensor_size(h) == 0 and lib.aule_tensor_count() == 1
    assert lib.aule_tensor_create(1, 1, 1, 1) == 1                             # first free slot is reused
    lib.aule_tensor_clear_all()
    # 1024-slot limit (src/lib.zig:17)
    hs = [lib.aule_tensor_create(1, 1, 1, 1) for _ in range(1024)]
    assert hs[-1] == 1024 and lib.aule_tensor_create(1, 1, 1, 1) == 0
    assert lib.aule_get_error() == b"Max tensors reached"
    lib.aule_tensor_clear_all()
    assert lib.aule_tensor_count() == 0


def test_out_of_scope_stubs_return_minus3(A):
    lib = A._lib
    h = lib.aule_tensor_create(1, 1, 4, 32)
    assert lib.aule_attention_forward_paged(h, h, h, h, 0, 0, 0, -1) == -3
    assert lib.aule_spatial_sort(h, h, h, 0) == -3
    assert lib.aule_attention_forward_gravity(h, h, h, h, 0, 0, h, 0, 4, -1) == -3
    assert lib.aule_attention_forward_gpu(h, h, h, h, h, h, 0, -1) == -3        # RoPE handles
    assert lib.aule_attention_forward_gpu(h, h, h, h, 0, 0, 0, 8) == 0          # sliding window is supported
    assert lib.aule_attention_forward_gpu(h, h, h, 99, 0, 0, 0, -1) == -1       # bad handle
    lib.aule_tensor_destroy(h)


@pytest.mark.parametrize("shape", [(1, 1, 16, 16), (1, 1, 32, 32), (1, 1, 64, 64), (1, 2, 32, 32),
                                   (1, 4, 64, 32), (1, 8, 64, 64), (2, 8, 64, 64)])
def test_zig_test_shapes_forward_vs_ref(A, oracle_mod, shape):
    """tests/test_attention.zig:18-31 shapes, inputs (u*2-1)*0.5, rule max_abs<1e-4 or max_rel<1e-3;
    we hold 1e-5 against the fp64 judge and 1e-4 against the zig-order fp32 restatement."""
    rng = np.random.RandomState(42)
    q, k, v = (((rng.rand(*shape) * 2 - 1) * 0.5).astype(np.float32) for _ in range(3))
    out = A.forward_host(q, k, v, causal=False)
    assert_close(out, oracle_mod.fwd_f64(q, k, v, False)[0], 1e-5, 1e-5, "host fwd")
    assert np.abs(out - oracle_mod.ref_forward(q, k, v, False)).max() < 1e-4
    out_c = A.forward_host(q, k, v, causal=True)
    assert np.abs(out_c - oracle_mod.ref_forward(q, k, v, True)).max() < 1e-4


def test_known_answer_cases_on_gpu(A):
    # KAT-1 (attention_ref.zig:250-298), D=4 exercises the padded-pitch path
    q = np.full((1, 1, 2, 4), 0.5, np.float32)
    v = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32).reshape(1, 1, 2, 4)
    np.testing.assert_allclose(A.forward_host(q, q, v).reshape(2, 4), [[3, 4, 5, 6]] * 2, atol=1e-3)
    # KAT-2 (tests/test_attention.zig:158-219)
    q = np.full((1, 1, 4, 8), 0.5, np.float32)
    v = np.arange(32, dtype=np.float32).reshape(1, 1, 4, 8)
    np.testing.assert_allclose(A.forward_host(q, q, v).reshape(4, 8), np.tile(np.arange(12, 20), (4, 1)), atol=0.01)
    # KAT-3 (:221-270)
    q = (10.0 * np.eye(8, 8, dtype=np.float32)).reshape(1, 1, 8, 8)
    v = (0.1 * np.arange(8, dtype=np.float32))[:, None].repeat(8, 1).reshape(1, 1, 8, 8)
    assert np.abs(A.forward_host(q, q, v) - v).max() < 0.1
    # stability (:272-325)
    rng = np.random.RandomState(1)
    q, k, v = (rng.uniform(-5, 5, (1, 2, 32, 32)).astype(np.float32) for _ in range(3))
    assert np.isfinite(A.forward_host(q, k, v)).all()


def test_handle_path_gqa_cross_attention(A, oracle_mod):
    """aule_attention_forward_gpu: Hkv from K's shape, Sk from K (tests/test_gqa_unit.py:46-55,
    tests/test_cross_attn.py:54-60, 1e-3 there)."""
    rng = np.random.RandomState(2)
    q = rng.randn(2, 12, 16, 64).astype(np.float32)
    k = rng.randn(2, 2, 32, 64).astype(np.float32)
    v = rng.randn(2, 2, 32, 64).astype(np.float32)
    for causal in (False, True):
        out = A.attention(q, k, v, causal=causal)
        assert_close(out, oracle_mod.fwd_f64(q, k, v, causal)[0], 1e-5, 1e-5, f"gqa causal={causal}")
    with pytest.raises(Exception):
        A.attention(q, k[:, :, :, :32], v[:, :, :, :32])
    # shape mismatch surfaces as -3 "ShapeMismatch"
    qt, kt = A.tensor((1, 2, 8, 32)), A.tensor((1, 2, 8, 64))
    from aule import AuleError
    with pytest.raises(AuleError, match="ShapeMismatch"):
        A.attention_gpu(qt, kt, kt, qt)
    qt.destroy(); kt.destroy()


def test_training_path_host_pointers(A, oracle_mod):
    """aule_attention_forward_with_lse + aule_attention_backward (src/lib.zig:765, :639)."""
    rng = np.random.RandomState(3)
    for shape, causal in (((1, 4, 48, 64), True), ((2, 2, 33, 32), False), ((1, 2, 40, 128), True),
                          ((1, 2, 24, 20), True)):
        q, k, v, do = (rng.randn(*shape).astype(np.float32) for _ in range(4))
        out, lse = A.attention_forward_with_lse(q, k, v, causal=causal)
        ref, ref_lse = oracle_mod.fwd_f64(q, k, v, causal)
        assert_close(out, ref, 1e-5, 1e-5, "out")
        assert_close(lse, ref_lse, 1e-5, 1e-5, "lse")
        dq, dk, dv = A.attention_backward(q, k, v, out, do, lse, causal=causal)
        rq, rk, rv = oracle_mod.bwd_f64(q, k, v, do, causal)
        for name, a, b in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
            assert_close(a, b, 3e-5 * max(1.0, float(np.abs(b).max())), 3e-5, name)


def test_ex_rejects_bad_arguments(A):
    from aule import _capi
    lib = A._lib
    d = _capi.AttnDesc()
    assert lib.aule_attention_forward_ex(ctypes.byref(d)) == -3                # struct_size 0
    d.struct_size = ctypes.sizeof(_capi.AttnDesc)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = 2, 1, 3, 2, 8, 8, 64
    assert lib.aule_attention_forward_ex(ctypes.byref(d)) == -3                # Hq % Hkv
    d.heads_q = 4
    d.head_dim = 48
    assert lib.aule_attention_forward_ex(ctypes.byref(d)) == -3                # head_dim
    d.head_dim = 64
    d.window_size = 4                                                          # accepted (sliding window)
    assert lib.aule_attention_forward_ex(ctypes.byref(d)) == -3                # null pointers
    assert b"null" in lib.aule_get_error()


def test_library_loaded_before_torch_still_finds_the_device():
    """ONE HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64, libaule.so links the system's.  Loading
    libaule.so first used to leave both in the process -- torch's took the device and aule_init() failed with "no ROCm-capable
    device" (build() followed by smoke() in one interpreter).  _capi.load() now loads torch's runtime first when torch is installed
    but not imported yet; this runs that order in a fresh interpreter and counts the runtimes mapped."""
    import subprocess
    import sys
    from conftest import ROOT
    prog = r'''
import os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "aule-attention_amd"))
from aule import _capi
assert "torch" not in sys.modules
lib = _capi.load()
import torch
assert torch.cuda.is_available()
_capi.get_lib()          # aule_init()
hip = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l})
assert len(hip) == 1, hip
import aule
q = torch.randn(1, 2, 128, 64, device="cuda", dtype=torch.bfloat16)
o = aule.flash_attention(q, q, q, causal=True)
torch.cuda.synchronize()
assert torch.isfinite(o.float()).all()
print("ORDER_OK", hip[0])
'''
    r = subprocess.run([sys.executable, "-c", prog, ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "ORDER_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]


def test_launch_entries_refuse_with_the_checkers_texts_and_still_launch(A, oracle_mod):
    """The descriptor checkers of aule_capi.cpp through the launch entries, on tiny shapes: every refused descriptor returns its code
    with the exact aule_get_error() text and launches nothing (the outputs keep their fill), the empty-extent cases return 0 and write
    nothing, and one accepted call per entry point still computes the right thing."""
    import torch
    from aule import _capi
    from util import BWD_TOL, fwd_tol
    lib = _capi.get_lib()
    dev = torch.device("cuda", 0)
    FILL = 7.0
    g = torch.Generator(device="cpu").manual_seed(11)
    rand = lambda *shape, dtype=torch.float16: torch.randn(*shape, generator=g).to(dev, dtype)
    filled = lambda *shape, dtype=torch.float16: torch.full(shape, FILL, device=dev, dtype=dtype)

    def refused(call, d, changes, code, text):
        keep = {f: getattr(d, f) for f in changes}
        for f, v in changes.items():
            setattr(d, f, v)
        rc = call(ctypes.byref(d))
        err = lib.aule_get_error().decode()
        for f, v in keep.items():
            setattr(d, f, v)
        assert (rc, err) == (code, text), (changes, rc, err)

    # ---- forward and backward: B 1, Hq 2, Hkv 1, Sq = Sk = 64, D 32, fp16
    B, Hq, Hkv, S, D = 1, 2, 1, 64, 32
    q, k, v, do = rand(B, Hq, S, D), rand(B, Hkv, S, D), rand(B, Hkv, S, D), rand(B, Hq, S, D)
    out, lse = filled(B, Hq, S, D), filled(B, Hq, S, dtype=torch.float32)
    dq, dk, dv = filled(B, Hq, S, D), filled(B, Hkv, S, D), filled(B, Hkv, S, D)
    f = _capi.AttnDesc()
    b = _capi.AttnBwdDesc()
    for d in (f, b):
        d.struct_size, d.dtype, d.causal, d.window_size, d.device = ctypes.sizeof(d), _capi.DTYPE_F16, 1, -1, 0
        d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, S, S, D
        d.q, d.k, d.v, d.out, d.lse = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr()
    b.dout, b.dq, b.dk, b.dv = do.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    need = int(lib.aule_attention_backward_workspace_size(ctypes.byref(b)))
    ws = torch.zeros(need, device=dev, dtype=torch.uint8)
    b.workspace, b.workspace_bytes = ws.data_ptr(), need
    shared = [   # the rules both directions share say "Attention failed" in both
        ({"causal": 3}, "Attention failed: unknown causal mode 3 (0 none, 1 top-left, 2 bottom-right)"),
        ({"causal": -1}, "Attention failed: unknown causal mode -1 (0 none, 1 top-left, 2 bottom-right)"),
        ({"causal": 2, "seq_k": 32}, "Attention failed: bottom-right causal alignment needs seq_k (32) >= seq_q (64)"),
        ({"dtype": 3}, "Attention failed: unknown dtype 3"),
        ({"dtype": -1}, "Attention failed: unknown dtype -1"),
        ({"head_dim": 48}, "Attention failed: head_dim 48 unsupported (32, 64, 128 or 256; pad to the next size)"),
        ({"head_dim": 0}, "Attention failed: head_dim 0 unsupported (32, 64, 128 or 256; pad to the next size)"),
        ({"head_dim": 512}, "Attention failed: head_dim 512 unsupported (32, 64, 128 or 256; pad to the next size)"),
        ({"heads_kv": 0}, "Attention failed: heads_q (2) must be divisible by heads_kv (0)"),
        ({"heads_q": 3, "heads_kv": 2}, "Attention failed: heads_q (3) must be divisible by heads_kv (2)"),
        ({"seq_k": 1 << 24}, "Attention failed: problem too large"),          # seq_k * head_dim * 4 bytes = 2^31
        ({"seq_q": 1 << 24}, "Attention failed: problem too large"),
    ]
    for changes, text in shared:
        refused(lib.aule_attention_forward_ex, f, changes, -3, text)
        refused(lib.aule_attention_backward_ex, b, changes, -3, text)
    for size in (0, ctypes.sizeof(f) - 8):
        refused(lib.aule_attention_forward_ex, f, {"struct_size": size}, -3, "Attention failed: bad descriptor (struct_size mismatch)")
    for size in (0, ctypes.sizeof(b) - 8):
        refused(lib.aule_attention_backward_ex, b, {"struct_size": size}, -3, "Backward failed: bad descriptor (struct_size mismatch)")
    refused(lib.aule_attention_forward_ex, f, {"seq_k": 0}, -3, "Attention failed: empty key sequence")
    refused(lib.aule_attention_forward_ex, f, {"out": None}, -3, "Attention failed: null tensor pointer")
    refused(lib.aule_attention_backward_ex, b, {"seq_k": 0}, -3, "Backward failed: empty sequence")
    refused(lib.aule_attention_backward_ex, b, {"seq_q": 0}, -3, "Backward failed: empty sequence")
    refused(lib.aule_attention_backward_ex, b, {"dk": None}, -3, "Backward failed: null tensor pointer")
    # (the text names the minimum, which the size query's answer may exceed by the optional dS room: found through the route hook)
    b.workspace_bytes = need - 1
    least = need if lib.aule_hip_debug_backward_route(ctypes.byref(b)) == -3 else None
    b.workspace_bytes = need
    assert least is not None, "the size query asks for more than the minimum on this shape: pick the minimum another way"
    refused(lib.aule_attention_backward_ex, b, {"workspace_bytes": 0}, -3, "Backward failed: workspace too small (0 < %d bytes)" % least)
    refused(lib.aule_attention_backward_ex, b, {"workspace_bytes": least - 1}, -3, "Backward failed: workspace too small (%d < %d bytes)" % (least - 1, least))
    assert lib.aule_attention_forward_ex(None) == -3 and lib.aule_attention_backward_ex(None) == -3
    assert lib.aule_attention_backward_workspace_size(None) == 0 and lib.aule_attention_forward_workspace_size(None) == 0
    # nothing to do: 0, nothing written (no output element; for the backward no key element either)
    for changes in ({"batch": 0}, {"seq_q": 0}, {"heads_q": 0}):
        refused(lib.aule_attention_forward_ex, f, changes, 0, lib.aule_get_error().decode())
    refused(lib.aule_attention_backward_ex, b, {"batch": 0}, 0, lib.aule_get_error().decode())
    torch.cuda.synchronize()
    for name, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert bool((t == FILL).all()), name + " was written by a refused or empty call"
    # accepted
    assert lib.aule_attention_forward_ex(ctypes.byref(f)) == 0 and lib.aule_attention_backward_ex(ctypes.byref(b)) == 0
    torch.cuda.synchronize()
    qn, kn, vn, dn = (x.float().cpu().numpy() for x in (q, k, v, do))
    ref, ref_lse = oracle_mod.fwd_f64(qn, kn, vn, True)
    assert_close(out.float().cpu().numpy(), ref, *fwd_tol("fp16", np.abs(vn).max()), "forward_ex")
    assert_close(lse.cpu().numpy(), ref_lse, 1e-3, 1e-3, "forward_ex lse")
    for name, got, r in zip(("dq", "dk", "dv"), (dq, dk, dv), oracle_mod.bwd_f64(qn, kn, vn, dn, True)):
        assert_close(got.float().cpu().numpy(), r, BWD_TOL["fp16"][0] * max(1.0, float(np.abs(r).max())), BWD_TOL["fp16"][1], "backward_ex " + name)

    # ---- paged decode, 16-bit and FP8 caches: batch 1, heads 2 / 1, D 32, block_size 8, max_blocks 2
    bs, mb = 8, 2
    pq, pout = rand(1, Hq, D), filled(1, Hq, D)
    kc, vc = rand(mb, bs, Hkv, D), rand(mb, bs, Hkv, D)
    kc8, vc8 = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
    ones = torch.ones(Hkv, device=dev, dtype=torch.float32)
    bt = torch.tensor([[1, 0]], device=dev, dtype=torch.int32)
    cl = torch.tensor([13], device=dev, dtype=torch.int32)
    for fp8, what, call in ((False, "Paged attention", lib.aule_attention_paged_decode_ex), (True, "Paged FP8 attention", lib.aule_attention_paged_decode_fp8_ex)):
        p = _capi.PagedFp8Desc() if fp8 else _capi.PagedDesc()
        p.struct_size, p.dtype, p.window_size, p.device = ctypes.sizeof(p), _capi.DTYPE_F16, -1, 0
        p.batch, p.heads_q, p.heads_kv, p.head_dim, p.block_size, p.max_blocks = 1, Hq, Hkv, D, bs, mb
        p.q, p.out, p.block_tables, p.context_lens = pq.data_ptr(), pout.data_ptr(), bt.data_ptr(), cl.data_ptr()
        p.k_cache, p.v_cache = (kc8.data_ptr(), vc8.data_ptr()) if fp8 else (kc.data_ptr(), vc.data_ptr())
        if fp8:
            p.k_scale, p.v_scale = ones.data_ptr(), ones.data_ptr()
        pout.fill_(FILL)
        for size in (0, ctypes.sizeof(p) - 8):
            refused(call, p, {"struct_size": size}, -3, what + " failed: bad descriptor (struct_size mismatch)")
        for dt in (0, 3):
            refused(call, p, {"dtype": dt}, -3, what + (" failed: dtype (of q / out) must be fp16 or bf16" if fp8 else " failed: dtype must be fp16 or bf16"))
        refused(call, p, {"head_dim": 256}, -3, what + " failed: head_dim 256 unsupported (32, 64 or 128)")
        refused(call, p, {"head_dim": 48}, -3, what + " failed: head_dim 48 unsupported (32, 64 or 128)")
        refused(call, p, {"heads_kv": 0}, -3, what + " failed: heads_q (2) must be divisible by heads_kv (0)")
        refused(call, p, {"heads_q": 3, "heads_kv": 2}, -3, what + " failed: heads_q (3) must be divisible by heads_kv (2)")
        for changes in ({"block_size": 0}, {"max_blocks": 0}, {"block_size": 1 << 15, "max_blocks": 1 << 15}):
            refused(call, p, changes, -3, what + " failed: bad block_size / max_blocks")
        refused(call, p, {"out": None}, -3, what + " failed: null tensor pointer")
        if fp8:
            refused(call, p, {"v_scale": None}, -3, what + " failed: null scale pointer (k_scale and v_scale are [heads_kv] fp32 device arrays)")
        refused(call, p, {"batch": 0}, 0, lib.aule_get_error().decode())
        torch.cuda.synchronize()
        assert bool((pout == FILL).all()), what
        assert call(ctypes.byref(p)) == 0
        torch.cuda.synchronize()
        kn, vn = ((kc8, vc8) if fp8 else (kc, vc))
        vn = vn.float().cpu().numpy()
        ref = oracle_mod.paged_decode_f64(pq.float().cpu().numpy(), kn.float().cpu().numpy(), vn, bt.cpu().numpy(), cl.cpu().numpy())
        assert_close(pout.float().cpu().numpy(), ref, *fwd_tol("fp16", np.abs(vn).max()), what)

    # ---- aule_rope_ex: 2 rows of heads, seq 8, head_dim 32, fp32
    x, y = rand(1, 2, 8, D, dtype=torch.float32), filled(1, 2, 8, D, dtype=torch.float32)
    cos_n, sin_n = oracle_mod.rope_tables(8, D)
    cos, sin = torch.from_numpy(cos_n).to(dev), torch.from_numpy(sin_n).to(dev)
    r = _capi.RopeDesc()
    r.struct_size, r.dtype, r.rows_bh, r.seq, r.head_dim, r.row_pitch = ctypes.sizeof(r), _capi.DTYPE_F32, 2, 8, D, D
    r.table_len, r.table_pitch, r.layout, r.inverse, r.pos_offset, r.device = 8, 0, _capi.ROPE_HALF, 0, 0, 0
    r.in_, r.out, r.cos, r.sin = x.data_ptr(), y.data_ptr(), cos.data_ptr(), sin.data_ptr()
    for changes, text in (({"struct_size": 0}, "RoPE failed: bad descriptor (struct_size mismatch)"),
                          ({"dtype": 3}, "RoPE failed: unknown dtype 3"),
                          ({"head_dim": 33}, "RoPE failed: head_dim (33) must be even and <= row_pitch (32)"),
                          ({"head_dim": 0}, "RoPE failed: head_dim (0) must be even and <= row_pitch (32)"),
                          ({"row_pitch": 16}, "RoPE failed: head_dim (32) must be even and <= row_pitch (16)"),
                          ({"layout": 2}, "RoPE failed: unknown layout 2"),
                          ({"table_len": 4}, "RoPE failed: table too short (4 rows < seq 8 + pos_offset 0)"),
                          ({"pos_offset": 1}, "RoPE failed: table too short (8 rows < seq 8 + pos_offset 1)"),
                          ({"table_pitch": 8}, "RoPE failed: table_pitch (8) < head_dim/2"),
                          ({"rows_bh": 1 << 40}, "RoPE failed: problem too large"),
                          ({"cos": None}, "RoPE failed: null pointer")):
        refused(lib.aule_rope_ex, r, changes, -3, text)
    for changes in ({"rows_bh": 0}, {"seq": 0}):
        refused(lib.aule_rope_ex, r, changes, 0, lib.aule_get_error().decode())
    torch.cuda.synchronize()
    assert bool((y == FILL).all())
    assert lib.aule_rope_ex(ctypes.byref(r)) == 0
    torch.cuda.synchronize()
    want = oracle_mod.rope_f64(x.cpu().numpy(), cos_n, sin_n)
    assert_close(y.cpu().numpy(), want, 1e-5 * max(1.0, float(np.abs(want).max())), 0, "rope_ex")
