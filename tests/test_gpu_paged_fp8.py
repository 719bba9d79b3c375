"""Paged decode over an FP8 (OCP e4m3fn) KV cache with per-KV-head scales, on the GPU
(the KvFp8 instances of csrc/fa_fwd_splitkv_gfx950.hip behind aule.flash_attention_paged_amd / aule_attention_paged_decode_fp8_ex).

The judge is the fp64 oracle `paged_decode_f64` on the DEQUANTISED caches -- scale[hk] * float(code), formed in float64 on
the host -- and the 16-bit-rounded query; never the kernel under test and never the 16-bit kernel.  The bound is the
project's forward bound fwd_tol(dtype, max |v_scale * V|), unchanged: the conversion of a code to 16 bit is exact, both
scales are applied in fp32 to fp32 quantities (relative error 2^-24), and the two error terms of the 16-bit algorithm (P
rounded to the V type, O rounded to storage) are the ones fwd_tol accounts for."""
import ctypes
import math

import numpy as np
import pytest

from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

CASES = [  # dtype, B, Hq, Hkv, D, block_size, context lens, window   (the list of tests/test_gpu_paged.py)
    ("bf16", 4, 32, 8, 128, 16, [1000, 37, 4096, 1], -1),
    ("fp16", 2, 32, 1, 64, 128, [5000, 129], -1),
    ("bf16", 3, 8, 8, 128, 8, [0, 77, 300], -1),
    ("fp16", 2, 16, 4, 32, 32, [2048, 2047], 256),
    ("bf16", 1, 64, 8, 128, 64, [20000], -1),
    ("bf16", 3, 16, 4, 128, 48, [1000, 47, 4000], -1),
    ("fp16", 2, 32, 8, 64, 24, [3001, 25], -1),
    ("fp16", 2, 8, 2, 32, 100, [2500, 99], 300),
    ("bf16", 2, 8, 8, 128, 1, [700, 3], -1),
    ("bf16", 2, 32, 4, 64, 33, [5000, 1], 64),
]
CODE_8 = 0x50   # e4m3fn code of 8.0: magnitudes 0 .. CODE_8 are the finite codes with |x| <= 8


def _decode(codes_u8):
    """uint8 codes -> float64 values (host)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(codes_u8)).view(torch.float8_e4m3fn).float().numpy().astype(np.float64)


def _codes_of(t8):
    return t8.view(__import__("torch").uint8).cpu().numpy()


def _uniform_codes(rng, shape):
    return (rng.randint(0, CODE_8 + 1, size=shape) | (rng.randint(0, 2, size=shape) << 7)).astype(np.uint8)


def _table(rng, B, bs, lens, num_blocks, extra_cols=2):
    nblk = [(n + bs - 1) // bs for n in lens]
    bt = np.zeros((B, max(max(nblk), 1) + extra_cols), dtype=np.int32)    # unused columns point at block 0
    perm = rng.permutation(num_blocks)
    used = 0
    for b in range(B):
        bt[b, :nblk[b]] = perm[used:used + nblk[b]]
        used += nblk[b]
    return bt


def _to_fp8(torch, codes_u8):
    return torch.from_numpy(codes_u8).cuda().view(torch.float8_e4m3fn)


def _run(torch, q, kcodes, vcodes, bt, cl, dtype, scale=None, window=-1, k_scale=None, v_scale=None):
    import aule
    out = aule.flash_attention_paged_amd(torch.from_numpy(q).to("cuda", torch_dtype(dtype)), _to_fp8(torch, kcodes),
                                         _to_fp8(torch, vcodes), torch.from_numpy(bt).cuda(), torch.from_numpy(cl).cuda(),
                                         scale=scale, window_size=window, k_scale=k_scale, v_scale=v_scale)
    return out


def _oracle(oracle_mod, q, kcodes, vcodes, ks, vs, bt, cl, scale=None, window=-1):
    """ks, vs: [Hkv] float64 (or None = 1).  Returns (reference, max |v_scale * V|)."""
    K, V = _decode(kcodes), _decode(vcodes)
    if ks is not None:
        K = K * np.asarray(ks, dtype=np.float64).reshape(1, 1, -1, 1)
    if vs is not None:
        V = V * np.asarray(vs, dtype=np.float64).reshape(1, 1, -1, 1)
    return oracle_mod.paged_decode_f64(q, K, V, bt, cl, scale, window), float(np.abs(V).max())


def _ids(c):
    return f"{c[0]}-B{c[1]}-H{c[2]}kv{c[3]}-D{c[4]}-bs{c[5]}-w{c[7]}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp8_paged_vs_oracle_with_helper_scales(case, oracle_mod):
    """Caches built by aule.quantize_kv_cache_fp8 from 3 N(0,1) data: per-head scales that are not 1 and differ."""
    import torch
    import aule
    dtype, B, Hq, Hkv, D, bs, lens, window = case
    rng = np.random.RandomState(131)
    nblk = [(n + bs - 1) // bs for n in lens]
    num_blocks = sum(nblk) + 3
    q = quantize(rng.randn(B, Hq, D).astype(np.float32), dtype)
    kc8, ks = aule.quantize_kv_cache_fp8(torch.from_numpy(3 * rng.randn(num_blocks, bs, Hkv, D).astype(np.float32)))
    vc8, vs = aule.quantize_kv_cache_fp8(torch.from_numpy(3 * rng.randn(num_blocks, bs, Hkv, D).astype(np.float32)))
    if Hkv > 1:
        assert len(set(ks.tolist())) > 1 and len(set(vs.tolist())) > 1
    assert not bool((ks == 1).any()) and not bool((vs == 1).any())
    bt = _table(rng, B, bs, lens, num_blocks)
    cl = np.array(lens, dtype=np.int32)
    kcodes, vcodes = _codes_of(kc8), _codes_of(vc8)
    out = _run(torch, q, kcodes, vcodes, bt, cl, dtype, None, window, k_scale=ks, v_scale=vs).float().cpu().numpy()
    ref, vmax = _oracle(oracle_mod, q, kcodes, vcodes, ks.double().numpy(), vs.double().numpy(), bt, cl, None, window)
    atol, rtol = fwd_tol(dtype, vmax)
    print("max err %.3g (atol %.3g)" % (np.abs(out - ref).max(), atol))
    assert_close(out, ref, atol, rtol, "fp8 paged, helper scales")


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_fp8_paged_vs_oracle_without_scales(case, oracle_mod):
    """k_scale = v_scale = None on codes drawn uniformly from the finite ones with |x| <= 8 (subnormals and both zeros
    included)."""
    import torch
    dtype, B, Hq, Hkv, D, bs, lens, window = case
    rng = np.random.RandomState(132)
    nblk = [(n + bs - 1) // bs for n in lens]
    num_blocks = sum(nblk) + 3
    q = quantize(0.25 * rng.randn(B, Hq, D).astype(np.float32), dtype)
    kcodes = _uniform_codes(rng, (num_blocks, bs, Hkv, D))
    vcodes = _uniform_codes(rng, (num_blocks, bs, Hkv, D))
    bt = _table(rng, B, bs, lens, num_blocks)
    cl = np.array(lens, dtype=np.int32)
    out = _run(torch, q, kcodes, vcodes, bt, cl, dtype, None, window).float().cpu().numpy()
    ref, vmax = _oracle(oracle_mod, q, kcodes, vcodes, None, None, bt, cl, None, window)
    atol, rtol = fwd_tol(dtype, vmax)
    print("max err %.3g (atol %.3g)" % (np.abs(out - ref).max(), atol))
    assert_close(out, ref, atol, rtol, "fp8 paged, no scales")


def _small_problem(rng, dtype, B=3, Hq=16, Hkv=4, D=128, bs=16, lens=(900, 33, 2048)):
    nblk = [(n + bs - 1) // bs for n in lens]
    num_blocks = sum(nblk) + 2
    q = quantize(0.25 * rng.randn(B, Hq, D).astype(np.float32), dtype)
    kcodes = _uniform_codes(rng, (num_blocks, bs, Hkv, D))
    vcodes = _uniform_codes(rng, (num_blocks, bs, Hkv, D))
    bt = _table(rng, B, bs, list(lens), num_blocks)
    return q, kcodes, vcodes, bt, np.array(lens, dtype=np.int32)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_scales_mean_what_the_header_says(dtype, oracle_mod):
    """k_scale doubled with `scale` halved gives the same logits: both calls are within fwd_tol of their oracle (which is
    the same).  They are also BIT-IDENTICAL, and that is asserted: the kernel's softmax factor is the plain fp32 product
    (scale * log2 e) * k_scale[hk], and halving one factor while doubling the other is exact.  v_scale * 2 doubles the
    output to within one output ulp (in fact exactly: the partials are scaled by a power of two).  Float, 0-d tensor and
    [Hkv] tensor forms of one scale give equal outputs."""
    import torch
    rng = np.random.RandomState(7)
    q, kcodes, vcodes, bt, cl = _small_problem(rng, dtype)
    Hkv, D = kcodes.shape[2], q.shape[2]
    ks = np.array([0.37, 1.9, 0.052, 3.3])
    vs = np.array([2.5, 0.11, 0.73, 1.0])
    sc = 1.0 / math.sqrt(D)
    tk, tv = torch.tensor(ks, dtype=torch.float32), torch.tensor(vs, dtype=torch.float32)
    a = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, tk, tv)
    b = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc / 2, -1, 2 * tk, tv)
    ref, vmax = _oracle(oracle_mod, q, kcodes, vcodes, tk.double().numpy(), tv.double().numpy(), bt, cl, sc)
    atol, rtol = fwd_tol(dtype, vmax)
    assert_close(a.float().cpu().numpy(), ref, atol, rtol, "k_scale, scale")
    assert_close(b.float().cpu().numpy(), ref, atol, rtol, "2 k_scale, scale / 2")
    assert torch.equal(a, b)
    c = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, tk, 2 * tv)
    ulp = 2.0 ** (-7 if dtype == "bf16" else -10)
    d = (c.double() - 2 * a.double()).abs()
    assert bool((d <= ulp * (2 * a.double()).abs() + 2.0 ** -24).all()), float(d.max())
    # one value in three forms
    f = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, 0.75, 1.5)
    z = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, torch.tensor(0.75), torch.tensor(1.5, device="cuda"))
    t = _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, torch.full((Hkv,), 0.75, device="cuda"), torch.full((Hkv,), 1.5))
    assert torch.equal(f, z) and torch.equal(f, t)
    # and None is 1.0
    assert torch.equal(_run(torch, q, kcodes, vcodes, bt, cl, dtype, sc), _run(torch, q, kcodes, vcodes, bt, cl, dtype, sc, -1, 1.0, 1.0))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fp8_agrees_with_the_16_bit_path_on_the_expanded_cache(dtype, oracle_mod):
    """Power-of-two scales, so scale * code rounded to the query type is exact and the 16-bit call sees the same K and V:
    the two differ by summation order and output rounding only -- at most 2^-7 max|ref| (bf16) / 2^-10 max|ref| (fp16),
    the form test_paged_equals_contiguous_decode uses.  Both are also held to the oracle bound."""
    import torch
    import aule
    rng = np.random.RandomState(8)
    q, kcodes, vcodes, bt, cl = _small_problem(rng, dtype)
    ks = np.array([0.5, 2.0, 0.25, 1.0])
    vs = np.array([4.0, 0.125, 1.0, 0.5])
    dt = torch_dtype(dtype)
    K16 = torch.from_numpy(_decode(kcodes) * ks.reshape(1, 1, -1, 1)).to(dt)
    V16 = torch.from_numpy(_decode(vcodes) * vs.reshape(1, 1, -1, 1)).to(dt)
    assert np.array_equal(K16.double().numpy(), _decode(kcodes) * ks.reshape(1, 1, -1, 1))   # the expansion is exact
    assert np.array_equal(V16.double().numpy(), _decode(vcodes) * vs.reshape(1, 1, -1, 1))
    got8 = _run(torch, q, kcodes, vcodes, bt, cl, dtype, None, -1, torch.tensor(ks, dtype=torch.float32),
                torch.tensor(vs, dtype=torch.float32)).float().cpu().numpy()
    got16 = aule.flash_attention_paged_amd(torch.from_numpy(q).to("cuda", dt), K16.cuda(), V16.cuda(),
                                           torch.from_numpy(bt).cuda(), torch.from_numpy(cl).cuda()).float().cpu().numpy()
    ref, vmax = _oracle(oracle_mod, q, kcodes, vcodes, ks, vs, bt, cl)
    atol, rtol = fwd_tol(dtype, vmax)
    assert_close(got8, ref, atol, rtol, "fp8")
    assert_close(got16, ref, atol, rtol, "16-bit on the expanded cache")
    diff = float(np.abs(got8 - got16).max())
    bound = 2.0 ** (-7 if dtype == "bf16" else -10) * float(np.abs(ref).max())
    print("fp8 vs 16-bit: %.3g (bound %.3g)" % (diff, bound))
    assert diff <= bound, (diff, bound)


def test_fp8_robustness_carried_over(oracle_mod):
    """Context length 0 -> zeros; a context length beyond max_blocks * block_size is clamped on the device (equal to the
    clamped call); block table and lengths as CPU tensors; a non-contiguous cache view."""
    import torch
    import aule
    torch.manual_seed(9)
    rng = np.random.RandomState(9)
    B, Hq, Hkv, D, bs, nb = 3, 8, 2, 128, 16, 6
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.float16)
    kcodes = _uniform_codes(rng, (B * nb, bs, Hkv, D))
    vcodes = _uniform_codes(rng, (B * nb, bs, Hkv, D))
    kc, vc = _to_fp8(torch, kcodes), _to_fp8(torch, vcodes)
    ks, vs = torch.tensor([0.3, 1.7], device="cuda"), torch.tensor([2.0, 0.6], device="cuda")
    bt = torch.arange(B * nb, dtype=torch.int32).reshape(B, nb)            # CPU on purpose
    full = torch.tensor([nb * bs, nb * bs, 0], dtype=torch.int32)
    over = torch.tensor([nb * bs + 1000, 2 ** 30, -5], dtype=torch.int32)
    ref = aule.flash_attention_paged_amd(q, kc, vc, bt, full, k_scale=ks, v_scale=vs)
    got = aule.flash_attention_paged_amd(q, kc, vc, bt, over, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert bool((ref[2] == 0).all())                                       # no key: zeros
    want, vmax = _oracle(oracle_mod, q.float().cpu().numpy(), kcodes, vcodes, ks.double().cpu().numpy(),
                         vs.double().cpu().numpy(), bt.numpy(), full.numpy())
    atol, rtol = fwd_tol("fp16", vmax)
    assert_close(ref.float().cpu().numpy(), want, atol, rtol, "fp8 paged, CPU tables")
    # a non-contiguous view (every other head of a cache with twice the heads) equals its contiguous copy
    wide_k = _to_fp8(torch, _uniform_codes(rng, (B * nb, bs, 2 * Hkv, D)))
    wide_v = _to_fp8(torch, _uniform_codes(rng, (B * nb, bs, 2 * Hkv, D)))
    vk, vv = wide_k[:, :, ::2], wide_v[:, :, ::2]
    assert not vk.is_contiguous()
    a = aule.flash_attention_paged_amd(q, vk, vv, bt, full, k_scale=ks, v_scale=vs)
    b = aule.flash_attention_paged_amd(q, vk.contiguous(), vv.contiguous(), bt, full, k_scale=ks, v_scale=vs)
    assert torch.equal(a, b)


def test_fp8_cache_offsets_beyond_2_gib(oracle_mod):
    """The 16-bit suite allocates no cache of 4 GiB, so this is the other form: block tables that point at the LAST
    blocks of an FP8 cache of more than 2 GiB (byte offsets past 2^31), checked against the oracle on the gathered rows."""
    import torch
    import aule
    B, Hq, Hkv, D, bs, per_seq = 2, 16, 8, 128, 16, 40
    blk_bytes = bs * Hkv * D
    num_blocks = (2 ** 31) // blk_bytes + B * per_seq + 8   # every block in use starts past 2^31 bytes
    g = torch.Generator(device="cuda").manual_seed(11)

    def cache():
        mag = torch.randint(0, CODE_8 + 1, (num_blocks, bs, Hkv, D), device="cuda", dtype=torch.uint8, generator=g)
        mag[-B * per_seq:] |= (torch.randint(0, 2, (B * per_seq, bs, Hkv, D), device="cuda", dtype=torch.uint8, generator=g) << 7)
        return mag
    ku, vu = cache(), cache()
    last = torch.arange(num_blocks - B * per_seq, num_blocks, dtype=torch.int32)
    bt = last[torch.randperm(B * per_seq, generator=torch.Generator().manual_seed(12))].reshape(B, per_seq).contiguous()
    assert int(bt.min()) * blk_bytes > 2 ** 31
    cl = torch.tensor([per_seq * bs, per_seq * bs - 21], dtype=torch.int32)
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.bfloat16, generator=g) * 0.25
    ks = torch.linspace(0.2, 1.6, Hkv)
    vs = torch.linspace(1.5, 0.3, Hkv)
    out = aule.flash_attention_paged_amd(q, ku.view(torch.float8_e4m3fn), vu.view(torch.float8_e4m3fn), bt.cuda(), cl.cuda(),
                                         k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    # the oracle sees only the blocks in use, renumbered
    first = num_blocks - B * per_seq
    ksub, vsub = ku[first:].cpu().numpy(), vu[first:].cpu().numpy()
    ref, vmax = _oracle(oracle_mod, q.float().cpu().numpy(), ksub, vsub, ks.double().numpy(), vs.double().numpy(),
                        (bt - first).numpy(), cl.numpy())
    atol, rtol = fwd_tol("bf16", vmax)
    assert_close(out.float().cpu().numpy(), ref, atol, rtol, "fp8 paged, offsets past 2 GiB")


def _capture(torch, fn, steps=3):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    outs = []
    with torch.cuda.graph(g):
        for _ in range(steps):
            outs.append(fn())
    return g, outs


def test_fp8_paged_decode_capture_replays_bit_identical():
    """As tests/test_gpu_graph.py does for the 16-bit paged decode; the scales are device tensors."""
    import torch
    import aule
    torch.manual_seed(3)
    rng = np.random.RandomState(3)
    B, Hq, Hkv, D, bs, n = 4, 32, 8, 128, 16, 4096
    nb = n // bs
    kc = _to_fp8(torch, _uniform_codes(rng, (B * nb, bs, Hkv, D)))
    vc = _to_fp8(torch, _uniform_codes(rng, (B * nb, bs, Hkv, D)))
    q = torch.randn(B, Hq, D, device="cuda", dtype=torch.float16)
    bt = torch.randperm(B * nb, device="cuda").to(torch.int32).view(B, nb)
    cl = torch.tensor([n, 1000, 37, n - 1], device="cuda", dtype=torch.int32)
    ks = torch.linspace(0.2, 1.6, Hkv, device="cuda")
    vs = torch.linspace(1.5, 0.3, Hkv, device="cuda")
    fn = lambda: aule.flash_attention_paged_amd(q, kc, vc, bt, cl, k_scale=ks, v_scale=vs)   # noqa: E731
    eager = fn()
    torch.cuda.synchronize()
    g, outs = _capture(torch, fn)
    for _ in range(3):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, eager) for o in outs)


def _fp8_desc(torch, q, kc, vc, bt, cl, out, ks, vs):
    from aule import _capi
    B, Hq, D = q.shape
    d = _capi.PagedFp8Desc()
    d.struct_size = ctypes.sizeof(_capi.PagedFp8Desc)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[q.dtype]
    d.batch, d.heads_q, d.heads_kv, d.head_dim = B, Hq, kc.shape[2], D
    d.block_size, d.max_blocks = kc.shape[1], bt.shape[1]
    d.scale, d.window_size, d.device = 0.0, -1, q.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr()
    d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
    d.k_scale, d.v_scale = ks.data_ptr(), vs.data_ptr()
    return d


def test_fp8_c_abi_directly(oracle_mod):
    """aule_attention_paged_decode_fp8_ex with a caller workspace of exactly the queried size and with none (equal
    results, nothing written past the buffer, right against the oracle); -3 and an error text for a null scale pointer,
    head_dim 256 and an fp32 dtype."""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    rng = np.random.RandomState(21)
    qn, kcodes, vcodes, btn, cln = _small_problem(rng, "bf16")
    q = torch.from_numpy(qn).to("cuda", torch.bfloat16)
    kc, vc = _to_fp8(torch, kcodes), _to_fp8(torch, vcodes)
    bt, cl = torch.from_numpy(btn).cuda(), torch.from_numpy(cln).cuda()
    ks = torch.tensor([0.4, 1.1, 2.2, 0.9], device="cuda")
    vs = torch.tensor([1.3, 0.2, 0.8, 3.0], device="cuda")
    res = []
    for mode in ("exact", "none"):
        out = torch.empty_like(q)
        d = _fp8_desc(torch, q, kc, vc, bt, cl, out, ks, vs)
        need = int(lib.aule_attention_paged_decode_fp8_workspace_size(ctypes.byref(d)))
        assert need > 0
        buf = torch.full((need + 4096,), 0x5A, device="cuda", dtype=torch.uint8)
        if mode == "exact":
            d.workspace, d.workspace_bytes = buf.data_ptr(), need
        assert lib.aule_attention_paged_decode_fp8_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert bool((buf[need:] == 0x5A).all()), "wrote past the workspace it was given"
        if mode == "exact":
            assert not bool((buf[:need] == 0x5A).all()), "did not use the workspace it was given"
        res.append(out)
    assert torch.equal(res[0], res[1])
    ref, vmax = _oracle(oracle_mod, qn, kcodes, vcodes, ks.double().cpu().numpy(), vs.double().cpu().numpy(), btn, cln)
    atol, rtol = fwd_tol("bf16", vmax)
    assert_close(res[0].float().cpu().numpy(), ref, atol, rtol, "fp8 paged through the C-ABI")

    def refused(change, needle):
        d = _fp8_desc(torch, q, kc, vc, bt, cl, torch.empty_like(q), ks, vs)
        change(d)
        assert lib.aule_attention_paged_decode_fp8_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg, msg

    refused(lambda d: setattr(d, "k_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "v_scale", None), "scale pointer")
    refused(lambda d: setattr(d, "head_dim", 256), "head_dim 256")
    refused(lambda d: setattr(d, "dtype", 0), "fp16 or bf16")
    refused(lambda d: setattr(d, "struct_size", 120), "struct_size")
