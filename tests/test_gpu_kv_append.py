"""The paged KV cache append on the GPU (csrc/kv_append_gfx950.hip behind aule.paged_kv_append / aule_kv_cache_append_ex).

The reference has no such kernel, so the expected values come from torch on the CPU -- row copies for 16-bit caches,
(x.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn) for FP8 caches, compared as integers with no tolerance -- and
from the existing, oracle-pinned rotation pass (aule._torch.rope_raw), never from the call under test.  Every GPU step runs
once.  Caches that must stay untouched start from random bits or a canary, so a stray write fails the test."""
import ctypes
import math

import numpy as np
import pytest

from util import assert_close, fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

DTYPES = ["fp16", "bf16"]
HEAD_DIMS = [32, 64, 128]
BLOCK_SIZES = [8, 16, 32, 48]
KV_HEADS = [8, 2, 1]        # of an 8-query-head model: MHA, GQA, MQA (the append sees the KV heads only)


def _bits(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.uint8)


def _rand16(torch, g, shape, dtype, mag=1.0):
    return (torch.randn(*shape, generator=g) * mag).to(torch_dtype(dtype))


def _random_cache(torch, g, shape, dtype):
    """random BITS of the cache's type (NaN patterns included: comparisons are on integers)"""
    if dtype == "fp8":
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn)
    return torch.randint(-2 ** 15, 2 ** 15, shape, generator=g, dtype=torch.int16).view(torch_dtype(dtype))


def _slots(g, torch, T, num_slots):
    return torch.randperm(num_slots, generator=g)[:T].to(torch.int64)


def _ref_codes(torch, x, s):
    """the issue's formula on the CPU: x [T, Hkv, D] 16-bit, s [Hkv] fp32 -> uint8 codes"""
    return (x.float() / s.view(1, -1, 1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _expect(torch, cache0, rows, slots):
    """cache0 with rows written at the valid slots, on the CPU (integer views)"""
    want = _bits(cache0).clone()
    flat = want.view(-1, want.shape[2], want.shape[3])
    ok = (slots >= 0) & (slots < flat.shape[0])
    flat[slots[ok]] = _bits(rows)[ok]
    return want


def _helper_scales(torch, x):
    import aule
    _, s = aule.quantize_kv_cache_fp8(x.unsqueeze(1))
    return s


# ---- 1. 16-bit caches -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_16_bit_cache_rows_are_bit_copies_and_the_rest_is_untouched(dtype, D):
    import torch
    import aule
    g = torch.Generator().manual_seed(1000 + D)
    for bs in BLOCK_SIZES:
        for Hkv in KV_HEADS:
            nb, T = 7, 37
            k, v = _rand16(torch, g, (T, Hkv, D), dtype), _rand16(torch, g, (T, Hkv, D), dtype)
            kc0, vc0 = _random_cache(torch, g, (nb, bs, Hkv, D), dtype), _random_cache(torch, g, (nb, bs, Hkv, D), dtype)
            slots = _slots(g, torch, T, nb * bs)
            kc, vc = kc0.cuda(), vc0.cuda()
            assert aule.paged_kv_append(k.cuda(), v.cuda(), kc, vc, slots.cuda()) is None
            ctx = (dtype, D, bs, Hkv)
            assert torch.equal(_bits(kc).cpu(), _expect(torch, kc0, k, slots)), ctx
            assert torch.equal(_bits(vc).cpu(), _expect(torch, vc0, v, slots)), ctx


# ---- 2. FP8 caches --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_codes_equal_the_cpu_formula(dtype, D):
    """Per-head scales from quantize_kv_cache_fp8 (amax / 448: the largest value of each head lands on +-448 exactly) and
    scales of 1.0 on data that exceeds 448 (saturation)."""
    import torch
    import aule
    g = torch.Generator().manual_seed(2000 + D)
    for bs in BLOCK_SIZES:
        for Hkv in KV_HEADS:
            nb, T = 5, 29
            heads = torch.logspace(-2, 2.5, Hkv).view(1, Hkv, 1)
            k = (torch.randn(T, Hkv, D, generator=g) * heads).to(torch_dtype(dtype))
            v = (torch.randn(T, Hkv, D, generator=g) * heads.flip(1)).to(torch_dtype(dtype))
            slots = _slots(g, torch, T, nb * bs)
            for mode in ("helper", "one"):
                if mode == "helper":
                    ks, vs = _helper_scales(torch, k), _helper_scales(torch, v)
                    assert not bool((ks == 1).any())
                    kw = dict(k_scale=ks, v_scale=vs.cuda())
                else:
                    ks = vs = torch.ones(Hkv)
                    kw = dict(k_scale=1.0, v_scale=None)
                kc0, vc0 = _random_cache(torch, g, (nb, bs, Hkv, D), "fp8"), _random_cache(torch, g, (nb, bs, Hkv, D), "fp8")
                kc, vc = kc0.cuda(), vc0.cuda()
                aule.paged_kv_append(k.cuda(), v.cuda(), kc, vc, slots.cuda(), **kw)
                ctx = (dtype, D, bs, Hkv, mode)
                wk, wv = _ref_codes(torch, k, ks), _ref_codes(torch, v, vs)
                assert not bool(((wk & 0x7F) == 0x7F).any())                      # no NaN code among the expected
                assert torch.equal(_bits(kc).cpu(), _expect(torch, kc0, wk, slots)), ctx
                assert torch.equal(_bits(vc).cpu(), _expect(torch, vc0, wv, slots)), ctx


PLANTED = [  # (input, expected e4m3fn code with scale 1.0): round to nearest even, saturation, NaN -- the issue's table
    (0.0, 0), (-0.0, 128), (1.0, 56), (447.9, 126), (448.0, 126), (465.0, 126), (1e9, 126), (float("inf"), 126),
    (float("-inf"), 254), (2.0 ** -9, 1), (2.0 ** -10, 0), (2.0 ** -11, 0), (1.5 * 2.0 ** -10, 1), (float("nan"), None),
]


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_planted_values(dtype, D):
    """A row of planted values in K and in V (both halves of the row), scale 1.0, against the table and against torch's
    cast on the CPU wherever that is not NaN."""
    import torch
    import aule
    T, Hkv, nb, bs = 3, 2, 2, 4
    vals = torch.tensor([p[0] for p in PLANTED], dtype=torch.float32)
    n = len(PLANTED)
    assert 2 * n <= D or D == 32
    x = torch.zeros(T, Hkv, D)
    if D == 32:          # 14 values do not fit one half twice: first half and second half carry the list once, staggered
        x[1, 1, :n] = vals
        x[2, 0, D - n:] = vals
        where = [(1, 1, 0), (2, 0, D - n)]
    else:
        x[1, 1, 3:3 + n] = vals
        x[1, 1, D // 2 + 1:D // 2 + 1 + n] = vals
        where = [(1, 1, 3), (1, 1, D // 2 + 1)]
    x = x.to(torch_dtype(dtype))
    slots = torch.tensor([5, 0, 2], dtype=torch.int64)
    kc = torch.full((nb, bs, Hkv, D), 0x55, dtype=torch.uint8).view(torch.float8_e4m3fn).cuda()
    vc = kc.clone()
    aule.paged_kv_append(x.cuda(), x.cuda(), kc, vc, slots.cuda(), k_scale=torch.ones(Hkv), v_scale=1.0)
    cpu = (x.float() / 1.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    for cache in (kc, vc):
        got = _bits(cache).cpu().view(-1, Hkv, D)
        for (t, h, off) in where:
            row = got[int(slots[t]), h, off:off + n].tolist()
            print(dtype, D, row)
            for (val, code), have, torch_code in zip(PLANTED, row, cpu[t, h, off:off + n].tolist()):
                if code is None:
                    assert have in (127, 255), (val, have)
                else:
                    assert have == code, (val, have, code)
                    assert torch_code == code, (val, torch_code, code)      # the premise: torch's CPU cast agrees with the table
        other = torch.ones(nb * bs, dtype=torch.bool)
        other[slots] = False
        assert bool((got[other] == 0x55).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_appended_cache_equals_quantize_kv_cache_fp8(dtype):
    import torch
    import aule
    g = torch.Generator().manual_seed(5)
    nb, bs, Hkv, D = 9, 16, 4, 128
    cache = (torch.randn(nb, bs, Hkv, D, generator=g) * torch.tensor([0.01, 1.0, 7.0, 300.0]).view(1, 1, Hkv, 1)).to(torch_dtype(dtype))
    want_k, ks = aule.quantize_kv_cache_fp8(cache)
    want_v, vs = aule.quantize_kv_cache_fp8(cache.flip(0), per_head=False)
    kc = torch.zeros(nb, bs, Hkv, D, dtype=torch.uint8).view(torch.float8_e4m3fn).cuda()
    vc = kc.clone()
    rows = cache.view(nb * bs, Hkv, D)
    perm = torch.randperm(nb * bs, generator=g)              # token order is not slot order
    slots = torch.arange(nb * bs)[perm]
    aule.paged_kv_append(rows[perm].cuda(), cache.flip(0).reshape(nb * bs, Hkv, D)[perm].cuda(), kc, vc, slots.cuda(),
                         k_scale=ks, v_scale=vs)
    assert torch.equal(_bits(kc).cpu(), _bits(want_k))
    assert torch.equal(_bits(vc).cpu(), _bits(want_v))


# ---- 3. strides -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_inputs_equal_the_contiguous_call(dtype, cache_dtype):
    import torch
    import aule
    g = torch.Generator().manual_seed(31)
    H, D, nb, bs = 4, 64, 6, 16
    T = 41

    def caches():
        gg = torch.Generator().manual_seed(32)
        c = _random_cache(torch, gg, (nb, bs, H, D), "fp8" if cache_dtype == "fp8" else dtype)
        return c.cuda(), c.clone().cuda()
    kw = dict(k_scale=torch.linspace(0.5, 2.0, H), v_scale=0.25) if cache_dtype == "fp8" else {}
    slots = _slots(g, torch, T, nb * bs).cuda()
    # K and V as slices of one fused projection buffer [T, 3, H, D]
    qkv = _rand16(torch, g, (T, 3, H, D), dtype, 3.0).cuda()
    k, v = qkv[:, 1], qkv[:, 2]
    assert not k.is_contiguous() and k.stride() == (3 * H * D, D, 1)
    a_k, a_v = caches()
    aule.paged_kv_append(k, v, a_k, a_v, slots, **kw)
    b_k, b_v = caches()
    aule.paged_kv_append(k.contiguous(), v.contiguous(), b_k, b_v, slots, **kw)
    assert torch.equal(_bits(a_k), _bits(b_k)) and torch.equal(_bits(a_v), _bits(b_v))
    assert not torch.equal(_bits(a_k), _bits(caches()[0]))
    # a [B, Hkv, S, D] prefill tensor through the transposed view of one batch element; K and V with different strides
    B, S = 3, T
    kb = _rand16(torch, g, (B, H, S, D), dtype, 3.0).cuda()
    vb = _rand16(torch, g, (B, H, S + 5, D), dtype, 3.0).cuda()
    k, v = kb[1].transpose(0, 1), vb[2, :, 2:2 + S].transpose(0, 1)
    assert k.stride() == (D, S * D, 1) and v.stride() == (D, (S + 5) * D, 1)
    a_k, a_v = caches()
    aule.paged_kv_append(k, v, a_k, a_v, slots, **kw)
    b_k, b_v = caches()
    aule.paged_kv_append(k.contiguous(), v.contiguous(), b_k, b_v, slots, **kw)
    assert torch.equal(_bits(a_k), _bits(b_k)) and torch.equal(_bits(a_v), _bits(b_v))
    # and the contiguous call is right (16-bit: the rows themselves)
    if cache_dtype == "same":
        assert torch.equal(_bits(a_k).view(-1, H, D)[slots], _bits(k.contiguous()))
        assert torch.equal(_bits(a_v).view(-1, H, D)[slots], _bits(v.contiguous()))


# ---- 4. skipped slots -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
def test_skipped_slots_write_nothing(cache_dtype):
    """Each cache is a view into the middle of a larger tensor of canaries: a write through a bad slot would land in memory
    this test owns (the margins hold more rows than any slot offset used here) and fail it."""
    import torch
    import aule
    g = torch.Generator().manual_seed(41)
    nb, bs, Hkv, D, dtype = 4, 8, 2, 64, "bf16"
    n = nb * bs * Hkv * D
    row = Hkv * D
    margin = 2048 * row                                        # elements on each side: slots down to -2048, up to +2048
    tdt, canary = (torch.uint8, 0xA5) if cache_dtype == "fp8" else (torch.int16, 0x5A5A)

    def big():
        return torch.full((margin + n + margin,), canary, dtype=tdt, device="cuda")
    kbig, vbig = big(), big()
    view = lambda b: b[margin:margin + n].view(nb, bs, Hkv, D).view(torch.float8_e4m3fn if cache_dtype == "fp8" else torch.bfloat16)  # noqa: E731
    kc, vc = view(kbig), view(vbig)
    assert kc.is_contiguous() and kc.data_ptr() % 16 == 0
    ns = nb * bs
    slots = torch.tensor([3, -1, ns - 1, -7, ns, ns + 1, 0, ns + 5, ns + 1000, -2048, 17, -ns], dtype=torch.int64)
    T = slots.numel()
    k, v = _rand16(torch, g, (T, Hkv, D), dtype, 2.0), _rand16(torch, g, (T, Hkv, D), dtype, 2.0)
    kw = dict(k_scale=0.5, v_scale=2.0) if cache_dtype == "fp8" else {}
    aule.paged_kv_append(k.cuda(), v.cuda(), kc, vc, slots.cuda(), **kw)
    torch.cuda.synchronize()
    valid = (slots >= 0) & (slots < ns)
    assert valid.tolist() == [True, False, True, False, False, False, True, False, False, False, True, False]
    for bigt, src, s in ((kbig, k, 0.5), (vbig, v, 2.0)):
        host = bigt.cpu()
        assert bool((host[:margin] == canary).all()) and bool((host[margin + n:] == canary).all())
        inner = host[margin:margin + n].view(ns, Hkv, D)
        rows = _ref_codes(torch, src, torch.full((Hkv,), s)) if cache_dtype == "fp8" else _bits(src)
        assert torch.equal(inner[slots[valid]], rows[valid])
        untouched = torch.ones(ns, dtype=torch.bool)
        untouched[slots[valid]] = False
        assert bool((inner[untouched] == canary).all())
    # every slot skipped, with the rotation on and positions that are garbage: nothing is read from the table, nothing written
    cos, sin = torch.ones(4, D // 2, device="cuda"), torch.zeros(4, D // 2, device="cuda")
    k_before, v_before = kbig.cpu(), vbig.cpu()
    bad = torch.full((T,), -1, dtype=torch.int64)
    aule.paged_kv_append(k.cuda(), v.cuda(), kc, vc, bad.cuda(), cos=cos, sin=sin, positions=torch.full((T,), 2 ** 50, dtype=torch.int64), **kw)
    torch.cuda.synchronize()
    assert torch.equal(kbig.cpu(), k_before) and torch.equal(vbig.cpu(), v_before)


# ---- 5. fused RoPE --------------------------------------------------------------------------------------------------

ROPE_TOL = {"fp16": 2e-3, "bf16": 1.6e-2}      # tests/test_gpu_rope.py: one rounding to the I/O dtype


@pytest.mark.parametrize("D", HEAD_DIMS)
@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rope_is_the_rotation_pass_then_the_plain_append(dtype, cache_dtype, D, oracle_mod):
    import torch
    import aule
    from aule import _torch as at
    g = torch.Generator().manual_seed(51)
    Hkv, nb, bs, table_len = 2, 12, 16, 300
    # decode positions of 5 sequences, then a prefill chunk of 40 tokens that starts at position 131, then a skipped token
    positions = torch.cat([torch.tensor([17, 0, 255, 64, 299]), torch.arange(131, 171), torch.tensor([-9])]).to(torch.int64)
    T = positions.numel()
    slots = _slots(g, torch, T, nb * bs)
    slots[-1] = -1
    k, v = _rand16(torch, g, (T, Hkv, D), dtype, 2.0).cuda(), _rand16(torch, g, (T, Hkv, D), dtype, 2.0).cuda()
    cos_n, sin_n = oracle_mod.rope_tables(table_len, D)
    cos, sin = torch.from_numpy(cos_n).float().cuda(), torch.from_numpy(sin_n).float().cuda()
    kw = dict(k_scale=torch.tensor([0.7, 1.9]), v_scale=torch.tensor([1.0, 0.3])) if cache_dtype == "fp8" else {}

    def caches():
        c = _random_cache(torch, torch.Generator().manual_seed(52), (nb, bs, Hkv, D), "fp8" if cache_dtype == "fp8" else dtype)
        return c.cuda(), c.clone().cuda()
    f_k, f_v = caches()
    aule.paged_kv_append(k, v, f_k, f_v, slots.cuda(), cos=cos, sin=sin, positions=positions.to(torch.int32).cuda(), **kw)
    # the existing pass on the gathered table rows (token t -> row t of the gathered tables), then the un-fused append
    live = positions.clamp(min=0)
    kr = at.rope_raw(k.transpose(0, 1)[None].contiguous(), cos[live.cuda()].contiguous(), sin[live.cuda()].contiguous(), "half")
    kr = kr[0].transpose(0, 1).contiguous()
    u_k, u_v = caches()
    aule.paged_kv_append(kr, v, u_k, u_v, slots.cuda(), **kw)
    assert torch.equal(_bits(f_k), _bits(u_k)) and torch.equal(_bits(f_v), _bits(u_v))
    ok = slots >= 0
    # V is never rotated; the un-fused append of (1) / (2) is itself right
    s_v = kw.get("v_scale", None)
    want_v = _ref_codes(torch, v.cpu(), s_v) if cache_dtype == "fp8" else _bits(v.cpu())
    assert torch.equal(_bits(f_v).cpu().view(-1, Hkv, D)[slots[ok]], want_v[ok])
    assert torch.equal(_bits(f_k).cpu(), _expect(torch, caches()[0].cpu(), _ref_codes(torch, kr.cpu(), kw["k_scale"]) if cache_dtype == "fp8" else kr.cpu(), slots))
    # the rotated K against the fp64 oracle's rotation, with the rotation tests' own bound
    want = oracle_mod.rope_f64(k.float().cpu().numpy().transpose(1, 0, 2)[None], cos_n[live.numpy()], sin_n[live.numpy()], "half", False, 0)
    want = want[0].transpose(1, 0, 2)[ok.numpy()]
    tol = ROPE_TOL[dtype] * max(1.0, float(np.abs(want).max()))
    assert_close(kr.float().cpu().numpy()[ok.numpy()], want, tol, 0, "rotation pass")
    if cache_dtype == "same":
        got = f_k.view(-1, Hkv, D)[slots[ok].cuda()].float().cpu().numpy()
        print("max |rotated K - oracle| %.3g (bound %.3g)" % (np.abs(got - want).max(), tol))
        assert_close(got, want, tol, 0, "fused rotation in the cache")


# ---- 6. end to end --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
def test_prefill_then_decode_steps_through_shuffled_block_tables(cache_dtype, oracle_mod):
    """Prefill append of n tokens per sequence, then m single-token appends, slots from aule.paged_slot_mapping; after every
    decode step the paged decode over the appended cache equals, bit for bit, the same call over a cache filled by torch
    indexing (FP8: with the CPU formula's codes).  The FP8 result also stays within tests/test_gpu_paged_fp8.py's bound of
    the fp64 oracle on the dequantised cache."""
    import torch
    import aule
    g = torch.Generator().manual_seed(61)
    dtype, B, Hq, Hkv, D, bs, m = "bf16", 3, 8, 2, 128, 16, 5
    n = [70, 16, 33]
    max_blocks = (max(n) + m + bs - 1) // bs + 1
    nb = B * max_blocks + 3
    bt = torch.randperm(nb, generator=g)[:B * max_blocks].view(B, max_blocks).to(torch.int32)
    fp8 = cache_dtype == "fp8"
    ks, vs = (torch.tensor([0.011, 0.02]), torch.tensor([0.009, 0.03])) if fp8 else (None, None)
    kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    cdt = torch.float8_e4m3fn if fp8 else torch_dtype(dtype)
    zero = lambda: torch.zeros(nb, bs, Hkv, D, dtype=torch.uint8 if fp8 else torch_dtype(dtype)).view(cdt)  # noqa: E731
    a_k, a_v = zero().cuda(), zero().cuda()          # filled by the append
    r_k, r_v = zero(), zero()                        # filled by torch indexing on the CPU

    def put_ref(k, v, slots):
        ok = slots >= 0
        rk = _ref_codes(torch, k, ks) if fp8 else _bits(k)
        rv = _ref_codes(torch, v, vs) if fp8 else _bits(v)
        _bits(r_k).view(-1, Hkv, D)[slots[ok]] = rk[ok]
        _bits(r_v).view(-1, Hkv, D)[slots[ok]] = rv[ok]

    # prefill: every sequence's tokens in one call, taken from [B, Hkv, S, D] tensors without a copy where a sequence is alone
    seq = torch.cat([torch.full((x,), b) for b, x in enumerate(n)])
    pos = torch.cat([torch.arange(x) for x in n])
    slots = aule.paged_slot_mapping(bt, pos, bs, seq_ids=seq)
    k, v = _rand16(torch, g, (sum(n), Hkv, D), dtype), _rand16(torch, g, (sum(n), Hkv, D), dtype)
    aule.paged_kv_append(k.cuda(), v.cuda(), a_k, a_v, slots.cuda(), **kw)
    put_ref(k, v, slots)
    lens = torch.tensor(n, dtype=torch.int32)
    btc = bt.cuda()
    for step in range(m):
        k, v = _rand16(torch, g, (B, Hkv, D), dtype), _rand16(torch, g, (B, Hkv, D), dtype)
        slots = aule.paged_slot_mapping(btc, lens.cuda(), bs)          # on the device: no host round trip
        aule.paged_kv_append(k.cuda(), v.cuda(), a_k, a_v, slots, **kw)
        put_ref(k, v, slots.cpu())
        lens = lens + 1
        q = _rand16(torch, g, (B, Hq, D), dtype).cuda()
        got = aule.flash_attention_paged_amd(q, a_k, a_v, btc, lens.cuda(), **kw)
        ref = aule.flash_attention_paged_amd(q, r_k.cuda(), r_v.cuda(), btc, lens.cuda(), **kw)
        assert torch.equal(got, ref), step
    assert torch.equal(_bits(a_k).cpu(), _bits(r_k)) and torch.equal(_bits(a_v).cpu(), _bits(r_v))
    if fp8:
        K = r_k.float().double().numpy() * ks.double().numpy().reshape(1, 1, -1, 1)
        V = r_v.float().double().numpy() * vs.double().numpy().reshape(1, 1, -1, 1)
        want = oracle_mod.paged_decode_f64(q.float().cpu().numpy(), K, V, bt.numpy(), lens.numpy(), None, -1)
        atol, rtol = fwd_tol(dtype, float(np.abs(V).max()))
        print("fp8 end to end: max err %.3g (atol %.3g)" % (np.abs(got.float().cpu().numpy() - want).max(), atol))
        assert_close(got.float().cpu().numpy(), want, atol, rtol, "fp8 decode over the appended cache")


# ---- 7. graph capture -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
def test_append_and_decode_capture_replays_bit_identical(cache_dtype):
    """append (with the rotation) + paged decode captured once on one stream; three steps replayed after writing new values
    into the captured slot_mapping, positions, context_lens and input tensors in place; outputs and caches equal the eager
    run's bit for bit."""
    import torch
    import aule
    g = torch.Generator().manual_seed(71)
    dtype, B, Hq, Hkv, D, bs, steps = "fp16", 4, 16, 4, 128, 16, 3
    start = [100, 15, 31, 64]
    max_blocks = 8
    nb = B * max_blocks
    bt = torch.randperm(nb, generator=g).view(B, max_blocks).to(torch.int32).cuda()
    fp8 = cache_dtype == "fp8"
    kw = dict(k_scale=torch.linspace(0.02, 0.05, Hkv).cuda(), v_scale=torch.linspace(0.04, 0.01, Hkv).cuda()) if fp8 else {}
    cos, sin = aule.precompute_rope_frequencies(256, D, device="cuda")
    cos, sin = cos.contiguous(), sin.contiguous()
    base = _random_cache(torch, g, (nb, bs, Hkv, D), "fp8") if fp8 else _rand16(torch, g, (nb, bs, Hkv, D), dtype)
    if fp8:   # finite codes only: the decode reads the whole context
        base = (_bits(base) & 0x77).view(torch.float8_e4m3fn)
    ins = [tuple(_rand16(torch, g, s, dtype).cuda() for s in ((B, Hkv, D), (B, Hkv, D), (B, Hq, D))) for _ in range(steps)]
    # static tensors of the captured step
    k_in, v_in, q_in = (torch.empty_like(x) for x in ins[0])
    slot_in = torch.empty(B, dtype=torch.int64, device="cuda")
    pos_in = torch.empty(B, dtype=torch.int64, device="cuda")
    len_in = torch.empty(B, dtype=torch.int32, device="cuda")

    def set_step(i):
        pos = torch.tensor(start) + i
        k_in.copy_(ins[i][0]); v_in.copy_(ins[i][1]); q_in.copy_(ins[i][2])
        pos_in.copy_(pos)
        slot_in.copy_(aule.paged_slot_mapping(bt, pos.cuda(), bs))
        len_in.copy_((pos + 1).to(torch.int32))

    def run(kc, vc):
        aule.paged_kv_append(k_in, v_in, kc, vc, slot_in, cos=cos, sin=sin, positions=pos_in, **kw)
        return aule.flash_attention_paged_amd(q_in, kc, vc, bt, len_in, **kw)

    e_k, e_v = base.clone().cuda(), base.clone().cuda()
    eager = []
    for i in range(steps):
        set_step(i)
        eager.append(run(e_k, e_v).clone())
    torch.cuda.synchronize()
    c_k, c_v = base.clone().cuda(), base.clone().cuda()
    set_step(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run(c_k, c_v)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(c_k, c_v)
    for i in range(steps):
        set_step(i)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[i]), i
    assert torch.equal(_bits(c_k), _bits(e_k)) and torch.equal(_bits(c_v), _bits(e_v))
    assert not torch.equal(_bits(c_k).cpu(), _bits(base))


# ---- 8. large caches ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cache_dtype", ["same", "fp8"])
def test_cache_offsets_beyond_2_gib(cache_dtype):
    """One K and one V cache of more than 2 GiB each with the highest slots written (byte offsets past 2^31, for the 16-bit
    cache element offsets past 2^30 as well); only those slots and their neighbours are read back."""
    import torch
    import aule
    g = torch.Generator().manual_seed(81)
    dtype, Hkv, D, bs = "bf16", 8, 128, 16
    esz = 1 if cache_dtype == "fp8" else 2
    blk_bytes = bs * Hkv * D * esz
    tail = 4                                                       # blocks read back
    nb = (2 ** 31) // blk_bytes + tail + 4
    cdt = torch.float8_e4m3fn if cache_dtype == "fp8" else torch.bfloat16
    kc = torch.empty(nb, bs, Hkv, D, dtype=torch.uint8 if esz == 1 else torch.int16, device="cuda").view(cdt)
    vc = torch.empty_like(kc)
    assert kc.numel() * esz > 2 ** 31 and (nb - tail) * blk_bytes > 2 ** 31
    canary = 0x33 if esz == 1 else 0x3333
    _bits(kc)[-tail:] = canary
    _bits(vc)[-tail:] = canary
    ns = nb * bs
    # the last block whole, a few slots of the one before, and one slot past the end
    slots = torch.cat([torch.arange(ns - bs, ns), torch.tensor([ns - bs - 1, ns - 2 * bs + 3, ns])]).to(torch.int64)
    slots = slots[torch.randperm(slots.numel(), generator=g)]
    T = slots.numel()
    k, v = _rand16(torch, g, (T, Hkv, D), dtype, 2.0), _rand16(torch, g, (T, Hkv, D), dtype, 2.0)
    kw = dict(k_scale=torch.linspace(0.5, 1.5, Hkv), v_scale=0.75) if cache_dtype == "fp8" else {}
    aule.paged_kv_append(k.cuda(), v.cuda(), kc, vc, slots.cuda(), **kw)
    torch.cuda.synchronize()
    first = (nb - tail) * bs
    for cache, src, s in ((kc, k, kw.get("k_scale")), (vc, v, torch.full((Hkv,), 0.75))):
        got = _bits(cache)[-tail:].cpu().view(tail * bs, Hkv, D)
        rows = _ref_codes(torch, src, s) if cache_dtype == "fp8" else _bits(src)
        want = torch.full_like(got, canary)
        ok = slots < ns
        want[slots[ok] - first] = rows[ok]
        assert torch.equal(got, want)


# ---- 9. the C-ABI directly ------------------------------------------------------------------------------------------

def _desc(torch, k, v, kc, vc, slots, ks=None, vs=None, cos=None, sin=None, pos=None):
    from aule import _capi
    d = _capi.KvAppendDesc()
    d.struct_size = ctypes.sizeof(_capi.KvAppendDesc)
    d.dtype = {torch.float16: 1, torch.bfloat16: 2}[k.dtype]
    d.cache_dtype = 1 if kc.dtype == torch.float8_e4m3fn else 0
    d.num_tokens, d.heads_kv, d.head_dim = k.shape
    d.num_blocks, d.block_size = kc.shape[0], kc.shape[1]
    d.key_token_stride, d.key_head_stride = k.stride(0), k.stride(1)
    d.value_token_stride, d.value_head_stride = v.stride(0), v.stride(1)
    d.device = k.device.index or 0
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.key, d.value, d.k_cache, d.v_cache, d.slot_mapping = k.data_ptr(), v.data_ptr(), kc.data_ptr(), vc.data_ptr(), slots.data_ptr()
    if ks is not None:
        d.k_scale, d.v_scale = ks.data_ptr(), vs.data_ptr()
    if cos is not None:
        d.cos, d.sin, d.positions = cos.data_ptr(), sin.data_ptr(), pos.data_ptr()
        d.table_len, d.table_pitch = cos.shape[0], cos.stride(0)
    return d


def test_c_abi_directly():
    """aule_kv_cache_append_ex through ctypes with raw pointers on the current stream: an FP8 append with rotation from a
    table with a row pitch, num_tokens = 0, and -3 plus an error text for every kind of bad descriptor."""
    import torch
    from aule import _capi
    from aule import _torch as at
    import test_kv_append_host as host
    lib = _capi.get_lib()
    g = torch.Generator().manual_seed(91)
    T, Hkv, D, nb, bs = 19, 4, 64, 5, 8
    k, v = _rand16(torch, g, (T, Hkv, D), "fp16", 2.0).cuda(), _rand16(torch, g, (T, Hkv, D), "fp16", 2.0).cuda()
    slots = _slots(g, torch, T, nb * bs).cuda()
    ks, vs = torch.linspace(0.3, 0.9, Hkv).cuda(), torch.linspace(1.2, 0.4, Hkv).cuda()
    wide = torch.randn(64, 2, D // 2 + 4, generator=g).cuda()       # tables with a pitch of D/2 + 4 floats
    cos, sin = wide[:, 0, :D // 2], wide[:, 1, :D // 2]
    pos = torch.randint(0, 64, (T,), generator=g).cuda()
    kc = torch.zeros(nb, bs, Hkv, D, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn)
    vc = kc.clone()
    d = _desc(torch, k, v, kc, vc, slots, ks, vs, cos, sin, pos)
    assert d.table_pitch == 2 * (D // 2 + 4)
    assert lib.aule_kv_cache_append_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    kr = at.rope_raw(k.transpose(0, 1)[None].contiguous(), cos[pos].contiguous(), sin[pos].contiguous(), "half")[0].transpose(0, 1)
    zero = torch.zeros(nb, bs, Hkv, D, dtype=torch.uint8).view(torch.float8_e4m3fn)
    assert torch.equal(_bits(kc).cpu(), _expect(torch, zero, _ref_codes(torch, kr.cpu(), ks.cpu()), slots.cpu()))
    assert torch.equal(_bits(vc).cpu(), _expect(torch, zero, _ref_codes(torch, v.cpu(), vs.cpu()), slots.cpu()))
    # num_tokens == 0: fine, no launch, pointers not needed
    before = _bits(kc).clone()
    d0 = _desc(torch, k, v, kc, vc, slots, ks, vs)
    d0.num_tokens = 0
    d0.key = d0.value = d0.slot_mapping = None
    assert lib.aule_kv_cache_append_ex(ctypes.byref(d0)) == 0
    # every bad descriptor of the host test's list, on a descriptor that is otherwise this (valid, 16-bit) call
    k16, v16 = torch.zeros(nb, bs, Hkv, D, dtype=torch.float16, device="cuda"), torch.zeros(nb, bs, Hkv, D, dtype=torch.float16, device="cuda")
    assert lib.aule_kv_cache_append_ex(None) == -3
    for field, bad in host.BAD_FIELDS:
        dd = _desc(torch, k, v, k16, v16, slots)
        if isinstance(bad, int) and bad >= 0x1000:        # the made-up pointers of the host list: real memory here
            bad = ks.data_ptr() + (bad & 0xF)
        setattr(dd, field, bad)
        assert lib.aule_kv_cache_append_ex(ctypes.byref(dd)) == -3, (field, bad)
        assert b"KV cache append failed" in lib.aule_get_error(), field
    dd = _desc(torch, k, v, kc, vc, slots, ks, vs)
    dd.v_scale = None                                      # FP8 without a scale array
    assert lib.aule_kv_cache_append_ex(ctypes.byref(dd)) == -3 and b"scale pointer" in lib.aule_get_error()
    dd = _desc(torch, k, v, kc, vc, slots, ks, vs, cos, sin, pos)
    dd.table_pitch = D // 2 + 2                            # rows that are not 16-byte multiples
    assert lib.aule_kv_cache_append_ex(ctypes.byref(dd)) == -3 and b"table_pitch" in lib.aule_get_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(kc), before) and not bool(k16.any()) and not bool(v16.any())
