"""The latent cache append of the paged MLA on the GPU (csrc/mla_kv_append_gfx950.hip behind aule.mla_kv_append /
aule_mla_kv_append_ex): row slot_mapping[t] of the [num_blocks * block_size, 576] cache <- [c_kv[t] | rope(k_pe[t])].

The expected values come from torch on the CPU -- row copies for a 16-bit cache, (x.float() / s).clamp(-448, 448).to(float8_e4m3fn)
for an FP8 one, compared as integers with no tolerance -- and from the existing, oracle-pinned rotation pass (aule._torch.rope_raw on
the gathered table rows), never from the call under test.  Caches start from random bits, so a stray write fails the test.  The last
tests run the serving step end to end: append, then flash_attention_mla_paged_fp8 over the cache it wrote, eagerly and as a graph."""
import ctypes

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from util import torch_dtype

pytestmark = pytest.mark.gpu

DTYPES = ["fp16", "bf16"]
LAYOUTS = ["half", "interleaved"]
C, R, W = 512, 64, 576


def _rand16(torch, g, shape, dtype, mag=1.0):
    return (torch.randn(*shape, generator=g) * mag).to(torch_dtype(dtype))


def _random_cache(torch, g, nb, bs, kind):
    """random BITS of the cache's type (NaN patterns included: comparisons are on integers); kind "fp8" or a 16-bit dtype name"""
    if kind == "fp8":
        return torch.randint(0, 256, (nb, bs, W), generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn)
    return torch.randint(-2 ** 15, 2 ** 15, (nb, bs, W), generator=g, dtype=torch.int16).view(torch_dtype(kind))


def _bits(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.uint8)


def _ref_codes(torch, rows, s):
    """the issue's formula on the CPU: rows [T, 576] 16-bit, s one fp32 value -> uint8 codes (division, then clamp, then cast)"""
    s = torch.as_tensor(s, dtype=torch.float32).reshape(())
    return (rows.float() / s).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)


def _expect(torch, cache0, rows_bits, slots, skip=None):
    """cache0's bits with rows_bits [T, 576] written at the valid slots of the tokens that are not skipped (CPU, integer views)"""
    want = _bits(cache0).clone()
    flat = want.view(-1, W)
    ok = (slots >= 0) & (slots < flat.shape[0])
    if skip is not None:
        ok &= ~skip
    flat[slots[ok]] = rows_bits[ok]
    return want


def _rotated(torch, k_pe, cos, sin, positions, layout):
    """rope_raw (the rotation pass, pinned against the oracle by its own tests) on k_pe [T, 64] with the table rows positions[t]
    gathered; a position outside the table (such a token is skipped) takes row 0.  Returns a CPU tensor."""
    from aule._torch import rope_raw
    p = positions.clone()
    p[(p < 0) | (p >= cos.shape[0])] = 0
    x = k_pe.contiguous().view(1, 1, -1, R).cuda()
    return rope_raw(x, cos[p].contiguous().cuda(), sin[p].contiguous().cuda(), layout=layout).view(-1, R).cpu()


def _tables(torch, g, n):
    ang = torch.rand(n, R // 2, generator=g) * 6.2831853
    return torch.cos(ang), torch.sin(ang)


# ---- 1. 16-bit cache ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_16_bit_cache_rows_are_bit_copies_and_the_rest_is_untouched(dtype):
    """T = 37 tokens (68 threads each: ten workgroups, the last one part full), block sizes that are and are not a power of two,
    one token, and the [T, 1, 64] / 4-d spellings"""
    import torch
    import aule
    g = torch.Generator().manual_seed(100)
    for bs, T in ((16, 37), (24, 37), (16, 1)):
        nb = 7
        c, r = _rand16(torch, g, (T, C), dtype), _rand16(torch, g, (T, R), dtype)
        cache0 = _random_cache(torch, g, nb, bs, dtype)
        slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.int64)
        want = _expect(torch, cache0, _bits(torch.cat([c, r], 1)), slots)
        cache = cache0.cuda()
        assert aule.mla_kv_append(c.cuda(), r.cuda(), cache, slots.cuda()) is None
        assert torch.equal(_bits(cache).cpu(), want), (dtype, bs, T)
        cache = cache0.cuda().view(nb, bs, 1, W)
        aule.mla_kv_append(c.cuda(), r.cuda().view(T, 1, R), cache, slots.to(torch.int32).cuda())
        assert torch.equal(_bits(cache).cpu().view(nb, bs, W), want), (dtype, bs, T)


# ---- 2. FP8 cache ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_codes_equal_the_cpu_formula(dtype):
    """the scale of quantize_mla_cache_fp8 (amax / 448: the largest value lands on +-448 exactly), given as a device tensor, a CPU
    0-d tensor and a float; and a scale of 1.0 (None) on data that exceeds 448 (saturation)"""
    import torch
    import aule
    g = torch.Generator().manual_seed(200)
    nb, bs, T = 5, 16, 29
    for mode in ("device", "cpu0d", "float", "none"):
        mag = 300.0 if mode == "none" else 1.0
        c, r = _rand16(torch, g, (T, C), dtype, mag), _rand16(torch, g, (T, R), dtype, mag)
        rows = torch.cat([c, r], 1)
        _, s = aule.quantize_mla_cache_fp8(rows.view(1, T, W))
        assert float(s) != 1.0
        if mode == "none":
            s = torch.ones(1)
            assert float(rows.float().abs().max()) > 448
        ks = {"device": s.cuda(), "cpu0d": s.reshape(()), "float": float(s), "none": None}[mode]
        cache0 = _random_cache(torch, g, nb, bs, "fp8")
        slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.int64)
        codes = _ref_codes(torch, rows, s)
        assert not bool(((codes & 0x7F) == 0x7F).any()) and int((codes & 0x7F).max()) == 126
        cache = cache0.cuda()
        aule.mla_kv_append(c.cuda(), r.cuda(), cache, slots.cuda(), kv_scale=ks)
        assert torch.equal(_bits(cache).cpu(), _expect(torch, cache0, codes, slots)), (dtype, mode)


PLANTED = [  # (input, expected e4m3fn code with scale 1.0): round to nearest even, saturation, -0, subnormals, NaN
    (0.0, 0), (-0.0, 128), (1.0, 56), (448.0, 126), (-448.0, 254), (464.0, 126), (-464.0, 254), (480.0, 126), (32768.0, 126), (float("inf"), 126),
    (float("-inf"), 254), (2.0 ** -9, 1), (-(2.0 ** -9), 129), (2.0 ** -10, 0), (2.0 ** -11, 0), (1.5 * 2.0 ** -10, 1), (3 * 2.0 ** -9, 3),
    (7 * 2.0 ** -9, 7), (2.0 ** -6, 8), (float("nan"), None),
]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fp8_planted_values(dtype):
    """planted values in c_kv (at a chunk's start and across chunks) and in both halves of k_pe, scale 1.0, against the table and
    against torch's cast on the CPU wherever that is not NaN"""
    import torch
    import aule
    T, nb, bs = 3, 2, 4
    vals = torch.tensor([p[0] for p in PLANTED], dtype=torch.float32)
    n = len(PLANTED)
    assert n <= R // 2
    c, r = torch.zeros(T, C), torch.zeros(T, R)
    c[0, :n], c[1, 501 - n:501], r[1, :n], r[2, R - n:] = vals, vals, vals, vals
    where = [(0, 0), (1, 501 - n), (1, C), (2, W - n)]
    c, r = c.to(torch_dtype(dtype)), r.to(torch_dtype(dtype))
    assert torch.equal(c[0, :n].float().nan_to_num(7.0), vals.nan_to_num(7.0))   # every planted value is exact in both dtypes
    slots = torch.tensor([5, 0, 6], dtype=torch.int64)
    cache = torch.zeros(nb, bs, W, dtype=torch.uint8).view(torch.float8_e4m3fn).cuda()
    aule.mla_kv_append(c.cuda(), r.cuda(), cache, slots.cuda(), kv_scale=1.0)
    got = cache.view(torch.uint8).cpu().view(-1, W)
    want = _ref_codes(torch, torch.cat([c, r], 1), 1.0)
    for t, at in where:
        for i, (x, code) in enumerate(PLANTED):
            g_ = int(got[slots[t], at + i])
            if code is None:
                assert g_ & 0x7F == 0x7F, (dtype, t, x, g_)
            else:
                assert g_ == code == int(want[t, at + i]), (dtype, t, x, g_, code, int(want[t, at + i]))
    nan = torch.isnan(torch.cat([c, r], 1).float())
    assert torch.equal(got[slots][~nan], want[~nan])


# ---- 3. fused rotation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["same", "fp8"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_rotation_equals_the_rotation_pass_then_the_plain_rows(dtype, layout, kind):
    import torch
    import aule
    g = torch.Generator().manual_seed(300)
    nb, bs, T, table_len = 6, 16, 41, 50
    c, r = _rand16(torch, g, (T, C), dtype), _rand16(torch, g, (T, R), dtype)
    cos, sin = _tables(torch, g, table_len)
    pos = torch.randint(0, table_len, (T,), generator=g)
    pos[0], pos[1] = 0, table_len - 1
    rows = torch.cat([c, _rotated(torch, r, cos, sin, pos, layout)], 1)
    assert not torch.equal(_bits(rows[:, C:]), _bits(r))
    slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.int64)
    cache0 = _random_cache(torch, g, nb, bs, dtype if kind == "same" else "fp8")
    kw = {}
    if kind == "fp8":
        _, s = aule.quantize_mla_cache_fp8(rows.view(1, T, W))
        kw["kv_scale"] = s.cuda()
        rows_bits = _ref_codes(torch, rows, s)
    else:
        rows_bits = _bits(rows)
    cache = cache0.cuda()
    aule.mla_kv_append(c.cuda(), r.cuda(), cache, slots.cuda(), cos=cos.cuda(), sin=sin, positions=pos.cuda(), rope_layout=layout, **kw)
    assert torch.equal(_bits(cache).cpu(), _expect(torch, cache0, rows_bits, slots)), (dtype, layout, kind)
    # the other layout gives other bits (the layouts are not confused)
    other = torch.cat([c, _rotated(torch, r, cos, sin, pos, LAYOUTS[1 - LAYOUTS.index(layout)])], 1)
    assert not torch.equal(_bits(other), _bits(rows))


# ---- 4. skips and strides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["same", "fp8"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_skipped_tokens_write_nothing_and_strided_inputs_equal_contiguous_ones(dtype, kind):
    """slots -1, just past the cache, far past it and hugely negative; positions -1 and table_len: NOTHING of such a token's row is
    written (its c_kv part included); inputs that are slices of one wider tensor give the contiguous call's bits"""
    import torch
    import aule
    g = torch.Generator().manual_seed(400)
    nb, bs, T, table_len = 4, 16, 23, 30
    fused = _rand16(torch, g, (T, C + R + 24), dtype)
    c, r = fused[:, :C], fused[:, C + 8:C + 8 + R]
    assert c.stride(0) == r.stride(0) == C + R + 24 and not c.is_contiguous()
    cos, sin = _tables(torch, g, table_len)
    pos = torch.randint(0, table_len, (T,), generator=g)
    slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.int64)
    slots[2], slots[5], slots[7], slots[11] = -1, nb * bs, nb * bs + 12345, -2 ** 40
    pos[3], pos[9], pos[2] = -1, table_len, table_len + 7          # (token 2: a skipped slot needs no valid position)
    skip = (pos < 0) | (pos >= table_len)
    kw = dict(kv_scale=torch.tensor(0.03125)) if kind == "fp8" else {}
    cache0 = _random_cache(torch, g, nb, bs, dtype if kind == "same" else "fp8")
    for layout in LAYOUTS:
        rows = torch.cat([c, _rotated(torch, r, cos, sin, pos, layout)], 1)
        rows_bits = _ref_codes(torch, rows, 0.03125) if kind == "fp8" else _bits(rows)
        want = _expect(torch, cache0, rows_bits, slots, skip)
        fused_d = fused.cuda()
        cache = cache0.cuda()
        aule.mla_kv_append(fused_d[:, :C], fused_d[:, C + 8:C + 8 + R], cache, slots.cuda(), cos=cos, sin=sin, positions=pos, rope_layout=layout, **kw)
        assert torch.equal(_bits(cache).cpu(), want), (dtype, kind, layout, "strided")
        cache = cache0.cuda()
        aule.mla_kv_append(c.contiguous().cuda(), r.contiguous().cuda(), cache, slots.cuda(), cos=cos, sin=sin, positions=pos, rope_layout=layout, **kw)
        assert torch.equal(_bits(cache).cpu(), want), (dtype, kind, layout, "contiguous")
    # without rotation only the slots skip
    rows = torch.cat([c, r], 1)
    want = _expect(torch, cache0, _ref_codes(torch, rows, 0.03125) if kind == "fp8" else _bits(rows), slots)
    cache = cache0.cuda()
    fused_d = fused.cuda()
    aule.mla_kv_append(fused_d[:, :C], fused_d[:, C + 8:C + 8 + R], cache, slots.cuda(), **kw)
    assert torch.equal(_bits(cache).cpu(), want), (dtype, kind, "no rotation")
    # every token skipped: the cache keeps every bit
    cache = cache0.cuda()
    aule.mla_kv_append(fused_d[:, :C], fused_d[:, C + 8:C + 8 + R], cache, torch.full((T,), -1).cuda(), **kw)
    assert torch.equal(_bits(cache).cpu(), _bits(cache0))


# ---- 5. the C entry inside guard bands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout", [("same", 0), ("fp8", 1)])
def test_c_entry_inside_an_arena(kind, layout):
    """every tensor of the call between guard bands of one allocation, strided inputs and pitched tables: the guards stay intact, the
    inputs unchanged, the cache holds exactly the expected rows and its other bytes keep the poison"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    dtype = "bf16"
    g = torch.Generator().manual_seed(500 + layout)
    nb, bs, T, table_len, pitch, cs, rs = 3, 24, 19, 12, 36, C + 16, R + 8
    cw, rw = _rand16(torch, g, (T, cs), dtype), _rand16(torch, g, (T, rs), dtype)
    cos_w, sin_w = torch.zeros(table_len, pitch), torch.zeros(table_len, pitch)
    cos_w[:, :32], sin_w[:, :32] = _tables(torch, g, table_len)
    pos = torch.randint(0, table_len, (T,), generator=g)
    slots = torch.randperm(nb * bs, generator=g)[:T].to(torch.int64)
    slots[4], pos[6] = -1, table_len
    ks = torch.tensor([0.0625])
    esize = 1 if kind == "fp8" else 2
    host = dict(c=cw, r=rw, slots=slots, pos=pos, cos=cos_w, sin=sin_w, ks=ks)
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in host.items()] + [("cache", nb * bs * W * esize, "out")]
    arena = Arena(torch, regions, W * 2)
    kept = {k: arena.upload(k, v) for k, v in host.items()}
    arena.fill(POISON)
    d = _capi.MlaKvAppendDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.rope_layout = 2, 1 if kind == "fp8" else 0, layout
    d.total_tokens, d.num_blocks, d.block_size, d.table_len, d.table_pitch = T, nb, bs, table_len, pitch
    d.c_kv_token_stride, d.k_pe_token_stride = cs, rs
    d.device = torch.cuda.current_device()
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d.c_kv, d.k_pe, d.kv_cache, d.slot_mapping = arena.ptr("c"), arena.ptr("r"), arena.ptr("cache"), arena.ptr("slots")
    d.cos, d.sin, d.positions = arena.ptr("cos"), arena.ptr("sin"), arena.ptr("pos")
    if kind == "fp8":
        d.kv_scale = arena.ptr("ks")
    assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    assert arena.guards_intact(), arena.damage()
    for k, v in kept.items():
        assert arena.unchanged(k, v), k
    c, r = cw[:, :C], rw[:, :R]
    rows = torch.cat([c, _rotated(torch, r, cos_w[:, :32], sin_w[:, :32], pos, LAYOUTS[layout])], 1)
    if kind == "fp8":
        cache0 = torch.full((nb, bs, W), POISON, dtype=torch.uint8).view(torch.float8_e4m3fn)
        rows_bits = _ref_codes(torch, rows, ks)
    else:
        cache0 = torch.full((nb, bs, W), -1, dtype=torch.int16).view(torch.bfloat16)
        rows_bits = _bits(rows)
    want = _expect(torch, cache0, rows_bits, slots, (pos < 0) | (pos >= table_len))
    got = arena.view("cache", torch.uint8 if kind == "fp8" else torch.int16, (nb, bs, W)).cpu()
    assert torch.equal(got, want)
    # refusals with a device present: nothing is written
    arena.bytes("cache").fill_(POISON)
    d.k_pe_token_stride = 60
    assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == -3
    d.k_pe_token_stride, d.rope_layout = rs, 7
    assert lib.aule_mla_kv_append_ex(ctypes.byref(d)) == -3
    torch.cuda.synchronize()
    assert bool((arena.bytes("cache") == POISON).all())


# ---- 6. end to end: append + FP8 attention over shuffled block tables, eagerly and as a graph -----------------------------------------
class Serving:
    """Three sequences with a few cached tokens each and three more to come; one FP8 latent cache that starts as random bits (NaN
    codes included, in every slot that is never appended: the attention must not read them).  `ref`
    is the cache as torch fills it on the CPU with the formula (rotation: rope_raw on gathered table rows)."""

    def __init__(self, torch, dtype, layout, seed):
        g = torch.Generator().manual_seed(seed)
        self.torch, self.dtype, self.layout, self.bs, self.Hq = torch, dtype, layout, 16, 16
        self.lens, self.steps = [20, 5, 33], 3
        B = len(self.lens)
        need = [(n + self.steps + self.bs - 1) // self.bs for n in self.lens]
        nb = sum(need) + 2
        perm = torch.randperm(nb, generator=g)
        self.bt = torch.zeros(B, 16, dtype=torch.int32)   # 256 keys of capacity: the plan splits the keys in two
        at = 0
        for b in range(B):
            self.bt[b, :need[b]] = perm[at:at + need[b]].to(torch.int32)
            at += need[b]
        self.c = [_rand16(torch, g, (n + self.steps, C), dtype) for n in self.lens]
        self.r = [_rand16(torch, g, (n + self.steps, R), dtype) for n in self.lens]
        self.q = _rand16(torch, g, (self.steps, B, self.Hq, W), dtype)
        self.cos, self.sin = _tables(torch, g, 64)
        self.ks = torch.tensor([6.0 / 448])
        self.cache0 = _random_cache(torch, g, nb, self.bs, "fp8")
        self.ref = self.cache0.clone()

    def tokens(self, lo, hi):
        """(c_kv, k_pe, positions, sequence ids) of tokens lo(b) .. hi(b) - 1 of every sequence, packed"""
        torch = self.torch
        B = len(self.lens)
        pos = torch.cat([torch.arange(lo(b), hi(b)) for b in range(B)])
        seq = torch.cat([torch.full((hi(b) - lo(b),), b, dtype=torch.int64) for b in range(B)])
        c = torch.cat([self.c[b][lo(b):hi(b)] for b in range(B)])
        r = torch.cat([self.r[b][lo(b):hi(b)] for b in range(B)])
        return c, r, pos, seq

    def fill_ref(self, c, r, pos, slots):
        torch = self.torch
        rows = torch.cat([c, _rotated(torch, r, self.cos, self.sin, pos, self.layout)], 1)
        self.ref.view(torch.uint8).view(-1, W)[slots.cpu()] = _ref_codes(torch, rows, self.ks)


@pytest.mark.parametrize("mode", ["eager", "graph"])
@pytest.mark.parametrize("dtype,layout", [("bf16", "interleaved"), ("fp16", "half")])
def test_prefill_append_then_decode_steps(dtype, layout, mode):
    """prefill-append the cached tokens, then three decode steps of append + flash_attention_mla_paged_fp8: at every step the cache
    equals the one torch fills with the formula, and the attention result equals the call over THAT cache, bit for bit.  graph: the
    append and the attention of a step are captured once and replayed twice per step on inputs copied into static buffers."""
    import torch
    import aule
    s = Serving(torch, dtype, layout, 600)
    B = len(s.lens)
    bt, ks, cos, sin = s.bt.cuda(), s.ks.cuda(), s.cos.cuda(), s.sin.cuda()
    cache = s.cache0.cuda()
    scale = 192 ** -0.5
    # prefill
    c, r, pos, seq = s.tokens(lambda b: 0, lambda b: s.lens[b])
    slots = aule.paged_slot_mapping(bt, pos.cuda(), s.bs, seq.cuda())
    aule.mla_kv_append(c.cuda(), r.cuda(), cache, slots, kv_scale=ks, cos=cos, sin=sin, positions=pos.cuda(), rope_layout=layout)
    s.fill_ref(c, r, pos, slots)
    assert torch.equal(cache.view(torch.uint8).cpu(), s.ref.view(torch.uint8)), "prefill"
    assert not torch.equal(s.ref.view(torch.uint8), s.cache0.view(torch.uint8))

    # static inputs of a step
    c_in, r_in = torch.empty(B, C, device="cuda", dtype=torch_dtype(dtype)), torch.empty(B, R, device="cuda", dtype=torch_dtype(dtype))
    pos_in, slots_in = torch.zeros(B, device="cuda", dtype=torch.int64), torch.zeros(B, device="cuda", dtype=torch.int64)
    ctx_in, q_in = torch.zeros(B, device="cuda", dtype=torch.int32), torch.empty(B, s.Hq, W, device="cuda", dtype=torch_dtype(dtype))

    def step():
        aule.mla_kv_append(c_in, r_in, cache, slots_in, kv_scale=ks, cos=cos, sin=sin, positions=pos_in, rope_layout=layout)
        return aule.flash_attention_mla_paged_fp8(q_in, cache, bt, ctx_in, scale=scale, return_lse=True, kv_scale=ks)

    def load(i):
        c, r, pos, seq = s.tokens(lambda b: s.lens[b] + i, lambda b: s.lens[b] + i + 1)
        slots = aule.paged_slot_mapping(bt, pos.cuda(), s.bs)
        c_in.copy_(c); r_in.copy_(r); pos_in.copy_(pos); slots_in.copy_(slots); q_in.copy_(s.q[i])
        ctx_in.copy_((pos + 1).to(torch.int32))
        s.fill_ref(c, r, pos, slots)

    graph = None
    if mode == "graph":
        load(0)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()      # (writes step 0's rows: what the first replay writes again)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out, lse = step()
    seen = []
    for i in range(s.steps):
        if i > 0 or mode == "eager":
            load(i)
        if graph is None:
            out, lse = step()
        else:
            out.zero_(); lse.zero_()
            graph.replay()
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cache.view(torch.uint8).cpu(), s.ref.view(torch.uint8)), (mode, i)
        want, want_lse = aule.flash_attention_mla_paged_fp8(q_in, s.ref.cuda(), bt, ctx_in, scale=scale, return_lse=True, kv_scale=ks)
        assert same_bits(torch, out, want) and same_bits(torch, lse, want_lse), (mode, i)
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
        seen.append(out.clone())
    assert not same_bits(torch, seen[0], seen[1]) and not same_bits(torch, seen[1], seen[2])


def test_refusals_on_the_device():
    import torch
    import aule
    c, r = torch.zeros(4, C, dtype=torch.bfloat16, device="cuda"), torch.zeros(4, R, dtype=torch.bfloat16, device="cuda")
    cache = torch.zeros(2, 16, W, dtype=torch.bfloat16, device="cuda")
    slots = torch.arange(4, device="cuda")
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        aule.mla_kv_append(c.cpu(), r.cpu(), cache.cpu(), slots.cpu())
    with pytest.raises(ValueError, match="every tensor must live on"):
        aule.mla_kv_append(c, r, cache.cpu(), slots)
    with pytest.raises(ValueError, match="must be torch.float8_e4m3fn"):
        aule.mla_kv_append(c, r, cache.to(torch.float16), slots)
    with pytest.raises(ValueError, match="unknown rope_layout"):
        aule.mla_kv_append(c, r, cache, slots, rope_layout="gptj")
    assert aule.mla_kv_append(c[:0], r[:0], cache, slots[:0]) is None
    assert not bool(cache.any())
    assert np.array_equal(cache.float().cpu().numpy(), np.zeros((2, 16, W), dtype=np.float32))
