"""The paged MLA over an FP8 latent cache on the GPU (csrc/fa_fwd_mla_paged_fp8_gfx950.hip behind aule.flash_attention_mla_paged_fp8 /
aule_attention_mla_paged_fp8_ex): kv_cache [num_blocks, block_size, 576] e4m3fn codes and ONE scale, key = kv_scale * float(code row).

Three kinds of check, on the shapes of tests/test_gpu_mla.py (its Case makes the inputs: N(0, 1) latents, here quantised with
aule.quantize_mla_cache_fp8):
  exact    the kernel converts the codes exactly to q's dtype and then runs the 16-bit kernel's arithmetic, so with kv_scale = 1 the
           call equals flash_attention_mla_paged on codes.to(q.dtype) bit for bit, and with kv_scale = 2^-3 it equals 2^-3 times
           that call with scale * 2^-3 (a power of two commutes with every rounding as long as nothing is subnormal: asserted);
  parity   for the scale quantize_mla_cache_fp8 gives, against the fp64 decode oracle on the dequantised cache, with the project's
           bounds: fwd_tol(dtype, max |dequantised V|) and 1e-3 for lse.  The maxima are printed;
  memory   NaN codes in every slot that is no live key change no bit; rows of no sequence keep their bytes; hostile offsets and an
           arena with guard bands."""
import ctypes
import math

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from test_gpu_mla import DECODE, DTYPE_CODE, QK, VD, Case, _desc, _judge, _nsplit, _poisoned
from util import torch_dtype

pytestmark = pytest.mark.gpu

NAN_CODE = 0x7F


class Fp8Case(Case):
    """A Case whose latent cache is quantised: `codes` (float8_e4m3fn, CPU) and `kv_scale` ([1] fp32, CPU) are what the device sees;
    `kv` becomes the dequantised cache in float64 (what the oracle sees) and `vmax` its largest |V|.  offset > 0: latents
    |N(0, 1)| + offset instead of N(0, 1) (every value, so every output that sees a key, is well away from zero).  kv_scale given: the
    codes are the latents themselves rounded to e4m3fn and the cache is kv_scale times them (logits of unit scale at any kv_scale near 1)."""

    def __init__(self, *args, offset=0.0, kv_scale=None, **kw):
        import torch
        import aule
        super().__init__(*args, **kw)
        lat = torch.from_numpy(self.kv)
        if offset:
            lat = lat.abs() + offset
        if kv_scale is None:
            self.codes, self.kv_scale = aule.quantize_mla_cache_fp8(lat.to(torch_dtype(self.dtype)))
        else:
            self.codes, self.kv_scale = lat.to(torch.float8_e4m3fn), torch.tensor([kv_scale], dtype=torch.float32)
        self.kv = self.codes.double().numpy() * float(self.kv_scale)
        self.vmax = float(np.abs(self.kv[..., :VD]).max())

    def device(self, torch):
        q, _, bt, cl, cu = super().device(torch)
        return q, self.codes.cuda(), bt, cl, cu

    def run(self, torch, scale=None, tensors=None, kv_scale="own", codes=None):
        """the FP8 call; kv_scale "own": the quantiser's, as a device tensor"""
        import aule
        q, kv, bt, cl, cu = tensors or self.device(torch)
        ks = self.kv_scale.cuda() if isinstance(kv_scale, str) else kv_scale
        return aule.flash_attention_mla_paged_fp8(q, kv if codes is None else codes, bt, cl, cu, max_seqlen_q=None if cu is None else self.max_sq,
                                                  scale=scale, return_lse=True, kv_scale=ks)

    def run16(self, torch, scale, tensors):
        """the 16-bit call on the codes converted (exactly) to q's dtype"""
        import aule
        q, kv, bt, cl, cu = tensors
        return aule.flash_attention_mla_paged(q, kv.to(q.dtype), bt, cl, cu, max_seqlen_q=None if cu is None else self.max_sq, scale=scale,
                                              return_lse=True)

    def live_slots(self):
        """[num_blocks * block_size] bool: the cache rows that are a key of some sequence"""
        live = np.zeros(self.codes.shape[0] * self.bs, dtype=bool)
        L = np.clip(self.cl.astype(np.int64), 0, self.bt.shape[1] * self.bs)
        for b in range(self.B):
            j = np.arange(int(L[b]))
            live[self.bt[b][j // self.bs].astype(np.int64) * self.bs + j % self.bs] = True
        return live


def _desc8(torch, c, tensors, out, lse, ks, ws=None, T=None):
    """aule_mla_paged_fp8_desc: the 16-bit descriptor's bytes (test_gpu_mla._desc), then kv_scale"""
    from aule import _capi
    d16 = _desc(torch, c, tensors, out, lse, ws, T)
    d = _capi.MlaPagedFp8Desc()
    ctypes.memmove(ctypes.byref(d), ctypes.byref(d16), ctypes.sizeof(d16))
    d.struct_size = ctypes.sizeof(d)
    d.kv_scale = ks.data_ptr()
    return d


def _c_call8(torch, c, tensors, out, lse, ks, ws=None, T=None):
    from aule import _capi
    lib = _capi.get_lib()
    d = _desc8(torch, c, tensors, out, lse, ks, ws, T)
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    return d


# the cases of the issue's table: (id, constructor arguments, whether the plan splits the keys)
def _decode_cases():
    for dtype, Hq, bs, Ls, extra, _, split in DECODE:
        yield ("decode-%s-H%d-bs%d-%s" % (dtype, Hq, bs, "_".join(map(str, Ls))), (11, dtype, Hq, bs, Ls), dict(extra_cols=extra), split)


def _ragged_cases():
    for dtype in ("bf16", "fp16"):
        yield ("ragged-" + dtype, (22, dtype, 24, 16, [70, 2, 0, 40]), dict(ns=[3, 4, 2, 2], lead=2, tail=3, q_pad=8), None)


def _split_cases():
    for dtype, L in (("bf16", 1500), ("fp16", 1500), ("bf16", 40), ("fp16", 0)):
        yield ("split-%s-L%d" % (dtype, L), (31, dtype, 16, 64, [L]), dict(table_lens=[2048], extra_cols=0), True)


ALL_CASES = list(_decode_cases()) + list(_ragged_cases()) + list(_split_cases())


def _same_owned(torch, c, a, b):
    own = torch.from_numpy(c.owned()).cuda()
    return same_bits(torch, a[0][own], b[0][own]) and same_bits(torch, a[1][own], b[1][own])


# --------------------------------------------------------------------------------------------------------------------------------- exact
@pytest.mark.parametrize("name,args,kw,split", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_scale_one_equals_the_16_bit_call_on_the_converted_codes(name, args, kw, split):
    """the two kernels differ only in how a tile reaches LDS: any difference is a tile-mapping bug.  `scale` is chosen so that the
    logits are those of the dequantised problem (the codes reach +-448)."""
    import torch
    c = Fp8Case(*args, **kw)
    tensors = c.device(torch)
    scale = float(c.kv_scale) / math.sqrt(QK)
    got = c.run(torch, scale, tensors, kv_scale=1.0)
    want = c.run16(torch, scale, tensors)
    torch.cuda.synchronize()
    if split is not None:
        assert (_nsplit(_desc(torch, c, tensors, got[0], got[1])) > 1) == split
    assert _same_owned(torch, c, got, want), name
    # kv_scale None is 1.0, a tensor of 1.0 is 1.0, the 4-d spelling of the cache is the same call, and two runs give the same bits
    q, kv, bt, cl, cu = tensors
    for ks, cache in ((None, kv), (torch.ones(1, device="cuda"), kv), (torch.tensor(1.0), kv.view(kv.shape[0], c.bs, 1, QK))):
        again = c.run(torch, scale, tensors, kv_scale=ks, codes=cache)
        assert _same_owned(torch, c, again, got), (name, ks)
    own = c.owned()
    lse = got[1].cpu().numpy()[own]
    assert not np.isnan(lse).any() and bool(torch.isfinite(got[0][torch.from_numpy(own).cuda()].float()).all())


@pytest.mark.parametrize("name,args,kw,split", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_scale_an_eighth_equals_an_eighth_of_the_16_bit_call(name, args, kw, split):
    """kv_scale = 2^-3: out = 2^-3 * (the 16-bit call on the unscaled codes with scale * 2^-3), lse the same bits.  The latents are
    |N(0, 1)| + 0.5, so every code is at least 0.5 / kv_scale > 32 and every output that sees a key is a mean of such values: no
    result is a 16-bit subnormal, which the test asserts."""
    import torch
    c = Fp8Case(*args, offset=0.5, **kw)
    assert float(c.codes.float()[..., :VD].min()) >= 32
    tensors = c.device(torch)
    scale = 8.0 * float(c.kv_scale) / math.sqrt(QK)
    got = c.run(torch, scale, tensors, kv_scale=torch.tensor([0.125], device="cuda"))
    want = c.run16(torch, scale * 0.125, tensors)
    torch.cuda.synchronize()
    own = torch.from_numpy(c.owned()).cuda()
    eighth = (want[0][own].float() * 0.125)
    tiny = torch.finfo(torch_dtype(c.dtype)).tiny
    nonzero = eighth != 0
    assert bool((eighth[nonzero].abs() >= tiny).all()) and bool((eighth[nonzero].abs() >= 4).all()), name
    assert bool(nonzero.any()) or c.cl.max() == 0
    assert same_bits(torch, got[0][own], eighth.to(got[0].dtype)), name
    assert same_bits(torch, got[1][own], want[1][own]), name


# -------------------------------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("name,args,kw,split", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_general_scale_vs_the_decode_oracle(name, args, kw, split, oracle_mod):
    """kv_scale from quantize_mla_cache_fp8 (a device tensor), judged as tests/test_gpu_mla.py judges the 16-bit call: the fp64 decode
    oracle on kv_scale * codes, fwd_tol(dtype, max |dequantised V|) and 1e-3 for lse"""
    import torch
    c = Fp8Case(*args, **kw)
    assert float(c.kv_scale) not in (1.0, 0.125) and math.frexp(float(c.kv_scale))[0] != 0.5   # no power of two
    scale = 192 ** -0.5 if c.Hq == 5 else None
    out, lse = c.run(torch, scale)
    torch.cuda.synchronize()
    assert out.shape == (c.T, c.Hq, VD) and out.dtype == torch_dtype(c.dtype) and lse.shape == (c.T, c.Hq) and lse.dtype == torch.float32
    _judge(c, out, lse, oracle_mod, "fp8 " + name, scale)
    # a float is the same scale
    again = c.run(torch, scale, kv_scale=float(c.kv_scale))
    assert _same_owned(torch, c, again, (out, lse))


# --------------------------------------------------------------------------------------------------------- keys past a sequence's length
@pytest.mark.parametrize("name,args,kw", [(c[0], c[1], c[2]) for c in ALL_CASES if c[0] in (
    "decode-bf16-H16-bs16-1_33_200", "decode-fp16-H16-bs24-1_33_200", "decode-fp16-H128-bs64-63_64_65", "ragged-bf16", "ragged-fp16", "split-bf16-L1500",
    "split-bf16-L40")])
def test_nan_codes_in_every_slot_that_is_no_live_key(name, args, kw):
    """every cache row that is not a key of some sequence holds the NaN code in all 576 bytes: out and lse equal the call with zeros
    there bit for bit, and nothing is NaN"""
    import torch
    c = Fp8Case(*args, **kw)
    tensors = c.device(torch)
    live = torch.from_numpy(c.live_slots()).view(-1, 1)
    assert bool((~live).any()) and bool(live.any())
    flat = c.codes.view(torch.uint8).view(-1, QK)
    with_nan = torch.where(live, flat, torch.full_like(flat, NAN_CODE)).view(c.codes.shape).view(torch.float8_e4m3fn).cuda()
    with_zero = torch.where(live, flat, torch.zeros_like(flat)).view(c.codes.shape).view(torch.float8_e4m3fn).cuda()
    assert bool(torch.isnan(with_nan.float()).any())
    a = c.run(torch, None, tensors, codes=with_nan)
    b = c.run(torch, None, tensors, codes=with_zero)
    torch.cuda.synchronize()
    assert _same_owned(torch, c, a, b), name
    own = torch.from_numpy(c.owned()).cuda()
    assert bool(torch.isfinite(a[0][own].float()).all()) and not bool(torch.isnan(a[1][own]).any())
    sees = torch.from_numpy(np.repeat(np.array([min(int(x), c.bt.shape[1] * c.bs) > 0 for x in c.cl]), c.toks)).cuda()
    if c.ns is None:   # plain decode: every row of a sequence with keys sees one
        assert bool(torch.isfinite(a[1][own][sees]).all())


# ------------------------------------------------------------------------------------------------------- rows never written, clamps
def test_unowned_rows_keep_their_bytes_and_lengths_are_clamped(oracle_mod):
    import torch
    c = Fp8Case(41, "bf16", 24, 16, [70, 1, 40], ns=[3, 1, 2], lead=1, tail=4)
    tensors = c.device(torch)
    ks = c.kv_scale.cuda()
    own = torch.from_numpy(c.owned()).cuda()
    out, lse = _poisoned(torch, c)
    _c_call8(torch, c, tensors, out, lse, ks)
    assert bool((out.view(torch.int16)[~own] == -1).all()) and bool((lse.view(torch.int32)[~own] == -1).all())
    _judge(c, out, lse, oracle_mod, "fp8 C entry, lead 1, tail 4")
    want, want_lse = c.run(torch, None, tensors)
    assert same_bits(torch, out[own], want[own]) and same_bits(torch, lse[own], want_lse[own])
    # plain decode with total_tokens padded past the batch
    cd = Fp8Case(42, "fp16", 16, 16, [1, 33, 200], tail=5)
    td = cd.device(torch)
    out, lse = _poisoned(torch, cd)
    _c_call8(torch, cd, td, out, lse, cd.kv_scale.cuda())
    assert bool((out.view(torch.int16)[3:] == -1).all()) and bool((lse.view(torch.int32)[3:] == -1).all())
    _judge(cd, out, lse, oracle_mod, "fp8 C entry, decode, tail 5")
    # context_lens above the table's capacity: the clamped call, bit for bit
    cap = tensors[2].shape[1] * c.bs
    big, at_cap, neg = tensors[3].clone(), tensors[3].clone(), tensors[3].clone()
    big[0], at_cap[0], neg[0] = cap + 1000, cap, -7
    a, al = c.run(torch, None, tensors[:3] + (big,) + tensors[4:])
    b, bl = c.run(torch, None, tensors[:3] + (at_cap,) + tensors[4:])
    assert same_bits(torch, a[own], b[own]) and same_bits(torch, al[own], bl[own]) and not same_bits(torch, a[own], want[own])
    a, al = c.run(torch, None, tensors[:3] + (neg,) + tensors[4:])
    assert bool((a[1:4] == 0).all()) and bool(torch.isneginf(al[1:4]).all())


def test_hostile_offsets_write_nothing_outside_out():
    import torch
    c = Fp8Case(43, "bf16", 24, 16, [70, 1, 40], ns=[3, 1, 2])
    q, kv, bt, cl, cu = c.device(torch)
    ks = c.kv_scale.cuda()
    for hostile in ([0, 4, c.T + 5, c.T + 100], [-5, 2, 1, 2 ** 31 - 1], [c.T + 1, c.T + 2, c.T + 3, c.T + 4]):
        big_out, big_lse = _poisoned(torch, c, c.T + 8)
        cu.copy_(torch.tensor(hostile, dtype=torch.int32, device="cuda"))
        _c_call8(torch, c, (q, kv, bt, cl, cu), big_out[4:4 + c.T], big_lse[4:4 + c.T], ks)
        for x in (big_out.view(torch.int16), big_lse.view(torch.int32)):
            assert bool((x[:4] == -1).all()) and bool((x[4 + c.T:] == -1).all()), hostile


def test_poisoned_workspace_does_not_change_a_split_result():
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    c = Fp8Case(31, "bf16", 16, 64, [1500], table_lens=[2048], extra_cols=0)
    tensors = c.device(torch)
    ks = c.kv_scale.cuda()
    want, want_lse = c.run(torch, None, tensors)
    out, lse = _poisoned(torch, c)
    size = lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(_desc8(torch, c, tensors, out, lse, ks)))
    assert size > 0 and size == lib.aule_attention_mla_paged_workspace_size(ctypes.byref(_desc(torch, c, tensors, out, lse)))
    for nbytes, with_lse in ((size, True), (size, False), (64, True)):   # (64: too small, the library allocates on the stream)
        out, lse = _poisoned(torch, c)
        ws = torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")
        _c_call8(torch, c, tensors, out, lse if with_lse else None, ks, ws)
        assert same_bits(torch, out, want)
        assert same_bits(torch, lse, want_lse) if with_lse else bool((lse.view(torch.int32) == -1).all())


@pytest.mark.parametrize("which", ["decode", "ragged-split"])
def test_inside_an_arena(which, oracle_mod):
    """every tensor of the call -- the codes and the scale included -- between guard bands of one allocation, outputs and workspace
    poisoned: the guards stay intact, the inputs unchanged, and the owned rows equal the plain call's bits"""
    import torch
    from aule import _capi
    lib = _capi.get_lib()
    if which == "decode":
        c = Fp8Case(51, "fp16", 16, 16, [1, 33, 150], extra_cols=0, tail=2)
    else:
        c = Fp8Case(52, "bf16", 24, 64, [700, 3, 129], ns=[3, 1, 2], table_lens=[1024] * 3, extra_cols=0, lead=1, tail=2)
    plain = c.device(torch)
    own = torch.from_numpy(c.owned()).cuda()
    if which == "decode":   # (the Python call takes no padded rows with null offsets: the first B rows are the sequences')
        want, want_lse = (x[own] for x in _poisoned(torch, c))
        want[:], want_lse[:] = c.run(torch, None, (plain[0][:c.B],) + plain[1:])
    else:
        want, want_lse = (x[own] for x in c.run(torch, None, plain))
    probe_out, probe_lse = _poisoned(torch, c)
    d0 = _desc8(torch, c, plain, probe_out, probe_lse, c.kv_scale.cuda())
    size = int(lib.aule_attention_mla_paged_fp8_workspace_size(ctypes.byref(d0)))
    assert (size > 0) == (which == "ragged-split")
    dt = torch_dtype(c.dtype)
    host = dict(q=torch.from_numpy(c.q).to(dt), kv=c.codes.view(torch.uint8), bt=torch.from_numpy(c.bt), cl=torch.from_numpy(c.cl), ks=c.kv_scale)
    if c.cu is not None:
        host["cu"] = torch.from_numpy(c.cu)
    regions = [(k, v.numel() * v.element_size(), "in") for k, v in host.items()]
    regions += [("out", c.T * c.Hq * VD * 2, "out"), ("lse", c.T * c.Hq * 4, "out"), ("ws", max(size, 16), "ws")]
    arena = Arena(torch, regions, QK * 2)
    kept = {k: arena.upload(k, v) for k, v in host.items()}
    arena.fill(POISON)
    tensors = (arena.view("q", dt, (c.T, c.Hq, QK)), arena.view("kv", torch.float8_e4m3fn, tuple(c.codes.shape)),
               arena.view("bt", torch.int32, c.bt.shape), arena.view("cl", torch.int32, c.cl.shape),
               arena.view("cu", torch.int32, c.cu.shape) if c.cu is not None else None)
    out, lse = arena.view("out", dt, (c.T, c.Hq, VD)), arena.view("lse", torch.float32, (c.T, c.Hq))
    _c_call8(torch, c, tensors, out, lse, arena.view("ks", torch.float32, (1,)), arena.bytes("ws") if size else None)
    assert arena.guards_intact(), arena.damage()
    for k, v in kept.items():
        assert arena.unchanged(k, v), k
    assert same_bits(torch, out[own], want) and same_bits(torch, lse[own], want_lse)
    assert bool((out.view(torch.int16)[~own] == -1).all()) and bool((lse.view(torch.int32)[~own] == -1).all())
    _judge(c, out, lse, oracle_mod, "fp8 arena, " + which)


# -------------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_on_the_device():
    import torch
    import aule
    from aule import _capi
    lib = _capi.get_lib()
    c = Fp8Case(71, "bf16", 16, 16, [1, 33, 200])
    q, kv, bt, cl, _ = c.device(torch)
    ks = c.kv_scale.cuda()
    with pytest.raises(aule.AuleError, match="no CPU fallback"):
        aule.flash_attention_mla_paged_fp8(q.cpu(), kv.cpu(), bt.cpu(), cl.cpu(), kv_scale=c.kv_scale)
    with pytest.raises(ValueError, match="must be torch.float8_e4m3fn"):
        aule.flash_attention_mla_paged_fp8(q, kv.to(q.dtype), bt, cl)
    with pytest.raises(ValueError, match="fp16 / bf16"):
        aule.flash_attention_mla_paged(q, kv, bt, cl)
    with pytest.raises(ValueError, match="kv_scale must be None, a float, or a 0-d"):
        aule.flash_attention_mla_paged_fp8(q, kv, bt, cl, kv_scale=torch.ones(2, device="cuda"))
    out, lse = _poisoned(torch, c)

    def refused(change, needle):
        d = _desc8(torch, c, (q, kv, bt, cl, None), out, lse, ks)
        change(d)
        assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == -3
        msg = lib.aule_get_error()
        msg = msg.decode() if isinstance(msg, bytes) else str(msg)
        assert needle in msg and msg.startswith("Paged MLA FP8 attention failed: "), msg

    refused(lambda d: setattr(d, "qk_dim", 512), "qk_dim 512")
    refused(lambda d: setattr(d, "struct_size", 136), "struct_size")
    refused(lambda d: setattr(d, "kv_scale", None), "null kv_scale")
    refused(lambda d: setattr(d, "kv_scale", ks.data_ptr() + 2), "4-byte aligned")
    refused(lambda d: setattr(d, "kv_cache", kv.data_ptr() + 8), "16-byte aligned")
    torch.cuda.synchronize()
    assert bool((out.view(torch.int16) == -1).all())
    d = _desc8(torch, c, (q, kv, bt, cl, None), out, lse, ks)
    d.heads_q = 0
    assert lib.aule_attention_mla_paged_fp8_ex(ctypes.byref(d)) == 0
    assert DTYPE_CODE[c.dtype] == d.dtype
