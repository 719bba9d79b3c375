"""The indexer's write side on the GPU (csrc/mla_indexer_append_gfx950.hip behind aule.mla_indexer_k_append / mla_indexer_q_rotate):
rows of 128 through norm, RoPE and the Hadamard rotation, one rounding, then a dense store or the paged index-key cache.

The reference is `_transform` in fp64 on the CPU (the Hadamard as the explicit +-1 matrix).  The transform's bar is
|got - ref| <= u |ref| + A, u = 2^-8 (bf16) / 2^-11 (fp16), one rounding of the output type; A covers the fp32 evaluation and is
4 x the largest absolute error of `_transform` run in plain fp32 torch against the fp64 reference on the same inputs -- computed from
the reference alone, never from the kernel's output.  Everything about the FP8 cache, the skips, the pipeline and the graph is
compared as integers."""
import functools

import pytest
import torch

import aule

pytestmark = pytest.mark.gpu

T, H, NB, BS, TABLE = 37, 3, 5, 8, 48   # a partial wave (8 rows) and a partial workgroup (32 rows); 40 cache rows
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
EPS = 1e-6
PATTERN = 0xA5


@functools.lru_cache(None)
def _inputs(dtype):
    """CPU inputs, made once per dtype: N(0, 1) with one channel per row scaled by 50; keys are a column slice of a wider tensor,
    queries three heads of a row with 8 elements of padding; slots shuffled over the cache; a real rotary table."""
    g = torch.Generator().manual_seed(7)
    def rows(*shape):
        x = torch.randn(*shape, 128, generator=g)
        return x * (1 + 49 * torch.nn.functional.one_hot(torch.randint(0, 128, shape, generator=g), 128))
    kbase = torch.randn(T, 192, generator=g)
    kbase[:, 64:] = rows(T)
    qbase = torch.randn(T, H * 128 + 8, generator=g)
    qbase[:, :H * 128] = rows(T, H).flatten(1)
    ang = torch.arange(TABLE, dtype=torch.float64)[:, None] * (10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32))
    return dict(kbase=kbase.to(DT[dtype]), qbase=qbase.to(DT[dtype]), cos=ang.cos().float(), sin=ang.sin().float(),
                pos=torch.randint(0, TABLE, (T,), generator=g), slots=torch.randperm(NB * BS, generator=g)[:T],
                w=1 + 0.1 * torch.randn(128, generator=g), b=0.1 * torch.randn(128, generator=g))


def _transform(x, dt, w=None, b=None, cos=None, sin=None, pos=None, layout=None, off=0, had=False):
    """steps 1-3 of the row transform on x [T, heads, 128], evaluated in dtype dt"""
    x = x.to(dt)
    if w is not None:
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        x = (x - mu) / torch.sqrt(var + EPS) * w.to(dt) + (b.to(dt) if b is not None else 0)
    if layout is not None:
        c, s = cos[pos].to(dt)[:, None], sin[pos].to(dt)[:, None]
        r = x[..., off:off + 64]
        x1, x2 = (r[..., :32], r[..., 32:]) if layout == "half" else (r[..., 0::2], r[..., 1::2])
        y1, y2 = x1 * c - x2 * s, x1 * s + x2 * c
        y = torch.cat((y1, y2), -1) if layout == "half" else torch.stack((y1, y2), -1).flatten(-2)
        x = torch.cat((x[..., :off], y, x[..., off + 64:]), -1)
    if had:
        i = torch.arange(128)
        bits = i[:, None] & i[None, :]
        parity = sum((bits >> n) & 1 for n in range(7)) & 1
        x = x @ (1 - 2 * parity).to(dt) * 2.0 ** -3.5
    return x


def _stage_args(z, rope, off, norm, had):
    """(reference keywords, API keywords on the device) of one combination of stages"""
    ref, api = dict(off=off, had=had), dict(rope_offset=off, hadamard=had)
    if rope:
        ref.update(cos=z["cos"], sin=z["sin"], pos=z["pos"], layout=rope)
        api.update(cos=z["cos"].cuda(), sin=z["sin"].cuda(), positions=z["pos"].cuda(), rope_layout=rope)
    if norm:
        ref.update(w=z["w"], b=z["b"] if norm == "bias" else None)
        api.update(norm_weight=z["w"].cuda(), norm_bias=z["b"].cuda() if norm == "bias" else None, eps=EPS)
    return ref, api


def _cache(dtype, fill=0):
    """(cache, k_scale or None) on the device, every byte `fill`; dtype "fp8" or a 16-bit name"""
    if dtype == "fp8":
        return (torch.full((NB, BS, 128), fill, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn),
                torch.full((NB, BS, 4), fill, dtype=torch.uint8, device="cuda").view(torch.float32).view(NB, BS))
    return torch.full((NB, BS, 256), fill, dtype=torch.uint8, device="cuda").view(DT[dtype]), None


# dtype, rope, rope_offset, norm, hadamard, destination: every value of every axis, every stage alone, the two serving combinations
CASES = [
    ("bf16", None, 0, None, False, "dense"),
    ("bf16", "half", 0, None, False, "dense"),
    ("fp16", "interleaved", 64, None, False, "cache"),
    ("bf16", None, 0, "bias", False, "cache"),
    ("fp16", None, 0, "nobias", False, "cache"),
    ("bf16", None, 0, None, True, "inplace"),
    ("fp16", None, 0, None, True, "cache"),
    ("bf16", "half", 0, "bias", True, "cache"),
    ("bf16", "interleaved", 0, None, True, "inplace"),
    ("fp16", "half", 64, "nobias", True, "cache"),
    ("bf16", "interleaved", 64, "bias", True, "cache"),
]


@pytest.mark.parametrize("dtype,rope,off,norm,had,dest", CASES, ids=lambda v: str(v))
def test_transform_against_fp64(dtype, rope, off, norm, had, dest):
    z = _inputs(dtype)
    ref_kw, api_kw = _stage_args(z, rope, off, norm, had)
    if dest == "cache":
        x = z["kbase"][:, None, 64:]                                     # [T, 1, 128]
        cache, _ = _cache(dtype)
        assert aule.mla_indexer_k_append(z["kbase"].cuda()[:, 64:], cache, z["slots"].cuda(), **api_kw) is None
        got = cache.view(-1, 128)[z["slots"].cuda()][:, None]
    else:
        x = z["qbase"][:, :H * 128].unflatten(1, (H, 128))
        qbase = z["qbase"].cuda()
        q = qbase[:, :H * 128].unflatten(1, (H, 128))
        got = aule.mla_indexer_q_rotate(q, out=q if dest == "inplace" else None, **api_kw)
        assert (got.data_ptr() == q.data_ptr()) == (dest == "inplace") and got.shape == q.shape
        assert torch.equal(qbase[:, H * 128:].cpu(), z["qbase"][:, H * 128:])     # the padding between the tokens
        if dest == "dense":
            assert got.is_contiguous() and torch.equal(q.cpu(), x)
    ref = _transform(x, torch.float64, **ref_kw)
    A = 4 * float((_transform(x, torch.float32, **ref_kw).double() - ref).abs().max())
    err = (got.cpu().double() - ref).abs()
    bound = U[dtype] * ref.abs() + A
    print("max |err| %.3e, A %.3e, max err / bound %.3f" % (float(err.max()), A, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("fmt", ["amax", "ue8m0"])
def test_fp8_cache_is_the_16_bit_result_quantised(fmt, dtype):
    """norm without bias, RoPE and Hadamard into both cache kinds; token 5 is an all-zero row at position 0 (table row (1, 0): it stays +0)"""
    z = _inputs(dtype)
    k = z["kbase"].cuda()[:, 64:].clone()
    k[5] = 0
    pos = z["pos"].clone()
    pos[5] = 0
    _, kw = _stage_args(dict(z, pos=pos), "half", 0, "nobias", True)
    slots = z["slots"].cuda()
    c16, _ = _cache(dtype)
    c8, sc = _cache("fp8")
    aule.mla_indexer_k_append(k, c16, slots, **kw)
    aule.mla_indexer_k_append(k, c8, slots, k_scale=sc, scale_format=fmt, **kw)
    r, codes, scale = c16.view(-1, 128)[slots].cpu(), c8.view(torch.uint8).view(-1, 128)[slots].cpu(), sc.view(-1)[slots].cpu()
    want_codes, s0 = aule.quantize_indexer_cache_fp8(r[None])
    want_codes, s0 = want_codes[0].view(torch.uint8), s0[0]
    if fmt == "ue8m0":
        bits = ((s0.view(torch.int32) + 0x007FFFFF) & 0x7F800000).clamp_min(0x00800000)
        assert bool(((scale.view(torch.int32) & 0x007FFFFF) == 0).all())                  # powers of two
        s0 = bits.view(torch.float32)
        want_codes = (r.float() / s0[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(scale.view(torch.int32), s0.view(torch.int32))
    assert torch.equal(codes, want_codes)
    assert float(scale[5]) == 1.0 and not codes[5].any() and codes.any()


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_skipped_tokens_and_unaddressed_slots_keep_their_bytes(kind):
    z = _inputs("bf16")
    slots, pos = z["slots"].clone(), z["pos"].clone()
    slots[3], slots[7], pos[11] = -1, NB * BS, TABLE
    _, kw = _stage_args(dict(z, pos=pos), "interleaved", 0, "bias", True)
    cache, sc = _cache(kind, PATTERN)
    aule.mla_indexer_k_append(z["kbase"].cuda()[:, 64:], cache, slots.cuda(), k_scale=sc, **kw)
    written = torch.zeros(NB * BS, dtype=torch.bool)
    written[slots[[t for t in range(T) if t not in (3, 7, 11)]]] = True
    rows = cache.view(torch.uint8).view(NB * BS, -1).cpu()
    assert bool((rows[~written] == PATTERN).all()) and int((~written).sum()) == NB * BS - (T - 3)
    assert bool((rows[written] != PATTERN).any(1).all())
    if sc is not None:
        sbytes = sc.view(torch.uint8).view(NB * BS, 4).cpu()
        assert bool((sbytes[~written] == PATTERN).all()) and bool((sbytes[written] != PATTERN).any(1).all())


def test_the_indexer_reads_what_the_append_wrote():
    z = _inputs("bf16")
    _, kw = _stage_args(z, "half", 0, None, True)
    table = torch.randperm(NB, generator=torch.Generator().manual_seed(3))
    j = torch.arange(T)
    slots = (table[j // BS] * BS + j % BS).cuda()            # key j of the one sequence sits at logical position j
    c16, _ = _cache("bf16")
    c8, sc = _cache("fp8")
    sc.fill_(1.0)                                            # an unwritten row: codes 0, scale 1 = quantize_indexer_cache_fp8 of zeros
    aule.mla_indexer_k_append(z["kbase"].cuda()[:, 64:], c16, slots, **kw)
    aule.mla_indexer_k_append(z["kbase"].cuda()[:, 64:], c8, slots, k_scale=sc, **kw)
    q = aule.mla_indexer_q_rotate(z["qbase"].cuda()[:, :H * 128].unflatten(1, (H, 128)), **kw)
    weights = torch.rand(T, H, generator=torch.Generator().manual_seed(4)).cuda()
    tables = dict(block_tables=table[None].int().cuda(), context_lens=torch.tensor([T], dtype=torch.int32).cuda(),
                  cu_seqlens_q=torch.tensor([0, T], dtype=torch.int32).cuda(), max_seqlen_q=T)
    got = aule.mla_indexer_logits(q, weights, c8, k_scale=sc, **tables)
    codes, s = aule.quantize_indexer_cache_fp8(c16.cpu())
    want = aule.mla_indexer_logits(q, weights, codes.cuda(), k_scale=s.cuda(), **tables)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and bool(torch.isfinite(got[:, 0]).all())


def test_graph_replays_read_the_new_slots_and_keys():
    z = _inputs("bf16")
    _, kw = _stage_args(z, "half", 0, "bias", True)
    k, slots = z["kbase"].cuda()[:, 64:].clone(), z["slots"].cuda()
    cache, sc = _cache("fp8")
    step = lambda c, s: aule.mla_indexer_k_append(k, c, slots, k_scale=s, **kw)   # noqa: E731
    step(cache, sc)              # (the library is initialised before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(cache, sc)
    for i in range(3):
        if i:   # new contents, in place: other keys, other slots
            k.copy_(k.flip(0) * (1 + i))
            slots.copy_((slots + 3 * i) % (NB * BS))
        cache.view(torch.uint8).zero_()
        sc.zero_()
        graph.replay()
        graph.replay()
        want, want_sc = _cache("fp8")
        step(want, want_sc)
        torch.cuda.synchronize()
        assert torch.equal(cache.view(torch.uint8), want.view(torch.uint8)) and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32)), i
