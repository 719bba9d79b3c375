"""Sparse MLA attention on the GPU (csrc/fa_fwd_mla_sparse_gfx950.hip behind aule.flash_attention_mla_sparse /
aule_attention_mla_sparse_ex): every token attends to the rows of the latent cache that its own list of slots names.

The judge is formed here: per token, fp64 NumPy on the quantised inputs -- gather the valid rows (duplicates kept), scores,
log-sum-exp, P @ rows[:, :512].  Bounds are the project's: util.fwd_tol(dtype, max |V|) for out, 1e-3 for lse, lse == -inf exactly
where a token has no valid entry; every check prints the maxima it reached.  Inputs are N(0, 1) quantised to the dtype.  Every launch
of the C entry writes into buffers pre-filled with 0xFF inside a hostile.Arena (guard bands intact afterwards, inputs unchanged), and
every cache row that no valid entry names holds NaN bits."""
import ctypes
import math

import numpy as np
import pytest

from hostile import POISON, Arena, same_bits
from util import assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

LSE_ATOL = 1e-3
QK, VD = 576, 512
DTYPE_CODE = {"fp16": 1, "bf16": 2}
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


class Problem:
    """Seeded q [T, Hq, 576] and latent cache [nb, bs, 576] of N(0, 1) quantised to `dtype` (float32 arrays holding the quantised
    values).  fp8: the cache is quantised with aule.quantize_mla_cache_fp8 -- `codes` / `kv_scale` are what the device sees and `kv`
    becomes the dequantised cache (what the judge sees).  q_pad > 0: q is a slice of a wider projection."""

    def __init__(self, seed, dtype, T, Hq, nb, bs, fp8=False, q_pad=0):
        import torch
        import aule
        rng = np.random.RandomState(seed)
        self.rng, self.dtype, self.T, self.Hq, self.nb, self.bs, self.S, self.fp8, self.q_pad = rng, dtype, T, Hq, nb, bs, nb * bs, fp8, q_pad
        self.q = quantize(rng.randn(T, Hq, QK).astype(np.float32), dtype)
        self.kv = quantize(rng.randn(nb, bs, QK).astype(np.float32), dtype).astype(np.float64)
        self.codes = self.kv_scale = None
        if fp8:
            self.codes, self.kv_scale = aule.quantize_mla_cache_fp8(torch.from_numpy(self.kv).to(torch_dtype(dtype)))
            self.kv = self.codes.double().numpy() * float(self.kv_scale)
        self.vmax = float(np.abs(self.kv[..., :VD]).max())

    def draw(self, topk, replace=None):
        """[T, topk] int32 valid slots, a different list per token (with repeats only when the list is longer than the cache)"""
        replace = topk > self.S if replace is None else replace
        return np.stack([self.rng.choice(self.S, size=topk, replace=replace) for _ in range(self.T)]).astype(np.int32)

    def valid(self, idx):
        return (idx >= 0) & (idx < self.S)

    def cache_bytes(self, idx):
        """the cache as the device sees it, every row that no valid entry of idx names filled with NaN bits"""
        import torch
        named = np.zeros(self.S, dtype=bool)
        named[idx[self.valid(idx)]] = True
        dead = torch.from_numpy(~named)
        if self.fp8:
            c = self.codes.clone().view(torch.uint8).reshape(self.S, QK)
            c[dead] = 0x7F
            return c.view(torch.float8_e4m3fn).reshape(self.nb, self.bs, QK)
        c = torch.from_numpy(self.kv).to(torch_dtype(self.dtype)).reshape(self.S, QK).view(torch.int16)
        c[dead] = -1
        return c.view(torch_dtype(self.dtype)).reshape(self.nb, self.bs, QK)

    def judge(self, idx, scale=None):
        """(out [T, Hq, 512], lse [T, Hq]) in float64"""
        sc = 1.0 / math.sqrt(QK) if scale is None else scale
        flat = self.kv.reshape(self.S, QK)
        out, lse = np.zeros((self.T, self.Hq, VD)), np.full((self.T, self.Hq), -np.inf)
        for t in range(self.T):
            rows = flat[idx[t][self.valid(idx[t])]]
            if len(rows):
                s = self.q[t].astype(np.float64) @ rows.T * sc
                m = s.max(axis=-1, keepdims=True)
                p = np.exp(s - m)
                lse[t] = m[:, 0] + np.log(p.sum(axis=-1))
                out[t] = (p / p.sum(axis=-1, keepdims=True)) @ rows[:, :VD]
        return out, lse


def check(p, got, idx, what, scale=None, ref=None, lse_atol=LSE_ATOL):
    """out / lse against the judge with the project's bounds; prints and returns the maxima.  (lse_atol: tools/fuzz_serving.py's hard-data
    draws pass a bound computed from the reference alone; every test of this file keeps LSE_ATOL.)"""
    out, lse = got[0].float().cpu().numpy().astype(np.float64), got[1].cpu().numpy().astype(np.float64)
    ref, lref = p.judge(idx, scale) if ref is None else ref
    atol, rtol = fwd_tol(p.dtype, p.vmax)
    none = ~np.isfinite(lref)
    oerr = float(np.abs(out - ref).max())
    lerr = float(np.abs(lse[~none] - lref[~none]).max()) if (~none).any() else 0.0
    print("%s: max |out err| %.3g (atol %.3g + %.3g |ref|), max |lse err| %.3g (bound %.3g), rows without a key %d of %d"
          % (what, oerr, atol, rtol, lerr, lse_atol, int(none.sum()), none.size))
    assert not np.isnan(out).any() and not np.isnan(lse).any(), what
    assert_close(out, ref, atol, rtol, what)
    assert np.array_equal(np.isneginf(lse), none), "%s: lse must be -inf exactly where a token has no valid entry" % what
    assert bool((out[none] == 0).all()), "%s: a token without a valid entry must give zeros" % what
    assert lerr <= lse_atol, (what, lerr)
    return oerr, lerr


def _desc(torch, p, T, topk):
    from aule import _capi
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.cache_dtype, d.heads_q = DTYPE_CODE[p.dtype], int(p.fp8), p.Hq
    d.num_blocks, d.block_size, d.total_tokens, d.topk = p.nb, p.bs, T, topk
    d.q_token_stride = (p.Hq + p.q_pad) * QK
    d.device = torch.cuda.current_device()
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return d


def plan_of(torch, p, T, topk):
    """(row blocks, rows per block, nsplit, grid, workspace bytes) from the plan hook"""
    from aule import _capi
    out = (ctypes.c_int32 * 6)()
    d = _desc(torch, p, T, topk)
    assert _capi.load().aule_hip_debug_mla_sparse_plan(ctypes.byref(d), out, 6) == 6
    return out[0], out[1], out[2], out[3], (out[5] << 32) | (out[4] & 0xffffffff)


class Launch:
    """One problem's tensors inside an Arena, the C entry run on them: q (a slice of a wider projection when p.q_pad), the poisoned
    cache, the list, the FP8 scale, out, lse and (ws_bytes > 0) a caller workspace.  Outputs, workspace and guards are 0xFF before
    every run; after it the guards are intact and the inputs unchanged."""

    def __init__(self, torch, p, idx, scale=None, kv_scale="own", ws_bytes=0, cache=None):
        self.torch, self.p, self.idx, self.scale = torch, p, np.ascontiguousarray(idx, dtype=np.int32), scale
        self.T, self.topk = self.idx.shape
        dt = torch_dtype(p.dtype)
        q = torch.zeros((self.T, p.Hq + p.q_pad, QK), dtype=dt)
        q[:, :p.Hq] = torch.from_numpy(p.q[:self.T]).to(dt)
        cache = p.cache_bytes(self.idx) if cache is None else cache
        regions = [("q", q.numel() * 2, "in"), ("kv", cache.numel() * cache.element_size(), "in"), ("idx", self.idx.size * 4, "in"),
                   ("ks", 4, "in"), ("out", self.T * p.Hq * VD * 2, "out"), ("lse", self.T * p.Hq * 4, "out")]
        if ws_bytes:
            regions.append(("ws", ws_bytes, "ws"))
        self.arena = a = Arena(torch, regions, QK * 2)
        ks = p.kv_scale if isinstance(kv_scale, str) else torch.tensor([1.0 if kv_scale is None else kv_scale], dtype=torch.float32)
        self.inputs = {"q": a.upload("q", q), "kv": a.upload("kv", cache), "idx": a.upload("idx", self.idx),
                       "ks": a.upload("ks", ks if ks is not None else torch.ones(1))}
        self.q = a.view("q", dt, (self.T, p.Hq + p.q_pad, QK))[:, :p.Hq]
        self.kv = a.view("kv", cache.dtype, (p.nb, p.bs, QK))
        self.indices = a.view("idx", torch.int32, (self.T, self.topk))
        self.ks = a.view("ks", torch.float32, (1,))
        self.out = a.view("out", dt, (self.T, p.Hq, VD))
        self.lse = a.view("lse", torch.float32, (self.T, p.Hq))

    def desc(self, ws=True):
        a, d = self.arena, _desc(self.torch, self.p, self.T, self.topk)
        d.scale = 0.0 if self.scale is None else self.scale
        d.q, d.kv_cache, d.indices, d.out, d.lse = a.ptr("q"), a.ptr("kv"), a.ptr("idx"), a.ptr("out"), a.ptr("lse")
        if self.p.fp8:
            d.kv_scale = a.ptr("ks")
        if ws and "ws" in a.regions:
            d.workspace, d.workspace_bytes = a.ptr("ws"), a.size("ws")
        return d

    def run(self, d=None, expect=0):
        """the C entry; returns clones of (out, lse)"""
        from aule import _capi
        torch, a = self.torch, self.arena
        lib = _capi.get_lib()
        a.fill(POISON)
        rc = lib.aule_attention_mla_sparse_ex(ctypes.byref(self.desc() if d is None else d))
        torch.cuda.synchronize()
        assert rc == expect, (rc, lib.aule_get_error())
        assert a.guards_intact(), a.damage()
        for name, was in self.inputs.items():
            assert a.unchanged(name, was), name
        return self.out.clone(), self.lse.clone()

    def python(self, **kw):
        """the Python entry on the same tensors"""
        import aule
        if self.p.fp8:
            kw.setdefault("kv_scale", self.ks)
        got = aule.flash_attention_mla_sparse(self.q, self.kv, self.indices, scale=self.scale, return_lse=True, **kw)
        self.torch.cuda.synchronize()
        return got


def _same(torch, a, b):
    return same_bits(torch, a[0], b[0]) and same_bits(torch, a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ 1. shapes at the seams
HEADS = (1, 16, 64, 65, 128)     # a partial block, a full one, a second block of one row, two full
TOPKS = (1, 63, 64, 65, 129, 200, 512)
BLOCKS = ((1, 300), (16, 19), (48, 7))   # (block_size, num_blocks): a few hundred slots
# (block size, dtype and the padding of q's token stride rotate with periods 3, 2 and 4, so both dtypes meet a dense and a padded q)
SEAMS = [(Hq, topk) + BLOCKS[(i + j) % 3] + (("bf16", "fp16")[(i + j) % 2], 8 * ((i + j) % 4 // 2))
         for i, Hq in enumerate(HEADS) for j, topk in enumerate(TOPKS)]
assert {(c[4], c[5]) for c in SEAMS} == {("bf16", 0), ("bf16", 8), ("fp16", 0), ("fp16", 8)}


@pytest.mark.parametrize("Hq,topk,bs,nb,dtype,q_pad", SEAMS, ids=lambda x: str(x))
def test_shapes_at_the_seams(Hq, topk, bs, nb, dtype, q_pad):
    """three tokens with different lists, through the C entry (in the arena) and the Python entry (the same bits)"""
    import torch
    p = Problem(100 + Hq + topk, dtype, 3, Hq, nb, bs, q_pad=q_pad)
    idx = p.draw(topk)
    run = Launch(torch, p, idx)
    assert run.q.stride(0) == (Hq + q_pad) * QK
    got = run.run()
    rb, rows, nsplit, grid, _ = plan_of(torch, p, 3, topk)
    assert rb == (Hq + 63) // 64 and grid == 3 * rb * nsplit
    check(p, got, idx, "seams H%d topk%d bs%d %s nsplit %d" % (Hq, topk, bs, dtype, nsplit))
    py = run.python()
    assert py[0].shape == (3, Hq, VD) and py[0].dtype == torch_dtype(dtype) and py[1].shape == (3, Hq) and py[1].dtype == torch.float32
    assert _same(torch, py, got)
    # the 4-d spelling of the cache, the [T, 1, topk] spelling of the list and out alone are the same call
    import aule
    alone = aule.flash_attention_mla_sparse(run.q, run.kv.view(nb, bs, 1, QK), run.indices.view(3, 1, topk))
    assert same_bits(torch, alone, got[0])


def test_unpaged_latent_and_no_tokens():
    """a contiguous [L, 576] latent is the cache [L, 1, 576]; T = 0 returns empty tensors"""
    import torch
    import aule
    p = Problem(7, "bf16", 2, 16, 333, 1)
    idx = p.draw(100)
    run = Launch(torch, p, idx)
    got = run.run()
    check(p, got, idx, "un-paged latent [333, 576]")
    out, lse = aule.flash_attention_mla_sparse(run.q[:0], run.kv, run.indices[:0], return_lse=True)
    assert out.shape == (0, 16, VD) and lse.shape == (0, 16)
    d = run.desc()
    d.total_tokens = 0
    got0 = run.run(d)
    assert bool((got0[0].view(torch.int16) == -1).all()) and bool((got0[1].view(torch.int32) == -1).all())   # nothing was launched


# -------------------------------------------------------------------------------------------------------------------- 2. invalid entries
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_invalid_entries_are_skipped(dtype):
    """-1 scattered through the list, entries >= S, INT32_MIN, INT32_MAX, one whole 64-entry tile invalid in the middle, and a token
    whose every entry is invalid: the call equals the judge, and the call on the list with those entries removed"""
    import torch
    p = Problem(21, dtype, 3, 16, 19, 16)
    topk = 200
    idx = p.draw(topk).astype(np.int64)
    bad = np.array([-1, p.S, p.S + 5, I32_MIN, I32_MAX, -7, 2 * p.S])
    for t in (0, 1):
        at = p.rng.choice(topk, size=50, replace=False)
        idx[t, at] = bad[p.rng.randint(len(bad), size=50)]
    idx[0, 64:128] = bad[p.rng.randint(len(bad), size=64)]      # tile 1 of token 0: nothing valid
    idx[1, 0], idx[1, topk - 1] = -1, I32_MAX                  # ... the first and the last entry of token 1
    idx[2] = bad[p.rng.randint(len(bad), size=topk)]          # token 2: no valid entry
    idx = idx.astype(np.int32)
    assert 60 < p.valid(idx[0]).sum() < 140 and not p.valid(idx[0, 64:128]).any() and not p.valid(idx[2]).any()
    run = Launch(torch, p, idx)
    got = run.run()
    ref = p.judge(idx)
    check(p, got, idx, "invalid entries %s" % dtype, ref=ref)
    assert bool((got[0][2] == 0).all()) and bool(torch.isneginf(got[1][2]).all())
    assert _same(torch, run.python(), got)
    # the lists with the invalid entries removed, one token at a time (their lengths differ); the cache poisoned as before
    for t in (0, 1):
        keep = idx[t][p.valid(idx[t])][None, :]
        one = Problem(21, dtype, 3, 16, 19, 16)
        one.q, one.T = p.q[t:t + 1], 1
        lean = Launch(torch, one, keep, cache=p.cache_bytes(idx)).run()
        check(one, lean, keep, "token %d, %d valid entries alone" % (t, keep.shape[1]), ref=(ref[0][t:t + 1], ref[1][t:t + 1]))
        # ... and the two calls against each other, at the same bounds
        atol, rtol = fwd_tol(dtype, p.vmax)
        with_o, lean_o = got[0][t:t + 1].float().cpu().numpy().astype(np.float64), lean[0].float().cpu().numpy().astype(np.float64)
        oerr = float(np.abs(with_o - lean_o).max())
        lerr = float((got[1][t].double() - lean[1][0].double()).abs().max())
        print("token %d, with the invalid entries against without: max |out diff| %.3g (atol %.3g + %.3g |ref|), max |lse diff| %.3g (bound %.3g)"
              % (t, oerr, atol, rtol, lerr, LSE_ATOL))
        assert_close(with_o, lean_o, atol, rtol, "with and without the invalid entries")
        assert lerr <= LSE_ATOL, (t, lerr)


# ------------------------------------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("dtype,Hq", [("bf16", 65), ("fp16", 16)])
def test_one_valid_entry_returns_its_row_bit_for_bit(dtype, Hq):
    """p = 1, l = 1: out is the row's first 512 elements, whatever tile the entry sits in; lse is its score"""
    import torch
    p = Problem(31, dtype, 3, Hq, 19, 16)
    topk = 130
    idx = np.full((3, topk), -1, dtype=np.int32)
    slots = p.rng.choice(p.S, size=3, replace=False)
    for t, at in enumerate((0, 70, topk - 1)):
        idx[t, at] = slots[t]
    run = Launch(torch, p, idx)
    got = run.run()
    check(p, got, idx, "one valid entry %s H%d" % (dtype, Hq))
    rows = run.kv.reshape(p.S, QK)[torch.from_numpy(slots).cuda()][:, :VD]
    assert same_bits(torch, got[0], rows[:, None, :].expand(3, Hq, VD).contiguous())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_entry_twice_is_the_same_out_and_ln2_more_lse(dtype):
    import torch
    p = Problem(32, dtype, 3, 16, 19, 16)
    idx = p.draw(100)
    twice = np.repeat(idx, 2, axis=1)
    a, b = Launch(torch, p, idx).run(), Launch(torch, p, twice).run()
    ref = p.judge(idx)
    check(p, a, idx, "plain list %s" % dtype, ref=ref)
    check(p, b, twice, "every entry twice %s" % dtype, ref=(ref[0], ref[1] + math.log(2.0)))
    gap = (b[1] - a[1]).double().cpu().numpy()
    print("lse(twice) - lse(once) - ln 2: max |.| %.3g" % np.abs(gap - math.log(2.0)).max())
    assert np.abs(gap - math.log(2.0)).max() <= LSE_ATOL


# ------------------------------------------------------------------------------------------------------ 4. the dense call as a special case
@pytest.mark.parametrize("dtype,Hq,bs,Ls", [("bf16", 16, 1, [1, 64, 100, 191]), ("fp16", 128, 1, [1, 64, 100, 191]),
                                             ("bf16", 65, 16, [1, 64, 100, 176])])
def test_contiguous_lists_equal_the_paged_decode_bit_for_bit(dtype, Hq, bs, Ls):
    """indices[t] = the slots of positions 0 .. L_t - 1 of sequence t, padded with -1 to a multiple of 64: both calls plan one split
    (asserted from the two hooks: the table's capacity is at most 191 keys) and run the same tile step on the same image"""
    import torch
    import aule
    from aule import _capi
    B, cap = len(Ls), max(Ls)
    max_blocks = cap // bs
    assert max_blocks * bs == cap <= 191
    nb = B * max_blocks + 3
    p = Problem(41, dtype, B, Hq, nb, bs)
    bt = np.stack([p.rng.permutation(nb)[:max_blocks] for _ in range(B)]).astype(np.int32)
    topk = (cap + 63) // 64 * 64
    idx = np.full((B, topk), -1, dtype=np.int32)
    for b, L in enumerate(Ls):
        idx[b, :L] = aule.paged_slot_mapping(torch.from_numpy(bt), torch.arange(L), bs, seq_ids=torch.full((L,), b)).to(torch.int32).numpy()
    run = Launch(torch, p, idx)
    got = run.run()
    check(p, got, idx, "contiguous lists %s H%d bs%d" % (dtype, Hq, bs))
    # both plans: one split
    assert plan_of(torch, p, B, topk)[2] == 1
    dd = _capi.MlaPagedDesc()
    dd.struct_size = ctypes.sizeof(dd)
    dd.dtype, dd.batch, dd.heads_q, dd.qk_dim, dd.v_dim = DTYPE_CODE[dtype], B, Hq, QK, VD
    dd.block_size, dd.max_blocks, dd.total_tokens, dd.max_seqlen_q, dd.q_token_stride = bs, max_blocks, B, 1, Hq * QK
    dense_plan = (ctypes.c_int32 * 6)()
    assert _capi.load().aule_hip_debug_mla_plan(ctypes.byref(dd), dense_plan, 6) == 6 and dense_plan[2] == 1
    want = aule.flash_attention_mla_paged(run.q, run.kv, torch.from_numpy(bt).cuda(), torch.tensor(Ls, dtype=torch.int32).cuda(), return_lse=True)
    torch.cuda.synchronize()
    assert _same(torch, got, want)


# -------------------------------------------------------------------------------------------------------------------------------- 5. FP8
@pytest.mark.parametrize("dtype,Hq,topk", [("bf16", 16, 200), ("fp16", 65, 129), ("bf16", 128, 512)])
def test_fp8_cache(dtype, Hq, topk):
    """codes from quantize_mla_cache_fp8.  kv_scale = 1: the 16-bit sparse call on codes.to(q.dtype), bit for bit; the quantiser's
    scale (a device tensor): within the bounds of the judge on the dequantised cache"""
    import torch
    import aule
    p = Problem(51, dtype, 3, Hq, 19, 16, fp8=True)
    assert float(p.kv_scale) != 1.0 and math.frexp(float(p.kv_scale))[0] != 0.5   # no power of two
    idx = p.draw(topk)
    idx[1, ::7] = -1
    run = Launch(torch, p, idx)
    got = run.run()
    check(p, got, idx, "fp8 %s H%d topk%d, kv_scale %.4g" % (dtype, Hq, topk, float(p.kv_scale)))
    assert _same(torch, run.python(), got)
    assert _same(torch, run.python(kv_scale=float(p.kv_scale)), got)
    # scale one: `scale` chosen so that the logits are those of the dequantised problem (the codes reach +-448)
    sc = float(p.kv_scale) / math.sqrt(QK)
    one = aule.flash_attention_mla_sparse(run.q, run.kv, run.indices, scale=sc, return_lse=True, kv_scale=1.0)
    none = aule.flash_attention_mla_sparse(run.q, run.kv, run.indices, scale=sc, return_lse=True)
    as16 = aule.flash_attention_mla_sparse(run.q, run.kv.to(run.q.dtype), run.indices, scale=sc, return_lse=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(run.kv.to(run.q.dtype).float()).any())   # the rows nobody names are NaN in both caches
    assert _same(torch, one, as16) and _same(torch, none, as16)


# ------------------------------------------------------------------------------------------------------------------------------ 6. splits
def test_split_lists_whole_splits_empty_and_the_workspace_rule():
    import torch
    from aule import _capi
    p = Problem(61, "bf16", 1, 16, 64, 64)
    topk = 2048
    idx = p.draw(topk)
    rb, rows, nsplit, grid, ws_bytes = plan_of(torch, p, 1, topk)
    assert nsplit > 1 and grid == nsplit and ws_bytes == (nsplit * 16 * 514 * 4 + 15) // 16 * 16
    assert _capi.load().aule_attention_mla_sparse_workspace_size(ctypes.byref(_desc(torch, p, 1, topk))) == ws_bytes
    run = Launch(torch, p, idx, ws_bytes=ws_bytes)           # a caller workspace of exactly the queried size
    got = run.run()
    check(p, got, idx, "split list, nsplit %d, caller workspace" % nsplit)
    assert _same(torch, run.run(), got)                      # two runs: the same bits
    assert _same(torch, run.run(run.desc(ws=False)), got)    # ... and with the library's own workspace
    assert _same(torch, run.python(), got)
    # one 16 bytes smaller: refused, and nothing is launched
    d = run.desc()
    d.workspace_bytes = ws_bytes - 16
    refused = run.run(d, expect=-3)
    assert "workspace_bytes" in str(_capi.get_lib().aule_get_error())
    assert bool((refused[0].view(torch.int16) == -1).all()) and bool((refused[1].view(torch.int32) == -1).all())
    # the second half of the list invalid: whole splits are empty
    half = idx.copy()
    half[:, topk // 2:] = -1
    run2 = Launch(torch, p, half, ws_bytes=ws_bytes)
    got2 = run2.run()
    check(p, got2, half, "split list, second half invalid")
    assert _same(torch, run2.run(), got2)
    # ... and every entry invalid: all of them are
    none = np.full((1, topk), I32_MAX, dtype=np.int32)
    got3 = Launch(torch, p, none, ws_bytes=ws_bytes).run()
    assert bool((got3[0] == 0).all()) and bool(torch.isneginf(got3[1]).all())


def test_forced_split_counts_give_the_same_attention():
    """aule_hip_debug_mla_sparse_launch_nsplit (what the bench measures the plan's split cap with): any count of key ranges is the
    judge's result within the bounds, the plan's own count the entry's bits, and a count past the tiles is clamped to them"""
    import torch
    from aule import _capi
    p = Problem(62, "fp16", 2, 65, 19, 16)
    topk = 500
    idx = p.draw(topk)
    idx[1, 64:192] = -1
    planned = plan_of(torch, p, 2, topk)[2]
    assert planned == 4   # 8 tiles
    run = Launch(torch, p, idx, ws_bytes=(8 * 2 * 65 * 514 * 4 + 15) // 16 * 16)
    want = run.run()
    ref = p.judge(idx)
    lib = _capi.get_lib()
    got = {}
    for n in (1, 3, 4, 8, 64):
        run.arena.fill(POISON)
        assert lib.aule_hip_debug_mla_sparse_launch_nsplit(ctypes.byref(run.desc()), n) == 0, lib.aule_get_error()
        torch.cuda.synchronize()
        assert run.arena.guards_intact(), run.arena.damage()
        got[n] = (run.out.clone(), run.lse.clone())
        check(p, got[n], idx, "forced nsplit %d" % n, ref=ref)
    assert _same(torch, got[planned], want) and _same(torch, got[64], got[8])


# ----------------------------------------------------------------------------------------------------------------------- 7. graph capture
def test_graph_replay_reads_the_current_list_and_scale():
    """one call captured (return_lse, a tensor kv_scale), indices and the scale overwritten, replayed: the eager call on the new
    contents, bit for bit.  (The process keeps the hardware-queue default it was started with.)"""
    import torch
    import aule
    p = Problem(71, "bf16", 2, 16, 19, 16, fp8=True)
    topk = 256
    idx = p.draw(topk)
    run = Launch(torch, p, idx)
    assert plan_of(torch, p, 2, topk)[2] > 1     # attention kernel and combine: two nodes

    def fn():
        return aule.flash_attention_mla_sparse(run.q, run.kv, run.indices, return_lse=True, kv_scale=run.ks)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = fn()
    g.replay()
    torch.cuda.synchronize()
    first = fn()
    assert _same(torch, res, first)
    check(p, res, idx, "graph replay, the captured contents")
    # new contents: a list within the rows that hold data, holes included, and twice the scale
    new = idx[:, ::-1].copy()
    new[0, 5:40] = -1
    new[1, 100:] = I32_MIN
    run.indices.copy_(torch.from_numpy(new).cuda())
    run.ks.mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    eager = fn()
    torch.cuda.synchronize()
    assert _same(torch, res, eager) and not _same(torch, res, first)
    p.kv = p.kv * 2.0
    p.vmax *= 2.0
    check(p, res, new, "graph replay, the new contents")
