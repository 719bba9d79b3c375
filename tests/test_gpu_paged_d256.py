"""Paged attention at head_dim 256 on the GPU (csrc/fa_fwd_paged_d256_gfx950.hip behind aule.flash_attention_paged_d256 /
aule_attention_paged_d256_ex): decode, verify and prompt chunks against the paged cache, with key-range splits.

The judge is plain fp64 NumPy, written here (`judge`).  Bars: out within util.fwd_tol(dtype, max |V|), lse within 1e-3
(tests/test_gpu_paged_prefill.py's bound), rows without a key exactly zeros / -inf, rows of no sequence untouched.  Every cache slot no
sequence may read holds NaN, and every table entry past a sequence's last visible block an out-of-range number.  Shapes are the
smallest that reach each path: a block is 64 packed rows (token-major, g = Hq / Hkv heads per token), a wave 32 of them, a key tile 64
keys; block sizes 16 (shift), 24 (divide) and 128 (larger than a tile)."""
import ctypes
import math

import numpy as np
import pytest

from util import assert_close, fwd_tol, torch_dtype

pytestmark = pytest.mark.gpu

D = 256
LSE_ATOL = 1e-3
BAD_BLOCK = 2 ** 30   # a table entry nothing may follow
POISON = 4096.0   # (a bf16 value)


class Case:
    """One seeded ragged batch: sequence b has ns[b] new tokens, Ls[b] keys and a table row for cap[b] keys; `lead` / `tail`: rows of no sequence"""

    def __init__(self, dtype="bf16", fp8=False, Hq=4, Hkv=2, bs=16, ns=(1,), Ls=(100,), cap=None, lead=0, tail=0, seed=0):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.dtype, self.fp8, self.Hq, self.Hkv, self.bs, self.B = dtype, fp8, Hq, Hkv, bs, len(ns)
        cap = [max(x, 1) for x in (Ls if cap is None else cap)]
        nblk = [-(-c // bs) for c in cap]
        pool = sum(nblk) + 3
        perm = torch.randperm(pool, generator=g).tolist()   # shuffled tables
        self.bt = np.full((self.B, max(nblk)), BAD_BLOCK, dtype=np.int32)
        assert all(min(max(L, 0), max(nblk) * bs) <= n * bs for L, n in zip(Ls, nblk))
        self.cu = (lead + np.concatenate([[0], np.cumsum(ns)])).astype(np.int32)
        self.cl = np.array(Ls, dtype=np.int32)
        self.T = int(self.cu[-1]) + tail
        self.max_sq = max(max(ns), 1)
        td = torch_dtype(dtype)
        cd = torch.float8_e4m3fn if fp8 else td
        self.q = (torch.randn(self.T, Hq, D, generator=g) * (0.25 if fp8 else 1.0)).to(td)
        kv = [torch.full((pool, bs, Hkv, D), float("nan")) for _ in range(2)]
        for b in range(self.B):
            live = -(-min(Ls[b], nblk[b] * bs) // bs)   # blocks with a visible key: the others keep BAD_BLOCK
            self.bt[b, :live] = [perm.pop() for _ in range(live)]
            rows = min(max(Ls[b], 0), nblk[b] * bs)
            for x in kv:
                vals = torch.randn(rows, Hkv, D, generator=g).to(cd).float()
                j = torch.arange(rows)
                x[torch.from_numpy(self.bt[b].astype(np.int64))[j // bs], j % bs] = vals
        self.k, self.v = (x.to(cd) for x in kv)   # (exact: the values are the cache type's already)
        self.ks, self.vs = (torch.rand(Hkv, generator=g) * 1.75 + 0.25 for _ in range(2)) if fp8 else (None, None)
        self.dev = {}

    def on_device(self):
        if not self.dev:
            import torch
            to = lambda x: None if x is None else (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).cuda()   # noqa: E731
            self.dev = {n: to(getattr(self, n)) for n in ("q", "k", "v", "bt", "cl", "cu", "ks", "vs")}
        return self.dev


def judge(c, cl=None, cu=None, max_sq=None, window=-1, scale=None, ks=None, vs=None, decode=False):
    """(out [T, Hq, 256], lse [T, Hq], owned [T]) in float64 for the values given (default: the case's own)"""
    cl = c.cl if cl is None else cl
    cu = np.arange(c.B + 1) if decode else c.cu if cu is None else cu
    max_sq = 1 if decode else c.max_sq if max_sq is None else max_sq
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    one = np.ones(c.Hkv)
    ks, vs = (one if x is None else np.asarray(x, dtype=np.float64) for x in ((c.ks if ks is None else ks), (c.vs if vs is None else vs)))
    q, K, V = (x.float().numpy().astype(np.float64) for x in (c.q, c.k, c.v))
    out, lse, owned = np.zeros((c.T, c.Hq, D)), np.full((c.T, c.Hq), -np.inf), np.zeros(c.T, dtype=bool)
    for b in range(c.B):
        L = min(max(int(cl[b]), 0), c.bt.shape[1] * c.bs)
        s = min(max(int(cu[b]), 0), c.T)
        n = min(min(max(int(cu[b + 1]), s), c.T) - s, max_sq)
        owned[s:s + n] = True
        if n == 0 or L == 0:
            continue
        j, p = np.arange(L), L - n + np.arange(n)
        k = K[c.bt[b][j // c.bs], j % c.bs] * ks[None, :, None]
        v = V[c.bt[b][j // c.bs], j % c.bs] * vs[None, :, None]
        see = (j[None] <= p[:, None]) & ((window <= 0) | (p[:, None] - j[None] < window))
        sc = np.einsum("nhgd,lhd->nhgl", q[s:s + n].reshape(n, c.Hkv, -1, D), k) * scale
        sc = np.where(see[:, None, None, :], sc, -np.inf)
        m = sc.max(axis=-1)
        w = np.exp(sc - np.where(np.isfinite(m), m, 0.0)[..., None])
        z = w.sum(axis=-1)
        out[s:s + n] = (np.einsum("nhgl,lhd->nhgd", w, v) / np.where(z > 0, z, 1.0)[..., None]).reshape(n, c.Hq, D)
        with np.errstate(divide="ignore"):
            lse[s:s + n] = np.where(z > 0, m + np.log(z), -np.inf).reshape(n, c.Hq)
    return out, lse, owned, float(np.abs(V[np.isfinite(V)]).max() * np.abs(vs).max())


def run(c, decode=False, nsplit=None, window=-1, scale=None, max_sq=None):
    from aule._torch import paged_d256
    d = c.on_device()
    return paged_d256(d["q"], d["k"], d["v"], d["bt"], d["cl"], None if decode else d["cu"], 1 if decode else (max_sq or c.max_sq), scale=scale,
                      window_size=window, k_scale=d["ks"], v_scale=d["vs"], return_lse=True, force_nsplit=nsplit)


def check(c, got, ref, what):
    out, lse = (x.float().cpu().numpy() for x in got)
    ro, rl, owned, vmax = ref
    atol, rtol = fwd_tol(c.dtype, vmax)
    assert_close(out[owned], ro[owned], atol, rtol, what + " out")
    dark = np.isneginf(rl[owned])
    assert np.array_equal(np.isneginf(lse[owned]), dark), what + ": -inf exactly where a row sees no key"
    assert not out[owned][dark].any(), what + ": a row without a key is zeros"
    assert_close(lse[owned][~dark], rl[owned][~dark], LSE_ATOL, 0.0, what + " lse")


# (id, Case arguments, call arguments).  g * n against 32 / 64: 1, 2, 31, 33, 64, 65, 130; L against the tile and the table
CASES = [
    ("rows-g1-31-33-65", dict(Hq=2, Hkv=2, ns=(31, 33, 65), Ls=(200, 64, 65), bs=24), {}),
    ("rows-g2-130-64-2", dict(Hq=4, Hkv=2, ns=(65, 32, 1), Ls=(130, 63, 1), bs=16, dtype="fp16"), {}),
    ("rows-g8-64-65", dict(Hq=8, Hkv=1, ns=(8, 9), Ls=(200, 65), bs=128), dict(scale=0.11)),
    ("decode-g1", dict(Hq=2, Hkv=2, ns=(1,) * 6, Ls=(0, 1, 63, 64, 65, 200), bs=16), dict(decode=True)),
    ("decode-g2-fp16", dict(Hq=4, Hkv=2, ns=(1,) * 6, Ls=(0, 1, 63, 64, 65, 200), bs=24, dtype="fp16"), dict(decode=True, scale=0.05)),
    ("short-clamped", dict(Hq=4, Hkv=2, ns=(5, 3, 4), Ls=(3, 10000, 200), cap=(3, 208, 200), bs=16), {}),
    ("fp8-general", dict(fp8=True, Hq=4, Hkv=2, ns=(1, 5, 40), Ls=(300, 65, 40), bs=24), {}),
    ("fp8-decode-split", dict(fp8=True, dtype="fp16", Hq=8, Hkv=1, ns=(1, 1), Ls=(5, 700), bs=128), dict(decode=True, nsplit=4)),
] + [("split-%s" % k, dict(Hq=4, Hkv=2, ns=(1, 3), Ls=(5, 1500), bs=16, seed=3), dict(nsplit=k)) for k in (1, 2, 5, 24, None)] + [
    ("plan-batch1", dict(Hq=2, Hkv=1, ns=(1,), Ls=(1500,), bs=128), dict(decode=True)),
] + [("window-%d-n%d%s" % (w, n, "-split" if k else ""), dict(Hq=4, Hkv=2, ns=(n,), Ls=(300,), bs=24, seed=w), dict(window=w, nsplit=k))
     for w, n, k in ((1, 1, None), (64, 5, None), (100, 1, None), (100, 5, 3), (64, 1, 2), (1, 5, None))]


@pytest.mark.parametrize("name,make,call", CASES, ids=[c[0] for c in CASES])
def test_meets_the_judge(name, make, call):
    c = Case(**make)
    ref = judge(c, window=call.get("window", -1), scale=call.get("scale"), decode=call.get("decode", False))
    check(c, run(c, **call), ref, name)


def test_two_runs_of_a_split_call_agree_bit_for_bit():
    import torch
    c = Case(Hq=4, Hkv=2, ns=(1, 3), Ls=(5, 1500), bs=16, seed=3)
    a, b = run(c, nsplit=5), run(c, nsplit=5)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fp8_with_unit_scales_equals_the_16_bit_call_on_the_codes(dtype):
    import torch
    c = Case(fp8=True, dtype=dtype, Hq=4, Hkv=2, ns=(1, 6), Ls=(200, 70), bs=16)
    d = c.on_device()
    d["ks"].fill_(1.0), d["vs"].fill_(1.0)
    got = run(c, nsplit=2)
    d["k"], d["v"], d["ks"], d["vs"] = c.k.float().to(torch_dtype(dtype)).cuda(), c.v.float().to(torch_dtype(dtype)).cuda(), None, None
    same = run(c, nsplit=2)
    assert torch.equal(got[0].view(torch.int16), same[0].view(torch.int16)) and torch.equal(got[1].view(torch.int32), same[1].view(torch.int32))


def test_agrees_with_the_dense_head_dim_256_kernel_on_the_gathered_keys():
    import torch
    import aule
    c = Case(Hq=4, Hkv=2, ns=(40,), Ls=(150,), bs=16)
    d = c.on_device()
    out, _ = run(c)
    j = torch.arange(150, device="cuda")
    k, v = (x[d["bt"][0].long()[j // 16], j % 16].permute(1, 0, 2)[None].contiguous() for x in (d["k"], d["v"]))
    dense = aule.flash_attention(d["q"].permute(1, 0, 2)[None].contiguous(), k, v, causal="bottom-right")[0].permute(1, 0, 2)
    atol, rtol = fwd_tol(c.dtype, float(v.float().abs().max()), sides=2)
    assert_close(out.float().cpu().numpy(), dense.float().cpu().numpy(), atol, rtol, "paged against dense")


def test_graph_replays_read_lengths_offsets_and_scales_as_they_stand():
    import torch
    c = Case(fp8=True, Hq=4, Hkv=2, ns=(4, 2, 6), Ls=(100, 300, 70), bs=16, tail=2)
    d = c.on_device()
    with torch.cuda.stream(torch.cuda.Stream()):
        run(c)   # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run(c)
    states = [(c.cl, c.cu, c.ks.numpy(), c.vs.numpy()),
              (np.array([60, 1, 64], np.int32), np.array([0, 6, 7, 12], np.int32), np.array([0.5, 1.5]), np.array([2.0, 0.25])),
              (np.array([100, 300, 0], np.int32), np.array([2, 3, 9, 9], np.int32), np.array([1.0, 0.3]), np.array([0.7, 1.1]))]
    for i, (cl, cu, ks, vs) in enumerate(states + states[:1]):
        for name, val in (("cl", cl), ("cu", cu), ("ks", ks.astype(np.float32)), ("vs", vs.astype(np.float32))):
            d[name].copy_(torch.from_numpy(val))
        graph.replay()
        torch.cuda.synchronize()
        check(c, got, judge(c, cl=cl, cu=cu, ks=ks, vs=vs), "replay %d" % i)


@pytest.mark.parametrize("fp8", [False, True], ids=["kv16", "fp8"])
def test_c_entry_writes_only_owned_rows_with_a_workspace_of_the_queried_size(fp8):
    """poisoned out / lse, gaps in cu_seqlens_q and a sequence cut by max_seqlen_q: rows of no sequence keep the poison, the others meet the judge"""
    import torch
    from aule import _capi
    c = Case(fp8=fp8, Hq=4, Hkv=2, ns=(3, 9, 1), Ls=(90, 600, 20), bs=24, lead=2, tail=3)
    dv = c.on_device()
    lib = _capi.get_lib()
    out = torch.full((c.T, c.Hq, D), POISON, device="cuda", dtype=torch_dtype(c.dtype))
    lse = torch.full((c.T, c.Hq), POISON, device="cuda", dtype=torch.float32)
    d = _capi.PagedD256Desc()
    d.struct_size, d.dtype, d.cache_dtype = ctypes.sizeof(d), _capi.DTYPE_BF16, _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.batch, d.heads_q, d.heads_kv, d.head_dim = c.B, c.Hq, c.Hkv, D
    d.block_size, d.max_blocks, d.total_tokens, d.max_seqlen_q = c.bs, c.bt.shape[1], c.T, 5
    d.window_size, d.device, d.q_token_stride = -1, -1, c.Hq * D
    d.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name, t in (("q", dv["q"]), ("k_cache", dv["k"]), ("v_cache", dv["v"]), ("block_tables", dv["bt"]), ("context_lens", dv["cl"]),
                    ("cu_seqlens_q", dv["cu"]), ("out", out), ("lse", lse)) + ((("k_scale", dv["ks"]), ("v_scale", dv["vs"])) if fp8 else ()):
        setattr(d, name, t.data_ptr())
    need = int(lib.aule_attention_paged_d256_workspace_size(ctypes.byref(d)))
    plan = (ctypes.c_int32 * 6)()
    assert lib.aule_hip_debug_paged_d256_plan(ctypes.byref(d), plan, 6) == 6 and plan[2] > 1 and need > 0
    ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    assert lib.aule_attention_paged_d256_ex(ctypes.byref(d)) == 0, lib.aule_get_error()
    torch.cuda.synchronize()
    ref = judge(c, max_sq=5)
    check(c, (out, lse), ref, "C entry")
    free = ~ref[2]
    assert free.sum() == 2 + 3 + 4 and (out.float().cpu().numpy()[free] == POISON).all() and (lse.cpu().numpy()[free] == POISON).all()
