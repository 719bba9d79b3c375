"""Which bytes a launch may depend on, and which it may write: every attention entry point of the C-ABI inside a tests/hostile.py
arena -- every pointer in it, guard bands round every tensor, the workspace exactly as large as the size query answers.

Dense (aule_attention_forward_ex, _forward_rope_ex, _backward_ex; the cases of hostile.FWD_CASES / BWD_CASES, one test each):
  R0  guards, outputs and workspace 0x00: the results whose bits everything below is compared with
  R1  guards, outputs and workspace 0xFF (NaN in every format): results bit-identical to R0, every guard byte still 0xFF, every
      input byte as uploaded, the route that ran is the case's; the results are right against the fp64 oracle (bounds of util.py)
  R2  forward with lse = NULL: out bit-identical to R0, the lse region untouched
  I1  all K and V rows of one (batch, kv head) unit are NaN bits, the last unit and then the first: every output of every other
      unit is bit-identical to R0
  I2  all Q rows of one query head are NaN bits (backward: its dO, out and lse rows too): out / lse / dq of every other query head,
      siblings of its GQA group included, and dk / dv of every other unit are bit-identical to R0
Paged (aule_attention_paged_decode_ex, _paged_decode_fp8_ex, _paged_query_ex): the friendly problem of
tests/test_gpu_paged_query.py::Problem against the same problem with NaN bits in every cache slot no (table, length) addresses,
unused table columns pointing at an all-NaN trap block, and out / lse / workspace / guards 0xFF: bit-identical results, guards and
inputs intact, right against the oracle, zeros (lse -inf) for rows that see no key.

A test collects every property that fails and reports them together.  The default dispatch only."""
import ctypes
import os

import numpy as np
import pytest

import hostile
from hostile import BWD_CASES, ELEM, FRIENDLY, FWD_CASES, POISON, Arena, case_id, same_bits
from test_gpu_paged_query import LSE_ATOL, Problem
from util import LSE_TOL, assert_close, fwd_tol, quantize, torch_dtype

pytestmark = pytest.mark.gpu

FULL_ORACLE = 5e7     # B Hq Sq Sk D above which the scalar fp64 oracle takes seconds: 64 sampled rows / one unit instead


@pytest.fixture(scope="module")
def env():
    import torch
    from aule import _capi
    for var in os.environ:   # (the default dispatch; the switches are read once per process)
        assert not var.startswith(("AULE_HIP_FWD_", "AULE_HIP_W4_", "AULE_HIP_BWD_")) and var != "AULE_HIP_F32_SPLIT", var
    return torch, _capi, _capi.get_lib()


def _inputs(case, seed):
    _, dtype, B, Hq, Hkv, Sq, Sk, D, _, _, _ = case
    rng = np.random.RandomState(seed)
    shapes = ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D))
    return [quantize(rng.randn(*s).astype(np.float32), dtype) for s in shapes]     # q, k, v, dout


class _Check:
    """collects the properties that fail"""

    def __init__(self):
        self.failed = []

    def __call__(self, ok, what):
        if not ok:
            self.failed.append(what)
            print("FAILED:", what)

    def close(self, fn, what):
        try:
            fn()
        except AssertionError as e:
            self(False, "%s: %s" % (what, e))

    def arena(self, ar, originals, what):
        self(ar.guards_intact(), "%s: guard bytes written: %r" % (what, ar.damage()))
        for name, orig in originals.items():
            self(ar.unchanged(name, orig), "%s: input %s was written" % (what, name))


def _units(t, nunits):
    """[B, H, S, ...] -> [units, H / (units / B), S, ...]: the heads of one (batch, kv head) unit side by side"""
    B, H = t.shape[:2]
    return t.reshape((nunits, B * H // nunits) + tuple(t.shape[2:]))


def _others_identical(torch, got, want, nunits, skip):
    """every unit but `skip` (per-head tensors: skip is a flat head index when nunits = B * H) is bit-identical"""
    keep = [u for u in range(nunits) if u != skip]
    if not keep:
        return True
    g, w = _units(got, nunits), _units(want, nunits)
    return same_bits(torch, g[keep], w[keep])


def _poisoned(ar, name, dtype, shape, nunits, unit):
    """NaN bits in every row of one unit of an input; returns the bytes to put back"""
    saved = ar.bytes(name).clone()
    _units(ar.view(name, dtype, shape), nunits)[unit].view(ar.torch.uint8).fill_(POISON)
    return saved


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_forward(case, env, oracle_mod):
    torch, _capi, lib = env
    route, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, how = case
    tdt, es = torch_dtype(dtype), ELEM[dtype]
    qn, kn, vn, _ = _inputs(case, 7000 + route)
    d = hostile.fill_problem(_capi.AttnDesc(), case, torch.cuda.current_device())
    d.stream = torch.cuda.current_stream().cuda_stream
    need = int(lib.aule_attention_forward_workspace_size(ctypes.byref(d)))
    regions = [("q", qn.size * es, "in"), ("k", kn.size * es, "in"), ("v", vn.size * es, "in")]
    if how == "rope":
        cos, sin = oracle_mod.rope_tables(Sq, D)
        regions += [("cos", cos.size * 4, "in"), ("sin", sin.size * 4, "in")]
    regions += [("out", qn.size * es, "out"), ("lse", B * Hq * Sq * 4, "out"), ("ws", need, "ws")]
    ar = Arena(torch, regions, D * es)
    orig = {n: ar.upload(n, torch.from_numpy(x).to(tdt)) for n, x in (("q", qn), ("k", kn), ("v", vn))}
    rope = None
    if how == "rope":
        orig["cos"], orig["sin"] = ar.upload("cos", cos), ar.upload("sin", sin)
        rope = _capi.AttnRope()
        rope.struct_size = ctypes.sizeof(rope)
        rope.layout, rope.table_len, rope.table_pitch, rope.q_pos_offset = _capi.ROPE_HALF, Sq, D // 2, 0
        rope.cos, rope.sin = ar.ptr("cos"), ar.ptr("sin")
        assert lib.aule_attention_forward_rope_fusable(ctypes.byref(d), ctypes.byref(rope)) == 1
    d.q, d.k, d.v, d.out = ar.ptr("q"), ar.ptr("k"), ar.ptr("v"), ar.ptr("out")
    if need:
        d.workspace, d.workspace_bytes = ar.ptr("ws"), need
    check = _Check()

    def launch(pattern, what, lse=True):
        ar.fill(pattern)
        d.lse = ar.ptr("lse") if lse else None
        if rope is not None:
            _capi.check(lib.aule_attention_forward_rope_ex(ctypes.byref(d), ctypes.byref(rope)), "aule_attention_forward_rope_ex")
        else:
            _capi.check(lib.aule_attention_forward_ex(ctypes.byref(d)), "aule_attention_forward_ex")
        torch.cuda.synchronize()
        ran = int(lib.aule_hip_debug_last_forward_route())
        check(ran == route, "%s: route %d ran, the case is listed under %d" % (what, ran, route))
        return ar.view("out", tdt, (B, Hq, Sq, D)).clone(), ar.view("lse", torch.float32, (B, Hq, Sq)).clone()

    out0, lse0 = launch(FRIENDLY, "R0")
    out1, lse1 = launch(POISON, "R1")
    check(same_bits(torch, out1, out0), "R1: out depends on what the outputs / the workspace / the guards held")
    check(same_bits(torch, lse1, lse0), "R1: lse depends on what the outputs / the workspace / the guards held")
    check.arena(ar, orig, "R1")
    out2, lse2 = launch(POISON, "R2", lse=False)
    check(same_bits(torch, out2, out0), "R2 (lse = NULL): out differs from R0")
    check(bool((ar.bytes("lse") == POISON).all()), "R2 (lse = NULL): the lse region was written")
    check.arena(ar, orig, "R2")

    # the oracle on R1's results
    qo = quantize(oracle_mod.rope_f64(qn, cos, sin, "half"), dtype) if how == "rope" else qn
    atol, rtol = fwd_tol(dtype, np.abs(vn).max())
    got, got_lse = out1.float().cpu().numpy(), lse1.cpu().numpy()
    if float(B) * Hq * Sq * Sk * D <= FULL_ORACLE:
        ref, ref_lse = oracle_mod.fwd_f64(qo, kn, vn, causal, None, window)
    else:
        rows = np.sort(np.random.RandomState(1).choice(B * Hq * Sq, min(64, B * Hq * Sq), replace=False)).astype(np.int64)
        ref, ref_lse = oracle_mod.fwd_rows_f64(qo, kn, vn, rows, causal, None, window)
        got, got_lse = got.reshape(-1, D)[rows], got_lse.reshape(-1)[rows]
    none = np.isneginf(ref_lse)
    check.close(lambda: assert_close(got, ref, atol, rtol, "out"), "oracle")
    check(np.array_equal(np.isneginf(got_lse), none), "oracle: lse is -inf exactly where a row sees no key")
    check.close(lambda: assert_close(got_lse[~none], ref_lse[~none], LSE_TOL[dtype], LSE_TOL[dtype], "lse"), "oracle")

    units, heads = B * Hkv, B * Hq
    for unit in ((units - 1, 0) if units > 1 else ()):      # I1 (one unit: there is no neighbour)
        what = "I1, K / V of unit %d of %d NaN" % (unit, units)
        saved = [_poisoned(ar, n, tdt, (B, Hkv, Sk, D), units, unit) for n in ("k", "v")]
        o, l = launch(POISON, what)
        check(_others_identical(torch, o, out0, units, unit), what + ": out of another unit changed")
        check(_others_identical(torch, l, lse0, units, unit), what + ": lse of another unit changed")
        check(ar.guards_intact(), what + ": guard bytes written: %r" % (ar.damage(),))
        for n, s in zip(("k", "v"), saved):
            ar.bytes(n).copy_(s)
    if heads > 1:                                           # I2
        head = 1
        what = "I2, Q of head %d of %d NaN" % (head, heads)
        saved = _poisoned(ar, "q", tdt, (B, Hq, Sq, D), heads, head)
        o, l = launch(POISON, what)
        check(_others_identical(torch, o, out0, heads, head), what + ": out of another head changed")
        check(_others_identical(torch, l, lse0, heads, head), what + ": lse of another head changed")
        check(ar.guards_intact(), what + ": guard bytes written: %r" % (ar.damage(),))
        ar.bytes("q").copy_(saved)
    check.arena(ar, orig, "inputs put back")
    assert not check.failed, "\n".join(check.failed)


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_backward(case, env, oracle_mod):
    torch, _capi, lib = env
    from aule import _torch as at
    route, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, how = case
    tdt, es = torch_dtype(dtype), ELEM[dtype]
    qn, kn, vn, don = _inputs(case, 9000 + route)
    d = hostile.fill_problem(_capi.AttnBwdDesc(), case, torch.cuda.current_device())
    d.stream = torch.cuda.current_stream().cuda_stream
    d.q = d.k = d.v = d.out = d.dout = d.lse = d.dq = d.dk = d.dv = 4096      # (the size query reads no pointer)
    need = hostile.bwd_workspace_bytes(lib, d, case)
    qb, kb = qn.size * es, kn.size * es
    ar = Arena(torch, [("q", qb, "in"), ("k", kb, "in"), ("v", kb, "in"), ("dout", qb, "in"), ("out", qb, "in"),
                       ("lse", B * Hq * Sq * 4, "in"), ("dq", qb, "out"), ("dk", kb, "out"), ("dv", kb, "out"), ("ws", need, "ws")], D * es)
    orig = {n: ar.upload(n, torch.from_numpy(x).to(tdt)) for n, x in (("q", qn), ("k", kn), ("v", vn), ("dout", don))}
    # out and lse: the library's own forward on the same inputs
    fo, fl = at.fwd_raw(ar.view("q", tdt, qn.shape), ar.view("k", tdt, kn.shape), ar.view("v", tdt, vn.shape), causal, D ** -0.5,
                        want_lse=True, window=window)
    torch.cuda.synchronize()
    orig["out"], orig["lse"] = ar.upload("out", fo), ar.upload("lse", fl)
    for n in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv"):
        setattr(d, n, ar.ptr(n))
    d.workspace, d.workspace_bytes = ar.ptr("ws"), need
    check = _Check()

    def launch(pattern, what):
        ar.fill(pattern)
        _capi.check(lib.aule_attention_backward_ex(ctypes.byref(d)), "aule_attention_backward_ex")
        torch.cuda.synchronize()
        ran = int(lib.aule_hip_debug_last_backward_route())
        check(ran == route, "%s: route %d ran, the case is listed under %d" % (what, ran, route))
        return [ar.view(n, tdt, s).clone() for n, s in (("dq", qn.shape), ("dk", kn.shape), ("dv", kn.shape))]

    g0 = launch(FRIENDLY, "R0")
    g1 = launch(POISON, "R1")
    for name, a, b in zip(("dq", "dk", "dv"), g1, g0):
        check(same_bits(torch, a, b), "R1: %s depends on what the outputs / the workspace / the guards held" % name)
    check.arena(ar, orig, "R1")

    # the oracle on R1's results
    got = [g.float().cpu().numpy() for g in g1]
    g = Hq // Hkv
    if float(B) * Hq * Sq * Sk * D <= FULL_ORACLE:
        ref = oracle_mod.bwd_f64(qn, kn, vn, don, causal, None, window)
    else:
        b, hk = (B * Hkv // 2) // Hkv, (B * Hkv // 2) % Hkv
        ref = oracle_mod.bwd_head_f64(qn, kn, vn, don, head=(b, hk), causal=causal, window=window)
        got = [got[0][b, hk * g:(hk + 1) * g], got[1][b, hk], got[2][b, hk]]
    for name, a, r in zip(("dq", "dk", "dv"), got, ref):
        check.close(lambda: hostile.grad_close(a, r, dtype, name), "oracle")
    if causal == 1 and Sk > Sq and window <= 0:       # keys no query sees: written, as zeros
        for name, t in zip(("dk", "dv"), g1[1:]):
            check(bool((t[:, :, Sq:] == 0).all()), "R1: %s of the keys no query sees is not zero" % name)

    units, heads = B * Hkv, B * Hq
    for unit in ((units - 1, 0) if units > 1 else ()):      # I1 (one unit: there is no neighbour)
        what = "I1, K / V of unit %d of %d NaN" % (unit, units)
        saved = [_poisoned(ar, n, tdt, (B, Hkv, Sk, D), units, unit) for n in ("k", "v")]
        got = launch(POISON, what)
        for name, a, b in zip(("dq", "dk", "dv"), got, g0):
            check(_others_identical(torch, a, b, units, unit), "%s: %s of another unit changed" % (what, name))
        check(ar.guards_intact(), what + ": guard bytes written: %r" % (ar.damage(),))
        for n, s in zip(("k", "v"), saved):
            ar.bytes(n).copy_(s)
    if heads > 1:                                           # I2
        head = 1
        what = "I2, Q / dO / out / lse of head %d of %d NaN" % (head, heads)
        names = (("q", tdt, qn.shape), ("dout", tdt, qn.shape), ("out", tdt, qn.shape), ("lse", torch.float32, (B, Hq, Sq)))
        saved = [_poisoned(ar, n, t, s, heads, head) for n, t, s in names]
        got = launch(POISON, what)
        check(_others_identical(torch, got[0], g0[0], heads, head), what + ": dq of another head changed")
        for name, a, b in zip(("dk", "dv"), got[1:], g0[1:]):
            check(_others_identical(torch, a, b, units, head // g), "%s: %s of another unit changed" % (what, name))
        check(ar.guards_intact(), what + ": guard bytes written: %r" % (ar.damage(),))
        for (n, _, _), s in zip(names, saved):
            ar.bytes(n).copy_(s)
    check.arena(ar, orig, "inputs put back")
    assert not check.failed, "\n".join(check.failed)


# ------------------------------------------------------------------------------------------------------------------------------------
# entry ("decode" / "query"), dtype, cache kind, B, Hq, Hkv, Sq, D, block size, context lens, window
_DECODE = [
    ("bf16", 3, 8, 2, 64, 16, [37, 0, 1], -1),
    ("fp16", 2, 4, 1, 128, 24, [100, 48], -1),       # the general address path; 48: nothing stale in its last block, the next column trapped
    ("bf16", 2, 4, 4, 32, 128, [130, 5], 20),        # blocks larger than a tile
]
PAGED_CASES = [("decode", dt, kind, B, Hq, Hkv, 1, D, bs, lens, w) for kind in ("16", "fp8") for dt, B, Hq, Hkv, D, bs, lens, w in _DECODE] + [
    ("query", "bf16", "16", 2, 16, 4, 5, 128, 16, [2000, 3], -1),      # the second sequence is shorter than the query
    ("query", "fp16", "fp8", 2, 8, 2, 7, 64, 24, [1500, 100], 16),
    ("query", "bf16", "16", 1, 4, 1, 64, 64, 128, [1100], -1),
]


def _hostile_cache(p, dev, bt):
    """p's device cache with one more block, NaN bits in every slot that (bt, clamped lengths) does not address"""
    nb, bs = dev.shape[:2]
    addressed = np.zeros((nb + 1, bs), dtype=bool)
    for b, n in enumerate(p.clamped_lens()):
        j = np.arange(int(n))
        addressed[bt[b][j // bs], j % bs] = True
    assert not addressed[nb].any()
    bits = np.concatenate([dev, dev[:1]]).copy()
    bits[~addressed] = 0xFF if bits.dtype == np.uint8 else -1
    return bits


@pytest.mark.parametrize("case", PAGED_CASES, ids=lambda c: "%s-%s-kv%s-B%dH%dkv%d-Sq%d-D%d-bs%d-w%d" % (c[:9] + (c[10],)))
def test_paged(case, env, oracle_mod):
    torch, _capi, lib = env
    entry, dtype, kind, B, Hq, Hkv, Sq, D, bs, lens, window = case
    tdt = torch_dtype(dtype)
    p = Problem(51, dtype, kind, B, Hq, Hkv, Sq, D, bs, lens)
    fp8, query = p.fp8, entry == "query"
    nb = p.kdev.shape[0]
    # the caches as the device's bits: e4m3 codes, or the 16-bit patterns
    if fp8:
        kbits, vbits = p.kdev, p.vdev
    else:
        kbits, vbits = (torch.from_numpy(x).to(tdt).view(torch.int16).numpy() for x in (p.kdev, p.vdev))
    nblk = [(n + bs - 1) // bs for n in lens]
    trapped = p.bt.copy()
    for b in range(B):
        trapped[b, nblk[b]:] = nb                      # the trap block
    problems = {
        "friendly": (np.concatenate([kbits, kbits[1:2]]), np.concatenate([vbits, vbits[1:2]]), p.bt, FRIENDLY),
        "hostile": (_hostile_cache(p, kbits, trapped), _hostile_cache(p, vbits, trapped), trapped, POISON),
    }
    d = _capi.PagedQueryDesc() if query else (_capi.PagedFp8Desc() if fp8 else _capi.PagedDesc())
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim = hostile.DTYPE_CODE[dtype], B, Hq, Hkv, D
    d.block_size, d.max_blocks = bs, p.bt.shape[1]
    d.scale, d.window_size, d.device = 0.0, window, torch.cuda.current_device()
    d.stream = torch.cuda.current_stream().cuda_stream
    d.q = d.k_cache = d.v_cache = d.block_tables = d.context_lens = d.out = 4096        # (the size query reads no pointer)
    if query:
        d.seq_q, d.cache_dtype = Sq, 1 if fp8 else 0
    if fp8:
        d.k_scale = d.v_scale = 4096
    size, run = {("decode", False): (lib.aule_attention_paged_decode_workspace_size, lib.aule_attention_paged_decode_ex),
                 ("decode", True): (lib.aule_attention_paged_decode_fp8_workspace_size, lib.aule_attention_paged_decode_fp8_ex),
                 ("query", False): (lib.aule_attention_paged_query_workspace_size, lib.aule_attention_paged_query_ex),
                 ("query", True): (lib.aule_attention_paged_query_workspace_size, lib.aule_attention_paged_query_ex)}[(entry, fp8)]
    need = int(size(ctypes.byref(d)))
    assert need > 0
    es, ces = 2, (1 if fp8 else 2)
    cache_bytes = (nb + 1) * bs * Hkv * D * ces
    regions = [("q", p.q.size * es, "in"), ("k_cache", cache_bytes, "in"), ("v_cache", cache_bytes, "in"),
               ("block_tables", p.bt.size * 4, "in"), ("context_lens", B * 4, "in")]
    if fp8:
        regions += [("k_scale", Hkv * 4, "in"), ("v_scale", Hkv * 4, "in")]
    regions += [("out", p.q.size * es, "out")] + ([("lse", B * Hq * Sq * 4, "out")] if query else []) + [("ws", need, "ws")]
    ar = Arena(torch, regions, max(D * es, Hkv * D * ces))
    for n, _, _ in regions:
        if n != "lse":
            setattr(d, n if n != "ws" else "workspace", ar.ptr(n))
    d.workspace_bytes = need
    if query:
        d.lse = ar.ptr("lse")
    check = _Check()
    res = {}
    for name, (kc, vc, bt, pattern) in problems.items():
        orig = {"q": ar.upload("q", torch.from_numpy(p.q).to(tdt)), "k_cache": ar.upload("k_cache", kc), "v_cache": ar.upload("v_cache", vc),
                "block_tables": ar.upload("block_tables", bt.astype(np.int32)), "context_lens": ar.upload("context_lens", p.cl)}
        if fp8:
            orig["k_scale"] = ar.upload("k_scale", p.ks.astype(np.float32))
            orig["v_scale"] = ar.upload("v_scale", p.vs.astype(np.float32))
        ar.fill(pattern)
        _capi.check(run(ctypes.byref(d)), "paged " + entry)
        torch.cuda.synchronize()
        check.arena(ar, orig, name)
        res[name] = (ar.view("out", tdt, (B, Hq, Sq, D)).clone(),
                     ar.view("lse", torch.float32, (B, Hq, Sq)).clone() if query else None)
    check(same_bits(torch, res["hostile"][0], res["friendly"][0]), "out depends on cache slots / table columns / memory it does not own")
    if query:
        check(same_bits(torch, res["hostile"][1], res["friendly"][1]), "lse depends on cache slots / table columns / memory it does not own")

    # the oracle on the hostile problem's results (the slots it addresses are the friendly problem's)
    out = res["hostile"][0].float().cpu().numpy()
    atol, rtol = fwd_tol(dtype, p.vmax)
    if query:
        lse = res["hostile"][1].cpu().numpy().astype(np.float64)
        ref, lref = p.judge(oracle_mod, window), p.lse_f64(window)
        none = ~np.isfinite(lref)
        check.close(lambda: assert_close(out, ref, atol, rtol, "out"), "oracle")
        check(np.array_equal(np.isneginf(lse), none), "lse is -inf exactly where a row sees no key")
        check(not np.isnan(lse).any(), "lse holds a NaN")
        check(bool((out[none] == 0).all()), "a row that sees no key is zeros")
        lerr = float(np.abs(lse[~none] - lref[~none]).max()) if (~none).any() else 0.0
        print("max |lse err| %.3g (bound %.3g), rows without a key %d" % (lerr, LSE_ATOL, int(none.sum())))
        check(lerr <= LSE_ATOL, "oracle: lse error %.3g > %.3g" % (lerr, LSE_ATOL))
        if case[9] == [2000, 3]:
            check(int(none.sum()) == Hq * 2, "queries 0 and 1 of the second sequence sit at negative positions")
    else:
        ref = oracle_mod.paged_decode_f64(p.q[:, :, 0], p.K, p.V, p.bt, p.clamped_lens(), None, window)
        check.close(lambda: assert_close(out[:, :, 0], ref, atol, rtol, "out"), "oracle")
        for b, n in enumerate(lens):
            if n == 0:
                check(bool((res["hostile"][0][b] == 0).all()), "a sequence of length 0 gives zeros over the poisoned output")
    assert not check.failed, "\n".join(check.failed)
