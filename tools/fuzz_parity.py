#!/usr/bin/env python3
"""Randomised differential test of the whole forward/backward dispatch against the fp64 oracle: random dtype, batch,
GQA ratio, Sq, Sk, head_dim, causal mode, window and scale sign -- the combinations nobody wrote a case for.
Deterministic per seed; prints every failing configuration.   python tools/fuzz_parity.py [n=200] [seed=0]
Other kinds: `paged`, `rope`, `split` (small grids + fused rotation), `long` (round 6: Sq 2048 / 4096, gradients judged head by head),
`window` (round 6: the window instances of the one-wave-per-SIMD forward -- forward + LSE of every row).
`d256 [n=100] [seed=0]` and `pad [n=100] [seed=0]`: head_dim 256 (csrc/fa_fwd_d256_gfx950.hip, fa_bwd_d256_gfx950.hip) and the head sizes
aule.flash_attention zero-pads, each a pure draw_KIND(rng) -> cfg and a run_KIND(cfg, seed); every failing draw prints the line that runs
it again:   python tools/fuzz_parity.py one d256 "<cfg as printed>" SEED      (below: "d256 and pad").
The paged prefill / query, the paged cascade, the paged MLA and the varlen entries have a tool of their own: tools/fuzz_serving.py."""
import ctypes, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import oracle
from aule import _torch as at, _capi
from util import BWD_TOL, LSE_TOL, fwd_tol, quantize, torch_dtype

def route(dtype, B, Hq, Hkv, Sq, Sk, D, code, W):
    d = _capi.AttnDesc(); d.struct_size = ctypes.sizeof(_capi.AttnDesc)
    d.dtype = {"fp32": 0, "fp16": 1, "bf16": 2}[dtype]
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, Sq, Sk, D
    d.causal, d.window_size = code, W
    return _capi.get_lib().aule_hip_debug_forward_route(ctypes.byref(d))

def grad_grow(dtype, smax):
    """how the gradient bound follows the largest |logit| smax of a problem"""
    if dtype == "fp32": return max(1.0, smax / 8.0)
    # 16-bit gradients at a temperature far above the default (|S| in the tens: the softmax is nearly one-hot, so the 2^-9
    # roundings of P and dS no longer average over many keys): measured worst over 900 draws 1.04e-2 of max|grad| at
    # scale 1.0, D = 128 (|S| ~ 45) against the suite's 1e-2 for the default temperature -- the bound follows |S| gently
    return min(1.5, math.sqrt(smax / 16.0)) if smax > 16.0 else 1.0

def grad_tol(name, dtype, g, Sq, Sk, D, causal, W, scale, grow, wantmax):
    """(atol, rtol) of gradient `name` (dq / dk / dv) of one configuration: |got - want| <= atol + rtol |want|.  From the configuration, the
    logit magnitude (grow = grad_grow(dtype, smax)) and max|want| alone."""
    a, r = BWD_TOL[dtype]
    keys_eff = min(Sk, Sq) if causal == "top" else Sk      # the most keys any row sees
    if W > 0: keys_eff = min(keys_eff, W)
    if dtype == "bf16" and ((scale is not None and abs(scale) * math.sqrt(D) > 2.0) or keys_eff < 32):
        a = 1e-2      # sharp softmax -- a large scale, or so few keys that single weights are O(1) -- (tests/test_gpu_bwd.py, grad_close): the reference's own bar
    # dK / dV accumulate g * Sq rows; where the true gradient vanishes (one key: P = 1, dS = dP - delta cancels
    # exactly) what is left is rounding noise ~ eps |dP| |q| sqrt(rows): plain NumPy fp32 leaves 1.3e-5 at 1600 rows
    acc = max(1.0, math.sqrt(g * Sq / 256.0)) if (dtype == "fp32" and name != "dq") else 1.0
    if dtype == "bf16":
        # the tightened bf16 bound (5e-3 of max|grad|, round 5) was measured on sums over <= ~1000 terms; the 16-bit roundings of dS / P add up like a
        # random walk over the terms a gradient element sums (dQ: Sk keys; dK, dV: g Sq rows): B1 H1 Sq200 Sk5000 D32 reads 6.8e-3 of max|grad| for dQ
        acc = max(1.0, math.sqrt((Sk if name == "dq" else g * Sq) / 512.0))
    return a * grow * acc * max(1.0, wantmax), r

def draw(rng):
    dtype = rng.choice(["bf16", "bf16", "fp16", "fp32"])
    D = int(rng.choice([32, 64, 128]))
    Hkv = int(rng.choice([1, 1, 2, 3, 4, 8])); g = int(rng.choice([1, 1, 2, 4, 8, 5])); Hq = Hkv * g
    B = int(rng.choice([1, 1, 2, 3, 9]))
    Sq = int(rng.choice([1, 1, 2, 3, 7, 16, 17, 31, 33, 64, 65, 100, 200, 256, 257, 300, 512, 700, 1024, 1300]))   # (>= 512: several Q blocks -> the tile stream's seams)
    Sk = int(rng.choice([1, 5, 63, 64, 65, 130, 500, 1023, 1024, 1025, 2047, 2100, 3000, 4096, 5000, 9000]))
    causal = rng.choice(["none", "none", "top", "br", "br"])
    if causal == "br" and Sk < Sq: Sk = Sq + int(rng.choice([0, 1, 100, 1500, 4000]))
    W = int(rng.choice([-1, -1, -1, 1, 7, 64, 100, 1000]))
    scale = None if rng.rand() < 0.7 else float(rng.choice([0.3, -0.2, 0.05, 1.0]))
    # keep the fp64 judge (fwd + bwd ~ 8 B Hq Sq Sk D flops) within ~0.5 s
    while 8.0 * B * Hq * Sq * Sk * D > 6e8:
        if B > 1: B = 1
        elif Hq > Hkv and g > 1: g = max(1, g // 2); Hq = Hkv * g
        elif Hkv > 1: Hkv = 1; Hq = g
        elif Sq > 64 and Sq * 4 > Sk: Sq = Sq // 2
        elif Hq > Hkv and g > 1: g = max(1, g // 2); Hq = Hkv * g
        else: Sk = max(Sq if causal == "br" else 1, Sk // 2)
    return dtype, B, Hq, Hkv, Sq, Sk, D, causal, W, scale

def run(cfg, seed):
    dtype, B, Hq, Hkv, Sq, Sk, D, causal, W, scale = cfg
    cz = {"none": False, "top": True, "br": "bottom-right"}[causal]
    code = {"none": 0, "top": 1, "br": 2}[causal]
    rng = np.random.RandomState(seed)
    q, k, v, do = (quantize(rng.randn(*s).astype(np.float32), dtype) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)))
    sc = (1 / math.sqrt(D)) if scale is None else scale
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(dtype))
    tq, tk, tv, tdo = dev(q), dev(k), dev(v), dev(do)
    out, lse = at.fwd_raw(tq, tk, tv, cz, sc, window=W)
    dq, dk, dv = at.bwd_raw(tq, tk, tv, out, tdo, lse, cz, sc, window=W)
    torch.cuda.synchronize()
    ref, rl = oracle.fwd_f64(q, k, v, cz, scale, W)
    rq, rk, rv = oracle.bwd_f64(q, k, v, do, cz, scale, W)
    errs = []
    o = out.float().cpu().numpy()
    atol, rtol = fwd_tol(dtype, float(np.abs(v).max()))
    # fp32 arithmetic error grows with the logit magnitude (dO ~ 2^-23 |S| |V| through exp): a plain NumPy fp32
    # softmax(QK^T)V is 2e-7 from the fp64 judge at |S| ~ 5 and 1.5e-5 at |S| ~ 53 on the same inputs, like the kernel.
    # The suite's fixed 1e-5 assumes the default temperature; here the scale is random, so the bound follows |S|.
    g = Hq // Hkv
    smax = max(float(np.abs(q[b, h] @ k[b, h // g].T).max()) for b in range(B) for h in range(Hq)) * abs(sc)
    if dtype == "fp32": atol += 2.0 ** -22 * smax * float(np.abs(v).max())
    grow = grad_grow(dtype, smax)
    if not np.isfinite(o).all(): errs.append("out non-finite")
    elif (np.abs(o - ref) > atol + rtol * np.abs(ref)).any(): errs.append(f"out err {np.abs(o-ref).max():.3e}")
    gl = lse.cpu().numpy(); fin = np.isfinite(rl)
    if not np.all(np.isneginf(gl[~fin])): errs.append("lse of empty rows not -inf")
    if fin.any() and np.abs(gl[fin] - rl[fin]).max() > LSE_TOL[dtype] + 1e-5 * np.abs(rl[fin]).max(): errs.append(f"lse err {np.abs(gl[fin]-rl[fin]).max():.3e}")
    for name, got, want in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        gg = got.float().cpu().numpy()
        if not np.isfinite(gg).all(): errs.append(name + " non-finite"); continue
        tol, r = grad_tol(name, dtype, g, Sq, Sk, D, causal, W, scale, grow, float(np.abs(want).max()))
        if (np.abs(gg - want) > tol + r * np.abs(want)).any(): errs.append(f"{name} err {np.abs(gg-want).max():.3e} (tol {tol:.1e})")
    return route(dtype, B, Hq, Hkv, Sq, Sk, D, code, W), errs

def run_paged(rng, i):
    """Random paged-decode problem against oracle.paged_decode_f64: shuffled block tables, ragged lengths (0 and 1
    included), power-of-two and other block sizes, GQA ratios, window."""
    import aule
    dtype = rng.choice(["bf16", "fp16"])
    D = int(rng.choice([32, 64, 128])); Hkv = int(rng.choice([1, 2, 4, 8])); g = int(rng.choice([1, 2, 4, 8, 16])); Hq = Hkv * g
    B = int(rng.choice([1, 2, 3, 5, 8])); bs = int(rng.choice([1, 3, 8, 16, 24, 32, 33, 64, 100, 128]))
    lens = [int(rng.choice([0, 1, 2, bs, bs + 1, 31, 32, 33, 100, 777, 1500, 4000])) for _ in range(B)]
    W = int(rng.choice([-1, -1, 1, 17, 256]))
    scale = None if rng.rand() < 0.7 else float(rng.choice([0.3, -0.2]))
    nblk = [(n + bs - 1) // bs for n in lens]
    num_blocks = sum(nblk) + int(rng.choice([0, 1, 5]))
    num_blocks = max(num_blocks, 1)
    r2 = np.random.RandomState(5000 + i)
    q = quantize(r2.randn(B, Hq, D).astype(np.float32), dtype)
    kc = quantize(r2.randn(num_blocks, bs, Hkv, D).astype(np.float32), dtype)
    vc = quantize(r2.randn(num_blocks, bs, Hkv, D).astype(np.float32), dtype)
    bt = np.zeros((B, max(max(nblk), 1) + int(rng.choice([0, 2]))), dtype=np.int32)
    perm = r2.permutation(num_blocks); used = 0
    for b in range(B):
        bt[b, :nblk[b]] = perm[used:used + nblk[b]]; used += nblk[b]
    cl = np.array(lens, dtype=np.int32)
    dt = torch_dtype(dtype)
    out = aule.flash_attention_paged_amd(torch.from_numpy(q).to("cuda", dt), torch.from_numpy(kc).to("cuda", dt),
                                         torch.from_numpy(vc).to("cuda", dt), torch.from_numpy(bt).cuda(), torch.from_numpy(cl).cuda(),
                                         scale=scale, window_size=W).float().cpu().numpy()
    ref = oracle.paged_decode_f64(q, kc, vc, bt, cl, scale, W)
    atol, rtol = fwd_tol(dtype, float(np.abs(vc).max()))
    cfg = (dtype, B, Hq, Hkv, D, bs, lens, W, scale)
    if not np.isfinite(out).all(): return cfg, ["non-finite"]
    bad = np.abs(out - ref) > atol + rtol * np.abs(ref)
    return cfg, ([f"err {np.abs(out-ref).max():.3e}"] if bad.any() else [])


def run_rope(rng, i):
    """Random RoPE pass against oracle.rope_f64: dtype, layout, inverse, offset, vector and scalar head dims, in place."""
    dtype = rng.choice(["bf16", "fp16", "fp32"])
    B, H, S = int(rng.choice([1, 2, 3])), int(rng.choice([1, 2, 5, 8])), int(rng.choice([1, 2, 31, 64, 100, 333]))
    D = int(rng.choice([2, 6, 16, 20, 32, 48, 64, 80, 96, 128]))
    layout = rng.choice(["half", "interleaved"]); inverse = bool(rng.rand() < 0.4); off = int(rng.choice([0, 0, 1, 7, 50]))
    r2 = np.random.RandomState(7000 + i)
    x = quantize(r2.randn(B, H, S, D).astype(np.float32), dtype)
    cos, sin = oracle.rope_tables(S + off + int(rng.choice([0, 3])), D)
    want = oracle.rope_f64(x, cos, sin, layout, inverse, off)
    dev = lambda a, d="fp32": torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(d))
    tx = dev(x, dtype)
    got = at.rope_raw(tx, dev(cos), dev(sin), layout, inverse, off)
    at.rope_raw(tx, dev(cos), dev(sin), layout, inverse, off, out=tx)
    tol = {"fp32": 2e-6, "fp16": 2e-3, "bf16": 1.6e-2}[dtype] * max(1.0, float(np.abs(want).max()))
    cfg = (dtype, B, H, S, D, layout, inverse, off)
    errs = []
    if np.abs(got.float().cpu().numpy() - want).max() > tol: errs.append(f"err {np.abs(got.float().cpu().numpy()-want).max():.3e}")
    if not torch.equal(tx, got): errs.append("in place != out of place")
    return cfg, errs


def run_split(rng, i):
    """Small grids with long keys (route 7: pairs of causal Q blocks, or non-causal blocks, cut into pieces + merge) and, on
    the same draw, the fused query rotation against the two-pass form.  Forward only (out + LSE vs the fp64 judge): the
    shapes that reach this route cost the judge seconds each."""
    dtype = rng.choice(["bf16", "fp16"])
    D = int(rng.choice([64, 128])); Hkv = int(rng.choice([1, 2, 4])); g = int(rng.choice([1, 2, 4])); Hq = Hkv * g
    Sq = int(rng.randint(1100, 3200)); causal = rng.choice(["none", "top", "br"])
    Sk = Sq if causal == "top" and rng.rand() < 0.7 else int(Sq + rng.choice([0, 1, 63, 500, 2000]))
    if causal == "none" and rng.rand() < 0.5: Sk = int(rng.randint(2048, 5000))
    scale = None if rng.rand() < 0.7 else float(rng.choice([0.3, -0.2, 0.05]))
    cz = {"none": False, "top": True, "br": "bottom-right"}[causal]
    code = {"none": 0, "top": 1, "br": 2}[causal]
    r = route(dtype, 1, Hq, Hkv, Sq, Sk, D, code, -1)
    cfg = (dtype, 1, Hq, Hkv, Sq, Sk, D, causal, scale)
    r2 = np.random.RandomState(9000 + i)
    q, k, v = (quantize(r2.randn(*s).astype(np.float32), dtype) for s in ((1, Hq, Sq, D), (1, Hkv, Sk, D), (1, Hkv, Sk, D)))
    sc = (1 / math.sqrt(D)) if scale is None else scale
    dev = lambda a, d=dtype: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(d))
    tq, tk, tv = dev(q), dev(k), dev(v)
    out, lse = at.fwd_raw(tq, tk, tv, cz, sc)
    ref, rl = oracle.fwd_f64(q, k, v, cz, scale, -1)
    errs = []
    atol, rtol = fwd_tol(dtype, float(np.abs(v).max()))
    o = out.float().cpu().numpy()
    if not np.isfinite(o).all(): errs.append("out non-finite")
    elif (np.abs(o - ref) > atol + rtol * np.abs(ref)).any(): errs.append(f"out err {np.abs(o-ref).max():.3e}")
    if np.abs(lse.cpu().numpy() - rl).max() > LSE_TOL[dtype] + 1e-5 * np.abs(rl).max(): errs.append(f"lse err {np.abs(lse.cpu().numpy()-rl).max():.3e}")
    # fused query rotation == rope(Q) pass + attention, bit for bit, whenever both launches take the plain tile stream
    qoff = Sk - Sq if causal == "br" else 0
    cos, sin = oracle.rope_tables(max(Sq + qoff, Sk) + 2, D)
    tc, ts = dev(cos, "fp32"), dev(sin, "fp32")
    if at.rope_fusable(tq, tk, code, -1, tc, ts, qoff, sc):
        fused = at.fwd_raw(tq, tk, tv, cz, sc, want_lse=False, q_rope=(tc, ts, qoff))[0]
        qr = at.rope_raw(tq, tc, ts, "half", False, qoff)
        two = at.fwd_raw(qr, tk, tv, cz, sc, want_lse=False)[0]
        if r == 6:
            if not torch.equal(fused, two): errs.append("fused rotation != two-pass (same kernel)")
        elif (fused.float() - two.float()).abs().max().item() > 2 * atol + 0.02: errs.append("fused rotation far from two-pass")
    return (r, cfg), errs


def run_long(rng, i):
    """Round 6: the sizes the backward's longest streams run -- Sq in {2048, 4096}, 16-bit, D 64 / 128, MHA and GQA,
    every causal mode, causal windows -- forward (sampled rows) AND backward against the fp64 judges.  The whole-problem C judge
    would take minutes per draw here; gradients are checked head by head (oracle.bwd_head_f64: one KV head + its query group at
    full S) on two random (batch, kv-head) units, the forward on 48 sampled rows (oracle.fwd_rows_f64)."""
    dtype = rng.choice(["bf16", "bf16", "fp16"])
    D = int(rng.choice([64, 128, 128])); Hkv = int(rng.choice([1, 2, 4, 8])); g = int(rng.choice([1, 1, 2, 4])); Hq = Hkv * g
    B = int(rng.choice([1, 2, 4]))
    Sq = int(rng.choice([2048, 4096, 4096, 2048 + 77, 4096 - 131]))
    causal = rng.choice(["none", "top", "top", "br"])
    Sk = Sq if rng.rand() < 0.6 else int(rng.choice([2048, 4096, 5000, 8192]))
    if causal == "br" and Sk < Sq: Sk = Sq + int(rng.choice([0, 100, 4000]))
    W = int(rng.choice([-1, -1, -1, 256, 1024])) if causal != "none" else -1
    scale = None if rng.rand() < 0.8 else float(rng.choice([0.05, 0.12]))
    cz = {"none": False, "top": True, "br": "bottom-right"}[causal]
    code = {"none": 0, "top": 1, "br": 2}[causal]
    cfg = (dtype, B, Hq, Hkv, Sq, Sk, D, causal, W, scale)
    sc = (1 / math.sqrt(D)) if scale is None else scale
    gen = torch.Generator(device="cuda").manual_seed(11000 + i)
    dt = torch_dtype(dtype)
    tq, tdo = (torch.randn(B, Hq, Sq, D, device="cuda", dtype=dt, generator=gen) for _ in range(2))
    tk, tv = (torch.randn(B, Hkv, Sk, D, device="cuda", dtype=dt, generator=gen) for _ in range(2))
    out, lse = at.fwd_raw(tq, tk, tv, cz, sc, window=W)
    dq, dk, dv = at.bwd_raw(tq, tk, tv, out, tdo, lse, cz, sc, window=W)
    torch.cuda.synchronize()
    errs = []
    r2 = np.random.RandomState(12000 + i)
    a, r = BWD_TOL[dtype]
    keys_eff = min(Sk, Sq) if causal == "top" else Sk
    if W > 0: keys_eff = min(keys_eff, W)
    for _ in range(2):
        b, hk = int(r2.randint(B)), int(r2.randint(Hkv))
        f = lambda t, hh=slice(hk * g, (hk + 1) * g): t[b, hh].float().cpu().numpy()
        rq, rk, rv = oracle.bwd_head_f64(f(tq), f(tk, hk), f(tv, hk), f(tdo), None, cz, scale, W)
        for name, got, want in (("dq", f(dq), rq), ("dk", f(dk, hk), rk), ("dv", f(dv, hk), rv)):
            if not np.isfinite(got).all(): errs.append(f"{name}[{b},{hk}] non-finite"); continue
            # (the accumulation-length term of run(): a gradient element sums Sk keys (dQ) or g Sq rows (dK, dV) of 16-bit-rounded terms)
            acc = max(1.0, math.sqrt(min(keys_eff if name == "dq" else g * Sq, 8192) / 512.0)) if dtype == "bf16" else 1.0
            tol = a * acc * max(1.0, float(np.abs(want).max()))
            e = np.abs(got - want)
            if (e > tol + r * np.abs(want)).any(): errs.append(f"{name}[{b},{hk}] err {e.max():.3e} = {e.max()/max(1.0, float(np.abs(want).max())):.2e} of max|grad| (tol {tol:.1e})")
    rows = r2.randint(0, B * Hq * Sq, size=48).astype(np.int64)
    qf, kf, vf = (t.float().cpu().numpy() for t in (tq, tk, tv))
    ro, rl = oracle.fwd_rows_f64(qf, kf, vf, rows, cz, scale, W)
    o = out.float().cpu().numpy().reshape(-1, D)[rows]; gl = lse.cpu().numpy().reshape(-1)[rows]
    atol, rtol = fwd_tol(dtype, float(np.abs(vf).max()))
    fin = np.isfinite(rl)
    if (np.abs(o - ro) > atol + rtol * np.abs(ro)).any(): errs.append(f"out err {np.abs(o-ro).max():.3e}")
    if fin.any() and np.abs(gl[fin] - rl[fin]).max() > LSE_TOL[dtype] + 1e-5 * np.abs(rl[fin]).max(): errs.append(f"lse err {np.abs(gl[fin]-rl[fin]).max():.3e}")
    return (route(dtype, B, Hq, Hkv, Sq, Sk, D, code, W), cfg), errs


def run_window(rng, i):
    """Round 6: causal sliding windows on the one-wave-per-SIMD forward's window instances (fa_fwd_w4_gfx950.hip WIN): 16-bit, D 64 / 128, top-left
    and bottom-right causal with offsets that are no tile multiples, windows from 128 keys to beyond the sequence -- aligned and not --, ragged
    last blocks, GQA; one draw in four with a key whose logit towers over its head's, placed at random (in front of some rows' windows, inside
    others': the fixed reference under- or overflows and the exact-maximum stream has to repair those parts).  Every output row and LSE
    against the fp64 judge."""
    dtype = rng.choice(["bf16", "bf16", "fp16"])
    D = int(rng.choice([64, 128, 128])); Hkv = int(rng.choice([1, 2, 4])); g = int(rng.choice([1, 1, 2, 4])); Hq = Hkv * g
    B = int(rng.choice([1, 1, 2]))
    Sq = int(rng.choice([257, 300, 512, 513, 700, 1000, 1024, 1100, 1536, 2048, 2048 + 77, 3000]))
    causal = rng.choice(["top", "top", "br"])
    Sk = Sq if causal == "top" else Sq + int(rng.choice([0, 1, 63, 64, 100, 1000, 2049]))
    W = int(rng.choice([128, 129, 191, 192, 200, 255, 256, 257, 300, 511, 512, 640, 1000, 1024, 1500, 2500]))
    scale = None if rng.rand() < 0.8 else float(rng.choice([0.05, 0.2]))
    while 4.0 * B * Hq * Sq * Sk * D > 1.2e9:       # (the fp64 judge within ~1 s)
        if B > 1: B = 1
        elif g > 1: g //= 2; Hq = Hkv * g
        elif Hkv > 1: Hkv //= 2; Hq = Hkv * g
        else: break
    cz = {"top": True, "br": "bottom-right"}[causal]
    code = {"top": 1, "br": 2}[causal]
    spike = rng.rand() < 0.25
    cfg = (dtype, B, Hq, Hkv, Sq, Sk, D, causal, W, scale, "spike" if spike else "")
    r2 = np.random.RandomState(21000 + i)
    q, k, v = (quantize(r2.randn(*s).astype(np.float32), dtype) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D)))
    if spike:
        row, key = int(r2.randint(Sq)), int(r2.randint(Sk))
        k[:, 0, key, :] = quantize((20.0 * q[:, 0, row, :]).astype(np.float32), dtype)
    sc = (1 / math.sqrt(D)) if scale is None else scale
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(dtype))
    out, lse = at.fwd_raw(dev(q), dev(k), dev(v), cz, sc, window=W)
    torch.cuda.synchronize()
    ref, rl = oracle.fwd_f64(q, k, v, cz, scale, W)
    errs = []
    o = out.float().cpu().numpy(); gl = lse.cpu().numpy()
    atol, rtol = fwd_tol(dtype, float(np.abs(v).max()))
    if not np.isfinite(o).all(): errs.append("out non-finite")
    elif (np.abs(o - ref) > atol + rtol * np.abs(ref)).any(): errs.append(f"out err {np.abs(o-ref).max():.3e}")
    smax = abs(sc) * float(np.abs((q[:, 0, row, :].astype(np.float64) * k[:, 0, key, :]).sum(-1)).max()) if spike else 1.0   # (LSE at |S| in the hundreds: fp32 arithmetic)
    if np.abs(gl - rl).max() > LSE_TOL[dtype] * max(1.0, smax / 64.0) + 1e-5 * np.abs(rl).max(): errs.append(f"lse err {np.abs(gl-rl).max():.3e}")
    return (route(dtype, B, Hq, Hkv, Sq, Sk, D, code, W), cfg), errs


# ------------------------------------------------------------------------------------------------- d256 and pad: the draws (pure)
# head_dim 256 (csrc/fa_fwd_d256_gfx950.hip, fa_bwd_d256_gfx950.hip) and the head sizes aule.flash_attention zero-pads.  As in
# tools/fuzz_serving.py a kind is a pure draw -- draw_KIND(rng) -> cfg, a dict of plain values with eval(repr(cfg)) == cfg -- and a run,
# run_KIND(cfg, seed) -> (route, errs); dense_reference(cfg, seed) is everything of a run that needs no GPU.  The lists are the smallest
# shapes on both sides of each seam of these kernels: query blocks of 128 rows = 4 x 32, key tiles of 64 (forward, dQ), key blocks of 128
# with 32-row query tiles (dK/dV).
D256_G, D256_HKV, D256_B = [1, 2, 3, 5, 8], [1, 2, 3], [1, 2, 3]
D256_SQ = [1, 2, 31, 32, 33, 64, 127, 128, 129, 200, 257, 300]
D256_SK = [1, 2, 31, 63, 64, 65, 127, 128, 129, 191, 257, 300, 513, 1025]
D256_BR_AHEAD = [0, 1, 37, 100]        # bottom-right with Sk < Sq drawn: Sk = Sq + one of these (an offset off the tile grid)
D256_W = [-1, -1, 1, 7, 63, 64, 65, 100, 200]
D256_SCALES = [0.3, -0.2, 0.02, 0.1, 0.0]
D256_BUDGET = 3e8                      # 8 B Hq Sq Sk D flops of the scalar fp64 judge (forward + backward): ~0.25 s
PAD_D = [8, 40, 72, 96, 120, 136, 160, 192, 224, 248]
PAD_SQ, PAD_SK, PAD_W, PAD_SCALE = [2, 31, 33, 64, 129, 200], [2, 63, 65, 129, 257], [-1, -1, 7, 64, 100], 0.1
SPIKE_PLACES = ("first", "last", "edge")


def _pick(rng, xs):
    return xs[int(rng.randint(len(xs)))]


def _smaller(xs, x):
    """the next smaller member of the sorted list xs (x itself when it is the smallest)"""
    lower = [y for y in xs if y < x]
    return lower[-1] if lower else x


def row_keys(c, i):
    """(lo, hi): the keys lo .. hi query row i of configuration c sees (none when hi < lo) -- the oracle's mask rule"""
    pos = i + (c["Sk"] - c["Sq"] if c["causal"] == "br" else 0)
    hi = c["Sk"] - 1 if c["causal"] == "none" else min(pos, c["Sk"] - 1)
    lo = max(0, pos - c["W"] + 1) if c["W"] > 0 else 0
    return lo, hi


def blind_rows(c):
    """query rows that see no key"""
    return [i for i in range(c["Sq"]) if row_keys(c, i)[1] < row_keys(c, i)[0]]


def unseen_keys(c):
    """keys no query row sees"""
    seen = [False] * c["Sk"]
    for i in range(c["Sq"]):
        lo, hi = row_keys(c, i)
        for j in range(lo, hi + 1): seen[j] = True
    return [j for j in range(c["Sk"]) if not seen[j]]


def _shrink(c, g, D):
    """g, then Hkv, then B, then Sk, each to the next smaller member of its list, until the judge's cost is within D256_BUDGET"""
    sks = sorted(set(D256_SK + PAD_SK + ([c["Sq"] + a for a in D256_BR_AHEAD] if c["causal"] == "br" else [])))
    if c["causal"] == "br": sks = [x for x in sks if x >= c["Sq"]]
    while 8.0 * c["B"] * c["Hkv"] * g * c["Sq"] * c["Sk"] * D > D256_BUDGET:
        if g > 1: g = _smaller(D256_G, g)
        elif c["Hkv"] > 1: c["Hkv"] = _smaller(D256_HKV, c["Hkv"])
        elif c["B"] > 1: c["B"] = _smaller(D256_B, c["B"])
        elif _smaller(sks, c["Sk"]) < c["Sk"]: c["Sk"] = _smaller(sks, c["Sk"])
        else: break
    c["Hq"] = c["Hkv"] * g


def draw_d256(rng):
    """One head_dim 256 configuration.  One draw in three carries hard data (`hard`; forward and LSE only, 16-bit dtypes only):
    ("spike", logit, b, head, row, key, place) -- key `key` of that row's KV head becomes m q[b, head, row] with m such that the pair's logit
    is `logit` (155 .. 245 in natural units at the draw's scale), the key in the first or the last 64-key tile the row sees or on a tile
    edge (key % 64 in {0, 63}), the row one that sees at least two keys -- or ("offset", c, kv head): c added to every key of one KV head."""
    c = {}
    c["dtype"] = _pick(rng, ["bf16", "bf16", "fp16", "fp32"])
    c["Hkv"], g, c["B"] = _pick(rng, D256_HKV), _pick(rng, D256_G), _pick(rng, D256_B)
    c["Sq"], c["Sk"] = _pick(rng, D256_SQ), _pick(rng, D256_SK)
    c["causal"] = _pick(rng, ["none", "top", "br"])
    if c["causal"] == "br" and c["Sk"] < c["Sq"]: c["Sk"] = c["Sq"] + _pick(rng, D256_BR_AHEAD)
    c["W"] = _pick(rng, D256_W)
    c["scale"] = None if int(rng.randint(10)) < 6 else _pick(rng, D256_SCALES)
    hard = int(rng.randint(3)) == 0
    if hard:
        if c["dtype"] == "fp32": c["dtype"] = _pick(rng, ["bf16", "fp16"])
        if c["scale"] == 0.0: c["scale"] = None        # (at scale 0 no key can tower: every logit is 0)
    _shrink(c, g, 256)
    c["hard"] = None
    if hard:
        rows = [i for i in range(c["Sq"]) if row_keys(c, i)[1] > row_keys(c, i)[0]]
        if int(rng.randint(2)) == 0 and rows:
            i = _pick(rng, rows)
            lo, hi = row_keys(c, i)
            keys = dict(first=list(range(lo, min(hi, lo // 64 * 64 + 63) + 1)), last=list(range(max(lo, hi // 64 * 64), hi + 1)),
                        edge=[j for j in range(lo, hi + 1) if j % 64 in (0, 63)])
            place = _pick(rng, [p for p in SPIKE_PLACES if keys[p]])
            c["hard"] = ("spike", round(float(rng.uniform(155.0, 245.0)), 1), int(rng.randint(c["B"])), int(rng.randint(c["Hq"])), i,
                         _pick(rng, keys[place]), place)
        else:
            c["hard"] = ("offset", float(_pick(rng, [2, 4])), int(rng.randint(c["Hkv"])))
    return c


def draw_pad(rng):
    """One configuration of a head size that aule.flash_attention zero-pads (to 32 / 64 / 128 / 256), run through the public entry with
    autograd.  Shapes in which some row sees two keys; a default-scale draw is fp32, an explicit-scale draw (PAD_SCALE) bf16 or fp16: what a
    default-scale draw is for is the scale -- 1/sqrt(D) of the true D, taken before the padding and whatever the dtype -- and only the fp32
    tolerance is tight enough for 1/sqrt(Dp) to land 20 x the tolerance away at every size: softmax weights move by at most
    0.224 (1 - sqrt(D / Dp)) between two keys, 0.0036 at D = 248, which is below bf16's rounding of P whatever the data."""
    c = {}
    c["D"] = _pick(rng, PAD_D)
    c["scale"] = None if int(rng.randint(2)) == 0 else PAD_SCALE
    dtype = _pick(rng, ["bf16", "fp16"])
    c["dtype"] = "fp32" if c["scale"] is None else dtype
    c["Hkv"], g, c["B"] = _pick(rng, [1, 2]), _pick(rng, [1, 2, 3]), _pick(rng, [1, 2])
    c["Sq"], c["Sk"] = _pick(rng, PAD_SQ), _pick(rng, PAD_SK)
    c["causal"] = _pick(rng, ["none", "top", "br"])
    if c["causal"] == "br" and c["Sk"] < c["Sq"]: c["Sk"] = c["Sq"] + _pick(rng, D256_BR_AHEAD)
    c["W"] = _pick(rng, PAD_W)
    _shrink(c, g, c["D"])
    c["hard"] = None
    return c


# The fixed-seed slices of the suite (tests/test_gpu_fuzz.py runs them, tests/test_fuzz_d256_draws.py keeps the seeds chosen for what they
# reach): slice -> (kind, draws, seed of the draw stream, which draws of the stream: hard / Gaussian / all).
SLICES = dict(d256=("d256", 24, 20, False), d256_hard=("d256", 12, 6, True), pad=("pad", 12, 839, None))
SEED0 = dict(d256=41000, d256_hard=41500, pad=42000)          # data seed of draw i of a slice: SEED0[slice] + i
DRAW = dict(d256=draw_d256, pad=draw_pad)


def draws(kind, n, seed, hard=None):
    """the first n configurations of `kind` at `seed` (hard: True / False keeps the hard / the Gaussian draws of the stream); pure"""
    rng, res = np.random.RandomState(seed), []
    while len(res) < n:
        c = DRAW[kind](rng)
        if hard is None or (c["hard"] is not None) == hard: res.append(c)
    return res


def slice_draws(name):
    """[(cfg, data seed)] of a suite slice"""
    kind, n, seed, hard = SLICES[name]
    return [(c, SEED0[name] + i) for i, c in enumerate(draws(kind, n, seed, hard))]


# ------------------------------------------------------------------------------------------- d256 and pad: the reference side (no GPU)
CZ = {"none": False, "top": True, "br": "bottom-right"}


def _softmax_f64(q, k, vis, sc, g):
    """P [B, Hq, Sq, Sk] in fp64 (rows without a visible key: zeros)"""
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), np.repeat(k, g, axis=1).astype(np.float64)) * sc
    s = np.where(vis, s, -np.inf)
    m = s.max(axis=-1, keepdims=True)
    e = np.exp(s - np.where(np.isfinite(m), m, 0.0))
    den = e.sum(axis=-1, keepdims=True)
    return e / np.where(den > 0, den, 1.0)


def lse_np(q, k, vis, sc, g, ft):
    """[B, Hq, Sq] log-sum-exp of the visible logits in plain NumPy arithmetic of type ft (-inf where a row sees none)"""
    s = np.einsum("bhqd,bhkd->bhqk", q.astype(ft), np.repeat(k, g, axis=1).astype(ft)) * ft(sc)
    s = np.where(vis, s, ft(-np.inf))
    m = s.max(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = m + np.log(np.exp(s - np.where(np.isfinite(m), m, ft(0.0))[..., None]).sum(axis=-1))
    return np.where(np.isfinite(m), val, -np.inf).astype(np.float64)


def delta_model(q, k, v, do, vis, sc, g, dtype):
    """(e_dq, e_dk) [B, Hkv]: the largest |g_model - g| per (batch, KV head) of dq (over the head's query group) and dk, g the fp64
    gradient formula dS = P (dP - delta) and g_model the same with delta = rowsum(dO * O) from O rounded to the storage dtype -- what the
    backward entry is given (test_gpu_mla_backward.rounding_model, test_gpu_sinks.grads_model).  dv = P^T dO reads no delta."""
    B, Hq, Sq, D = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    q64, do64 = q.astype(np.float64), do.astype(np.float64)
    kk, vv = np.repeat(k, g, axis=1).astype(np.float64), np.repeat(v, g, axis=1).astype(np.float64)
    P = _softmax_f64(q, k, vis, sc, g)
    O, dP = np.einsum("bhqk,bhkd->bhqd", P, vv), np.einsum("bhqd,bhkd->bhqk", do64, vv)
    res = []
    for Ouse in (O, quantize(O.astype(np.float32), dtype).astype(np.float64)):
        dS = P * (dP - (do64 * Ouse).sum(axis=-1, keepdims=True)) * sc
        res.append((np.einsum("bhqk,bhkd->bhqd", dS, kk), np.einsum("bhqk,bhqd->bhkd", dS, q64).reshape(B, Hkv, g, Sk, D).sum(axis=2)))
    e_dq = np.abs(res[1][0] - res[0][0]).reshape(B, Hkv, -1).max(axis=-1)
    e_dk = np.abs(res[1][1] - res[0][1]).reshape(B, Hkv, -1).max(axis=-1)
    return e_dq, e_dk


def dense_inputs(c, seed):
    """q, k, v, dout of a d256 / pad configuration, quantised to its dtype, the hard-data treatment applied; and the spiked pair's logit"""
    D, dtype = c.get("D", 256), c["dtype"]
    rng = np.random.RandomState(seed)
    shapes = ((c["B"], c["Hq"], c["Sq"], D), (c["B"], c["Hkv"], c["Sk"], D), (c["B"], c["Hkv"], c["Sk"], D), (c["B"], c["Hq"], c["Sq"], D))
    q, k, v, do = (quantize(rng.randn(*s).astype(np.float32), dtype) for s in shapes)
    sc = (1 / math.sqrt(D)) if c["scale"] is None else c["scale"]
    h, logit = c["hard"], None
    if h is not None and h[0] == "spike":
        _, want, b, head, i, j, _ = h
        row = q[b, head, i].astype(np.float64)
        k[b, head // (c["Hq"] // c["Hkv"]), j] = quantize((want / (sc * float(row @ row)) * row).astype(np.float32), dtype)
        logit = sc * float(row @ k[b, head // (c["Hq"] // c["Hkv"]), j].astype(np.float64))
    elif h is not None:
        k[:, h[2]] = quantize((k[:, h[2]] + h[1]).astype(np.float32), dtype)
    return q, k, v, do, sc, logit


def dense_reference(c, seed):
    """Everything of a d256 / pad run that needs no GPU: the quantised inputs, the fp64 judges and every bound, each from the configuration
    and the reference alone.  R["facts"]: what tests/test_fuzz_d256_draws.py asserts about the reference (the spike's and the wrong
    scale's distance from the judge in units of the forward tolerance, whether the delta allowance is the wider gradient bound)."""
    D, dtype = c.get("D", 256), c["dtype"]
    g, cz = c["Hq"] // c["Hkv"], CZ[c["causal"]]
    q, k, v, do, sc, logit = dense_inputs(c, seed)
    R = dict(q=q, k=k, v=v, do=do, sc=sc, cz=cz, D=D, facts={})
    vis = oracle._vis_mask(c["Sq"], c["Sk"], cz, c["W"])
    assert [i for i in range(c["Sq"]) if not vis[i].any()] == blind_rows(c) and [j for j in range(c["Sk"]) if not vis[:, j].any()] == unseen_keys(c)
    R["blind"], R["unseen"] = ~vis.any(axis=1), ~vis.any(axis=0)
    R["out"], R["lse"] = oracle.fwd_f64(q, k, v, cz, c["scale"], c["W"])
    vmax = float(np.abs(v).max())
    smax = float(np.abs(np.einsum("bhqd,bhkd->bhqk", q.astype(np.float64), np.repeat(k, g, axis=1).astype(np.float64))).max()) * abs(sc)
    atol, rtol = fwd_tol(dtype, vmax)
    if dtype == "fp32": atol += 2.0 ** -22 * smax * vmax        # (run(): fp32 arithmetic error follows |S|)
    R["out_tol"] = (atol, rtol)
    fin = np.isfinite(R["lse"])
    R["lse_tol"] = LSE_TOL[dtype] + (1e-5 * float(np.abs(R["lse"][fin]).max()) if dtype == "fp32" and fin.any() else 0.0)
    units = lambda a, b: float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())   # noqa: E731   (distance in forward tolerances)
    if c["hard"] is not None:
        # the fuzz_serving rule: fp32 arithmetic error of an LSE grows with |S|; the bound follows what plain NumPy fp32 leaves of the same rows
        gap = np.abs(lse_np(q, k, vis, sc, g, np.float32)[fin] - lse_np(q, k, vis, sc, g, np.float64)[fin])
        R["facts"]["lse_f32_gap"] = float(gap.max()) if gap.size else 0.0
        R["lse_tol"] = max(R["lse_tol"], 4.0 * R["facts"]["lse_f32_gap"])
        if c["hard"][0] == "spike":
            _, _, b, head, i, j, _ = c["hard"]
            plain = dense_inputs(dict(c, hard=None), seed)[1]
            without, _ = oracle.fwd_f64(q[b:b + 1, head:head + 1], plain[b:b + 1, head // g:head // g + 1], v[b:b + 1, head // g:head // g + 1], cz, c["scale"], c["W"])
            R["facts"].update(logit=logit, spike_units=units(without[0, 0, i], R["out"][b, head, i]))
        return R
    if "D" in c and c["scale"] is None:
        Dp = next(x for x in at.SUPPORTED_HEAD_DIMS if x >= D)
        R["facts"]["wrong_scale_units"] = units(oracle.fwd_f64(q, k, v, cz, 1 / math.sqrt(Dp), c["W"])[0], R["out"])
    R["dq"], R["dk"], R["dv"] = oracle.bwd_f64(q, k, v, do, cz, c["scale"], c["W"])
    grow = grad_grow(dtype, smax)
    R["grad_tol"] = {n: grad_tol(n, dtype, g, c["Sq"], c["Sk"], D, c["causal"], c["W"], c["scale"], grow, float(np.abs(R[n]).max())) for n in ("dq", "dk", "dv")}
    R["floor"] = {}
    if dtype != "fp32":
        e_dq, e_dk = delta_model(q, k, v, do, vis, sc, g, dtype)
        R["floor"] = dict(dq=4.0 * np.repeat(e_dq, g, axis=1)[:, :, None, None], dk=4.0 * e_dk[:, :, None, None])
        R["facts"]["delta_rel"] = max(float(e_dq.max()) / max(1.0, float(np.abs(R["dq"]).max())), float(e_dk.max()) / max(1.0, float(np.abs(R["dk"]).max())))
        R["facts"]["delta_binds"] = bool((R["floor"]["dq"] > R["grad_tol"]["dq"][0]).any() or (R["floor"]["dk"] > R["grad_tol"]["dk"][0]).any())
    return R


# ------------------------------------------------------------------------------------------------------ d256 and pad: the runs (GPU)
def _same_bits(a, b):
    view = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(view), b.contiguous().view(view)))


def _judge_dense(c, R, got, errs, stats):
    """got: name -> device tensor (out, lse and, on Gaussian draws, dq, dk, dv) against R = dense_reference(c, seed)"""
    n = {name: t.float().cpu().numpy().astype(np.float64) for name, t in got.items()}
    worst = lambda key, x: stats.__setitem__(key, max(stats.get(key, 0.0), float(x)))   # noqa: E731
    atol, rtol = R["out_tol"]
    if not np.isfinite(n["out"]).all(): errs.append("out non-finite")
    else:
        e = np.abs(n["out"] - R["out"])
        worst("out", e.max()); worst("out_units", (e / (atol + rtol * np.abs(R["out"]))).max())
        if (e > atol + rtol * np.abs(R["out"])).any(): errs.append(f"out err {e.max():.3e} (atol {atol:.2e})")
    blind, unseen = R["blind"], R["unseen"]
    if n["out"][:, :, blind].any(): errs.append("out of a row without a visible key is not zero")
    if "lse" in n:
        fin = np.isfinite(R["lse"])
        assert np.array_equal(~fin, np.broadcast_to(blind, fin.shape))
        if not np.isneginf(n["lse"][~fin]).all(): errs.append("lse of a row without a visible key is not -inf")
        if fin.any():
            e = np.abs(n["lse"][fin] - R["lse"][fin])
            worst("lse", e.max() if np.isfinite(e).all() else np.inf)
            if not (e <= R["lse_tol"]).all(): errs.append(f"lse err {e.max():.3e} (bound {R['lse_tol']:.2e})")
    for name in ("dq", "dk", "dv"):
        if name not in n: continue
        gg, want = n[name], R[name]
        if not np.isfinite(gg).all(): errs.append(name + " non-finite"); continue
        if name == "dq" and gg[:, :, blind].any(): errs.append("dq of a row without a visible key is not zero")
        if name != "dq" and gg[:, :, unseen].any(): errs.append(name + " of a key no query sees is not zero")
        tol, r = R["grad_tol"][name]
        e = np.abs(gg - want)
        worst(name, e.max() / max(1.0, float(np.abs(want).max())))
        if (e > np.maximum(tol + r * np.abs(want), R["floor"].get(name, 0.0))).any(): errs.append(f"{name} err {e.max():.3e} (tol {tol:.1e})")
    if R["facts"].get("delta_binds"): stats["delta_binds"] = stats.get("delta_binds", 0) + 1


def _last_backward_route():
    return int(_capi.get_lib().aule_hip_debug_last_backward_route())


def run_d256(cfg, seed, stats=None):
    """One head_dim 256 configuration on the GPU: out, lse and (Gaussian draws) dq, dk, dv against the fp64 judges, zeros and -inf exactly
    where nothing is visible, the routes, and the exact relations: two runs, batch element 0 alone, and the MHA call on K and V repeated
    per query head give the same bits."""
    c, stats = cfg, {} if stats is None else stats
    R = dense_reference(c, seed)
    errs, cz, sc, W, g, back = [], R["cz"], R["sc"], c["W"], c["Hq"] // c["Hkv"], c["hard"] is None
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", torch_dtype(c["dtype"]))   # noqa: E731

    def call(tq, tk, tv, tdo):
        out, lse = at.fwd_raw(tq, tk, tv, cz, sc, window=W)
        res = dict(out=out, lse=lse)
        if back:
            res["dq"], res["dk"], res["dv"] = at.bwd_raw(tq, tk, tv, out, tdo, lse, cz, sc, window=W)
        torch.cuda.synchronize()
        return res

    t = [dev(R[n]) for n in ("q", "k", "v", "do")]
    got = call(*t)
    f32 = c["dtype"] == "fp32"
    r = route(c["dtype"], c["B"], c["Hq"], c["Hkv"], c["Sq"], c["Sk"], 256, {"none": 0, "top": 1, "br": 2}[c["causal"]], W)
    if r != (0 if f32 else 9): errs.append(f"forward route {r}")
    if back:
        rb, bits = _last_backward_route(), (128 | 32) if f32 else 128
        if rb & bits != bits: errs.append(f"backward route {rb}")
    _judge_dense(c, R, got, errs, stats)
    again = call(*t)
    for name in got:
        if not _same_bits(got[name], again[name]): errs.append("two runs give different bits in " + name)
    if c["B"] > 1:
        one = call(*(x[:1].contiguous() for x in t))
        for name in got:
            if not _same_bits(one[name], got[name][:1]): errs.append("batch element 0 alone differs from the batch in " + name)
    if g > 1:
        mha = call(t[0], t[1].repeat_interleave(g, dim=1), t[2].repeat_interleave(g, dim=1), t[3])
        for name in ("out", "lse", "dq"):
            if name in got and not _same_bits(mha[name], got[name]): errs.append("the MHA call on repeated K / V differs in " + name)
    return r, errs


def run_pad(cfg, seed, stats=None):
    """One zero-padded head size through aule.flash_attention with autograd, judged at the true D; shapes and dtypes of what comes back"""
    import aule
    c, stats = cfg, {} if stats is None else stats
    R = dense_reference(c, seed)
    errs, D = [], c["D"]
    tdt = torch_dtype(c["dtype"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda", tdt)   # noqa: E731

    def call():
        tq, tk, tv = (dev(R[n]).requires_grad_(True) for n in ("q", "k", "v"))
        out = aule.flash_attention(tq, tk, tv, causal=R["cz"], scale=c["scale"], window_size=c["W"])
        out.backward(dev(R["do"]))
        torch.cuda.synchronize()
        res = dict(out=out.detach(), dq=tq.grad, dk=tk.grad, dv=tv.grad)
        for name, like in (("out", tq), ("dq", tq), ("dk", tk), ("dv", tv)):
            if res[name].shape != like.shape or res[name].dtype != tdt: errs.append(f"{name} comes back as {tuple(res[name].shape)} {res[name].dtype}")
        return res

    got = call()
    rb = _last_backward_route()
    if D > 128 and not rb & 128: errs.append(f"backward route {rb}")
    if errs: return rb, errs
    _judge_dense(c, R, got, errs, stats)
    again = call()
    for name in got:
        if not _same_bits(got[name], again[name]): errs.append("two runs give different bits in " + name)
    return rb, errs


RUN = dict(d256=run_d256, pad=run_pad)


def run_list(kind, cfgs_seeds):
    """[(cfg, data seed)] -> (failures [(i, seed, cfg, errs)], maxima, routes); prints a `one` line for every failing draw.  An
    exception -- a refusal of a call that should be valid, or a device error -- is a finding and ends the run."""
    failures, worst, routes = [], {}, {}
    for i, (cfg, seed) in enumerate(cfgs_seeds):
        stats = {}
        try:
            r, errs = RUN[kind](cfg, seed, stats)
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001
            failures.append((i, seed, cfg, ["EXCEPTION %s: %s" % (type(e).__name__, " ".join(str(e).split())[:200])]))
            print("FAIL %s #%d: python tools/fuzz_parity.py one %s \"%r\" %d : %s -- the run stops here" % (kind, i, kind, cfg, seed, failures[-1][3][0]), flush=True)
            break
        routes[r] = routes.get(r, 0) + 1
        for key, x in stats.items():
            worst[key] = worst.get(key, 0) + x if key == "delta_binds" else max(worst.get(key, 0.0), x)
        if errs:
            failures.append((i, seed, cfg, errs))
            print("FAIL %s #%d: python tools/fuzz_parity.py one %s \"%r\" %d : %s" % (kind, i, kind, cfg, seed, "; ".join(errs)), flush=True)
    return failures, worst, routes


def _fmt(worst):
    return ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "one" and sys.argv[2] in RUN:
        # one printed configuration again: python tools/fuzz_parity.py one d256 "<cfg as printed>" SEED
        import ast
        stats = {}
        r, errs = RUN[sys.argv[2]](ast.literal_eval(sys.argv[3]), int(sys.argv[4]), stats)
        print("%s route=%s: %s  [%s]" % (sys.argv[2], r, "; ".join(errs) if errs else "clean", _fmt(stats)))
        sys.exit(1 if errs else 0)
    if len(sys.argv) > 1 and sys.argv[1] in RUN:
        kind = sys.argv[1]
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 100; seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
        failures, worst, routes = run_list(kind, [(c, SEED0[kind] + i) for i, c in enumerate(draws(kind, n, seed))])
        print("%s: %d configurations at seed %d, %d failing; maxima: %s; routes: %s" % (kind, n, seed, len(failures), _fmt(worst), dict(sorted(routes.items()))))
        sys.exit(1 if failures else 0)
    if len(sys.argv) > 1 and sys.argv[1] == "one":
        # one configuration again: python tools/fuzz_parity.py one bf16 1 4 2 31 500 128 br -1 0.3 1001   (scale: a number or "none")
        a = sys.argv[2:]
        cfg = (a[0], int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), a[7], int(a[8]), None if a[9] == "none" else float(a[9]))
        r, errs = run(cfg, int(a[10]))
        print(f"route={r} cfg={cfg}: {'; '.join(errs) if errs else 'clean'}")
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] in ("split", "long", "window"):
        kind = sys.argv[1]
        n = int(sys.argv[2]) if len(sys.argv) > 2 else 40; seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
        rng = np.random.RandomState(seed); bad = 0; routes = {}
        for i in range(n):
            try:
                (r, cfg), errs = {"split": run_split, "long": run_long, "window": run_window}[kind](rng, i)
            except Exception as e:  # noqa: BLE001
                (r, cfg), errs = (-9, ("?",)), [f"EXCEPTION {type(e).__name__}: {str(e)[:160]}"]
            routes[r] = routes.get(r, 0) + 1
            if errs:
                bad += 1; print(f"FAIL {kind} #{i} route={r} cfg={cfg}: {'; '.join(errs)}", flush=True)
        print(f"{kind}: {n} configurations, {bad} failing; forward routes exercised: {dict(sorted(routes.items()))}")
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] in ("paged", "rope"):
        mode = sys.argv[1]; n = int(sys.argv[2]) if len(sys.argv) > 2 else 200; seed = int(sys.argv[3]) if len(sys.argv) > 3 else 0
        rng = np.random.RandomState(seed); bad = 0
        for i in range(n):
            try:
                cfg, errs = (run_paged if mode == "paged" else run_rope)(rng, i)
            except Exception as e:  # noqa: BLE001
                cfg, errs = ("?",), [f"EXCEPTION {type(e).__name__}: {str(e)[:160]}"]
            if errs:
                bad += 1; print(f"FAIL {mode} #{i} cfg={cfg}: {'; '.join(errs)}", flush=True)
        print(f"{mode}: {n} configurations, {bad} failing")
        sys.exit(0)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    rng = np.random.RandomState(seed)
    routes, bad = {}, 0
    for i in range(n):
        cfg = draw(rng)
        try:
            r, errs = run(cfg, 1000 + i)
        except Exception as e:  # noqa: BLE001
            r, errs = -9, [f"EXCEPTION {type(e).__name__}: {str(e)[:160]}"]
        routes[r] = routes.get(r, 0) + 1
        if errs:
            bad += 1
            print(f"FAIL #{i} route={r} cfg={cfg}: {'; '.join(errs)}", flush=True)
    print(f"{n} configurations, {bad} failing; forward routes exercised: {dict(sorted(routes.items()))}")
