#!/usr/bin/env python3
"""Logit soft-capping at head_dim 256 (softcap = 50, Gemma-2): each capped entry against (a) its uncapped twin on the same tensors --
the price of the cap -- and (b) the torch route there was: gather where paged, matmul, tanh, softmax, matmul.  Same process, warm,
alternated round by round, medians over the rounds with the spread, per call through the Python layer; a timed window repeats its call
until it holds about 20 ms of device time.  bf16, 16 q / 8 kv heads, causal.

Legs: variable-length forward and forward + backward on the SFT mix (sequence lengths 512 .. 4096, 16 K tokens) and on 8 x 4096; paged
decode at batch 8 / 64 x 8 K / 32 K keys, one token per sequence, 16-bit and FP8 cache, block 16, shuffled table.  The torch route of a
varlen leg runs sequence by sequence (its scores are [heads, n, n] fp32); of a decode leg on the gathered, dequantised keys, timed with
the gather.  Ratios are other / capped: below 1 the capped call LOSES.  --out FILE also writes the table there.  --rounds N (default 5)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

D, HQ, HKV, BS, CAP, WINDOW_MS = 256, 16, 8, 16, 50.0, 20
SCALE = D ** -0.5


def _window(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternated(calls, rounds):
    """{name: (median us, "median (min .. max)")}, warm, alternated round by round"""
    iters = {}
    for key, f in calls.items():
        _window(f, 2)
        iters[key] = min(400, max(2, int(WINDOW_MS * 1e3 / _window(f, 2)) + 1))
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(_window(f, iters[key]))
    return {k: (sorted(v)[len(v) // 2], f"{sorted(v)[len(v) // 2]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})") for k, v in t.items()}


def torch_capped(q, k, v, causal_offset):
    """q [n, Hq, D], k / v [L, Hkv, D] -> [n, Hq, D]: matmul, tanh, mask, softmax, matmul"""
    g = q.shape[1] // k.shape[1]
    s = torch.einsum("nhgd,lhd->hgnl", q.view(q.shape[0], -1, g, D).float(), k.float()) * SCALE
    s = CAP * torch.tanh(s / CAP)
    n, L = q.shape[0], k.shape[0]
    see = torch.arange(L, device=q.device)[None] <= torch.arange(n, device=q.device)[:, None] + causal_offset
    p = torch.softmax(s.masked_fill(~see, float("-inf")), dim=-1)
    return torch.einsum("hgnl,lhd->nhgd", p, v.float()).reshape(n, -1, D).to(q.dtype)


def varlen_leg(name, lens, backward, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    T = sum(lens)
    q, k, v, do = (torch.randn(T, h, D, device="cuda", dtype=torch.bfloat16, generator=g).requires_grad_(backward) for h in (HQ, HKV, HKV, HQ))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device="cuda")
    kw = dict(max_seqlen_q=max(lens), max_seqlen_k=max(lens), causal=True)

    def done(out, lo=0, hi=T):
        if backward:
            torch.autograd.grad(out, (q, k, v), do.detach()[lo:hi])

    def torch_route():
        at = 0
        for n in lens:
            done(torch_capped(q[at:at + n], k[at:at + n], v[at:at + n], 0), at, at + n)
            at += n
    calls = {"capped": lambda: done(aule.flash_attention_varlen_d256_softcap(q, k, v, CAP, cu, cu, **kw)),
             "uncapped twin": lambda: done(aule.flash_attention_varlen_d256(q, k, v, cu, cu, **kw)), "torch route": torch_route}
    return name, alternated(calls, rounds)


def decode_leg(B, L, fp8, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    nblk = B * L // BS
    q = torch.randn(B, HQ, D, device="cuda", dtype=torch.bfloat16, generator=g)
    kc, vc = (torch.randn(nblk, BS, HKV, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
    ks = vs = None
    if fp8:
        kc, vc = kc.to(torch.float8_e4m3fn), vc.to(torch.float8_e4m3fn)
        ks, vs = (torch.full((HKV,), x, device="cuda") for x in (1.25, 0.75))
    bt = torch.randperm(nblk, device="cuda", generator=g).to(torch.int32).view(B, L // BS)
    cl = torch.full((B,), L, dtype=torch.int32, device="cuda")
    kw = dict(k_scale=ks, v_scale=vs)

    def torch_route():
        k, v = (x[bt.long()].reshape(B, L, HKV, D) for x in (kc, vc))
        if fp8:
            k, v = k.float() * ks[None, None, :, None], v.float() * vs[None, None, :, None]
        s = torch.einsum("bhgd,blhd->bhgl", q.view(B, HKV, -1, D).float(), k.float()) * SCALE
        p = torch.softmax(CAP * torch.tanh(s / CAP), dim=-1)
        return torch.einsum("bhgl,blhd->bhgd", p, v.float()).reshape(B, HQ, D).to(q.dtype)
    calls = {"capped": lambda: aule.flash_attention_paged_d256_softcap(q, kc, vc, CAP, bt, cl, **kw),
             "uncapped twin": lambda: aule.flash_attention_paged_d256(q, kc, vc, bt, cl, **kw), "torch route": torch_route}
    return "decode B=%d L=%d %s" % (B, L, "fp8" if fp8 else "bf16"), alternated(calls, rounds)


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    sft = [4096, 2048, 2048, 1024, 1024, 1024, 1024, 512, 512, 512, 512, 512, 512, 512, 512]
    lines = ["softcap = %g, bf16, %d q / %d kv heads, head_dim 256; us per call, median (min .. max) over %d alternated rounds; x = other / capped" % (CAP, HQ, HKV, rounds),
             "device: %s" % torch.cuda.get_device_name(0)]
    legs = [lambda b=b, n=n, l=l: varlen_leg("varlen %s %s" % (n, "fwd+bwd" if b else "fwd"), l, b, rounds)
            for n, l in (("SFT mix 16K", sft), ("8 x 4096", [4096] * 8)) for b in (False, True)]
    legs += [lambda B=B, L=L, f=f: decode_leg(B, L, f, rounds) for f in (False, True) for B in (8, 64) for L in (8192, 32768)]
    for leg in legs:
        name, r = leg()
        cap = r["capped"][0]
        lines.append("%-28s capped %s | twin %s x%.2f | torch %s x%.2f" % (name, r["capped"][1], r["uncapped twin"][1], r["uncapped twin"][0] / cap,
                                                                            r["torch route"][1], r["torch route"][0] / cap))
        print(lines[-1], flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
