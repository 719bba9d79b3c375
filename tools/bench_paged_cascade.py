#!/usr/bin/env python3
"""Paged cascade: aule.flash_attention_paged_cascade (the shared prefix read once for the batch, the own keys by the paged
prefill, one merge) against the calls that treat the prefix as every sequence's private keys -- the same batch with the
prefix blocks written in front of each sequence's own blocks in its block table ("concatenated tables"):
aule.flash_attention_paged_prefill, and for the decode legs aule.flash_attention_paged_amd too -- on the same tensors in the
same process, alternated round by round, warm.  The method of tools/bench_paged_prefill.py.

Shapes: bf16 queries, 32 query / 8 KV heads, head_dim 128, block 16, shuffled block tables; 16-bit and FP8 caches.
  (a) 64 decodes (one new token each) with 256 own keys behind a shared prefix of 2 K, 8 K and 32 K keys;
  (b) 8 sequences x 512 new tokens (512 own keys) behind a shared prefix of 4 K and 32 K keys.
The prefix table is sized to the prefix, except in two decode legs whose table holds 32 K keys for a prefix of 2 K and 8 K:
the key splits are planned from the table's capacity, so most of them then hold no key.  Per leg the median over the rounds
and the spread (min .. max) of each call and the ratios comparator / cascade (above 1: the cascade is faster).  Before a leg
is timed the calls are compared (the forward bound of tests/util.py, two roundings).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  Legs run in this
one process and the first failure stops the run.  A timed window repeats its call until it holds about 40 ms of device time.
--out FILE also writes the table there.  --rounds N (default 5)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
WINDOW_MS = 40
LEGS = [  # name, sequences, new tokens of each, own keys of each (the new ones included), shared prefix keys, keys the prefix table holds
    ("64 decodes, 256 own, prefix 2 K", 64, 1, 256, 2048, 2048),
    ("64 decodes, 256 own, prefix 8 K", 64, 1, 256, 8192, 8192),
    ("64 decodes, 256 own, prefix 32 K", 64, 1, 256, 32768, 32768),
    ("... prefix 2 K in a 32 K table", 64, 1, 256, 2048, 32768),
    ("... prefix 8 K in a 32 K table", 64, 1, 256, 8192, 32768),
    ("8 x 512, prefix 4 K", 8, 512, 512, 4096, 4096),
    ("8 x 512, prefix 32 K", 8, 512, 512, 32768, 32768),
]


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def leg(name, B, n, own, P, table, fp8, rounds, lines):
    g = torch.Generator(device="cuda").manual_seed(B + 2 * fp8 + P)
    dt = torch.bfloat16
    npre, ntab, nown = P // BS, table // BS, (own + BS - 1) // BS
    nb, T = ntab + B * nown, B * n
    q = torch.randn(T, HQ, D, device="cuda", dtype=dt, generator=g)
    kc = torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
    vc = torch.randn(nb, BS, HKV, D, device="cuda", dtype=dt, generator=g)
    kw = {}
    if fp8:
        kc, ks = aule.quantize_kv_cache_fp8(kc)
        vc, vs = aule.quantize_kv_cache_fp8(vc)
        kw = dict(k_scale=ks, v_scale=vs)
    perm = torch.randperm(nb, device="cuda", generator=g).to(torch.int32)
    pbt = perm[:ntab].contiguous()                 # the plan sees the table's capacity, the kernel prefix_len
    bt = perm[ntab:].view(B, nown).contiguous()
    bt_cat = torch.cat([pbt[None, :npre].expand(B, -1), bt], dim=1).contiguous()
    plen = torch.tensor([P], device="cuda", dtype=torch.int32)
    cl = torch.full((B,), own, device="cuda", dtype=torch.int32)
    cl_cat = cl + P
    cu = torch.arange(0, T + 1, n, device="cuda", dtype=torch.int32)

    calls = {"cascade": lambda: aule.flash_attention_paged_cascade(q, kc, vc, pbt, plen, bt, cl, cu, max_seqlen_q=n, **kw),
             "prefill": lambda: aule.flash_attention_paged_prefill(q, kc, vc, bt_cat, cl_cat, cu, max_seqlen_q=n, **kw)}
    if n == 1:
        calls["decode"] = lambda: aule.flash_attention_paged_amd(q, kc, vc, bt_cat, cl_cat, **kw)
    got = {k: f() for k, f in calls.items()}
    torch.cuda.synchronize()
    vmax = float((vc.float() * vs.view(1, 1, HKV, 1)).abs().max()) if fp8 else float(vc.float().abs().max())
    for k in list(calls)[1:]:
        bound = 1e-3 + 2 * 2.0 ** -9 * vmax + 2 * 2.0 ** -8 * got[k].float().abs()
        if not bool(((got["cascade"].float() - got[k].float()).abs() <= bound).all()):
            raise SystemExit(f"{name} fp8 {fp8}: the cascade and {k} on the concatenated tables disagree")

    def window(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters * 1e3

    # warm, then size every timed window to about WINDOW_MS of device time (a shorter one measures the clock and the scheduler)
    iters = {}
    for key, f in calls.items():
        window(f, 2)
        iters[key] = min(400, max(3, int(WINDOW_MS * 1e3 / window(f, 2)) + 1))
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(window(f, iters[key]))
    med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
    span = {k: f"{med[k]:9.1f} ({min(v):9.1f} .. {max(v):9.1f})" for k, v in t.items()}
    line = (f"  {name:34s} {'fp8' if fp8 else '16b'}: cascade {span['cascade']} us   paged prefill, concatenated tables {span['prefill']} us"
            f"   prefill / cascade {med['prefill'] / med['cascade']:5.2f}x")
    if "decode" in calls:
        line += f"   paged decode, concatenated tables {span['decode']} us   decode / cascade {med['decode'] / med['cascade']:5.2f}x"
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_cascade needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    head = (f"# tools/bench_paged_cascade.py   (one MI355X; {HQ} q / {HKV} kv heads, head_dim {D}, block_size {BS}, bf16 queries, shuffled "
            f"block tables; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, host launch cost included)")
    print(head, flush=True)
    lines = [head]
    for name, B, n, own, P, table in LEGS:
        for fp8 in (False, True):
            signal.alarm(budget)
            leg(name, B, n, own, P, table, fp8, rounds, lines)
            signal.alarm(0)
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
