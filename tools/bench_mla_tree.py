#!/usr/bin/env python3
"""Tree verify over the latent cache: aule.flash_attention_mla_paged_tree against the routes there were, on the same cache in the same
process, alternated round by round, warm (the manner of tools/bench_tree.py):
  (a) tree        the tree entry: batch sequences of 32 draft nodes each, one call;
  (b) chain       aule.flash_attention_mla_paged / _fp8 at the same n (a chain of 32): the price of the mask and of the key range that
                  is not cut at a row block's last position;
  (c) per path    the route without a tree entry: one sequence per root-to-leaf path (batch x paths sequences of `depth` tokens) through
                  aule.flash_attention_mla_paged / _fp8; the block tables share the context blocks (the context is a multiple of the
                  block size) and each path has one private block for its tokens -- the latent is read once per path;
  (d) sparse      aule.flash_attention_mla_sparse with the same visibility as per-token slot lists (context 1 K and 8 K only).
Shape: bf16, latent 576 / 512, block size 64, shuffled block tables; 16 and 128 heads; batch 8 and 64; context 1 K, 8 K and 32 K; 16-bit
and FP8 caches.  Tree: 32 nodes, depth 5 -- 4 roots, 7 nodes on every later level: 7 paths (tools/bench_tree.py's).

Per leg the median over the rounds and the spread (min .. max) of each route and the ratios comparator / tree: above 1 the tree call
wins.  A leg where the tree call is slower than (b) by more than the spread between boxes (ratio below 0.96), or slower than (c) at all,
is marked **loses** with its figure.  Nothing here is a pass / fail number and no dispatch rule reads these figures.  Before a leg is
timed (a) and (d) are compared (two 16-bit results).

Every leg runs under its own alarm (--leg-timeout seconds, default 120): a leg that hangs ends the process.  A timed window repeats its
call until it holds about 40 ms of device time.  --out FILE also writes the table there.  --rounds N (default 5)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import aule  # noqa: E402
from bench_tree import WIDTHS, WINDOW_MS, tree, window_us  # noqa: E402

QK, VD, BS = 576, 512, 64
LOSS_B, LOSS_C = 0.96, 1.0
SPARSE_MAX_CTX = 8192


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def case(heads, batch, ctx, fp8):
    g = torch.Generator(device="cuda").manual_seed(11)
    parents, paths = tree()
    n, depth, npaths = len(parents), len(WIDTHS), len(paths)
    assert ctx % BS == 0 and n <= BS
    ctx_blocks = ctx // BS
    per = ctx_blocks + 1 + npaths                     # a sequence's blocks: context, the tree's block, one private block per path
    num_blocks = batch * per
    kv = torch.randn((num_blocks, BS, QK), device="cuda", dtype=torch.bfloat16, generator=g)
    scale = {}
    if fp8:
        kv = (kv * 2).to(torch.float8_e4m3fn)
        scale = dict(kv_scale=torch.full((1,), 0.5, device="cuda"))
    own = torch.randperm(num_blocks, device="cuda", generator=g).to(torch.int32).view(batch, per)          # shuffled pages
    bt = own[:, :ctx_blocks + 1].contiguous()
    bt_paths = torch.cat([own[:, :ctx_blocks].repeat_interleave(npaths, 0), own[:, ctx_blocks + 1:].reshape(-1, 1)], 1).contiguous()
    cl = torch.full((batch,), ctx + n, device="cuda", dtype=torch.int32)
    cl_paths = torch.full((batch * npaths,), ctx + depth, device="cuda", dtype=torch.int32)
    cu = torch.arange(batch + 1, device="cuda", dtype=torch.int32) * n
    cu_paths = torch.arange(batch * npaths + 1, device="cuda", dtype=torch.int32) * depth
    q = torch.randn(batch * n, heads, QK, device="cuda", dtype=torch.bfloat16, generator=g)
    at = torch.tensor(paths, device="cuda")                                                                 # [paths, depth]
    q_paths = q.view(batch, n, heads, QK)[:, at].reshape(batch * npaths * depth, heads, QK).contiguous()
    words = aule.tree_mask_from_parents(torch.tensor(parents, device="cuda")).repeat(batch).contiguous()
    dense = aule.flash_attention_mla_paged_fp8 if fp8 else aule.flash_attention_mla_paged

    def a():
        return aule.flash_attention_mla_paged_tree(q, kv, words, bt, cl, cu, max_seqlen_q=n, **scale)

    def b():
        return dense(q, kv, bt, cl, cu, max_seqlen_q=n, **scale)

    def c():
        return dense(q_paths, kv, bt_paths, cl_paths, cu_paths, max_seqlen_q=depth, **scale)

    calls = {"a": a, "b": b, "c": c}
    if ctx <= SPARSE_MAX_CTX:
        # the same visibility as lists: the context's slots, then the node's ancestors and itself in the tree's block (-1: no entry)
        j = torch.arange(ctx, device="cuda")
        ctx_slots = bt[:, :ctx_blocks].long()[:, j // BS] * BS + j % BS                                      # [batch, ctx]
        anc = torch.full((n, depth), -1, dtype=torch.long)
        for i in range(n):
            k, node = 0, i
            while node >= 0:
                anc[i, k] = node
                k, node = k + 1, parents[node]
        anc = anc.cuda()
        tree_slots = torch.where(anc[None] >= 0, bt[:, ctx_blocks].long()[:, None, None] * BS + anc[None], anc[None])     # [batch, n, depth]
        idx = torch.cat([ctx_slots[:, None, :].expand(batch, n, ctx), tree_slots], 2).reshape(batch * n, ctx + depth).to(torch.int32).contiguous()

        def d():
            return aule.flash_attention_mla_sparse(q, kv, idx, **scale)

        calls["d"] = d
        x, y = a().float(), d().float()
        bound = 1e-3 + 2 * 2.0 ** -9 * float(kv[..., :VD].float().abs().max()) * (0.5 if fp8 else 1.0) + 2.0 ** -7 * y.abs()
        if not bool(((x - y).abs() <= bound).all()):
            raise SystemExit("the tree call and the sparse call on the same lists disagree")
    return calls, npaths


def leg(heads, batch, ctx, fp8, rounds, lines):
    calls, npaths = case(heads, batch, ctx, fp8)
    torch.cuda.synchronize()
    iters = {}
    for key, f in calls.items():
        window_us(f, 2)
        iters[key] = min(2000, max(3, int(WINDOW_MS * 1e3 / window_us(f, 2)) + 1))
    t = {key: [] for key in calls}
    for _ in range(rounds):
        for key, f in calls.items():
            t[key].append(window_us(f, iters[key]))
    med = {key: sorted(x)[len(x) // 2] for key, x in t.items()}
    span = {key: f"{med[key]:8.1f} ({min(x):8.1f} .. {max(x):8.1f})" for key, x in t.items()}

    def ratio(key, loss):
        r = med[key] / med["a"]
        return f"**loses {r:5.3f}x**" if r < loss else f"        {r:5.3f}x  "

    line = (f"  heads {heads:3d} batch {batch:2d} context {ctx:5d} {'fp8 ' if fp8 else '16  '}: (a) tree {span['a']} us   (b) chain {span['b']} us   "
            f"(c) {npaths} paths x {len(WIDTHS)} tokens {span['c']} us   (b) / (a) {ratio('b', LOSS_B)}   (c) / (a) {ratio('c', LOSS_C)}")
    if "d" in calls:
        line += f"   (d) sparse {span['d']} us   (d) / (a) {med['d'] / med['a']:5.3f}x"
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_mla_tree needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    parents, paths = tree()
    head = (f"# tools/bench_mla_tree.py   (one MI355X; latent {QK} / {VD}, bf16, block size {BS}, shuffled tables; tree of {len(parents)} nodes, "
            f"depth {len(WIDTHS)}, {len(paths)} root-to-leaf paths; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us "
            f"per call, host launch cost included; ratios are comparator / tree, 'loses': (b) below {LOSS_B} or (c) below {LOSS_C})")
    print(head, flush=True)
    lines = [head]
    for fp8 in (False, True):
        for heads in (16, 128):
            for batch in (8, 64):
                for ctx in (1024, 8192, 32768):
                    signal.alarm(budget)
                    leg(heads, batch, ctx, fp8, rounds, lines)
                    signal.alarm(0)
                    torch.cuda.empty_cache()
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
