#!/usr/bin/env python3
"""Tree verify: aule.flash_attention_paged_query_tree against the routes there were, on the same cache in the same process, alternated
round by round, warm:
  (a) tree query    the tree entry: batch sequences of 32 draft nodes each, one call;
  (b) plain query   aule.flash_attention_paged_query at the same seq_q (a chain of 32): what the mask costs on top of it;
  (c) per path      the route without a tree entry: one sequence per root-to-leaf path (batch x paths sequences of `depth` tokens) through
                    aule.flash_attention_paged_query; the block tables share the context blocks (the context is a multiple of the block
                    size) and each path has one private block for its tokens -- the context is read once per path;
  (d) prefill tree  the same batch through aule.flash_attention_paged_prefill_tree.
Shape: bf16, 32 query / 8 KV heads, head_dim 128, block size 16; batch 8 and 64; context 1 K and 8 K; 16-bit and FP8 caches.
Tree: 32 nodes, depth 5 -- 4 roots, 7 nodes on every later level (three roots with two children, one with one, then chains): 7 paths.

Per case the median over the rounds and the spread (min .. max) of each route and the ratios comparator / tree query: above 1 the tree
query wins; a ratio below 0.96 -- the tree query slower than the comparator by more than the spread between boxes -- is set in **bold**.
Nothing here is a pass / fail number.  Before a case is timed (a) and (d) are compared (two 16-bit results).

Every case runs under its own alarm (--leg-timeout seconds, default 120): a case that hangs ends the process.  A timed window repeats
its call until it holds about 40 ms of device time.  --out FILE also writes the table there.  --rounds N (default 5)."""
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
import torch  # noqa: E402

import aule  # noqa: E402

HQ, HKV, D, BS = 32, 8, 128, 16
WIDTHS = [4, 7, 7, 7, 7]          # nodes per level
WINDOW_MS = 40
LOSS = 0.96


def _arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def tree():
    """parents of the 32 nodes, level by level, and the root-to-leaf paths"""
    parents, level = [], []
    for depth, width in enumerate(WIDTHS):
        first = len(parents)
        for i in range(width):
            parents.append(-1 if depth == 0 else level[min(i // 2, len(level) - 1)] if depth == 1 else level[i])
        level = list(range(first, first + width))
    paths = []
    for leaf in level:
        path, j = [], leaf
        while j >= 0:
            path.append(j)
            j = parents[j]
        paths.append(path[::-1])
    return parents, paths


def case(batch, ctx, fp8):
    g = torch.Generator(device="cuda").manual_seed(11)
    parents, paths = tree()
    n, depth, npaths = len(parents), len(WIDTHS), len(paths)
    ctx_blocks, tree_blocks = ctx // BS, (n + BS - 1) // BS
    num_blocks = batch * (ctx_blocks + tree_blocks + npaths)
    shape = (num_blocks, BS, HKV, D)
    if fp8:
        kc, vc = ((torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g) * 2).to(torch.float8_e4m3fn) for _ in range(2))
        scales = dict(k_scale=torch.full((HKV,), 0.5, device="cuda"), v_scale=torch.full((HKV,), 0.5, device="cuda"))
    else:
        kc, vc = (torch.randn(shape, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(2))
        scales = {}
    # sequence b: context blocks, then the tree's blocks, then one private block per path
    per = ctx_blocks + tree_blocks + npaths
    base = torch.arange(batch, device="cuda", dtype=torch.int32)[:, None] * per
    bt = base + torch.arange(ctx_blocks + tree_blocks, device="cuda", dtype=torch.int32)[None, :]
    bt_paths = torch.cat([(base + torch.arange(ctx_blocks, device="cuda", dtype=torch.int32)[None, :]).repeat_interleave(npaths, 0),
                          (base + ctx_blocks + tree_blocks + torch.arange(npaths, device="cuda", dtype=torch.int32)[None, :]).reshape(-1, 1)], 1)
    cl = torch.full((batch,), ctx + n, device="cuda", dtype=torch.int32)
    cl_paths = torch.full((batch * npaths,), ctx + depth, device="cuda", dtype=torch.int32)
    q = torch.randn(batch, HQ, n, D, device="cuda", dtype=torch.bfloat16, generator=g)
    q_paths = q[:, :, torch.tensor(paths, device="cuda")].permute(0, 2, 1, 3, 4).reshape(batch * npaths, HQ, depth, D).contiguous()
    q_packed = q.permute(0, 2, 1, 3).reshape(batch * n, HQ, D).contiguous()
    words = aule.tree_mask_from_parents(torch.tensor(parents, device="cuda")).repeat(batch, 1).contiguous()
    words_packed = words.reshape(-1)
    cu = torch.arange(batch + 1, device="cuda", dtype=torch.int32) * n

    def a():
        return aule.flash_attention_paged_query_tree(q, kc, vc, words, bt, cl, **scales)

    def b():
        return aule.flash_attention_paged_query(q, kc, vc, bt, cl, **scales)

    def c():
        return aule.flash_attention_paged_query(q_paths, kc, vc, bt_paths, cl_paths, **scales)

    def d():
        return aule.flash_attention_paged_prefill_tree(q_packed, kc, vc, words_packed, bt, cl, cu, max_seqlen_q=n, **scales)

    x, y = a().float(), d().view(batch, n, HQ, D).permute(0, 2, 1, 3).float()
    bound = 1e-3 + 2 * 2.0 ** -9 * float(vc.float().abs().max()) * (0.5 if fp8 else 1.0) + 2.0 ** -7 * y.abs()
    if not bool(((x - y).abs() <= bound).all()):
        raise SystemExit("the tree query and the prefill tree disagree")
    return {"a": a, "b": b, "c": c, "d": d}, npaths


def window_us(f, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def leg(batch, ctx, fp8, rounds, lines):
    calls, npaths = case(batch, ctx, fp8)
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

    def ratio(key):
        r = med[key] / med["a"]
        return f"**{r:5.3f}x**" if r < LOSS else f"  {r:5.3f}x  "

    line = (f"  batch {batch:2d} context {ctx:4d} {'fp8 ' if fp8 else '16  '}: (a) tree query {span['a']} us   (b) plain query {span['b']} us   "
            f"(c) {npaths} paths x {len(WIDTHS)} tokens {span['c']} us   (d) prefill tree {span['d']} us   (b) / (a) {ratio('b')}   (c) / (a) {ratio('c')}   "
            f"(d) / (a) {ratio('d')}")
    print(line, flush=True)
    lines.append(line)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_tree needs a GPU: a timing taken anywhere else says nothing")
    rounds, budget = _arg("--rounds", 5), _arg("--leg-timeout", 120)
    signal.signal(signal.SIGALRM, signal.SIG_DFL)      # the default action ends the process, also from inside a blocked device call
    parents, paths = tree()
    head = (f"# tools/bench_tree.py   (one MI355X; {HQ} q / {HKV} kv heads, head_dim {D}, bf16, block size {BS}; tree of {len(parents)} nodes, depth "
            f"{len(WIDTHS)}, {len(paths)} root-to-leaf paths; {rounds} alternated rounds of ~{WINDOW_MS} ms windows, median (min .. max) us per call, "
            f"host launch cost included; ratios are comparator / tree query, bold below {LOSS})")
    print(head, flush=True)
    lines = [head]
    for fp8 in (False, True):
        for batch in (8, 64):
            for ctx in (1024, 8192):
                signal.alarm(budget)
                leg(batch, ctx, fp8, rounds, lines)
                signal.alarm(0)
                torch.cuda.empty_cache()
    if "--out" in sys.argv:
        path = _arg("--out", "", str)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
