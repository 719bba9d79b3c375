#!/usr/bin/env python3
"""Variable-length packed batches at head_dim 256: aule.flash_attention_varlen_d256 against one aule.flash_attention call per sequence
and one padded dense call, both at head_dim 256 from the same build -- the legs, the alternated rounds, the windows, the medians and
the agreement check of tools/bench_varlen.py (its docstring states them), with 16 query / 8 KV heads.  Shapes: the SFT mix (64
sequences of 64 .. 4096 tokens), 512 x 64 and 8 x 4096, forward and forward + backward.

    python tools/bench_varlen_d256.py --out profiles/varlen_d256_bench.txt      (--rounds N, --leg-timeout SECONDS as the base tool)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_varlen as base  # noqa: E402

if __name__ == "__main__":
    b = base.BATCHES
    base.main(16, 8, 256, base.aule.flash_attention_varlen_d256, "tools/bench_varlen_d256.py", [b[1], b[2], b[0]])
