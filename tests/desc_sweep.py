"""The fixed sweep of good, bad and edge descriptors behind tests/golden/capi_desc_contract.npz, and the child process that asks
every host-only entry point of the library about every case of it (default environment only: no AULE_HIP_* switch).

    python tests/desc_sweep.py            # prints the library in the tree against the committed table, entry by entry

A case is a valid base descriptor with one mutation: one field (bottom_right: three) set to a bad or edge value.  The table was
recorded from the library BEFORE aule_capi.cpp got one checker per descriptor kind -- every entry point then had its own subset of
the rules -- and it cannot be made again from this tree: a difference is a bug, except where the checkers deliberately refuse what
an entry used to answer for (tests/test_capi_symbols.py::test_descriptor_contract_matches_the_recorded_table names those cases by
mutation and entry point).  Without a device the CU count answers 256, so the table holds on every machine."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_desc_contract.npz")

ATTN_FIELDS = ("dtype", "batch", "heads_q", "heads_kv", "seq_q", "seq_k", "head_dim", "causal", "window_size", "scale")
ATTN_BASES = (                                            # forward route / backward mask in the default environment
    (2, 4, 32, 32, 4096, 4096, 128, 1, -1, 0.0),          # 8 / 2|4     bf16 MHA, the headline shape
    (2, 1, 8, 8, 8192, 8192, 128, 1, -1, 0.125),          # 7 / 2|4     small causal grid: key-range pieces
    (1, 1, 32, 8, 1, 8192, 64, 0, -1, 0.0),               # 5           fp16 GQA decode
    (2, 8, 32, 8, 1, 8192, 128, 2, -1, 0.0),              # 4           one bottom-right query: the non-causal streaming corner
    (1, 1, 8, 8, 64, 1000, 128, 2, -1, 0.0),              # 5           short bottom-right chunk against a KV history
    (0, 4, 8, 8, 512, 512, 64, 0, -1, 0.0),               # 0 / 32      fp32
    (1, 2, 16, 1, 300, 300, 32, 1, 100, -0.1),            # 1 / 8|16    fp16 MQA, D = 32, window, negative scale, odd sizes
    (2, 1, 8, 2, 512, 512, 256, 1, -1, 0.0),              # 9 / 128     head_dim 256
    (0, 1, 8, 8, 300, 300, 256, 0, -1, 0.0),              # 0 / 128|32  fp32 at head_dim 256
)
PAGED_FIELDS = ("dtype", "batch", "heads_q", "heads_kv", "head_dim", "block_size", "max_blocks", "window_size", "scale")
PAGED_BASES = (                                           # (fields ..., fp8)
    (1, 2, 4, 1, 32, 16, 64, -1, 0.0, 0),
    (2, 8, 32, 8, 128, 16, 2048, -1, 0.0, 0),
    (2, 64, 8, 8, 64, 128, 64, -1, 0.0, 1),
    (1, 1, 32, 8, 128, 32, 2048, -1, 0.125, 1),
)
NAN = float("nan")


def attn_mutations(base):
    """(name, {field: value}) for one base; "struct_size" values are offsets from the kind's sizeof (None: struct_size 0)."""
    b = dict(zip(ATTN_FIELDS, base))
    sq = max(b["seq_q"], 2)
    return ([("none", {})] +
            [("struct_size", {"struct_size": v}) for v in (None, -8)] +
            [("dtype", {"dtype": v}) for v in (-1, 3)] +
            [("head_dim", {"head_dim": v}) for v in (0, 48, 512)] +
            [("heads_kv", {"heads_kv": v}) for v in (0, 3)] +        # (3 divides none of the bases' heads_q)
            [("causal", {"causal": v}) for v in (-1, 3)] +
            [("bottom_right", {"causal": 2, "seq_q": sq, "seq_k": sq - 1})] +
            [(f, {f: 0}) for f in ("seq_q", "seq_k", "batch")] +
            [("window_size", {"window_size": v}) for v in (0, -5, b["seq_q"])] +
            [("scale", {"scale": v}) for v in (0.0, NAN, -0.5)])


def attn_cases():
    """(base index, mutation name, the mutated fields) in the table's order."""
    return [(i, name, fields) for i, base in enumerate(ATTN_BASES) for name, fields in attn_mutations(base)]


def paged_cases():
    muts = ([("none", {})] +
            [("struct_size", {"struct_size": v}) for v in (None, -8)] +
            [("dtype", {"dtype": v}) for v in (-1, 0, 3)] +
            [("head_dim", {"head_dim": v}) for v in (0, 48, 256)] +
            [("heads_kv", {"heads_kv": v}) for v in (0, 3)] +
            [("batch", {"batch": 0}), ("block_size", {"block_size": 0}), ("max_blocks", {"max_blocks": 0}),
             ("blocks_2^30", {"block_size": 1 << 15, "max_blocks": 1 << 15})] +
            [("window_size", {"window_size": v}) for v in (0, -5, 100)] +
            [("scale", {"scale": v}) for v in (0.0, NAN, -0.5)])
    return [(i, name, fields) for i in range(len(PAGED_BASES)) for name, fields in muts]


# columns of the "fwd" rows: the four scalar answers, then aule_hip_debug_forward_plan's ints (zero-padded)
FWD_WS, FUSABLE, ROUTE, PLAN_RET, SPLIT_RET, PLAN0, PLAN_CAP = 0, 1, 2, 3, 4, 5, 16
# columns of the "bwd" rows: the size query, the route hook with workspace_bytes 0 and 2^40
BWD_WS, BWD_ROUTE_0, BWD_ROUTE_BIG = 0, 1, 2


def _fill(d, names, base, fields):
    import ctypes
    d.struct_size = ctypes.sizeof(d)
    for f, v in zip(names, base):
        setattr(d, f, v)
    for f, v in fields.items():
        if f == "struct_size":
            d.struct_size = 0 if v is None else ctypes.sizeof(d) + v
        else:
            setattr(d, f, v)


TRAPPED = -(1 << 62)   # recorded where the library the table was made from died of a signal (an integer division by a zero field)


def ask_library(path, record=False):
    """Every case through the library loaded in THIS process (what the child process runs), saved to `path`."""
    import ctypes
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
    from aule import _capi
    lib = _capi.load()

    gold = None if record else np.load(FIXTURE)

    def ask(table, row, col, fn, *args):
        """fn(*args), the answer for gold[table][row][col].  Recording: tried in a forked copy of this process first, TRAPPED if that copy
        dies of a signal.  Otherwise: not asked where the table says TRAPPED (no answer to compare with, and this process would die)."""
        if gold is not None and gold[table][row].flat[col] == TRAPPED:
            return TRAPPED
        if record:
            pid = os.fork()
            if pid == 0:
                fn(*args)
                os._exit(0)
            if os.WIFSIGNALED(os.waitpid(pid, 0)[1]):
                return TRAPPED
        return int(fn(*args))

    I32 = ctypes.c_int32
    buf = (I32 * 4096)()
    fwd, bwd, splits, split_off = [], [], [], [0]
    for n, (i, _, fields) in enumerate(attn_cases()):
        base = ATTN_BASES[i]
        d = _capi.AttnDesc()
        _fill(d, ATTN_FIELDS, base, fields)
        r = _capi.AttnRope()                               # one valid rotation descriptor: enough rows for every base
        r.struct_size, r.layout, r.table_len, r.table_pitch = ctypes.sizeof(_capi.AttnRope), _capi.ROPE_HALF, 40000, 0
        r.q_pos_offset = d.seq_k - d.seq_q if d.causal == 2 and d.seq_k >= d.seq_q else 0
        r.cos, r.sin = 0x10000, 0x20000
        row = [0] * (PLAN0 + PLAN_CAP)
        row[FWD_WS] = ask("fwd", n, FWD_WS, lib.aule_attention_forward_workspace_size, ctypes.byref(d))
        row[FUSABLE] = ask("fwd", n, FUSABLE, lib.aule_attention_forward_rope_fusable, ctypes.byref(d), ctypes.byref(r))
        row[ROUTE] = ask("fwd", n, ROUTE, lib.aule_hip_debug_forward_route, ctypes.byref(d))
        for j in range(PLAN_CAP):
            buf[j] = 0
        row[PLAN_RET] = ask("fwd", n, PLAN_RET, lib.aule_hip_debug_forward_plan, ctypes.byref(d), buf, PLAN_CAP)
        row[PLAN0:] = buf[:PLAN_CAP]
        row[SPLIT_RET] = ask("fwd", n, SPLIT_RET, lib.aule_hip_debug_forward_split_plan, ctypes.byref(d), buf, 4096)
        splits.extend(buf[:max(row[SPLIT_RET], 0)])
        split_off.append(len(splits))
        fwd.append(row)
        b = _capi.AttnBwdDesc()
        _fill(b, ATTN_FIELDS, base, fields)
        brow = [ask("bwd", n, BWD_WS, lib.aule_attention_backward_workspace_size, ctypes.byref(b))]
        for col, ws in ((BWD_ROUTE_0, 0), (BWD_ROUTE_BIG, 1 << 40)):
            b.workspace_bytes = ws
            brow.append(ask("bwd", n, col, lib.aule_hip_debug_backward_route, ctypes.byref(b)))
        bwd.append(brow)
    paged = []
    for n, (i, _, fields) in enumerate(paged_cases()):
        fp8 = PAGED_BASES[i][-1]
        p = _capi.PagedFp8Desc() if fp8 else _capi.PagedDesc()
        _fill(p, PAGED_FIELDS, PAGED_BASES[i][:-1], fields)
        size = lib.aule_attention_paged_decode_fp8_workspace_size if fp8 else lib.aule_attention_paged_decode_workspace_size
        paged.append(ask("paged", n, 0, size, ctypes.byref(p)))
    np.savez_compressed(path, fwd=np.asarray(fwd, np.int64), bwd=np.asarray(bwd, np.int64), split=np.asarray(splits, np.int32),
                        split_off=np.asarray(split_off, np.int32), paged=np.asarray(paged, np.int64))


def run():
    """What the library answers for every case, in a child process without any AULE_HIP_* switch: "fwd" and "bwd" (one row per case of
    attn_cases(), columns above), route 7's dumps ("split", case i at split_off[i] : split_off[i + 1]) and "paged"."""
    import numpy as np
    e = {k: v for k, v in os.environ.items() if not k.startswith("AULE_HIP_")}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "desc.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import numpy as np
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        ask_library(sys.argv[2], record=len(sys.argv) > 3)
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "--record":
        # How the committed table was made; it cannot be made again from this tree.  AULE_LIBRARY_PATH named a build of commit d6c5f33
        # ("Forward: one host-side launch plan for route, workspace and grid"), the last one before the descriptor checkers.  That
        # library divided by zero fields in some entries: every call is tried in a forked copy first (TRAPPED).
        assert os.environ.get("AULE_LIBRARY_PATH"), "name the recorded library with AULE_LIBRARY_PATH"
        e = {k: v for k, v in os.environ.items() if not k.startswith("AULE_HIP_")}
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", sys.argv[2], "record"], env=e, check=True)
        sys.exit(0)
    gold, got = np.load(FIXTURE), run()
    for k in gold.files:
        same = gold[k].shape == got[k].shape and np.array_equal(gold[k], got[k])
        print(k, gold[k].shape, "equal" if same else "differences: %d" % (int((gold[k] != got[k]).sum()) if gold[k].shape == got[k].shape else -1))
