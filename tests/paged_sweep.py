"""The fixed sweep of good, bad and edge arguments behind tests/golden/paged_contract.json: what the paged family -- decode, FP8 decode,
query, prefill, cascade -- answers before it needs a device, through the C entries and through the Python wrappers, asked in a child
process that never initialises the library (default environment only: no AULE_HIP_* switch).

    python tests/paged_sweep.py            # prints the tree against the committed table, entry by entry

C entries: a case is a valid base descriptor of one kind (16-bit and FP8 caches, MHA, GQA and MQA between the bases) with one mutation --
one field set to a bad or edge value, or two fields whose rules fail together, which pins the order of the checks.  Recorded per case: the
kind's workspace query, the seven integers of aule_hip_debug_shared_prefix_plan, and for the two launch entries that check the descriptor
before they need a device (prefill, cascade) the return code and the whole text of aule_get_error().  The decode and query launch entries
answer -1 before they look at a descriptor in a process like this one; their refusals are the GPU suite's (tests/test_gpu_paged_refusals.py).

Python wrappers: the four calls on CPU tensors, one or two faults per case; recorded: the exception's type name and whole message.  The
decode is asked only what it answers before it loads the library (with CPU tensors it goes on to initialise it, and what that says
depends on the machine): its table and length rules, checked after the move to the device, are not in the table.

The table was recorded from commit 1c78223 ("Paged cascade: shared prefix read once per batch, plus a state merge"), the last one in
which every paged entry point carried its own copy of the argument rules, and it cannot be made again from this tree: a difference is a
bug, except the cases tests/test_paged_contract.py names by operation and mutation.  Without a device the CU count answers 256, which
is also the MI355X's, so the plans hold on every machine."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "paged_contract.json")
NAN = float("nan")
PTR = 4096                                                 # a 16-byte aligned non-null dummy: no entry asked here reads through it

# kind -> (the _capi structure, its workspace query or None, its device-free launch entry or None)
KINDS = {
    "decode": ("PagedDesc", "aule_attention_paged_decode_workspace_size", None),
    "decode_fp8": ("PagedFp8Desc", "aule_attention_paged_decode_fp8_workspace_size", None),
    "query": ("PagedQueryDesc", "aule_attention_paged_query_workspace_size", None),
    "prefill": ("PagedPrefillDesc", None, "aule_attention_paged_prefill_ex"),
    "cascade": ("PagedCascadeDesc", "aule_attention_paged_cascade_workspace_size", "aule_attention_paged_cascade_ex"),
}
# base problems: dtype, fp8, batch, heads_q, heads_kv, head_dim, block_size, max_blocks, scale     (heads_kv = 5 divides no heads_q here)
BASES = (
    (2, 0, 3, 32, 8, 128, 16, 64, 0.0),                    # bf16 GQA, 16-bit cache
    (1, 1, 2, 8, 8, 64, 16, 40, 0.125),                    # fp16 MHA, FP8 cache
    (2, 1, 4, 4, 1, 32, 24, 7, 0.0),                       # bf16 MQA, FP8 cache, a block size that is no power of two
    (1, 0, 1, 64, 8, 64, 1, 700, -0.1),                    # fp16 GQA 8:1, 16-bit cache, one-key blocks, negative scale
)
TENSORS = ("q", "k_cache", "v_cache", "block_tables", "context_lens", "cu_seqlens_q", "out", "prefix_block_table", "prefix_len")


def bases(kind):
    """The bases a kind can state: aule_paged_desc has no FP8 cache, aule_paged_fp8_desc nothing else."""
    return [i for i, b in enumerate(BASES) if kind not in ("decode", "decode_fp8") or b[1] == (kind == "decode_fp8")]


def fill(kind, base):
    from aule import _capi
    dtype, fp8, B, Hq, Hkv, D, bs, mb, scale = BASES[base]
    d = getattr(_capi, KINDS[kind][0])()
    names = {n for n, _ in d._fields_}
    d.struct_size = ctypes.sizeof(d)
    d.dtype, d.batch, d.heads_q, d.heads_kv, d.head_dim, d.block_size, d.max_blocks, d.scale = dtype, B, Hq, Hkv, D, bs, mb, scale
    for n, v in (("cache_dtype", fp8), ("window_size", -1), ("seq_q", 4), ("total_tokens", 700), ("max_seqlen_q", 512),
                 ("q_token_stride", Hq * D), ("max_prefix_blocks", 128)):
        if n in names:
            setattr(d, n, v)
    for n in TENSORS:
        if n in names:
            setattr(d, n, PTR)
    if fp8:
        d.k_scale = d.v_scale = PTR
    return d


def mutations(kind, base):
    """(name, {field: value}) for one kind and base, in the table's order; "struct_size" values are offsets from the kind's sizeof (None:
    struct_size 0).  A mutation that names a field the kind does not have is left out."""
    from aule import _capi
    dtype, fp8, B, Hq, Hkv, D, bs, mb, scale = BASES[base]
    names = {n for n, _ in getattr(_capi, KINDS[kind][0])._fields_}
    tok = Hq * D
    nulls = {n: None for n in TENSORS if n in names}
    one = ([("struct_size", v) for v in (None, -8, 8)] + [("dtype", v) for v in (-1, 0, 3)] + [("cache_dtype", v) for v in (2, -1, 1 - fp8)] +
           [("head_dim", v) for v in (0, 48, 256)] + [("heads_kv", v) for v in (0, 5)] + [("batch", 0), ("heads_q", 0), ("total_tokens", 0)] +
           [("block_size", 0)] + [("max_blocks", v) for v in (0, 1 << 26, 1 << 28)] + [("max_prefix_blocks", v) for v in (0, 1, 1 << 26)] +
           [("window_size", v) for v in (0, -5, 100)] + [("scale", v) for v in (0.0, NAN, -0.5)] + [("seq_q", v) for v in (0, 1, 64, 65)] +
           [("max_seqlen_q", v) for v in (0, 1, 1 << 20)] + [("q_token_stride", v) for v in (tok - 8, tok - 4, 0, -4096, tok + 4, 3 * tok)] +
           [("total_tokens", v) for v in (1, 1 << 29, 1 << 30)] + [("batch", 1 << 30)] + [(n, None) for n in TENSORS] +
           [("k_scale", None if fp8 else PTR), ("v_scale", None if fp8 else PTR), ("lse", PTR), ("workspace", PTR)] +
           [("q", PTR + 8), ("out", PTR + 2), ("k_cache", PTR + 1), ("v_cache", PTR + 4)])
    muts = [("none", {})] + [("%s=%r" % (f, v), {f: v}) for f, v in one]
    many = [  # nothing to do, with null pointers; then two rules that fail together
        ("batch=0,null", dict(nulls, batch=0)), ("heads_q=0,null", dict(nulls, heads_q=0, q_token_stride=0)),
        ("total_tokens=0,null", dict(nulls, total_tokens=0)), ("total_tokens=0+head_dim", {"total_tokens": 0, "head_dim": 256}),
        ("batch=0+head_dim", {"batch": 0, "head_dim": 256}), ("batch=0+misaligned", {"batch": 0, "q": PTR + 8}),
        ("struct_size+dtype", {"struct_size": -8, "dtype": 0}), ("dtype+cache_dtype", {"dtype": 0, "cache_dtype": 2}),
        ("dtype+head_dim", {"dtype": 0, "head_dim": 48}), ("cache_dtype+head_dim", {"cache_dtype": 2, "head_dim": 48}),
        ("head_dim+heads_kv", {"head_dim": 48, "heads_kv": 5}), ("heads_kv+seq_q", {"heads_kv": 5, "seq_q": 65}),
        ("heads_kv+block_size", {"heads_kv": 0, "block_size": 0}), ("seq_q+block_size", {"seq_q": 65, "block_size": 0}),
        ("max_blocks+max_prefix_blocks", {"max_blocks": 0, "max_prefix_blocks": 0}), ("block_size+max_seqlen_q", {"block_size": 0, "max_seqlen_q": 0}),
        ("max_prefix_blocks+max_seqlen_q", {"max_prefix_blocks": 0, "max_seqlen_q": 0}), ("max_seqlen_q+stride", {"max_seqlen_q": 0, "q_token_stride": 0}),
        ("stride+total_tokens", {"q_token_stride": tok + 4, "total_tokens": 1 << 30}), ("batch+rows", {"batch": 1 << 30, "total_tokens": 1 << 29}),
        ("rows+null", {"total_tokens": 1 << 29, "q": None}), ("stride+null", {"q_token_stride": tok + 4, "q": None}),
        ("block_size+null", {"block_size": 0, "out": None}), ("null+scale", {"k_cache": None, "k_scale": None if fp8 else PTR}),
        ("null+misaligned", {"context_lens": None, "q": PTR + 8}), ("scale+misaligned", {"v_scale": None if fp8 else PTR, "out": PTR + 2}),
    ]
    muts += many
    return [(name, fields) for name, fields in muts if all(f in names for f in fields)]


def c_cases():
    return [(kind, base, name, fields) for kind in KINDS for base in bases(kind) for name, fields in mutations(kind, base)]


def ask_c(lib):
    """{"kind/base/mutation": [workspace bytes or None, [plan return, the seven ints] or None, [return code, error text] or None]}"""
    from aule import _capi
    plan = (ctypes.c_int32 * 7)()
    out = {}
    for kind, base, name, fields in c_cases():
        d = fill(kind, base)
        for f, v in fields.items():
            if f == "struct_size":
                d.struct_size = 0 if v is None else ctypes.sizeof(d) + v
            else:
                setattr(d, f, v)
        _, size, entry = KINDS[kind]
        row = [int(getattr(lib, size)(ctypes.byref(d))) if size else None, None, None]
        if kind == "cascade":
            for i in range(7):
                plan[i] = -1
            row[1] = [int(lib.aule_hip_debug_shared_prefix_plan(ctypes.byref(d), plan, 7)), list(plan)]
        if entry:
            rc = int(getattr(lib, entry)(ctypes.byref(d)))
            row[2] = [rc, _capi.last_error(lib) if rc != 0 else ""]   # (a call that succeeds leaves the text of the one before)
        out["%s/%d/%s" % (kind, base, name)] = row
    return out


def py_cases():
    """(operation, name, the call as a thunk) in the table's order.  Every tensor is a CPU tensor; the shapes are those of the
    test_argument_errors_are_value_errors_before_any_launch tests."""
    import torch
    import aule
    from aule._torch import paged_decode
    B, T, Hq, Hkv, Sq, D, bs = 2, 10, 8, 2, 4, 64, 16
    f16 = torch.float16
    q = {"decode": torch.zeros(B, Hq, D, dtype=f16), "query": torch.zeros(B, Hq, Sq, D, dtype=f16), "prefill": torch.zeros(T, Hq, D, dtype=f16)}
    q["cascade"] = q["prefill"]
    c8 = torch.zeros(4, bs, Hkv, D).to(torch.float8_e4m3fn)
    c16 = torch.zeros(4, bs, Hkv, D, dtype=f16)
    bt, cl = torch.zeros(B, 2, dtype=torch.int32), torch.full((B,), 5, dtype=torch.int32)
    cu = torch.tensor([0, 5, 10], dtype=torch.int32)
    pbt, pl = torch.zeros(3, dtype=torch.int32), torch.tensor([20], dtype=torch.int32)
    fns = {"decode": paged_decode, "query": aule.flash_attention_paged_query, "prefill": aule.flash_attention_paged_prefill,
           "cascade": aule.flash_attention_paged_cascade}

    def cache(Hkv=Hkv, D=D, bs=bs, dtype=f16):
        return torch.zeros(4, bs, Hkv, D).to(dtype)

    def call(op, **kw):
        a = dict(q=q[op], k_cache=c16, v_cache=c16, block_tables=bt, context_lens=cl)
        if op in ("prefill", "cascade"):
            a["cu_seqlens_q"] = cu
        if op == "cascade":
            a.update(prefix_block_table=pbt, prefix_len=pl)
        for k, v in kw.items():
            if k == "caches":
                a["k_cache"] = a["v_cache"] = v
            else:
                a[k] = v
        return lambda: fns[op](**a)

    def qlike(op, D=D, dtype=f16, Hq=Hq):
        s = list(q[op].shape)
        s[1], s[-1] = Hq, D
        return torch.zeros(*s, dtype=dtype)

    cases = []
    for op in fns:
        ragged, own = op in ("prefill", "cascade"), []
        add = lambda name, **kw: own.append((op, name, call(op, **kw)))   # noqa: E731
        add("q_rank", q=q[op].unsqueeze(0).unsqueeze(0))
        add("cache_rank", caches=c16[0])
        add("v_cache_shape", v_cache=c16[:2])
        add("head_dim_mismatch", caches=cache(D=32))
        add("heads_kv=3", caches=cache(Hkv=3))
        add("heads_kv=0", caches=cache(Hkv=0))
        add("cache_dtypes_differ", k_cache=c8)
        for other in (torch.float8_e4m3fnuz, torch.float8_e5m2):
            add("cache_%s" % str(other).split(".")[1], caches=cache(dtype=other))
        add("q_fp32,fp8_cache", q=q[op].float(), caches=c8)
        add("q_fp32,fp32_cache", q=q[op].float(), caches=c16.float())
        add("q_fp16,bf16_cache", caches=c16.to(torch.bfloat16))
        add("k_scale,16_bit_cache", k_scale=0.5)
        add("v_scale,16_bit_cache", v_scale=torch.ones(Hkv))
        add("k_scale_shape", caches=c8, k_scale=torch.ones(Hkv + 1))
        add("v_scale_shape", caches=c8, v_scale=torch.ones(Hkv, 2))
        add("head_dim=256", q=qlike(op, D=256), caches=cache(D=256))
        add("head_dim=256,fp8", q=qlike(op, D=256), caches=cache(D=256, dtype=torch.float8_e4m3fn))
        # two faults at once: the order of the rules
        add("head_dim_mismatch+heads_kv", caches=cache(D=32, Hkv=3))
        add("heads_kv+cache_dtypes_differ", k_cache=cache(Hkv=3, dtype=torch.float8_e4m3fn), v_cache=cache(Hkv=3))
        add("q_fp32+k_scale,16_bit_cache", q=q[op].float(), caches=c16.float(), k_scale=0.5)
        add("k_scale,16_bit_cache+head_dim=256", q=qlike(op, D=256), caches=cache(D=256), k_scale=0.5)
        add("head_dim=256+k_scale_shape", q=qlike(op, D=256), caches=cache(D=256, dtype=torch.float8_e4m3fn), k_scale=torch.ones(Hkv + 1))
        add("k_scale_shape+v_scale_shape", caches=c8, k_scale=torch.ones(Hkv + 1), v_scale=torch.ones(Hkv, 2))
        if op == "decode":
            add("q_4d_one_token,k_scale_shape", q=q[op].unsqueeze(2), caches=c8, k_scale=torch.ones(Hkv + 1))   # accepted as far as the scale rule
            add("q_4d_four_tokens", q=q["query"])
            own.append((op, "public,cpu", lambda: aule.flash_attention_paged_amd(q["decode"], c16, c16, bt, cl)))
            cases += own
            continue                                       # (what follows the decode answers only with the library initialised)
        add("block_size=0", caches=cache(bs=0))
        for name, bad_bt, bad_cl in (("bt_rank", bt[0], cl), ("cl_short", bt, cl[:1]), ("max_blocks=0", bt[:, :0], cl), ("cl_rank", bt, cl.view(B, 1))):
            add(name, block_tables=bad_bt, context_lens=bad_cl)
        add("head_dim=256+block_size=0", q=qlike(op, D=256), caches=cache(D=256, bs=0))
        add("block_size=0+bt_rank", caches=cache(bs=0), block_tables=bt[0])
        add("bt_rank+k_scale_shape", caches=c8, block_tables=bt[0], k_scale=torch.ones(Hkv + 1))
        if op == "query":
            add("bt_batch", block_tables=bt[:1])
            for n in (0, 65):
                add("seq_q=%d" % n, q=torch.zeros(B, Hq, n, D, dtype=f16))
            add("heads_kv+seq_q", q=torch.zeros(B, Hq, 65, D, dtype=f16), caches=cache(Hkv=3))
            add("seq_q+cache_dtypes_differ", q=torch.zeros(B, Hq, 65, D, dtype=f16), k_cache=c8)
        if ragged:
            for name, bad in (("cu_short", cu[:2]), ("cu_long", torch.zeros(B + 2, dtype=torch.int32)), ("cu_rank", cu.view(1, B + 1)), ("cu_list", [0, 5, 10])):
                add(name, cu_seqlens_q=bad)
            for name, bad in (("cu_int64", cu.long()), ("cu_fp32", cu.float()), ("cu_int16", cu.to(torch.int16))):
                add(name, cu_seqlens_q=bad)
            for bad in (0, -3, 2.5, True):
                add("max_seqlen_q=%r" % (bad,), max_seqlen_q=bad)
            wide = torch.zeros(T, Hq * D + 4, dtype=f16)
            add("q_stride", q=wide[:, :Hq * D].view(T, Hq, D))
            add("q_offset", q=torch.zeros(T * Hq * D + 4, dtype=f16)[4:].view(T, Hq, D))
            add("bt_rank+cu_short", block_tables=bt[0], cu_seqlens_q=cu[:2])
            add("cu_long+cu_int64", cu_seqlens_q=torch.zeros(B + 2, dtype=torch.int64))
            add("cu_int64+max_seqlen_q", cu_seqlens_q=cu.long(), max_seqlen_q=0)
            add("max_seqlen_q+k_scale_shape", caches=c8, max_seqlen_q=0, k_scale=torch.ones(Hkv + 1))
            add("k_scale_shape+q_stride", q=wide[:, :Hq * D].view(T, Hq, D), caches=c8, k_scale=torch.ones(Hkv + 1))
            fused = torch.zeros(T, 3 * Hq * D, dtype=f16)
            add("ok,fused_slice", q=fused[:, Hq * D:2 * Hq * D].view(T, Hq, D), max_seqlen_q=5)
            add("ok,heads_transposed", q=torch.zeros(Hq, T, D, dtype=f16).transpose(0, 1))
            add("ok,one_token", q=q[op][:1], cu_seqlens_q=torch.tensor([0, 1, 1], dtype=torch.int32))
        if op == "cascade":
            for name, bad in (("pbt_empty", pbt[:0]), ("pbt_rank", pbt.view(1, 3)), ("pbt_fp32", pbt.float()), ("pbt_list", [0, 1, 2])):
                add(name, prefix_block_table=bad)
            for name, bad in (("pl_int64", pl.long()), ("pl_two", torch.zeros(2, dtype=torch.int32)), ("pl_0d", torch.tensor(20, dtype=torch.int32)),
                              ("pl_float", 2.5), ("pl_bool", True), ("pl_none", None), ("pl_2^31", 1 << 31)):
                add(name, prefix_len=bad)
            add("block_size=0+pbt_empty", caches=cache(bs=0), prefix_block_table=pbt[:0])
            add("pbt_empty+pl_int64", prefix_block_table=pbt[:0], prefix_len=pl.long())
            add("pl_int64+bt_rank", prefix_len=pl.long(), block_tables=bt[0])
            add("window_size", window_size=16)
            for n in (20, 0, -5):
                add("ok,prefix_len=%d" % n, prefix_len=n, max_seqlen_q=5)
            add("ok,pbt_int64", prefix_block_table=pbt.long())
        add("ok", **({"max_seqlen_q": 5} if ragged else {}))
        add("ok,fp8,scales", caches=c8, k_scale=0.5, v_scale=torch.ones(Hkv), return_lse=True)
        add("ok,fp8,scalar_tensor_scales", caches=c8, k_scale=torch.tensor(0.5), v_scale=torch.ones(1))
        cases += own
    return cases


def ask_py():
    """{"operation/case": [exception type name, message]} ("" and "" for a call that returns)"""
    import aule

    def refuse():
        raise AssertionError("the sweep reached the library: CPU tensors must be refused before it")
    aule._capi.get_lib = refuse
    out = {}
    for op, name, thunk in py_cases():
        try:
            thunk()
            out["%s/%s" % (op, name)] = ["", ""]
        except Exception as e:   # noqa: BLE001
            out["%s/%s" % (op, name)] = [type(e).__name__, str(e)]
    assert aule._capi._initialized is False, "the sweep must not initialise the library"
    return out


def ask(path):
    """Every case through the package and the library loaded in THIS process (what the child process runs), saved to `path`."""
    sys.path.insert(0, os.path.join(ROOT, "aule-attention_amd"))
    from aule import _capi
    table = {"c": ask_c(_capi.load()), "py": ask_py()}
    with open(path, "w") as fh:
        json.dump(table, fh, indent=0, sort_keys=True)
        fh.write("\n")


def run():
    """What the tree answers for every case, in a child process without any AULE_HIP_* switch: {"c": ..., "py": ...}."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("AULE_HIP_")}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "paged.json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        with open(path) as fh:
            return json.load(fh)


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


def differences(gold, got):
    """[(table, key, recorded, now)] over the union of the keys (None: the entry is missing on that side)"""
    return [(t, k, gold[t].get(k), got[t].get(k)) for t in ("c", "py") for k in sorted(set(gold[t]) | set(got[t])) if gold[t].get(k) != got[t].get(k)]


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        ask(sys.argv[2])
        sys.exit(0)
    if len(sys.argv) > 2 and sys.argv[1] == "--record":
        # How the committed table was made; it cannot be made again from this tree: this file ran in a checkout of commit 1c78223, and
        # AULE_LIBRARY_PATH named the library built from it.
        assert os.environ.get("AULE_LIBRARY_PATH"), "name the recorded library with AULE_LIBRARY_PATH"
        e = {k: v for k, v in os.environ.items() if not k.startswith("AULE_HIP_")}
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", sys.argv[2]], env=e, check=True)
        sys.exit(0)
    gold, got = load_fixture(), run()
    diff = differences(gold, got)
    print("c: %d entries, py: %d entries, %d differ" % (len(gold["c"]), len(gold["py"]), len(diff)))
    for t, k, was, now in diff:
        print(" ", t, k, "recorded", was, "now", now)
