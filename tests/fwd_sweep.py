"""The fixed sweep of forward problems behind tests/golden/fwd_plan_sweep.npz, and the child process that asks the library
about every case of it (the switches are read once per process, so every leg is a process of its own).

    python tests/fwd_sweep.py            # prints the library in the tree against the committed table, leg by leg

The table was recorded from the library BEFORE the forward's launch plan (fa_fwd_plan.h) replaced the two dispatch ladders and
the dry-run size queries: routes, workspace sizes and route 7's split plan from that library as it was, the sub-plans (route 8
grid, route 4 chunk plan, route 5 plan, fp32 pieces) from a copy of it whose launchers reported the values they computed.  It is
not regenerated when a value changes: a difference is a bug.  Without a device the CU count answers 256, so the table holds on
every machine."""
import itertools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "fwd_plan_sweep.npz")

DTYPES = (0, 1, 2)
BATCHES = (1, 4, 32)
HEADS = ((8, 8), (32, 8), (16, 1))                      # MHA, GQA, MQA
DIMS = (32, 64, 128, 256)
CAUSALS = (0, 1, 2)                                     # 2 = bottom-right (the short chunk against a KV history)
WINDOWS = (-1, 100, 512)
SCALES = (0.125, -0.1, 0.0)                             # 0 = the default 1 / sqrt(D)
SEQS = ((1, 1024), (1, 8192), (1, 32768), (16, 1024), (16, 8192), (16, 32768), (64, 1024), (64, 8192), (64, 32768),   # routes 4 / 5
        (512, 512), (2048, 2048), (4096, 4096), (8192, 8192),                                                          # routes 7 / 8
        (128, 128), (512, 192), (300, 300), (1000, 5000))                                                              # short K (route 1), odd sizes
# leg name -> environment on top of one with no AULE_HIP_FWD_* / AULE_HIP_W4_* / AULE_HIP_F32_SPLIT variable
LEGS = {
    "default": {},
    "kernel_pp": {"AULE_HIP_FWD_KERNEL": "pp"},
    "softmax_classic": {"AULE_HIP_FWD_SOFTMAX": "classic"},
    "splitkv_0": {"AULE_HIP_FWD_SPLITKV": "0"},
    "ppsplit_0": {"AULE_HIP_FWD_PPSPLIT": "0"},
    "split_0": {"AULE_HIP_FWD_SPLIT": "0"},
    "w4_window_0": {"AULE_HIP_W4_WINDOW": "0"},
    "w4_unpair_0": {"AULE_HIP_W4_UNPAIR": "0"},
    "w4_order_pairs": {"AULE_HIP_W4_ORDER": "pairs"},
    "f32_split_0": {"AULE_HIP_F32_SPLIT": "0"},
}
# sub-plan integers of aule_hip_debug_forward_plan behind {route, bytes low, bytes high}, by route (include/aule.h)
SUB_INTS = {0: 1, 1: 0, 4: 5, 5: 8, 7: 4, 8: 6, 9: 0}

PAGED_BATCHES = (1, 2, 8, 64)
PAGED_HEADS = ((4, 1), (32, 8), (8, 8))
PAGED_DIMS = (32, 64, 128)
PAGED_BLOCK_SIZES = (16, 32, 128)
PAGED_MAX_BLOCKS = (1, 64, 2048)


def cases():
    """(dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, scale) in the table's order (bottom-right needs Sk >= Sq)."""
    return [(dt, B, hq, hkv, sq, sk, D, c, w, s)
            for dt, B, (hq, hkv), (sq, sk), D, c, w, s in itertools.product(DTYPES, BATCHES, HEADS, SEQS, DIMS, CAUSALS, WINDOWS, SCALES)
            if not (c == 2 and sk < sq)]


def paged_cases():
    """(dtype, B, Hq, Hkv, D, block_size, max_blocks, fp8) in the table's order."""
    return [(dt, B, hq, hkv, D, bs, mb, fp8)
            for dt, B, (hq, hkv), D, bs, mb, fp8 in itertools.product((1, 2), PAGED_BATCHES, PAGED_HEADS, PAGED_DIMS, PAGED_BLOCK_SIZES,
                                                                      PAGED_MAX_BLOCKS, (0, 1))]


_CHILD = r'''
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from aule import _capi
import fwd_sweep
lib = ctypes.CDLL(_capi.find_library())
P, I32 = ctypes.POINTER(_capi.AttnDesc), ctypes.c_int32
route = lib.aule_hip_debug_forward_route; route.restype, route.argtypes = I32, [P]
size = lib.aule_attention_forward_workspace_size; size.restype, size.argtypes = ctypes.c_uint64, [P]
split = lib.aule_hip_debug_forward_split_plan; split.restype, split.argtypes = I32, [P, ctypes.POINTER(I32), I32]
plan = getattr(lib, "aule_hip_debug_forward_plan", None)
if plan is not None:
    plan.restype, plan.argtypes = I32, [P, ctypes.POINTER(I32), I32]
buf = (I32 * 4096)()
d = _capi.AttnDesc()
d.struct_size = ctypes.sizeof(_capi.AttnDesc)
ref = ctypes.byref(d)
routes, sizes, splits, split_off, plans, plan_off = [], [], [], [0], [], [0]
for (dt, B, hq, hkv, sq, sk, D, c, w, s) in fwd_sweep.cases():
    d.dtype, d.causal, d.window_size, d.scale = dt, c, w, s
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, hq, hkv, sq, sk, D
    r = route(ref)
    routes.append(r)
    sizes.append(size(ref))
    if r == 7:
        n = split(ref, buf, 4096)
        assert n > 0, n
        splits.extend(buf[:n])
    else:
        assert split(ref, None, 0) == 0
    split_off.append(len(splits))
    if plan is not None:
        n = plan(ref, buf, 4096)
        assert n >= 3 and plan(ref, None, 0) == -n and plan(ref, buf, n - 1) == -n, n
        plans.extend(buf[:n])
        plan_off.append(len(plans))
out = {"route": np.asarray(routes, np.int8), "ws": np.asarray(sizes, np.int64),
       "split": np.asarray(splits, np.int32), "split_off": np.asarray(split_off, np.int32)}
if plan is not None:
    out["plan"], out["plan_off"] = np.asarray(plans, np.int32), np.asarray(plan_off, np.int32)
if sys.argv[4] == "paged":
    psize = lib.aule_attention_paged_decode_workspace_size
    psize.restype, psize.argtypes = ctypes.c_uint64, [ctypes.POINTER(_capi.PagedDesc)]
    psize8 = lib.aule_attention_paged_decode_fp8_workspace_size
    psize8.restype, psize8.argtypes = ctypes.c_uint64, [ctypes.POINTER(_capi.PagedFp8Desc)]
    paged = []
    for (dt, B, hq, hkv, D, bs, mb, fp8) in fwd_sweep.paged_cases():
        p = _capi.PagedFp8Desc() if fp8 else _capi.PagedDesc()
        p.struct_size = ctypes.sizeof(p)
        p.dtype, p.batch, p.heads_q, p.heads_kv, p.head_dim, p.block_size, p.max_blocks, p.window_size = dt, B, hq, hkv, D, bs, mb, -1
        paged.append((psize8 if fp8 else psize)(ctypes.byref(p)))
    out["paged"] = np.asarray(paged, np.int64)
np.savez(sys.argv[3], **out)
'''


def run_leg(env, paged=False):
    """What the library answers for every case of the sweep, in a child process with `env` on top of a clean one: "route", "ws",
    route 7's dumps ("split", case i at split_off[i] : split_off[i + 1]) and, where the library has aule_hip_debug_forward_plan,
    its output ("plan", "plan_off"); paged: the two paged workspace-size entries over paged_cases() as well ("paged")."""
    import numpy as np
    e = {k: v for k, v in os.environ.items() if not k.startswith(("AULE_HIP_FWD_", "AULE_HIP_W4_")) and k != "AULE_HIP_F32_SPLIT"}
    e.update(env)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "leg.npz")
        r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "aule-attention_amd"), os.path.join(ROOT, "tests"), path,
                            "paged" if paged else ""], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


def sub_plans(leg):
    """The sub-plan integers of a run_leg() result as one flat array and its offsets: "plan" without the three leading ints."""
    import numpy as np
    off = leg["plan_off"]
    keep = np.ones(leg["plan"].size, bool)
    for j in range(3):
        keep[off[:-1] + j] = False
    return leg["plan"][keep], off - 3 * np.arange(off.size, dtype=off.dtype)


if __name__ == "__main__":
    import numpy as np
    if len(sys.argv) > 1 and sys.argv[1] == "--record":
        # How the committed table was made; it cannot be made again from this tree.  AULE_LIBRARY_PATH named the library of the
        # commit before fa_fwd_plan.h, AULE_SWEEP_SUB_LIBRARY a build of that commit plus a dump hook that was never committed (its
        # patch is in the description of the pull request that added this file): its launchers reported the values they computed
        # through an aule_hip_debug_forward_plan of the same output contract.
        table = {}
        for leg, env in LEGS.items():
            got = run_leg(env, paged=leg == "default")
            assert "plan" not in got
            sub = run_leg(dict(env, AULE_LIBRARY_PATH=os.environ["AULE_SWEEP_SUB_LIBRARY"]))
            for k in ("route", "ws", "split", "split_off"):
                assert np.array_equal(got[k], sub[k]), (leg, k)
                table[leg + "." + k] = got[k]
            table[leg + ".sub"], table[leg + ".sub_off"] = sub_plans(sub)
            if "paged" in got:
                table["paged"] = got["paged"]
        np.savez_compressed(sys.argv[2], **table)
        sys.exit(0)
    gold = np.load(FIXTURE)
    for leg, env in LEGS.items():
        got = run_leg(env)
        print(leg, "cases", got["route"].size, "differences:", "route", int((got["route"] != gold[leg + ".route"]).sum()),
              "ws", int((got["ws"] != gold[leg + ".ws"]).sum()), "split", int(not np.array_equal(got["split"], gold[leg + ".split"])))
