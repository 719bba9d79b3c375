"""The fixed sweep of backward problems behind tests/golden/bwd_workspace_sweep.npz, and the child process that asks the
library about every case of it (the mode switches are read once per process, so every leg is a process of its own).

    python tests/bwd_sweep.py            # prints the sizes of the library in the tree against the committed table

The table was recorded from the library BEFORE the backward's launch plan (fa_bwd_plan.h) replaced the size functions; it is
not regenerated when a size changes: a difference is a bug."""
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "bwd_workspace_sweep.npz")

DTYPES = (0, 1, 2)
BATCHES = (1, 4, 64)
HEADS = ((1, 1), (8, 8), (32, 8), (32, 1))
SEQS = ((1, 8192), (64, 64), (300, 300), (2048, 2048), (4096, 4096), (1000, 5000))
DIMS = (32, 64, 128, 256)
CAUSALS = (0, 1, 2)
WINDOWS = (-1, 100)
# leg name -> environment on top of one with no AULE_HIP_BWD_* / AULE_HIP_F32_SPLIT variable
LEGS = {
    "default": {},
    "spill": {"AULE_HIP_BWD_MODE": "spill"},
    "recompute": {"AULE_HIP_BWD_MODE": "recompute"},
    "dkv_old": {"AULE_HIP_BWD_DKV": "old"},
    "dkv_new": {"AULE_HIP_BWD_DKV": "new"},
}


def cases():
    """(dtype, B, Hq, Hkv, Sq, Sk, D, causal, window) in the table's order."""
    return [(dt, B, hq, hkv, sq, sk, D, c, w)
            for dt, B, (hq, hkv), (sq, sk), D, c, w in itertools.product(DTYPES, BATCHES, HEADS, SEQS, DIMS, CAUSALS, WINDOWS)]


_CHILD = r'''
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from aule import _capi
import bwd_sweep
lib = ctypes.CDLL(_capi.find_library())
size = lib.aule_attention_backward_workspace_size
size.restype, size.argtypes = ctypes.c_uint64, [ctypes.POINTER(_capi.AttnBwdDesc)]
route = getattr(lib, "aule_hip_debug_backward_route", None)
if route is not None:
    route.restype, route.argtypes = ctypes.c_int32, [ctypes.POINTER(_capi.AttnBwdDesc)]
want, r_want, r_extra = [], [], json.loads(sys.argv[3])
for i, (dt, B, hq, hkv, sq, sk, D, c, w) in enumerate(json.loads(sys.argv[4]) or bwd_sweep.cases()):
    d = _capi.AttnBwdDesc()
    d.struct_size = ctypes.sizeof(_capi.AttnBwdDesc)
    d.dtype, d.causal, d.window_size = dt, c, w
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, hq, hkv, sq, sk, D
    want.append(int(size(ctypes.byref(d))))
    if route is not None:
        d.workspace_bytes = want[-1]
        r_want.append(int(route(ctypes.byref(d))))
        if r_extra:                      # ... and with the workspace sizes the caller names (one per case)
            d.workspace_bytes = r_extra[i]
            r_extra[i] = int(route(ctypes.byref(d)))
print(json.dumps({"want": want, "route_want": r_want, "route_extra": r_extra}))
'''


def run_leg(env, extra_ws=None, cases=None):
    """Sizes ("want") and, where the library has the hook, routes with that much workspace ("route_want") of every case of the sweep
    (or of `cases`) in a child process with `env` on top of a clean one.  extra_ws: one workspace_bytes per case to ask the route
    hook about as well ("route_extra")."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("AULE_HIP_BWD_") and k != "AULE_HIP_F32_SPLIT"}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "aule-attention_amd"), os.path.join(ROOT, "tests"),
                        json.dumps(extra_ws or []), json.dumps(cases)], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    import numpy as np
    if len(sys.argv) > 1 and sys.argv[1] == "--record":   # (how the committed table was made, from the parent's library)
        np.savez_compressed(sys.argv[2], **{leg: np.asarray(run_leg(env)["want"], dtype=np.int64) for leg, env in LEGS.items()})
        sys.exit(0)
    gold = np.load(FIXTURE)
    for leg, env in LEGS.items():
        got = np.asarray(run_leg(env)["want"], dtype=np.int64)
        print(leg, "cases", got.size, "differences", int((got != gold[leg]).sum()))
