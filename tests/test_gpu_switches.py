"""The run-time switches whose effect the plan tables do not see, or see only in part (csrc/fa_switches.h): they change how a launcher
fills its kernel's parameters, which of two kernels it starts, or a grid the recorded sweeps reach on few shapes, so tests/fwd_sweep.py
and tests/bwd_sweep.py alone cannot tell a reader that lost them from one that reads them.  One small case per switch, each in a child process of its own with the switch set (the library reads its switches
once per process): the child asserts through aule_hip_debug_switches that the switch is in force, runs the case, asserts the route
that ran through the last-route hooks and compares output and LSE (gradients for the backward case) with the fp64 oracle at the
suite's bounds (tests/util.py).  The children run one after another, each under its own time limit; after the first one that
exits non-zero no further child is started."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FWD_W4 = ("bf16", 1, 2, 2, 512, 512, 128, 1, -1)        # route 8, two Q blocks, eight KV tiles in the longer one
FWD_WIN = ("fp16", 1, 2, 2, 512, 512, 128, 1, 128)      # route 8's window instances (route 1 with the window instances off)
FWD_SHORT = ("bf16", 1, 8, 2, 4, 1024, 64, 0, -1)       # route 5 by the plan (two units: not route 4's corner): 16 partials per row, so the merge of the
                                                        # split-KV file that routes 4 and 5 share picks its kernel by the switch
BWD_SPILL = ("bf16", 1, 2, 2, 256, 256, 128, 1, -1)     # the 5-matmul backward: dQ = dS K runs
# (id, environment = the words aule_hip_debug_switches must report, direction, case, route that must have run)
CASES = [
    ("w4-bodies-generic", {"AULE_HIP_W4_BODIES": "generic"}, "fwd", FWD_W4, 8),
    ("w4-order-pairs", {"AULE_HIP_W4_ORDER": "pairs"}, "fwd", FWD_W4, 8),
    ("w4-unpair-0", {"AULE_HIP_W4_UNPAIR": "0"}, "fwd", FWD_W4, 8),
    ("w4-window-0", {"AULE_HIP_W4_WINDOW": "0"}, "fwd", FWD_WIN, 1),
    ("w4-wtail-0", {"AULE_HIP_W4_WTAIL": "0"}, "fwd", FWD_WIN, 8),
    ("w4-wtail-99", {"AULE_HIP_W4_WTAIL": "99"}, "fwd", FWD_WIN, 8),
    ("fwd-combine-wg", {"AULE_HIP_FWD_COMBINE": "wg"}, "fwd", FWD_SHORT, 5),
    ("dqs-rev-0", {"AULE_HIP_DQS_REV": "0", "AULE_HIP_BWD_MODE": "spill"}, "bwd", BWD_SPILL, 1 | 4),
]

_CHILD = r'''
import json, math, os, sys
root = sys.argv[1]
sys.path[:0] = [os.path.join(root, "aule-attention_amd"), root, os.path.join(root, "tests")]
from util import BWD_TOL, LSE_TOL, assert_close, assert_switches, fwd_tol, quantize, torch_dtype
import numpy as np, torch                               # (torch first: the library binds to the HIP runtime torch brings)
import oracle
want, direction, (dtype, B, Hq, Hkv, Sq, Sk, D, causal, W), route = json.loads(sys.argv[2])
assert_switches(want)                                   # first: the leg's switches are what the library resolved
from aule import _capi, _torch as at
rng = np.random.RandomState(29)
q, k, v, do = (quantize(rng.randn(*s).astype(np.float32), dtype) for s in ((B, Hq, Sq, D), (B, Hkv, Sk, D), (B, Hkv, Sk, D), (B, Hq, Sq, D)))
tq, tk, tv, tdo = (torch.from_numpy(x).to("cuda", torch_dtype(dtype)) for x in (q, k, v, do))
sc = 1 / math.sqrt(D)
out, lse = at.fwd_raw(tq, tk, tv, causal, sc, window=W)
torch.cuda.synchronize()
lib = _capi.get_lib()
if direction == "fwd":
    ran = int(lib.aule_hip_debug_last_forward_route())
    assert ran == route, ("forward route", ran, route)
ref, ref_lse = oracle.fwd_f64(q, k, v, bool(causal), None, W)
atol, rtol = fwd_tol(dtype, np.abs(v).max())
o, l = out.float().cpu().numpy(), lse.cpu().numpy()
print("max |out - ref| %.3e (atol %.3e), max |lse - ref| %.3e (%.1e)" % (np.abs(o - ref).max(), atol, np.abs(l - ref_lse).max(), LSE_TOL[dtype]))
assert_close(o, ref, atol, rtol, "out")
assert_close(l, ref_lse, LSE_TOL[dtype], 1e-5, "lse")
if direction == "bwd":
    dq, dk, dv = at.bwd_raw(tq, tk, tv, out, tdo, lse, causal, sc, window=W)
    torch.cuda.synchronize()
    ran = int(lib.aule_hip_debug_last_backward_route())
    assert ran == route, ("backward route", ran, route)
    a, r = BWD_TOL[dtype]
    for name, got, ref_g in zip(("dq", "dk", "dv"), (dq, dk, dv), oracle.bwd_f64(q, k, v, do, bool(causal), None, W)):
        g = got.float().cpu().numpy()
        print("max |%s - ref| %.3e of max |ref| %.3e" % (name, np.abs(g - ref_g).max(), np.abs(ref_g).max()))
        assert_close(g, ref_g, a * max(1.0, float(np.abs(ref_g).max())), r, name)
print("CASE OK")
'''

_stopped = []   # the id of the first case whose child exited non-zero: nothing more runs on the device after it


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_switch_outside_the_plan_tables(case, oracle_mod):
    name, env, direction, shape, route = case
    assert not _stopped, "the child of %s exited non-zero: no further child is started" % _stopped[0]
    e = {k: v for k, v in os.environ.items() if not k.startswith(("AULE_HIP_FWD_", "AULE_HIP_W4_", "AULE_HIP_BWD_", "AULE_HIP_DQS_"))}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps([env, direction, shape, route])], env=e, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _stopped.append(name)
        raise
    print(r.stdout[-2000:])
    if r.returncode != 0:
        _stopped.append(name)
    assert r.returncode == 0 and "CASE OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]

