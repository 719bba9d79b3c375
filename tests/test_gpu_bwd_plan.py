"""The backward's launch plan and its launch are the same thing: for shapes that between them reach every route bit, what
aule_attention_backward_ex ran (aule_hip_debug_last_backward_route, stored by the launcher from the plan it executes) is what
aule_hip_debug_backward_route answers for the same descriptor without a device (csrc/fa_bwd_plan.h)."""
import ctypes
import os

import pytest

pytestmark = pytest.mark.gpu

F32, F16, BF16 = 0, 1, 2
# (name, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, workspace: "want" = what the size query asks for, "min" = without the dS room)
SHAPES = [
    ("fp32", F32, 1, 4, 4, 128, 128, 64, 1, -1, "want"),
    ("d256 bf16", BF16, 1, 4, 2, 256, 256, 256, 1, -1, "want"),
    ("d256 fp32", F32, 1, 2, 2, 128, 128, 256, 0, -1, "want"),
    ("d32", BF16, 1, 4, 4, 200, 200, 32, 1, -1, "want"),
    ("bf16 d128 mha causal", BF16, 2, 8, 8, 512, 512, 128, 1, -1, "want"),
    ("fp16 d128 gqa full", F16, 2, 8, 2, 384, 384, 128, 0, -1, "want"),
    ("bf16 d64 mha causal, two key blocks per wave", BF16, 4, 32, 32, 2048, 2048, 64, 1, -1, "want"),
    ("fp16 d64 gqa full", F16, 1, 8, 2, 300, 300, 64, 0, -1, "want"),
    ("bottom-right", BF16, 1, 8, 2, 256, 640, 128, 2, -1, "want"),
    ("windowed causal", BF16, 1, 8, 8, 512, 512, 128, 1, 100, "want"),
    ("spill-sized, dS room", BF16, 1, 8, 8, 2048, 2048, 128, 1, -1, "want"),
    ("spill-sized, no dS room", BF16, 1, 8, 8, 2048, 2048, 128, 1, -1, "min"),
    ("fp16 mqa 32/1 on the head-split kernel", F16, 1, 32, 1, 8192, 8192, 128, 1, -1, "want"),
    ("one query bottom-right, dS room", F16, 1, 32, 8, 1, 8192, 128, 2, -1, "want"),
    ("one query bottom-right, no dS room", F16, 1, 32, 8, 1, 8192, 128, 2, -1, "min"),
]


def test_the_launch_runs_what_the_plan_says():
    import torch
    from aule import _capi
    for var in os.environ:
        assert not var.startswith("AULE_HIP_BWD_"), var    # (the default dispatch; the switches are read once per process)
    lib = _capi.get_lib()
    seen = {}
    for name, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, room in SHAPES:
        tdt = (torch.float32, torch.float16, torch.bfloat16)[dtype]
        gen = torch.Generator(device="cuda").manual_seed(5)
        q, out, do = (torch.randn(B, Hq, Sq, D, device="cuda", dtype=tdt, generator=gen) for _ in range(3))
        k, v = (torch.randn(B, Hkv, Sk, D, device="cuda", dtype=tdt, generator=gen) for _ in range(2))
        lse = torch.full((B, Hq, Sq), 5.0, device="cuda", dtype=torch.float32)   # (any finite values: only the route is asserted)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        d = _capi.AttnBwdDesc()
        d.struct_size = ctypes.sizeof(_capi.AttnBwdDesc)
        d.dtype = dtype
        d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, Sq, Sk, D
        d.scale, d.causal, d.window_size, d.device = D ** -0.5, causal, window, torch.cuda.current_device()
        d.stream = torch.cuda.current_stream().cuda_stream
        d.q, d.k, d.v, d.out, d.dout, d.lse = (t.data_ptr() for t in (q, k, v, out, do, lse))
        d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
        n = int(lib.aule_attention_backward_workspace_size(ctypes.byref(d)))
        if room == "min":       # the dS room is whole batch elements of DsLayout units at the end
            n -= B * Hkv * 4 * ((Sk + 127) // 128) * (Hq // Hkv) * ((Sq + 31) // 32) * 2048
            d.workspace_bytes = n - 1
            assert lib.aule_hip_debug_backward_route(ctypes.byref(d)) == -3, name     # it IS the minimum
        ws = torch.empty((n,), device="cuda", dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), n
        planned = int(lib.aule_hip_debug_backward_route(ctypes.byref(d)))
        _capi.check(lib.aule_attention_backward_ex(ctypes.byref(d)), "aule_attention_backward_ex")
        torch.cuda.synchronize()
        ran = int(lib.aule_hip_debug_last_backward_route())
        print(name, "planned", planned, "ran", ran)
        assert planned > 0 and ran == planned, (name, planned, ran)
        assert not name.endswith(", dS room") or ran & 1, (name, ran)
        assert not name.endswith(", no dS room") or not ran & 1, (name, ran)
        seen[name] = ran
    assert seen["fp32"] == 32 and seen["d256 bf16"] == 128 and seen["d256 fp32"] == 128 | 32 and seen["d32"] == 8 | 16, seen
    assert seen["bf16 d64 mha causal, two key blocks per wave"] == 2 | 4 | 64, seen
    assert seen["fp16 mqa 32/1 on the head-split kernel"] & 16, seen
    bits = 0
    for r in seen.values():
        bits |= r
    assert bits == 255, seen
