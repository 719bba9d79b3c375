"""head_dim 256 without a GPU: the forward route the dispatcher picks, the workspace the backward asks for, and a resource audit
of the compiled D = 256 kernels (no scratch, no VGPR or SGPR spill in any instance)."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

from aule import _capi

ROUTE_D256 = 9
CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")


def _lib():
    lib = ctypes.CDLL(_capi.find_library())
    lib.aule_hip_debug_forward_route.restype = ctypes.c_int32
    lib.aule_hip_debug_forward_route.argtypes = [ctypes.POINTER(_capi.AttnDesc)]
    lib.aule_attention_backward_workspace_size.restype = ctypes.c_uint64
    lib.aule_attention_backward_workspace_size.argtypes = [ctypes.POINTER(_capi.AttnBwdDesc)]
    lib.aule_attention_forward_workspace_size.restype = ctypes.c_uint64
    lib.aule_attention_forward_workspace_size.argtypes = [ctypes.POINTER(_capi.AttnDesc)]
    return lib


def _desc(cls, dtype, B, Hq, Hkv, Sq, Sk, D, causal=0, window=-1, scale=0.0):
    d = cls()
    d.struct_size = ctypes.sizeof(cls)
    d.dtype, d.causal, d.window_size, d.scale = dtype, causal, window, scale
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, Sq, Sk, D
    return d


def _route(*a, **kw):
    return _lib().aule_hip_debug_forward_route(ctypes.byref(_desc(_capi.AttnDesc, *a, **kw)))


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("causal,window", [(0, -1), (1, -1), (2, -1), (0, 100), (1, 7), (2, 1000)])
@pytest.mark.parametrize("B,Hq,Hkv,Sq,Sk", [(1, 8, 8, 1, 8192), (8, 32, 8, 1, 8192), (2, 16, 16, 65, 1025),
                                           (4, 16, 16, 4096, 4096), (1, 32, 1, 8192, 8192), (1, 4, 2, 1000, 5000)])
def test_head_dim_256_takes_its_own_route(dtype, causal, window, B, Hq, Hkv, Sq, Sk):
    assert _route(dtype, B, Hq, Hkv, Sq, Sk, 256, causal, window) == ROUTE_D256
    assert _route(dtype, B, Hq, Hkv, Sq, Sk, 256, causal, window, scale=-0.2) == ROUTE_D256


def test_fp32_head_dim_256_stays_on_the_fp32_route():
    assert _route(0, 4, 16, 16, 4096, 4096, 256, 1) == 0
    assert _route(0, 1, 8, 2, 1, 8192, 256, 0) == 0


def test_head_dims_up_to_128_never_take_route_9():
    for D in (32, 64, 128):
        for shape in ((1, 8, 8, 1, 8192), (4, 32, 32, 4096, 4096), (1, 4, 2, 1000, 5000)):
            for causal in (0, 1, 2):
                assert _route(2, *shape, D, causal) != ROUTE_D256


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_backward_workspace_at_256_is_delta(dtype):
    lib = _lib()
    for B, Hq, Hkv, Sq, Sk in ((4, 16, 16, 4096, 4096), (1, 32, 8, 65, 1025), (2, 8, 1, 1, 777)):
        ws = lib.aule_attention_backward_workspace_size(ctypes.byref(_desc(_capi.AttnBwdDesc, dtype, B, Hq, Hkv, Sq, Sk, 256, 1)))
        assert ws > 0
        assert ws == (B * Hq * Sq * 4 + 255) // 256 * 256
    # the forward at D = 256 is one launch: no workspace, but the query accepts the size (a refused descriptor also answers 0,
    # so the dispatcher's route is what pins it: above)
    assert lib.aule_attention_forward_workspace_size(ctypes.byref(_desc(_capi.AttnDesc, 2, 8, 32, 8, 1, 8192, 256))) == 0


def _resource_usage(src, tmp_path):
    out = tmp_path / (os.path.basename(src) + ".o")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(out), src],
                       capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur is not None:
            res[cur][m.group(1)] = int(m.group(2))
    return res


@pytest.mark.parametrize("src,kernels", [("fa_fwd_d256_gfx950.hip", 3), ("fa_bwd_d256_gfx950.hip", 9)])
def test_d256_kernels_neither_spill_nor_use_scratch(tmp_path, src, kernels):
    res = _resource_usage(os.path.join(CSRC, src), tmp_path)
    names = [n for n in res if "d256" in n]
    assert len(names) == kernels, names   # bf16, fp16 and fp32 of every kernel
    for n in names:
        r = res[n]
        assert r.get("ScratchSize") == 0, (n, r)
        assert r.get("VGPRs Spill") == 0, (n, r)
        assert r.get("SGPRs Spill") == 0, (n, r)
