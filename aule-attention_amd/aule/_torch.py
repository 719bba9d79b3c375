"""PyTorch-ROCm binding of the gfx950 kernels (zero-copy, current stream, autograd).

Counterpart of the reference's FlashAttentionAMDFunc (python/aule/triton_flash_amd.py:
392-500) and flash_attention_amd (:503-536): same autograd contract -- forward saves
(q, k, v, out, lse), backward returns (dq, dk, dv) in the input dtype -- but the launches
go to libaule.so's aule_attention_forward_ex / aule_attention_backward_ex with
tensor.data_ptr() and the current HIP stream.  torch is plumbing here (device memory,
streams, autograd graph); the arithmetic is in aule-attention_amd/csrc/*.hip.
"""
import ctypes
import math
import os
import threading

import torch

from . import _capi

_DTYPES = {torch.float32: _capi.DTYPE_F32, torch.float16: _capi.DTYPE_F16, torch.bfloat16: _capi.DTYPE_BF16}
SUPPORTED_HEAD_DIMS = (32, 64, 128, 256)
PAGED_HEAD_DIMS = (32, 64, 128)   # paged decode has no D = 256 instance


_ALWAYS_AUTOGRAD = os.environ.get("AULE_HIP_ALWAYS_AUTOGRAD", "0") == "1"


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def causal_code(causal):
    """The C-ABI's AULE_CAUSAL_* code for the Python-level `causal` argument: False/None -> 0,
    True or "top-left" -> 1 (the reference's rule), "bottom-right" or 2 -> 2."""
    if isinstance(causal, str):
        try:
            return {"none": 0, "top-left": 1, "bottom-right": 2}[causal]
        except KeyError:
            raise ValueError(f"causal must be a bool, 'top-left' or 'bottom-right', got {causal!r}") from None
    if causal is None or causal is False:
        return 0
    if causal is True:
        return 1
    c = int(causal)
    if c not in (0, 1, 2):
        raise ValueError(f"causal code must be 0, 1 or 2, got {causal!r}")
    return c


def _abi_scale(scale):
    """The `_ex` descriptors read scale == 0 as "default 1/sqrt(D)" (a zero-initialised struct must work); this layer always
    resolves the default itself, so an explicit 0.0 -- uniform attention in the reference and in the oracle -- is passed
    as the smallest value the kernels treat the same way (they clamp |scale * log2 e| to 1e-30 anyway)."""
    scale = float(scale)
    return scale if scale != 0.0 else 1e-30


def _window_arg(window):
    """The descriptors' window_size: the window when it is one (> 0), else -1 (full attention)."""
    return int(window) if window is not None and window > 0 else -1


def _device_index(device):
    """The HIP ordinal of a torch device; an index-less "cuda" device means the current one at the time of the call."""
    return device.index if device.index is not None else torch.cuda.current_device()


def _attn_problem(d, q, k, causal, scale, window):
    """The problem statement AttnDesc and AttnBwdDesc share, from q [B,Hq,Sq,D] and k [B,Hkv,Sk,D]; returns d."""
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = q.shape[0], q.shape[1], k.shape[1], q.shape[2], k.shape[2], q.shape[3]
    d.scale = scale
    d.causal = causal_code(causal)
    d.window_size = _window_arg(window)
    return d


def _same_device(what, ref, *tensors):
    for t in tensors:
        if t.device != ref.device:
            raise ValueError(f"{what}: every tensor must live on {ref.device}, got one on {t.device}")


def _workspace(nbytes, device):
    """Partials of the two-launch short-query paths from torch's caching allocator: stream-ordered like the library's own
    hipMallocAsync fallback, but graph-aware -- under torch.cuda.graph capture it adds no alloc / free nodes (which cost
    more than the kernels of a decode step).  Freed by reference count after the launch; the allocator keeps the block
    on the launch stream's free list, so reuse is ordered behind the kernels that read it."""
    nbytes = int(nbytes)
    return torch.empty((nbytes,), device=device, dtype=torch.uint8) if nbytes > 0 else None


def _attn_rope(cos, sin, q_pos):
    r = _capi.AttnRope()
    r.struct_size = ctypes.sizeof(_capi.AttnRope)
    r.layout = _capi.ROPE_HALF
    r.table_len, r.table_pitch, r.q_pos_offset = cos.shape[0], cos.stride(0), int(q_pos)
    r.cos, r.sin = cos.data_ptr(), sin.data_ptr()
    return r


def fwd_raw(q, k, v, causal, scale, want_lse=True, window=-1, q_rope=None, out=None):
    """q [B,Hq,Sq,D], k/v [B,Hkv,Sk,D]: contiguous device tensors, D in SUPPORTED_HEAD_DIMS.
    Returns (out, lse or None).  Asynchronous on the current stream.
    out: write the result there (contiguous, q's shape / dtype / device) instead of a fresh tensor -- aule.dist computes its
    pieces straight into their place in the gathered tensor.
    q_rope = (cos, sin, q_pos): rotate Q inside the kernel (half-split pairs; K already rotated) -- only for shapes
    rope_fusable() accepts, AuleError otherwise."""
    lib = _capi.get_lib()
    _same_device("flash attention forward", q, k, v)
    B, Hq, Sq, D = q.shape
    if out is None:
        out = torch.empty_like(q)
    elif out.shape != q.shape or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous tensor of the query's shape, dtype and device")
    lse = torch.empty((B, Hq, Sq), device=q.device, dtype=torch.float32) if want_lse else None
    if q.numel() == 0:
        return out, lse
    d, ws_bytes = _fwd_desc(lib, q, k, causal, scale, window)
    d.stream = torch.cuda.current_stream(q.device).cuda_stream
    d.q, d.k, d.v, d.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    if ws_bytes:
        ws = torch.empty((ws_bytes,), device=q.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws_bytes
    if q_rope is not None:
        r = _attn_rope(*q_rope)
        _capi.check(lib.aule_attention_forward_rope_ex(ctypes.byref(d), ctypes.byref(r)), "aule_attention_forward_rope_ex")
    else:
        rc = lib.aule_attention_forward_ex(ctypes.byref(d))
        if rc != 0:
            _capi.check(rc, "aule_attention_forward_ex")
    return out, lse


# Per-call host cost (tools/host_overhead.py): the descriptor of a (dtype, shape, flags, device) combination is built
# once -- struct fill, flag decoding, the workspace-size query -- and kept; a call then sets the stream, four or five pointers and the
# workspace.  Per thread (a descriptor is mutated by the call that uses it).  Decode loops that need less than this layer can give
# (~15 us of Python + ctypes + two tensor allocations per call) capture the step in a hipGraph: INTEGRATION.md, tests/test_gpu_graph.py.
_desc_cache = threading.local()


def _fwd_desc(lib, q, k, causal, scale, window):
    cache = getattr(_desc_cache, "fwd", None)
    if cache is None:
        cache = _desc_cache.fwd = {}
    # (the key holds VALUES -- a 0-dim tensor or numpy scalar as `scale` / `window` hashes by identity, never hits and stays alive in
    # the cache -- and the RESOLVED device: an index-less "cuda" device means the current one at the time of the call)
    dev = _device_index(q.device)
    key = (q.dtype, tuple(q.shape), int(k.shape[1]), int(k.shape[2]), causal_code(causal), None if scale is None else float(scale),
           _window_arg(window), dev)
    ent = cache.get(key)
    if ent is None:
        d = _attn_problem(_capi.AttnDesc(), q, k, causal, _abi_scale(scale), window)
        d.device = dev
        if len(cache) >= 512:
            cache.clear()
        ent = cache[key] = (d, int(lib.aule_attention_forward_workspace_size(ctypes.byref(d))))
    return ent


def rope_fusable(q, k, causal, window, cos, sin, q_pos, scale=None):
    """Would the forward kernel rotate Q itself for this problem (aule_attention_forward_rope_fusable)?  Host logic only:
    no device, no aule_init().  scale: the softmax scale of the call (None = default); its sign is part of the problem the library
    plans (negative scales and causal windows of at least two key tiles are rotated in the kernel too since round 6), so the
    question is asked about the descriptor the launch will see."""
    lib = _capi.load()
    if q.dtype not in _DTYPES or q.numel() == 0 or cos.stride(-1) != 1:
        return False
    d = _attn_problem(_capi.AttnDesc(), q, k, causal, 0.0 if scale is None else _abi_scale(scale), window)
    r = _attn_rope(cos, sin, q_pos)
    return lib.aule_attention_forward_rope_fusable(ctypes.byref(d), ctypes.byref(r)) == 1


def bwd_raw(q, k, v, out, dout, lse, causal, scale, window=-1):
    lib = _capi.get_lib()
    _same_device("flash attention backward", q, k, v, out, dout, lse)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if q.numel() == 0 or k.numel() == 0:
        return dq.zero_(), dk.zero_(), dv.zero_()
    d = _attn_problem(_capi.AttnBwdDesc(), q, k, causal, _abi_scale(scale), window)
    d.device = _device_index(q.device)
    d.stream = _stream_ptr(q.device)
    d.q, d.k, d.v, d.out, d.dout, d.lse = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(),
                                            dout.data_ptr(), lse.data_ptr())
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    # delta [B,Hq,Sq] fp32 (+ fp32 dK/dV partials when the GQA head loop is split over workgroups)
    nbytes = int(lib.aule_attention_backward_workspace_size(ctypes.byref(d)))
    ws = torch.empty((nbytes,), device=q.device, dtype=torch.uint8)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    _capi.check(lib.aule_attention_backward_ex(ctypes.byref(d)), "aule_attention_backward_ex")
    return dq, dk, dv


class FlashAttentionHipFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, window=-1):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out, lse = fwd_raw(q, k, v, causal, scale, want_lse=True, window=window)
        ctx.save_for_backward(q, k, v, out, lse)      # triton_flash_amd.py:436
        ctx.causal, ctx.scale, ctx.window = causal, scale, window
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dout = dout.contiguous().to(q.dtype)
        # (the reference's backward drops the window, triton_flash_amd.py:447-500; here it is the true gradient)
        dq, dk, dv = bwd_raw(q, k, v, out, dout, lse, ctx.causal, ctx.scale, window=ctx.window)
        return dq, dk, dv, None, None, None


def _pad_head_dim(x, Dp):
    D = x.shape[-1]
    return x if D == Dp else torch.nn.functional.pad(x, (0, Dp - D))


def flash_attention_hip(q, k, v, causal=True, scale=None, window=-1):
    """Device tensors in, device tensor out, autograd-aware.  dtype fp16/bf16/fp32 run
    natively; anything else is computed in fp32 and cast back."""
    D = q.shape[-1]
    if D > 256:
        raise ValueError(f"head_dim must be <= 256 for the HIP backend, got {D}")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    orig_dtype = q.dtype
    if orig_dtype not in _DTYPES:
        q, k, v = q.float(), k.float(), v.float()
    if k.dtype != q.dtype or v.dtype != q.dtype:
        k, v = k.to(q.dtype), v.to(q.dtype)
    Dp = next(x for x in SUPPORTED_HEAD_DIMS if x >= D)
    if Dp != D:   # zero-padded head dim: dot products and outputs are unchanged
        q, k, v = _pad_head_dim(q, Dp), _pad_head_dim(k, Dp), _pad_head_dim(v, Dp)
    code = causal_code(causal)
    if code == 2 and k.shape[2] < q.shape[2]:
        raise ValueError(f"bottom-right causal alignment needs seq_len_k >= seq_len_q, got {k.shape[2]} < {q.shape[2]}")
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        out = FlashAttentionHipFunc.apply(q, k, v, code, float(scale), int(window))
    else:
        # inference: no autograd node (its apply() costs more CPU time than a decode kernel runs) and no LSE,
        # which only the backward reads.  AULE_HIP_ALWAYS_AUTOGRAD=1 restores the old route (A/B measurements).
        if _ALWAYS_AUTOGRAD:
            out = FlashAttentionHipFunc.apply(q, k, v, code, float(scale), int(window))
        else:
            out, _ = fwd_raw(q.contiguous(), k.contiguous(), v.contiguous(), code, float(scale), want_lse=False,
                             window=int(window))
    if Dp != D:
        out = out[..., :D]
    return out if out.dtype == orig_dtype else out.to(orig_dtype)


_ROPE_LAYOUTS = {"half": _capi.ROPE_HALF, "interleaved": _capi.ROPE_INTERLEAVED}


def _rope_tables(cos, sin, D, device):
    """cos / sin as contiguous fp32 [table_len, D/2] on `device` (the reference takes [S, D/2] or [1, S, D/2]:
    triton_flash.py:414-424)."""
    if cos is None or sin is None:
        raise ValueError("cos and sin are required for RoPE")
    if cos.shape[-1] != D // 2 or sin.shape[-1] != D // 2:
        raise ValueError(f"cos/sin must have shape [..., {D // 2}], got {tuple(cos.shape)} / {tuple(sin.shape)}")
    cos = cos.to(device=device, dtype=torch.float32).reshape(-1, D // 2).contiguous()
    sin = sin.to(device=device, dtype=torch.float32).reshape(-1, D // 2).contiguous()
    if cos.shape != sin.shape:
        raise ValueError("cos and sin must have the same shape")
    return cos, sin


def rope_raw(x, cos, sin, layout="half", inverse=False, pos_offset=0, out=None):
    """Rotary embedding pass on the HIP backend (csrc/rope_gfx950.hip): x [B,H,S,D] contiguous device tensor
    (fp32/fp16/bf16), cos/sin fp32 [table_len, D/2]; row s uses table row s + pos_offset.  `out` may be x."""
    lib = _capi.get_lib()
    B, H, S, D = x.shape
    if D % 2:
        raise ValueError(f"RoPE needs an even head_dim, got {D}")
    if out is None:
        out = torch.empty_like(x)
    if x.numel() == 0:
        return out
    if S + pos_offset > cos.shape[0]:
        raise ValueError(f"RoPE table has {cos.shape[0]} rows, sequence needs {S + pos_offset}")
    d = _capi.RopeDesc()
    d.struct_size = ctypes.sizeof(_capi.RopeDesc)
    d.dtype = _DTYPES[x.dtype]
    d.rows_bh, d.seq, d.head_dim, d.row_pitch = B * H, S, D, D
    d.table_len, d.table_pitch = cos.shape[0], 0
    d.layout, d.inverse, d.pos_offset = _ROPE_LAYOUTS[layout], 1 if inverse else 0, int(pos_offset)
    d.device = _device_index(x.device)
    d.stream = _stream_ptr(x.device)
    d.in_, d.out, d.cos, d.sin = x.data_ptr(), out.data_ptr(), cos.data_ptr(), sin.data_ptr()
    _capi.check(lib.aule_rope_ex(ctypes.byref(d)), "aule_rope_ex")
    return out


class FlashAttentionRopeHipFunc(torch.autograd.Function):
    """RoPE pass on Q and K, then the attention kernels on the rotated tensors.  The backward rotates dQ', dK' back
    (the rotation is orthogonal: its transpose is the rotation by the opposite angle) -- the reference's backward
    ignores the rotation altogether (triton_flash.py:479-526 differentiates the un-rotated q, k)."""

    @staticmethod
    def forward(ctx, q, k, v, cos, sin, causal, scale, window, layout, q_pos, Dp):
        qr = rope_raw(q.contiguous(), cos, sin, layout, False, q_pos)
        kr = rope_raw(k.contiguous(), cos, sin, layout, False, 0)
        D = q.shape[-1]
        if Dp != D:
            qr, kr, v = _pad_head_dim(qr, Dp), _pad_head_dim(kr, Dp), _pad_head_dim(v, Dp)
        v = v.contiguous()
        out, lse = fwd_raw(qr, kr, v, causal, scale, want_lse=True, window=window)
        ctx.save_for_backward(qr, kr, v, out, lse, cos, sin)
        ctx.args = (causal, scale, window, layout, q_pos, D)
        return out[..., :D] if Dp != D else out

    @staticmethod
    def backward(ctx, dout):
        qr, kr, v, out, lse, cos, sin = ctx.saved_tensors
        causal, scale, window, layout, q_pos, D = ctx.args
        Dp = qr.shape[-1]
        dout = dout.to(qr.dtype)
        dout = _pad_head_dim(dout, Dp).contiguous() if Dp != D else dout.contiguous()
        dq, dk, dv = bwd_raw(qr, kr, v, out, dout, lse, causal, scale, window=window)
        if Dp != D:
            dq, dk, dv = dq[..., :D].contiguous(), dk[..., :D].contiguous(), dv[..., :D]
        rope_raw(dq, cos, sin, layout, True, q_pos, out=dq)
        rope_raw(dk, cos, sin, layout, True, 0, out=dk)
        return dq, dk, dv, None, None, None, None, None, None, None, None


def flash_attention_rope_hip(q, k, v, cos, sin, causal=True, scale=None, window=-1, layout="half"):
    """RoPE + attention on device tensors, autograd-aware.  Query i uses table row i (row i + Sk - Sq with
    causal="bottom-right"), key j row j -- the positions of the reference's kernel (triton_flash.py:119, :169)."""
    D = q.shape[-1]
    if D > 256:
        raise ValueError(f"head_dim must be <= 256 for the HIP backend, got {D}")
    if D % 2:
        raise ValueError(f"RoPE needs an even head_dim, got {D}")
    if layout not in _ROPE_LAYOUTS:
        raise ValueError(f"layout must be 'half' or 'interleaved', got {layout!r}")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    orig_dtype = q.dtype
    if orig_dtype not in _DTYPES:
        q, k, v = q.float(), k.float(), v.float()
    if k.dtype != q.dtype or v.dtype != q.dtype:
        k, v = k.to(q.dtype), v.to(q.dtype)
    cos, sin = _rope_tables(cos, sin, D, q.device)
    code = causal_code(causal)
    Sq, Sk = q.shape[2], k.shape[2]
    if code == 2 and Sk < Sq:
        raise ValueError(f"bottom-right causal alignment needs seq_len_k >= seq_len_q, got {Sk} < {Sq}")
    q_pos = Sk - Sq if code == 2 else 0
    if max(Sq + q_pos, Sk) > cos.shape[0]:
        raise ValueError(f"RoPE table has {cos.shape[0]} rows, sequences need {max(Sq + q_pos, Sk)}")
    Dp = next(x for x in SUPPORTED_HEAD_DIMS if x >= D)
    needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
    if (not needs_grad and layout == "half" and Dp == D and os.environ.get("AULE_HIP_ROPE_FUSE", "1") != "0"
            and rope_fusable(q, k, code, window, cos, sin, q_pos, float(scale))):
        # inference: K is rotated once per key, Q on its way into the attention kernel's registers (one read and one
        # write of Q less; bit-identical to the two-pass form -- DESIGN.md 3.6).  The backward needs the rotated Q in
        # memory, so training keeps the separate pass.
        kr = rope_raw(k.contiguous(), cos, sin, layout, False, 0)
        out, _ = fwd_raw(q.contiguous(), kr, v.contiguous(), code, float(scale), want_lse=False, window=window,
                         q_rope=(cos, sin, q_pos))
        return out if out.dtype == orig_dtype else out.to(orig_dtype)
    out = FlashAttentionRopeHipFunc.apply(q, k, v, cos, sin, code, float(scale), int(window), layout, q_pos, Dp)
    return out if out.dtype == orig_dtype else out.to(orig_dtype)


FP8_MAX = 448.0   # largest finite OCP e4m3fn value


def quantize_kv_cache_fp8(cache, per_head=True):
    """Quantise a [num_blocks, block_size, heads_kv, head_dim] cache to OCP FP8 e4m3fn for the FP8 paged decode:
    returns (cache_fp8, scale) with scale [heads_kv] fp32 on the cache's device and cache ~= scale[hk] * cache_fp8.

    scale = amax / 448 per KV head (per_head=False: one value from the whole cache, repeated; 1.0 where everything is
    zero).  Values are divided by the scale and clamped to +-448 BEFORE the cast: torch's cast to float8_e4m3fn does not
    saturate (465.0 becomes NaN).  Plain torch ops, no kernel; works on CPU tensors."""
    if cache.dim() != 4:
        raise ValueError("expected a cache of shape [num_blocks, block_size, heads_kv, head_dim]")
    x = cache.float()
    Hkv = x.shape[2]
    if per_head:
        amax = x.abs().amax(dim=(0, 1, 3)) if x.numel() else x.new_zeros(Hkv)
    else:
        amax = (x.abs().amax() if x.numel() else x.new_zeros(())).expand(Hkv)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax)).contiguous()
    y = (x / scale.view(1, 1, Hkv, 1)).clamp_(-FP8_MAX, FP8_MAX)
    return y.to(torch.float8_e4m3fn), scale


def _scale_shape(s, Hkv, name):
    """The shape rule of k_scale / v_scale: None, a float, a 0-d or [1] tensor (one value for every head) or a [heads_kv] tensor.
    Returns whether a tensor `s` holds one value."""
    if not torch.is_tensor(s):
        return False
    one = s.dim() == 0 or s.shape == (1,)
    if not one and s.shape != (Hkv,):
        raise ValueError(f"{name} must be a float, a 0-d tensor or a [heads_kv] = [{Hkv}] tensor, got shape {tuple(s.shape)}")
    return one


def _fp8_scale(s, Hkv, device, name):
    """None / float / 0-d tensor / [heads_kv] tensor -> [heads_kv] fp32 on `device`, without a device->host copy."""
    if s is None:
        s = 1.0
    if not torch.is_tensor(s):
        return torch.full((Hkv,), float(s), dtype=torch.float32, device=device)
    if _scale_shape(s, Hkv, name):
        return s.to(device=device, dtype=torch.float32).reshape(1).expand(Hkv).contiguous()
    return s.to(device=device, dtype=torch.float32).contiguous()


def _paged_cache_is_fp8(op, inputs, k_cache, v_cache, k_scale, v_scale):
    """The cache-kind rules the paged operations share -- caches of one dtype, torch.float8_e4m3fn the only FP8 encoding,
    fp16 / bf16 inputs (and 16-bit caches) of one dtype, scales with FP8 caches only, head_dim in PAGED_HEAD_DIMS -- as ValueErrors
    in that operation's words.  op: "decode", "query", "prefill", "cascade" (inputs: (q,)) or "append" (inputs: (key, value)).
    Returns whether the caches are FP8."""
    if op == "append":
        name, fp8_use, same, with_fp8, dims_of = ("paged KV append", "the paged KV append writes", "key, value and caches",
                                                  "fp16 / bf16 key and value", "the paged KV cache")
    else:
        name, fp8_use, same, with_fp8 = f"paged {op}", f"the FP8 paged {op} takes", "query and caches", "an fp16 / bf16 query"
        dims_of = name if op == "decode" else "the " + name
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"k_cache ({k_cache.dtype}) and v_cache ({v_cache.dtype}) must have the same dtype")
    other_fp8 = tuple(t for t in (getattr(torch, n, None) for n in ("float8_e4m3fnuz", "float8_e5m2", "float8_e5m2fnuz"))
                      if t is not None)
    if k_cache.dtype in other_fp8:
        raise ValueError(f"{k_cache.dtype} caches are not supported: {fp8_use} torch.float8_e4m3fn only "
                         "(gfx950 converts OCP e4m3fn in hardware; e4m3fnuz is MI300X's encoding, e5m2 is not built)")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    dtype = inputs[0].dtype
    if dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != dtype for t in inputs[1:]) or (not fp8 and k_cache.dtype != dtype):
        raise ValueError(f"{name} runs in fp16 or bf16 ({same} in the same dtype, or float8_e4m3fn caches with {with_fp8})")
    if not fp8 and (k_scale is not None or v_scale is not None):
        raise ValueError("k_scale / v_scale apply to float8_e4m3fn caches only; a 16-bit cache holds the values themselves")
    D = inputs[0].shape[-1]
    if D not in PAGED_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {PAGED_HEAD_DIMS} for {dims_of}, got {D}")
    return fp8


# What the four paged attention calls have in common, one step each; a call is its steps in its own order (the order of the checks is
# part of what tests/golden/paged_contract.json records).  op: "decode", "query", "prefill" or "cascade".

def _paged_shapes(q, axes, k_cache, v_cache):
    """q [`axes`: heads second, head_dim last] against k_cache / v_cache [num_blocks, block_size, Hkv, D]; returns Hkv."""
    if q.dim() != axes.count(",") + 1 or k_cache.dim() != 4 or v_cache.shape != k_cache.shape:
        raise ValueError(f"expected q [{axes}] and k_cache/v_cache [num_blocks, block_size, Hkv, D]")
    Hq, D = q.shape[1], q.shape[-1]
    Hkv, Dk = k_cache.shape[2:]
    if Dk != D:
        raise ValueError(f"head_dim mismatch: query={D}, cache={Dk}")
    if Hkv == 0 or Hq % Hkv != 0:
        raise ValueError(f"heads_q ({Hq}) must be divisible by heads_kv ({Hkv})")
    return Hkv


def _paged_cache_kind(op, q, k_cache, v_cache, k_scale, v_scale):
    """_paged_cache_is_fp8, then a positive block size (the decode leaves that one to the library)."""
    fp8 = _paged_cache_is_fp8(op, (q,), k_cache, v_cache, k_scale, v_scale)
    if k_cache.shape[1] == 0:
        raise ValueError("block_size must be positive")
    return fp8


def _paged_tables(block_tables, context_lens, B=None):
    """block_tables [batch, max_blocks >= 1] and context_lens [batch], wherever the caller has them; the batch is B where q states
    one, else the tables' own.  Returns it."""
    if not (block_tables.dim() == 2 and block_tables.shape[1] > 0 and B in (None, block_tables.shape[0])
            and context_lens.shape == (block_tables.shape[0],)):
        raise ValueError("block_tables must be [batch, max_blocks] and context_lens [batch]")
    return block_tables.shape[0]


def _scale_shapes(fp8, Hkv, k_scale, v_scale):
    if fp8:
        _scale_shape(k_scale, Hkv, "k_scale")
        _scale_shape(v_scale, Hkv, "v_scale")


def _needs_device(op, q):
    if not q.is_cuda:
        raise _capi.AuleError(f"aule (HIP build): the paged {op} needs ROCm device tensors; there is no CPU fallback")


def _int32_on(device, *tensors):
    """Tables and lengths are read by the kernels: a CPU (or other-GPU) tensor would hand them a foreign pointer."""
    return [t.to(device=device, dtype=torch.int32).contiguous() for t in tensors]


def _paged_problem(d, q, k_cache, v_cache, out, bt, cl, scale, fp8=None):
    """The fields every paged descriptor has, from tensors on one device: heads and head_dim are q's second and last extent, the batch
    the tables' first.  fp8: the cache kind, for the kinds that state it in a field.  Returns d."""
    D = q.shape[-1]
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    if fp8 is not None:
        d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.batch, d.heads_q, d.heads_kv, d.head_dim = bt.shape[0], q.shape[1], k_cache.shape[2], D
    d.block_size, d.max_blocks = k_cache.shape[1], bt.shape[1]
    d.scale = _abi_scale(1.0 / math.sqrt(D) if scale is None else scale)
    d.device = _device_index(q.device)
    d.stream = _stream_ptr(q.device)
    d.q, d.k_cache, d.v_cache, d.out = q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr()
    d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
    return d


def _attach_workspace(d, size_query, device):
    """The workspace the library asks for `d`, attached; the caller holds what this returns until the launch is queued."""
    ws = _workspace(size_query(ctypes.byref(d)), device)
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    return ws


def _attach_scales(d, fp8, k_scale, v_scale, Hkv, device):
    """The [heads_kv] scale arrays of an FP8 cache, attached; the caller holds what this returns until the launch is queued."""
    if not fp8:
        return None
    ks, vs = _fp8_scale(k_scale, Hkv, device, "k_scale"), _fp8_scale(v_scale, Hkv, device, "v_scale")
    d.k_scale, d.v_scale = ks.data_ptr(), vs.data_ptr()
    return ks, vs


def _sinks_check(sinks, q):
    """The rules of the sink logits (attention sinks: aule.flash_attention_varlen_sinks documents them), none of which needs a device:
    a [heads_q] tensor on q's device, fp32 or of q's dtype."""
    Hq = q.shape[1]
    if not torch.is_tensor(sinks) or sinks.shape != (Hq,):
        raise ValueError(f"sinks must be a [heads_q] = [{Hq}] tensor, got "
                         f"{tuple(sinks.shape) if torch.is_tensor(sinks) else type(sinks).__name__}")
    if sinks.dtype not in (torch.float32, q.dtype):
        raise ValueError(f"sinks must be float32 or of q's dtype ({q.dtype}), got {sinks.dtype}")
    if sinks.device != q.device:
        raise ValueError(f"sinks must be on q's device ({q.device}), got {sinks.device}: the kernels read it on every launch")


def _sinks_f32(sinks):
    """The logits as the kernels read them: fp32, contiguous (a differentiable conversion: the gradient comes back in sinks' dtype)."""
    if sinks.dtype == torch.float32 and sinks.is_contiguous():
        return sinks
    return sinks.float().contiguous()


def _tree_mask_check(tree_mask, shape, what, q):
    """The rules of the tree words (tree masks: aule.flash_attention_paged_query_tree documents them), none of which needs a device: an
    int64 tensor of `shape`, contiguous (the kernels read it in place on every launch) and on q's device."""
    if not torch.is_tensor(tree_mask) or tuple(tree_mask.shape) != tuple(shape):
        raise ValueError(f"tree_mask must be a {what} = {list(shape)} tensor, got "
                         f"{tuple(tree_mask.shape) if torch.is_tensor(tree_mask) else type(tree_mask).__name__}")
    if tree_mask.dtype != torch.int64:
        raise ValueError(f"tree_mask must be int64 (one 64-bit word per new token, read on the device as it stands), got {tree_mask.dtype}")
    if not tree_mask.is_contiguous():
        raise ValueError("tree_mask must be contiguous: the kernels read it in place on every launch (pass tree_mask.contiguous())")
    if tree_mask.device != q.device:
        raise ValueError(f"tree_mask must be on q's device ({q.device}), got {tree_mask.device}: the kernels read it on every launch")


def _no_tree_extras(window_size, sinks):
    if _window_arg(window_size) > 0:
        raise ValueError("a sliding window is not defined over a tree (window_size must be off with tree_mask)")
    if sinks is not None:
        raise ValueError("sink logits together with a tree are not built")


def tree_mask_from_parents(parents):
    """aule.tree_mask_from_parents (documented there).  Torch ops only, on parents' device, no host synchronisation: the ancestor relation is
    closed by repeated squaring of the boolean matrix (ceil(log2(seq_q)) products), and each word is assembled from its two 32-bit halves,
    so that bit 63 never passes through a signed shift or a signed sum that overflows."""
    if not torch.is_tensor(parents) or parents.dim() not in (1, 2) or parents.dtype.is_floating_point or parents.dtype.is_complex \
            or parents.dtype == torch.bool:
        raise ValueError("parents must be an integer tensor [seq_q] or [batch, seq_q]")
    n = parents.shape[-1]
    if n > PAGED_QUERY_MAX_TOKENS:
        raise ValueError(f"a tree holds at most {PAGED_QUERY_MAX_TOKENS} new tokens per sequence, got {n}")
    p = parents.to(torch.int64)
    idx = torch.arange(n, device=p.device)
    ok = (p >= 0) & (p < idx)                                   # anything else: a child of the context
    # reach[.., i, j]: j is i itself or an ancestor of i
    reach = (idx.unsqueeze(-1) == idx) | ((p.unsqueeze(-1) == idx) & ok.unsqueeze(-1))
    steps = 1
    while steps < n:
        r = reach.to(torch.float32)
        reach = (r @ r) > 0
        steps *= 2
    w = torch.where(idx < 32, torch.ones_like(idx) << (idx % 32), torch.zeros_like(idx))      # bit j as a value < 2^32, j < 32
    lo = (reach.to(torch.int64) * w).sum(-1)
    hi = (reach.to(torch.int64) * torch.where(idx >= 32, torch.ones_like(idx) << (idx % 32), torch.zeros_like(idx))).sum(-1)
    hi = torch.where(hi >= (1 << 31), hi - (1 << 32), hi)       # the high half as a signed 32-bit value: the product below stays in range
    return (hi * (1 << 32)) | lo


def paged_decode(q, k_cache, v_cache, block_tables, context_lens, scale=None, window_size=-1, k_scale=None, v_scale=None):
    """Paged-KV decode on the HIP backend; counterpart of flash_attention_paged_amd
    (python/aule/triton_flash_amd.py:656-737), same argument meaning:

        q            [batch, heads_q, head_dim] (or [batch, heads_q, 1, head_dim]) fp16 / bf16
        k_cache      [num_blocks, block_size, heads_kv, head_dim]     v_cache: same
        block_tables [batch, max_blocks_per_seq] integer, context_lens [batch] integer
    Returns [batch, heads_q, head_dim].  No device->host synchronisation (the reference reads
    context_lens.max() on the host).

    The caches are either of the query's dtype or both torch.float8_e4m3fn (OCP FP8, the format gfx950 converts in
    hardware).  Then K = k_scale[hk] * float(k_cache) and V = v_scale[hk] * float(v_cache), with k_scale / v_scale each
    None (1.0), a float, a 0-d tensor or a [heads_kv] tensor; they reach the kernel as device arrays.  All argument
    errors are ValueErrors raised before the device is touched."""
    if q.dim() == 4:
        if q.shape[2] != 1:
            raise ValueError("PagedAttention only supports single query token")
        q = q.squeeze(2)
    Hkv = _paged_shapes(q, "B,Hq,D", k_cache, v_cache)
    B, Hq, _ = q.shape
    fp8 = _paged_cache_is_fp8("decode", (q,), k_cache, v_cache, k_scale, v_scale)
    d = _capi.PagedFp8Desc() if fp8 else _capi.PagedDesc()
    held = [_attach_scales(d, fp8, k_scale, v_scale, Hkv, q.device)]   # (what the launch reads, held until it is queued)
    lib = _capi.get_lib()
    q, k_cache, v_cache = q.contiguous(), k_cache.contiguous(), v_cache.contiguous()
    _same_device("paged decode", q, k_cache, v_cache)
    # (unlike its siblings the decode refuses no CPU tensor itself -- aule.flash_attention_paged_amd does -- and looks at the tables
    # after the move, without a rule about max_blocks or block_size: those are the library's here)
    bt, cl = _int32_on(q.device, block_tables, context_lens)
    if bt.dim() != 2 or bt.shape[0] != B or cl.shape != (B,):
        raise ValueError("block_tables must be [batch, max_blocks] and context_lens [batch]")
    out = torch.empty_like(q)
    if B * Hq == 0:
        return out
    _paged_problem(d, q, k_cache, v_cache, out, bt, cl, scale)
    d.window_size = _window_arg(window_size)
    size_query, launch = ("aule_attention_paged_decode_fp8_workspace_size", "aule_attention_paged_decode_fp8_ex") if fp8 else \
        ("aule_attention_paged_decode_workspace_size", "aule_attention_paged_decode_ex")
    held.append(_attach_workspace(d, getattr(lib, size_query), q.device))
    _capi.check(getattr(lib, launch)(ctypes.byref(d)), launch)
    return out


PAGED_QUERY_MAX_TOKENS = 64   # packed rows of the wave-per-chunk kernel family (csrc/fa_fwd_splitkv_gfx950.hip)


def paged_query(q, k_cache, v_cache, block_tables, context_lens, scale=None, window_size=-1, k_scale=None, v_scale=None,
                return_lse=False, sinks=None, tree_mask=None):
    """Paged attention for a short multi-token query per sequence (speculative verify, multi-token heads, a short prompt
    tail against a cached prefix); the MQ instances of csrc/fa_fwd_splitkv_gfx950.hip behind aule_attention_paged_query_ex:

        q            [batch, heads_q, seq_q, head_dim] fp16 / bf16, 1 <= seq_q <= 64
        k_cache, v_cache, block_tables, context_lens, k_scale, v_scale: as in paged_decode (16-bit or float8_e4m3fn caches)
    context_lens[b] counts the keys in the cache INCLUDING the seq_q new tokens (append them first: paged_kv_append).  Query
    i of sequence b sits at position p = L_b - seq_q + i (L_b: the length, clamped to what the block table addresses) and
    sees key j iff j <= p, and with window_size = W > 0 iff also p - j < W.  A query with p < 0 gives a row of zeros.
    Returns out [batch, heads_q, seq_q, head_dim], or (out, lse) with lse [batch, heads_q, seq_q] fp32 -- the natural log
    of the sum of exp(scaled score) over the visible keys, -inf for a row that sees none -- when return_lse is set.  No
    device->host synchronisation; captures into a graph.  All argument errors are ValueErrors raised before the device is
    touched.  sinks: [heads_q] sink logits (aule.flash_attention_paged_query_sinks), behind aule_attention_paged_query_sink_ex.
    tree_mask: [batch, seq_q] int64 words (aule.flash_attention_paged_query_tree), behind aule_attention_paged_query_tree_ex."""
    Hkv = _paged_shapes(q, "B,Hq,Sq,D", k_cache, v_cache)
    B, Hq, Sq, _ = q.shape
    if not 1 <= Sq <= PAGED_QUERY_MAX_TOKENS:
        raise ValueError(f"the paged query takes 1 to {PAGED_QUERY_MAX_TOKENS} query tokens per sequence, got {Sq} "
                         "(longer chunks and per-sequence lengths: flash_attention_paged_prefill)")
    fp8 = _paged_cache_kind("query", q, k_cache, v_cache, k_scale, v_scale)
    _paged_tables(block_tables, context_lens, B)
    _scale_shapes(fp8, Hkv, k_scale, v_scale)
    if sinks is not None:
        _sinks_check(sinks, q)
    if tree_mask is not None:
        _no_tree_extras(window_size, sinks)
        _tree_mask_check(tree_mask, (B, Sq), "[batch, seq_q]", q)
    _needs_device("query", q)
    lib = _capi.get_lib()
    q, k_cache, v_cache = q.contiguous(), k_cache.contiguous(), v_cache.contiguous()
    _same_device("paged query", q, k_cache, v_cache)
    bt, cl = _int32_on(q.device, block_tables, context_lens)
    out = torch.empty_like(q)
    lse = torch.empty((B, Hq, Sq), device=q.device, dtype=torch.float32) if return_lse else None
    if B * Hq == 0:
        return (out, lse) if return_lse else out
    kind = _capi.PagedQueryTreeDesc if tree_mask is not None else _capi.PagedQueryDesc if sinks is None else _capi.PagedQuerySinkDesc
    d = _paged_problem(kind(), q, k_cache, v_cache, out, bt, cl, scale, fp8)
    d.seq_q, d.window_size = Sq, _window_arg(window_size)
    d.lse = lse.data_ptr() if lse is not None else None
    size_query, launch = ("aule_attention_paged_query_workspace_size", "aule_attention_paged_query_ex") if sinks is None else \
        ("aule_attention_paged_query_sink_workspace_size", "aule_attention_paged_query_sink_ex")
    if tree_mask is not None:
        size_query, launch = "aule_attention_paged_query_tree_workspace_size", "aule_attention_paged_query_tree_ex"
        d.tree_mask = tree_mask.data_ptr()
    held = [_attach_workspace(d, getattr(lib, size_query), q.device),   # (until the launch is queued)
            _attach_scales(d, fp8, k_scale, v_scale, Hkv, q.device)]
    if sinks is not None:
        held.append(_sinks_f32(sinks))
        d.sinks = held[-1].data_ptr()
    _capi.check(getattr(lib, launch)(ctypes.byref(d)), launch)
    return (out, lse) if return_lse else out


# Variable-length packed batches: sequences of different lengths along one token axis, forward and backward
# (aule_attention_varlen_forward_ex / _backward_ex; csrc/fa_fwd_varlen_gfx950.hip, csrc/fa_bwd_varlen_gfx950.hip).

VARLEN_HEAD_DIMS = (32, 64, 128)


def _varlen_max(name, m):
    if m is not None and (isinstance(m, bool) or not isinstance(m, int) or m < 1):
        raise ValueError(f"{name} must be a positive int or None, got {m!r}")


def _varlen_check(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """Every rule of the arguments that needs no device.  Returns the batch."""
    if not (torch.is_tensor(q) and torch.is_tensor(k) and torch.is_tensor(v)) or q.dim() != 3 or k.dim() != 3 or v.shape != k.shape:
        raise ValueError("expected q [total_q, heads_q, head_dim] and k, v [total_k, heads_kv, head_dim] of one shape")
    (Hq, D), (Hkv, Dk) = q.shape[1:], k.shape[1:]
    if Dk != D:
        raise ValueError(f"head_dim mismatch: query={D}, key={Dk}")
    if Hkv == 0 or Hq % Hkv != 0:
        raise ValueError(f"heads_q ({Hq}) must be divisible by heads_kv ({Hkv})")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"variable-length attention is not built for {q.dtype}: fp16 and bf16 only")
    if k.dtype != q.dtype or v.dtype != q.dtype:
        raise ValueError(f"q, k and v must share one dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    if D == 0 or D > VARLEN_HEAD_DIMS[-1]:
        raise ValueError(f"variable-length attention is not built for head_dim {D}: 1 to {VARLEN_HEAD_DIMS[-1]}")
    return _varlen_offsets(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)


def _varlen_offsets(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k):
    """The rules of cu_seqlens_q / cu_seqlens_k [batch + 1] int32 and of the two maxima.  Returns the batch."""
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not torch.is_tensor(cu) or cu.dim() != 1 or cu.shape[0] < 1:
            raise ValueError(f"{name} must be a [batch + 1] tensor")
        if cu.dtype != torch.int32:
            raise ValueError(f"{name} must be int32 (it is read on the device as it stands), got {cu.dtype}")
    if cu_seqlens_k.shape != cu_seqlens_q.shape:
        raise ValueError(f"cu_seqlens_q {tuple(cu_seqlens_q.shape)} and cu_seqlens_k {tuple(cu_seqlens_k.shape)} must both be [batch + 1]")
    _varlen_max("max_seqlen_q", max_seqlen_q)
    _varlen_max("max_seqlen_k", max_seqlen_k)
    return cu_seqlens_q.shape[0] - 1


def _varlen_maxima(cu_q, cu_k, max_seqlen_q, max_seqlen_k):
    """The maxima the caller did not give, read from the offsets (on the device) with the one documented synchronisation: both in
    one read."""
    if max_seqlen_q is None or max_seqlen_k is None:
        if cu_q.shape[0] > 1:
            mq, mk = torch.stack(((cu_q[1:] - cu_q[:-1]).max(), (cu_k[1:] - cu_k[:-1]).max())).tolist()
        else:
            mq = mk = 1
        max_seqlen_q = max(int(mq), 1) if max_seqlen_q is None else max_seqlen_q
        max_seqlen_k = max(int(mk), 1) if max_seqlen_k is None else max_seqlen_k
    return max_seqlen_q, max_seqlen_k


def _varlen_rows(name, x):
    """x [T, H, D] as the kernels read it -- the heads of a token contiguous, the token stride free -- and that stride in elements."""
    T, H, D = x.shape
    if T > 1 and (x.stride(2) != 1 or x.stride(1) != D) or T <= 1 and not x.is_contiguous():
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else H * D
    if stride < H * D or stride % 8 != 0 or x.storage_offset() % 8 != 0:
        raise ValueError(f"{name}'s token stride ({stride}) and storage offset ({x.storage_offset()}) must be multiples of 8 elements "
                         f"and the stride at least heads * head_dim = {H * D} (16-byte loads); pass {name}.contiguous()")
    return x, stride


def _varlen_problem(d, q, k, v, sq, sk, sv, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window):
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.batch, d.heads_q, d.heads_kv, d.head_dim = cu_q.shape[0] - 1, q.shape[1], k.shape[1], q.shape[2]
    d.total_q, d.total_k = q.shape[0], k.shape[0]
    d.max_seqlen_q, d.max_seqlen_k = max(min(max_seqlen_q, q.shape[0]), 1), max(min(max_seqlen_k, k.shape[0]), 1)
    d.scale = _abi_scale(scale)
    d.causal = causal
    d.window_size = _window_arg(window)
    d.device = _device_index(q.device)
    d.q_token_stride, d.k_token_stride, d.v_token_stride = sq, sk, sv
    d.stream = _stream_ptr(q.device)
    d.q, d.k, d.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.cu_seqlens_q, d.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    return d


def varlen_fwd_raw(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window=-1, want_lse=True, sinks=None):
    """q [Tq,Hq,D], k / v [Tk,Hkv,D] device tensors (heads contiguous, D in VARLEN_HEAD_DIMS), cu_q / cu_k int32 [B + 1] on the same
    device, causal an AULE_CAUSAL_* code.  Returns (out, lse or None), both from torch.empty.  Asynchronous, no synchronisation.
    sinks: [Hq] fp32 contiguous sink logits on the same device (aule_attention_varlen_sink_forward_ex), or None."""
    lib = _capi.get_lib()
    _same_device("variable-length attention", q, k, v, cu_q, cu_k)
    (q, sq), (k, sk), (v, sv) = _varlen_rows("q", q), _varlen_rows("k", k), _varlen_rows("v", v)
    out = torch.empty(q.shape, device=q.device, dtype=q.dtype)
    lse = torch.empty(q.shape[:2], device=q.device, dtype=torch.float32) if want_lse else None
    if q.shape[0] * q.shape[1] * (cu_q.shape[0] - 1) == 0:
        return out, lse
    d = _varlen_problem(_capi.VarlenDesc() if sinks is None else _capi.VarlenSinkDesc(), q, k, v, sq, sk, sv, cu_q, cu_k, max_seqlen_q,
                        max_seqlen_k, causal, scale, window)
    d.out = out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    launch = "aule_attention_varlen_forward_ex"
    if sinks is not None:
        launch, d.sinks = "aule_attention_varlen_sink_forward_ex", sinks.data_ptr()
    _capi.check(getattr(lib, launch)(ctypes.byref(d)), launch)
    return out, lse


def varlen_bwd_raw(q, k, v, out, dout, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window=-1, sinks=None):
    """The gradients of varlen_fwd_raw: dq [Tq,Hq,D], dk, dv [Tk,Hkv,D], contiguous and ZERO in the rows no sequence owns (the
    library never writes those; they are allocated zero-filled here).  out, dout, lse contiguous.  Asynchronous, no synchronisation.
    sinks (the forward's): returns (dq, dk, dv, dsinks [Hq] fp32) through aule_attention_varlen_sink_backward_ex."""
    lib = _capi.get_lib()
    _same_device("variable-length attention backward", q, k, v, out, dout, lse, cu_q, cu_k)
    (q, sq), (k, sk), (v, sv) = _varlen_rows("q", q), _varlen_rows("k", k), _varlen_rows("v", v)
    dq = torch.zeros(q.shape, device=q.device, dtype=q.dtype)
    dk = torch.zeros(k.shape, device=k.device, dtype=k.dtype)
    dv = torch.zeros(v.shape, device=v.device, dtype=v.dtype)
    dsinks = None if sinks is None else torch.zeros(q.shape[1], device=q.device, dtype=torch.float32)
    grads = (dq, dk, dv) if sinks is None else (dq, dk, dv, dsinks)
    if q.shape[1] * (cu_q.shape[0] - 1) == 0 or q.shape[0] + k.shape[0] == 0:
        return grads
    d = _varlen_problem(_capi.VarlenBwdDesc() if sinks is None else _capi.VarlenSinkBwdDesc(), q, k, v, sq, sk, sv, cu_q, cu_k, max_seqlen_q,
                        max_seqlen_k, causal, scale, window)
    d.out, d.lse, d.dout = out.data_ptr(), lse.data_ptr(), dout.data_ptr()
    d.dq, d.dk, d.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    size_query, launch = "aule_attention_varlen_backward_workspace_size", "aule_attention_varlen_backward_ex"
    if sinks is not None:
        size_query, launch = "aule_attention_varlen_sink_backward_workspace_size", "aule_attention_varlen_sink_backward_ex"
        d.sinks, d.dsinks = sinks.data_ptr(), dsinks.data_ptr()
    ws = _attach_workspace(d, getattr(lib, size_query), q.device)   # delta [Tq, Hq] fp32 (and the dsinks partials); held until the launch is queued
    _capi.check(getattr(lib, launch)(ctypes.byref(d)), launch)
    del ws
    return grads


class FlashAttentionVarlenHipFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window):
        out, lse = varlen_fwd_raw(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window)
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k)
        ctx.problem = (max_seqlen_q, max_seqlen_k, causal, scale, window)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_seqlen_q, max_seqlen_k, causal, scale, window = ctx.problem
        dout = dout.contiguous().to(q.dtype)
        dq, dk, dv = varlen_bwd_raw(q, k, v, out, dout, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window)
        return dq, dk, dv, None, None, None, None, None, None, None


class FlashAttentionVarlenSinksHipFunc(torch.autograd.Function):
    """FlashAttentionVarlenHipFunc with sink logits ([Hq] fp32, contiguous): the saved lse includes the sink, so dq, dk and dv are the
    sinkless kernels' and dsinks is one reduction more."""

    @staticmethod
    def forward(ctx, q, k, v, sinks, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window):
        out, lse = varlen_fwd_raw(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window, sinks=sinks)
        ctx.save_for_backward(q, k, v, sinks, out, lse, cu_q, cu_k)
        ctx.problem = (max_seqlen_q, max_seqlen_k, causal, scale, window)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, sinks, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_seqlen_q, max_seqlen_k, causal, scale, window = ctx.problem
        dout = dout.contiguous().to(q.dtype)
        dq, dk, dv, dsinks = varlen_bwd_raw(q, k, v, out, dout, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, window, sinks=sinks)
        return dq, dk, dv, dsinks, None, None, None, None, None, None, None


def flash_attention_varlen_sinks(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True, scale=None,
                                 window_size=-1, return_lse=False):
    """flash_attention_varlen with per-head sink logits, autograd-aware over q, k, v and sinks (aule.flash_attention_varlen_sinks
    documents the arguments)."""
    return _varlen_attention(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window_size, return_lse, sinks)


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True, scale=None,
                           window_size=-1, return_lse=False):
    """Attention over a variable-length packed batch, autograd-aware (aule.flash_attention_varlen documents the arguments)."""
    return _varlen_attention(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window_size, return_lse)


_NO_SINKS = object()


def _varlen_attention(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, scale, window_size, return_lse, sinks=_NO_SINKS):
    """The two calls above: one set of checks, stride rules and head-dim padding; with sinks the sink entries behind them."""
    _varlen_check(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    if sinks is not _NO_SINKS:
        _sinks_check(sinks, q)
    code = causal_code(causal)
    D = q.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if D in VARLEN_HEAD_DIMS:   # (a padded copy is contiguous: only tensors read in place have strides to refuse)
        for name, x in (("q", q), ("k", k), ("v", v)):
            _varlen_rows(name, x)
    if not q.is_cuda:
        raise _capi.AuleError("aule (HIP build): variable-length attention needs ROCm device tensors; there is no CPU fallback")
    _same_device("variable-length attention", q, k, v)
    cu_q, cu_k = _int32_on(q.device, cu_seqlens_q, cu_seqlens_k)
    max_seqlen_q, max_seqlen_k = _varlen_maxima(cu_q, cu_k, max_seqlen_q, max_seqlen_k)
    Dp = next(x for x in VARLEN_HEAD_DIMS if x >= D)
    if Dp != D:   # zero-padded head dim: dot products and outputs are unchanged
        q, k, v = _pad_head_dim(q, Dp), _pad_head_dim(k, Dp), _pad_head_dim(v, Dp)
    window = _window_arg(window_size)
    sinks = None if sinks is _NO_SINKS else _sinks_f32(sinks)
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad or (sinks is not None and sinks.requires_grad)):
        if sinks is None:
            out, lse = FlashAttentionVarlenHipFunc.apply(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code, float(scale), window)
        else:
            out, lse = FlashAttentionVarlenSinksHipFunc.apply(q, k, v, sinks, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code, float(scale), window)
    else:
        out, lse = varlen_fwd_raw(q, k, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code, float(scale), window, want_lse=return_lse,
                                  sinks=None if sinks is None else sinks.detach())
    if Dp != D:
        out = out[..., :D]
    return (out, lse) if return_lse else out


# MLA prefill: the non-absorbed 192 / 128 form over a packed batch (aule_attention_mla_prefill_ex; csrc/fa_fwd_mla_prefill_gfx950.hip),
# and its differentiable twin flash_attention_mla_varlen (aule_attention_mla_prefill_backward_ex; csrc/fa_bwd_mla_prefill_gfx950.hip).

MLA_PREFILL_DIMS = (192, 128, 64)   # q / key, k_nope / v / out, k_pe


def _mla_prefill_rows(x, free_head_stride):
    """x [T, H, W] as the kernel reads it, and its (token stride, head stride) in elements: in place where the innermost stride is 1,
    the head stride is W (or, free_head_stride, any multiple of 8 from W up), the token stride a multiple of 8 that holds the heads
    and the storage offset a multiple of 8; else a contiguous copy."""
    T, H, W = x.shape
    hs = x.stride(1) if H > 1 else W
    least = (max(H, 1) - 1) * hs + W
    ts = x.stride(0) if T > 1 else least
    ok = x.stride(2) == 1 and (hs == W or free_head_stride and hs >= W and hs % 8 == 0) and ts >= least and ts % 8 == 0 \
        and x.storage_offset() % 8 == 0
    if not ok:
        x = x.contiguous()
        if x.storage_offset() % 8 != 0:   # (contiguous as it stood, at an offset that is no 16-byte boundary)
            x = x.clone()
        ts, hs = H * W, W
    return x, ts, hs


def _mla_prefill_problem(d, q, k_nope, k_pe, v, strides, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale):
    """The problem statement both MLA prefill descriptors share (the tensors as _mla_prefill_rows returned them, with their strides)."""
    sq, skn, hkn, sv, hv, skp = strides
    Tq, H, _ = q.shape
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.batch, d.heads, d.qk_dim, d.v_dim = cu_q.shape[0] - 1, H, MLA_PREFILL_DIMS[0], MLA_PREFILL_DIMS[1]
    d.total_q, d.total_k = Tq, k_nope.shape[0]
    d.max_seqlen_q, d.max_seqlen_k = max(min(max_seqlen_q, Tq), 1), max(min(max_seqlen_k, k_nope.shape[0]), 1)
    d.scale = _abi_scale(scale)
    d.causal = causal
    d.device = _device_index(q.device)
    d.q_token_stride, d.k_pe_token_stride = sq, skp
    d.k_nope_token_stride, d.k_nope_head_stride, d.v_token_stride, d.v_head_stride = skn, hkn, sv, hv
    d.stream = _stream_ptr(q.device)
    d.q, d.k_nope, d.k_pe, d.v = q.data_ptr(), k_nope.data_ptr(), k_pe.data_ptr(), v.data_ptr()
    d.cu_seqlens_q, d.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
    return d


def mla_prefill_raw(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale, want_lse=True):
    """q [Tq,H,192], k_nope / v [Tk,H,128], k_pe [Tk,64] device tensors, cu_q / cu_k int32 [B + 1] on the same device, causal an
    AULE_CAUSAL_* code, scale a float.  Returns (out [Tq,H,128], lse [Tq,H] or None), both from torch.empty.  Asynchronous, no
    synchronisation."""
    lib = _capi.get_lib()
    _same_device("MLA prefill", q, k_nope, k_pe, v, cu_q, cu_k)
    q, sq, _ = _mla_prefill_rows(q, False)
    k_nope, skn, hkn = _mla_prefill_rows(k_nope, True)
    v, sv, hv = _mla_prefill_rows(v, True)
    k_pe, skp, _ = _mla_prefill_rows(k_pe.unsqueeze(1), False)
    Tq, H, _ = q.shape
    out = torch.empty((Tq, H, MLA_PREFILL_DIMS[1]), device=q.device, dtype=q.dtype)
    lse = torch.empty((Tq, H), device=q.device, dtype=torch.float32) if want_lse else None
    if Tq * H * (cu_q.shape[0] - 1) == 0:
        return out, lse
    d = _mla_prefill_problem(_capi.MlaPrefillDesc(), q, k_nope, k_pe, v, (sq, skn, hkn, sv, hv, skp), cu_q, cu_k, max_seqlen_q, max_seqlen_k,
                             causal, scale)
    d.out = out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    _capi.check(lib.aule_attention_mla_prefill_ex(ctypes.byref(d)), "aule_attention_mla_prefill_ex")
    return out, lse


def mla_prefill(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True, scale=None,
                return_lse=False):
    """MLA prefill (aule.flash_attention_mla_prefill documents the arguments; aule_mla_prefill_desc in include/aule.h is the
    contract).  No autograd: inputs that require grad are refused."""
    k_pe, code = _mla_prefill_check(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal)
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k_nope, k_pe, v)):
        raise ValueError("MLA prefill has no backward (prefill is inference): detach the inputs or call it under torch.no_grad()")
    if not q.is_cuda:
        raise _capi.AuleError("aule (HIP build): MLA prefill needs ROCm device tensors; there is no CPU fallback")
    _same_device("MLA prefill", q, k_nope, k_pe, v)
    cu_q, cu_k = _int32_on(q.device, cu_seqlens_q, cu_seqlens_k)
    max_seqlen_q, max_seqlen_k = _varlen_maxima(cu_q, cu_k, max_seqlen_q, max_seqlen_k)
    out, lse = mla_prefill_raw(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code,
                               float(1.0 / math.sqrt(MLA_PREFILL_DIMS[0]) if scale is None else scale), want_lse=return_lse)
    return (out, lse) if return_lse else out


def _mla_prefill_check(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal):
    """Every rule of the MLA prefill arguments that needs no device.  Returns (k_pe as [total_k, 64], the causal code)."""
    DQ, DV, DR = MLA_PREFILL_DIMS
    if torch.is_tensor(k_pe) and k_pe.dim() == 3 and k_pe.shape[1] == 1:
        k_pe = k_pe[:, 0]
    if not all(torch.is_tensor(x) for x in (q, k_nope, k_pe, v)) or q.dim() != 3 or k_nope.dim() != 3 or v.dim() != 3 or k_pe.dim() != 2:
        raise ValueError("expected q [total_q, heads, 192], k_nope and v [total_k, heads, 128] and k_pe [total_k, 64] (or [total_k, 1, 64])")
    if (q.shape[2], k_nope.shape[2], v.shape[2], k_pe.shape[1]) != (DQ, DV, DV, DR):
        raise ValueError(f"MLA prefill is built for 192 / 128 / 128 / 64 exactly (nothing is padded): q={q.shape[2]}, k_nope={k_nope.shape[2]}, "
                         f"v={v.shape[2]}, k_pe={k_pe.shape[1]}")
    if k_nope.shape[1] != q.shape[1] or v.shape[1] != q.shape[1]:
        raise ValueError(f"MLA prefill is multi-head attention: q, k_nope and v must have one heads count, got {q.shape[1]}, {k_nope.shape[1]}, "
                         f"{v.shape[1]} (GQA is not built)")
    if v.shape[0] != k_nope.shape[0] or k_pe.shape[0] != k_nope.shape[0]:
        raise ValueError(f"k_nope, k_pe and v must have one total_k, got {k_nope.shape[0]}, {k_pe.shape[0]}, {v.shape[0]}")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"MLA prefill is not built for {q.dtype}: fp16 and bf16 only")
    if any(x.dtype != q.dtype for x in (k_nope, k_pe, v)):
        raise ValueError(f"q, k_nope, k_pe and v must share one dtype, got {q.dtype}, {k_nope.dtype}, {k_pe.dtype}, {v.dtype}")
    _varlen_offsets(cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k)
    return k_pe, causal_code(causal)


def mla_prefill_bwd_raw(q, k_nope, k_pe, v, out, dout, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale):
    """The gradients of mla_prefill_raw: dq [Tq,H,192], dkv [Tk,H,256] -- dk_nope its columns 0 .. 127 and dv 128 .. 255, written in
    place through the output strides -- and dk_pe [Tk,64]; ZERO in the rows no sequence owns (the library never writes those; they
    are allocated zero-filled here).  out, dout, lse contiguous.  Asynchronous, no synchronisation."""
    lib = _capi.get_lib()
    _same_device("MLA attention backward", q, k_nope, k_pe, v, out, dout, lse, cu_q, cu_k)
    q, sq, _ = _mla_prefill_rows(q, False)
    k_nope, skn, hkn = _mla_prefill_rows(k_nope, True)
    v, sv, hv = _mla_prefill_rows(v, True)
    k_pe, skp, _ = _mla_prefill_rows(k_pe.unsqueeze(1), False)
    (Tq, H, _), Tk = q.shape, k_nope.shape[0]
    DQ, DV, DR = MLA_PREFILL_DIMS
    dq = torch.zeros((Tq, H, DQ), device=q.device, dtype=q.dtype)
    dkv = torch.zeros((Tk, H, 2 * DV), device=q.device, dtype=q.dtype)
    dk_pe = torch.zeros((Tk, DR), device=q.device, dtype=q.dtype)
    if H * (cu_q.shape[0] - 1) == 0 or Tq + Tk == 0:
        return dq, dkv, dk_pe
    d = _mla_prefill_problem(_capi.MlaPrefillBwdDesc(), q, k_nope, k_pe, v, (sq, skn, hkn, sv, hv, skp), cu_q, cu_k, max_seqlen_q, max_seqlen_k,
                             causal, scale)
    d.out, d.lse, d.dout = out.data_ptr(), lse.data_ptr(), dout.data_ptr()
    d.dq, d.dk_pe = dq.data_ptr(), dk_pe.data_ptr()
    d.dk_nope, d.dv = dkv.data_ptr(), dkv.data_ptr() + DV * dkv.element_size()
    d.dk_nope_token_stride = d.dv_token_stride = H * 2 * DV
    d.dk_nope_head_stride = d.dv_head_stride = 2 * DV
    ws = _attach_workspace(d, lib.aule_attention_mla_prefill_backward_workspace_size, q.device)   # held until the launch is queued
    _capi.check(lib.aule_attention_mla_prefill_backward_ex(ctypes.byref(d)), "aule_attention_mla_prefill_backward_ex")
    del ws
    return dq, dkv, dk_pe


class FlashAttentionMlaVarlenHipFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale):
        out, lse = mla_prefill_raw(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale)
        ctx.save_for_backward(q, k_nope, k_pe, v, out, lse, cu_q, cu_k)
        ctx.problem = (max_seqlen_q, max_seqlen_k, causal, scale)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k_nope, k_pe, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_seqlen_q, max_seqlen_k, causal, scale = ctx.problem
        dout = dout.contiguous().to(q.dtype)
        dq, dkv, dk_pe = mla_prefill_bwd_raw(q, k_nope, k_pe, v, out, dout, lse, cu_q, cu_k, max_seqlen_q, max_seqlen_k, causal, scale)
        DV = MLA_PREFILL_DIMS[1]
        return dq, dkv[..., :DV], dk_pe, dkv[..., DV:], None, None, None, None, None, None


def flash_attention_mla_varlen(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True, scale=None,
                               return_lse=False):
    """MLA 192 / 128 attention over a variable-length packed batch, autograd-aware (aule.flash_attention_mla_varlen documents the
    arguments; aule_mla_prefill_bwd_desc in include/aule.h is the backward's contract).  The forward is flash_attention_mla_prefill's
    launch."""
    k_pe, code = _mla_prefill_check(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal)
    if not q.is_cuda:
        raise _capi.AuleError("aule (HIP build): MLA attention needs ROCm device tensors; there is no CPU fallback")
    _same_device("MLA attention", q, k_nope, k_pe, v)
    cu_q, cu_k = _int32_on(q.device, cu_seqlens_q, cu_seqlens_k)
    max_seqlen_q, max_seqlen_k = _varlen_maxima(cu_q, cu_k, max_seqlen_q, max_seqlen_k)
    scale = float(1.0 / math.sqrt(MLA_PREFILL_DIMS[0]) if scale is None else scale)
    if torch.is_grad_enabled() and any(x.requires_grad for x in (q, k_nope, k_pe, v)):
        out, lse = FlashAttentionMlaVarlenHipFunc.apply(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code, scale)
    else:
        out, lse = mla_prefill_raw(q, k_nope, k_pe, v, cu_q, cu_k, max_seqlen_q, max_seqlen_k, code, scale, want_lse=return_lse)
    return (out, lse) if return_lse else out


# The paged prefill in three steps; the paged cascade is the same three with its prefix between them.

def _ragged_kind(op, q, k_cache, v_cache, k_scale, v_scale):
    """Step 1, what the tensors are: heads_kv and whether the caches are FP8."""
    Hkv = _paged_shapes(q, "T,Hq,D", k_cache, v_cache)
    return Hkv, _paged_cache_kind(op, q, k_cache, v_cache, k_scale, v_scale)


def _ragged_offsets(B, cu_seqlens_q, max_seqlen_q):
    """The rules of cu_seqlens_q [batch + 1] int32 and of max_seqlen_q (a positive int, or None: read from the offsets)."""
    if not torch.is_tensor(cu_seqlens_q) or cu_seqlens_q.shape != (B + 1,):
        raise ValueError(f"cu_seqlens_q must be a [batch + 1] = [{B + 1}] tensor")
    if cu_seqlens_q.dtype != torch.int32:
        raise ValueError(f"cu_seqlens_q must be int32 (it is read on the device as it stands), got {cu_seqlens_q.dtype}")
    if max_seqlen_q is not None and (isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 1):
        raise ValueError(f"max_seqlen_q must be a positive int or None, got {max_seqlen_q!r}")


def _single_token_offsets(max_seqlen_q):
    """The rule of max_seqlen_q without cu_seqlens_q: plain decode, one token per sequence."""
    if max_seqlen_q not in (None, 1):
        raise ValueError(f"max_seqlen_q must be None or 1 without cu_seqlens_q (one token per sequence), got {max_seqlen_q!r}")


def _longest_sequence(cu, B):
    """max_seqlen_q read from the offsets on the device: the one documented synchronisation of the entries that take None for it."""
    return max(int((cu[1:] - cu[:-1]).max().item()), 1) if B > 0 else 1


def _ragged_result(q, width, return_lse):
    """out [T, Hq, width] of q's dtype and lse [T, Hq] fp32 (or None) from torch.empty, and what the call returns."""
    T, Hq, _ = q.shape
    out = torch.empty((T, Hq, width), device=q.device, dtype=q.dtype)
    lse = torch.empty((T, Hq), device=q.device, dtype=torch.float32) if return_lse else None
    return out, lse, (out, lse) if return_lse else out


def _latent_shapes(q, kv_cache):
    """The latent cache as the MLA readers take it: [num_blocks, block_size, 1, 576] is read as [num_blocks, block_size, 576]; q and the
    cache are 3-d and 576 wide."""
    if kv_cache.dim() == 4 and kv_cache.shape[2] == 1:
        kv_cache = kv_cache[:, :, 0]
    if q.dim() != 3 or kv_cache.dim() != 3:
        raise ValueError("expected q [T,Hq,576] and kv_cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576])")
    if q.shape[-1] != 576 or kv_cache.shape[-1] != 576:
        raise ValueError(f"the latent width must be 576 (512 + 64): query={q.shape[-1]}, cache={kv_cache.shape[-1]}")
    return kv_cache


def _packed_tokens(q):
    """q [T, Hq, D] as the ragged kernels read it -- heads contiguous, the token stride free -- and that stride in elements."""
    T, Hq, D = q.shape
    if T > 1 and (q.stride(2) != 1 or q.stride(1) != D) or T <= 1 and not q.is_contiguous():
        q = q.contiguous()
    q_stride = q.stride(0) if T > 1 else Hq * D
    if q_stride < Hq * D or q_stride % 8 != 0 or q.storage_offset() % 8 != 0:
        raise ValueError(f"q's token stride ({q_stride}) and storage offset ({q.storage_offset()}) must be multiples of 8 elements "
                         f"and the stride at least heads_q * head_dim = {Hq * D} (16-byte loads); pass q.contiguous()")
    return q, q_stride


def _ragged_queries(op, q, fp8, Hkv, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, k_scale, v_scale):
    """Step 2, the tables and the packed queries, the last rules before the device is needed.  Returns q as the kernels read it -- heads
    contiguous, the token stride free -- and that stride in elements."""
    B = _paged_tables(block_tables, context_lens)
    _ragged_offsets(B, cu_seqlens_q, max_seqlen_q)
    _scale_shapes(fp8, Hkv, k_scale, v_scale)
    q, q_stride = _packed_tokens(q)
    _needs_device(op, q)
    return q, q_stride


def _ragged_problem(op, d, q, q_stride, fp8, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, scale, return_lse):
    """Step 3, on the device: the tables next to q, max_seqlen_q (read from cu_seqlens_q where the caller gave none), out and lse,
    and d filled with everything the two kinds share.  Returns (what the call returns, the tensors d points to -- to be held until
    the launch is queued -- or None where there is nothing to launch)."""
    k_cache, v_cache = k_cache.contiguous(), v_cache.contiguous()
    _same_device("paged " + op, q, k_cache, v_cache)
    bt, cl, cu = _int32_on(q.device, block_tables, context_lens, cu_seqlens_q)
    B, (T, Hq, D) = bt.shape[0], q.shape
    if max_seqlen_q is None:
        max_seqlen_q = _longest_sequence(cu, B)
    out, lse, result = _ragged_result(q, D, return_lse)
    if T * B * Hq == 0:
        return result, None
    _paged_problem(d, q, k_cache, v_cache, out, bt, cl, scale, fp8)
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, min(max_seqlen_q, T), q_stride
    d.lse = lse.data_ptr() if lse is not None else None
    d.cu_seqlens_q = cu.data_ptr()
    return result, [k_cache, v_cache, bt, cl, cu]


def paged_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None, window_size=-1,
                  k_scale=None, v_scale=None, return_lse=False, sinks=None, tree_mask=None):
    """Paged prefill: ragged per-sequence queries against the paged KV cache (the step of a continuous-batching engine: a
    prompt chunk behind a cached prefix next to a short verify next to plain decodes); csrc/fa_fwd_paged_prefill_gfx950.hip
    behind aule_attention_paged_prefill_ex:

        q            [total_tokens, heads_q, head_dim] fp16 / bf16: the new tokens of all sequences packed along the first axis.
                     The token stride is free (a slice of a fused QKV projection is read in place) as long as it and the storage
                     offset are multiples of 8 elements; a q whose heads are not contiguous is copied.
        k_cache, v_cache, block_tables, context_lens, k_scale, v_scale: as in paged_query (16-bit or float8_e4m3fn caches)
        cu_seqlens_q [batch + 1] int32: sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1
        max_seqlen_q the largest number of new tokens of a sequence (sizes the grid; a longer sequence is cut to it).  None
                     reads it from cu_seqlens_q with ONE device->host synchronisation; pass it to keep the call free of
                     synchronisation and capturable into a graph.
    context_lens[b] counts the keys in the cache INCLUDING the new tokens (append them first: paged_kv_append).  With L_b, s_b
    and n_b the values clamped on the device (include/aule.h), token i of sequence b is row s_b + i, sits at position
    p = L_b - n_b + i and sees key j iff j <= p, and with window_size = W > 0 iff also p - j < W.  A token with p < 0 gives a
    row of zeros and lse = -inf.  Rows that belong to no sequence are never written: out (and lse) come from torch.empty.
    Returns out [total_tokens, heads_q, head_dim], or (out, lse) with lse [total_tokens, heads_q] fp32 when return_lse is
    set.  All argument errors are ValueErrors raised before the device is touched.  sinks: [heads_q] sink logits
    (aule.flash_attention_paged_prefill_sinks), behind aule_attention_paged_prefill_sink_ex.  tree_mask: [total_tokens] int64 words
    (aule.flash_attention_paged_prefill_tree), behind aule_attention_paged_prefill_tree_ex."""
    Hkv, fp8 = _ragged_kind("prefill", q, k_cache, v_cache, k_scale, v_scale)
    if sinks is not None:
        _sinks_check(sinks, q)
    if tree_mask is not None:
        _no_tree_extras(window_size, sinks)
        _tree_mask_check(tree_mask, (q.shape[0],), "[total_tokens]", q)
    q, q_stride = _ragged_queries("prefill", q, fp8, Hkv, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, k_scale, v_scale)
    lib = _capi.get_lib()
    d = _capi.PagedPrefillTreeDesc() if tree_mask is not None else _capi.PagedPrefillDesc() if sinks is None else _capi.PagedPrefillSinkDesc()
    result, held = _ragged_problem("prefill", d, q, q_stride, fp8, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q,
                                   scale, return_lse)
    if held is not None:
        d.window_size = _window_arg(window_size)
        held.append(_attach_scales(d, fp8, k_scale, v_scale, Hkv, q.device))
        launch = "aule_attention_paged_prefill_ex"
        if sinks is not None:
            launch = "aule_attention_paged_prefill_sink_ex"
            held.append(_sinks_f32(sinks))
            d.sinks = held[-1].data_ptr()
        if tree_mask is not None:
            launch = "aule_attention_paged_prefill_tree_ex"
            d.tree_mask = tree_mask.data_ptr()
        _capi.check(getattr(lib, launch)(ctypes.byref(d)), launch)
    return result


FP8MMA_HEAD_DIMS = (64, 128)


def quantize_rows_fp8(x):
    """aule.quantize_rows_fp8: per-row e4m3 codes and fp32 scales over the last axis, the rule csrc/fa_fwd_paged_prefill_fp8mma_gfx950.hip
    applies to q in registers (a true fp32 division by s = amax / 448, s = 1 for a zero row, round to nearest even)."""
    if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() < 1:
        raise ValueError("quantize_rows_fp8 takes a floating-point tensor with at least one axis")
    xf = x.float()
    amax = xf.abs().amax(dim=-1, keepdim=True)
    scales = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (xf / scales).clamp(-448.0, 448.0).to(torch.float8_e4m3fn), scales


def paged_prefill_fp8mma(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None, window_size=-1,
                         k_scale=None, v_scale=None, return_lse=False):
    """paged_prefill over an FP8 cache with both matrix products in FP8 (aule.flash_attention_paged_prefill_fp8mma states the
    arithmetic); csrc/fa_fwd_paged_prefill_fp8mma_gfx950.hip behind aule_attention_paged_prefill_fp8mma_ex.  The twin's steps and rules,
    plus this entry's own three: float8_e4m3fn caches, both scales given, head_dim 64 or 128."""
    Hkv, fp8 = _ragged_kind("prefill", q, k_cache, v_cache, k_scale, v_scale)
    if not fp8:
        raise ValueError(f"flash_attention_paged_prefill_fp8mma multiplies float8_e4m3fn codes: the caches must be float8_e4m3fn, got "
                         f"{k_cache.dtype} (a 16-bit cache: flash_attention_paged_prefill)")
    if k_scale is None or v_scale is None:
        raise ValueError("flash_attention_paged_prefill_fp8mma needs k_scale and v_scale, the scales the cache was written with "
                         "(flash_attention_paged_prefill takes 1.0 for a missing one)")
    if q.shape[-1] not in FP8MMA_HEAD_DIMS:
        raise ValueError(f"head_dim must be one of {FP8MMA_HEAD_DIMS} for flash_attention_paged_prefill_fp8mma, got {q.shape[-1]} "
                         "(head_dim 32: flash_attention_paged_prefill)")
    q, q_stride = _ragged_queries("prefill", q, fp8, Hkv, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, k_scale, v_scale)
    lib = _capi.get_lib()
    d = _capi.PagedPrefillDesc()
    result, held = _ragged_problem("prefill", d, q, q_stride, fp8, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q,
                                   scale, return_lse)
    if held is not None:
        d.window_size = _window_arg(window_size)
        held.append(_attach_scales(d, fp8, k_scale, v_scale, Hkv, q.device))
        _capi.check(lib.aule_attention_paged_prefill_fp8mma_ex(ctypes.byref(d)), "aule_attention_paged_prefill_fp8mma_ex")
    return result


def paged_cascade(q, k_cache, v_cache, prefix_block_table, prefix_len, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None,
                  scale=None, k_scale=None, v_scale=None, return_lse=False):
    """Paged cascade: paged_prefill for a batch whose sequences share a prefix (a system prompt, a few-shot header), the prefix
    read once for the whole batch; csrc/fa_fwd_paged_shared_prefix_gfx950.hip, the paged prefill and
    csrc/fa_merge_states_gfx950.hip behind aule_attention_paged_cascade_ex:

        q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, k_scale, v_scale: as in paged_prefill
        prefix_block_table [max_prefix_blocks] integer: the blocks of the shared prefix
        prefix_len   int32 [1] tensor on q's device, read and clamped on the device to what the table addresses; a Python int
                     is wrapped (a constant of a captured graph then; pass a tensor to change it between replays)
        block_tables [batch, max_blocks]: each sequence's OWN blocks;  context_lens [batch]: its OWN keys, the new tokens included
    The keys of sequence b are the P prefix keys followed by its L_b own keys: token i sits at own position p = L_b - n_b + i,
    sees every prefix key and own key j iff j <= p.  A token with p < 0 gives zeros and lse = -inf; P = 0 equals paged_prefill
    bit for bit.  Rows that belong to no sequence are never written.  The key splits of the prefix are planned from the prefix
    table's capacity (no device->host read): size the table to the prefix.  Returns out, or (out, lse) with return_lse; lse
    covers prefix and own keys.  Not built: a sliding window, head_dim 256, a backward.  All argument errors are ValueErrors
    raised before the device is touched."""
    Hkv, fp8 = _ragged_kind("cascade", q, k_cache, v_cache, k_scale, v_scale)
    if not torch.is_tensor(prefix_block_table) or prefix_block_table.dim() != 1 or prefix_block_table.shape[0] == 0 \
            or prefix_block_table.dtype not in (torch.int32, torch.int64):
        raise ValueError("prefix_block_table must be a non-empty integer [max_prefix_blocks] tensor")
    if torch.is_tensor(prefix_len):
        if prefix_len.shape != (1,) or prefix_len.dtype != torch.int32:
            raise ValueError(f"prefix_len must be an int32 [1] tensor (it is read on the device as it stands) or a Python int, "
                             f"got {prefix_len.dtype} {tuple(prefix_len.shape)}")
    elif isinstance(prefix_len, bool) or not isinstance(prefix_len, int) or not -2 ** 31 <= prefix_len < 2 ** 31:
        raise ValueError(f"prefix_len must be an int32 [1] tensor or a Python int, got {prefix_len!r}")
    q, q_stride = _ragged_queries("cascade", q, fp8, Hkv, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, k_scale, v_scale)
    lib = _capi.get_lib()
    d = _capi.PagedCascadeDesc()
    result, held = _ragged_problem("cascade", d, q, q_stride, fp8, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q,
                                   scale, return_lse)
    if held is not None:
        pbt, = _int32_on(q.device, prefix_block_table)
        plen = prefix_len.to(device=q.device) if torch.is_tensor(prefix_len) else torch.tensor([prefix_len], device=q.device, dtype=torch.int32)
        d.max_prefix_blocks, d.prefix_block_table, d.prefix_len = pbt.shape[0], pbt.data_ptr(), plen.data_ptr()
        held += [pbt, plen, _attach_workspace(d, lib.aule_attention_paged_cascade_workspace_size, q.device),
                 _attach_scales(d, fp8, k_scale, v_scale, Hkv, q.device)]
        _capi.check(lib.aule_attention_paged_cascade_ex(ctypes.byref(d)), "aule_attention_paged_cascade_ex")
    return result


def mla_paged(q, kv_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, scale=None, return_lse=False):
    """Paged multi-head latent attention (DeepSeek-V2 / V3 / R1, absorbed form), decode and short verify over a latent KV cache;
    csrc/fa_fwd_mla_paged_gfx950.hip behind aule_attention_mla_paged_ex, whose descriptor comment in include/aule.h is the contract:

        q            [total_tokens, heads_q, 576] fp16 / bf16 (512 compressed dimensions, then 64 rotary ones); token stride free as
                     in paged_prefill
        kv_cache     [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]) of q's dtype: ONE cache, a row is the key of
                     every head and, in its first 512 elements, the value
        block_tables, context_lens, cu_seqlens_q, max_seqlen_q: as in paged_prefill; cu_seqlens_q = None is plain decode (sequence
                     b owns row b: q.shape[0] == batch), and max_seqlen_q = None with offsets given costs ONE device->host
                     synchronisation
        scale        None = 1/sqrt(576), the library's rule; DeepSeek models pass their own 1/sqrt(192) * mscale
    Returns out [total_tokens, heads_q, 512], or (out, lse).  Rows that belong to no sequence are never written: out (and lse) come
    from torch.empty.  All argument errors are ValueErrors raised before the device is touched."""
    return _mla_paged(False, q, kv_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, scale, return_lse, None)


def mla_paged_fp8(q, kv_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, scale=None, return_lse=False, kv_scale=None):
    """mla_paged over an FP8 latent cache (csrc/fa_fwd_mla_paged_fp8_gfx950.hip behind aule_attention_mla_paged_fp8_ex): kv_cache
    [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]) torch.float8_e4m3fn, key = kv_scale * float(code row), value =
    its first 512 elements; kv_scale None (1.0), a float, or a 0-d / [1] tensor, which stays on the device (no device->host copy).
    Every other argument, the result and the errors are mla_paged's; lse includes kv_scale."""
    return _mla_paged(True, q, kv_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, scale, return_lse, kv_scale)


def _latent_cache_kind(what, dtype, kv_cache, fp8, kv_scale, sixteen):
    """The cache-kind rules of the two MLA readers and the latent append: a cache of the 16-bit `dtype`, or (fp8) torch.float8_e4m3fn
    codes with ONE scale -- None, a float, a 0-d or [1] tensor.  sixteen: where a 16-bit cache goes, for the message."""
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{what} must be fp16 or bf16, got {dtype}")
    if fp8:
        if kv_cache.dtype != torch.float8_e4m3fn:
            raise ValueError(f"an FP8 latent cache must be torch.float8_e4m3fn, got {kv_cache.dtype} (gfx950 converts OCP e4m3fn in "
                             f"hardware; e4m3fnuz and e5m2 are not built; {sixteen})")
        if torch.is_tensor(kv_scale) and not (kv_scale.dim() == 0 or kv_scale.shape == (1,)):
            raise ValueError(f"kv_scale must be None, a float, or a 0-d / [1] tensor (one value for the whole cache), got shape {tuple(kv_scale.shape)}")
    elif kv_scale is not None:
        raise ValueError("kv_scale applies to a float8_e4m3fn cache only; a 16-bit cache holds the values themselves")


_NO_TREE = object()   # (None is a caller's mistake where words are expected)


def mla_paged_tree(q, kv_cache, tree_mask, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None, return_lse=False,
                   kv_scale=None):
    """mla_paged / mla_paged_fp8 with a tree of new tokens per sequence (csrc/fa_fwd_mla_verify_gfx950.hip behind
    aule_attention_mla_paged_tree_ex; aule.flash_attention_mla_paged_tree documents the arguments).  The cache kind is kv_cache's dtype;
    tree_mask [total_tokens] int64 on q's device is read by the kernel on every launch.  Validation, descriptor prefix, workspace and the
    one possible synchronisation (max_seqlen_q = None) are mla_paged's."""
    return _mla_paged(None, q, kv_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, scale, return_lse, kv_scale, tree_mask)


def _mla_paged(fp8, q, kv_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, scale, return_lse, kv_scale, tree_mask=_NO_TREE):
    """Both cache kinds of the paged MLA: one validation, one descriptor (the FP8 kind's is the 16-bit kind's plus kv_scale; the tree
    kind's is the FP8 kind's plus the words and the cache kind, which it reads from kv_cache's dtype: fp8 = None)."""
    kv_cache = _latent_shapes(q, kv_cache)
    tree = tree_mask is not _NO_TREE
    if tree:
        fp8 = kv_cache.dtype != q.dtype
        _latent_cache_kind("q", q.dtype, kv_cache, fp8, kv_scale, "a 16-bit cache has q's dtype")
        if cu_seqlens_q is None:
            raise ValueError("cu_seqlens_q is required with tree_mask: a tree of one node per sequence is the decode call "
                             "(flash_attention_mla_paged / _fp8)")
        _tree_mask_check(tree_mask, (q.shape[0],), "[total_tokens]", q)
    elif fp8:
        _latent_cache_kind("q", q.dtype, kv_cache, True, kv_scale, "a 16-bit cache is flash_attention_mla_paged's")
    elif q.dtype not in (torch.float16, torch.bfloat16) or kv_cache.dtype != q.dtype:
        raise ValueError(f"q and kv_cache must share one of fp16 / bf16, got {q.dtype} and {kv_cache.dtype}")
    if kv_cache.shape[1] == 0:
        raise ValueError("block_size must be positive")
    B = _paged_tables(block_tables, context_lens, None if cu_seqlens_q is not None else q.shape[0])
    if cu_seqlens_q is not None:
        _ragged_offsets(B, cu_seqlens_q, max_seqlen_q)
    else:
        _single_token_offsets(max_seqlen_q)
    q, q_stride = _packed_tokens(q)
    _needs_device("MLA", q)
    lib = _capi.get_lib()
    kv_cache = kv_cache.contiguous()
    _same_device("paged MLA", q, kv_cache)
    held = _int32_on(q.device, block_tables, context_lens) + ([] if cu_seqlens_q is None else _int32_on(q.device, cu_seqlens_q))
    bt, cl, cu = held[0], held[1], held[2] if cu_seqlens_q is not None else None
    T, Hq, _ = q.shape
    if cu is None:
        max_seqlen_q = 1
    elif max_seqlen_q is None:
        max_seqlen_q = _longest_sequence(cu, B)
    out, lse, result = _ragged_result(q, 512, return_lse)
    if T * B * Hq == 0:
        return result
    d = _capi.MlaPagedTreeDesc() if tree else _capi.MlaPagedFp8Desc() if fp8 else _capi.MlaPagedDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.batch, d.heads_q, d.qk_dim, d.v_dim = B, Hq, 576, 512
    d.block_size, d.max_blocks = kv_cache.shape[1], bt.shape[1]
    d.total_tokens, d.max_seqlen_q, d.q_token_stride = T, min(max_seqlen_q, T), q_stride
    d.scale = _abi_scale(1.0 / math.sqrt(576) if scale is None else scale)
    d.device = _device_index(q.device)
    d.stream = _stream_ptr(q.device)
    d.q, d.kv_cache, d.out = q.data_ptr(), kv_cache.data_ptr(), out.data_ptr()
    d.block_tables, d.context_lens = bt.data_ptr(), cl.data_ptr()
    d.cu_seqlens_q = cu.data_ptr() if cu is not None else None
    d.lse = lse.data_ptr() if lse is not None else None
    entry = "aule_attention_mla_paged_tree" if tree else "aule_attention_mla_paged_fp8" if fp8 else "aule_attention_mla_paged"
    if fp8:
        held.append(_fp8_scale(kv_scale, 1, q.device, "kv_scale"))
        d.kv_scale = held[-1].data_ptr()
    if tree:
        d.tree_mask = tree_mask.data_ptr()
        d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    held += [kv_cache, _attach_workspace(d, getattr(lib, entry + "_workspace_size"), q.device)]   # held until the launch is queued
    _capi.check(getattr(lib, entry + "_ex")(ctypes.byref(d)), entry + "_ex")
    return result


MLA_SPARSE_MAX_TOPK = 65536


def mla_sparse(q, kv_cache, indices, scale=None, return_lse=False, kv_scale=None):
    """Sparse multi-head latent attention (DeepSeek-V3.2 "DSA", absorbed form): every token attends to the cache rows its own list
    names; csrc/fa_fwd_mla_sparse_gfx950.hip behind aule_attention_mla_sparse_ex, whose descriptor comment in include/aule.h is the
    contract (aule.flash_attention_mla_sparse documents the arguments).  One launch (plus the combine when the list is split), no
    device->host copy, no synchronisation.  All argument errors are ValueErrors raised before the device is touched; CPU tensors
    that pass them are an AuleError."""
    kv_cache = _latent_shapes(q, kv_cache)
    if torch.is_tensor(indices) and indices.dim() == 3 and indices.shape[1] == 1:
        indices = indices[:, 0]
    T, Hq, _ = q.shape
    fp8 = kv_cache.dtype != q.dtype
    _latent_cache_kind("q", q.dtype, kv_cache, fp8, kv_scale, "a 16-bit cache has q's dtype")
    if Hq == 0:
        raise ValueError("q has no heads")
    if not torch.is_tensor(indices) or indices.dim() != 2 or indices.shape[0] != T:
        raise ValueError(f"indices must be a [{T}, topk] (or [{T}, 1, topk]) int32 tensor of slots")
    if indices.dtype != torch.int32:
        raise ValueError(f"indices must be int32 (the kernel reads them as they stand; nothing is converted silently), got {indices.dtype}: "
                         f"pass indices.to(torch.int32)")
    topk = indices.shape[1]
    if not 1 <= topk <= MLA_SPARSE_MAX_TOPK:
        raise ValueError(f"topk (indices.shape[-1]) must be in 1 .. {MLA_SPARSE_MAX_TOPK}, got {topk}")
    if not indices.is_contiguous():
        raise ValueError("indices must be contiguous: the kernel reads them in place on every launch")
    if not kv_cache.is_contiguous():
        raise ValueError("kv_cache must be contiguous: it is addressed as a flat array of num_blocks * block_size slots")
    slots = kv_cache.shape[0] * kv_cache.shape[1]
    if not 1 <= slots <= 2 ** 31 - 1:
        raise ValueError(f"the cache must hold 1 .. 2^31 - 1 slots (num_blocks * block_size), got {slots}")
    if (T + 64) * Hq > 2 ** 31 - 1:
        raise ValueError(f"total_tokens * heads_q = {T} * {Hq} is too large (packed rows are counted in 32 bits)")
    if torch.is_grad_enabled() and (q.requires_grad or kv_cache.requires_grad):
        raise ValueError("sparse MLA attention has no backward: detach the inputs or call it under torch.no_grad()")
    q, q_stride = _packed_tokens(q)
    if not q.is_cuda:
        raise _capi.AuleError("aule (HIP build): sparse MLA attention needs ROCm device tensors; there is no CPU fallback")
    _same_device("sparse MLA", q, kv_cache, indices)
    out, lse, result = _ragged_result(q, 512, return_lse)
    if T == 0:
        return result
    lib = _capi.get_lib()
    d = _capi.MlaSparseDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.heads_q, d.num_blocks, d.block_size = Hq, kv_cache.shape[0], kv_cache.shape[1]
    d.total_tokens, d.topk, d.q_token_stride = T, topk, q_stride
    d.scale = _abi_scale(1.0 / math.sqrt(576) if scale is None else scale)
    d.device = _device_index(q.device)
    d.stream = _stream_ptr(q.device)
    d.q, d.kv_cache, d.indices, d.out = q.data_ptr(), kv_cache.data_ptr(), indices.data_ptr(), out.data_ptr()
    d.lse = lse.data_ptr() if lse is not None else None
    held = [q]
    if fp8:
        held.append(_fp8_scale(kv_scale, 1, q.device, "kv_scale"))
        d.kv_scale = held[-1].data_ptr()
    held.append(_attach_workspace(d, lib.aule_attention_mla_sparse_workspace_size, q.device))   # held until the launch is queued
    _capi.check(lib.aule_attention_mla_sparse_ex(ctypes.byref(d)), "aule_attention_mla_sparse_ex")
    return result


MLA_INDEXER_MAX_HEADS = 64
MLA_INDEXER_MAX_TOPK = 65536
_INDEXER_OUTPUTS = {"slots": _capi.INDEXER_SLOTS, "positions": _capi.INDEXER_POSITIONS}


def _indexer_tables(T, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, block_size):
    """The table, length and offset rules the two indexer entries share.  The kernels read these tensors IN PLACE on every launch (a
    graph replay sees their current contents), so nothing is converted or copied: int32 and contiguous or a ValueError.  Returns
    (batch, max_seqlen_q as the descriptor takes it); max_seqlen_q = None with offsets is total_tokens -- no sequence has more -- and
    costs no synchronisation, only a larger grid."""
    for name, t in (("block_tables", block_tables), ("context_lens", context_lens)) + ((("cu_seqlens_q", cu_seqlens_q),) if cu_seqlens_q is not None else ()):
        if not torch.is_tensor(t) or t.dtype != torch.int32:
            raise ValueError(f"{name} must be an int32 tensor (it is read on the device as it stands), got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous: the kernel reads it in place on every launch")
    B = _paged_tables(block_tables, context_lens, None if cu_seqlens_q is not None else T)
    if cu_seqlens_q is not None:
        _ragged_offsets(B, cu_seqlens_q, max_seqlen_q)
        max_seqlen_q = max(min(T if max_seqlen_q is None else max_seqlen_q, T), 1)
    else:
        _single_token_offsets(max_seqlen_q)
        max_seqlen_q = 1
    if isinstance(block_size, bool) or not isinstance(block_size, int) or block_size < 1:
        raise ValueError(f"block_size must be a positive int, got {block_size!r}")
    if block_size * block_tables.shape[1] >= 2 ** 30:
        raise ValueError(f"max_blocks * block_size = {block_tables.shape[1]} * {block_size} must stay below 2^30")
    return B, max_seqlen_q


def mla_indexer_logits(q, weights, k_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, k_scale=None):
    """The index logits of the sparse MLA's indexer, logits[t, s] = sum_h weights[t, h] * relu(q[t, h] . k[s]) over a paged cache of
    index keys; csrc/fa_mla_indexer_gfx950.hip behind aule_mla_indexer_logits_ex, whose descriptor comment in include/aule.h is the
    contract (aule.mla_indexer_logits documents the arguments).  One launch, no device->host copy, no synchronisation.  All argument
    errors are ValueErrors raised before the device is touched; CPU tensors that pass them are an AuleError."""
    if torch.is_tensor(k_cache) and k_cache.dim() == 4 and k_cache.shape[2] == 1:
        k_cache = k_cache[:, :, 0]
    if not torch.is_tensor(q) or not torch.is_tensor(k_cache) or q.dim() != 3 or k_cache.dim() != 3:
        raise ValueError("expected q [T,H,128] and k_cache [num_blocks, block_size, 128] (or [num_blocks, block_size, 1, 128])")
    if q.shape[-1] != 128 or k_cache.shape[-1] != 128:
        raise ValueError(f"the index head width must be 128: query={q.shape[-1]}, cache={k_cache.shape[-1]}")
    T, H, _ = q.shape
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"q must be fp16 or bf16, got {q.dtype}")
    if not 1 <= H <= MLA_INDEXER_MAX_HEADS:
        raise ValueError(f"the indexer takes 1 .. {MLA_INDEXER_MAX_HEADS} index heads, got {H}")
    fp8 = k_cache.dtype != q.dtype
    if fp8 and k_cache.dtype != torch.float8_e4m3fn:
        raise ValueError(f"k_cache must have q's dtype ({q.dtype}) or be torch.float8_e4m3fn codes with k_scale, got {k_cache.dtype}")
    if fp8 and k_scale is None:
        raise ValueError("a float8_e4m3fn k_cache needs k_scale, the per-row scales [num_blocks, block_size] fp32 (quantize_indexer_cache_fp8)")
    if not fp8 and k_scale is not None:
        raise ValueError("k_scale applies to a float8_e4m3fn cache only; a 16-bit cache holds the values themselves")
    if fp8 and (not torch.is_tensor(k_scale) or k_scale.dtype != torch.float32 or tuple(k_scale.shape) != tuple(k_cache.shape[:2])
                or not k_scale.is_contiguous()):
        raise ValueError(f"k_scale must be a contiguous fp32 tensor [num_blocks, block_size] = {list(k_cache.shape[:2])} (one scale per cache row)")
    if not torch.is_tensor(weights) or weights.dtype != torch.float32 or tuple(weights.shape) != (T, H) or not weights.is_contiguous():
        raise ValueError(f"weights must be a contiguous fp32 tensor [T, H] = [{T}, {H}]")
    if not k_cache.is_contiguous():
        raise ValueError("k_cache must be contiguous")
    if k_cache.shape[0] == 0 or k_cache.shape[1] == 0 or k_cache.shape[0] * k_cache.shape[1] > 2 ** 31 - 1:
        raise ValueError(f"the cache must hold 1 .. 2^31 - 1 rows (num_blocks * block_size), got {k_cache.shape[0]} * {k_cache.shape[1]}")
    B, max_sq = _indexer_tables(T, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, k_cache.shape[1])
    if torch.is_grad_enabled() and (q.requires_grad or weights.requires_grad or k_cache.requires_grad):
        raise ValueError("the MLA indexer has no backward: detach the inputs or call it under torch.no_grad()")
    q, q_stride = _packed_tokens(q)
    if not q.is_cuda:
        raise _capi.AuleError("aule (HIP build): the MLA indexer needs ROCm device tensors; there is no CPU fallback")
    tensors = [weights, k_cache, block_tables, context_lens] + ([k_scale] if fp8 else []) + ([cu_seqlens_q] if cu_seqlens_q is not None else [])
    _same_device("MLA indexer", q, *tensors)
    W = block_tables.shape[1] * k_cache.shape[1]
    logits = torch.empty((T, W), device=q.device, dtype=torch.float32)
    if T == 0 or B == 0:
        return logits
    lib = _capi.get_lib()
    d = _capi.MlaIndexerLogitsDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[q.dtype]
    d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.heads, d.head_dim, d.batch = H, 128, B
    d.num_blocks, d.block_size, d.max_blocks = k_cache.shape[0], k_cache.shape[1], block_tables.shape[1]
    d.total_tokens, d.max_seqlen_q = T, max_sq
    d.q_token_stride, d.logits_stride = q_stride, W
    d.device = _device_index(q.device)
    d.stream = _stream_ptr(q.device)
    d.q, d.weights, d.k_cache, d.logits = q.data_ptr(), weights.data_ptr(), k_cache.data_ptr(), logits.data_ptr()
    d.k_scale = k_scale.data_ptr() if fp8 else None
    d.block_tables, d.context_lens = block_tables.data_ptr(), context_lens.data_ptr()
    d.cu_seqlens_q = cu_seqlens_q.data_ptr() if cu_seqlens_q is not None else None
    _capi.check(lib.aule_mla_indexer_logits_ex(ctypes.byref(d)), "aule_mla_indexer_logits_ex")
    return logits


def _indexer_topk_args(topk, output):
    """The rules of topk and output, which mla_indexer checks before its first launch."""
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= MLA_INDEXER_MAX_TOPK:
        raise ValueError(f"topk must be an int in 1 .. {MLA_INDEXER_MAX_TOPK}, got {topk!r}")
    if output not in _INDEXER_OUTPUTS:
        raise ValueError(f"output must be 'slots' or 'positions', got {output!r}")


def mla_indexer_topk(logits, topk, block_tables, context_lens, block_size, cu_seqlens_q=None, max_seqlen_q=None, output="slots"):
    """The per-token top-k key lists of the sparse MLA's indexer from fp32 logits [T, max_blocks * block_size];
    csrc/fa_mla_indexer_gfx950.hip behind aule_mla_indexer_topk_ex, whose descriptor comment in include/aule.h is the contract
    (aule.mla_indexer_topk documents the arguments).  One launch, no synchronisation, deterministic.  All argument errors are
    ValueErrors raised before the device is touched; CPU tensors that pass them are an AuleError."""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"logits must be an fp32 [T, max_blocks * block_size] tensor, got {logits.dtype if torch.is_tensor(logits) else type(logits).__name__}")
    _indexer_topk_args(topk, output)
    T = logits.shape[0]
    B, max_sq = _indexer_tables(T, block_tables, context_lens, cu_seqlens_q, max_seqlen_q, block_size)
    W = block_tables.shape[1] * block_size
    if logits.shape[1] != W:
        raise ValueError(f"logits must have max_blocks * block_size = {block_tables.shape[1]} * {block_size} = {W} columns, got {logits.shape[1]}")
    if W > 1 and logits.stride(1) != 1 or T > 1 and logits.stride(0) < W:
        raise ValueError("the rows of logits must be contiguous (any row stride >= the width): pass logits.contiguous()")
    if torch.is_grad_enabled() and logits.requires_grad:
        raise ValueError("the MLA indexer has no backward: detach the inputs or call it under torch.no_grad()")
    if not logits.is_cuda:
        raise _capi.AuleError("aule (HIP build): the MLA indexer needs ROCm device tensors; there is no CPU fallback")
    _same_device("MLA indexer", logits, block_tables, context_lens, *([cu_seqlens_q] if cu_seqlens_q is not None else []))
    indices = torch.empty((T, topk), device=logits.device, dtype=torch.int32)
    if T == 0 or B == 0:
        return indices
    lib = _capi.get_lib()
    d = _capi.MlaIndexerTopkDesc()
    d.struct_size = ctypes.sizeof(d)
    d.output, d.topk, d.batch = _INDEXER_OUTPUTS[output], topk, B
    d.block_size, d.max_blocks = block_size, block_tables.shape[1]
    d.total_tokens, d.max_seqlen_q = T, max_sq
    d.logits_stride = logits.stride(0) if T > 1 else W
    d.device = _device_index(logits.device)
    d.stream = _stream_ptr(logits.device)
    d.logits, d.indices = logits.data_ptr(), indices.data_ptr()
    d.block_tables, d.context_lens = block_tables.data_ptr(), context_lens.data_ptr()
    d.cu_seqlens_q = cu_seqlens_q.data_ptr() if cu_seqlens_q is not None else None
    _capi.check(lib.aule_mla_indexer_topk_ex(ctypes.byref(d)), "aule_mla_indexer_topk_ex")
    return indices


def mla_indexer(q, weights, k_cache, block_tables, context_lens, topk, cu_seqlens_q=None, max_seqlen_q=None, k_scale=None, output="slots",
                return_logits=False):
    """mla_indexer_logits, then mla_indexer_topk on its result: the two launches in a row.  topk and output are checked before the
    first launch.  Returns indices [T, topk] int32, or (indices, logits)."""
    _indexer_topk_args(topk, output)
    logits = mla_indexer_logits(q, weights, k_cache, block_tables, context_lens, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q,
                                k_scale=k_scale)
    block_size = k_cache.shape[1]
    indices = mla_indexer_topk(logits, topk, block_tables, context_lens, block_size, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q,
                               output=output)
    return (indices, logits) if return_logits else indices


def quantize_indexer_cache_fp8(k_cache):
    """(codes, k_scale) for the indexer's FP8 key cache: float8_e4m3fn codes of an index key cache [num_blocks, block_size, 128] (or
    [..., 1, 128]) and one scale PER ROW, k_scale [num_blocks, block_size] fp32 = the row's amax / 448 (1.0 for an all-zero row), with
    k_cache ~= k_scale[..., None] * codes.  Divided, clamped to +-448 (torch's cast does not saturate), then cast.  Plain torch ops;
    works on CPU tensors."""
    if torch.is_tensor(k_cache) and k_cache.dim() == 4 and k_cache.shape[2] == 1:
        k_cache = k_cache[:, :, 0]
    if not torch.is_tensor(k_cache) or k_cache.dim() != 3 or k_cache.shape[-1] != 128:
        raise ValueError("expected an index key cache [num_blocks, block_size, 128] (or [num_blocks, block_size, 1, 128])")
    x = k_cache.float()
    amax = x.abs().amax(dim=-1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax)).contiguous()
    return (x / scale[..., None]).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn), scale


def quantize_mla_cache_fp8(kv_cache):
    """(codes, scale) for the FP8 paged MLA: float8_e4m3fn codes of a [num_blocks, block_size, 576] (or [..., 1, 576]) latent cache and
    ONE scale, a [1] fp32 tensor on the cache's device = amax / 448 (1.0 for an all-zero cache), with kv_cache ~= scale * codes.
    quantize_kv_cache_fp8's formula with one head: divided, clamped to +-448 (torch's cast does not saturate), then cast.  Plain torch
    ops; works on CPU tensors."""
    if kv_cache.dim() not in (3, 4) or kv_cache.shape[-1] != 576 or (kv_cache.dim() == 4 and kv_cache.shape[2] != 1):
        raise ValueError("expected a latent cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576])")
    x = kv_cache.float()
    amax = x.abs().amax().reshape(1) if x.numel() else x.new_zeros(1)
    scale = torch.where(amax > 0, amax / FP8_MAX, torch.ones_like(amax)).contiguous()
    return (x / scale).clamp_(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn), scale


def mla_kv_append(c_kv, k_pe, kv_cache, slot_mapping, kv_scale=None, cos=None, sin=None, positions=None, rope_layout="half"):
    """Write the latent rows of T new tokens into the paged MLA's cache, in place, with one launch (csrc/mla_kv_append_gfx950.hip
    behind aule_mla_kv_append_ex, whose descriptor comment in include/aule.h is the contract):

        c_kv [T, 512], k_pe [T, 64] (or [T, 1, 64]) fp16 / bf16 of one dtype; the last dimension contiguous, the token strides free
                       multiples of 8 elements (slices of the fused down-projection's output are read in place)
        kv_cache       [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]), contiguous: c_kv's dtype (the bits are
                       copied) or torch.float8_e4m3fn (code = cast(clamp(x / kv_scale, -448, 448)): quantize_mla_cache_fp8 with a
                       given scale; kv_scale None (1.0), a float or a 0-d / [1] tensor, which stays on the device)
        slot_mapping   [T] integer: block * block_size + offset (paged_slot_mapping); a negative slot or one past the cache skips the
                       token entirely; two tokens with the same slot in one call: which one wins is unspecified
        cos, sin, positions (all or none): rotate k_pe first -- tables [table_len, 32], token t uses row positions[t], rope_layout
                       "half" pairs (p, p + 32) or "interleaved" pairs (2p, 2p + 1), the arithmetic of rope_raw, rounded to the
                       input's dtype before any quantisation (bit-identical to rope_raw followed by the un-rotated append).  A
                       position outside the table skips the token entirely.
    Row slot_mapping[t] of the cache becomes [c_kv[t] | k_pe'[t]].  Returns None.  No device->host synchronisation; captures into a
    graph.  All argument errors are ValueErrors raised before the device is touched; CPU tensors are an AuleError."""
    if k_pe.dim() == 3 and k_pe.shape[1] == 1:
        k_pe = k_pe[:, 0]
    if kv_cache.dim() == 4 and kv_cache.shape[2] == 1:
        kv_cache = kv_cache[:, :, 0]
    if c_kv.dim() != 2 or k_pe.dim() != 2 or kv_cache.dim() != 3:
        raise ValueError("expected c_kv [T,512], k_pe [T,64] (or [T,1,64]) and kv_cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576])")
    if c_kv.shape[1] != 512 or k_pe.shape[1] != 64 or kv_cache.shape[2] != 576:
        raise ValueError(f"the latent row is 512 + 64 = 576 wide: c_kv={c_kv.shape[1]}, k_pe={k_pe.shape[1]}, cache={kv_cache.shape[2]}")
    T = c_kv.shape[0]
    if k_pe.shape[0] != T:
        raise ValueError(f"c_kv has {T} tokens, k_pe {k_pe.shape[0]}")
    if k_pe.dtype != c_kv.dtype:
        raise ValueError(f"c_kv and k_pe must share one of fp16 / bf16, got {c_kv.dtype} and {k_pe.dtype}")
    fp8 = kv_cache.dtype != c_kv.dtype
    _latent_cache_kind("c_kv and k_pe", c_kv.dtype, kv_cache, fp8, kv_scale, "a 16-bit cache has c_kv's dtype")
    if rope_layout not in _ROPE_LAYOUTS:
        raise ValueError(f"unknown rope_layout {rope_layout!r} ('half' or 'interleaved')")
    if not kv_cache.is_contiguous():
        raise ValueError("kv_cache must be contiguous: the append writes in place and cannot copy it")
    num_blocks, block_size, _ = kv_cache.shape
    if block_size == 0:
        raise ValueError("block_size must be positive")
    for name, t, w in (("c_kv", c_kv, 512), ("k_pe", k_pe, 64)):
        if t.stride(1) != 1:
            raise ValueError(f"the last dimension of {name} must be contiguous, got stride {t.stride(1)}")
        if T > 1 and t.stride(0) < w:
            raise ValueError(f"{name}: the token stride {t.stride(0)} is smaller than a row of {w} elements")
        if (T > 1 and t.stride(0) % 8) or t.storage_offset() % 8:
            raise ValueError(f"{name}: rows must be 16-byte aligned (the token stride and the storage offset multiples of 8 elements)")
    if slot_mapping.dim() != 1 or slot_mapping.shape[0] != T or slot_mapping.dtype.is_floating_point or slot_mapping.dtype == torch.bool:
        raise ValueError(f"slot_mapping must be an integer tensor of shape [{T}]")
    rope = cos is not None or sin is not None or positions is not None
    if rope:
        if cos is None or sin is None:
            raise ValueError("cos and sin are required for RoPE (both or neither)")
        if positions is None:
            raise ValueError("positions are required with cos / sin: token t is rotated by table row positions[t]")
        if positions.dim() != 1 or positions.shape[0] != T or positions.dtype.is_floating_point or positions.dtype == torch.bool:
            raise ValueError(f"positions must be an integer tensor of shape [{T}]")
        if cos.shape[-1] != 32 or sin.shape[-1] != 32:
            raise ValueError(f"cos/sin must have shape [..., 32], got {tuple(cos.shape)} / {tuple(sin.shape)}")
    if not c_kv.is_cuda:
        raise _capi.AuleError("aule (HIP build): the MLA KV append needs ROCm device tensors; there is no CPU fallback")
    _same_device("MLA KV append", c_kv, k_pe, kv_cache)
    if T == 0 or num_blocks == 0:
        return None
    lib = _capi.get_lib()
    dev = c_kv.device
    slots = slot_mapping.to(device=dev, dtype=torch.int64).contiguous()
    d = _capi.MlaKvAppendDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[c_kv.dtype]
    d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.rope_layout = _ROPE_LAYOUTS[rope_layout]
    d.total_tokens, d.num_blocks, d.block_size = T, num_blocks, block_size
    # (a stride of a dimension of extent 1 is never used: torch reports anything there)
    d.c_kv_token_stride = c_kv.stride(0) if T > 1 else 512
    d.k_pe_token_stride = k_pe.stride(0) if T > 1 else 64
    d.device = _device_index(dev)
    d.stream = _stream_ptr(dev)
    d.c_kv, d.k_pe, d.kv_cache, d.slot_mapping = c_kv.data_ptr(), k_pe.data_ptr(), kv_cache.data_ptr(), slots.data_ptr()
    held = [slots]
    if fp8:
        held.append(_fp8_scale(kv_scale, 1, dev, "kv_scale"))
        d.kv_scale = held[-1].data_ptr()
    if rope:
        c, s_ = _rope_tables(cos, sin, 64, dev)
        pos = positions.to(device=dev, dtype=torch.int64).contiguous()
        d.table_len, d.table_pitch = c.shape[0], c.stride(0)
        d.cos, d.sin, d.positions = c.data_ptr(), s_.data_ptr(), pos.data_ptr()
        held += [c, s_, pos]
    _capi.check(lib.aule_mla_kv_append_ex(ctypes.byref(d)), "aule_mla_kv_append_ex")
    return None


def merge_states(out_a, lse_a, out_b, lse_b):
    """Two attention states of the same queries over disjoint key sets into the state over their union
    (csrc/fa_merge_states_gfx950.hip behind aule_attention_merge_states_ex):

        out_a, out_b [..., heads, head_dim] fp16 / bf16 of one shape and dtype (head_dim a multiple of 8)
        lse_a, lse_b [..., heads] fp32: the natural log of each softmax denominator (the lse the attention calls return)
    out = (w_a out_a + w_b out_b) / (w_a + w_b), lse = M + log(w_a + w_b) with M = max(lse_a, lse_b), w_x = exp(lse_x - M).  A
    side with lse = -inf holds no key: the other side comes back bit for bit; both: zeros and -inf.  Returns (out, lse).  All
    argument errors are ValueErrors raised before the device is touched."""
    if not all(torch.is_tensor(t) for t in (out_a, lse_a, out_b, lse_b)):
        raise ValueError("merge_attention_states takes four tensors (out_a, lse_a, out_b, lse_b)")
    if out_a.dim() < 2 or out_b.shape != out_a.shape:
        raise ValueError(f"expected out_a and out_b of one shape [..., heads, head_dim], got {tuple(out_a.shape)} and {tuple(out_b.shape)}")
    if out_a.dtype not in (torch.float16, torch.bfloat16) or out_b.dtype != out_a.dtype:
        raise ValueError(f"out_a and out_b must both be fp16 or both bf16, got {out_a.dtype} and {out_b.dtype}")
    if lse_a.shape != out_a.shape[:-1] or lse_b.shape != out_a.shape[:-1]:
        raise ValueError(f"lse_a and lse_b must have out's shape without head_dim, {tuple(out_a.shape[:-1])}, "
                         f"got {tuple(lse_a.shape)} and {tuple(lse_b.shape)}")
    if lse_a.dtype != torch.float32 or lse_b.dtype != torch.float32:
        raise ValueError(f"lse_a and lse_b must be float32, got {lse_a.dtype} and {lse_b.dtype}")
    D, H = out_a.shape[-1], out_a.shape[-2]
    if D == 0 or D % 8 != 0 or D > 1024:
        raise ValueError(f"head_dim must be a multiple of 8 (at most 1024), got {D}")
    rows = out_a.numel() // (H * D) if H > 0 else 0
    if rows >= 2 ** 31 or rows * H >= 2 ** 31:
        raise ValueError("too many rows")
    if not out_a.is_cuda:
        raise _capi.AuleError("aule (HIP build): merge_attention_states needs ROCm device tensors; there is no CPU fallback")
    lib = _capi.get_lib()
    _same_device("merge_attention_states", out_a, lse_a, out_b, lse_b)
    out_a, lse_a, out_b, lse_b = out_a.contiguous(), lse_a.contiguous(), out_b.contiguous(), lse_b.contiguous()
    out, lse = torch.empty_like(out_a), torch.empty_like(lse_a)
    if rows * H == 0:
        return out, lse
    d = _capi.MergeStatesDesc()
    d.struct_size = ctypes.sizeof(d)
    d.dtype = _DTYPES[out_a.dtype]
    d.rows, d.heads, d.head_dim = rows, H, D
    d.device = _device_index(out_a.device)
    d.stream = _stream_ptr(out_a.device)
    d.out_a, d.lse_a, d.out_b, d.lse_b = out_a.data_ptr(), lse_a.data_ptr(), out_b.data_ptr(), lse_b.data_ptr()
    d.out, d.lse = out.data_ptr(), lse.data_ptr()
    _capi.check(lib.aule_attention_merge_states_ex(ctypes.byref(d)), "aule_attention_merge_states_ex")
    return out, lse


def paged_slot_mapping(block_tables, positions, block_size, seq_ids=None):
    """Cache slots of tokens at `positions` of their sequences, for paged_kv_append:

        slots[t] = block_tables[seq_ids[t], positions[t] // block_size] * block_size + positions[t] % block_size

    block_tables [num_seqs, max_blocks] integer, positions [T] integer, seq_ids [T] integer (default arange(T): the
    decode case, one new token per sequence).  A negative position gives slot -1, which the append skips.  Returns int64
    on block_tables' device.  Plain torch ops; works on CPU tensors."""
    block_size = int(block_size)
    if block_size <= 0:
        raise ValueError(f"block_size must be positive, got {block_size}")
    if block_tables.dim() != 2 or positions.dim() != 1:
        raise ValueError("expected block_tables [num_seqs, max_blocks] and positions [num_tokens]")
    dev = block_tables.device
    pos = positions.to(device=dev, dtype=torch.int64)
    T = pos.shape[0]
    if seq_ids is None:
        if T > block_tables.shape[0]:
            raise ValueError(f"{T} positions for {block_tables.shape[0]} sequences: pass seq_ids for more than one token per sequence")
        seq = torch.arange(T, device=dev, dtype=torch.int64)
    else:
        seq = seq_ids.to(device=dev, dtype=torch.int64)
        if seq.shape != pos.shape:
            raise ValueError("seq_ids must have the shape of positions")
    skip = pos < 0
    p = torch.where(skip, torch.zeros_like(pos), pos)
    blk = block_tables[seq, torch.div(p, block_size, rounding_mode="floor")].to(torch.int64)
    slots = blk * block_size + p % block_size
    return torch.where(skip, torch.full_like(slots, -1), slots)


def paged_kv_append(key, value, k_cache, v_cache, slot_mapping, k_scale=None, v_scale=None, cos=None, sin=None, positions=None):
    """Write the K and V rows of T new tokens into the paged caches, in place, with one launch (csrc/kv_append_gfx950.hip):

        key, value     [T, heads_kv, head_dim] fp16 / bf16; the last dimension contiguous, token and head strides free
                       (slices of a fused QKV projection, k[b].transpose(0, 1) of a [B, Hkv, S, D] tensor: no copy)
        k_cache, v_cache [num_blocks, block_size, heads_kv, head_dim], contiguous: key's dtype (rows are copied bit for
                       bit) or both torch.float8_e4m3fn (code = cast(clamp(x / scale[hk], -448, 448)), exactly
                       quantize_kv_cache_fp8 with given scales; k_scale / v_scale as in paged_decode)
        slot_mapping   [T] integer: block * block_size + offset (paged_slot_mapping); a negative slot or one past the cache
                       is skipped; two tokens with the same slot in one call: which one wins is unspecified
        cos, sin, positions: rotate K (never V) first -- half-split pairs, token t uses table row positions[t], the
                       arithmetic of rope_raw, rounded to key's dtype before any quantisation (bit-identical to rope_raw
                       followed by the un-rotated append).  A token with a skipped slot needs no valid position; a position
                       outside the table skips the token.
    Returns None.  No device->host synchronisation; captures into a graph.  All argument errors are ValueErrors raised
    before the device is touched; CPU tensors are an AuleError (there is no fallback)."""
    if key.dim() != 3 or value.dim() != 3 or k_cache.dim() != 4 or v_cache.dim() != 4:
        raise ValueError("expected key/value [T,Hkv,D] and k_cache/v_cache [num_blocks, block_size, Hkv, D]")
    if value.shape != key.shape:
        raise ValueError(f"key/value shape mismatch: key={tuple(key.shape)}, value={tuple(value.shape)}")
    if v_cache.shape != k_cache.shape:
        raise ValueError(f"k_cache/v_cache shape mismatch: k_cache={tuple(k_cache.shape)}, v_cache={tuple(v_cache.shape)}")
    T, Hkv, D = key.shape
    num_blocks, block_size, Hc, Dc = k_cache.shape
    if Dc != D:
        raise ValueError(f"head_dim mismatch: key={D}, cache={Dc}")
    if Hc != Hkv:
        raise ValueError(f"heads_kv mismatch: key={Hkv}, cache={Hc}")
    fp8 = _paged_cache_is_fp8("append", (key, value), k_cache, v_cache, k_scale, v_scale)
    if not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise ValueError("k_cache and v_cache must be contiguous: the append writes in place and cannot copy them")
    if block_size == 0 or Hkv == 0:
        raise ValueError("block_size and heads_kv must be positive")
    for name, t in (("key", key), ("value", value)):
        if t.stride(2) != 1:
            raise ValueError(f"the last dimension of {name} must be contiguous, got stride {t.stride(2)}")
        if T > 1 and t.stride(0) < D or Hkv > 1 and t.stride(1) < D:
            raise ValueError(f"{name}: token / head strides {tuple(t.stride()[:2])} are smaller than a row of {D} elements")
        if (T > 1 and t.stride(0) % 8) or (Hkv > 1 and t.stride(1) % 8) or t.storage_offset() % 8:
            raise ValueError(f"{name}: rows must be 16-byte aligned (token / head strides and the storage offset multiples of 8 elements)")
    if slot_mapping.dim() != 1 or slot_mapping.shape[0] != T or slot_mapping.dtype.is_floating_point or slot_mapping.dtype == torch.bool:
        raise ValueError(f"slot_mapping must be an integer tensor of shape [{T}]")
    rope = cos is not None or sin is not None or positions is not None
    if rope:
        if cos is None or sin is None:
            raise ValueError("cos and sin are required for RoPE (both or neither)")
        if positions is None:
            raise ValueError("positions are required with cos / sin: token t is rotated by table row positions[t]")
        if positions.dim() != 1 or positions.shape[0] != T or positions.dtype.is_floating_point or positions.dtype == torch.bool:
            raise ValueError(f"positions must be an integer tensor of shape [{T}]")
        if cos.shape[-1] != D // 2 or sin.shape[-1] != D // 2:
            raise ValueError(f"cos/sin must have shape [..., {D // 2}], got {tuple(cos.shape)} / {tuple(sin.shape)}")
    _scale_shapes(fp8, Hkv, k_scale, v_scale)
    if not key.is_cuda:
        raise _capi.AuleError("aule (HIP build): the paged KV append needs ROCm device tensors; there is no CPU fallback")
    _same_device("paged KV append", key, value, k_cache, v_cache)
    if T == 0 or num_blocks == 0:
        return None
    lib = _capi.get_lib()
    dev = key.device
    slots = slot_mapping.to(device=dev, dtype=torch.int64).contiguous()
    d = _capi.KvAppendDesc()
    d.struct_size = ctypes.sizeof(_capi.KvAppendDesc)
    d.dtype = _DTYPES[key.dtype]
    d.cache_dtype = _capi.KV_CACHE_FP8_E4M3 if fp8 else _capi.KV_CACHE_SAME
    d.num_tokens, d.heads_kv, d.head_dim, d.num_blocks, d.block_size = T, Hkv, D, num_blocks, block_size
    # (a stride of a dimension of extent 1 is never used: torch reports anything there)
    d.key_token_stride = key.stride(0) if T > 1 else Hkv * max(key.stride(1), D)
    d.key_head_stride = key.stride(1) if Hkv > 1 else D
    d.value_token_stride = value.stride(0) if T > 1 else Hkv * max(value.stride(1), D)
    d.value_head_stride = value.stride(1) if Hkv > 1 else D
    d.device = _device_index(dev)
    d.stream = _stream_ptr(dev)
    d.key, d.value, d.k_cache, d.v_cache = key.data_ptr(), value.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr()
    d.slot_mapping = slots.data_ptr()
    scales = _attach_scales(d, fp8, k_scale, v_scale, Hkv, dev)   # noqa: F841 (held until the launch is queued)
    if rope:
        c, s = _rope_tables(cos, sin, D, dev)
        pos = positions.to(device=dev, dtype=torch.int64).contiguous()
        d.table_len, d.table_pitch = c.shape[0], c.stride(0)
        d.cos, d.sin, d.positions = c.data_ptr(), s.data_ptr(), pos.data_ptr()
    _capi.check(lib.aule_kv_cache_append_ex(ctypes.byref(d)), "aule_kv_cache_append_ex")
    return None
