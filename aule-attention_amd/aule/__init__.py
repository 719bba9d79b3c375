"""aule (MI355X / gfx950 HIP build) -- drop-in for the hot path of aule-attention.

Keeps the public surface of the reference's python/aule/__init__.py for the
FlashAttention forward/backward path:

    flash_attention(query, key, value, rot_cos=None, rot_sin=None, causal=True,
                    scale=None, window_size=-1)                    (__init__.py:104)

with the same positional order, defaults, validation (ValueError conditions of
__init__.py:140-160) and container behaviour (torch in -> torch out on the same
device/dtype and inside autograd; NumPy in -> NumPy out).  There is ONE backend:
hand-written HIP kernels for gfx950 behind libaule.so.  No Triton, no Vulkan, no CPU
fallback -- when the library or a HIP device is missing the call raises AuleError.

Also carried: the SDPA shim install() / uninstall() / scaled_dot_product_attention
(__init__.py:288-442).  Not carried over (out of scope): ComfyUI
glue, gravity/sort features.  RoPE: flash_attention_rope / precompute_rope_frequencies / apply_rope_separate
(triton_flash.py:561-703) run a rotation pass + the attention kernels; flash_attention() itself keeps the
behaviour of the reference's ROCm route and ignores rot_cos / rot_sin with a warning.  Sliding window (window_size > 0) follows the convention of the
kernel the reference runs on ROCm (triton_flash_amd.py:179-183): key j is visible to query i only if
i - j < window_size, on top of the causal rule; unlike the reference, the backward honours it too.
"""
import logging
import math
import warnings

from ._capi import AuleError

__version__ = "0.5.0+hip.gfx950"
logger = logging.getLogger(__name__)

_verbose = False


def _validate(query, key, value):
    """Shape rules of the reference, same messages (__init__.py:140-160)."""
    if query.ndim != 4:
        raise ValueError(f"query must be 4D [batch, heads, seq_len, head_dim], got shape {query.shape}")
    if key.ndim != 4:
        raise ValueError(f"key must be 4D [batch, heads, seq_len, head_dim], got shape {key.shape}")
    if value.ndim != 4:
        raise ValueError(f"value must be 4D [batch, heads, seq_len, head_dim], got shape {value.shape}")
    batch_q, heads_q, seq_q, head_dim_q = query.shape
    batch_k, heads_kv, seq_k, head_dim_k = key.shape
    batch_v, heads_v, seq_v, head_dim_v = value.shape
    if batch_q != batch_k or batch_q != batch_v:
        raise ValueError(f"Batch size mismatch: query={batch_q}, key={batch_k}, value={batch_v}")
    if head_dim_q != head_dim_k or head_dim_q != head_dim_v:
        raise ValueError(f"head_dim mismatch: query={head_dim_q}, key={head_dim_k}, value={head_dim_v}")
    if seq_k != seq_v:
        raise ValueError(f"Key/value seq_len mismatch: key={seq_k}, value={seq_v}")
    if heads_kv != heads_v:
        raise ValueError(f"Key/value heads mismatch: key={heads_kv}, value={heads_v}")
    if heads_q % heads_kv != 0:
        raise ValueError(f"heads_q ({heads_q}) must be divisible by heads_kv ({heads_kv}) for GQA")


def _hip_device():
    import torch
    if not torch.cuda.is_available():
        raise AuleError("aule (HIP build): no ROCm device visible to PyTorch; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def flash_attention(query, key, value, rot_cos=None, rot_sin=None, causal=True, scale=None, window_size=-1):
    """FlashAttention-2 on MI355X.

    Args:
        query: [batch, heads_q, seq_len_q, head_dim] torch.Tensor or numpy.ndarray
        key, value: [batch, heads_kv, seq_len_k, head_dim]
        rot_cos, rot_sin: accepted for signature compatibility; ignored with a warning
            (the reference's ROCm route drops them too: __init__.py:204).
        causal: True = top-left aligned causal mask (query i sees keys j <= i), the reference's rule;
            "bottom-right" = query i sits at position i + seq_len_k - seq_len_q (the last query sees every
            key; needs seq_len_k >= seq_len_q) -- an additive option, not in the reference
        scale: softmax scale, default 1/sqrt(head_dim)
        window_size: -1 = full attention; W > 0 = sliding window, key j visible to query i only if i - j < W

    Returns: tensor/array shaped like `query`, same container type and dtype.
    Raises: ValueError for invalid shapes; AuleError if the HIP backend is unavailable.
    """
    import numpy as np
    try:
        import torch
        is_torch = isinstance(query, torch.Tensor)
    except ImportError as e:  # torch is the device-memory plumbing of this build
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e

    _validate(query, key, value)

    if rot_cos is not None or rot_sin is not None:
        warnings.warn("RoPE is not fused in the HIP backend, ignoring rot_cos/rot_sin", stacklevel=2)
    window = int(window_size) if window_size is not None and window_size > 0 else -1

    from ._torch import flash_attention_hip

    if _verbose:
        print(f"aule-attention: hip | shape={tuple(query.shape)} | causal={causal}")

    if is_torch:
        if query.is_cuda:
            if not (key.is_cuda and value.is_cuda):
                raise ValueError("query, key and value must be on the same device")
            return flash_attention_hip(query, key, value, causal=causal, scale=scale, window=window)
        # CPU torch tensor: the reference round-trips through its device backend and
        # returns a tensor on query.device (__init__.py:210-229); same here.
        dev = _hip_device()
        with torch.no_grad():
            out = flash_attention_hip(query.to(dev), key.to(dev), value.to(dev), causal=causal, scale=scale, window=window)
        return out.to(query.device)

    # NumPy in -> NumPy out (dtype follows the input, like _cpu_attention: __init__.py:247-271)
    dev = _hip_device()
    in_dtype = query.dtype
    comp = np.float16 if in_dtype == np.float16 else np.float32
    tq = torch.from_numpy(np.ascontiguousarray(query, dtype=comp)).to(dev)
    tk = torch.from_numpy(np.ascontiguousarray(key, dtype=comp)).to(dev)
    tv = torch.from_numpy(np.ascontiguousarray(value, dtype=comp)).to(dev)
    with torch.no_grad():
        out = flash_attention_hip(tq, tk, tv, causal=causal, scale=scale, window=window)
    out_np = out.cpu().numpy()
    return out_np if out_np.dtype == in_dtype else out_np.astype(in_dtype)


# Alias for compatibility (__init__.py:275)
attention = flash_attention


def flash_attention_paged_amd(q, k_cache, v_cache, block_tables, context_lens, scale=None, window_size=-1,
                              k_scale=None, v_scale=None):
    """PagedAttention for the decode phase (one query token per sequence, vLLM-style block tables); same name,
    arguments and result as the reference's export (python/aule/triton_flash_amd.py:656-737, __init__.py:59):

        q [batch, heads_q, head_dim]; k_cache, v_cache [num_blocks, block_size, heads_kv, head_dim];
        block_tables [batch, max_blocks_per_seq]; context_lens [batch]  ->  [batch, heads_q, head_dim]

    window_size > 0 keeps only the last window_size positions of each sequence.  fp16 / bf16 ROCm tensors.

    The caches may instead both be torch.float8_e4m3fn (OCP FP8; see quantize_kv_cache_fp8) with an fp16 / bf16 query:
    then K = k_scale[hk] * k_cache and V = v_scale[hk] * v_cache, k_scale / v_scale each None (1.0), a float, a 0-d
    tensor or a [heads_kv] tensor.  float8_e4m3fnuz / float8_e5m2 caches and scales with a 16-bit cache are ValueErrors."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    if not q.is_cuda:
        raise AuleError("aule (HIP build): paged decode needs ROCm device tensors; there is no CPU fallback")
    from ._torch import paged_decode
    return paged_decode(q, k_cache, v_cache, block_tables, context_lens, scale=scale, window_size=window_size,
                        k_scale=k_scale, v_scale=v_scale)


def flash_attention_paged_query(q, k_cache, v_cache, block_tables, context_lens, scale=None, window_size=-1,
                                k_scale=None, v_scale=None, return_lse=False):
    """PagedAttention for a short multi-token query per sequence: the step that adds more than one token (verifying the
    k + 1 draft tokens of speculative decoding, multi-token prediction heads, a short prompt tail against a cached prefix).
    Not in the reference; flash_attention_paged_amd keeps its one-token rule.

        q [batch, heads_q, seq_q, head_dim] fp16 / bf16 with 1 <= seq_q <= 64, the same for every sequence;
        k_cache, v_cache, block_tables, k_scale, v_scale as in flash_attention_paged_amd (16-bit or float8_e4m3fn caches);
        context_lens [batch]: the keys in the cache INCLUDING the seq_q new tokens -- append them first (paged_kv_append).

    Query i of sequence b sits at position p = context_lens[b] - seq_q + i and sees key j iff j <= p, and with
    window_size = W > 0 iff also p - j < W: the rule of flash_attention(causal="bottom-right") on the gathered K / V.  A
    query at a negative position (a sequence shorter than seq_q) gives a row of zeros.  Returns [batch, heads_q, seq_q,
    head_dim], or (out, lse) with return_lse=True: lse [batch, heads_q, seq_q] fp32, the natural log of the sum of
    exp(scaled score) over the visible keys (-inf where there is none).  seq_q = 1 equals flash_attention_paged_amd bit for
    bit.  seq_q > 64 and per-sequence query lengths: flash_attention_paged_prefill.  Out of scope: head_dim 256.  Argument errors are ValueErrors raised before
    the device is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_query
    return paged_query(q, k_cache, v_cache, block_tables, context_lens, scale=scale, window_size=window_size,
                       k_scale=k_scale, v_scale=v_scale, return_lse=return_lse)


def flash_attention_paged_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None,
                                  window_size=-1, k_scale=None, v_scale=None, return_lse=False):
    """PagedAttention for a ragged batch: every sequence brings its own number of new tokens (a prompt chunk behind a cached
    prefix, next to a short verify, next to plain decodes) -- the step of a continuous-batching engine, in one launch and
    without gathering the pages.  Not in the reference.

        q [total_tokens, heads_q, head_dim] fp16 / bf16: the new tokens of all sequences packed along the first axis (last
          dimension contiguous, token stride free: a slice of a fused QKV projection is read in place);
        k_cache, v_cache, block_tables, k_scale, v_scale as in flash_attention_paged_query (16-bit or float8_e4m3fn caches);
        context_lens [batch]: the keys in the cache INCLUDING the new tokens -- append them first (paged_kv_append);
        cu_seqlens_q [batch + 1] int32: sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 of q and of the result;
        max_seqlen_q: the largest number of new tokens of a sequence.  None computes it from cu_seqlens_q with one
          device->host synchronisation; passing it keeps the call free of synchronisation and capturable into a graph (a
          replay then reads the current contents of cu_seqlens_q, context_lens and block_tables).

    Token i of sequence b (n_b new tokens, L_b keys) sits at position p = L_b - n_b + i and sees key j iff j <= p, and with
    window_size = W > 0 iff also p - j < W: the rule of flash_attention(causal="bottom-right") on the gathered K / V.  All
    per-sequence values are clamped on the device (lengths to what the block table addresses, offsets to total_tokens, n_b
    to max_seqlen_q), so a stale value cannot index outside a buffer.  A token at a negative position gives a row of zeros
    (lse -inf); rows that belong to no sequence (a tail padded for graph capture) are never written.  Returns
    [total_tokens, heads_q, head_dim], or (out, lse) with return_lse=True: lse [total_tokens, heads_q] fp32, the natural log
    of the sum of exp(scaled score) over the visible keys.  Out of scope: head_dim 256; key-range splits -- a batch made
    only of single-token sequences at very long context is better served by flash_attention_paged_amd /
    flash_attention_paged_query; a backward pass.  Argument errors are ValueErrors raised before the device is touched; CPU
    tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_prefill
    return paged_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                         window_size=window_size, k_scale=k_scale, v_scale=v_scale, return_lse=return_lse)


def flash_attention_paged_prefill_fp8mma(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None,
                                         window_size=-1, k_scale=None, v_scale=None, return_lse=False):
    """flash_attention_paged_prefill over a float8_e4m3fn cache with BOTH matrix products in FP8: the cache's codes are multiplied as
    they are (gfx950's block-scaled e4m3 MFMA at scale 1), nothing is turned back into 16 bits.  Not in the reference.  Opt-in: nothing
    routes here by itself.

    Every argument, clamp, mask and result as flash_attention_paged_prefill, except: the caches must be float8_e4m3fn, k_scale and
    v_scale must be given, head_dim is 64 or 128, and there are no sink or tree twins.  What differs is the arithmetic.  Each row
    (token, head) of q is quantised in the kernel by the rule of quantize_rows_fp8 -- codes of q / s with s = amax|q| / 448 -- and s joins
    the score scale; the softmax weights are rounded to e4m3 after a factor 2^8, which cancels in out and is taken out of lse.  lse is
    that of the quantised q over the dequantised cache (the weights' rounding never reaches it) up to the matrix instruction's accumulation
    of the scores: it keeps about 20 bits below the largest product q_d k_d of a row, 2^-12 of that product at head_dim 128; out carries the weights' e4m3
    rounding (2^-4 relative per weight, averaged over the keys) on top.  Use it where the FP8 cache's own accuracy is already accepted.
    Argument errors are ValueErrors raised before the device is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_prefill_fp8mma
    return paged_prefill_fp8mma(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                                window_size=window_size, k_scale=k_scale, v_scale=v_scale, return_lse=return_lse)


def quantize_rows_fp8(x):
    """The per-row e4m3 quantisation flash_attention_paged_prefill_fp8mma applies to q, stated in torch ops (any device, the CPU included):
    over the last axis, a = max |x|, s = a / 448 in fp32 (1 where a = 0), codes = (x.float() / s) as float8_e4m3fn (round to nearest even;
    |x / s| <= 448 up to one fp32 rounding, which rounds back to 448).  Returns (codes, scales): codes of x's shape, scales fp32 [..., 1];
    codes.float() * scales is what the kernel multiplies with."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import quantize_rows_fp8 as impl
    return impl(x)


def flash_attention_paged_cascade(q, k_cache, v_cache, prefix_block_table, prefix_len, block_tables, context_lens, cu_seqlens_q,
                                  max_seqlen_q=None, scale=None, k_scale=None, v_scale=None, return_lse=False):
    """flash_attention_paged_prefill for a batch whose sequences share a prefix (a system prompt, a few-shot header): the
    shared keys are read once for the whole batch instead of once per sequence.  Not in the reference.

        q, k_cache, v_cache, cu_seqlens_q, max_seqlen_q, k_scale, v_scale as in flash_attention_paged_prefill;
        prefix_block_table [max_prefix_blocks] integer: the blocks that hold the shared prefix;
        prefix_len: its length in keys -- an int32 [1] tensor on the device (read and clamped there to what the table
          addresses; a graph replay sees its current value) or a Python int, which is wrapped;
        block_tables [batch, max_blocks]: each sequence's OWN blocks; context_lens [batch]: its OWN keys, INCLUDING the new
          tokens -- append them first (paged_kv_append).

    The keys of sequence b are the prefix followed by its own keys: token i (n_b new tokens, L_b own keys) sits at own
    position p = L_b - n_b + i, sees every prefix key and own key j iff j <= p.  A token with p < 0 gives zeros (lse -inf);
    rows that belong to no sequence are never written; prefix_len = 0 equals flash_attention_paged_prefill bit for bit.
    Three launches: the rows of all sequences packed into one dense problem per KV head against the prefix, split along the
    keys (planned from the prefix table's capacity -- size the table to the prefix); the paged prefill on the own keys; a
    merge (merge_attention_states' rule).  Returns [total_tokens, heads_q, head_dim], or (out, lse) with return_lse=True.
    Out of scope: a sliding window, head_dim 256, a backward pass.  Argument errors are ValueErrors raised before the device
    is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_cascade
    return paged_cascade(q, k_cache, v_cache, prefix_block_table, prefix_len, block_tables, context_lens, cu_seqlens_q,
                         max_seqlen_q=max_seqlen_q, scale=scale, k_scale=k_scale, v_scale=v_scale, return_lse=return_lse)


def flash_attention_mla_paged(q, kv_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, scale=None,
                              return_lse=False):
    """Paged multi-head LATENT attention (MLA, the DeepSeek-V2 / V3 / R1 family in its absorbed decode form): decode and short
    verify over a latent KV cache, without gathering the pages.  Not in the reference.  The contract is stated once, at
    aule_mla_paged_desc in include/aule.h; in short:

        q [total_tokens, heads_q, 576] fp16 / bf16: per head 512 compressed ("nope") dimensions, then 64 rotary ones; the token
          stride is free as in flash_attention_paged_prefill;
        kv_cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]) of q's dtype: ONE cache -- row pos of a
          sequence is the key of every query head (all 576 elements) and the value (elements 0..511); the kernel reads it
          from memory once for both products;
        block_tables [batch, max_blocks], context_lens [batch] (the keys INCLUDING the new tokens -- write them first, see
          below), cu_seqlens_q [batch + 1] int32 and max_seqlen_q as in flash_attention_paged_prefill, with the same
          device-side clamps, positions (token i of sequence b at p = L_b - n_b + i sees key j iff j <= p), zeros and
          lse = -inf for p < 0 or L_b = 0, and rows of no sequence never written;
        cu_seqlens_q=None is plain decode: sequence b owns row b, q.shape[0] == batch;
        max_seqlen_q=None with offsets given computes it with one device->host synchronisation; passing it keeps the call
          free of synchronisation and capturable into a graph (a replay reads the current cu_seqlens_q, context_lens and
          block_tables);
        scale=None is 1/sqrt(576), the library's rule -- DeepSeek models pass their own, 1/sqrt(192) * mscale (the softmax
          scale of the non-absorbed 128 + 64 head).

    Returns [total_tokens, heads_q, 512], or (out, lse) with return_lse=True: lse [total_tokens, heads_q] fp32, the natural
    log of the softmax denominator.  The keys of a sequence are split into ranges on the device from its own length (the
    number of ranges comes from the shape alone; partials are combined in a fixed order, so two runs give the same bits).
    mla_kv_append writes the new rows (one launch, with the rotation of the 64 rotary dimensions), with slots =
    paged_slot_mapping(block_tables, positions, block_size); an FP8 latent cache is flash_attention_mla_paged_fp8.  Out of
    scope: a sliding window, a backward pass; the non-absorbed 192 / 128 form of the prompt is flash_attention_mla_prefill.
    Argument errors are ValueErrors raised before the device is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_paged
    return mla_paged(q, kv_cache, block_tables, context_lens, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                     return_lse=return_lse)


def flash_attention_mla_paged_fp8(q, kv_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, scale=None,
                                  return_lse=False, kv_scale=None):
    """flash_attention_mla_paged over an FP8 latent cache: half the bytes per cached token, so twice the context or batch in
    the same memory.  The contract is aule_mla_paged_fp8_desc in include/aule.h; in short:

        kv_cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]) torch.float8_e4m3fn (OCP e4m3fn, the
          format gfx950 converts in hardware; e4m3fnuz, e5m2 and 16-bit caches are ValueErrors);
        kv_scale: ONE scale for the whole cache -- key = kv_scale * float(code row), value = its first 512 elements -- None
          (1.0), a float, or a 0-d / [1] tensor, which stays on the device (no device->host copy; a graph replay reads its
          current value).  quantize_mla_cache_fp8 makes (codes, scale) from a 16-bit cache; mla_kv_append writes the codes
          of new tokens;
        every other argument, the clamps, the rows that are written and the result: flash_attention_mla_paged.

    The codes are converted exactly to q's dtype inside the kernel and kv_scale multiplies the score scale and the fp32
    accumulators, never an element: with kv_scale = 1 the result equals flash_attention_mla_paged(q,
    kv_cache.to(q.dtype), ...) bit for bit.  lse includes kv_scale (the log of the denominator over the dequantised keys)."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_paged_fp8
    return mla_paged_fp8(q, kv_cache, block_tables, context_lens, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                         return_lse=return_lse, kv_scale=kv_scale)


def flash_attention_mla_paged_tree(q, kv_cache, tree_mask, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None,
                                   return_lse=False, kv_scale=None):
    """flash_attention_mla_paged / _fp8 for a TREE of new tokens per sequence instead of a chain: the verify step of tree drafters (MTP
    heads, EAGLE, Medusa) on the DeepSeek-V2 / V3 / R1 family, over the latent cache, in one call -- the latent is read once per
    sequence, not once per root-to-leaf path.  Not in the reference.  The contract is aule_mla_paged_tree_desc in include/aule.h; in short:

        kv_cache [num_blocks, block_size, 576] (or [num_blocks, block_size, 1, 576]): of q's dtype, or torch.float8_e4m3fn codes with
          kv_scale (None = 1.0, a float, or a 0-d / [1] tensor that stays on the device) -- the kind is read from kv_cache.dtype, and
          kv_scale with a 16-bit cache is a ValueError;
        tree_mask [total_tokens] int64, contiguous, on q's device, indexed by packed token: one 64-bit word per new token
          (tree_mask_from_parents builds them).  The kernel reads the words on every launch: no host copy, no synchronisation,
          capturable; a graph replay sees the current words;
        cu_seqlens_q [batch + 1] int32 is required (a tree of one node per sequence is the decode call);
        every other argument, the clamps, the rows that are written and the result: flash_attention_mla_paged.
    The rule is flash_attention_paged_prefill_tree's.  With L_b and n_b the clamped length and number of new tokens, a sequence with
    n_b <= 64 carries a tree (decided on the device): new token t is key L_b - n_b + t, and token i sees key j iff 0 <= j < L_b and
        j < L_b - n_b  (a context key)      or      bit j - (L_b - n_b) of tree_mask[s_b + i] is set.
    Any bit pattern is legal; a set bit at or beyond L_b is ignored; a token at a negative position (L_b < n_b) sees nothing; a row that
    sees no key gives out = 0 and lse = -inf.  A sequence with n_b > 64 (a prompt chunk in the same step) keeps the causal rule and its
    words are not read.  The chain words tree_mask[s_b + i] = (2 << i) - 1 give flash_attention_mla_paged's / _fp8's out and lse bit
    for bit (finite cached data).  Argument errors are ValueErrors raised before the device is touched; the only device->host
    synchronisation is max_seqlen_q=None's.
    Out of scope: more than 64 tree tokens per sequence, a window or sink logits (the MLA entries have neither), the cascade, any
    backward, and tree visibility inside mla_indexer: callers on DSA models filter the lists it emits by the tree themselves and
    pass them to flash_attention_mla_sparse."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_paged_tree
    return mla_paged_tree(q, kv_cache, _required_tree_mask(tree_mask), block_tables, context_lens, cu_seqlens_q, max_seqlen_q=max_seqlen_q,
                          scale=scale, return_lse=return_lse, kv_scale=kv_scale)


def flash_attention_mla_sparse(q, kv_cache, indices, scale=None, return_lse=False, kv_scale=None):
    """Sparse multi-head latent attention (DeepSeek-V3.2 "DSA" and its derivatives, absorbed form): every query token attends
    to the rows of the latent cache that ITS OWN list names -- what the model's indexer picked, typically 2048 keys -- in
    decode and in prefill.  The contract is stated once, at aule_mla_sparse_desc in include/aule.h; in short:

        q        [T, Hq, 576] fp16 / bf16, the last dimension contiguous; the token stride is free (a multiple of 8 elements,
                 at least Hq * 576: a slice of a wider projection is read in place), as in flash_attention_mla_paged
        kv_cache [num_blocks, block_size, 576] (or [..., 1, 576]), contiguous: q's dtype, or torch.float8_e4m3fn with kv_scale
                 (None = 1.0, a float, or a 0-d / [1] tensor that stays on the device) by flash_attention_mla_paged_fp8's rule;
                 a scale with a 16-bit cache is a ValueError.  The cache is addressed as a flat array of S = num_blocks *
                 block_size rows ("slots"), so a contiguous [L, 576] latent is the cache latent.view(L, 1, 576): sparse
                 prefill over an un-paged latent
        indices  [T, topk] (or [T, 1, topk]) int32, contiguous, on q's device, 1 <= topk <= 65536: indices[t, i] is a slot,
                 block * block_size + offset -- mla_kv_append's slot_mapping; from logical positions,
                 paged_slot_mapping(...).to(torch.int32).  Any other integer dtype is a ValueError (nothing is converted
                 silently)
        scale    None = 1/sqrt(576); DeepSeek models pass their own

    Token t, every head: the keys are the multiset { kv_cache.flat[indices[t, i]] : 0 <= indices[t, i] < S }.  Entries outside
    [0, S) are skipped (-1 is the conventional pad); a slot listed twice counts twice; there is NO causal rule -- the indexer
    is responsible for visibility.  scores = scale * q . key over 576 elements, values are the keys' first 512 elements.
    Returns out [T, Hq, 512], or (out, lse) with lse [T, Hq] fp32 (natural log of the denominator, kv_scale included); a
    token with no valid entry gives zeros and lse = -inf.  Every row of out / lse is written, and a cache row that no valid
    entry names is never read.  indices and a tensor kv_scale are read by the kernel on every launch: no host copy, no
    synchronisation, capturable, and a graph replay sees their current contents.  All argument errors are ValueErrors raised
    before the device is touched; CPU tensors that pass them are an AuleError; T = 0 returns empty tensors without a launch;
    tensors that require grad are refused.
    Out of scope: the indexer itself lives in aule.mla_indexer (its result is `indices`), a causal rule inside the kernel, packing several tokens' heads
    into one row block when Hq < 64, logical-position indices resolved through a block table inside the kernel, a backward,
    sink logits or tree masks with a list."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_sparse
    return mla_sparse(q, kv_cache, indices, scale=scale, return_lse=return_lse, kv_scale=kv_scale)


def mla_indexer_logits(q, weights, k_cache, block_tables, context_lens, cu_seqlens_q=None, max_seqlen_q=None, k_scale=None):
    """The index logits of the sparse MLA's indexer (DeepSeek-V3.2 "DSA"), with the head sum fused into the tile that made the
    scores:  logits[t, s] = sum_h weights[t, h] * relu(q[t, h, :] . k[s, :]).  The contract is stated once, at
    aule_mla_indexer_logits_desc in include/aule.h; in short:

        q        [T, H, 128] fp16 / bf16, 1 <= H <= 64, the last dimension contiguous; the token stride is free (a multiple of 8
                 elements, at least H * 128: a slice of a wider projection is read in place)
        weights  [T, H] fp32, contiguous: the caller folds H^-1/2, the softmax scale and any q scale into it
        k_cache  [num_blocks, block_size, 128] (or [..., 1, 128]), contiguous, one key row per position for all heads: q's dtype,
                 or torch.float8_e4m3fn codes with k_scale [num_blocks, block_size] fp32, one scale per row
                 (quantize_indexer_cache_fp8).  The scale multiplies the finished logit, never an element: with every scale 1
                 the FP8 call equals the 16-bit call on the converted codes bit for bit
        block_tables [batch, max_blocks], context_lens [batch], cu_seqlens_q [batch + 1]: int32, contiguous, on q's device, read
                 IN PLACE on every launch (nothing is converted: another dtype is a ValueError); the rules and device-side clamps
                 of flash_attention_mla_paged.  cu_seqlens_q = None is plain decode (sequence b owns row b, T == batch)
        max_seqlen_q  None = T with offsets (no synchronisation; it only sizes the grid and caps every sequence's new tokens)

    Token i of sequence b sits at position p = L_b - n_b + i and sees key j iff 0 <= j <= p.  Returns logits [T, W] fp32 with
    W = max_blocks * block_size: for a row that belongs to a sequence every column is written, the logit where the key is visible
    and -inf elsewhere; rows of no sequence are never written (torch.empty).  A cache row no token sees is never read.  Memory:
    T * W * 4 bytes -- 1 GB at 2048 tokens x 128 K columns: chunk T or size the table.  No host synchronisation, capturable, two
    runs are bit-identical.  All argument errors are ValueErrors raised before the device is touched; CPU tensors that pass
    them are an AuleError; tensors that require grad are refused.
    Out of scope: FP8 queries and FP8 MFMAs, a fused streaming top-k that never writes [T, W], an append kernel for the index
    keys, H > 64, a backward."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_indexer_logits as impl
    return impl(q, weights, k_cache, block_tables, context_lens, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, k_scale=k_scale)


def mla_indexer_topk(logits, topk, block_tables, context_lens, block_size, cu_seqlens_q=None, max_seqlen_q=None, output="slots"):
    """The per-token key lists of the sparse MLA's indexer from ANY fp32 logits [T, max_blocks * block_size] (row stride free).  The
    contract is stated once, at aule_mla_indexer_topk_desc in include/aule.h; in short: visibility comes from the positions
    (key j iff 0 <= j <= p, the arithmetic of mla_indexer_logits), not from -inf marks; among token t's visible keys the order
    is logit descending by numeric value (-0 == +0, a NaN ranks as -inf), then position ascending; the first min(topk, p + 1)
    are emitted in ASCENDING position order and the tail is -1; a token with p < 0 gets all -1; rows of no sequence are never
    written.  1 <= topk <= 65536.  output "slots": block_tables[b][pos // block_size] * block_size + pos % block_size, what
    flash_attention_mla_sparse consumes when the latent cache shares the table and the block size; "positions": the raw
    positions (map them with paged_slot_mapping for a latent cache of another block size).  Returns indices [T, topk] int32.
    Deterministic, no synchronisation, capturable.  Tables as in mla_indexer_logits: int32, contiguous, read in place.  All
    argument errors are ValueErrors raised before the device is touched; CPU tensors that pass them are an AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_indexer_topk as impl
    return impl(logits, topk, block_tables, context_lens, block_size, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, output=output)


def mla_indexer(q, weights, k_cache, block_tables, context_lens, topk, cu_seqlens_q=None, max_seqlen_q=None, k_scale=None, output="slots",
                return_logits=False):
    """The sparse MLA's indexer: mla_indexer_logits, then mla_indexer_topk on its result -- two launches in a row.  Returns
    indices [T, topk] int32 (or (indices, logits) with return_logits), which go straight into
    flash_attention_mla_sparse(q_latent, kv_cache, indices) when the latent cache shares block_tables and the block size."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_indexer as impl
    return impl(q, weights, k_cache, block_tables, context_lens, topk, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=max_seqlen_q, k_scale=k_scale,
                output=output, return_logits=return_logits)


def quantize_indexer_cache_fp8(k_cache):
    """(codes, k_scale) for mla_indexer_logits' FP8 cache: float8_e4m3fn codes of an index key cache [num_blocks, block_size, 128]
    and one scale per row, k_scale [num_blocks, block_size] fp32 = the row's amax / 448 (1.0 for an all-zero row), saturating.
    Plain torch ops; works on CPU tensors."""
    from ._torch import quantize_indexer_cache_fp8 as impl
    return impl(k_cache)


def mla_kv_append(c_kv, k_pe, kv_cache, slot_mapping, kv_scale=None, cos=None, sin=None, positions=None, rope_layout="half"):
    """The write side of the paged MLA's latent cache: put the rows [c_kv[t] | rope(k_pe[t])] of T new tokens into the cache
    flash_attention_mla_paged / _fp8 read, in place, with one launch; returns None.

        c_kv [T, 512], k_pe [T, 64] (or [T, 1, 64]) fp16 / bf16 (last dimension contiguous, token strides free multiples of
          8 elements: slices of the fused down-projection are read in place);
        kv_cache [num_blocks, block_size, 576] (or [..., 1, 576]) contiguous, c_kv's dtype (a copy of the bits) or
          torch.float8_e4m3fn (code = cast(clamp(x / kv_scale, -448, 448)) -- quantize_mla_cache_fp8 with a given scale, bit
          for bit; kv_scale None (1.0), a float, or a 0-d / [1] tensor that stays on the device);
        slot_mapping [T] integer = block * block_size + offset (see paged_slot_mapping); negative or past the cache: the
          token is skipped entirely; two tokens with the same slot in one call: which one wins is unspecified;
        cos, sin [table_len, 32], positions [T] (all or none): rotate k_pe by table row positions[t] first, rope_layout
          "half" (pairs (p, p + 32)) or "interleaved" (pairs (2p, 2p + 1), the layout of DeepSeek checkpoints); rounded to
          the input's dtype, then quantised: bit-identical to the rotation pass followed by the plain append.  A position
          outside the table skips the token entirely.

    Argument errors are ValueErrors raised before the device is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_kv_append as impl
    return impl(c_kv, k_pe, kv_cache, slot_mapping, kv_scale=kv_scale, cos=cos, sin=sin, positions=positions, rope_layout=rope_layout)


def quantize_mla_cache_fp8(kv_cache):
    """(codes, scale) for flash_attention_mla_paged_fp8: float8_e4m3fn codes of a latent cache and ONE scale, a [1] fp32 tensor
    = amax / 448 (1.0 for an all-zero cache), saturating -- quantize_kv_cache_fp8's formula with one head.  Plain torch ops;
    works on CPU tensors."""
    from ._torch import quantize_mla_cache_fp8 as impl
    return impl(kv_cache)


def flash_attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True, scale=None,
                           window_size=-1, return_lse=False):
    """Attention over a batch of sequences of DIFFERENT lengths packed along one token axis, forward and backward (autograd-aware):
    SFT with sequence packing, encoder batches without padding, prefill without a paged cache -- flash_attn_varlen_func's case.
    Not in the reference.

        q [total_q, heads_q, head_dim], k, v [total_k, heads_kv, head_dim] fp16 / bf16 ROCm tensors, heads_q % heads_kv == 0.
          The heads of a token contiguous, the token stride free as long as it and the storage offset are multiples of 8
          elements: the three slices of a fused [T, heads_q + 2 heads_kv, head_dim] projection are read in place.
        cu_seqlens_q, cu_seqlens_k [batch + 1] int32: sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1 of q and
          rows cu_seqlens_k[b] .. cu_seqlens_k[b + 1] - 1 of k / v.  They are read and clamped on the device (offsets to the
          totals, lengths to the maxima): a stale value cannot index outside a buffer.
        max_seqlen_q, max_seqlen_k: the largest number of query / key tokens of a sequence (they size the grids; a longer
          sequence is cut to its first max_seqlen_* tokens).  None reads it from the offsets with ONE device->host
          synchronisation; passing both keeps the call free of synchronisation and capturable into a graph.
        causal: False, True (top-left: token i sees keys j <= i) or "bottom-right" (token i of a sequence with n queries and L
          keys sits at position i + L - n; L < n is allowed, tokens at negative positions see nothing), as flash_attention.
        window_size: W > 0 keeps the keys j with position - j < W.

    head_dim 32, 64 and 128 run as they are; other head dims up to 128 are zero-padded as flash_attention does.  A token that
    sees no key gives a row of zeros (lse -inf, zero gradient).  Rows that belong to no sequence are never written: out (and
    lse) come from torch.empty; the gradients are zero there.  Returns [total_q, heads_q, head_dim], or (out, lse) with
    return_lse=True: lse [total_q, heads_q] fp32, the natural log of the softmax denominator.  Not built: head_dim > 128 and
    fp32 (ValueError).  All argument errors are ValueErrors raised before the device is touched; CPU tensors that pass them
    raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import flash_attention_varlen as impl
    return impl(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=max_seqlen_q, max_seqlen_k=max_seqlen_k, causal=causal,
                scale=scale, window_size=window_size, return_lse=return_lse)


def flash_attention_varlen_sinks(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True,
                                 scale=None, window_size=-1, return_lse=False):
    """flash_attention_varlen for models with learned ATTENTION SINKS (gpt-oss and its derivatives): every query head carries one logit
    that joins the softmax denominator and contributes no value.  Autograd-aware over q, k, v and sinks.  Not in the reference.

        sinks [heads_q], fp32 or q's dtype, on q's device: a raw logit, multiplied by neither scale nor k_scale.  The kernels read it
          on every launch (nothing copies it to the host: capturable, and a replay sees its current contents).
        every other argument, check, stride rule and the head-dim padding as flash_attention_varlen.

    For a query row of head h with visible keys j and scaled scores s_j:
        Z = sum_j exp(s_j) + exp(sinks[h])      out = sum_j exp(s_j) v_j / Z      lse = ln Z
    A row that sees no key gives out = 0 and lse = sinks[h].  sinks[h] = -inf means "no sink": that head's out and lse equal
    flash_attention_varlen's bit for bit.  NaN or +inf logits give unspecified values for their head only.  The gradient of sinks
    (in sinks' dtype) is -sum over the owned rows of exp(sinks[h] - lse) rowsum(dout * out): no atomics, the same bits on every run."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import flash_attention_varlen_sinks as impl
    return impl(q, k, v, sinks, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=max_seqlen_q, max_seqlen_k=max_seqlen_k, causal=causal,
                scale=scale, window_size=window_size, return_lse=return_lse)


def flash_attention_paged_prefill_sinks(q, k_cache, v_cache, sinks, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None,
                                        window_size=-1, k_scale=None, v_scale=None, return_lse=False):
    """flash_attention_paged_prefill with per-head sink logits (flash_attention_varlen_sinks states the definition): sinks [heads_q], fp32
    or q's dtype, on q's device; every other argument and rule as flash_attention_paged_prefill, k_scale of an FP8 cache in the
    scores and not in the sink.  A token that sees no key gives zeros and lse = sinks[h]; sinks[h] = -inf equals the sinkless call
    bit for bit.  Forward only."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_prefill
    return paged_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                         window_size=window_size, k_scale=k_scale, v_scale=v_scale, return_lse=return_lse, sinks=_required_sinks(sinks))


def flash_attention_paged_query_sinks(q, k_cache, v_cache, sinks, block_tables, context_lens, scale=None, window_size=-1, k_scale=None,
                                      v_scale=None, return_lse=False):
    """flash_attention_paged_query with per-head sink logits (flash_attention_varlen_sinks states the definition): sinks [heads_q], fp32
    or q's dtype, on q's device; every other argument and rule as flash_attention_paged_query.  seq_q = 1 is the decode step.  The
    sink joins the merge of the key-range partials as one more partial.  A query that sees no key gives zeros and lse = sinks[h];
    sinks[h] = -inf equals the sinkless call bit for bit.  Forward only."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_query
    return paged_query(q, k_cache, v_cache, block_tables, context_lens, scale=scale, window_size=window_size, k_scale=k_scale,
                       v_scale=v_scale, return_lse=return_lse, sinks=_required_sinks(sinks))


def flash_attention_paged_query_tree(q, k_cache, v_cache, tree_mask, block_tables, context_lens, scale=None, k_scale=None, v_scale=None,
                                     return_lse=False):
    """flash_attention_paged_query for a TREE of new tokens instead of a chain: the verify step of tree drafters (EAGLE, Medusa, SpecInfer).
    All seq_q nodes are appended to the cache and verified in one call; a node sees the cached context and its ancestors, not its siblings
    or cousins.  Not in the reference.

        tree_mask [batch, seq_q] int64, contiguous, on q's device: one 64-bit word per new token (tree_mask_from_parents builds them).
        The kernel reads the words on every launch: no host copy, no synchronisation, capturable; a graph replay sees the current words.
        every other argument: as flash_attention_paged_query (16-bit or float8_e4m3fn caches); there is no window_size.
    With L_b the clamped length and n = seq_q, new token t is key L_b - n + t.  Query i sees key j iff 0 <= j < L_b and
        j < L_b - n  (a context key)      or      bit j - (L_b - n) of tree_mask[b, i] is set.
    Any bit pattern is legal: no self bit is implied and no topological order required; bits at or above n and bits that name a key below
    0 are ignored.  A query at a negative position gives a row of zeros; a row that sees no key gives out = 0 and lse = -inf.  The chain
    words tree_mask[b, i] = (2 << i) - 1 give flash_attention_paged_query's out and lse bit for bit (finite cached data).  Wrong dtype,
    shape, device or a non-contiguous tree_mask raise ValueError before any launch.
    Out of scope: sliding windows over a tree, sink logits together with a tree, the cascade, head_dim 256, more than 64 tree tokens per
    sequence, any backward.  A tree over the latent cache of the MLA models is flash_attention_mla_paged_tree."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_query
    return paged_query(q, k_cache, v_cache, block_tables, context_lens, scale=scale, k_scale=k_scale, v_scale=v_scale, return_lse=return_lse,
                       tree_mask=_required_tree_mask(tree_mask))


def flash_attention_paged_prefill_tree(q, k_cache, v_cache, tree_mask, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=None, scale=None,
                                       k_scale=None, v_scale=None, return_lse=False):
    """flash_attention_paged_prefill with tree masks (flash_attention_paged_query_tree states the rule): tree_mask [total_tokens] int64,
    contiguous, on q's device, indexed by packed token.  A sequence whose clamped number of new tokens n_b is at most 64 carries a tree --
    decided on the device -- and token i of it reads the word of row s_b + i; a longer sequence (a prompt chunk in the same step) keeps the
    causal rule of flash_attention_paged_prefill and its words are not read.  Every other argument and rule as
    flash_attention_paged_prefill; there is no window_size.  Chain words give that call's out and lse bit for bit.
    Out of scope: sliding windows over a tree, sink logits together with a tree, the cascade, head_dim 256, more than 64 tree tokens per
    sequence, any backward.  A tree over the latent cache of the MLA models is flash_attention_mla_paged_tree."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_prefill
    return paged_prefill(q, k_cache, v_cache, block_tables, context_lens, cu_seqlens_q, max_seqlen_q=max_seqlen_q, scale=scale,
                         k_scale=k_scale, v_scale=v_scale, return_lse=return_lse, tree_mask=_required_tree_mask(tree_mask))


def tree_mask_from_parents(parents):
    """The words of flash_attention_paged_query_tree / flash_attention_paged_prefill_tree for a tree given by parent indices.

        parents [seq_q] or [batch, seq_q], any integer dtype, seq_q <= 64: parents[i] is the index of token i's parent among the new
        tokens; anything outside [0, i) means "child of the context" (a root of the draft).
    Returns int64 words of parents' shape with the self bit and all ancestor bits set; a chain (parents[i] = i - 1) gives (2 << i) - 1.
    Torch ops only, on parents' device, no host synchronisation; works on CPU tensors."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import tree_mask_from_parents as impl
    return impl(parents)


def _required_tree_mask(tree_mask):
    if tree_mask is None:
        raise ValueError("tree_mask must be an int64 tensor (the call without a tree: flash_attention_paged_query / flash_attention_paged_prefill / "
                         "flash_attention_mla_paged)")
    return tree_mask


def _required_sinks(sinks):
    if sinks is None:
        raise ValueError("sinks must be a [heads_q] tensor (the sinkless call: flash_attention_paged_prefill / flash_attention_paged_query)")
    return sinks


def flash_attention_mla_prefill(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True,
                                scale=None, return_lse=False):
    """MLA prefill: multi-head latent attention (DeepSeek-V2 / V3 / R1) in its NON-ABSORBED form, the form the prompt runs in, over
    a batch of sequences of different lengths packed along one token axis.  Forward only.  Not in the reference.  The contract is
    stated once, at aule_mla_prefill_desc in include/aule.h; in short:

        q [total_q, heads, 192] (q_nope | q_pe), k_nope and v [total_k, heads, 128], k_pe [total_k, 64] (or [total_k, 1, 64]),
          fp16 / bf16 ROCm tensors of one dtype: key row j of head h is [k_nope[j, h] | k_pe[j]], the rotated k_pe shared by all
          heads and never copied per head.  192 / 128 / 64 exactly: nothing is padded.
        k_nope and v carry their own token AND head strides, k_pe and q their own token stride: the two halves of a
          [total_k, heads, 256] kv_b output and columns 512.. of a [total_k, 576] down-projection are read in place.  A tensor
          whose innermost stride is not 1, or whose strides or storage offset are not multiples of 8 elements, is copied.
        cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal (False, True = top-left, "bottom-right"): as
          flash_attention_varlen, with the same device-side clamps and cuts; "bottom-right" with more keys than queries is
          chunked prefill.  There is no window.
        scale=None is 1/sqrt(192); models with a YaRN mscale pass their own.

    Returns [total_q, heads, 128], or (out, lse) with return_lse=True: lse [total_q, heads] fp32, the natural log of the softmax
    denominator -- two calls over disjoint key chunks are combined by merge_attention_states.  A token that sees no key gives
    zeros and lse = -inf; rows that belong to no sequence are never written (out and lse come from torch.empty).  One launch, no
    workspace; with both maxima given there is no synchronisation and the call captures into a graph.  No autograd: inputs that
    require grad are refused (ValueError).  Out of scope: a backward, a window, GQA, FP8 inputs, fused rotation.  Argument errors
    are ValueErrors raised before the device is touched; CPU tensors that pass them raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import mla_prefill
    return mla_prefill(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=max_seqlen_q, max_seqlen_k=max_seqlen_k,
                       causal=causal, scale=scale, return_lse=return_lse)


def flash_attention_mla_varlen(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=None, max_seqlen_k=None, causal=True,
                               scale=None, return_lse=False):
    """MLA 192 / 128 attention over a variable-length packed batch WITH autograd: flash_attention_mla_prefill for training and
    fine-tuning with sequence packing.  Not in the reference.  The arguments, their checks and the in-place rules are
    flash_attention_mla_prefill's, and the forward is the same launch: out and lse are bit-identical to that entry's.  The backward's
    contract is stated once, at aule_mla_prefill_bwd_desc in include/aule.h; in short:

        dq like q; dk_nope and dv are the two halves of ONE [total_k, heads, 256] buffer, written in place by the kernels (so the
          gradient of a fused kv_b output needs no concatenation); dk_pe -- the sum over the heads, accumulated in fp32 and
          rounded once -- in the shape k_pe was given, [total_k, 64] or [total_k, 1, 64].
        Rows that belong to no sequence are zero; a query that sees no key has dq = 0; a key that no query sees has zero gradients.
        Deterministic: no floating-point atomics, two runs agree bit for bit.
        Three or four launches (delta, dQ, dK/dV over head chunks, and the dk_pe reduce when the heads are cut into more than one
          chunk) on the current stream; with both maxima given there is no synchronisation.

    Returns [total_q, heads, 128], or (out, lse) with return_lse=True; lse is not differentiable.  Argument errors are ValueErrors
    raised before the device is touched; CPU tensors that pass them raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import flash_attention_mla_varlen as impl
    return impl(q, k_nope, k_pe, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q=max_seqlen_q, max_seqlen_k=max_seqlen_k, causal=causal,
                scale=scale, return_lse=return_lse)


def merge_attention_states(out_a, lse_a, out_b, lse_b):
    """Merge two attention states of the same queries over DISJOINT key sets into the state over their union: the step that
    combines partial results (a shared prefix and a private suffix, key ranges computed apart).  Not in the reference.

        out_a, out_b [..., heads, head_dim] fp16 / bf16; lse_a, lse_b [..., heads] fp32 -- the (out, lse) pairs that
        flash_attention_paged_query / _prefill / _cascade return with return_lse=True.

    out = (w_a out_a + w_b out_b) / (w_a + w_b) and lse = M + log(w_a + w_b), with M = max(lse_a, lse_b) and
    w_x = exp(lse_x - M).  A side with lse = -inf holds no key: the other side comes back bit for bit; both: zeros and -inf.
    The order of the pair does not change the bits.  Returns (out, lse).  Argument errors are ValueErrors raised before the
    device is touched; CPU tensors raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import merge_states
    return merge_states(out_a, lse_a, out_b, lse_b)


def quantize_kv_cache_fp8(cache, per_head=True):
    """(cache_fp8, scale) for the FP8 paged decode: float8_e4m3fn codes and a [heads_kv] fp32 scale = amax / 448 per KV
    head (per_head=False: one value, repeated), saturating.  Plain torch ops; works on CPU tensors."""
    from ._torch import quantize_kv_cache_fp8 as impl
    return impl(cache, per_head=per_head)


flash_attention_paged = flash_attention_paged_amd


def paged_kv_append(key, value, k_cache, v_cache, slot_mapping, k_scale=None, v_scale=None, cos=None, sin=None, positions=None):
    """The write side of the paged KV cache: put the K and V rows of T new tokens into the caches flash_attention_paged_amd
    reads, in place, with one launch; returns None.

        key, value [T, heads_kv, head_dim] fp16 / bf16 (last dimension contiguous, other strides free);
        k_cache, v_cache [num_blocks, block_size, heads_kv, head_dim] contiguous, key's dtype or both torch.float8_e4m3fn;
        slot_mapping [T] integer = block * block_size + offset (see paged_slot_mapping); negative or past the cache: skipped;
        two tokens with the same slot in one call: which one wins is unspecified.

    FP8 caches: code = cast(clamp(x / scale[hk], -448, 448)) -- quantize_kv_cache_fp8 with given scales, bit for bit --
    k_scale / v_scale each None (1.0), a float, a 0-d tensor or a [heads_kv] tensor.  cos, sin, positions: rotate K (not V)
    by table row positions[t] first (half-split pairs; rounded to key's dtype, then quantised: bit-identical to the rotation
    pass followed by the plain append).  Argument errors are ValueErrors raised before the device is touched; CPU tensors
    raise AuleError."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    from ._torch import paged_kv_append as impl
    return impl(key, value, k_cache, v_cache, slot_mapping, k_scale=k_scale, v_scale=v_scale, cos=cos, sin=sin,
                positions=positions)


def paged_slot_mapping(block_tables, positions, block_size, seq_ids=None):
    """slots[t] = block_tables[seq_ids[t], positions[t] // block_size] * block_size + positions[t] % block_size (int64) for
    paged_kv_append; seq_ids defaults to arange(T), the decode case; negative positions give -1.  Plain torch; works on CPU."""
    from ._torch import paged_slot_mapping as impl
    return impl(block_tables, positions, block_size, seq_ids=seq_ids)


# =============================================================================
# RoPE (reference python/aule/triton_flash.py:561-703, exported at __init__.py:72-75)
# =============================================================================
def flash_attention_rope(q, k, v, cos, sin, causal=True, scale=None, window_size=-1):
    """RoPE + FlashAttention-2; same name, arguments and result as the reference's export
    (triton_flash.py:561-603): half-split pairs, x_rot = x * cos + rotate_half(x) * sin, query i at table row i,
    key j at row j; cos / sin [seq_len, head_dim // 2] or [1, seq_len, head_dim // 2].

    On MI355X K is rotated by one HBM-streaming pass (csrc/rope_gfx950.hip) -- once per key, not once per Q block.  Q is
    rotated by the same pass when gradients are needed (the backward kernels read the rotated Q, and return the true
    gradients, rotated back -- the reference's backward does not) and inside the forward kernel, on its way into the
    registers, otherwise (bit-identical, one read and one write of Q less: DESIGN.md 3.6).  ROCm tensors; autograd-aware."""
    try:
        import torch  # noqa: F401
    except ImportError as e:
        raise AuleError("aule (HIP build) needs PyTorch-ROCm for device memory") from e
    _validate(q, k, v)
    if cos is None or sin is None:
        raise ValueError("cos and sin are required for RoPE")
    if not (q.is_cuda and k.is_cuda and v.is_cuda):
        raise AuleError("aule (HIP build): flash_attention_rope needs ROCm device tensors; there is no CPU fallback")
    window = int(window_size) if window_size is not None and window_size > 0 else -1
    from ._torch import flash_attention_rope_hip
    return flash_attention_rope_hip(q, k, v, cos, sin, causal=causal, scale=scale, window=window, layout="half")


def precompute_rope_frequencies(seq_len, head_dim, base=10000.0, device="cuda", dtype=None):
    """cos, sin [seq_len, head_dim // 2]: theta_p = base^(-p / (head_dim/2)), angle = position * theta_p
    (same signature and values as triton_flash.py:644-677)."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    half_dim = head_dim // 2
    freqs = 1.0 / (base ** (torch.arange(0, half_dim, device=device, dtype=dtype) / half_dim))
    angles = torch.arange(seq_len, device=device, dtype=dtype)[:, None] * freqs[None, :]
    return torch.cos(angles), torch.sin(angles)


def apply_rope_separate(q, k, cos, sin):
    """The rotation alone, (q_rot, k_rot), half-split pairs (triton_flash.py:680-703: the table is cut to
    q's sequence length and applied to both).  ROCm tensors run the HIP rotation pass."""
    if not (q.is_cuda and k.is_cuda):
        raise AuleError("aule (HIP build): apply_rope_separate needs ROCm device tensors; there is no CPU fallback")
    from ._torch import _rope_tables, rope_raw
    if k.shape[2] != q.shape[2]:
        raise ValueError(f"apply_rope_separate needs equal sequence lengths, got {q.shape[2]} and {k.shape[2]}")
    c, s = _rope_tables(cos, sin, q.shape[-1], q.device)
    return rope_raw(q.contiguous(), c, s, "half"), rope_raw(k.contiguous(), c, s, "half")


# =============================================================================
# PyTorch SDPA compatibility layer (reference __init__.py:288-442)
# =============================================================================
_original_sdpa = None
_installed = False
_SDPA_DTYPES = ("torch.float16", "torch.bfloat16", "torch.float32")


def scaled_dot_product_attention(query, key, value, attn_mask=None, dropout_p=0.0, is_causal=False,
                                 scale=None, enable_gqa=False):
    """Drop-in for torch.nn.functional.scaled_dot_product_attention (same signature as the reference's
    shim, __init__.py:288-297).  Runs the HIP kernels when it can and defers to PyTorch's own SDPA for
    what the kernels do not cover or run slower: attn_mask, dropout, head_dim > 256 or strictly between 128 and 256 (those run
    zero-padded to 256 here and measured slower than PyTorch's own SDPA: tools/d256_bench.py), non-4-D or non-ROCm tensors,
    dtypes other than fp16/bf16/fp32, and mismatched head counts without enable_gqa (PyTorch raises).
    torch's is_causal mask is top-left aligned, like this library's."""
    import torch
    import torch.nn.functional as F
    fallback = (
        attn_mask is not None or dropout_p > 0.0
        or not (isinstance(query, torch.Tensor) and query.is_cuda and key.is_cuda and value.is_cuda)
        or query.dim() != 4 or key.dim() != 4 or value.dim() != 4
        or (128 < query.shape[-1] < 256) or query.shape[-1] > 256 or key.shape[-1] != query.shape[-1] or value.shape[-1] != query.shape[-1]
        or str(query.dtype) not in _SDPA_DTYPES
        or (query.shape[1] != key.shape[1] and not enable_gqa)
        or key.shape[1] == 0 or query.shape[1] % max(1, key.shape[1]) != 0
        or key.shape[2] == 0
    )
    if fallback:
        fn = _original_sdpa if _original_sdpa is not None else F.scaled_dot_product_attention
        if fn is scaled_dot_product_attention:   # installed without a saved original: cannot recurse
            raise AuleError("scaled_dot_product_attention fallback requested but the original SDPA is unavailable")
        return fn(query, key, value, attn_mask=attn_mask, dropout_p=dropout_p, is_causal=is_causal,
                  scale=scale, enable_gqa=enable_gqa)
    return flash_attention(query, key, value, causal=is_causal, scale=scale)


def install(backend=None, verbose=False):
    """Route every torch.nn.functional.scaled_dot_product_attention call through this library
    (reference __init__.py:353-406).  `backend` may be None or 'hip' (the only backend of this build)."""
    global _original_sdpa, _installed, _verbose
    import torch
    import torch.nn.functional as F
    if backend is not None and backend != "hip":
        raise ValueError(f"Invalid backend '{backend}'. This build has one backend: 'hip' (or None)")
    _verbose = bool(verbose)
    if _installed:
        print(f"aule-attention: Updated (backend=hip, verbose={verbose})")
        return
    _original_sdpa = F.scaled_dot_product_attention
    F.scaled_dot_product_attention = scaled_dot_product_attention
    torch.nn.functional.scaled_dot_product_attention = scaled_dot_product_attention
    _installed = True
    print("aule-attention: Installed (HIP gfx950%s)" % (", verbose" if verbose else ""))


def uninstall():
    """Restore PyTorch's own SDPA (reference __init__.py:409-430)."""
    global _installed
    if not _installed:
        print("aule-attention: Not installed")
        return
    import torch
    import torch.nn.functional as F
    if _original_sdpa is not None:
        F.scaled_dot_product_attention = _original_sdpa
        torch.nn.functional.scaled_dot_product_attention = _original_sdpa
    _installed = False
    print("aule-attention: Uninstalled, restored PyTorch SDPA")


def get_available_backends():
    """Reference API (__init__.py:445-457); this build has exactly one backend."""
    from . import _capi
    try:
        _capi.get_lib()
        return ["hip"]
    except AuleError:
        return []


def get_backend_errors():
    from . import _capi
    try:
        _capi.get_lib()
        return {}
    except AuleError as e:
        return {"hip": str(e)}


def get_backend_info():
    from . import _capi
    info = {"backends": get_available_backends(), "version": __version__}
    if info["backends"]:
        from .hip import Aule
        info["hip"] = Aule().get_device_info()
        info["library"] = _capi.library_path()
    return info


def print_backend_info():
    """Backend status report (reference: python/aule/__init__.py:516-562); this build lists its one backend, the library it
    loaded and the device the C-ABI reports."""
    print("=" * 60)
    print("AULE-ATTENTION v" + __version__)
    print("=" * 60)
    print()
    backends = get_available_backends()
    print(f"Available backends: {backends}")
    print()
    if backends:
        info = get_backend_info()
        dev = info.get("hip", {})
        print("[1] HIP (gfx950 / MI355X, hand-written kernels behind libaule.so)")
        print(f"    GPU: {dev.get('device_name', 'Unknown')}")
        print(f"    Library: {info.get('library')}")
        print("    Status: FlashAttention-2 forward / backward, fp32 / fp16 / bf16")
        print()
    for name, err in get_backend_errors().items():
        print(f"[-] {name.upper()}: unavailable -- {err}")
        print()
    print("=" * 60)


def set_verbose(flag=True):
    global _verbose
    _verbose = bool(flag)


def __getattr__(name):
    # Aule / GpuTensor: the C-ABI consumer classes of the reference's vulkan.py, exported at package level like the reference does
    # (python/aule/__init__.py:565-592).  Resolved lazily: importing them loads libaule.so, which needs a HIP device.
    if name in ("Aule", "GpuTensor"):
        from . import hip
        return getattr(hip, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["flash_attention", "attention", "flash_attention_paged_amd", "flash_attention_paged", "flash_attention_paged_query", "flash_attention_paged_prefill", "flash_attention_paged_prefill_fp8mma", "quantize_rows_fp8", "flash_attention_paged_cascade", "flash_attention_mla_paged", "flash_attention_mla_paged_fp8", "flash_attention_mla_paged_tree", "flash_attention_mla_sparse", "mla_indexer_logits", "mla_indexer_topk", "mla_indexer", "quantize_indexer_cache_fp8", "mla_kv_append", "quantize_mla_cache_fp8", "flash_attention_varlen", "flash_attention_varlen_sinks", "flash_attention_paged_prefill_sinks", "flash_attention_paged_query_sinks", "flash_attention_paged_query_tree", "flash_attention_paged_prefill_tree", "tree_mask_from_parents", "flash_attention_mla_prefill", "flash_attention_mla_varlen", "merge_attention_states", "quantize_kv_cache_fp8", "paged_kv_append", "paged_slot_mapping",
           "flash_attention_rope", "precompute_rope_frequencies", "apply_rope_separate", "AuleError", "scaled_dot_product_attention", "install", "uninstall",
           "get_available_backends", "get_backend_errors", "get_backend_info", "print_backend_info", "Aule", "GpuTensor", "set_verbose",
           "__version__"]
