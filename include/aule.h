/*
 * include/aule.h -- C-ABI of libaule.so (MI355X / gfx950 HIP build).
 *
 * Drop-in boundary for the FlashAttention forward/backward hot path of
 * AuleTechnologies/Aule-Attention.  Every legacy symbol below has the exact
 * name, argument order, scalar widths and return-code convention of the
 * reference export it replaces (reference file:line cited per symbol; the
 * authoritative consumer-side declarations are the ctypes signatures in
 * python/aule/vulkan.py:224-406).  The "_ex" entry points at the bottom are
 * ADDITIVE: they carry what the legacy ABI cannot express (bf16/fp16 storage,
 * GQA/MQA, Sq != Sk, user scale, device pointers, streams).
 *
 * Calling convention: C.  No torch / C++ types cross this boundary.
 * Errors: negative int32 return + text from aule_get_error().
 * Threading: all entry points are serialised by one internal mutex (superset of
 * the reference contract, which has no locking: src/lib.zig:12-22).
 * Legacy compute calls are synchronous (device idle on return), like the
 * reference (src/attention_pipeline.zig:389-390, src/attention_gpu.zig:467-468).
 * "_ex" calls are asynchronous on the caller's HIP stream.
 */
#ifndef AULE_H
#define AULE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AULE_MAX_TENSORS 1024u /* src/lib.zig:17 MAX_TENSORS */

/* ---- lifecycle / info ---------------------------------------------------- */
int32_t aule_init(void);                     /* src/lib.zig:59   0 ok (idempotent), -1 + error text */
void aule_shutdown(void);                    /* src/lib.zig:105  destroys all tensors + context */
const char* aule_get_error(void);            /* src/lib.zig:124  static 512-B buffer, "No error" if none */
const char* aule_get_backend_name(void);     /* src/lib.zig:133  "HIP/ROCm" | "Not initialized" (backend.zig:496-502) */
int32_t aule_get_vendor(void);               /* src/lib.zig:144  1 = amd; -1 uninitialised */
int32_t aule_get_gpu_vendor(void);           /* src/lib.zig:274  same table */
int32_t aule_is_amd_optimized(void);         /* src/lib.zig:168  1 / -1 */
int32_t aule_has_fp16(void);                 /* src/lib.zig:184  1 / -1 */
int32_t aule_get_subgroup_size(void);        /* src/lib.zig:296  64 (wavefront) / -1 */
int32_t aule_get_device_name(uint8_t* buffer, uint32_t buffer_len); /* src/lib.zig:242 bytes copied (NUL-terminated, truncated) / -1 */
int32_t aule_set_shader_variant(uint8_t variant); /* src/lib.zig:202  0, -1 uninit, -2 unavailable (only variant 0 exists here) */
int32_t aule_get_shader_variant(void);            /* src/lib.zig:215 */
int32_t aule_has_shader_variant(uint8_t variant); /* src/lib.zig:226  1/0/-1 */
int32_t aule_supports_backward(void);        /* src/lib.zig:96   1 */

/* ---- host-pointer forward (MHA, Sq == Sk, fp32, scale = 1/sqrt(D)) -------- */
/* src/lib.zig:312-367.  0; -1 uninit; -2 alloc; -3 upload; -4 compute; -5 download */
int32_t aule_attention_forward(const float* query, const float* key, const float* value, float* output,
                               uint32_t batch_size, uint32_t num_heads, uint32_t seq_len,
                               uint32_t head_dim, int32_t causal);

/* ---- persistent device tensors (1-based slot handles, 0 = failure) -------- */
typedef uint64_t aule_tensor_handle;
aule_tensor_handle aule_tensor_create(uint32_t batch_size, uint32_t num_heads, uint32_t seq_len,
                                      uint32_t head_dim);      /* src/lib.zig:409 */
aule_tensor_handle aule_tensor_create_u32(uint32_t batch_size, uint32_t num_heads, uint32_t seq_len,
                                          uint32_t head_dim);  /* src/lib.zig:432 (aliases fp32 storage) */
void aule_tensor_destroy(aule_tensor_handle handle);           /* src/lib.zig:444 ignores 0 / out of range */
int32_t aule_tensor_upload(aule_tensor_handle handle, const float* data, uint32_t count);     /* :457  0; -1 bad handle; -3 size mismatch */
int32_t aule_tensor_download(aule_tensor_handle handle, float* output, uint32_t count);       /* :469 */
int32_t aule_tensor_download_u32(aule_tensor_handle handle, uint32_t* output, uint32_t count);/* :481 */
uint32_t aule_tensor_size(aule_tensor_handle handle);          /* src/lib.zig:626 element count, 0 if invalid */
uint32_t aule_tensor_count(void);                              /* src/lib.zig:383 */
uint32_t aule_tensor_max(void);                                /* src/lib.zig:392 */
void aule_tensor_clear_all(void);                              /* src/lib.zig:397 */

/* ---- handle-based forward: GQA (Hkv from K's shape), cross-attn, causal ---- */
/* src/lib.zig:496-529 -> backend.zig:318-370 -> attention_gpu.zig:360-453.     */
/* rot_cos/rot_sin: both 0 (no rotation) or both handles of fp32 tensors shaped   */
/* [1, 1, >= max(seq_q, seq_k), head_dim/2] (interleaved pairs, one table for all */
/* heads); anything else is -3 + error text.                                      */
/* window_size > 0: sliding window, key j visible to query i only if            */
/* i - j < window_size, on top of the causal rule (the convention of the kernel */
/* the reference runs on ROCm, python/aule/triton_flash_amd.py:179-183).        */
int32_t aule_attention_forward_gpu(aule_tensor_handle q, aule_tensor_handle k, aule_tensor_handle v,
                                   aule_tensor_handle output, aule_tensor_handle rot_cos,
                                   aule_tensor_handle rot_sin, int32_t causal, int32_t window_size);

/* ---- training path (host pointers, MHA, Sq == Sk, fp32) -------------------- */
/* src/lib.zig:765-852: O and LSE[B,H,S] = m + ln(l) of the scaled scores.      */
int32_t aule_attention_forward_with_lse(const float* query, const float* key, const float* value,
                                        float* output, float* lse, uint32_t batch_size,
                                        uint32_t num_heads, uint32_t seq_len, uint32_t head_dim,
                                        int32_t causal);
/* src/lib.zig:639-762: dQ,dK,dV from Q,K,V,O,dO,LSE.                           */
int32_t aule_attention_backward(const float* query, const float* key, const float* value,
                                const float* output, const float* grad_output, const float* lse,
                                float* grad_query, float* grad_key, float* grad_value,
                                uint32_t batch_size, uint32_t num_heads, uint32_t seq_len,
                                uint32_t head_dim, int32_t causal);

/* ---- out-of-scope features: exported so that ctypes attribute lookup in the  */
/* reference binding (vulkan.py:300-316) keeps working; they return -3.        */
int32_t aule_attention_forward_paged(aule_tensor_handle q, aule_tensor_handle k, aule_tensor_handle v,
                                     aule_tensor_handle output, aule_tensor_handle rot_cos,
                                     aule_tensor_handle rot_sin, int32_t causal,
                                     int32_t window_size);                    /* src/lib.zig:533 */
int32_t aule_spatial_sort(aule_tensor_handle keys, aule_tensor_handle values,
                          aule_tensor_handle indices, uint32_t sort_dim);     /* src/lib.zig:568 */
int32_t aule_attention_forward_gravity(aule_tensor_handle q, aule_tensor_handle k, aule_tensor_handle v,
                                       aule_tensor_handle output, aule_tensor_handle rot_cos,
                                       aule_tensor_handle rot_sin, aule_tensor_handle indices,
                                       int32_t causal, uint32_t max_attend,
                                       int32_t window_size);                  /* src/lib.zig:587 */

/* ========================================================================== */
/* Additive entry points (no reference counterpart; they are what the Python   */
/* surface aule.flash_attention binds for torch/ROCm tensors, replacing the    */
/* Triton launch at python/aule/triton_flash_amd.py:393-500).                 */
/* ========================================================================== */
typedef enum aule_dtype {
    AULE_DTYPE_F32 = 0,  /* fp32 storage, fp32 MFMA (v_mfma_f32_32x32x2_f32) */
    AULE_DTYPE_F16 = 1,  /* fp16 storage, fp16 MFMA, fp32 accumulate/softmax */
    AULE_DTYPE_BF16 = 2  /* bf16 storage, bf16 MFMA, fp32 accumulate/softmax */
} aule_dtype;

/* All tensors row-major contiguous: Q,O,dO,dQ [B,Hq,Sq,D]; K,V,dK,dV [B,Hkv,Sk,D];
 * LSE [B,Hq,Sq] fp32.  Pointers are DEVICE pointers on `device`.
 * head_dim in {32, 64, 128, 256} (paged decode: {32, 64, 128}); heads_q % heads_kv == 0.
 * `causal`: 0 = none; 1 = top-left aligned (query i sees keys j <= i), the rule of
 * every reference implementation; 2 = bottom-right aligned (query i sits at position
 * i + seq_k - seq_q, i.e. the last query sees every key; needs seq_k >= seq_q) --
 * an additive option for chunked prefill / decode against a longer KV history.
 * With mode 2 the sliding window is measured from the shifted position as well.
 * The handle-based and host entry points above keep the reference's rule (any
 * non-zero `causal` = top-left). */
#define AULE_CAUSAL_NONE 0
#define AULE_CAUSAL_TOP_LEFT 1
#define AULE_CAUSAL_BOTTOM_RIGHT 2
typedef struct aule_attn_desc {
    uint32_t struct_size;  /* = sizeof(aule_attn_desc) */
    int32_t dtype;         /* aule_dtype */
    uint32_t batch, heads_q, heads_kv, seq_q, seq_k, head_dim;
    float scale;           /* softmax scale; 0 or NaN => 1/sqrt(head_dim) */
    int32_t causal;        /* AULE_CAUSAL_* */
    int32_t window_size;   /* <= 0: full attention; W > 0: key j visible to query i only if i - j < W */
    int32_t device;        /* HIP device ordinal; -1 = current device */
    void* stream;          /* hipStream_t; NULL = default stream */
    const void* q;
    const void* k;
    const void* v;
    void* out;
    float* lse;            /* optional (NULL to skip) */
    void* workspace;       /* optional device buffer, 16-byte aligned, >= aule_attention_forward_workspace_size()  */
    uint64_t workspace_bytes;  /* bytes; NULL / too small: the library allocates stream-ordered (hipMallocAsync), which */
                           /* is correct everywhere but adds costly alloc/free nodes under hipGraph capture         */
} aule_attn_desc;

typedef struct aule_attn_bwd_desc {
    uint32_t struct_size;  /* = sizeof(aule_attn_bwd_desc) */
    int32_t dtype;
    uint32_t batch, heads_q, heads_kv, seq_q, seq_k, head_dim;
    float scale;
    int32_t causal;
    int32_t window_size;
    int32_t device;
    void* stream;
    const void* q;
    const void* k;
    const void* v;
    const void* out;
    const void* dout;
    const float* lse;
    void* dq;
    void* dk;
    void* dv;
    void* workspace;       /* >= aule_attention_backward_workspace_size() bytes, device memory */
    uint64_t workspace_bytes;
} aule_attn_bwd_desc;

/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. Asynchronous. */
int32_t aule_attention_forward_ex(const aule_attn_desc* desc);
int32_t aule_attention_backward_ex(const aule_attn_bwd_desc* desc);
/* Paged-KV decode (additive).  Replaces python/aule/triton_flash_amd.py:543-737            */
/* (_paged_attention_fwd_amd / flash_attention_paged_amd): one query token per sequence, vLLM-style block tables.  */
/* Asynchronous on `stream`; device pointers.                                                                     */
typedef struct aule_paged_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_desc) */
    int32_t dtype;             /* AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch, heads_q, heads_kv, head_dim;   /* head_dim 32, 64 or 128 */
    uint32_t block_size;       /* tokens per cache block */
    uint32_t max_blocks;       /* columns of block_tables */
    float scale;               /* 0 -> 1/sqrt(head_dim) */
    int32_t window_size;       /* > 0: only the last window_size positions (context_len - 1 - pos < window_size) */
    int32_t device;            /* HIP device ordinal, -1 = current */
    void* stream;              /* hipStream_t */
    const void* q;             /* [batch, heads_q, head_dim] */
    const void* k_cache;       /* [num_blocks, block_size, heads_kv, head_dim] */
    const void* v_cache;       /* same layout */
    const int32_t* block_tables;   /* [batch, max_blocks]: physical block of each logical block */
    const int32_t* context_lens;   /* [batch]: keys per sequence (0 -> output row of zeros); read on the device and clamped
                                      there to [0, max_blocks * block_size], so a stale value cannot index out of the table */
    void* out;                 /* [batch, heads_q, head_dim] */
    void* workspace;           /* optional, as aule_attn_desc.workspace; size from aule_attention_paged_decode_workspace_size() */
    uint64_t workspace_bytes;
} aule_paged_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_paged_decode_ex(const aule_paged_desc* desc);
/* Bytes of optional workspace the forward / paged decode would otherwise allocate itself for this descriptor   */
/* (0: single-launch path, nothing needed).  Host logic only; pointers in the descriptor are not read.           */
uint64_t aule_attention_forward_workspace_size(const aule_attn_desc* desc);
uint64_t aule_attention_paged_decode_workspace_size(const aule_paged_desc* desc);

/* Paged-KV decode over an FP8 cache (additive).  k_cache / v_cache hold OCP FP8 e4m3fn codes, one byte per element   */
/* (the format gfx950 converts in hardware; MI300X's e4m3fnuz and e5m2 are not accepted), q and out stay 16-bit:      */
/*     K[pos, hk, :] = k_scale[hk] * float(k_cache[block, off, hk, :])    V[pos, hk, :] = v_scale[hk] * float(v_cache[...]) */
/* and the result is aule_attention_paged_decode_ex's on that K / V.  The scales are device arrays read by the kernel */
/* (no host synchronisation; safe under graph capture).  Every other field means what it means in aule_paged_desc.   */
typedef struct aule_paged_fp8_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_fp8_desc) = 136 */
    int32_t dtype;             /* type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 (the caches are e4m3fn by definition) */
    uint32_t batch, heads_q, heads_kv, head_dim;   /* head_dim 32, 64 or 128 */
    uint32_t block_size;
    uint32_t max_blocks;
    float scale;               /* 0 -> 1/sqrt(head_dim) */
    int32_t window_size;
    int32_t device;
    void* stream;              /* offset 48 */
    const void* q;             /* [batch, heads_q, head_dim], 16-bit */
    const void* k_cache;       /* [num_blocks, block_size, heads_kv, head_dim] e4m3fn bytes */
    const void* v_cache;       /* same layout */
    const int32_t* block_tables;
    const int32_t* context_lens;
    void* out;                 /* [batch, heads_q, head_dim], 16-bit */
    void* workspace;           /* offset 104; optional, size from aule_attention_paged_decode_fp8_workspace_size() */
    uint64_t workspace_bytes;
    const float* k_scale;      /* offset 120; [heads_kv] fp32, device */
    const float* v_scale;      /* offset 128; [heads_kv] fp32, device */
} aule_paged_fp8_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments (null scale pointers included); -4 launch failure. */
int32_t aule_attention_paged_decode_fp8_ex(const aule_paged_fp8_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  Same plan as the 16-bit call of the same shape. */
uint64_t aule_attention_paged_decode_fp8_workspace_size(const aule_paged_fp8_desc* desc);

/* Paged attention for SHORT MULTI-TOKEN queries (additive): the step that adds seq_q > 1 tokens per sequence -- verifying the */
/* k + 1 draft tokens of speculative decoding, multi-token prediction heads, a short tail chunk of a prompt against a cached   */
/* prefix.  q and out are [batch, heads_q, seq_q, head_dim] fp16 / bf16 with 1 <= seq_q <= 64 (the same for every sequence);   */
/* the caches are either of that dtype (cache_dtype AULE_KV_CACHE_SAME, k_scale / v_scale NULL) or OCP e4m3fn codes with the   */
/* [heads_kv] fp32 device scales of aule_paged_fp8_desc (AULE_KV_CACHE_FP8_E4M3).  Cache layout, block-table rules and the     */
/* on-device clamp of context_lens are those of aule_attention_paged_decode_ex.  context_lens[b] counts the keys in the cache  */
/* INCLUDING the seq_q new tokens (append them first: aule_kv_cache_append_ex).  With L_b the clamped length, query i of       */
/* sequence b sits at position p = L_b - seq_q + i and sees key j iff j <= p, and with window_size = W > 0 iff also p - j < W   */
/* -- the bottom-right rule of AULE_CAUSAL_BOTTOM_RIGHT.  A query with p < 0 (a sequence shorter than seq_q) gives an output    */
/* row of zeros.  lse (optional) is [batch, heads_q, seq_q] fp32: the natural log of the sum of exp(scaled score) over the     */
/* visible keys, k_scale included; -inf for a row that sees no key.  seq_q = 1 gives aule_attention_paged_decode_ex /          */
/* _fp8_ex bit for bit.  seq_q > 64 and per-sequence query lengths: aule_attention_paged_prefill_ex.  Not built: head_dim 256. */
/* No host synchronisation, and no allocation when a workspace is passed: captures into a hipGraph.                            */
typedef struct aule_paged_query_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_query_desc) = 152 */
    int32_t dtype;             /* type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch, heads_q, heads_kv, head_dim;   /* head_dim 32, 64 or 128 */
    uint32_t block_size;
    uint32_t max_blocks;
    float scale;               /* 0 -> 1/sqrt(head_dim) */
    int32_t window_size;       /* > 0: query at position p sees only the keys j with p - j < window_size */
    int32_t device;
    void* stream;              /* offset 48 */
    const void* q;             /* [batch, heads_q, seq_q, head_dim], 16-bit */
    const void* k_cache;       /* [num_blocks, block_size, heads_kv, head_dim]: 16-bit of q's dtype, or e4m3fn bytes */
    const void* v_cache;       /* same layout */
    const int32_t* block_tables;   /* [batch, max_blocks] */
    const int32_t* context_lens;   /* [batch]: keys per sequence, the seq_q new ones included */
    void* out;                 /* [batch, heads_q, seq_q, head_dim], 16-bit */
    void* workspace;           /* offset 104; optional, size from aule_attention_paged_query_workspace_size() */
    uint64_t workspace_bytes;
    const float* k_scale;      /* offset 120; [heads_kv] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const float* v_scale;      /* offset 128 */
    float* lse;                /* offset 136; optional (NULL to skip): [batch, heads_q, seq_q] fp32 */
    uint32_t seq_q;            /* offset 144; 1 .. 64 */
    int32_t cache_dtype;       /* offset 148; AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3 */
} aule_paged_query_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_paged_query_ex(const aule_paged_query_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses on shape grounds. */
uint64_t aule_attention_paged_query_workspace_size(const aule_paged_query_desc* desc);

/* Paged PREFILL (additive): ragged per-sequence queries against the paged KV cache -- the step of a continuous-batching engine,  */
/* whose sequences bring different numbers of new tokens (a prompt chunk behind a cached prefix next to a short verify next to    */
/* plain decodes).  q is [total_tokens, heads_q, head_dim] fp16 / bf16: the new tokens of all sequences packed along the first    */
/* axis, q_token_stride elements from one token to the next (the heads of a token contiguous; a slice of a fused QKV projection   */
/* needs no copy).  out is [total_tokens, heads_q, head_dim] contiguous, lse (optional) [total_tokens, heads_q] fp32.  The two     */
/* cache kinds, the cache layout and the scales are those of aule_paged_query_desc.  cu_seqlens_q is [batch + 1] int32 on the      */
/* device; context_lens[b] counts the keys in the cache INCLUDING the new tokens (append them first: aule_kv_cache_append_ex).     */
/* Every per-sequence value is read and clamped on the device (no host synchronisation; a stale value cannot index outside a      */
/* buffer):  L_b = clamp(context_lens[b], 0, max_blocks * block_size),  s_b = clamp(cu[b], 0, total_tokens),                       */
/* e_b = clamp(cu[b + 1], s_b, total_tokens),  n_b = min(e_b - s_b, max_seqlen_q).  Token i (0 <= i < n_b) of sequence b is row    */
/* s_b + i of q / out / lse and sits at position p = L_b - n_b + i; it sees key j iff j <= p, and with window_size = W > 0 iff     */
/* also p - j < W (the bottom-right rule of aule_attention_paged_query_ex).  A token with p < 0, or a sequence with L_b = 0,       */
/* gives an output row of zeros and lse = -inf.  Rows that belong to no [s_b, s_b + n_b) -- a tail of total_tokens padded for     */
/* graph capture, whatever hostile offsets leave over -- are NEVER written.  A table entry at logical block                        */
/* >= ceil(L_b / block_size) is never dereferenced and a key row at or beyond L_b never read.  lse is the natural log of the sum   */
/* of exp(scaled score) over the visible keys, k_scale included.  One launch of ceil(min(max_seqlen_q, total_tokens) * (heads_q /  */
/* heads_kv) / 128) * heads_kv * batch workgroups, no workspace, no allocation: captures into a hipGraph, and a replay sees the    */
/* CURRENT contents of cu_seqlens_q, context_lens and block_tables.  Alignment: q, out and the caches 16-byte aligned.            */
/* Not built: head_dim 256; key-range splits (a batch made only of single-token sequences at very long context is better served    */
/* by aule_attention_paged_decode_ex / aule_attention_paged_query_ex, which split the keys over the device); a backward pass.      */
/* The descriptor is checked before the device is needed: -3 for a refused descriptor and 0 for one with nothing to do             */
/* (total_tokens = 0, batch = 0 or heads_q = 0) are answered without aule_init().                                                   */
typedef struct aule_paged_prefill_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_prefill_desc) = 152 */
    int32_t dtype;             /* type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* offset 8; AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3 */
    uint32_t batch;            /* offset 12; sequences */
    uint32_t heads_q, heads_kv, head_dim;   /* head_dim 32, 64 or 128 */
    uint32_t block_size;       /* offset 28; any value > 0 */
    uint32_t max_blocks;       /* offset 32; columns of block_tables */
    uint32_t total_tokens;     /* offset 36; rows of q / out; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 40; >= 1: sizes the grid, and caps every n_b */
    float scale;               /* offset 44; 0 -> 1/sqrt(head_dim) */
    int32_t window_size;       /* offset 48; > 0: the token at position p sees only the keys j with p - j < window_size */
    int32_t device;            /* offset 52; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 56; elements, >= heads_q * head_dim, a multiple of 8 */
    void* stream;              /* offset 64; hipStream_t */
    const void* q;             /* offset 72; [total_tokens, heads_q, head_dim], 16-bit */
    const void* k_cache;       /* offset 80; [num_blocks, block_size, heads_kv, head_dim]: 16-bit of q's dtype, or e4m3fn bytes */
    const void* v_cache;       /* offset 88; same layout */
    const int32_t* block_tables;   /* offset 96; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 104; [batch]: keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 112; [batch + 1], device */
    void* out;                 /* offset 120; [total_tokens, heads_q, head_dim], 16-bit, contiguous */
    float* lse;                /* offset 128; optional (NULL to skip): [total_tokens, heads_q] fp32 */
    const float* k_scale;      /* offset 136; [heads_kv] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const float* v_scale;      /* offset 144 */
} aule_paged_prefill_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_paged_prefill_ex(const aule_paged_prefill_desc* desc);

/* Paged prefill with FP8 matrix products (additive): aule_attention_paged_prefill_ex over an FP8 cache with BOTH products in e4m3 --   */
/* the cache's codes are multiplied as they are (v_mfma_scale_f32_32x32x64_f8f6f4, block scales 1.0), nothing is turned back into     */
/* 16-bit.  The same descriptor, the same rules, clamps, masks, grid and memory-safety contract; what differs is the arithmetic:      */
/* each row (token, head) of q is quantised in the kernel to e4m3 with its own scale amax|q| / 448 (1 for a zero row), which joins    */
/* the score scale, and the softmax weights are rounded to e4m3 after a factor 2^8 (the row's largest weight is 256; the factor       */
/* cancels in out and is taken out of lse).  lse is that of the quantised q: it never sees the rounding of the weights.  out carries  */
/* the e4m3 rounding of q and of the weights (2^-4 relative per weight) on top of the cache's own: use it where the FP8 cache's       */
/* accuracy is already accepted.  Refused (-3, with a reason): cache_dtype other than AULE_KV_CACHE_FP8_E4M3, head_dim 32 (64 and 128 */
/* are built), null scales.  No sinks, no tree masks.  Opt-in: nothing routes here by itself.  Nothing-to-do answers (0) and refusals  */
/* come before the device is needed, as for the twin.                                                                                 */
int32_t aule_attention_paged_prefill_fp8mma_ex(const aule_paged_prefill_desc* desc);

/* Paged CASCADE (additive): the paged prefill for a batch whose sequences share a prefix -- a system prompt, a few-shot header.   */
/* The shared keys live behind ONE table, prefix_block_table [max_prefix_blocks] int32, and are read once for the whole batch;     */
/* block_tables[b] lists only the sequence's OWN blocks and context_lens[b] counts only its OWN keys, the new tokens included.     */
/* prefix_len is [1] int32 on the DEVICE, read and clamped by the kernel: P = clamp(prefix_len[0], 0, max_prefix_blocks *          */
/* block_size).  Every other field, every clamp (L_b, s_b, e_b, n_b) and the rows that are written are those of                    */
/* aule_paged_prefill_desc.  The sequence's keys are the P prefix keys followed by its L_b own keys: token i of sequence b sits at  */
/* own position p = L_b - n_b + i, sees every prefix key and own key j iff j <= p.  A token with p < 0 gives zeros and lse = -inf   */
/* whatever the prefix holds; P = 0 gives aule_attention_paged_prefill_ex bit for bit, in out and lse.  A prefix table entry at     */
/* logical block >= ceil(P / block_size) is never dereferenced, a prefix key row at or beyond P never read.                         */
/* Three launches on `stream`: the shared-prefix kernel (the rows of all sequences packed densely per KV head, the prefix keys      */
/* split into nsplit ranges of whole 64-key tiles, one fp32 partial of head_dim + 2 floats per row and split), the paged prefill    */
/* unchanged on the own keys, and a merge of the partials into its result.  Workspace: at least                                     */
/*     round16(nsplit * total_tokens * heads_q * (head_dim + 2) * 4) + round16(total_tokens * heads_q * 4)   bytes                   */
/* (the partials, then the LSE of the own keys) with nsplit from the launch plan -- chosen on the host from the shape and the       */
/* prefix table's CAPACITY so that row blocks * heads_kv * nsplit covers the device's compute units, at most 32; there is no        */
/* device-to-host read: size the prefix table to the prefix.  aule_attention_paged_cascade_workspace_size() gives the number; a     */
/* call without a workspace, or with one that is too small or not 16-byte aligned, allocates on the stream.  No host                */
/* synchronisation, and no allocation when a workspace is passed: captures into a hipGraph, and a replay sees the CURRENT           */
/* prefix_len, context_lens, cu_seqlens_q and tables.  With hostile cu_seqlens_q that make two sequences own the same row, that     */
/* row's value is unspecified (and nothing outside out / lse is written).  Not built: a sliding window, head_dim 256, a backward.   */
/* The descriptor is checked before the device is needed, like aule_paged_prefill_desc.                                             */
typedef struct aule_paged_cascade_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_cascade_desc) = 184 */
    int32_t dtype;             /* type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* offset 8; AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3 */
    uint32_t batch;            /* offset 12; sequences */
    uint32_t heads_q, heads_kv, head_dim;   /* head_dim 32, 64 or 128 */
    uint32_t block_size;       /* offset 28; any value > 0, of both tables */
    uint32_t max_blocks;       /* offset 32; columns of block_tables */
    uint32_t total_tokens;     /* offset 36; rows of q / out; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 40; >= 1 */
    float scale;               /* offset 44; 0 -> 1/sqrt(head_dim) */
    uint32_t max_prefix_blocks;   /* offset 48; entries of prefix_block_table, >= 1 */
    int32_t device;            /* offset 52; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 56; elements, >= heads_q * head_dim, a multiple of 8 */
    void* stream;              /* offset 64; hipStream_t */
    const void* q;             /* offset 72; [total_tokens, heads_q, head_dim], 16-bit */
    const void* k_cache;       /* offset 80; [num_blocks, block_size, heads_kv, head_dim]: 16-bit of q's dtype, or e4m3fn bytes */
    const void* v_cache;       /* offset 88; same layout */
    const int32_t* block_tables;   /* offset 96; [batch, max_blocks]: own blocks */
    const int32_t* context_lens;   /* offset 104; [batch]: own keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 112; [batch + 1], device */
    void* out;                 /* offset 120; [total_tokens, heads_q, head_dim], 16-bit, contiguous */
    float* lse;                /* offset 128; optional (NULL to skip): [total_tokens, heads_q] fp32, over prefix and own keys */
    const float* k_scale;      /* offset 136; [heads_kv] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const float* v_scale;      /* offset 144 */
    const int32_t* prefix_block_table;   /* offset 152; [max_prefix_blocks] */
    const int32_t* prefix_len; /* offset 160; [1], device */
    void* workspace;           /* offset 168; optional, size from aule_attention_paged_cascade_workspace_size() */
    uint64_t workspace_bytes;  /* offset 176 */
} aule_paged_cascade_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_paged_cascade_ex(const aule_paged_cascade_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses or that has nothing to do. */
uint64_t aule_attention_paged_cascade_workspace_size(const aule_paged_cascade_desc* desc);

/* Paged MLA (additive): multi-head LATENT attention in its absorbed form (DeepSeek-V2 / V3 / R1) -- decode and short verify over a */
/* latent KV cache.  Dimensions: qk_dim = 576 (512 compressed dimensions, then 64 rotary ones) and v_dim = 512 are the only pair     */
/* accepted (anything else: -3); dtype fp16 or bf16.                                                                                  */
/* kv_cache is ONE cache, [num_blocks, block_size, 576] of q's dtype, contiguous, 16-byte aligned: row pos of sequence b is the key  */
/* of ALL query heads (all 576 elements) and the value (elements 0..511); the kernel fetches it once for both products.  The block   */
/* table rules are those of aule_attention_paged_decode_ex: block_tables [batch, max_blocks] int32, any block_size >= 1 (powers of   */
/* two index with a shift); an entry at logical block >= ceil(L_b / block_size) is never dereferenced and a row at or beyond L_b     */
/* never read.                                                                                                                        */
/* q is [total_tokens, heads_q, 576] with q_token_stride elements from one token to the next (a multiple of 8, >= heads_q * 576, the */
/* heads of a token contiguous); out is [total_tokens, heads_q, 512] contiguous; lse (optional) [total_tokens, heads_q] fp32, the    */
/* natural log of the softmax denominator.  q and out are 16-byte aligned.                                                            */
/* Ragged queries follow aule_paged_prefill_desc exactly: cu_seqlens_q [batch + 1] int32 on the device, context_lens[b] counts the   */
/* keys INCLUDING the new tokens, and every clamp is made on the device (no host synchronisation; a stale or hostile value cannot     */
/* index outside a buffer):  L_b = clamp(context_lens[b], 0, max_blocks * block_size),  s_b = clamp(cu[b], 0, total_tokens),          */
/* e_b = clamp(cu[b + 1], s_b, total_tokens),  n_b = min(e_b - s_b, max_seqlen_q).  Token i of sequence b is row s_b + i, sits at     */
/* p = L_b - n_b + i and sees key j iff j <= p.  A token with p < 0, or a sequence with L_b = 0, gives zeros and lse = -inf.  Rows    */
/* of no sequence are NEVER written.  cu_seqlens_q = NULL means plain decode: sequence b owns row b, n_b = 1, max_seqlen_q is read    */
/* as 1 (it must still be >= 1) and total_tokens >= batch is required.                                                                */
/* scale = 0 means 1/sqrt(576), the library's rule; DeepSeek callers pass their own 1/sqrt(192) * mscale.                             */
/* Launches: the packed rows of a sequence (token-major, head-minor) are cut into blocks of 64 and the keys of a sequence into        */
/* nsplit ranges; nsplit is fixed on the host from the shape alone -- row blocks * batch * nsplit covers the device's compute units,  */
/* at most 64 and at most one split per two 64-key tiles of the table's capacity -- and each workgroup derives its own sequence's     */
/* range on the device from L_b: split k owns tiles [k * ceil(tiles(L_b) / nsplit), ...).  nsplit = 1: one launch.  nsplit > 1: fp32  */
/* partials of 512 + 2 floats per (split, token, head) in the workspace and a combine kernel that adds them in split order (no        */
/* atomics: two runs are bit-identical).  Workspace bytes = round16(nsplit * total_tokens * heads_q * 514 * 4), 0 for nsplit = 1:     */
/* aule_attention_mla_paged_workspace_size() gives the number; a call without a workspace, or with one that is too small or not       */
/* 16-byte aligned, allocates on the stream.  No host synchronisation, and no allocation when a workspace is passed: captures into a  */
/* hipGraph, and a replay sees the CURRENT cu_seqlens_q, context_lens and block_tables.  With hostile cu_seqlens_q that make two      */
/* sequences own the same row, that row's value is unspecified (and nothing outside out / lse is written).                            */
/* An FP8 latent cache is aule_attention_mla_paged_fp8_ex below; the write side of both caches is aule_mla_kv_append_ex; a tree of   */
/* new tokens instead of the chain (tree drafters) is aule_attention_mla_paged_tree_ex below.                                        */
/* Not built: a sliding window; a backward.  The non-absorbed prefill form (192 / 128) is aule_attention_mla_prefill_ex below.       */
/* The descriptor is checked before the device is needed: -3 for a refused descriptor and 0 for one with nothing to do               */
/* (total_tokens = 0, batch = 0 or heads_q = 0) are answered without aule_init().                                                     */
typedef struct aule_mla_paged_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_paged_desc) = 136 */
    int32_t dtype;             /* offset 4; type of q / out / kv_cache: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch;            /* offset 8; sequences */
    uint32_t heads_q;          /* offset 12 */
    uint32_t qk_dim;           /* offset 16; 576 */
    uint32_t v_dim;            /* offset 20; 512 */
    uint32_t block_size;       /* offset 24; any value > 0 */
    uint32_t max_blocks;       /* offset 28; columns of block_tables */
    uint32_t total_tokens;     /* offset 32; rows of q / out; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 36; >= 1: sizes the grid, and caps every n_b */
    float scale;               /* offset 40; 0 -> 1/sqrt(576) */
    int32_t device;            /* offset 44; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 48; elements, >= heads_q * 576, a multiple of 8 */
    void* stream;              /* offset 56; hipStream_t */
    const void* q;             /* offset 64; [total_tokens, heads_q, 576], 16-bit */
    const void* kv_cache;      /* offset 72; [num_blocks, block_size, 576], q's dtype */
    const int32_t* block_tables;   /* offset 80; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 88; [batch]: keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 96; [batch + 1], device; NULL: plain decode */
    void* out;                 /* offset 104; [total_tokens, heads_q, 512], 16-bit, contiguous */
    float* lse;                /* offset 112; optional (NULL to skip): [total_tokens, heads_q] fp32 */
    void* workspace;           /* offset 120; optional, size from aule_attention_mla_paged_workspace_size() */
    uint64_t workspace_bytes;  /* offset 128 */
} aule_mla_paged_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_mla_paged_ex(const aule_mla_paged_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses or that has nothing to do. */
uint64_t aule_attention_mla_paged_workspace_size(const aule_mla_paged_desc* desc);

/* Paged MLA over an FP8 latent cache (additive).  aule_mla_paged_desc field for field -- the same offsets, the same rules, the same  */
/* clamps, rows, launches, plan and workspace -- with two differences:                                                                */
/*   kv_cache is [num_blocks, block_size, 576] OCP e4m3fn codes, one byte per element (contiguous, 16-byte aligned); dtype stays the  */
/*   type of q / out;                                                                                                                 */
/*   kv_scale is ONE fp32 value for the whole cache, a DEVICE array of 1 element read by the kernel (no host synchronisation; required,*/
/*   4-byte aligned):  key = kv_scale * float(code row), value = its first 512 elements.                                              */
/* The codes are converted exactly to q's 16-bit type on their way into the kernel's LDS image and everything after that is the       */
/* 16-bit kernel's arithmetic; kv_scale multiplies the score scale and the fp32 accumulators, never an element.  So lse includes      */
/* kv_scale (it is the log of the softmax denominator of the dequantised keys), and with kv_scale = 1 the call equals                 */
/* aule_attention_mla_paged_ex on the codes converted to q's dtype bit for bit.  aule_hip_debug_mla_plan answers for both kinds (the  */
/* plan depends on the shape alone).  The codes are what aule_mla_kv_append_ex writes with AULE_KV_CACHE_FP8_E4M3.                    */
typedef struct aule_mla_paged_fp8_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_paged_fp8_desc) = 144 */
    int32_t dtype;             /* offset 4; type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch;            /* offset 8; sequences */
    uint32_t heads_q;          /* offset 12 */
    uint32_t qk_dim;           /* offset 16; 576 */
    uint32_t v_dim;            /* offset 20; 512 */
    uint32_t block_size;       /* offset 24; any value > 0 */
    uint32_t max_blocks;       /* offset 28; columns of block_tables */
    uint32_t total_tokens;     /* offset 32; rows of q / out; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 36; >= 1: sizes the grid, and caps every n_b */
    float scale;               /* offset 40; 0 -> 1/sqrt(576) */
    int32_t device;            /* offset 44; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 48; elements, >= heads_q * 576, a multiple of 8 */
    void* stream;              /* offset 56; hipStream_t */
    const void* q;             /* offset 64; [total_tokens, heads_q, 576], 16-bit */
    const void* kv_cache;      /* offset 72; [num_blocks, block_size, 576], e4m3fn codes */
    const int32_t* block_tables;   /* offset 80; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 88; [batch]: keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 96; [batch + 1], device; NULL: plain decode */
    void* out;                 /* offset 104; [total_tokens, heads_q, 512], 16-bit, contiguous */
    float* lse;                /* offset 112; optional (NULL to skip): [total_tokens, heads_q] fp32 */
    void* workspace;           /* offset 120; optional, size from aule_attention_mla_paged_fp8_workspace_size() */
    uint64_t workspace_bytes;  /* offset 128 */
    const float* kv_scale;     /* offset 136; [1] fp32, device */
} aule_mla_paged_fp8_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure.  Checked before the device is needed, as above. */
int32_t aule_attention_mla_paged_fp8_ex(const aule_mla_paged_fp8_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  The number aule_attention_mla_paged_workspace_size gives for the shape. */
uint64_t aule_attention_mla_paged_fp8_workspace_size(const aule_mla_paged_fp8_desc* desc);

/* Paged MLA with TREE MASKS (additive): the verify step of tree drafters (MTP heads, EAGLE, Medusa, SpecInfer) over the latent cache   */
/* of either kind -- all nodes of a sequence's tree are appended to the cache and verified in one call, the latent read once per      */
/* sequence instead of once per root-to-leaf path.  The rule is the paged prefill tree's (TREE MASKS below), unchanged: tree_mask      */
/* holds one int64 word per packed token on the DEVICE, read as 64 bits by the kernel on every launch (no host copy, no                */
/* synchronisation, capturable: a replay sees the current words).  With L_b, s_b and n_b the values aule_mla_paged_desc clamps on the  */
/* device, a sequence with n_b <= 64 carries a tree (decided on the device): its token i is row s_b + i, sits at p = L_b - n_b + i,    */
/* and sees key j iff 0 <= j < L_b and                                                                                                 */
/*     j < L_b - n_b  (a context key)        or        bit j - (L_b - n_b) of tree_mask[s_b + i] is set.                                */
/* Any bit pattern is legal: no self bit is implied, no order required; a set bit at or beyond L_b is ignored; a token at a negative   */
/* position (L_b < n_b) sees nothing.  A sequence with n_b > 64 (a prompt chunk in the same step) keeps aule_mla_paged_desc's causal   */
/* rule and its words are not read.  A row without a visible key gives zeros and lse = -inf; rows of no sequence are never written.    */
/* The chain words tree_mask[s_b + i] = (2 << i) - 1 give out and lse of aule_attention_mla_paged_ex / _fp8_ex BIT FOR BIT (finite     */
/* cached data).  There is no window and there are no sinks: the MLA entries have neither.                                             */
/* The descriptor is aule_mla_paged_fp8_desc field for field through offset 143 -- the same rules, clamps, rows, launches, plan,       */
/* workspace and combine (aule_hip_debug_mla_plan answers for this kind too: the plan depends on the shape alone) -- and then          */
/* tree_mask and cache_dtype: AULE_KV_CACHE_SAME (kv_cache of q's dtype; kv_scale must be NULL) or AULE_KV_CACHE_FP8_E4M3 (e4m3fn      */
/* codes; kv_scale required, aule_mla_paged_fp8_desc's rule).  Refused with -3 and a reason, without aule_init(), beyond what the      */
/* twins refuse: a NULL cu_seqlens_q (a tree of one node per sequence is the decode call: aule_attention_mla_paged_ex), a NULL or not  */
/* 8-byte aligned tree_mask when there is work, a cache_dtype that is neither, kv_scale given with a 16-bit cache.                     */
/* Not built: more than 64 tree tokens per sequence; the cascade; tree visibility inside the MLA indexer (callers on DSA models filter */
/* the emitted lists and call aule_attention_mla_sparse_ex); any backward.                                                             */
typedef struct aule_mla_paged_tree_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_paged_tree_desc) = 160 */
    int32_t dtype;             /* offset 4; type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch;            /* offset 8; sequences */
    uint32_t heads_q;          /* offset 12 */
    uint32_t qk_dim;           /* offset 16; 576 */
    uint32_t v_dim;            /* offset 20; 512 */
    uint32_t block_size;       /* offset 24; any value > 0 */
    uint32_t max_blocks;       /* offset 28; columns of block_tables */
    uint32_t total_tokens;     /* offset 32; rows of q / out; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 36; >= 1: sizes the grid, and caps every n_b */
    float scale;               /* offset 40; 0 -> 1/sqrt(576) */
    int32_t device;            /* offset 44; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 48; elements, >= heads_q * 576, a multiple of 8 */
    void* stream;              /* offset 56; hipStream_t */
    const void* q;             /* offset 64; [total_tokens, heads_q, 576], 16-bit */
    const void* kv_cache;      /* offset 72; [num_blocks, block_size, 576], q's dtype or e4m3fn codes (cache_dtype) */
    const int32_t* block_tables;   /* offset 80; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 88; [batch]: keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 96; [batch + 1], device; required */
    void* out;                 /* offset 104; [total_tokens, heads_q, 512], 16-bit, contiguous */
    float* lse;                /* offset 112; optional (NULL to skip): [total_tokens, heads_q] fp32 */
    void* workspace;           /* offset 120; optional, size from aule_attention_mla_paged_tree_workspace_size() */
    uint64_t workspace_bytes;  /* offset 128 */
    const float* kv_scale;     /* offset 136; [1] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const int64_t* tree_mask;  /* offset 144; [total_tokens] int64, device, 8-byte aligned (required when there is work) */
    int32_t cache_dtype;       /* offset 152; AULE_KV_CACHE_SAME (q's dtype) or AULE_KV_CACHE_FP8_E4M3 */
    uint32_t reserved;         /* offset 156; padding, not read */
} aule_mla_paged_tree_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure.  Checked before the device is needed, as above. */
int32_t aule_attention_mla_paged_tree_ex(const aule_mla_paged_tree_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  The number aule_attention_mla_paged_workspace_size gives for the shape. */
uint64_t aule_attention_mla_paged_tree_workspace_size(const aule_mla_paged_tree_desc* desc);

/* SPARSE MLA (additive): absorbed multi-head latent attention over PER-TOKEN KEY LISTS (DeepSeek-V3.2 "DSA" and its derivatives: an    */
/* indexer picks a fixed number of keys per query token, typically 2048, and the attention runs over only those rows of the latent     */
/* cache, in decode and in prefill).  This comment is the contract.                                                                    */
/* q is [total_tokens, heads_q, 576], fp16 or bf16, q_token_stride elements from one token to the next (a multiple of 8, >= heads_q *  */
/* 576, the heads of a token contiguous: aule_mla_paged_desc's rule); out is [total_tokens, heads_q, 512] contiguous; lse (optional)   */
/* [total_tokens, heads_q] fp32.  q, out and kv_cache are 16-byte aligned.                                                             */
/* kv_cache is [num_blocks, block_size, 576], contiguous: of q's dtype (cache_dtype AULE_KV_CACHE_SAME, kv_scale NULL) or OCP e4m3fn   */
/* codes with ONE fp32 scale on the device (AULE_KV_CACHE_FP8_E4M3, kv_scale required, 4-byte aligned; key = kv_scale * float(code     */
/* row): exactly aule_mla_paged_fp8_desc's rule -- the scale multiplies the score scale and the fp32 accumulators, never an element,   */
/* and with kv_scale = 1 the call equals the 16-bit call on the converted codes bit for bit).  The cache is addressed as a FLAT array  */
/* of S = num_blocks * block_size rows ("slots"), so a contiguous [L, 576] latent is the cache [L, 1, 576]: sparse prefill over an     */
/* un-paged latent.                                                                                                                    */
/* indices is [total_tokens, topk] int32, contiguous, on the device, 1 <= topk <= 65536.  indices[t][i] is a slot, block * block_size  */
/* + offset: the convention of slot_mapping in aule_mla_kv_append_desc.                                                                */
/* RULE.  Token t, every head h: the key set is the multiset { kv_cache.flat[indices[t][i]] : 0 <= indices[t][i] < S }.  Entries       */
/* outside [0, S) are skipped (-1 is the conventional pad; INT32_MIN and INT32_MAX are legal); a slot listed twice counts twice; there */
/* is NO causal rule -- the indexer is responsible for visibility.  scores = scale * q . key over all 576 elements (scale = 0 means    */
/* 1/sqrt(576)), values are the key's first 512 elements, lse is the natural log of the softmax denominator (kv_scale included).  A    */
/* token with no valid entry gives zeros and lse = -inf.                                                                               */
/* READS AND WRITES.  Every one of the total_tokens rows of out / lse is written.  A cache row that no valid entry names is never read */
/* and cannot influence the result (an invalid entry contributes a row of zeros with weight 0, not some other row).  indices and       */
/* kv_scale are read by the kernel on every launch: no host copy, no synchronisation, and no allocation when a workspace is passed, so */
/* the call captures into a hipGraph and a replay sees their CURRENT contents.                                                         */
/* LAUNCHES.  Work item (split, row block, token): a row block is 64 heads of ONE token, row_blocks = ceil(heads_q / 64); the list is  */
/* cut into tiles = ceil(topk / 64) tiles of 64 entries and nsplit ranges, nsplit fixed on the host from the shape alone:              */
/* nsplit = clamp(ceil(CUs / (total_tokens * row_blocks)), 1, min(64, max(1, tiles / 2))); split k owns tiles [k * ceil(tiles /        */
/* nsplit), ...).  nsplit = 1: one launch.  nsplit > 1: fp32 partials of 512 + 2 floats per (split, token, head) in the workspace,     */
/* aule_mla_paged_desc's layout, added by its combine kernel in split order (no atomics: two runs are bit-identical).  Workspace bytes */
/* = round16(nsplit * total_tokens * heads_q * 514 * 4), 0 for nsplit = 1: aule_attention_mla_sparse_workspace_size() gives the        */
/* number.  workspace = NULL: allocated and freed on the stream; a workspace that is given but smaller than that (or not 16-byte       */
/* aligned) is refused with -3 and nothing is launched.                                                                                */
/* REFUSED with -3 and a reason naming the field (aule_get_error), before the device is needed: a wrong struct_size; dtype outside     */
/* {fp16, bf16}; cache_dtype outside {0, 1}; an FP8 cache without kv_scale, kv_scale with a 16-bit cache; heads_q < 1; topk outside    */
/* 1..65536; num_blocks * block_size outside 1..2^31-1; total_tokens < 0; q_token_stride too small or not a multiple of 8;             */
/* (total_tokens + 64) * heads_q or the grid past 2^31-1; a null or misaligned required pointer; a caller workspace smaller than the   */
/* plan's.  The size query and the plan hook give the same verdict on every field and read no pointer.  total_tokens = 0 returns 0     */
/* without a launch and without aule_init().                                                                                           */
/* The lists come from the indexer, aule_mla_indexer_logits_ex + aule_mla_indexer_topk_ex below.                                       */
/* Not built: a causal rule in the kernel; packing several tokens' heads into one row block when heads_q < 64; logical positions       */
/* resolved through a block table in the kernel; a backward; sink logits or tree masks with a list.                                    */
typedef struct aule_mla_sparse_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_sparse_desc) = 120 */
    int32_t dtype;             /* offset 4; type of q / out: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* offset 8; AULE_KV_CACHE_SAME (q's dtype) or AULE_KV_CACHE_FP8_E4M3 */
    int32_t heads_q;           /* offset 12; >= 1 */
    uint32_t num_blocks;       /* offset 16; num_blocks * block_size = S, 1 .. 2^31 - 1 */
    uint32_t block_size;       /* offset 20 */
    int32_t total_tokens;      /* offset 24; rows of q / out / indices; 0: returns 0 without a launch */
    int32_t topk;              /* offset 28; entries per token, 1 .. 65536 */
    float scale;               /* offset 32; 0 -> 1/sqrt(576) */
    int32_t device;            /* offset 36; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 40; elements, >= heads_q * 576, a multiple of 8 */
    void* stream;              /* offset 48; hipStream_t */
    const void* q;             /* offset 56; [total_tokens, heads_q, 576], 16-bit */
    const void* kv_cache;      /* offset 64; [num_blocks, block_size, 576], q's dtype or e4m3fn codes */
    const int32_t* indices;    /* offset 72; [total_tokens, topk] slots, device */
    const float* kv_scale;     /* offset 80; [1] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    void* out;                 /* offset 88; [total_tokens, heads_q, 512], 16-bit, contiguous */
    float* lse;                /* offset 96; optional (NULL to skip): [total_tokens, heads_q] fp32 */
    void* workspace;           /* offset 104; optional, size from aule_attention_mla_sparse_workspace_size() */
    uint64_t workspace_bytes;  /* offset 112 */
} aule_mla_sparse_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_mla_sparse_ex(const aule_mla_sparse_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses or that has nothing to do. */
uint64_t aule_attention_mla_sparse_workspace_size(const aule_mla_sparse_desc* desc);

/* MLA INDEXER (additive): the producer of aule_mla_sparse_desc's key lists (DeepSeek-V3.2 "DSA"): index logits over a paged cache of  */
/* index keys, then the top-k key list of every query token.  Two entries, two launches; these two comments are the contract.           */
/* LOGITS.  logits[t][s] = sum_h weights[t][h] * relu(q[t][h][:] . k[s][:]), fp32.                                                       */
/* q is [total_tokens, heads, 128], fp16 or bf16, 1 <= heads <= 64, q_token_stride elements from one token to the next (a multiple of  */
/* 8, >= heads * 128, the heads of a token contiguous: a slice of a wider projection is read in place); weights is [total_tokens,      */
/* heads] fp32, contiguous -- the caller folds heads^-1/2, the softmax scale and any q scale into it.  k_cache is [num_blocks,         */
/* block_size, 128], contiguous, ONE key row per position shared by all heads: of q's dtype (cache_dtype AULE_KV_CACHE_SAME, k_scale   */
/* NULL) or OCP e4m3fn codes (AULE_KV_CACHE_FP8_E4M3) with a PER-ROW scale k_scale [num_blocks, block_size] fp32 on the device, key =  */
/* k_scale[row] * float(code row).  The codes are converted exactly to q's type and the row scale multiplies the finished logit,       */
/* never an element (relu commutes with a positive scale): with every scale 1 the call equals the 16-bit call on the converted codes   */
/* bit for bit.  q and k_cache are 16-byte aligned, weights, k_scale and logits 4-byte.                                                 */
/* block_tables [batch, max_blocks], context_lens [batch], cu_seqlens_q [batch + 1] (NULL: plain decode, sequence b owns row b,        */
/* max_seqlen_q read as 1, total_tokens >= batch) and max_seqlen_q follow aule_mla_paged_desc exactly, every clamp made on the device: */
/* L_b = clamp(context_lens[b], 0, W) with W = max_blocks * block_size, s_b = clamp(cu[b], 0, total_tokens), e_b = clamp(cu[b + 1],    */
/* s_b, total_tokens), n_b = min(e_b - s_b, max_seqlen_q).  Token i of sequence b is row s_b + i, sits at p = L_b - n_b + i and sees   */
/* key j iff 0 <= j <= p.  A table entry is clamped to [0, num_blocks) before it is used; an entry at logical block >= ceil(L_b /      */
/* block_size) is never dereferenced.  No host synchronisation, no allocation: the call captures into a hipGraph and a replay sees the */
/* CURRENT tables, lengths, offsets and weights.                                                                                        */
/* OUTPUT.  logits is [total_tokens, W] fp32 with logits_stride >= W elements from row to row.  For a row that belongs to a sequence   */
/* EVERY one of the W columns is written: the logit where the key is visible, -inf elsewhere.  A cache row (and a k_scale entry) that  */
/* no token sees is never read.  Rows of no sequence are NEVER written.  Cost: total_tokens * W * 4 bytes (1 GB at 2048 x 128 K):     */
/* callers chunk total_tokens or size the table.                                                                                        */
/* LAUNCH.  Work item (sequence, group of 4 tokens, chunk of keys); every column of every owned row belongs to exactly one item: no    */
/* workspace, no combine, no atomics, two runs are bit-identical.  The grid is fixed on the host from (batch, max_seqlen_q, W, compute */
/* units): token groups = ceil(max_seqlen_q / 4), key chunks = clamp(ceil(4 * CUs / (batch * token groups)), 1, ceil(W / 128)) evened  */
/* out to chunks of a multiple of 128 keys; aule_hip_debug_mla_indexer_plan() gives the numbers.                                        */
/* REFUSED with -3 and a reason naming the field (aule_get_error), before the device is needed: a wrong struct_size; dtype outside     */
/* {fp16, bf16}; cache_dtype outside {0, 1}; heads outside 1..64; head_dim != 128; num_blocks = 0; block_size / max_blocks zero or W   */
/* >= 2^30; max_seqlen_q = 0; q_token_stride too small or not a multiple of 8; logits_stride < W; batch / total_tokens >= 2^30; plain  */
/* decode with total_tokens < batch; a grid past 2^31 - 1; and, by the launch alone, a null or misaligned pointer, an FP8 cache        */
/* without k_scale, k_scale with a 16-bit cache.  The plan hook gives the same verdict on every field and reads no pointer.            */
/* total_tokens = 0 or batch = 0 returns 0 without a launch and without aule_init().                                                   */
/* Not built: FP8 queries and FP8 MFMAs; a fused streaming top-k that never writes [total_tokens, W]; an append kernel for the index   */
/* keys; heads > 64; a backward.                                                                                                        */
typedef struct aule_mla_indexer_logits_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_indexer_logits_desc) = 136 */
    int32_t dtype;             /* offset 4; type of q: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* offset 8; AULE_KV_CACHE_SAME (q's dtype) or AULE_KV_CACHE_FP8_E4M3 */
    uint32_t heads;            /* offset 12; index heads, 1 .. 64 */
    uint32_t head_dim;         /* offset 16; 128 */
    uint32_t batch;            /* offset 20; sequences; 0: returns 0 without a launch */
    uint32_t num_blocks;       /* offset 24; blocks of k_cache, >= 1 */
    uint32_t block_size;       /* offset 28; any value > 0 */
    uint32_t max_blocks;       /* offset 32; columns of block_tables; W = max_blocks * block_size < 2^30 */
    uint32_t total_tokens;     /* offset 36; rows of q / weights / logits; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 40; >= 1: sizes the grid, and caps every n_b */
    int32_t device;            /* offset 44; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 48; elements, >= heads * 128, a multiple of 8 */
    int64_t logits_stride;     /* offset 56; elements, >= W */
    void* stream;              /* offset 64; hipStream_t */
    const void* q;             /* offset 72; [total_tokens, heads, 128], 16-bit */
    const float* weights;      /* offset 80; [total_tokens, heads] fp32 */
    const void* k_cache;       /* offset 88; [num_blocks, block_size, 128], q's dtype or e4m3fn codes */
    const float* k_scale;      /* offset 96; [num_blocks, block_size] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const int32_t* block_tables;   /* offset 104; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 112; [batch]: keys per sequence, the new ones included */
    const int32_t* cu_seqlens_q;   /* offset 120; [batch + 1], device; NULL: plain decode */
    float* logits;             /* offset 128; [total_tokens, logits_stride] fp32 */
} aule_mla_indexer_logits_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_mla_indexer_logits_ex(const aule_mla_indexer_logits_desc* desc);

/* TOP-K.  indices[t][:] = the key list of token t from logits [total_tokens, W] fp32 (logits_stride >= W; ANY such tensor, not       */
/* necessarily aule_mla_indexer_logits_ex's), 1 <= topk <= 65536, with the tables, lengths, offsets and clamps of the logits entry.    */
/* RULE, fully canonical.  Visibility comes from the position arithmetic (key j iff 0 <= j <= p), NOT from -inf marks: a visible -inf  */
/* still counts as visible, and columns past p are never read.  Among token t's visible keys, order by logit descending, then by       */
/* position ascending; logits compare by numeric value (-0 == +0) and a NaN ranks as -inf.  The first min(topk, p + 1) keys are        */
/* emitted in ASCENDING POSITION order; the tail is padded with -1.  A token with p < 0 gets all -1.  Rows of no sequence are NEVER    */
/* written.  The result is deterministic: no atomics on global memory, two runs are bit-identical.                                     */
/* output AULE_INDEXER_SLOTS: entry = block_tables[b][pos / block_size] * block_size + pos % block_size (the table entry as it stands: */
/* nothing is dereferenced through it), the slot_mapping convention aule_mla_sparse_desc consumes when the latent cache shares the     */
/* table and the block size.  AULE_INDEXER_POSITIONS: the raw positions, for a latent cache with another block size.                   */
/* LAUNCH.  One workgroup per (sequence, token below max_seqlen_q): batch * max_seqlen_q workgroups.  p + 1 <= topk: every visible key, */
/* no logit is read.  Else a radix select over an order-preserving 32-bit key (4 passes of 8 bits, histograms in LDS) finds the        */
/* threshold, ties at the threshold go to the lowest positions, and one ordered compaction pass writes the list.  No host              */
/* synchronisation, no allocation, capturable; a replay sees the current logits, tables, lengths and offsets.                          */
/* REFUSED with -3 and a reason naming the field, before the device is needed: a wrong struct_size; output outside {0, 1}; topk        */
/* outside 1..65536; reserved != 0; block_size / max_blocks zero or W >= 2^30; max_seqlen_q = 0; logits_stride < W; batch /            */
/* total_tokens >= 2^30; plain decode with total_tokens < batch; batch * max_seqlen_q past 2^31 - 1; a null or misaligned pointer.     */
/* total_tokens = 0 or batch = 0 returns 0 without a launch and without aule_init().                                                   */
#define AULE_INDEXER_SLOTS 0      /* cache slots through the block table */
#define AULE_INDEXER_POSITIONS 1  /* logical positions */
typedef struct aule_mla_indexer_topk_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_indexer_topk_desc) = 96 */
    int32_t output;            /* offset 4; AULE_INDEXER_SLOTS or AULE_INDEXER_POSITIONS */
    int32_t topk;              /* offset 8; entries per token, 1 .. 65536 */
    uint32_t batch;            /* offset 12; sequences; 0: returns 0 without a launch */
    uint32_t block_size;       /* offset 16; any value > 0 */
    uint32_t max_blocks;       /* offset 20; columns of block_tables; W = max_blocks * block_size < 2^30 */
    uint32_t total_tokens;     /* offset 24; rows of logits / indices; 0: returns 0 without a launch */
    uint32_t max_seqlen_q;     /* offset 28; >= 1: sizes the grid, and caps every n_b */
    int32_t device;            /* offset 32; HIP device ordinal, -1 = current */
    uint32_t reserved;         /* offset 36; 0 */
    int64_t logits_stride;     /* offset 40; elements, >= W */
    void* stream;              /* offset 48; hipStream_t */
    const float* logits;       /* offset 56; [total_tokens, logits_stride] fp32 */
    const int32_t* block_tables;   /* offset 64; [batch, max_blocks] */
    const int32_t* context_lens;   /* offset 72; [batch] */
    const int32_t* cu_seqlens_q;   /* offset 80; [batch + 1], device; NULL: plain decode */
    int32_t* indices;          /* offset 88; [total_tokens, topk] int32, contiguous */
} aule_mla_indexer_topk_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_mla_indexer_topk_ex(const aule_mla_indexer_topk_desc* desc);

/* VARIABLE-LENGTH packed batches (additive): sequences of different lengths packed along one token axis, forward and backward --   */
/* SFT with sequence packing, encoder batches without padding, prefill without a paged cache (flash_attn_varlen_func's case).        */
/* Tensors: q, out, dout, dq are [total_q, heads_q, head_dim] and k, v, dk, dv [total_k, heads_kv, head_dim], fp16 or bf16, with     */
/* heads_q % heads_kv == 0 and head_dim 32, 64 or 128; lse is [total_q, heads_q] fp32.  The heads of a token are contiguous; q, k    */
/* and v each carry their own token stride in elements (q_token_stride >= heads_q * head_dim, k_token_stride and v_token_stride      */
/* >= heads_kv * head_dim, all multiples of 8: slices of a fused QKV projection need no copy).  out, lse, dout, dq, dk and dv are    */
/* contiguous; every tensor is 16-byte aligned.                                                                                      */
/* Sequence bounds: cu_seqlens_q and cu_seqlens_k are [batch + 1] int32 on the DEVICE, read and clamped in the kernels (no host      */
/* read, no host synchronisation; a stale value cannot index outside a buffer):                                                      */
/*     s_q = clamp(cu_q[b], 0, total_q)   e_q = clamp(cu_q[b+1], s_q, total_q)   n = min(e_q - s_q, max_seqlen_q)                    */
/*     s_k = clamp(cu_k[b], 0, total_k)   e_k = clamp(cu_k[b+1], s_k, total_k)   L = min(e_k - s_k, max_seqlen_k)                    */
/* max_seqlen_q and max_seqlen_k are host integers >= 1: they size the grids and cut a longer sequence to its first max_seqlen_*     */
/* tokens, as aule_paged_prefill_desc.max_seqlen_q does.                                                                             */
/* Visibility: query token i of sequence b is row s_q + i, key j is row s_k + j.  The query's position is pos = i for                */
/* AULE_CAUSAL_NONE and AULE_CAUSAL_TOP_LEFT and pos = i + L - n for AULE_CAUSAL_BOTTOM_RIGHT (L < n is allowed: tokens with         */
/* pos < 0 see nothing).  Key j < L is visible iff (!causal || j <= pos), and with window_size = W > 0 iff also pos - j < W: the     */
/* rules of aule_attn_desc, applied per sequence.                                                                                    */
/* Empty and unowned rows: a query row with no visible key gives out = 0, lse = -inf and dq = 0 and contributes nothing to dk / dv.  */
/* Every owned query row of out, lse and dq is written, every owned key row of dk and dv too (zeros if no query sees it, n = 0       */
/* included).  Rows of out, lse, dq, dk and dv that belong to no [s_q, s_q + n) or [s_k, s_k + L) are NEVER written.  With hostile   */
/* offsets that make two sequences own one row, that row's value is unspecified, and nothing outside the outputs is written.         */
/* Softmax in log2 units with fp32 m, l and accumulators; lse is the natural log of the softmax denominator.                         */
/* Forward: one launch of ceil(min(max_seqlen_q, total_q) * (heads_q / heads_kv) / 128) * heads_kv * batch workgroups, no workspace. */
/* Backward: three launches on `stream` (delta, dQ, dK/dV); the workspace is delta [total_q, heads_q] fp32,                          */
/* aule_attention_varlen_backward_workspace_size() bytes.  workspace NULL: the library allocates on the stream; a workspace that is  */
/* given but too small or not 16-byte aligned is refused.  No host synchronisation, and no allocation when a workspace is passed:    */
/* both capture into a hipGraph, and a replay sees the CURRENT contents of cu_seqlens_q / cu_seqlens_k.                              */
/* The descriptors are checked before the device is needed: -3 with a reason (struct_size, dtype, head_dim, head ratio, causal code, */
/* strides, alignment, null pointers, max_seqlen_* < 1, (total_q + 128) * (heads_q / heads_kv) beyond 32 bits, a workspace that is   */
/* too small) and 0 for a call with nothing to do (forward: total_q = 0, batch = 0 or heads_q = 0; backward: batch = 0, heads_q = 0, */
/* or total_q = 0 and total_k = 0) are answered without aule_init().  total_k = 0 with total_q > 0 writes zeros and -inf to the      */
/* owned rows (k and v may then be NULL); a backward with total_q = 0 zeroes the owned dk and dv rows (the query-side pointers may   */
/* then be NULL).  Not built: fp32, head_dim 256, FP8 inputs, key-range splits for one long sequence.                                */
typedef struct aule_varlen_desc {
    uint32_t struct_size;      /* = sizeof(aule_varlen_desc) = 144 */
    int32_t dtype;             /* AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch;            /* offset 8; sequences */
    uint32_t heads_q, heads_kv, head_dim;   /* offsets 12, 16, 20; head_dim 32, 64 or 128 */
    uint32_t total_q;          /* offset 24; rows of q / out */
    uint32_t total_k;          /* offset 28; rows of k / v */
    uint32_t max_seqlen_q;     /* offset 32; >= 1: sizes the grid, and caps every n */
    uint32_t max_seqlen_k;     /* offset 36; >= 1: caps every L (and sizes the backward's dK/dV grid) */
    float scale;               /* offset 40; 0 -> 1/sqrt(head_dim) */
    int32_t causal;            /* offset 44; AULE_CAUSAL_* */
    int32_t window_size;       /* offset 48; > 0: on; any value is accepted (one that masks nothing, INT32_MAX included, equals no window bit for bit) */
    int32_t device;            /* offset 52; HIP device ordinal, -1 = current */
    int64_t q_token_stride;    /* offset 56; elements, >= heads_q * head_dim, a multiple of 8 */
    int64_t k_token_stride;    /* offset 64; elements, >= heads_kv * head_dim, a multiple of 8 */
    int64_t v_token_stride;    /* offset 72 */
    void* stream;              /* offset 80; hipStream_t */
    const void* q;             /* offset 88 */
    const void* k;             /* offset 96 */
    const void* v;             /* offset 104 */
    const int32_t* cu_seqlens_q;   /* offset 112; [batch + 1], device */
    const int32_t* cu_seqlens_k;   /* offset 120; [batch + 1], device */
    void* out;                 /* offset 128; [total_q, heads_q, head_dim], contiguous */
    float* lse;                /* offset 136; optional (NULL to skip): [total_q, heads_q] fp32 */
} aule_varlen_desc;
/* The same problem statement (every field up to cu_seqlens_k at the same offset), then the backward's tensors. */
typedef struct aule_varlen_bwd_desc {
    uint32_t struct_size;      /* = sizeof(aule_varlen_bwd_desc) = 192 */
    int32_t dtype;
    uint32_t batch;
    uint32_t heads_q, heads_kv, head_dim;
    uint32_t total_q;
    uint32_t total_k;
    uint32_t max_seqlen_q;
    uint32_t max_seqlen_k;
    float scale;
    int32_t causal;
    int32_t window_size;
    int32_t device;
    int64_t q_token_stride;
    int64_t k_token_stride;
    int64_t v_token_stride;
    void* stream;              /* offset 80 */
    const void* q;
    const void* k;
    const void* v;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;   /* offset 120 */
    const void* out;           /* offset 128; the forward's out */
    const float* lse;          /* offset 136; the forward's lse (required) */
    const void* dout;          /* offset 144; [total_q, heads_q, head_dim], contiguous */
    void* dq;                  /* offset 152; [total_q, heads_q, head_dim], contiguous */
    void* dk;                  /* offset 160; [total_k, heads_kv, head_dim], contiguous */
    void* dv;                  /* offset 168 */
    void* workspace;           /* offset 176; optional, size from aule_attention_varlen_backward_workspace_size() */
    uint64_t workspace_bytes;  /* offset 184 */
} aule_varlen_bwd_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_varlen_forward_ex(const aule_varlen_desc* desc);
int32_t aule_attention_varlen_backward_ex(const aule_varlen_bwd_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses. */
uint64_t aule_attention_varlen_backward_workspace_size(const aule_varlen_bwd_desc* desc);

/* ATTENTION SINKS (additive): per-head sink logits for the variable-length, paged-prefill and paged-query entries above -- the    */
/* models whose heads each carry a learned logit that joins the softmax denominator and contributes no value (gpt-oss and its      */
/* derivatives).  sinks is [heads_q] fp32 on the DEVICE: a raw logit, multiplied by neither scale nor k_scale; the kernels read it   */
/* on every launch and nothing copies it to the host, so a captured call replays with its CURRENT contents.  For a query row of     */
/* head h with visible keys j and scaled scores s_j (scale, and k_scale of an FP8 cache, included):                                 */
/*     Z = sum_j exp(s_j) + exp(sinks[h])        out = sum_j exp(s_j) v_j / Z        lse = ln Z                                     */
/* Visibility, clamps, owned rows, alignment, workspaces and every other rule are EXACTLY those of the sinkless twin each           */
/* descriptor repeats field for field at the same offsets (the new pointers are appended; the descriptors are checked through that  */
/* prefix).  A row that sees no key gives out = 0 and lse = sinks[h] (the twin: -inf).  sinks[h] = -inf means "no sink": out and    */
/* lse of that head equal the twin's bit for bit, a row without a key included (0 and -inf).  A NaN or +inf logit gives unspecified */
/* values for that head only; a logit never takes part in an address.                                                               */
/* Backward (variable-length): dq, dk and dv come from the kernels of aule_attention_varlen_backward_ex given the sink-inclusive    */
/* lse; dsinks [heads_q] fp32 is  dsinks[h] = - sum over the rows some sequence owns of exp(sinks[h] - lse[row, h]) delta[row, h],  */
/* delta = rowsum(dout * out): two more launches, no atomics, a fixed summation order (two runs agree bit for bit), exactly         */
/* heads_q floats written; 0 for a head with sinks[h] = -inf.  The workspace is the sinkless backward's plus the reduction's        */
/* partials.  A call with nothing to do (the twin's rule) returns 0 and leaves dsinks unwritten.                                    */
/* A NULL sinks (or dsinks) is refused with -3 and a reason; refusals and calls with nothing to do are answered without aule_init() */
/* (aule_attention_paged_query_sink_ex: refusals of a NULL sinks and of the descriptor's shape).  seq_q = 1 in the query entry is   */
/* the decode call.  Not built: sinks for the dense aule_attention_forward_ex, the cascade, the MLA entries, head_dim 256.          */
typedef struct aule_varlen_sink_desc {
    uint32_t struct_size;      /* = sizeof(aule_varlen_sink_desc) = 152 */
    int32_t dtype;
    uint32_t batch;
    uint32_t heads_q, heads_kv, head_dim;
    uint32_t total_q;
    uint32_t total_k;
    uint32_t max_seqlen_q;
    uint32_t max_seqlen_k;
    float scale;
    int32_t causal;
    int32_t window_size;
    int32_t device;
    int64_t q_token_stride;
    int64_t k_token_stride;
    int64_t v_token_stride;
    void* stream;              /* offset 80 */
    const void* q;
    const void* k;
    const void* v;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;   /* offset 120 */
    void* out;                 /* offset 128 */
    float* lse;                /* offset 136; optional (NULL to skip): ln Z, the sink included */
    const float* sinks;        /* offset 144; [heads_q] fp32, device (required) */
} aule_varlen_sink_desc;
typedef struct aule_varlen_sink_bwd_desc {
    uint32_t struct_size;      /* = sizeof(aule_varlen_sink_bwd_desc) = 208 */
    int32_t dtype;
    uint32_t batch;
    uint32_t heads_q, heads_kv, head_dim;
    uint32_t total_q;
    uint32_t total_k;
    uint32_t max_seqlen_q;
    uint32_t max_seqlen_k;
    float scale;
    int32_t causal;
    int32_t window_size;
    int32_t device;
    int64_t q_token_stride;
    int64_t k_token_stride;
    int64_t v_token_stride;
    void* stream;              /* offset 80 */
    const void* q;
    const void* k;
    const void* v;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;   /* offset 120 */
    const void* out;           /* offset 128; the sink forward's out */
    const float* lse;          /* offset 136; the sink forward's lse (required) */
    const void* dout;          /* offset 144 */
    void* dq;                  /* offset 152 */
    void* dk;                  /* offset 160 */
    void* dv;                  /* offset 168 */
    void* workspace;           /* offset 176; optional, size from aule_attention_varlen_sink_backward_workspace_size() */
    uint64_t workspace_bytes;  /* offset 184 */
    const float* sinks;        /* offset 192; [heads_q] fp32, device (required) */
    float* dsinks;             /* offset 200; [heads_q] fp32, device (required): written */
} aule_varlen_sink_bwd_desc;
typedef struct aule_paged_prefill_sink_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_prefill_sink_desc) = 160 */
    int32_t dtype;
    int32_t cache_dtype;       /* offset 8 */
    uint32_t batch;            /* offset 12 */
    uint32_t heads_q, heads_kv, head_dim;
    uint32_t block_size;       /* offset 28 */
    uint32_t max_blocks;       /* offset 32 */
    uint32_t total_tokens;     /* offset 36 */
    uint32_t max_seqlen_q;     /* offset 40 */
    float scale;               /* offset 44 */
    int32_t window_size;       /* offset 48 */
    int32_t device;            /* offset 52 */
    int64_t q_token_stride;    /* offset 56 */
    void* stream;              /* offset 64 */
    const void* q;             /* offset 72 */
    const void* k_cache;       /* offset 80 */
    const void* v_cache;       /* offset 88 */
    const int32_t* block_tables;   /* offset 96 */
    const int32_t* context_lens;   /* offset 104 */
    const int32_t* cu_seqlens_q;   /* offset 112 */
    void* out;                 /* offset 120 */
    float* lse;                /* offset 128; optional (NULL to skip): ln Z, the sink included */
    const float* k_scale;      /* offset 136 */
    const float* v_scale;      /* offset 144 */
    const float* sinks;        /* offset 152; [heads_q] fp32, device (required) */
} aule_paged_prefill_sink_desc;
typedef struct aule_paged_query_sink_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_query_sink_desc) = 160 */
    int32_t dtype;
    uint32_t batch, heads_q, heads_kv, head_dim;
    uint32_t block_size;
    uint32_t max_blocks;
    float scale;
    int32_t window_size;
    int32_t device;
    void* stream;              /* offset 48 */
    const void* q;
    const void* k_cache;
    const void* v_cache;
    const int32_t* block_tables;
    const int32_t* context_lens;
    void* out;
    void* workspace;           /* offset 104; optional, size from aule_attention_paged_query_sink_workspace_size() */
    uint64_t workspace_bytes;
    const float* k_scale;      /* offset 120 */
    const float* v_scale;      /* offset 128 */
    float* lse;                /* offset 136; optional (NULL to skip): ln Z, the sink included */
    uint32_t seq_q;            /* offset 144; 1 .. 64 (1: the decode) */
    int32_t cache_dtype;       /* offset 148 */
    const float* sinks;        /* offset 152; [heads_q] fp32, device (required) */
} aule_paged_query_sink_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_varlen_sink_forward_ex(const aule_varlen_sink_desc* desc);
int32_t aule_attention_varlen_sink_backward_ex(const aule_varlen_sink_bwd_desc* desc);
int32_t aule_attention_paged_prefill_sink_ex(const aule_paged_prefill_sink_desc* desc);
int32_t aule_attention_paged_query_sink_ex(const aule_paged_query_sink_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses on shape grounds.  The backward's  */
/* is aule_attention_varlen_backward_workspace_size() of the same problem plus the partials of the dsinks reduction; the query's is   */
/* aule_attention_paged_query_workspace_size() of the same problem.                                                                  */
uint64_t aule_attention_varlen_sink_backward_workspace_size(const aule_varlen_sink_bwd_desc* desc);
uint64_t aule_attention_paged_query_sink_workspace_size(const aule_paged_query_sink_desc* desc);

/* TREE MASKS (additive): the paged query and the paged prefill with a TREE of new tokens instead of a chain -- the verify step of   */
/* tree drafters (EAGLE, Medusa, SpecInfer): all nodes are appended to the cache and verified in one call; a node sees the cached    */
/* context and its ancestors, not its siblings or cousins.  tree_mask holds one int64 word per new token on the DEVICE, read as 64   */
/* bits by the kernel on every launch (no host copy, no synchronisation, capturable).  For a sequence with L keys in the cache      */
/* (after the twin's clamps) and n new tokens, new token t is key L - n + t; query token i sees key j iff 0 <= j < L and             */
/*     j < L - n  (a context key)        or        bit j - (L - n) of tree_mask[row i] is set.                                       */
/* Any bit pattern is legal: no self bit is implied, no order required; bits at or above n and bits that name a key below 0 are      */
/* ignored.  A query at a negative position gives zeros, a row that sees no key out = 0 and lse = -inf, keys at or beyond L are      */
/* never read.  The chain words tree_mask[i] = (2 << i) - 1 give out and lse of the twin entry BIT FOR BIT (finite cached data).    */
/* Query entry: tree_mask [batch, seq_q], row b * seq_q + i.  Prefill entry: tree_mask [total_tokens], indexed by packed token; a   */
/* sequence carries a tree iff its clamped n <= 64 (decided on the device), a longer one (a prompt chunk in the same step) keeps the */
/* twin's causal rule and its words are not read.  Every other rule, the workspace included, is the twin's: each descriptor is its   */
/* twin field for field plus tree_mask and is checked by the twin's checker.  Refused with -3 and a reason, without aule_init():     */
/* a NULL tree_mask when there is work, and window_size > 0 (a window is not defined over a tree).  Not built: sliding windows or    */
/* sink logits with a tree, the cascade, head_dim 256, more than 64 tree tokens per sequence, any backward.  The same rule over    */
/* the latent cache of the MLA models is aule_attention_mla_paged_tree_ex above.                                                    */
typedef struct aule_paged_query_tree_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_query_tree_desc) = 160 */
    int32_t dtype;
    uint32_t batch, heads_q, heads_kv, head_dim;
    uint32_t block_size;
    uint32_t max_blocks;
    float scale;
    int32_t window_size;       /* <= 0 (a window is refused) */
    int32_t device;
    void* stream;              /* offset 48 */
    const void* q;
    const void* k_cache;
    const void* v_cache;
    const int32_t* block_tables;
    const int32_t* context_lens;
    void* out;
    void* workspace;           /* offset 104; optional, size from aule_attention_paged_query_tree_workspace_size() */
    uint64_t workspace_bytes;
    const float* k_scale;      /* offset 120 */
    const float* v_scale;      /* offset 128 */
    float* lse;                /* offset 136; optional (NULL to skip) */
    uint32_t seq_q;            /* offset 144; 1 .. 64 */
    int32_t cache_dtype;       /* offset 148 */
    const int64_t* tree_mask;  /* offset 152; [batch, seq_q] int64, device (required) */
} aule_paged_query_tree_desc;
typedef struct aule_paged_prefill_tree_desc {
    uint32_t struct_size;      /* = sizeof(aule_paged_prefill_tree_desc) = 160 */
    int32_t dtype;
    int32_t cache_dtype;       /* offset 8 */
    uint32_t batch;            /* offset 12 */
    uint32_t heads_q, heads_kv, head_dim;
    uint32_t block_size;       /* offset 28 */
    uint32_t max_blocks;       /* offset 32 */
    uint32_t total_tokens;     /* offset 36 */
    uint32_t max_seqlen_q;     /* offset 40 */
    float scale;               /* offset 44 */
    int32_t window_size;       /* offset 48; <= 0 (a window is refused) */
    int32_t device;            /* offset 52 */
    int64_t q_token_stride;    /* offset 56 */
    void* stream;              /* offset 64 */
    const void* q;             /* offset 72 */
    const void* k_cache;       /* offset 80 */
    const void* v_cache;       /* offset 88 */
    const int32_t* block_tables;   /* offset 96 */
    const int32_t* context_lens;   /* offset 104 */
    const int32_t* cu_seqlens_q;   /* offset 112 */
    void* out;                 /* offset 120 */
    float* lse;                /* offset 128; optional (NULL to skip) */
    const float* k_scale;      /* offset 136 */
    const float* v_scale;      /* offset 144 */
    const int64_t* tree_mask;  /* offset 152; [total_tokens] int64, device (required) */
} aule_paged_prefill_tree_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_paged_query_tree_ex(const aule_paged_query_tree_desc* desc);
int32_t aule_attention_paged_prefill_tree_ex(const aule_paged_prefill_tree_desc* desc);
/* Host logic only; pointers in the descriptor are not read: aule_attention_paged_query_workspace_size() of the same problem.        */
uint64_t aule_attention_paged_query_tree_workspace_size(const aule_paged_query_tree_desc* desc);

/* Merge of two attention states (additive): out_a, out_b [rows, heads, head_dim] fp16 / bf16 are attention outputs of the same    */
/* queries over two DISJOINT key sets, lse_a, lse_b [rows, heads] fp32 the natural logs of their softmax denominators (the lse of  */
/* the calls above).  With M = max(lse_a, lse_b) and w_x = exp(lse_x - M):                                                          */
/*     out = (w_a out_a + w_b out_b) / (w_a + w_b)        lse = M + log(w_a + w_b)                                                  */
/* the state over the union of the keys.  A side with lse = -inf holds no key: the result is the other side bit for bit; both:     */
/* zeros and -inf.  The result does not depend on the order of the pair.  out may alias out_a or out_b (a thread reads the 16   */
/* bytes it writes); lse must NOT overlap lse_a or lse_b -- every thread of a row reads both -- and such a call is refused (-3).    */
/* head_dim: any multiple of 8; everything contiguous, out_a / out_b / out 16-byte aligned.  One launch, no workspace.             */
typedef struct aule_merge_states_desc {
    uint32_t struct_size;      /* = sizeof(aule_merge_states_desc) = 80 */
    int32_t dtype;             /* AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t rows;             /* offset 8; 0: returns 0 without a launch */
    uint32_t heads;            /* offset 12 */
    uint32_t head_dim;         /* offset 16; a multiple of 8, at most 1024 */
    int32_t device;            /* offset 20; HIP device ordinal, -1 = current */
    void* stream;              /* offset 24; hipStream_t */
    const void* out_a;         /* offset 32 */
    const float* lse_a;        /* offset 40 */
    const void* out_b;         /* offset 48 */
    const float* lse_b;        /* offset 56 */
    void* out;                 /* offset 64 */
    float* lse;                /* offset 72 */
} aule_merge_states_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_merge_states_ex(const aule_merge_states_desc* desc);

/* MLA PREFILL (additive): multi-head latent attention in its NON-ABSORBED form, the form the prompt runs in (DeepSeek-V2 / V3 / R1), */
/* over a variable-length packed batch; forward only.  Every head has its own 128-wide k_nope and 128-wide v (the two slices of the  */
/* kv_b up-projection), all heads of a token share one 64-wide rotated k_pe, queries are 192 wide (q_nope | q_pe), the output is 128  */
/* wide: key row j of head h is [k_nope[j, h] | k_pe[j]].  It is MHA: one heads count.  This comment is the contract.                */
/* Tensors (fp16 or bf16, one dtype), strides in ELEMENTS, each a multiple of 8; every pointer 16-byte aligned:                       */
/*     q      [total_q, heads, 192]   q_token_stride >= heads * 192, the heads of a token contiguous                                  */
/*     k_nope [total_k, heads, 128]   k_nope_head_stride >= 128, k_nope_token_stride >= (heads - 1) * k_nope_head_stride + 128        */
/*     v      [total_k, heads, 128]   v_head_stride >= 128, v_token_stride >= (heads - 1) * v_head_stride + 128                       */
/*     k_pe   [total_k, 64]           k_pe_token_stride >= 64                                                                         */
/*     out    [total_q, heads, 128]   contiguous        lse [total_q, heads] fp32, contiguous, optional (NULL to skip)                */
/* The head strides exist so that the two halves of a [total_k, heads, 256] kv_b output are read in place (head stride 256, token     */
/* stride heads * 256, v = k_nope + 128 elements); the k_pe token stride so that columns 512.. of a [total_k, 576] down-projection    */
/* are (token stride 576).  Head strides are below 2^30.  Nothing is padded: 192 / 128 / 64 exactly (qk_dim, v_dim state the first    */
/* two).                                                                                                                              */
/* Sequence bounds: cu_seqlens_q and cu_seqlens_k are [batch + 1] int32 on the DEVICE, max_seqlen_q and max_seqlen_k host integers   */
/* >= 1; the clamps, the cuts to the first max_seqlen_* tokens, the rows that are written and the behaviour under hostile offsets are */
/* EXACTLY those of aule_varlen_desc above (s_q, e_q, n, s_k, e_k, L): query i < n is row s_q + i, key j < L is row s_k + j.          */
/* Mask: causal is AULE_CAUSAL_NONE, _TOP_LEFT (pos = i) or _BOTTOM_RIGHT (pos = i + L - n); key j < L is visible iff                 */
/* (!causal || j <= pos).  L < n is allowed (tokens with pos < 0 see nothing); L > n with bottom-right is chunked prefill.  There is  */
/* no window.  scale = 0 means 1/sqrt(192); callers with a YaRN mscale pass their own.                                                */
/* A query row with no visible key gives out = 0 and lse = -inf; rows of no sequence are NEVER written.  Softmax in log2 units with   */
/* fp32 m, l and accumulators; lse is the natural log of the softmax denominator, so two calls over disjoint key chunks are merged    */
/* by aule_attention_merge_states_ex (chunked prefill against an up-projected context chunk: two calls and a merge).                  */
/* One launch of ceil(min(max_seqlen_q, total_q) / 128) * heads * batch workgroups, no workspace, no host synchronisation: captures   */
/* into a hipGraph, and a replay sees the CURRENT contents of cu_seqlens_q / cu_seqlens_k.                                            */
/* The descriptor is checked before the device is needed: -3 with a reason (struct_size, dtype, qk_dim / v_dim, causal code, each     */
/* stride too small or not a multiple of 8, alignment, null pointers, max_seqlen_* < 1, sizes beyond 32 bits) and 0 for a call with   */
/* nothing to do (total_q = 0, batch = 0 or heads = 0) are answered without aule_init().  total_k = 0 with total_q > 0 writes zeros   */
/* and -inf to the owned rows; k_nope, k_pe and v may then be NULL.                                                                   */
/* Not built: a backward of THIS entry (it saves nothing for one; the differentiable form is aule_attention_mla_prefill_backward_ex   */
/* below); a sliding window; GQA (heads_kv != heads_q); FP8 inputs; the rotation of q_pe / k_pe fused into the kernel;                */
/* key-range splits for one long sequence.                                                                                            */
typedef struct aule_mla_prefill_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_prefill_desc) = 176 */
    int32_t dtype;             /* offset 4; AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    uint32_t batch;            /* offset 8; sequences */
    uint32_t heads;            /* offset 12 */
    uint32_t qk_dim;           /* offset 16; 192 */
    uint32_t v_dim;            /* offset 20; 128 */
    uint32_t total_q;          /* offset 24; rows of q / out; 0: returns 0 without a launch */
    uint32_t total_k;          /* offset 28; rows of k_nope / k_pe / v */
    uint32_t max_seqlen_q;     /* offset 32; >= 1: sizes the grid, and caps every n */
    uint32_t max_seqlen_k;     /* offset 36; >= 1: caps every L */
    float scale;               /* offset 40; 0 -> 1/sqrt(192) */
    int32_t causal;            /* offset 44; AULE_CAUSAL_* */
    int32_t device;            /* offset 48; HIP device ordinal, -1 = current */
    uint32_t reserved;         /* offset 52; not read */
    int64_t q_token_stride;        /* offset 56 */
    int64_t k_nope_token_stride;   /* offset 64 */
    int64_t k_nope_head_stride;    /* offset 72 */
    int64_t v_token_stride;        /* offset 80 */
    int64_t v_head_stride;         /* offset 88 */
    int64_t k_pe_token_stride;     /* offset 96 */
    void* stream;              /* offset 104; hipStream_t */
    const void* q;             /* offset 112 */
    const void* k_nope;        /* offset 120 */
    const void* k_pe;          /* offset 128 */
    const void* v;             /* offset 136 */
    const int32_t* cu_seqlens_q;   /* offset 144; [batch + 1], device */
    const int32_t* cu_seqlens_k;   /* offset 152; [batch + 1], device */
    void* out;                 /* offset 160; [total_q, heads, 128], contiguous */
    float* lse;                /* offset 168; optional (NULL to skip): [total_q, heads] fp32 */
} aule_mla_prefill_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_mla_prefill_ex(const aule_mla_prefill_desc* desc);

/* MLA PREFILL BACKWARD (additive): the gradients of aule_attention_mla_prefill_ex for training and fine-tuning with sequence packing. */
/* This comment is the contract.  The problem statement -- every field up to cu_seqlens_k -- is aule_mla_prefill_desc's, at the same  */
/* offsets and under the same rules (tensors, strides, clamps of cu_seqlens_*, cuts by max_seqlen_*, the three causal modes, scale);  */
/* then the backward's tensors, of the same dtype:                                                                                    */
/*     out, dout [total_q, heads, 128]   contiguous; out and lse [total_q, heads] fp32 are the forward's results (lse is required)    */
/*     dq        [total_q, heads, 192]   contiguous                                                                                   */
/*     dk_nope   [total_k, heads, 128]   dk_nope_head_stride >= 128, dk_nope_token_stride >= (heads - 1) * dk_nope_head_stride + 128  */
/*     dv        [total_k, heads, 128]   dv_head_stride >= 128, dv_token_stride >= (heads - 1) * dv_head_stride + 128                 */
/*     dk_pe     [total_k, 64]           contiguous: the sum over the heads of the gradient of key columns 128 .. 191                 */
/* The four output strides are in ELEMENTS, multiples of 8, head strides below 2^30: the input-side rules, so that the gradient of a  */
/* [total_k, heads, 256] kv_b output is written in place into one buffer (head stride 256, token stride heads * 256,                  */
/* dv = dk_nope + 128 elements).  Every pointer is 16-byte aligned (lse 4-byte).                                                      */
/* Rows written: every owned row -- dq rows s_q .. s_q + n - 1 (zeros for a query without a visible key), dk_nope, dv and dk_pe rows  */
/* s_k .. s_k + L - 1 (zeros for a key no query sees, n = 0 included) -- and only those 192 / 128 / 128 / 64 elements of them; rows   */
/* of no sequence and the bytes between strided rows are NEVER written.  With hostile overlapping offsets the value of a doubly owned */
/* row is unspecified; nothing outside the outputs and the workspace is written.                                                     */
/* Launches, all on `stream`, no host synchronisation: delta = rowsum(dout * out), dQ, dK/dV and, when the plan cuts the heads into   */
/* more than one chunk, the dk_pe reduce.  The dK/dV kernel sums dk_pe over the heads of a chunk in registers; chunk c writes an fp32 */
/* partial to plane c of [n_chunks, total_k, 64] and the reduce adds the planes in chunk order.  There are no floating-point atomics: */
/* two runs of one call agree bit for bit.  n_chunks is at most 16 (aule_hip_debug_mla_prefill_backward_plan reports the plan).       */
/* Workspace: delta [total_q, heads] fp32 on a 256-byte boundary, then the planes when the reduce runs;                               */
/* aule_attention_mla_prefill_backward_workspace_size() gives the bytes.  workspace = NULL: allocated and freed on the stream; with   */
/* a workspace passed the call allocates nothing, captures into a hipGraph, and a replay sees the CURRENT cu_seqlens_*.               */
/* Checked before the device is needed: -3 with a reason -- the forward descriptor's list, plus null out / lse / dout / gradient      */
/* pointers, each output stride too small or not a multiple of 8, alignment, a workspace too small or not 16-byte aligned -- and 0    */
/* for a call with nothing to do (batch = 0, heads = 0, or total_q = 0 and total_k = 0) are answered without aule_init().             */
/* total_q = 0 with total_k > 0 zeroes the owned key rows (q, out, lse, dout, dq may then be NULL); total_k = 0 with total_q > 0      */
/* zeroes the owned dq rows (the key-side pointers may then be NULL).                                                                 */
typedef struct aule_mla_prefill_bwd_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_prefill_bwd_desc) = 264 */
    int32_t dtype;
    uint32_t batch;
    uint32_t heads;
    uint32_t qk_dim;
    uint32_t v_dim;
    uint32_t total_q;
    uint32_t total_k;
    uint32_t max_seqlen_q;
    uint32_t max_seqlen_k;     /* also sizes the dK/dV grid */
    float scale;
    int32_t causal;
    int32_t device;
    uint32_t reserved;
    int64_t q_token_stride;
    int64_t k_nope_token_stride;
    int64_t k_nope_head_stride;
    int64_t v_token_stride;
    int64_t v_head_stride;
    int64_t k_pe_token_stride;
    void* stream;
    const void* q;
    const void* k_nope;
    const void* k_pe;
    const void* v;
    const int32_t* cu_seqlens_q;
    const int32_t* cu_seqlens_k;
    const void* out;               /* offset 160; the forward's out */
    const float* lse;              /* offset 168; the forward's lse (required) */
    const void* dout;              /* offset 176; [total_q, heads, 128], contiguous */
    void* dq;                      /* offset 184; [total_q, heads, 192], contiguous */
    void* dk_nope;                 /* offset 192 */
    void* dk_pe;                   /* offset 200; [total_k, 64], contiguous */
    void* dv;                      /* offset 208 */
    int64_t dk_nope_token_stride;  /* offset 216 */
    int64_t dk_nope_head_stride;   /* offset 224 */
    int64_t dv_token_stride;       /* offset 232 */
    int64_t dv_head_stride;        /* offset 240 */
    void* workspace;               /* offset 248; optional, size from aule_attention_mla_prefill_backward_workspace_size() */
    uint64_t workspace_bytes;      /* offset 256 */
} aule_mla_prefill_bwd_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_attention_mla_prefill_backward_ex(const aule_mla_prefill_bwd_desc* desc);
/* Host logic only; pointers in the descriptor are not read.  0 for a descriptor the launch refuses or that has nothing to do. */
uint64_t aule_attention_mla_prefill_backward_workspace_size(const aule_mla_prefill_bwd_desc* desc);

/* Rotary position embedding pass (additive; SURVEY.md 8f row N1, second half).  Replaces the rotation the           */
/* reference fuses into its kernels: python/aule/triton_flash.py:32-52,:112-131,:165-180 (layout HALF) and            */
/* shaders/attention_f32.comp:98-111,:132-145 (layout INTERLEAVED).  x is [rows_bh, seq, head_dim] with               */
/* `row_pitch` elements per row; row s uses table row s + pos_offset; `inverse` applies the transposed rotation       */
/* (dQ', dK' -> dQ, dK).  in == out is allowed.  Asynchronous on `stream`; device pointers.                           */
#define AULE_ROPE_HALF 0         /* pairs (p, p + head_dim/2) */
#define AULE_ROPE_INTERLEAVED 1  /* pairs (2p, 2p + 1) */
typedef struct aule_rope_desc {
    uint32_t struct_size;      /* = sizeof(aule_rope_desc) */
    int32_t dtype;             /* aule_dtype */
    uint64_t rows_bh;          /* batch * heads */
    uint32_t seq, head_dim;    /* head_dim even (any size; 16-byte vector path when head_dim % 16 == 0) */
    uint32_t row_pitch;        /* elements per row, >= head_dim */
    uint32_t table_len;        /* rows of cos / sin; seq + pos_offset <= table_len */
    uint32_t table_pitch;      /* floats per table row; 0 = head_dim/2 */
    int32_t layout;            /* AULE_ROPE_* */
    int32_t inverse;
    uint32_t pos_offset;
    int32_t device;
    void* stream;
    const void* in;
    void* out;
    const float* cos;          /* [table_len, head_dim/2] fp32 */
    const float* sin;
} aule_rope_desc;
int32_t aule_rope_ex(const aule_rope_desc* desc);

/* Paged KV cache append (additive; the write side of aule_attention_paged_decode_ex / _fp8_ex).  One launch writes the K  */
/* and V rows of num_tokens new tokens into the [num_blocks, block_size, heads_kv, head_dim] caches:                          */
/*     row slot_mapping[t] (= block * block_size + offset) of k_cache / v_cache  <-  key[t], value[t]                         */
/* key / value are [num_tokens, heads_kv, head_dim] fp16 / bf16 with a contiguous last dimension and free token and head      */
/* strides (in elements, separate for key and value: slices of a fused QKV projection and transposed [B, H, S, D] views need   */
/* no copy).  A slot that is negative (vLLM's padding) or >= num_blocks * block_size is skipped: that token is neither read   */
/* nor written.  Two tokens of one call with the same slot: which of them the cache holds afterwards is unspecified.          */
/* cache_dtype AULE_KV_CACHE_SAME: the caches hold the input's dtype, rows are copied bit for bit; k_scale / v_scale must be   */
/* NULL.  AULE_KV_CACHE_FP8_E4M3: the caches hold OCP e4m3fn codes,                                                            */
/*     code = cast_e4m3fn(clamp(x / scale[hk], -448, 448))                                                                    */
/* -- correctly rounded fp32 division, round to nearest even (subnormals included), saturating, NaN stays a NaN code, -0      */
/* stays -0 -- with k_scale / v_scale [heads_kv] fp32 DEVICE arrays read by the kernel (no host synchronisation).             */
/* Optional rotation of K only (all of cos, sin, positions given; all NULL with table_len = table_pitch = 0: none):           */
/* AULE_ROPE_HALF pairs, token t uses table row positions[t]; aule_rope_ex's arithmetic, rounded once to the input's dtype    */
/* and only then quantised, so the result equals aule_rope_ex() followed by the un-rotated append bit for bit.  A token        */
/* whose slot is skipped needs no valid position; a position outside [0, table_len) skips the token.                          */
/* Alignment: key, value, the caches, cos and sin 16-byte aligned; the four strides multiples of 8; table_pitch % 4 == 0.     */
/* Asynchronous on `stream`; device pointers; captures into a hipGraph (no allocation, no synchronisation).                  */
#define AULE_KV_CACHE_SAME 0      /* caches of the input's 16-bit dtype */
#define AULE_KV_CACHE_FP8_E4M3 1  /* caches of OCP e4m3fn codes + per-KV-head scales */
typedef struct aule_kv_append_desc {
    uint32_t struct_size;      /* = sizeof(aule_kv_append_desc) = 168 */
    int32_t dtype;             /* of key / value: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* AULE_KV_CACHE_* */
    uint32_t num_tokens;       /* 0: returns 0 without a launch */
    uint32_t heads_kv;
    uint32_t head_dim;         /* 32, 64 or 128 */
    uint32_t num_blocks;
    uint32_t block_size;       /* any value > 0 */
    int64_t key_token_stride;  /* offset 32; elements, >= head_dim */
    int64_t key_head_stride;   /* elements, >= head_dim */
    int64_t value_token_stride;
    int64_t value_head_stride;
    uint32_t table_len;        /* offset 64; rows of cos / sin (0 without rotation) */
    uint32_t table_pitch;      /* floats per table row; 0 = head_dim/2 */
    int32_t device;            /* HIP device ordinal, -1 = current */
    uint32_t reserved;         /* 0 */
    void* stream;              /* offset 80; hipStream_t */
    const void* key;           /* [num_tokens, heads_kv, head_dim] */
    const void* value;
    void* k_cache;             /* offset 104; [num_blocks, block_size, heads_kv, head_dim], contiguous */
    void* v_cache;
    const int64_t* slot_mapping;   /* offset 120; [num_tokens] */
    const float* k_scale;      /* [heads_kv] fp32 (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const float* v_scale;
    const float* cos;          /* offset 144; [table_len, head_dim/2] fp32, or NULL */
    const float* sin;
    const int64_t* positions;  /* offset 160; [num_tokens], or NULL */
} aule_kv_append_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_kv_cache_append_ex(const aule_kv_append_desc* desc);

/* Latent cache append (additive; the write side of aule_attention_mla_paged_ex / _fp8_ex).  One launch writes the latent rows of    */
/* total_tokens new tokens into the [num_blocks, block_size, 576] cache:                                                              */
/*     row slot_mapping[t] of kv_cache viewed as [num_blocks * block_size, 576]  <-  [ c_kv[t] | rope(k_pe[t]) ]                      */
/* c_kv is [total_tokens, 512] and k_pe [total_tokens, 64], fp16 / bf16, last dimension contiguous, each with a free token stride in  */
/* elements (a multiple of 8, >= the row): slices of the fused down-projection's output are read in place.                            */
/* A slot that is negative (padding) or >= num_blocks * block_size skips the token ENTIRELY: nothing of its row is written, the c_kv  */
/* part included.  Two tokens of one call with the same slot: which of them the cache holds afterwards is unspecified.                */
/* cache_dtype AULE_KV_CACHE_SAME: the cache holds the input's dtype, the bits are copied; kv_scale must be NULL.                     */
/* AULE_KV_CACHE_FP8_E4M3: the cache holds OCP e4m3fn codes, code = cast_e4m3fn(clamp(x / kv_scale[0], -448, 448)) by the rules of    */
/* aule_kv_cache_append_ex (correctly rounded division, round to nearest even, saturating, NaN stays NaN, -0 stays -0), kv_scale a    */
/* DEVICE array of 1 fp32 read by the kernel.                                                                                         */
/* Optional rotation of k_pe (all of cos, sin, positions given with table_len > 0; all NULL with table_len = table_pitch = 0: none):  */
/* tables [table_len, 32] fp32 with table_pitch floats per row (0 = 32), token t uses row positions[t]; rope_layout AULE_ROPE_HALF    */
/* pairs (p, p + 32), AULE_ROPE_INTERLEAVED pairs (2p, 2p + 1); aule_rope_ex's arithmetic, rounded once to the input's dtype and only */
/* then quantised: the result equals aule_rope_ex() followed by the un-rotated append bit for bit.  With rotation, a position outside */
/* [0, table_len) skips the token entirely as a bad slot does; a token whose slot is skipped needs no valid position.                 */
/* Alignment: c_kv, k_pe, kv_cache, cos and sin 16-byte aligned; kv_scale 4-byte; table_pitch % 4 == 0.                                */
/* Asynchronous on `stream`; device pointers; captures into a hipGraph (no allocation, no synchronisation).  The descriptor is       */
/* checked before the device is needed: -3 for a refused one and 0 for total_tokens = 0 are answered without aule_init().             */
typedef struct aule_mla_kv_append_desc {
    uint32_t struct_size;      /* = sizeof(aule_mla_kv_append_desc) = 128 */
    int32_t dtype;             /* offset 4; of c_kv / k_pe: AULE_DTYPE_F16 or AULE_DTYPE_BF16 */
    int32_t cache_dtype;       /* offset 8; AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3 */
    int32_t rope_layout;       /* offset 12; AULE_ROPE_HALF or AULE_ROPE_INTERLEAVED (read with rotation only, but always checked) */
    uint32_t total_tokens;     /* offset 16; 0: returns 0 without a launch */
    uint32_t num_blocks;       /* offset 20 */
    uint32_t block_size;       /* offset 24; any value > 0 */
    uint32_t table_len;        /* offset 28; rows of cos / sin (0 without rotation) */
    uint32_t table_pitch;      /* offset 32; floats per table row; 0 = 32 */
    int32_t device;            /* offset 36; HIP device ordinal, -1 = current */
    int64_t c_kv_token_stride; /* offset 40; elements, >= 512, a multiple of 8 */
    int64_t k_pe_token_stride; /* offset 48; elements, >= 64, a multiple of 8 */
    void* stream;              /* offset 56; hipStream_t */
    const void* c_kv;          /* offset 64; [total_tokens, 512] */
    const void* k_pe;          /* offset 72; [total_tokens, 64] */
    void* kv_cache;            /* offset 80; [num_blocks, block_size, 576], contiguous */
    const int64_t* slot_mapping;   /* offset 88; [total_tokens] */
    const float* kv_scale;     /* offset 96; [1] fp32, device (AULE_KV_CACHE_FP8_E4M3), else NULL */
    const float* cos;          /* offset 104; [table_len, 32] fp32, or NULL */
    const float* sin;          /* offset 112 */
    const int64_t* positions;  /* offset 120; [total_tokens], or NULL */
} aule_mla_kv_append_desc;
/* 0 ok; -1 uninitialised; -3 invalid/unsupported arguments; -4 launch failure. */
int32_t aule_mla_kv_append_ex(const aule_mla_kv_append_desc* desc);

/* Attention with the query rotation fused into the kernel (additive; inference path).  Replaces the Q half of       */
/* python/aule/triton_flash.py:112-131 (the reference rotates Q in its forward prologue); K must arrive rotated --   */
/* once per key by aule_rope_ex(), e.g. when it is appended to a KV cache -- because the tiled kernel re-reads every */
/* K tile once per 256 query rows and would repeat the rotation each time.  Q is read un-rotated and */
/* rotated in registers with exactly aule_rope_ex()'s arithmetic and rounding: the result is bit-identical to        */
/* aule_rope_ex(Q) followed by aule_attention_forward_ex(), minus one read and one write of Q.  Taken only by the    */
/* persistent forward kernel: fp16 / bf16, head_dim 64 or 128, AULE_ROPE_HALF, 16-byte aligned tables with           */
/* table_pitch % 4 == 0, no sliding window other than a causal one of >= 128 keys (round 6: the kernel's window     */
/* instances) -- ask aule_attention_forward_rope_fusable() (host logic only; 1 = yes)                               */
/* and fall back to the two calls otherwise; aule_attention_forward_rope_ex() returns -3 for other configurations.   */
typedef struct aule_attn_rope {
    uint32_t struct_size;      /* = sizeof(aule_attn_rope) */
    int32_t layout;            /* AULE_ROPE_HALF */
    uint32_t table_len;        /* rows of cos / sin; seq_q + q_pos_offset <= table_len */
    uint32_t table_pitch;      /* floats per table row; 0 = head_dim/2 */
    uint32_t q_pos_offset;     /* query i uses table row i + q_pos_offset (seq_k - seq_q for bottom-right causal) */
    uint32_t reserved;
    const float* cos;          /* [table_len, head_dim/2] fp32 */
    const float* sin;
} aule_attn_rope;
int32_t aule_attention_forward_rope_ex(const aule_attn_desc* desc, const aule_attn_rope* rope);
int32_t aule_attention_forward_rope_fusable(const aule_attn_desc* desc, const aule_attn_rope* rope);

uint64_t aule_attention_backward_workspace_size(const aule_attn_bwd_desc* desc);

/* Build/ABI identification: "aule-hip gfx950 <abi>" */
const char* aule_hip_build_info(void);
/* Debug (not part of the drop-in ABI): forward kernel aule_attention_forward_ex would pick for `desc` --        */
/* 0 fp32, 1 ping-pong, 4 split-KV, 5 tiled split, 7 one wave per SIMD over key-range pieces, 8 one wave per SIMD,  */
/* 9 the head_dim 256 kernel (16-bit); -3 bad.                                                                       */
/* Host logic only, no aule_init().                                                                                  */
int32_t aule_hip_debug_forward_route(const aule_attn_desc* desc);
/* Debug: the route of the most recent forward launch of this process (the same codes); 0 before the first.          */
int32_t aule_hip_debug_last_forward_route(void);
/* Debug: the launch plan of aule_attention_forward_ex(desc) (csrc/fa_fwd_plan.h) as integers -- out = {route, workspace */
/* bytes low 32 bits, high 32 bits, then the chosen route's own plan: 0 {key-range pieces per Q block}; 4 {32-row tiles   */
/* per unit, key tiles per wave, workgroups along the keys, partials per row, partial rows}; 5 {heads per KV head, packed */
/* rows, Q blocks, base workgroups, key tiles, KV splits, keys per split, 32-row tiles per unit}; 7 {pieces n, pairs, Q   */
/* blocks, work items}; 8 {paired, work per head, work items, workgroups, rounds, heads per round}; 1 and 9 nothing}.     */
/* Returns the ints written (negative: the capacity needed); -3 bad.  Host logic only, no aule_init().                    */
int32_t aule_hip_debug_forward_plan(const aule_attn_desc* desc, int32_t* out, int32_t cap);
/* Debug: the launch plan of the shared-prefix kernel of aule_attention_paged_cascade_ex(desc) as integers -- out = {row blocks    */
/* of 128 packed rows, 64-key tiles of the prefix table's capacity, nsplit, tiles per split, workgroups, workspace bytes low 32     */
/* bits, high 32 bits}: split k owns tiles [k * tiles per split, min((k + 1) * tiles per split, tiles)).  Returns the ints written  */
/* (negative: the capacity needed), 0 for a descriptor with nothing to do; -3 bad.  Host logic only, no aule_init(), no pointer of  */
/* the descriptor is read.                                                                                                         */
int32_t aule_hip_debug_shared_prefix_plan(const aule_paged_cascade_desc* desc, int32_t* out, int32_t cap);
/* Debug: the launch plan of aule_attention_mla_paged_ex(desc) as integers -- out = {row blocks, rows per block (64), nsplit,       */
/* workgroups (row blocks * nsplit * batch), workspace bytes low 32 bits, high 32 bits}.  Returns the ints written (negative: the   */
/* capacity needed), 0 for a descriptor with nothing to do; -3 bad.  Host logic only, no aule_init(), no pointer of the descriptor  */
/* is read (the pointer rules of the launch are not applied); without a device it plans for 256 compute units.                      */
int32_t aule_hip_debug_mla_plan(const aule_mla_paged_desc* desc, int32_t* out, int32_t cap);
/* Debug: the launch plan of aule_attention_mla_sparse_ex(desc) as integers -- out = {row blocks (ceil(heads_q / 64)), rows per     */
/* block (64), nsplit, workgroups (total_tokens * row blocks * nsplit), workspace bytes low 32 bits, high 32 bits}.  Returns the    */
/* ints written (negative: the capacity needed), 0 for a descriptor with nothing to do; -3 bad.  Host logic only, no aule_init(),   */
/* no pointer of the descriptor is read (the pointer and workspace rules of the launch are not applied); without a device it plans  */
/* for 256 compute units.                                                                                                           */
int32_t aule_hip_debug_mla_sparse_plan(const aule_mla_sparse_desc* desc, int32_t* out, int32_t cap);
/* Debug: aule_attention_mla_sparse_ex(desc) with `nsplit` key ranges instead of the plan's, clamped to 1 .. min(64, ceil(topk /    */
/* 64)); nsplit < 1: -3.  Every other rule and return value of the entry; a caller workspace is sized for this nsplit.  For the     */
/* bench that measures the plan's "one split per two tiles" cap (tools/bench_mla_sparse.py); results equal the entry's within the   */
/* forward bounds, bit for bit only at the plan's own nsplit.                                                                       */
int32_t aule_hip_debug_mla_sparse_launch_nsplit(const aule_mla_sparse_desc* desc, int32_t nsplit);
/* Debug: the launch plan of aule_mla_indexer_logits_ex(desc) as integers -- out = {tokens per group (4), token groups              */
/* (ceil(max_seqlen_q / 4); plain decode: 1), keys per chunk (a multiple of 128), key chunks, workgroups (batch * token groups *    */
/* key chunks)}.  Chunk c owns columns [c * keys per chunk, ...) cut at W, so every (token group, column) has one owner.  Returns   */
/* the ints written (negative: the capacity needed), 0 for a descriptor with nothing to do; -3 bad.  Host logic only, no            */
/* aule_init(), no pointer of the descriptor is read (the pointer rules of the launch are not applied); without a device it plans   */
/* for 256 compute units.                                                                                                           */
int32_t aule_hip_debug_mla_indexer_plan(const aule_mla_indexer_logits_desc* desc, int32_t* out, int32_t cap);
/* Debug: the launch plan of aule_attention_mla_prefill_backward_ex(desc) as integers -- out = {heads per chunk, n_chunks (the last    */
/* chunk may be short), the bound of n_chunks (16), delta workgroups, dQ workgroups, dK/dV workgroups (key blocks * batch * n_chunks),  */
/* reduce workgroups, 1 if the reduce runs (else the dK/dV kernel writes dk_pe itself), workspace bytes low 32 bits, high 32 bits}.     */
/* Returns the ints written (negative: the capacity needed), 0 for a descriptor with nothing to do; -3 bad.  Host logic only, no       */
/* aule_init(), no pointer of the descriptor is read; without a device it plans for 256 compute units.                                 */
int32_t aule_hip_debug_mla_prefill_backward_plan(const aule_mla_prefill_bwd_desc* desc, int32_t* out, int32_t cap);
/* Debug: bit mask of the kernels the most recent backward launch of this process ran -- 1 the 5-matmul mode (delta pass, dK/dV kernel  */
/* spilling its dS, dQ = dS K), 2 / 4 the one-wave-per-SIMD dQ / dK/dV kernel, 8 / 16 their two-waves-per-SIMD predecessors, 32 the    */
/* fp32 kernels, 64 (with 4) the D = 64 dK/dV instance with two key blocks per wave, 128 the head_dim 256 kernels (with 32 for fp32);  */
/* 0 before the first backward.  Lets a test assert                                                                                   */
/* the mode a shape takes by itself.                                                                                      */
int32_t aule_hip_debug_last_backward_route(void);
/* Debug: the same bit mask (BwdRoute, csrc/fa_bwd_plan.h) for the call aule_attention_backward_ex(desc) WOULD make with                */
/* desc->workspace_bytes bytes of workspace: the launch plan, not a launch.  -3 for a descriptor that call refuses on shape grounds       */
/* (struct_size, dtype, head_dim, head ratio, causal code, workspace_bytes below the minimum).  Host logic only, no aule_init(), no      */
/* pointer of the descriptor is read.                                                                                                 */
int32_t aule_hip_debug_backward_route(const aule_attn_bwd_desc* desc);
/* Debug: the causal-split plan of route 7 (small causal grids) as integers -- out = {pieces n, pairs, then per pair of   */
/* Q blocks: tiles of the far block, of the near block, cut positions b[0..8]}; returns the ints written (negative: the */
/* capacity needed), 0 when the shape does not take that route.  Host logic only.                                       */
int32_t aule_hip_debug_forward_split_plan(const aule_attn_desc* desc, int32_t* out, int32_t cap);
/* Debug: the work item of workgroup `bid` of a grid of batch * heads_q * nblk workgroups -- out4 = {batch, kv head, q head,  */
/* block}.  ranked = 0: unit by unit (flag: last block first), the 16-bit kernels; ranked = 1: block rank by block rank over  */
/* all units (flag: descending), the fp32 kernels.  Host logic only; -3 on a bad argument.                                    */
/* Debug: the run-time switches the library resolved from this process's environment (docs/SWITCHES.md; read once, on first use) as     */
/* text, one line per switch: NAME=<value>\n with stable words (auto|recompute|spill, default|old|new, default|pp, integers, ...); an    */
/* unset or unrecognised setting prints as the default it resolves to.  Writes at most cap bytes (NUL-terminated) and returns the bytes   */
/* the whole text needs, NUL included.  No lock, no device, no aule_init().                                                               */
uint64_t aule_hip_debug_switches(char* buf, uint64_t cap);
int32_t aule_hip_debug_work_order(int32_t ranked, int32_t bid, int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t nblk, int32_t flag, int32_t* out4);

/* ---- Direct peer exchange between the per-GPU processes of one node (additive; no counterpart in the reference, which  */
/* is single-device: SURVEY.md 8e).  A rank allocates its receive buffer here, publishes the 64-byte handle by any means    */
/* (aule.dist uses the process group), opens its peers' handles, and copies pieces of its output straight into their        */
/* buffers over xGMI -- no RCCL algorithm choice in the data path.  Every call: 0, or -1 bad argument / -2 allocation /     */
/* -4 HIP error with the text in aule_get_error().  No aule_init() needed; `device` < 0 = the current device.               */
typedef struct aule_ipc_handle { unsigned char bytes[64]; } aule_ipc_handle;   /* = hipIpcMemHandle_t */
int32_t aule_peer_alloc(int32_t device, uint64_t bytes, void** ptr, aule_ipc_handle* handle);   /* hipMalloc + hipIpcGetMemHandle */
int32_t aule_peer_free(int32_t device, void* ptr);
int32_t aule_peer_open(int32_t device, const aule_ipc_handle* handle, void** ptr);              /* another process's buffer, mapped here */
int32_t aule_peer_close(int32_t device, void* ptr);
/* dst / src: device pointers (local, or a peer's from aule_peer_open) + byte offsets applied by the caller; asynchronous on */
/* `stream` (a hipStream_t of `device`).                                                                                      */
int32_t aule_peer_copy_async(int32_t device, void* dst, const void* src, uint64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AULE_H */
