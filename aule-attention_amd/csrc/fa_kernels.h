// fa_kernels.h -- host-visible launch interface of the gfx950 attention kernels.
//
// Plain C++ (no torch, no HIP types beyond hipStream_t) so that aule_capi.cpp
// can call the launchers.  Every launcher is asynchronous on `stream` and
// returns a hipError_t-compatible int (0 = success).
//
// Tensor layout (row-major contiguous, as the reference's Triton path makes
// them: python/aule/triton_flash_amd.py:404-407):
//   Q, O, dO, dQ : [B, Hq,  Sq, D]      K, V, dK, dV : [B, Hkv, Sk, D]
//   LSE, delta   : [B, Hq, Sq] fp32
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <atomic>

namespace aule_hip {

enum DType : int { kF32 = 0, kF16 = 1, kBF16 = 2 };

struct FwdArgs {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;  // may be null
    int B, Hq, Hkv, Sq, Sk, D;
    float scale;  // softmax scale (already defaulted by the caller)
    int causal;
    int dtype;
    int window = -1;  // sliding window: key j visible to query i only if i - j < window (<= 0: off)
    int coff = 0;     // causal position offset: query i sits at position i + coff (0 = the reference's top-left
                      // rule; Sk - Sq = bottom-right alignment); also shifts the window
    // Partials of the two-launch short-query paths: the caller's buffer when it is large enough (no allocation at
    // all -- what a hipGraph capture wants: hipMallocAsync / hipFreeAsync become graph nodes that cost more than the
    // kernels of a decode step), otherwise a stream-ordered allocation.
    void* ws = nullptr;
    uint64_t ws_bytes = 0;
    // Fused query rotation (fwd_rope_fusable() shapes only): Q is rotated on its way into the kernel's registers with the
    // half-split pairs of rope_gfx950.hip; K must arrive rotated.  Tables [rope_rows, rope_pitch] fp32, query i -> row i + rope_pos.
    const float* rope_cos = nullptr;
    const float* rope_sin = nullptr;
    int rope_rows = 0, rope_pitch = 0, rope_pos = 0;
    int device = -1;   // the descriptor's device ordinal (-1: the current device): the grid-sizing queries ask THAT device's CU
                       // count, also from the entry points that never switch devices (workspace size, route, fusable)
};

// Compute units of `device` (-1: the current one), asked once per device id and process: launch paths call this several times
// per launch (route, plan, grid).
inline int device_cu_count(int device) {
    static std::atomic<int> cached[64];   // (zero-initialised; API threads may race to fill an entry with the same value)
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev < 0 || dev >= 64) return 256;
    const int have = cached[dev].load(std::memory_order_relaxed);
    if (have > 0) return have;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

// The workspace of one launch: the caller's buffer, or hipMallocAsync / hipFreeAsync on the launch stream.
struct ScopedWorkspace {
    void* ptr = nullptr;
    bool owned = false;
    hipStream_t stream;
    hipError_t err = hipSuccess;
    ScopedWorkspace(size_t bytes, void* user, uint64_t user_bytes, hipStream_t s) : stream(s) {
        if (user != nullptr && user_bytes >= bytes && (reinterpret_cast<uintptr_t>(user) & 15) == 0) {
            ptr = user;
            return;
        }
        err = hipMallocAsync(&ptr, bytes, s);
        owned = err == hipSuccess;
    }
    ~ScopedWorkspace() {
        if (owned) (void)hipFreeAsync(ptr, stream);
    }
    ScopedWorkspace(const ScopedWorkspace&) = delete;
    ScopedWorkspace& operator=(const ScopedWorkspace&) = delete;
};

struct BwdArgs {
    const void* q;
    const void* k;
    const void* v;
    const void* o;
    const void* dout;
    const float* lse;
    void* dq;
    void* dk;
    void* dv;
    float* delta;  // the workspace (layout and sizes: BwdPlan, fa_bwd_plan.h): delta [B,Hq,Sq] fp32 first
    const float* lse2 = nullptr;   // internal (16-bit path): L' = LSE log2(e) [B,Hq,Sq], published by the dQ kernel behind delta
    const float* ndelta = nullptr; // internal (16-bit path): - delta, behind L' (the C operand the one-wave-per-SIMD dK/dV kernel starts dP from)
    int B, Hq, Hkv, Sq, Sk, D;
    float scale;
    int causal;
    int dtype;
    int window = -1;  // as FwdArgs::window (the reference's backward ignores it; this one honours it)
    int coff = 0;     // as FwdArgs::coff
    unsigned long long* dbg = nullptr;   // debug: s_memtime stamps of the dK/dV kernel's workgroup 0 (bf16 D128 causal)
    unsigned long long* dbg_dq = nullptr;   // ... of the dQ kernel's workgroup 0
    void* ds = nullptr;            // internal (16-bit path, 5-matmul backward): the dS workspace of this call's batch chunk (DsLayout)
    uint64_t ws_bytes = 0;         // bytes behind `delta` (0 = just BwdPlan::min_bytes: the recompute pair runs)
    uint64_t ws_floor = 0;         // the dS room starts no lower than this: the minimum of the problem as the caller stated and sized it (aule_capi.cpp: fill_bwd_args)
    bool dkv4_k2 = false;          // internal (launch_bwd_dkv4, D = 64): BwdPlan::k2, the two-key-blocks-per-wave instance
    int device = -1;               // the descriptor's device ordinal (-1: the current one): the grid-sizing rules ask THAT device's CU count (as FwdArgs::device)
};

// The dS workspace of the 5-matmul backward (round 5; fa_bwd_dkv4_gfx950.hip SPILL instances write it, fa_bwd_dqs_gfx950.hip reads it).
// A UNIT is the packed 16-bit dS of one (32-key block, 32-row query block) tile exactly as the dK/dV kernel holds it for its own
// dK MFMAs: 2 KB = [kk = 16-row query step][lane = key n + 32 hi][16 bytes = query rows 16 kk + 4 hi + {0..3}, 16 kk + 8 + 4 hi + {0..3}].
// Units of one (batch, KV head) GROUP and one 32-key block kb32 form a COLUMN of xs = g * nq32 units in the dK/dV kernel's stream
// order -- block-major, head-minor since round 6: query block qb32 of head hh of the group -> x = g * qb32 + hh -- so that the
// writer's address is its loop counter (its stream starts at the first query block fq that sees the 128-key block: x0 = g * fq).
// Columns are padded to whole 128-key blocks (nkb32p = 4 * ceil(Sk / 128)): every wave of the dK/dV kernel owns a column.
struct DsLayout {
    int nq32, nkb32p;
    long long xs;              // units per column
    long long group_bytes;     // nkb32p * xs * 2048
    static DsLayout of(int Hq, int Hkv, int Sq, int Sk) {
        DsLayout l;
        l.nq32 = (Sq + 31) / 32;
        l.nkb32p = 4 * ((Sk + 127) / 128);
        l.xs = (long long)(Hq / (Hkv > 0 ? Hkv : 1)) * l.nq32;
        l.group_bytes = (long long)l.nkb32p * l.xs * 2048;
        return l;
    }
};

// Paged-KV decode (python/aule/triton_flash_amd.py:543-737): one query token per sequence.
//   q, out : [B, Hq, D]      k_cache, v_cache : [num_blocks, block_size, Hkv, D]   (16-bit dtypes)
//   block_tables : [B, max_blocks] int32 (physical block of each logical block), context_lens : [B] int32
// FP8 caches (cache_kind = kCacheFp8E4M3): k_cache / v_cache hold OCP e4m3fn codes, one byte per element, and
//   K = k_scale[hk] * code, V = v_scale[hk] * code with k_scale, v_scale : [Hkv] fp32 on the device; q / out stay 16-bit.
enum CacheKind : int { kCache16 = 0, kCacheFp8E4M3 = 1 };
struct PagedArgs {
    const void* q;
    const void* k_cache;
    const void* v_cache;
    void* out;
    const int* block_tables;
    const int* context_lens;
    int B, Hq, Hkv, D;
    int block_size, max_blocks;
    float scale;
    int window;   // > 0: attend only to the last `window` positions (context_len - 1 - pos < window)
    int dtype;
    void* ws = nullptr;             // as FwdArgs::ws / ws_bytes
    uint64_t ws_bytes = 0;
    int cache_kind = kCache16;          // element type of the caches (dtype is the type of q / out)
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only
    const float* v_scale = nullptr;
    // launch_paged_query only (launch_paged_decode reads neither): Sq query tokens per sequence, q / out [B, Hq, Sq, D], the last Sq
    // positions of each sequence -- query i at position context_len - Sq + i sees the keys at or before it (and inside the window
    // measured from there); a query at a negative position gives zeros.  lse [B, Hq, Sq] fp32 or null (-inf where no key is seen)
    int Sq = 1;
    float* lse = nullptr;
    // launch_paged_query only: per-head sink logits [Hq] fp32 on the device, or null -- a raw logit (not scaled) that
    // joins the softmax denominator and carries no value; a row that sees no key then gives out = 0 and lse = sinks[head]
    const float* sinks = nullptr;
    // launch_paged_query only: a tree of new tokens instead of a chain.  [B, Sq] int64 words on the device or null; query i
    // sees every context key (j < context_len - Sq) and new token t (key context_len - Sq + t) iff bit t of word (b, i) is set.  No window,
    // no sinks (-1).  The chain words (2 << i) - 1 give the bits of the call without a tree
    const long long* tree_mask = nullptr;
};

// Rotary embedding pass (rope_gfx950.hip): x [nheads, S, D] with `pitch` elements per row, tables [>= S + pos_offset, D/2]
// fp32; layout 0 = half-split pairs (p, p + D/2), 1 = interleaved pairs (2p, 2p + 1); in == out is allowed.
struct RopeArgs {
    const void* in;
    void* out;
    const float* cos;
    const float* sin;
    long long nheads;   // B * H
    int S, D, pitch;
    int layout, inverse, pos_offset;
    int dtype;
    int table_pitch = 0;   // floats per table row; 0 = D/2
};
int launch_rope(const RopeArgs& a, hipStream_t stream);

// Paged KV cache append (kv_append_gfx950.hip): key / value [T, Hkv, D] 16-bit with free token / head strides (elements, last
// dimension contiguous) -> row slot_mapping[t] of k_cache / v_cache [num_blocks, block_size, Hkv, D], which hold either the
// input's dtype (kCache16: a copy) or e4m3fn codes of x / scale[hk] (kCacheFp8E4M3).  cos != null: K is rotated first (half-split
// pairs, table row positions[t]).  Slots outside [0, num_blocks * block_size) are skipped.  The caller guarantees 16-byte aligned
// pointers, strides % 8 == 0 and table_pitch % 4 == 0.
struct KvAppendArgs {
    const void* key;
    const void* value;
    void* k_cache;
    void* v_cache;
    const long long* slot_mapping;   // [T] int64
    int T, Hkv, D;
    long long num_blocks;
    int block_size;
    long long k_token_stride, k_head_stride, v_token_stride, v_head_stride;
    int dtype;                          // of key / value: kF16 or kBF16
    int cache_kind = kCache16;
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only: [Hkv] fp32
    const float* v_scale = nullptr;
    const float* cos = nullptr;         // [table_len, D/2] fp32, table_pitch floats per row (0 = D/2)
    const float* sin = nullptr;
    const long long* positions = nullptr;   // [T] int64
    long long table_len = 0;
    int table_pitch = 0;
};
int launch_kv_append(const KvAppendArgs& a, hipStream_t stream);   // -1: unsupported arguments

// Latent cache append (mla_kv_append_gfx950.hip), the write side of the paged MLA: row slot_mapping[t] of kv_cache
// [num_blocks * block_size, 576] <- [c_kv[t] (512) | rope(k_pe[t] (64), table row positions[t])], 16-bit inputs with free token strides
// (elements).  kCache16: the bits are copied; kCacheFp8E4M3: e4m3fn codes of x / kv_scale[0] (launch_kv_append's rules).  cos != null:
// k_pe is rotated first, rope_layout 0 = pairs (p, p + 32), 1 = pairs (2p, 2p + 1); tables [table_len, 32] fp32.  A slot outside
// [0, num_blocks * block_size), or with rotation a position outside [0, table_len), skips the whole token.  The caller guarantees
// 16-byte aligned pointers, strides % 8 == 0 and table_pitch % 4 == 0.
struct MlaKvAppendArgs {
    const void* c_kv;
    const void* k_pe;
    void* kv_cache;
    const long long* slot_mapping;   // [T] int64
    int T;
    long long num_blocks;
    int block_size;
    long long c_kv_token_stride, k_pe_token_stride;
    int dtype;                          // of c_kv / k_pe: kF16 or kBF16
    int cache_kind = kCache16;
    const float* kv_scale = nullptr;    // kCacheFp8E4M3 only: [1] fp32, device
    const float* cos = nullptr;         // [table_len, 32] fp32, table_pitch floats per row (0 = 32)
    const float* sin = nullptr;
    const long long* positions = nullptr;   // [T] int64
    long long table_len = 0;
    int table_pitch = 0;
    int rope_layout = 0;
};
int launch_mla_kv_append(const MlaKvAppendArgs& a, hipStream_t stream);   // -1: unsupported arguments

// Paged prefill (fa_fwd_paged_prefill_gfx950.hip): ragged per-sequence queries against the paged cache, one launch, no workspace.
//   q [T, Hq, D] 16-bit, the new tokens of all sequences packed along the first axis (q_token_stride elements between tokens, the
//   heads of a token contiguous), out [T, Hq, D] contiguous, lse [T, Hq] fp32 or null; caches, table, lengths and scales as PagedArgs;
//   cu_seqlens_q [B + 1] int32 on the device.  Sequence b: L = clamp(context_lens[b], 0, max_blocks * block_size),
//   s = clamp(cu[b], 0, T), e = clamp(cu[b + 1], s, T), n = min(e - s, max_seqlen_q); token i < n is row s + i, sits at position
//   L - n + i and sees the keys at or before it (and inside the window measured from there).  Rows outside every [s, s + n) are
//   never written.  The caller guarantees 16-byte aligned q / out / caches and q_token_stride % 8 == 0.
struct PagedPrefillArgs {
    const void* q;
    const void* k_cache;
    const void* v_cache;
    void* out;
    float* lse = nullptr;
    const int* block_tables;
    const int* context_lens;
    const int* cu_seqlens_q;
    int T, B, Hq, Hkv, D;
    int max_seqlen_q;
    long long q_token_stride;
    int block_size, max_blocks;
    float scale;
    int window;
    int dtype;
    int cache_kind = kCache16;
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only
    const float* v_scale = nullptr;
    const float* sinks = nullptr;       // [Hq] fp32 sink logits or null, as PagedArgs::sinks
    // [T] int64 words or null: a sequence with n <= 64 carries a tree -- token i sees every context key (j < L - n) and
    // new token t iff bit t of word s + i is set; a longer one keeps the causal rule and its words are not read.  No window, no sinks (-1)
    const long long* tree_mask = nullptr;
};
// workgroups of the launch: ceil(min(max_seqlen_q, T) * (Hq / Hkv) / 128) x Hkv x B (tests, tools)
long long paged_prefill_grid(const PagedPrefillArgs& a);
int launch_paged_prefill(const PagedPrefillArgs& a, hipStream_t stream);   // -1: unsupported arguments
// The same over an FP8 cache with both matrix products in FP8 (fa_fwd_paged_prefill_fp8mma_gfx950.hip): q is quantised per
// row in the kernel, K / V codes are multiplied as they are.  Same arguments, clamps and grid; -1 also for cache_kind != kCacheFp8E4M3,
// null scales, sinks, tree_mask and D outside {64, 128}.
int launch_paged_prefill_fp8mma(const PagedPrefillArgs& a, hipStream_t stream);

// Shared-prefix pass of the paged cascade (fa_fwd_paged_shared_prefix_gfx950.hip): every one of the T tokens of q sees the first
// P = clamp(prefix_len[0], 0, max_prefix_blocks * block_size) keys of ONE block table, no mask, no per-sequence data.  The rows of
// the whole batch are packed token-major per KV head (row r = token r / g, head hk g + r % g) and the keys are split into nsplit
// ranges of whole 64-key tiles; work item (KV head, 128 rows, split) writes the fp32 partial of its rows:
//   part [nsplit][T * Hq][D + 2]: un-normalised O (v_scale applied), m (log2 units), l -- row = token * Hq + head; a split that
//   holds no key of the prefix writes m = -inf, l = 0 and leaves O alone (a reader skips it).
struct SharedPrefixArgs {
    const void* q;
    const void* k_cache;
    const void* v_cache;
    float* part = nullptr;
    const int* prefix_block_table = nullptr;   // [max_prefix_blocks] int32
    const int* prefix_len = nullptr;           // [1] int32, device
    int T, Hq, Hkv, D;
    long long q_token_stride;
    int block_size, max_prefix_blocks;
    float scale;
    int dtype;
    int cache_kind = kCache16;
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only
    const float* v_scale = nullptr;
    int device = -1;                    // as FwdArgs::device
};
// The launch plan of the pass, and of the cascade's workspace: the one statement of the rule (launch, workspace query, debug hook).
// The key bound is the table's capacity -- prefix_len lives on the device and is not read here.
constexpr int kSharedPrefixMaxSplit = 32;
struct SharedPrefixPlan {
    int row_blocks = 0;        // ceil(T * g / 128)
    int tiles = 0;             // ceil(max_prefix_blocks * block_size / 64)
    int nsplit = 0;            // 1 .. kSharedPrefixMaxSplit, every split non-empty by capacity
    int tiles_per_split = 0;   // split k: tiles [k * tiles_per_split, min((k + 1) * tiles_per_split, tiles))
    long long grid = 0;        // row_blocks * Hkv * nsplit
    uint64_t part_bytes = 0;   // nsplit * T * Hq * (D + 2) * 4
    uint64_t lse_offset = 0;   // part_bytes rounded up to 16: the suffix LSE [T * Hq] fp32 of a cascade call without an lse buffer
    uint64_t ws_bytes = 0;     // lse_offset + T * Hq * 4, rounded up to 16
};
SharedPrefixPlan shared_prefix_plan(const SharedPrefixArgs& a);   // all zero: nothing to launch, or arguments the launch refuses
int launch_shared_prefix(const SharedPrefixArgs& a, const SharedPrefixPlan& plan, hipStream_t stream);   // -1: unsupported arguments

// Merges of attention states (fa_merge_states_gfx950.hip).
// Two states (out 16-bit [rows, D], lse fp32 [rows], natural log) into one; out may alias out_a or out_b, lse must not overlap
// lse_a or lse_b (the caller checks).  D % 8 == 0.
struct MergeStatesArgs {
    const void* out_a;
    const float* lse_a;
    const void* out_b;
    const float* lse_b;
    void* out;
    float* lse;
    long long rows;
    int D;
    int dtype;
};
int launch_merge_states(const MergeStatesArgs& a, hipStream_t stream);
// The cascade's merge: the nsplit partials of launch_shared_prefix into the suffix state (out, lse) launch_paged_prefill left, in
// place, for exactly the rows that launch wrote (its clamps of cu_seqlens_q / context_lens, own_capacity = max_blocks * block_size);
// a token at a negative own position keeps its zeros and -inf, a row whose prefix holds no key keeps its bits.
struct CascadeMergeArgs {
    const float* part;
    int nsplit;
    void* out;
    float* lse;
    const int* context_lens;
    const int* cu_seqlens_q;
    int T, B, Hq, D;
    int max_seqlen_q;
    int own_capacity;
    int dtype;
};
long long cascade_merge_grid(const CascadeMergeArgs& a);
int launch_cascade_merge(const CascadeMergeArgs& a, hipStream_t stream);

// Paged multi-head latent attention (fa_fwd_mla_paged_gfx950.hip): ragged queries q [T, Hq, 576] against ONE latent cache
//   kv_cache [num_blocks, block_size, 576] 16-bit of q's dtype (kCache16), or e4m3fn codes with ONE fp32 device scale (kCacheFp8E4M3:
//   key = kv_scale[0] * float(code), fa_fwd_mla_paged_fp8_gfx950.hip) -- row pos of a sequence is the key of all heads (576 elements) and,
//   in its first 512 elements, the value; out [T, Hq, 512] contiguous, lse [T, Hq] fp32 or null.  Table, lengths, cu_seqlens_q,
//   the clamps and the rows that are written as PagedPrefillArgs; cu_seqlens_q = null: sequence b owns row b, one token each
//   (T >= B).  The caller guarantees 16-byte aligned q / out / kv_cache and q_token_stride % 8 == 0.
struct MlaArgs {
    const void* q;
    const void* kv_cache;
    void* out;
    float* lse = nullptr;
    const int* block_tables;
    const int* context_lens;
    const int* cu_seqlens_q = nullptr;
    int T, B, Hq;
    int max_seqlen_q;                   // (1 with a null cu_seqlens_q)
    long long q_token_stride;
    int block_size, max_blocks;
    float scale;
    int dtype;
    int device = -1;                    // as FwdArgs::device
    int cache_kind = kCache16;          // element type of kv_cache (dtype is the type of q / out)
    const float* kv_scale = nullptr;    // kCacheFp8E4M3 only: [1] fp32, device
    // Tree masks (fa_fwd_mla_verify_gfx950.hip; the contract is aule_mla_paged_tree_desc): [T] int64 on the device, one word per packed
    // token -- a sequence with at most 64 new tokens sees the context and the new tokens its words name, a longer one stays causal.
    // Needs cu_seqlens_q; null: the causal chain.  Plan, workspace and combine do not depend on it.
    const long long* tree_mask = nullptr;
};
// The launch plan (mla_plan, beside the kernel: the one statement of the rule for launch, workspace query and debug hook).
constexpr int kMlaRows = 64;       // packed rows (token-major, head-minor) per workgroup
constexpr int kMlaMaxSplit = 64;   // key ranges per sequence, at most
struct MlaPlan {
    int row_blocks = 0;        // ceil(min(max_seqlen_q, T) * Hq / 64)
    int rows_per_block = 0;    // 64
    int nsplit = 0;            // 1 .. kMlaMaxSplit; split k of sequence b owns 64-key tiles [k * ceil(tiles(L_b) / nsplit), ...)
    long long grid = 0;        // row_blocks * nsplit * B
    uint64_t ws_bytes = 0;     // nsplit > 1: round16(nsplit * T * Hq * 514 * 4), else 0
};
MlaPlan mla_plan(const MlaArgs& a);   // all zero: nothing to launch; no pointer is read
int launch_mla_paged(const MlaArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream);   // -1: unsupported arguments

// Sparse latent attention (fa_fwd_mla_sparse_gfx950.hip): q [T, Hq, 576] against the rows of the latent cache that a per-token list
//   names -- indices [T, topk] int32, entry = a slot (row of the cache read as a flat [slots, 576] array); an entry outside [0, slots)
//   is skipped, a slot listed twice counts twice, and there is no causal rule.  Cache kinds, kv_scale, out, lse and the caller's
//   guarantees as MlaArgs.  The contract is aule_mla_sparse_desc in include/aule.h.
struct MlaSparseArgs {
    const void* q;
    const void* kv_cache;
    void* out;
    float* lse = nullptr;
    const int* indices;
    int T, Hq;
    int topk;                           // 1 .. kMlaSparseMaxTopk
    int slots;                          // num_blocks * block_size, 1 .. 2^31 - 1
    long long q_token_stride;
    float scale;
    int dtype;
    int device = -1;                    // as FwdArgs::device
    int cache_kind = kCache16;
    const float* kv_scale = nullptr;    // kCacheFp8E4M3 only: [1] fp32, device
};
constexpr int kMlaSparseMaxTopk = 65536;
// The launch plan (mla_sparse_plan, beside the kernel: the one statement of row blocks, nsplit, grid and workspace for launch, size
// query and debug hook).  MlaPlan's fields with a token in a sequence's place: row_blocks = ceil(Hq / 64) blocks of ONE token's heads,
// nsplit from ceil(topk / 64) tiles, grid = T * row_blocks * nsplit.  All zero: nothing to launch; no pointer is read.
// force_nsplit > 0 (the bench's debug entry alone, to measure what the rule's cap costs): that many ranges instead of the rule's,
// within 1 .. min(kMlaMaxSplit, tiles).
MlaPlan mla_sparse_plan(int T, int Hq, int topk, int device, int force_nsplit = 0);
int launch_mla_sparse(const MlaSparseArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream);   // -1: unsupported arguments

// The indexer of the sparse MLA (fa_mla_indexer_gfx950.hip): the index logits I[t, s] = sum_h w[t, h] * relu(q[t, h, :] . k[s, :]) of
//   ragged query tokens over a paged cache of index keys (one 128-wide row per position), and the top-k key list of every token.  The
//   tables, lengths, offsets and their device-side clamps are MlaArgs'; the contracts are aule_mla_indexer_logits_desc and
//   aule_mla_indexer_topk_desc in include/aule.h.
struct MlaIndexerArgs {
    const void* q;                      // [T, H, 128] 16-bit, q_token_stride elements per token
    const float* weights;               // [T, H]
    const void* k_cache;                // [num_blocks, block_size, 128]: q's dtype, or e4m3fn codes
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only: [num_blocks, block_size] fp32, device
    const int* block_tables;
    const int* context_lens;
    const int* cu_seqlens_q = nullptr;  // null: sequence b owns row b
    float* logits;                      // [T, logits_stride >= max_blocks * block_size]
    int T, B, H;
    int num_blocks, block_size, max_blocks;
    int max_seqlen_q;
    long long q_token_stride, logits_stride;
    int dtype;
    int device = -1;                    // as FwdArgs::device
    int cache_kind = kCache16;
};
constexpr int kMlaIndexerMaxHeads = 64;
constexpr int kMlaIndexerMaxTopk = 65536;
// The launch plan of the logits (mla_indexer_plan, beside the kernel: the one statement of the grid for the launch and the debug
// hook): work item (sequence, group of group_tokens tokens, chunk of chunk_keys keys), token_groups = ceil(max_seqlen_q /
// group_tokens), key_chunks * chunk_keys >= W = max_blocks * block_size, grid = B * token_groups * key_chunks.  From the shape alone;
// all zero: nothing to launch.
struct MlaIndexerPlan {
    int group_tokens = 0, token_groups = 0;
    int chunk_keys = 0, key_chunks = 0;
    long long grid = 0;
};
MlaIndexerPlan mla_indexer_plan(int B, int max_seqlen_q, long long W, int device);
int launch_mla_indexer_logits(const MlaIndexerArgs& a, const MlaIndexerPlan& plan, hipStream_t stream);   // -1: unsupported arguments
struct MlaIndexerTopkArgs {
    const float* logits;                // [T, logits_stride]
    int* indices;                       // [T, topk]
    const int* block_tables;
    const int* context_lens;
    const int* cu_seqlens_q = nullptr;
    int T, B, topk;
    int block_size, max_blocks;
    int max_seqlen_q;
    long long logits_stride;
    bool positions = false;             // raw positions instead of slots through the table
};
int launch_mla_indexer_topk(const MlaIndexerTopkArgs& a, hipStream_t stream);   // one workgroup per (sequence, token); -1: unsupported

// The cut of a sequence's length every ragged entry applies (paged prefill, variable-length, MLA prefill): no sequence has more
// tokens than the batch.
// I: int, or a descriptor's uint32_t fields compared as they stand (total < 2^30: the checkers) -- a max_seqlen of 2^31 or more cuts
// to the batch there, not to a negative number.
template <class I>
inline int seqlen_cut(I max_seqlen, I total) { return (int)(max_seqlen < total ? max_seqlen : total); }
// The kernels' block lookup (block_of, fa_device.h) shifts when the block size is a power of two: its shift, -1 for any other size
inline int shift_of(int block_size) { return (block_size & (block_size - 1)) == 0 ? __builtin_ctz((unsigned)block_size) : -1; }

// Variable-length packed batches (fa_fwd_varlen_gfx950.hip, fa_bwd_varlen_gfx950.hip): sequences of different lengths packed
// along one token axis, forward and backward.
//   q, out, dout, dq [Tq, Hq, D] and k, v, dk, dv [Tk, Hkv, D] 16-bit, lse / delta [Tq, Hq] fp32; the heads of a token contiguous,
//   q / k / v with their own token strides (elements), everything else contiguous; cu_seqlens_q / cu_seqlens_k [B + 1] int32 on the
//   device.  Sequence b: s_q = clamp(cu_q[b], 0, Tq), e_q = clamp(cu_q[b + 1], s_q, Tq), n = min(e_q - s_q, max_seqlen_q), and
//   s_k, e_k, L the same from cu_k, Tk, max_seqlen_k.  Query i < n is row s_q + i and sits at position i (causal 0, 1) or
//   i + L - n (causal 2); key j < L is row s_k + j and is visible iff (!causal || j <= pos) and, with a window W > 0, pos - j < W.
//   Rows outside every [s_q, s_q + n) / [s_k, s_k + L) are never written.  The caller guarantees 16-byte aligned tensors and
//   strides % 8 == 0.
struct VarlenArgs {
    const void* q;
    const void* k;
    const void* v;
    void* out = nullptr;          // forward: written
    float* lse = nullptr;         // forward: written (null: skipped); backward: read
    const void* o = nullptr;      // backward: the forward's out
    const void* dout = nullptr;
    void* dq = nullptr;
    void* dk = nullptr;
    void* dv = nullptr;
    float* delta = nullptr;       // backward workspace: [Tq, Hq] fp32
    const int* cu_seqlens_q;
    const int* cu_seqlens_k;
    int Tq, Tk, B, Hq, Hkv, D;
    int max_seqlen_q, max_seqlen_k;
    long long q_token_stride, k_token_stride, v_token_stride;
    float scale;
    int causal;                   // 0 none, 1 top-left, 2 bottom-right
    int window;
    int dtype;
    const float* sinks = nullptr; // [Hq] fp32 sink logits or null, as PagedArgs::sinks: the forward's epilogue and launch_varlen_dsinks
};
// The cuts the kernels and the grids run with
inline int varlen_max_sq(const VarlenArgs& a) { return seqlen_cut(a.max_seqlen_q, a.Tq); }
inline int varlen_max_sk(const VarlenArgs& a) { return seqlen_cut(a.max_seqlen_k, a.Tk); }
// The window the kernels run with: 0 (off) for window <= 0 and for a window that masks nothing -- no position differs from a key by
// min(max_seqlen_q, Tq) + min(max_seqlen_k, Tk) or more under any of the three causal modes -- so that "effectively off" values up to
// INT32_MAX never enter the kernels' range arithmetic.  The one statement of the rule, for both launchers.
inline int varlen_window(const VarlenArgs& a) {
    const long long span = (long long)varlen_max_sq(a) + varlen_max_sk(a);
    return a.window > 0 && a.window < span ? a.window : 0;
}
// What both launchers refuse: the head grouping, the causal mode, and token strides that overlap heads or break 16-byte rows.
inline bool varlen_args_ok(const VarlenArgs& a) {
    if (a.Hkv <= 0 || a.Hq % a.Hkv != 0 || a.causal < 0 || a.causal > 2) return false;
    if (a.q_token_stride < (long long)a.Hq * a.D || a.q_token_stride % 8 != 0) return false;
    if (a.k_token_stride < (long long)a.Hkv * a.D || a.k_token_stride % 8 != 0) return false;
    if (a.v_token_stride < (long long)a.Hkv * a.D || a.v_token_stride % 8 != 0) return false;
    return true;
}
// workgroups: forward and dQ ceil(min(max_seqlen_q, Tq) * (Hq / Hkv) / 128) x Hkv x B, dK/dV ceil(min(max_seqlen_k, Tk) / 128) x Hkv x B
long long varlen_fwd_grid(const VarlenArgs& a);
long long varlen_dkdv_grid(const VarlenArgs& a);
uint64_t varlen_bwd_workspace_bytes(long long Tq, int Hq);   // delta
int launch_varlen_fwd(const VarlenArgs& a, hipStream_t stream);   // -1: unsupported arguments
int launch_varlen_bwd(const VarlenArgs& a, hipStream_t stream);   // delta, dQ, dK/dV on `stream`
// The gradient of the sink logits (fa_bwd_sinks_gfx950.hip), after launch_varlen_bwd on the same stream: reads a.lse (the forward's, sinks
// included), a.delta (that launch's workspace), a.sinks and a.cu_seqlens_q over the owned rows only; two launches, no atomics, a fixed
// summation order; `partials` is varlen_dsinks_partial_bytes(a) bytes of workspace; exactly Hq floats of dsinks are written.
uint64_t varlen_dsinks_partial_bytes(const VarlenArgs& a);
int launch_varlen_dsinks(const VarlenArgs& a, float* dsinks, float* partials, hipStream_t stream);   // -1: unsupported arguments

// MLA prefill, the non-absorbed form (fa_fwd_mla_prefill_gfx950.hip): ragged 192 / 128 attention over a packed batch, forward only.
//   q [Tq, H, 192] with its token stride, k_nope and v [Tk, H, 128] each with a token AND a head stride, k_pe [Tk, 64] with its
//   token stride (all in elements); out [Tq, H, 128] contiguous, lse [Tq, H] fp32 or null.  Key row j of a sequence is
//   [k_nope[s_k + j, h] | k_pe[s_k + j]] for head h.  cu_seqlens_*, the clamps, the cuts, the positions and the visibility rule as
//   VarlenArgs with Hkv = Hq and no window.  The caller guarantees 16-byte aligned tensors and strides % 8 == 0.
struct MlaPrefillArgs {
    const void* q;
    const void* k_nope;
    const void* k_pe;
    const void* v;
    void* out = nullptr;
    float* lse = nullptr;         // null: skipped
    const int* cu_seqlens_q;
    const int* cu_seqlens_k;
    int Tq, Tk, B, H;
    int max_seqlen_q, max_seqlen_k;
    long long q_token_stride;
    long long k_nope_token_stride, k_nope_head_stride;
    long long v_token_stride, v_head_stride;
    long long k_pe_token_stride;
    float scale;
    int causal;                   // 0 none, 1 top-left, 2 bottom-right
    int dtype;
};
long long mla_prefill_grid(const MlaPrefillArgs& a);   // workgroups: ceil(min(max_seqlen_q, Tq) / 128) x H x B
int launch_mla_prefill(const MlaPrefillArgs& a, hipStream_t stream);   // -1: unsupported arguments

// Its backward (fa_bwd_mla_prefill_gfx950.hip): delta, dQ, dK/dV over head chunks and, with more than one chunk, the dk_pe reduce.
//   fwd states the problem (out and lse there are not read); o, dout [Tq, H, 128] and dq [Tq, H, 192] contiguous, lse [Tq, H] fp32,
//   dk_nope, dv [Tk, H, 128] each with a token AND a head stride (elements), dk_pe [Tk, 64] contiguous.
struct MlaPrefillBwdArgs {
    MlaPrefillArgs fwd;
    const void* o = nullptr;
    const float* lse = nullptr;
    const void* dout = nullptr;
    void* dq = nullptr;
    void* dk_nope = nullptr;
    void* dk_pe = nullptr;
    void* dv = nullptr;
    long long dk_nope_token_stride = 0, dk_nope_head_stride = 0;
    long long dv_token_stride = 0, dv_head_stride = 0;
};
constexpr int kMlaBwdMaxChunks = 16;   // head chunks of the dK/dV kernel, at most: the dk_pe planes take at most 16 * Tk * 64 * 4 bytes
struct MlaPrefillBwdPlan {
    int heads_per_chunk = 0;   // chunk c owns heads [c * heads_per_chunk, min(H, (c + 1) * heads_per_chunk))
    int n_chunks = 0;          // ceil(H / heads_per_chunk), 1 .. max_chunks
    int max_chunks = 0;        // kMlaBwdMaxChunks
    long long delta_grid = 0;  // ceil(Tq * H / 4)
    long long dq_grid = 0;     // ceil(min(max_seqlen_q, Tq) / 128) x H x B
    long long dkdv_grid = 0;   // ceil(min(max_seqlen_k, Tk) / 128) x B x n_chunks
    long long reduce_grid = 0; // ceil(min(max_seqlen_k, Tk) / 128) x B when the reduce runs, else 0
    bool reduce = false;       // n_chunks > 1: the chunks write fp32 planes and the reduce kernel writes dk_pe
    bool ok = true;            // false: a grid beyond 31 bits
    uint64_t delta_bytes = 0;  // [Tq, H] fp32 on a 256-byte boundary
    uint64_t ws_bytes = 0;     // delta_bytes + (reduce ? n_chunks * Tk * 64 * 4 : 0)
};
// all grids zero: nothing to launch; no pointer is read; `device` (-1: the current one) supplies the CU count
MlaPrefillBwdPlan mla_prefill_bwd_plan(int Tq, int Tk, int B, int H, int max_seqlen_q, int max_seqlen_k, int device);
int launch_mla_prefill_bwd(const MlaPrefillBwdArgs& a, const MlaPrefillBwdPlan& plan, void* ws, hipStream_t stream);   // -1: unsupported arguments

// Returns 0 on success, a hipError_t value on launch failure, -1 for an
// unsupported (dtype, D) combination.
int launch_paged_decode(const PagedArgs& a, hipStream_t stream);   // either cache_kind; kCacheFp8E4M3 with a null scale array is -1
int launch_paged_query(const PagedArgs& a, hipStream_t stream);    // ... with PagedArgs::Sq in 1 .. 64 tokens per sequence (else -1)
int launch_fwd(const FwdArgs& a, hipStream_t stream);
// merge partials [npart][B*Hkv*nrt*32][D+2] fp32 (un-normalised O, m in log2 units, l) into O / LSE (fa_fwd_splitkv_gfx950.hip)
int launch_splitkv_combine(const FwdArgs& a, float* part, int npart, int nrt, hipStream_t stream);
// FwdPlan::route of fwd_plan(a) (fa_fwd_plan.h: the plan, the workspace size): 0 fp32, 1 ping-pong, 4 split-KV, 5 tiled + packed rows + KV splits, 7 / 8 one-wave-per-SIMD, 9 head_dim 256
int fwd_route(const FwdArgs& a);
int fwd_last_route();   // ... of the most recent launch_fwd of this process; 0 before the first
int fwd_plan_dump(const FwdArgs& a, int* out, int cap);   // the plan as integers (tests): route, ws_bytes low / high, the route's sub-plan
// launch_fwd honours FwdArgs::rope_* for these arguments (otherwise it refuses them: rotate Q with launch_rope first)
bool fwd_rope_fusable(const FwdArgs& a);
// the split plan of route 7 as integers (tests): fwd_split_plan_dump in fa_fwd_w4_gfx950.hip, the plan itself in fa_fwd_split.h
int fwd_split_plan_dump(const FwdArgs& a, int* out, int cap);
// blockIdx -> (batch, kv head, q head, block) of decode_work (ranked = 0) / decode_work_ranked (1) on the host (tests): fa_fwd_f32.hip
void work_order_dump(int ranked, int bid, int B, int Hq, int Hkv, int nblk, int flag, int* out4);
// bytes of workspace launch_fwd / launch_paged_decode (Sq = 1) or launch_paged_query would allocate for these arguments (0: single-launch path)
uint64_t fwd_workspace_bytes(const FwdArgs& a);
uint64_t paged_workspace_bytes(const PagedArgs& a);
int launch_bwd(const BwdArgs& a, hipStream_t stream);
int bwd_last_route();   // BwdPlan::route of the most recent launch_bwd of this process (fa_bwd_plan.h: the plan, the workspace sizes); 0 before the first

// Set the max-dynamic-LDS attribute on every kernel (call once per device).
int configure_kernels();

}  // namespace aule_hip
