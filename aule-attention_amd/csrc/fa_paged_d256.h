// fa_paged_d256.h -- the host interface of the paged attention at head_dim 256 (fa_fwd_paged_d256_gfx950.hip): the
// arguments, the launch plan and the launch.  The contract is aule_paged_d256_desc in include/aule.h.
#pragma once
#include "fa_kernels.h"

namespace aule_hip {

// Ragged queries q [T, Hq, 256] 16-bit against a paged cache k_cache / v_cache [num_blocks, block_size, Hkv, 256] of q's dtype
// (kCache16) or of e4m3fn codes with per-KV-head scales (kCacheFp8E4M3); out [T, Hq, 256] contiguous, lse [T, Hq] fp32 or null.
// Table, lengths, cu_seqlens_q, the clamps, the window and the rows that are written as PagedPrefillArgs; cu_seqlens_q = null:
// sequence b owns row b, one token each (T >= B).  The caller guarantees 16-byte aligned q / out / caches and q_token_stride % 8 == 0.
struct PagedD256Args {
    const void* q;
    const void* k_cache;
    const void* v_cache;
    void* out;
    float* lse = nullptr;
    const int* block_tables;
    const int* context_lens;
    const int* cu_seqlens_q = nullptr;
    int T, B, Hq, Hkv;
    int max_seqlen_q;                   // (1 with a null cu_seqlens_q)
    long long q_token_stride;
    int block_size, max_blocks;
    float scale;
    int window;                         // > 0: on
    int dtype;
    int device = -1;                    // as FwdArgs::device
    int cache_kind = kCache16;
    const float* k_scale = nullptr;     // kCacheFp8E4M3 only: [Hkv] fp32, device
    const float* v_scale = nullptr;
};

constexpr int kPagedD256Rows = 64;       // packed rows (token-major within the KV head) per workgroup
constexpr int kPagedD256MaxSplit = 64;   // key ranges per (sequence, KV head, row block), at most: a lane per split in the combine
constexpr int kPagedD256PartFloats = 256 + 2;   // fp32 per (split, token, head) of the workspace: un-normalised O, then {m, l}

// The launch plan: the one statement of row blocks, nsplit, grid and workspace (launch, size query, debug hooks), from the shape
// alone.  WHICH tiles a split owns is decided on the device from each sequence's clamped length, the block's positions and the window.
struct PagedD256Plan {
    int row_blocks = 0;        // ceil(min(max_seqlen_q, T) * (Hq / Hkv) / 64)
    int rows_per_block = 0;    // 64
    int nsplit = 0;            // 1 .. kPagedD256MaxSplit
    long long grid = 0;        // row_blocks * nsplit * Hkv * B
    uint64_t ws_bytes = 0;     // nsplit > 1: round16(nsplit * T * Hq * 258 * 4), else 0
};
// all zero: nothing to launch; no pointer is read.  force_nsplit > 0 (the debug launch alone): that many ranges, at most 64.
PagedD256Plan paged_d256_plan(const PagedD256Args& a, int force_nsplit = 0);
// (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1)  -1: unsupported arguments
int launch_paged_d256(const PagedD256Args& a, const PagedD256Plan& plan, void* ws, hipStream_t stream);
// The same with logit soft-capping, s = softcap tanh(scale q.k / softcap) (fa_fwd_paged_d256_softcap_gfx950.hip):
// `softcap` finite and > 0, the plan and the workspace those of the plain launch.
int launch_paged_d256_softcap(const PagedD256Args& a, float softcap, const PagedD256Plan& plan, void* ws, hipStream_t stream);

}  // namespace aule_hip
