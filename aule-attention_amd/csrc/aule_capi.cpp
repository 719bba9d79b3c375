// aule_capi.cpp -- extern "C" implementation of include/aule.h on the HIP runtime.
//
// Re-exports the C-ABI of the reference's src/lib.zig (global context, 1024-slot
// tensor table, 512-byte error buffer, negative return codes) over the gfx950
// kernels in this directory.  The reference's host language for this layer is
// Zig; no Zig toolchain exists in the build image, so the layer is C++ with
// identical symbol names and signatures (see INTEGRATION.md for the Zig `extern`
// block a maintainer would add to bind it).
//
// There is deliberately NO CPU fallback here: if no HIP device is present
// aule_init() fails with -1 and every compute entry point returns -1.
#include "../../include/aule.h"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <initializer_list>
#include <mutex>

#include <dlfcn.h>

#include "fa_bwd_plan.h"
#include "fa_kernels.h"
#include "fa_switches.h"

// abi2: optional workspace / workspace_bytes appended to the forward and paged descriptors (96 -> 112, 104 -> 120)
static_assert(sizeof(aule_attn_desc) == 112 && offsetof(aule_attn_desc, lse) == 88 && offsetof(aule_attn_desc, workspace) == 96,
              "aule_attn_desc layout is part of the ABI");
static_assert(sizeof(aule_paged_desc) == 120 && offsetof(aule_paged_desc, workspace) == 104,
              "aule_paged_desc layout is part of the ABI");
static_assert(sizeof(aule_paged_fp8_desc) == 136 && offsetof(aule_paged_fp8_desc, stream) == 48 &&
                  offsetof(aule_paged_fp8_desc, workspace) == 104 && offsetof(aule_paged_fp8_desc, k_scale) == 120 &&
                  offsetof(aule_paged_fp8_desc, v_scale) == 128,
              "aule_paged_fp8_desc layout is part of the ABI");
static_assert(offsetof(aule_paged_fp8_desc, q) == offsetof(aule_paged_desc, q) &&
                  offsetof(aule_paged_fp8_desc, workspace_bytes) == offsetof(aule_paged_desc, workspace_bytes) &&
                  offsetof(aule_paged_fp8_desc, k_scale) == sizeof(aule_paged_desc),
              "aule_paged_fp8_desc starts with aule_paged_desc (the paged entry points read both through that prefix)");
static_assert(sizeof(aule_paged_query_desc) == 152 && offsetof(aule_paged_query_desc, stream) == 48 &&
                  offsetof(aule_paged_query_desc, workspace) == 104 && offsetof(aule_paged_query_desc, k_scale) == 120 &&
                  offsetof(aule_paged_query_desc, v_scale) == 128 && offsetof(aule_paged_query_desc, lse) == 136 &&
                  offsetof(aule_paged_query_desc, seq_q) == 144 && offsetof(aule_paged_query_desc, cache_dtype) == 148,
              "aule_paged_query_desc layout is part of the ABI");
static_assert(sizeof(aule_paged_prefill_desc) == 152 && offsetof(aule_paged_prefill_desc, cache_dtype) == 8 &&
                  offsetof(aule_paged_prefill_desc, batch) == 12 && offsetof(aule_paged_prefill_desc, block_size) == 28 &&
                  offsetof(aule_paged_prefill_desc, max_blocks) == 32 && offsetof(aule_paged_prefill_desc, total_tokens) == 36 &&
                  offsetof(aule_paged_prefill_desc, max_seqlen_q) == 40 && offsetof(aule_paged_prefill_desc, scale) == 44 &&
                  offsetof(aule_paged_prefill_desc, window_size) == 48 && offsetof(aule_paged_prefill_desc, device) == 52 &&
                  offsetof(aule_paged_prefill_desc, q_token_stride) == 56 && offsetof(aule_paged_prefill_desc, stream) == 64 &&
                  offsetof(aule_paged_prefill_desc, q) == 72 && offsetof(aule_paged_prefill_desc, k_cache) == 80 &&
                  offsetof(aule_paged_prefill_desc, v_cache) == 88 && offsetof(aule_paged_prefill_desc, block_tables) == 96 &&
                  offsetof(aule_paged_prefill_desc, context_lens) == 104 && offsetof(aule_paged_prefill_desc, cu_seqlens_q) == 112 &&
                  offsetof(aule_paged_prefill_desc, out) == 120 && offsetof(aule_paged_prefill_desc, lse) == 128 &&
                  offsetof(aule_paged_prefill_desc, k_scale) == 136 && offsetof(aule_paged_prefill_desc, v_scale) == 144,
              "aule_paged_prefill_desc layout is part of the ABI");
static_assert(sizeof(aule_paged_cascade_desc) == 184 && offsetof(aule_paged_cascade_desc, cache_dtype) == 8 &&
                  offsetof(aule_paged_cascade_desc, batch) == 12 && offsetof(aule_paged_cascade_desc, block_size) == 28 &&
                  offsetof(aule_paged_cascade_desc, max_blocks) == 32 && offsetof(aule_paged_cascade_desc, total_tokens) == 36 &&
                  offsetof(aule_paged_cascade_desc, max_seqlen_q) == 40 && offsetof(aule_paged_cascade_desc, scale) == 44 &&
                  offsetof(aule_paged_cascade_desc, max_prefix_blocks) == 48 && offsetof(aule_paged_cascade_desc, device) == 52 &&
                  offsetof(aule_paged_cascade_desc, q_token_stride) == 56 && offsetof(aule_paged_cascade_desc, stream) == 64 &&
                  offsetof(aule_paged_cascade_desc, q) == 72 && offsetof(aule_paged_cascade_desc, k_cache) == 80 &&
                  offsetof(aule_paged_cascade_desc, v_cache) == 88 && offsetof(aule_paged_cascade_desc, block_tables) == 96 &&
                  offsetof(aule_paged_cascade_desc, context_lens) == 104 && offsetof(aule_paged_cascade_desc, cu_seqlens_q) == 112 &&
                  offsetof(aule_paged_cascade_desc, out) == 120 && offsetof(aule_paged_cascade_desc, lse) == 128 &&
                  offsetof(aule_paged_cascade_desc, k_scale) == 136 && offsetof(aule_paged_cascade_desc, v_scale) == 144 &&
                  offsetof(aule_paged_cascade_desc, prefix_block_table) == 152 && offsetof(aule_paged_cascade_desc, prefix_len) == 160 &&
                  offsetof(aule_paged_cascade_desc, workspace) == 168 && offsetof(aule_paged_cascade_desc, workspace_bytes) == 176,
              "aule_paged_cascade_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_paged_desc) == 136 && offsetof(aule_mla_paged_desc, batch) == 8 && offsetof(aule_mla_paged_desc, qk_dim) == 16 &&
                  offsetof(aule_mla_paged_desc, block_size) == 24 && offsetof(aule_mla_paged_desc, total_tokens) == 32 &&
                  offsetof(aule_mla_paged_desc, scale) == 40 && offsetof(aule_mla_paged_desc, q_token_stride) == 48 &&
                  offsetof(aule_mla_paged_desc, stream) == 56 && offsetof(aule_mla_paged_desc, q) == 64 && offsetof(aule_mla_paged_desc, kv_cache) == 72 &&
                  offsetof(aule_mla_paged_desc, block_tables) == 80 && offsetof(aule_mla_paged_desc, context_lens) == 88 &&
                  offsetof(aule_mla_paged_desc, cu_seqlens_q) == 96 && offsetof(aule_mla_paged_desc, out) == 104 && offsetof(aule_mla_paged_desc, lse) == 112 &&
                  offsetof(aule_mla_paged_desc, workspace) == 120 && offsetof(aule_mla_paged_desc, workspace_bytes) == 128,
              "aule_mla_paged_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_paged_fp8_desc) == 144 && offsetof(aule_mla_paged_fp8_desc, kv_scale) == 136 &&
                  offsetof(aule_mla_paged_fp8_desc, kv_scale) == sizeof(aule_mla_paged_desc) &&
                  offsetof(aule_mla_paged_fp8_desc, batch) == offsetof(aule_mla_paged_desc, batch) &&
                  offsetof(aule_mla_paged_fp8_desc, qk_dim) == offsetof(aule_mla_paged_desc, qk_dim) &&
                  offsetof(aule_mla_paged_fp8_desc, total_tokens) == offsetof(aule_mla_paged_desc, total_tokens) &&
                  offsetof(aule_mla_paged_fp8_desc, scale) == offsetof(aule_mla_paged_desc, scale) &&
                  offsetof(aule_mla_paged_fp8_desc, q_token_stride) == offsetof(aule_mla_paged_desc, q_token_stride) &&
                  offsetof(aule_mla_paged_fp8_desc, stream) == offsetof(aule_mla_paged_desc, stream) &&
                  offsetof(aule_mla_paged_fp8_desc, q) == offsetof(aule_mla_paged_desc, q) &&
                  offsetof(aule_mla_paged_fp8_desc, kv_cache) == offsetof(aule_mla_paged_desc, kv_cache) &&
                  offsetof(aule_mla_paged_fp8_desc, cu_seqlens_q) == offsetof(aule_mla_paged_desc, cu_seqlens_q) &&
                  offsetof(aule_mla_paged_fp8_desc, out) == offsetof(aule_mla_paged_desc, out) &&
                  offsetof(aule_mla_paged_fp8_desc, lse) == offsetof(aule_mla_paged_desc, lse) &&
                  offsetof(aule_mla_paged_fp8_desc, workspace) == offsetof(aule_mla_paged_desc, workspace) &&
                  offsetof(aule_mla_paged_fp8_desc, workspace_bytes) == offsetof(aule_mla_paged_desc, workspace_bytes),
              "aule_mla_paged_fp8_desc starts with aule_mla_paged_desc (the MLA entry points read both through that prefix)");
// The tree kind of the paged MLA: the FP8 kind field for field (so the 16-bit kind too), then tree_mask and cache_dtype.
#define AULE_MLA_TREE_SAME(f) (offsetof(aule_mla_paged_tree_desc, f) == offsetof(aule_mla_paged_fp8_desc, f))
static_assert(sizeof(aule_mla_paged_tree_desc) == 160 && offsetof(aule_mla_paged_tree_desc, tree_mask) == 144 &&
                  offsetof(aule_mla_paged_tree_desc, tree_mask) == sizeof(aule_mla_paged_fp8_desc) &&
                  offsetof(aule_mla_paged_tree_desc, cache_dtype) == 152 && offsetof(aule_mla_paged_tree_desc, reserved) == 156 &&
                  offsetof(aule_mla_paged_tree_desc, kv_scale) == 136 && AULE_MLA_TREE_SAME(dtype) && AULE_MLA_TREE_SAME(batch) &&
                  AULE_MLA_TREE_SAME(heads_q) && AULE_MLA_TREE_SAME(qk_dim) && AULE_MLA_TREE_SAME(v_dim) && AULE_MLA_TREE_SAME(block_size) &&
                  AULE_MLA_TREE_SAME(max_blocks) && AULE_MLA_TREE_SAME(total_tokens) && AULE_MLA_TREE_SAME(max_seqlen_q) && AULE_MLA_TREE_SAME(scale) &&
                  AULE_MLA_TREE_SAME(device) && AULE_MLA_TREE_SAME(q_token_stride) && AULE_MLA_TREE_SAME(stream) && AULE_MLA_TREE_SAME(q) &&
                  AULE_MLA_TREE_SAME(kv_cache) && AULE_MLA_TREE_SAME(block_tables) && AULE_MLA_TREE_SAME(context_lens) &&
                  AULE_MLA_TREE_SAME(cu_seqlens_q) && AULE_MLA_TREE_SAME(out) && AULE_MLA_TREE_SAME(lse) && AULE_MLA_TREE_SAME(workspace) &&
                  AULE_MLA_TREE_SAME(workspace_bytes) && AULE_MLA_TREE_SAME(kv_scale),
              "aule_mla_paged_tree_desc is aule_mla_paged_fp8_desc plus tree_mask and cache_dtype");
#undef AULE_MLA_TREE_SAME
static_assert(sizeof(aule_mla_sparse_desc) == 120 && offsetof(aule_mla_sparse_desc, dtype) == 4 && offsetof(aule_mla_sparse_desc, cache_dtype) == 8 &&
                  offsetof(aule_mla_sparse_desc, heads_q) == 12 && offsetof(aule_mla_sparse_desc, num_blocks) == 16 &&
                  offsetof(aule_mla_sparse_desc, block_size) == 20 && offsetof(aule_mla_sparse_desc, total_tokens) == 24 &&
                  offsetof(aule_mla_sparse_desc, topk) == 28 && offsetof(aule_mla_sparse_desc, scale) == 32 && offsetof(aule_mla_sparse_desc, device) == 36 &&
                  offsetof(aule_mla_sparse_desc, q_token_stride) == 40 && offsetof(aule_mla_sparse_desc, stream) == 48 &&
                  offsetof(aule_mla_sparse_desc, q) == 56 && offsetof(aule_mla_sparse_desc, kv_cache) == 64 && offsetof(aule_mla_sparse_desc, indices) == 72 &&
                  offsetof(aule_mla_sparse_desc, kv_scale) == 80 && offsetof(aule_mla_sparse_desc, out) == 88 && offsetof(aule_mla_sparse_desc, lse) == 96 &&
                  offsetof(aule_mla_sparse_desc, workspace) == 104 && offsetof(aule_mla_sparse_desc, workspace_bytes) == 112,
              "aule_mla_sparse_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_indexer_logits_desc) == 136 && offsetof(aule_mla_indexer_logits_desc, dtype) == 4 &&
                  offsetof(aule_mla_indexer_logits_desc, cache_dtype) == 8 && offsetof(aule_mla_indexer_logits_desc, heads) == 12 &&
                  offsetof(aule_mla_indexer_logits_desc, head_dim) == 16 && offsetof(aule_mla_indexer_logits_desc, batch) == 20 &&
                  offsetof(aule_mla_indexer_logits_desc, num_blocks) == 24 && offsetof(aule_mla_indexer_logits_desc, block_size) == 28 &&
                  offsetof(aule_mla_indexer_logits_desc, max_blocks) == 32 && offsetof(aule_mla_indexer_logits_desc, total_tokens) == 36 &&
                  offsetof(aule_mla_indexer_logits_desc, max_seqlen_q) == 40 && offsetof(aule_mla_indexer_logits_desc, device) == 44 &&
                  offsetof(aule_mla_indexer_logits_desc, q_token_stride) == 48 && offsetof(aule_mla_indexer_logits_desc, logits_stride) == 56 &&
                  offsetof(aule_mla_indexer_logits_desc, stream) == 64 && offsetof(aule_mla_indexer_logits_desc, q) == 72 &&
                  offsetof(aule_mla_indexer_logits_desc, weights) == 80 && offsetof(aule_mla_indexer_logits_desc, k_cache) == 88 &&
                  offsetof(aule_mla_indexer_logits_desc, k_scale) == 96 && offsetof(aule_mla_indexer_logits_desc, block_tables) == 104 &&
                  offsetof(aule_mla_indexer_logits_desc, context_lens) == 112 && offsetof(aule_mla_indexer_logits_desc, cu_seqlens_q) == 120 &&
                  offsetof(aule_mla_indexer_logits_desc, logits) == 128,
              "aule_mla_indexer_logits_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_indexer_topk_desc) == 96 && offsetof(aule_mla_indexer_topk_desc, output) == 4 &&
                  offsetof(aule_mla_indexer_topk_desc, topk) == 8 && offsetof(aule_mla_indexer_topk_desc, batch) == 12 &&
                  offsetof(aule_mla_indexer_topk_desc, block_size) == 16 && offsetof(aule_mla_indexer_topk_desc, max_blocks) == 20 &&
                  offsetof(aule_mla_indexer_topk_desc, total_tokens) == 24 && offsetof(aule_mla_indexer_topk_desc, max_seqlen_q) == 28 &&
                  offsetof(aule_mla_indexer_topk_desc, device) == 32 && offsetof(aule_mla_indexer_topk_desc, reserved) == 36 &&
                  offsetof(aule_mla_indexer_topk_desc, logits_stride) == 40 && offsetof(aule_mla_indexer_topk_desc, stream) == 48 &&
                  offsetof(aule_mla_indexer_topk_desc, logits) == 56 && offsetof(aule_mla_indexer_topk_desc, block_tables) == 64 &&
                  offsetof(aule_mla_indexer_topk_desc, context_lens) == 72 && offsetof(aule_mla_indexer_topk_desc, cu_seqlens_q) == 80 &&
                  offsetof(aule_mla_indexer_topk_desc, indices) == 88,
              "aule_mla_indexer_topk_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_kv_append_desc) == 128 && offsetof(aule_mla_kv_append_desc, dtype) == 4 &&
                  offsetof(aule_mla_kv_append_desc, cache_dtype) == 8 && offsetof(aule_mla_kv_append_desc, rope_layout) == 12 &&
                  offsetof(aule_mla_kv_append_desc, total_tokens) == 16 && offsetof(aule_mla_kv_append_desc, num_blocks) == 20 &&
                  offsetof(aule_mla_kv_append_desc, block_size) == 24 && offsetof(aule_mla_kv_append_desc, table_len) == 28 &&
                  offsetof(aule_mla_kv_append_desc, table_pitch) == 32 && offsetof(aule_mla_kv_append_desc, device) == 36 &&
                  offsetof(aule_mla_kv_append_desc, c_kv_token_stride) == 40 && offsetof(aule_mla_kv_append_desc, k_pe_token_stride) == 48 &&
                  offsetof(aule_mla_kv_append_desc, stream) == 56 && offsetof(aule_mla_kv_append_desc, c_kv) == 64 &&
                  offsetof(aule_mla_kv_append_desc, k_pe) == 72 && offsetof(aule_mla_kv_append_desc, kv_cache) == 80 &&
                  offsetof(aule_mla_kv_append_desc, slot_mapping) == 88 && offsetof(aule_mla_kv_append_desc, kv_scale) == 96 &&
                  offsetof(aule_mla_kv_append_desc, cos) == 104 && offsetof(aule_mla_kv_append_desc, sin) == 112 &&
                  offsetof(aule_mla_kv_append_desc, positions) == 120,
              "aule_mla_kv_append_desc layout is part of the ABI");
#define AULE_SAME_OFFSET(field) (offsetof(aule_paged_cascade_desc, field) == offsetof(aule_paged_prefill_desc, field))
static_assert(AULE_SAME_OFFSET(struct_size) && AULE_SAME_OFFSET(dtype) && AULE_SAME_OFFSET(cache_dtype) && AULE_SAME_OFFSET(batch) && AULE_SAME_OFFSET(heads_q) &&
                  AULE_SAME_OFFSET(heads_kv) && AULE_SAME_OFFSET(head_dim) && AULE_SAME_OFFSET(block_size) && AULE_SAME_OFFSET(max_blocks) &&
                  AULE_SAME_OFFSET(total_tokens) && AULE_SAME_OFFSET(max_seqlen_q) && AULE_SAME_OFFSET(scale) &&
                  offsetof(aule_paged_cascade_desc, max_prefix_blocks) == offsetof(aule_paged_prefill_desc, window_size) && AULE_SAME_OFFSET(device) &&
                  AULE_SAME_OFFSET(q_token_stride) && AULE_SAME_OFFSET(stream) && AULE_SAME_OFFSET(q) && AULE_SAME_OFFSET(k_cache) && AULE_SAME_OFFSET(v_cache) &&
                  AULE_SAME_OFFSET(block_tables) && AULE_SAME_OFFSET(context_lens) && AULE_SAME_OFFSET(cu_seqlens_q) && AULE_SAME_OFFSET(out) &&
                  AULE_SAME_OFFSET(lse) && AULE_SAME_OFFSET(k_scale) && AULE_SAME_OFFSET(v_scale) &&
                  offsetof(aule_paged_cascade_desc, prefix_block_table) == sizeof(aule_paged_prefill_desc),
              "aule_paged_cascade_desc starts with aule_paged_prefill_desc but for the word at 48, max_prefix_blocks where that has window_size "
              "(its launch arguments are filled through that prefix, the window dropped)");
#undef AULE_SAME_OFFSET
static_assert(sizeof(aule_varlen_desc) == 144 && offsetof(aule_varlen_desc, batch) == 8 && offsetof(aule_varlen_desc, heads_q) == 12 &&
                  offsetof(aule_varlen_desc, head_dim) == 20 && offsetof(aule_varlen_desc, total_q) == 24 &&
                  offsetof(aule_varlen_desc, total_k) == 28 && offsetof(aule_varlen_desc, max_seqlen_q) == 32 &&
                  offsetof(aule_varlen_desc, max_seqlen_k) == 36 && offsetof(aule_varlen_desc, scale) == 40 &&
                  offsetof(aule_varlen_desc, causal) == 44 && offsetof(aule_varlen_desc, window_size) == 48 &&
                  offsetof(aule_varlen_desc, device) == 52 && offsetof(aule_varlen_desc, q_token_stride) == 56 &&
                  offsetof(aule_varlen_desc, k_token_stride) == 64 && offsetof(aule_varlen_desc, v_token_stride) == 72 &&
                  offsetof(aule_varlen_desc, stream) == 80 && offsetof(aule_varlen_desc, q) == 88 && offsetof(aule_varlen_desc, k) == 96 &&
                  offsetof(aule_varlen_desc, v) == 104 && offsetof(aule_varlen_desc, cu_seqlens_q) == 112 &&
                  offsetof(aule_varlen_desc, cu_seqlens_k) == 120 && offsetof(aule_varlen_desc, out) == 128 &&
                  offsetof(aule_varlen_desc, lse) == 136,
              "aule_varlen_desc layout is part of the ABI");
static_assert(sizeof(aule_varlen_bwd_desc) == 192 && offsetof(aule_varlen_bwd_desc, out) == 128 && offsetof(aule_varlen_bwd_desc, lse) == 136 &&
                  offsetof(aule_varlen_bwd_desc, dout) == 144 && offsetof(aule_varlen_bwd_desc, dq) == 152 &&
                  offsetof(aule_varlen_bwd_desc, dk) == 160 && offsetof(aule_varlen_bwd_desc, dv) == 168 &&
                  offsetof(aule_varlen_bwd_desc, workspace) == 176 && offsetof(aule_varlen_bwd_desc, workspace_bytes) == 184,
              "aule_varlen_bwd_desc layout is part of the ABI");
#define AULE_VARLEN_SAME(field) (offsetof(aule_varlen_bwd_desc, field) == offsetof(aule_varlen_desc, field))
static_assert(AULE_VARLEN_SAME(dtype) && AULE_VARLEN_SAME(batch) && AULE_VARLEN_SAME(heads_q) && AULE_VARLEN_SAME(heads_kv) && AULE_VARLEN_SAME(head_dim) &&
                  AULE_VARLEN_SAME(total_q) && AULE_VARLEN_SAME(total_k) && AULE_VARLEN_SAME(max_seqlen_q) && AULE_VARLEN_SAME(max_seqlen_k) &&
                  AULE_VARLEN_SAME(scale) && AULE_VARLEN_SAME(causal) && AULE_VARLEN_SAME(window_size) && AULE_VARLEN_SAME(device) &&
                  AULE_VARLEN_SAME(q_token_stride) && AULE_VARLEN_SAME(k_token_stride) && AULE_VARLEN_SAME(v_token_stride) && AULE_VARLEN_SAME(stream) &&
                  AULE_VARLEN_SAME(q) && AULE_VARLEN_SAME(k) && AULE_VARLEN_SAME(v) && AULE_VARLEN_SAME(cu_seqlens_q) && AULE_VARLEN_SAME(cu_seqlens_k),
              "aule_varlen_bwd_desc states the problem in the fields of aule_varlen_desc, up to cu_seqlens_k: both are checked through that prefix");
#undef AULE_VARLEN_SAME
// The sink kinds: each repeats its twin field for field at the same offsets and appends its pointers, so it is checked and read through
// the twin's type (the twin's own checker, with the sink kind's size).
#define AULE_SINK_SAME(kind, twin, field) (offsetof(kind, field) == offsetof(twin, field))
#define AULE_SINK_SAME_VARLEN(kind, twin)                                                                                                                   \
    (AULE_SINK_SAME(kind, twin, dtype) && AULE_SINK_SAME(kind, twin, batch) && AULE_SINK_SAME(kind, twin, heads_q) && AULE_SINK_SAME(kind, twin, heads_kv) && \
     AULE_SINK_SAME(kind, twin, head_dim) && AULE_SINK_SAME(kind, twin, total_q) && AULE_SINK_SAME(kind, twin, total_k) &&                                   \
     AULE_SINK_SAME(kind, twin, max_seqlen_q) && AULE_SINK_SAME(kind, twin, max_seqlen_k) && AULE_SINK_SAME(kind, twin, scale) &&                            \
     AULE_SINK_SAME(kind, twin, causal) && AULE_SINK_SAME(kind, twin, window_size) && AULE_SINK_SAME(kind, twin, device) &&                                  \
     AULE_SINK_SAME(kind, twin, q_token_stride) && AULE_SINK_SAME(kind, twin, k_token_stride) && AULE_SINK_SAME(kind, twin, v_token_stride) &&               \
     AULE_SINK_SAME(kind, twin, stream) && AULE_SINK_SAME(kind, twin, q) && AULE_SINK_SAME(kind, twin, k) && AULE_SINK_SAME(kind, twin, v) &&                \
     AULE_SINK_SAME(kind, twin, cu_seqlens_q) && AULE_SINK_SAME(kind, twin, cu_seqlens_k) && AULE_SINK_SAME(kind, twin, out) && AULE_SINK_SAME(kind, twin, lse))
static_assert(sizeof(aule_varlen_sink_desc) == 152 && offsetof(aule_varlen_sink_desc, sinks) == 144 && offsetof(aule_varlen_sink_desc, sinks) == sizeof(aule_varlen_desc) &&
                  AULE_SINK_SAME_VARLEN(aule_varlen_sink_desc, aule_varlen_desc),
              "aule_varlen_sink_desc is aule_varlen_desc plus sinks");
static_assert(sizeof(aule_varlen_sink_bwd_desc) == 208 && offsetof(aule_varlen_sink_bwd_desc, sinks) == 192 && offsetof(aule_varlen_sink_bwd_desc, dsinks) == 200 &&
                  offsetof(aule_varlen_sink_bwd_desc, sinks) == sizeof(aule_varlen_bwd_desc) && AULE_SINK_SAME_VARLEN(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc) &&
                  AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, dout) && AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, dq) &&
                  AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, dk) && AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, dv) &&
                  AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, workspace) && AULE_SINK_SAME(aule_varlen_sink_bwd_desc, aule_varlen_bwd_desc, workspace_bytes),
              "aule_varlen_sink_bwd_desc is aule_varlen_bwd_desc plus sinks and dsinks");
#undef AULE_SINK_SAME_VARLEN
#define AULE_PREFILL_SINK_SAME(field) AULE_SINK_SAME(aule_paged_prefill_sink_desc, aule_paged_prefill_desc, field)
static_assert(sizeof(aule_paged_prefill_sink_desc) == 160 && offsetof(aule_paged_prefill_sink_desc, sinks) == 152 &&
                  offsetof(aule_paged_prefill_sink_desc, sinks) == sizeof(aule_paged_prefill_desc) && AULE_PREFILL_SINK_SAME(dtype) && AULE_PREFILL_SINK_SAME(cache_dtype) &&
                  AULE_PREFILL_SINK_SAME(batch) && AULE_PREFILL_SINK_SAME(heads_q) && AULE_PREFILL_SINK_SAME(heads_kv) && AULE_PREFILL_SINK_SAME(head_dim) &&
                  AULE_PREFILL_SINK_SAME(block_size) && AULE_PREFILL_SINK_SAME(max_blocks) && AULE_PREFILL_SINK_SAME(total_tokens) && AULE_PREFILL_SINK_SAME(max_seqlen_q) &&
                  AULE_PREFILL_SINK_SAME(scale) && AULE_PREFILL_SINK_SAME(window_size) && AULE_PREFILL_SINK_SAME(device) && AULE_PREFILL_SINK_SAME(q_token_stride) &&
                  AULE_PREFILL_SINK_SAME(stream) && AULE_PREFILL_SINK_SAME(q) && AULE_PREFILL_SINK_SAME(k_cache) && AULE_PREFILL_SINK_SAME(v_cache) &&
                  AULE_PREFILL_SINK_SAME(block_tables) && AULE_PREFILL_SINK_SAME(context_lens) && AULE_PREFILL_SINK_SAME(cu_seqlens_q) && AULE_PREFILL_SINK_SAME(out) &&
                  AULE_PREFILL_SINK_SAME(lse) && AULE_PREFILL_SINK_SAME(k_scale) && AULE_PREFILL_SINK_SAME(v_scale),
              "aule_paged_prefill_sink_desc is aule_paged_prefill_desc plus sinks");
#undef AULE_PREFILL_SINK_SAME
#define AULE_QUERY_SINK_SAME(field) AULE_SINK_SAME(aule_paged_query_sink_desc, aule_paged_query_desc, field)
static_assert(sizeof(aule_paged_query_sink_desc) == 160 && offsetof(aule_paged_query_sink_desc, sinks) == 152 &&
                  offsetof(aule_paged_query_sink_desc, sinks) == sizeof(aule_paged_query_desc) && AULE_QUERY_SINK_SAME(dtype) && AULE_QUERY_SINK_SAME(batch) &&
                  AULE_QUERY_SINK_SAME(heads_q) && AULE_QUERY_SINK_SAME(heads_kv) && AULE_QUERY_SINK_SAME(head_dim) && AULE_QUERY_SINK_SAME(block_size) &&
                  AULE_QUERY_SINK_SAME(max_blocks) && AULE_QUERY_SINK_SAME(scale) && AULE_QUERY_SINK_SAME(window_size) && AULE_QUERY_SINK_SAME(device) &&
                  AULE_QUERY_SINK_SAME(stream) && AULE_QUERY_SINK_SAME(q) && AULE_QUERY_SINK_SAME(k_cache) && AULE_QUERY_SINK_SAME(v_cache) &&
                  AULE_QUERY_SINK_SAME(block_tables) && AULE_QUERY_SINK_SAME(context_lens) && AULE_QUERY_SINK_SAME(out) && AULE_QUERY_SINK_SAME(workspace) &&
                  AULE_QUERY_SINK_SAME(workspace_bytes) && AULE_QUERY_SINK_SAME(k_scale) && AULE_QUERY_SINK_SAME(v_scale) && AULE_QUERY_SINK_SAME(lse) &&
                  AULE_QUERY_SINK_SAME(seq_q) && AULE_QUERY_SINK_SAME(cache_dtype),
              "aule_paged_query_sink_desc is aule_paged_query_desc plus sinks");
#undef AULE_QUERY_SINK_SAME
// The tree kinds (tree masks: include/aule.h), pinned the same way: the twin field for field, then tree_mask.
#define AULE_PREFILL_TREE_SAME(field) AULE_SINK_SAME(aule_paged_prefill_tree_desc, aule_paged_prefill_desc, field)
static_assert(sizeof(aule_paged_prefill_tree_desc) == 160 && offsetof(aule_paged_prefill_tree_desc, tree_mask) == 152 &&
                  offsetof(aule_paged_prefill_tree_desc, tree_mask) == sizeof(aule_paged_prefill_desc) && AULE_PREFILL_TREE_SAME(dtype) && AULE_PREFILL_TREE_SAME(cache_dtype) &&
                  AULE_PREFILL_TREE_SAME(batch) && AULE_PREFILL_TREE_SAME(heads_q) && AULE_PREFILL_TREE_SAME(heads_kv) && AULE_PREFILL_TREE_SAME(head_dim) &&
                  AULE_PREFILL_TREE_SAME(block_size) && AULE_PREFILL_TREE_SAME(max_blocks) && AULE_PREFILL_TREE_SAME(total_tokens) && AULE_PREFILL_TREE_SAME(max_seqlen_q) &&
                  AULE_PREFILL_TREE_SAME(scale) && AULE_PREFILL_TREE_SAME(window_size) && AULE_PREFILL_TREE_SAME(device) && AULE_PREFILL_TREE_SAME(q_token_stride) &&
                  AULE_PREFILL_TREE_SAME(stream) && AULE_PREFILL_TREE_SAME(q) && AULE_PREFILL_TREE_SAME(k_cache) && AULE_PREFILL_TREE_SAME(v_cache) &&
                  AULE_PREFILL_TREE_SAME(block_tables) && AULE_PREFILL_TREE_SAME(context_lens) && AULE_PREFILL_TREE_SAME(cu_seqlens_q) && AULE_PREFILL_TREE_SAME(out) &&
                  AULE_PREFILL_TREE_SAME(lse) && AULE_PREFILL_TREE_SAME(k_scale) && AULE_PREFILL_TREE_SAME(v_scale),
              "aule_paged_prefill_tree_desc is aule_paged_prefill_desc plus tree_mask");
#undef AULE_PREFILL_TREE_SAME
#define AULE_QUERY_TREE_SAME(field) AULE_SINK_SAME(aule_paged_query_tree_desc, aule_paged_query_desc, field)
static_assert(sizeof(aule_paged_query_tree_desc) == 160 && offsetof(aule_paged_query_tree_desc, tree_mask) == 152 &&
                  offsetof(aule_paged_query_tree_desc, tree_mask) == sizeof(aule_paged_query_desc) && AULE_QUERY_TREE_SAME(dtype) && AULE_QUERY_TREE_SAME(batch) &&
                  AULE_QUERY_TREE_SAME(heads_q) && AULE_QUERY_TREE_SAME(heads_kv) && AULE_QUERY_TREE_SAME(head_dim) && AULE_QUERY_TREE_SAME(block_size) &&
                  AULE_QUERY_TREE_SAME(max_blocks) && AULE_QUERY_TREE_SAME(scale) && AULE_QUERY_TREE_SAME(window_size) && AULE_QUERY_TREE_SAME(device) &&
                  AULE_QUERY_TREE_SAME(stream) && AULE_QUERY_TREE_SAME(q) && AULE_QUERY_TREE_SAME(k_cache) && AULE_QUERY_TREE_SAME(v_cache) &&
                  AULE_QUERY_TREE_SAME(block_tables) && AULE_QUERY_TREE_SAME(context_lens) && AULE_QUERY_TREE_SAME(out) && AULE_QUERY_TREE_SAME(workspace) &&
                  AULE_QUERY_TREE_SAME(workspace_bytes) && AULE_QUERY_TREE_SAME(k_scale) && AULE_QUERY_TREE_SAME(v_scale) && AULE_QUERY_TREE_SAME(lse) &&
                  AULE_QUERY_TREE_SAME(seq_q) && AULE_QUERY_TREE_SAME(cache_dtype),
              "aule_paged_query_tree_desc is aule_paged_query_desc plus tree_mask");
#undef AULE_QUERY_TREE_SAME
#undef AULE_SINK_SAME
static_assert(sizeof(aule_mla_prefill_desc) == 176 && offsetof(aule_mla_prefill_desc, dtype) == 4 && offsetof(aule_mla_prefill_desc, batch) == 8 &&
                  offsetof(aule_mla_prefill_desc, heads) == 12 && offsetof(aule_mla_prefill_desc, qk_dim) == 16 &&
                  offsetof(aule_mla_prefill_desc, v_dim) == 20 && offsetof(aule_mla_prefill_desc, total_q) == 24 &&
                  offsetof(aule_mla_prefill_desc, total_k) == 28 && offsetof(aule_mla_prefill_desc, max_seqlen_q) == 32 &&
                  offsetof(aule_mla_prefill_desc, max_seqlen_k) == 36 && offsetof(aule_mla_prefill_desc, scale) == 40 &&
                  offsetof(aule_mla_prefill_desc, causal) == 44 && offsetof(aule_mla_prefill_desc, device) == 48 &&
                  offsetof(aule_mla_prefill_desc, reserved) == 52 && offsetof(aule_mla_prefill_desc, q_token_stride) == 56 &&
                  offsetof(aule_mla_prefill_desc, k_nope_token_stride) == 64 && offsetof(aule_mla_prefill_desc, k_nope_head_stride) == 72 &&
                  offsetof(aule_mla_prefill_desc, v_token_stride) == 80 && offsetof(aule_mla_prefill_desc, v_head_stride) == 88 &&
                  offsetof(aule_mla_prefill_desc, k_pe_token_stride) == 96 && offsetof(aule_mla_prefill_desc, stream) == 104 &&
                  offsetof(aule_mla_prefill_desc, q) == 112 && offsetof(aule_mla_prefill_desc, k_nope) == 120 &&
                  offsetof(aule_mla_prefill_desc, k_pe) == 128 && offsetof(aule_mla_prefill_desc, v) == 136 &&
                  offsetof(aule_mla_prefill_desc, cu_seqlens_q) == 144 && offsetof(aule_mla_prefill_desc, cu_seqlens_k) == 152 &&
                  offsetof(aule_mla_prefill_desc, out) == 160 && offsetof(aule_mla_prefill_desc, lse) == 168,
              "aule_mla_prefill_desc layout is part of the ABI");
static_assert(sizeof(aule_mla_prefill_bwd_desc) == 264 && offsetof(aule_mla_prefill_bwd_desc, out) == 160 && offsetof(aule_mla_prefill_bwd_desc, lse) == 168 &&
                  offsetof(aule_mla_prefill_bwd_desc, dout) == 176 && offsetof(aule_mla_prefill_bwd_desc, dq) == 184 &&
                  offsetof(aule_mla_prefill_bwd_desc, dk_nope) == 192 && offsetof(aule_mla_prefill_bwd_desc, dk_pe) == 200 &&
                  offsetof(aule_mla_prefill_bwd_desc, dv) == 208 && offsetof(aule_mla_prefill_bwd_desc, dk_nope_token_stride) == 216 &&
                  offsetof(aule_mla_prefill_bwd_desc, dk_nope_head_stride) == 224 && offsetof(aule_mla_prefill_bwd_desc, dv_token_stride) == 232 &&
                  offsetof(aule_mla_prefill_bwd_desc, dv_head_stride) == 240 && offsetof(aule_mla_prefill_bwd_desc, workspace) == 248 &&
                  offsetof(aule_mla_prefill_bwd_desc, workspace_bytes) == 256,
              "aule_mla_prefill_bwd_desc layout is part of the ABI");
#define AULE_MLA_PREFILL_SAME(field) (offsetof(aule_mla_prefill_bwd_desc, field) == offsetof(aule_mla_prefill_desc, field))
static_assert(AULE_MLA_PREFILL_SAME(dtype) && AULE_MLA_PREFILL_SAME(batch) && AULE_MLA_PREFILL_SAME(heads) && AULE_MLA_PREFILL_SAME(qk_dim) &&
                  AULE_MLA_PREFILL_SAME(v_dim) && AULE_MLA_PREFILL_SAME(total_q) && AULE_MLA_PREFILL_SAME(total_k) && AULE_MLA_PREFILL_SAME(max_seqlen_q) &&
                  AULE_MLA_PREFILL_SAME(max_seqlen_k) && AULE_MLA_PREFILL_SAME(scale) && AULE_MLA_PREFILL_SAME(causal) && AULE_MLA_PREFILL_SAME(device) &&
                  AULE_MLA_PREFILL_SAME(reserved) && AULE_MLA_PREFILL_SAME(q_token_stride) && AULE_MLA_PREFILL_SAME(k_nope_token_stride) &&
                  AULE_MLA_PREFILL_SAME(k_nope_head_stride) && AULE_MLA_PREFILL_SAME(v_token_stride) && AULE_MLA_PREFILL_SAME(v_head_stride) &&
                  AULE_MLA_PREFILL_SAME(k_pe_token_stride) && AULE_MLA_PREFILL_SAME(stream) && AULE_MLA_PREFILL_SAME(q) && AULE_MLA_PREFILL_SAME(k_nope) &&
                  AULE_MLA_PREFILL_SAME(k_pe) && AULE_MLA_PREFILL_SAME(v) && AULE_MLA_PREFILL_SAME(cu_seqlens_q) && AULE_MLA_PREFILL_SAME(cu_seqlens_k),
              "aule_mla_prefill_bwd_desc states the problem in the fields of aule_mla_prefill_desc, up to cu_seqlens_k: both are checked through that prefix");
#undef AULE_MLA_PREFILL_SAME
static_assert(sizeof(aule_merge_states_desc) == 80 && offsetof(aule_merge_states_desc, rows) == 8 &&
                  offsetof(aule_merge_states_desc, heads) == 12 && offsetof(aule_merge_states_desc, head_dim) == 16 &&
                  offsetof(aule_merge_states_desc, device) == 20 && offsetof(aule_merge_states_desc, stream) == 24 &&
                  offsetof(aule_merge_states_desc, out_a) == 32 && offsetof(aule_merge_states_desc, lse_a) == 40 &&
                  offsetof(aule_merge_states_desc, out_b) == 48 && offsetof(aule_merge_states_desc, lse_b) == 56 &&
                  offsetof(aule_merge_states_desc, out) == 64 && offsetof(aule_merge_states_desc, lse) == 72,
              "aule_merge_states_desc layout is part of the ABI");
static_assert(offsetof(aule_paged_query_desc, q) == offsetof(aule_paged_fp8_desc, q) &&
                  offsetof(aule_paged_query_desc, workspace_bytes) == offsetof(aule_paged_fp8_desc, workspace_bytes) &&
                  offsetof(aule_paged_query_desc, v_scale) == offsetof(aule_paged_fp8_desc, v_scale) &&
                  offsetof(aule_paged_query_desc, lse) == sizeof(aule_paged_fp8_desc),
              "aule_paged_query_desc starts with aule_paged_fp8_desc (its launch arguments are filled through that prefix)");
static_assert(sizeof(aule_attn_bwd_desc) == 144, "aule_attn_bwd_desc layout is part of the ABI");
static_assert(offsetof(aule_attn_bwd_desc, dtype) == offsetof(aule_attn_desc, dtype) && offsetof(aule_attn_bwd_desc, head_dim) == offsetof(aule_attn_desc, head_dim) &&
                  offsetof(aule_attn_bwd_desc, scale) == offsetof(aule_attn_desc, scale) && offsetof(aule_attn_bwd_desc, device) == offsetof(aule_attn_desc, device) &&
                  offsetof(aule_attn_bwd_desc, stream) == 48 && offsetof(aule_attn_desc, stream) == 48 && offsetof(aule_attn_bwd_desc, q) == offsetof(aule_attn_desc, q),
              "aule_attn_bwd_desc starts with aule_attn_desc's problem statement (both kinds are checked and read through that prefix)");
static_assert(sizeof(aule_kv_append_desc) == 168 && offsetof(aule_kv_append_desc, key_token_stride) == 32 &&
                  offsetof(aule_kv_append_desc, table_len) == 64 && offsetof(aule_kv_append_desc, stream) == 80 &&
                  offsetof(aule_kv_append_desc, k_cache) == 104 && offsetof(aule_kv_append_desc, slot_mapping) == 120 &&
                  offsetof(aule_kv_append_desc, cos) == 144 && offsetof(aule_kv_append_desc, positions) == 160,
              "aule_kv_append_desc layout is part of the ABI");

namespace {

using aule_hip::BwdArgs;
using aule_hip::FwdArgs;

struct DevTensor {
    void* ptr = nullptr;      // device memory, rows padded to `pitch` floats
    uint32_t shape[4] = {0, 0, 0, 0};
    uint64_t count = 0;       // logical element count (B*H*S*D)
    uint32_t pitch = 0;       // padded head_dim (32 / 64 / 128 / 256, or D itself if D > 256)
    bool used = false;
};

std::mutex g_mu;
bool g_init = false;
int g_device = 0;
uint64_t g_configured_mask = 0;  // devices on which kernel attributes were set
char g_err[512];
size_t g_err_len = 0;
DevTensor g_tensors[AULE_MAX_TENSORS];
int g_variant = 0;

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    int n = vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    if (n < 0) n = 0;
    if ((size_t)n >= sizeof(g_err)) n = sizeof(g_err) - 1;
    g_err_len = (size_t)n;
}

// (the caller holds g_mu)
bool initialised() {
    if (!g_init) set_error("Library not initialized. Call aule_init() first.");
    return g_init;
}

// The mask the kernels run, from an entry point's causal code and window and the Sq / Sk already in `a` (FwdArgs or BwdArgs):
// coff from the code; a window that masks nothing is dropped -- W >= Sq + coff, the last query sits at position Sq - 1 + coff;
// and one query at the bottom-right position sees every key: with no window the causal mask masks nothing, and the problem is
// the non-causal one (which has the faster short-query paths).
template <class Args>
void set_mask(Args& a, int32_t causal_code, int32_t window, bool drop_trivial_causal = true) {
    a.causal = causal_code != 0;
    a.coff = causal_code == AULE_CAUSAL_BOTTOM_RIGHT ? a.Sk - a.Sq : 0;
    a.window = (window > 0 && (uint32_t)window < (uint32_t)a.Sq + (uint32_t)a.coff) ? window : -1;
    if (drop_trivial_causal && a.causal && a.Sq == 1 && a.coff > 0 && a.window <= 0) a.causal = a.coff = 0;
}

float resolve_scale(float scale, uint32_t D) {
    if (scale == 0.0f || std::isnan(scale)) return 1.0f / std::sqrt((float)D);
    return scale;
}

// The problem statement the forward and backward descriptors share (aule_attn_bwd_desc read through its prefix), into FwdArgs or BwdArgs.
template <class Args>
void fill_problem(const aule_attn_desc* d, Args& a, bool drop_trivial_causal) {
    a.B = (int)d->batch; a.Hq = (int)d->heads_q; a.Hkv = (int)d->heads_kv;
    a.Sq = (int)d->seq_q; a.Sk = (int)d->seq_k; a.D = (int)d->head_dim;
    a.scale = resolve_scale(d->scale, d->head_dim);
    a.dtype = d->dtype; a.device = d->device;
    set_mask(a, d->causal, d->window_size, drop_trivial_causal);
}

uint32_t pad_dim(uint32_t d) {
    if (d <= 32) return 32;
    if (d <= 64) return 64;
    if (d <= 128) return 128;
    if (d <= 256) return 256;
    return d;
}

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            switched = hipSetDevice(dev) == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

int ensure_configured() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    if (dev < 64 && (g_configured_mask >> dev) & 1) return 0;
    int rc = aule_hip::configure_kernels();
    if (rc != 0) {
        set_error("Kernel configuration failed on device %d: %s", dev, hipGetErrorString((hipError_t)rc));
        return -4;
    }
    if (dev < 64) g_configured_mask |= (1ull << dev);
    return 0;
}

DevTensor* lookup(uint64_t h) {
    if (h == 0 || h > AULE_MAX_TENSORS) return nullptr;
    DevTensor* t = &g_tensors[h - 1];
    return t->used ? t : nullptr;
}

void free_tensor(DevTensor* t) {
    if (t->used && t->ptr) (void)hipFree(t->ptr);
    *t = DevTensor();
}

// Padded temporary for the host-pointer entry points.
struct Temp {
    float* ptr = nullptr;
    ~Temp() {
        if (ptr) (void)hipFree(ptr);
    }
    bool alloc(size_t rows, uint32_t pitch) {
        if (hipMalloc((void**)&ptr, rows * pitch * sizeof(float)) != hipSuccess) return false;
        return hipMemset(ptr, 0, rows * pitch * sizeof(float)) == hipSuccess;
    }
};

bool upload_rows(float* dst, uint32_t pitch, const float* src, size_t rows, uint32_t d) {
    return hipMemcpy2D(dst, pitch * sizeof(float), src, d * sizeof(float), d * sizeof(float), rows,
                       hipMemcpyHostToDevice) == hipSuccess;
}

bool download_rows(float* dst, const float* src, uint32_t pitch, size_t rows, uint32_t d) {
    return hipMemcpy2D(dst, d * sizeof(float), src, pitch * sizeof(float), d * sizeof(float), rows,
                       hipMemcpyDeviceToHost) == hipSuccess;
}

int run_fwd_f32(const float* q, const float* k, const float* v, float* o, float* lse, uint32_t B, uint32_t Hq,
                uint32_t Hkv, uint32_t Sq, uint32_t Sk, uint32_t Dlogical, uint32_t Dp, int causal, int window = -1) {
    FwdArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o; a.lse = lse;
    a.B = (int)B; a.Hq = (int)Hq; a.Hkv = (int)Hkv; a.Sq = (int)Sq; a.Sk = (int)Sk; a.D = (int)Dp;
    a.scale = 1.0f / std::sqrt((float)Dlogical);  // attention_pipeline.zig:329
    set_mask(a, causal != 0 ? AULE_CAUSAL_TOP_LEFT : AULE_CAUSAL_NONE, window);   // (the legacy entries: any non-zero `causal` is top-left)
    a.dtype = aule_hip::kF32;
    int rc = aule_hip::launch_fwd(a, nullptr);
    if (rc != 0) return rc;
    return (int)hipDeviceSynchronize();
}

}  // namespace

namespace aule_hip {
#ifdef AULE_DEBUG_HOOKS
int launch_fwd_pp_timeline(const FwdArgs& a, unsigned long long* dbg, hipStream_t stream);
int launch_fwd_w4_timeline(const FwdArgs& a, unsigned long long* dbg, hipStream_t stream);
#endif
int configure_fwd();
int configure_bwd();
int configure_kernels() {
    int rc = configure_fwd();
    if (rc) return rc;
    return configure_bwd();
}
}  // namespace aule_hip

extern "C" {

int32_t aule_init(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_init) return 0;  // idempotent (src/lib.zig:60-63)
    // AULE_BACKEND (src/backends/backend.zig:86-100): "hip" forces the backend this library IS -- a no-op; any value the
    // reference does not know falls through to its auto-detection, i.e. to HIP here; "vulkan" and "cpu" name backends
    // this build does not contain (no multi-backend dispatch, no CPU fallback): fail loudly instead of running something else.
    if (const char* b = getenv("AULE_BACKEND")) {
        if (strcmp(b, "vulkan") == 0 || strcmp(b, "cpu") == 0) {
            set_error("Failed to initialize backend: AULE_BACKEND=%s, but this library contains the HIP (gfx950) backend only", b);
            return -1;
        }
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("Failed to initialize backend: no HIP device (%s)",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return -1;
    }
    int dev = 0;
    if (const char* s = getenv("AULE_HIP_DEVICE")) {
        dev = atoi(s);
        if (dev < 0 || dev >= n) {
            set_error("Failed to initialize backend: AULE_HIP_DEVICE=%d out of range (0..%d)", dev, n - 1);
            return -1;
        }
    } else if (hipGetDevice(&dev) != hipSuccess) {
        dev = 0;
    }
    g_device = dev;
    {
        DeviceGuard g(g_device);
        int rc = ensure_configured();
        if (rc != 0) return -1;
    }
    g_init = true;
    g_err_len = 0;
    return 0;
}

void aule_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_init) {
        DeviceGuard g(g_device);
        for (auto& t : g_tensors) free_tensor(&t);
    }
    g_init = false;
}

const char* aule_get_error(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_err_len == 0) return "No error";
    g_err[g_err_len] = 0;
    return g_err;
}

const char* aule_get_backend_name(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? "HIP/ROCm" : "Not initialized";  // backend.zig:496-502
}

int32_t aule_get_vendor(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? 1 : -1;
}
int32_t aule_get_gpu_vendor(void) { return aule_get_vendor(); }

int32_t aule_is_amd_optimized(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? 1 : -1;
}

int32_t aule_has_fp16(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? 1 : -1;
}

int32_t aule_get_subgroup_size(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? 64 : -1;
}

int32_t aule_get_device_name(uint8_t* buffer, uint32_t buffer_len) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    if (buffer == nullptr || buffer_len == 0) return 0;
    hipDeviceProp_t prop;
    const char* name = "HIP Device";
    if (hipGetDeviceProperties(&prop, g_device) == hipSuccess) name = prop.name;
    size_t n = strlen(name);
    if (n > buffer_len - 1) n = buffer_len - 1;
    memcpy(buffer, name, n);
    buffer[n] = 0;
    return (int32_t)n;
}

int32_t aule_set_shader_variant(uint8_t variant) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    if (variant != 0) {
        set_error("Shader variant %u not available (the HIP build has one kernel family)", (unsigned)variant);
        return -2;
    }
    g_variant = 0;
    return 0;
}

int32_t aule_get_shader_variant(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? g_variant : -1;
}

int32_t aule_has_shader_variant(uint8_t variant) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    return variant == 0 ? 1 : 0;
}

int32_t aule_supports_backward(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return g_init ? 1 : 0;
}

/* ---------------------------------------------------------------- tensors */
aule_tensor_handle aule_tensor_create(uint32_t b, uint32_t h, uint32_t s, uint32_t d) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) {
        set_error("Not initialized");
        return 0;
    }
    int slot = -1;
    for (int i = 0; i < (int)AULE_MAX_TENSORS; ++i)
        if (!g_tensors[i].used) {
            slot = i;
            break;
        }
    if (slot < 0) {
        set_error("Max tensors reached");
        return 0;
    }
    const uint64_t rows = (uint64_t)b * h * s;
    const uint32_t pitch = pad_dim(d);
    DevTensor t;
    t.shape[0] = b; t.shape[1] = h; t.shape[2] = s; t.shape[3] = d;
    t.count = rows * d;
    t.pitch = pitch;
    const size_t bytes = (size_t)rows * pitch * sizeof(float);
    DeviceGuard g(g_device);
    if (bytes > 0) {
        hipError_t e = hipMalloc(&t.ptr, bytes);
        if (e != hipSuccess) {
            set_error("Create tensor failed: %s", hipGetErrorString(e));
            return 0;
        }
        (void)hipMemset(t.ptr, 0, bytes);
    }
    t.used = true;
    g_tensors[slot] = t;
    return (aule_tensor_handle)(slot + 1);
}

aule_tensor_handle aule_tensor_create_u32(uint32_t b, uint32_t h, uint32_t s, uint32_t d) {
    return aule_tensor_create(b, h, s, d);  // src/lib.zig:432-442: u32 aliases fp32 storage
}

void aule_tensor_destroy(aule_tensor_handle handle) {
    std::lock_guard<std::mutex> lk(g_mu);
    DevTensor* t = lookup(handle);
    if (!t) return;
    DeviceGuard g(g_device);
    free_tensor(t);
}

int32_t aule_tensor_upload(aule_tensor_handle handle, const float* data, uint32_t count) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    DevTensor* t = lookup(handle);
    if (!t) return -1;
    if ((uint64_t)count != t->count) {  // backend.zig:277
        set_error("Upload failed: size mismatch (tensor has %llu elements, got %u)",
                  (unsigned long long)t->count, count);
        return -3;
    }
    if (count == 0) return 0;
    DeviceGuard g(g_device);
    const size_t rows = (size_t)t->shape[0] * t->shape[1] * t->shape[2];
    if (!upload_rows((float*)t->ptr, t->pitch, data, rows, t->shape[3])) {
        set_error("Upload failed: %s", hipGetErrorString(hipGetLastError()));
        return -3;
    }
    return 0;
}

int32_t aule_tensor_download(aule_tensor_handle handle, float* output, uint32_t count) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    DevTensor* t = lookup(handle);
    if (!t) return -1;
    if ((uint64_t)count != t->count) {  // backend.zig:298
        set_error("Download failed: size mismatch (tensor has %llu elements, got %u)",
                  (unsigned long long)t->count, count);
        return -3;
    }
    if (count == 0) return 0;
    DeviceGuard g(g_device);
    const size_t rows = (size_t)t->shape[0] * t->shape[1] * t->shape[2];
    if (!download_rows(output, (const float*)t->ptr, t->pitch, rows, t->shape[3])) {
        set_error("Download failed: %s", hipGetErrorString(hipGetLastError()));
        return -3;
    }
    return 0;
}

int32_t aule_tensor_download_u32(aule_tensor_handle handle, uint32_t* output, uint32_t count) {
    return aule_tensor_download(handle, reinterpret_cast<float*>(output), count);
}

uint32_t aule_tensor_size(aule_tensor_handle handle) {
    std::lock_guard<std::mutex> lk(g_mu);
    DevTensor* t = lookup(handle);
    return t ? (uint32_t)t->count : 0;
}

uint32_t aule_tensor_count(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    uint32_t n = 0;
    for (auto& t : g_tensors) n += t.used ? 1 : 0;
    return n;
}

uint32_t aule_tensor_max(void) { return AULE_MAX_TENSORS; }

void aule_tensor_clear_all(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return;
    DeviceGuard g(g_device);
    for (auto& t : g_tensors) free_tensor(&t);
}

/* ------------------------------------------------------- handle-based fwd */
int32_t aule_attention_forward_gpu(aule_tensor_handle qh, aule_tensor_handle kh, aule_tensor_handle vh,
                                   aule_tensor_handle oh, aule_tensor_handle rot_cos,
                                   aule_tensor_handle rot_sin, int32_t causal, int32_t window_size) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    DevTensor* q = lookup(qh);
    DevTensor* k = lookup(kh);
    DevTensor* v = lookup(vh);
    DevTensor* o = lookup(oh);
    if (!q || !k || !v || !o) return -1;
    // rot_cos / rot_sin: both or neither; [.., S, D/2] tables, interleaved pairs (shaders/attention_f32.comp:98-111)
    DevTensor* rc_t = nullptr;
    DevTensor* rs_t = nullptr;
    if (rot_cos != 0 || rot_sin != 0) {
        rc_t = lookup(rot_cos);
        rs_t = lookup(rot_sin);
        if (!rc_t || !rs_t) return -1;
    }
    // window_size > 0: sliding window, key j visible to query i only if i - j < window_size (the convention of
    // the kernel the reference runs on ROCm, triton_flash_amd.py:179-183; the Vulkan shaders use others)
    // shape rules of attention_gpu.zig:383-404
    const uint32_t B = q->shape[0], Hq = q->shape[1], Sq = q->shape[2], D = q->shape[3];
    const uint32_t Hkv = k->shape[1], Sk = k->shape[2];
    bool ok = k->shape[0] == B && Hkv != 0 && Hq % Hkv == 0 && k->shape[3] == D;
    ok = ok && v->shape[0] == B && v->shape[1] == Hkv && v->shape[2] == Sk && v->shape[3] == D;
    ok = ok && o->shape[0] == B && o->shape[1] == Hq && o->shape[2] == Sq && o->shape[3] == D;
    if (!ok) {
        set_error("Attention failed: error.ShapeMismatch");
        return -3;
    }
    if (D > 256) {
        set_error("Attention failed: error.HeadDimTooLarge (head_dim %u > 256)", D);
        return -3;
    }
    if (q->count == 0) return 0;
    if (Sk == 0) {
        set_error("Attention failed: error.ShapeMismatch (empty key sequence)");
        return -3;
    }
    DeviceGuard g(g_device);
    const float* qp = (const float*)q->ptr;
    const float* kp = (const float*)k->ptr;
    float* rot = nullptr;   // rotated copies of Q and K (the handle tensors are the caller's and stay untouched)
    if (rc_t) {
        // one table shared by every batch and head, indexed by position: a flat [positions, D/2] buffer however its three
        // leading dimensions spell it -- [1, 1, S, D/2], [1, S, 1, D/2], [S, 1, 1, D/2] ("or similar broadcastable": the
        // reference's attention_gpu.zig does not look at the shape at all) -- with at least max(Sq, Sk) positions.  A genuine
        // [B, H, S', D/2] tensor (more than one leading dimension > 1) is refused: it used to pass a flattened-row count check
        // and was then read across head boundaries.
        const uint32_t need = Sq > Sk ? Sq : Sk;
        auto positions = [](const DevTensor* t, uint32_t& n) {
            int big = 0;
            n = 1;
            for (int i = 0; i < 3; ++i)
                if (t->shape[i] != 1) { ++big; n = t->shape[i]; }
            return big <= 1;
        };
        uint32_t nc = 0, ns = 0;
        if ((D & 1) || rc_t->shape[3] != D / 2 || rs_t->shape[3] != D / 2 || !positions(rc_t, nc) || !positions(rs_t, ns) ||
            nc < need || ns < need || rc_t->pitch != rs_t->pitch) {
            set_error("Attention failed: error.ShapeMismatch (rot_cos / rot_sin must be one [>= seq, head_dim/2] table: "
                      "at most one of the three leading dimensions larger than 1)");
            return -3;
        }
        const size_t nq = (size_t)B * Hq * Sq * q->pitch, nk = (size_t)B * Hkv * Sk * k->pitch;
        if (hipMalloc((void**)&rot, (nq + nk) * sizeof(float)) != hipSuccess) {
            set_error("Attention failed: error.OutOfDeviceMemory");
            return -3;
        }
        // The pass writes columns [0, D) only; the fp32 kernels run at the padded width and need pad = 0
        // (handle tensors are zero-padded on upload), so the copies must not carry allocator garbage there.
        if (q->pitch != D && hipMemset(rot, 0, (nq + nk) * sizeof(float)) != hipSuccess) {
            (void)hipFree(rot);
            set_error("Attention failed: RoPE pass: could not clear the workspace");
            return -3;
        }
        aule_hip::RopeArgs r;
        r.cos = (const float*)rc_t->ptr; r.sin = (const float*)rs_t->ptr; r.table_pitch = (int)rc_t->pitch;
        r.D = (int)D; r.layout = AULE_ROPE_INTERLEAVED; r.inverse = 0; r.pos_offset = 0; r.dtype = aule_hip::kF32;
        r.in = q->ptr; r.out = rot; r.nheads = (long long)B * Hq; r.S = (int)Sq; r.pitch = (int)q->pitch;
        int e = aule_hip::launch_rope(r, nullptr);
        r.in = k->ptr; r.out = rot + nq; r.nheads = (long long)B * Hkv; r.S = (int)Sk; r.pitch = (int)k->pitch;
        if (e == 0) e = aule_hip::launch_rope(r, nullptr);
        if (e != 0) {
            (void)hipFree(rot);
            set_error("Attention failed: RoPE pass: %s", e > 0 ? hipGetErrorString((hipError_t)e) : "unsupported shape");
            return -3;
        }
        qp = rot; kp = rot + nq;
    }
    int rc = run_fwd_f32(qp, kp, (const float*)v->ptr, (float*)o->ptr, nullptr,
                         B, Hq, Hkv, Sq, Sk, D, q->pitch, causal, window_size);
    if (rot) (void)hipFree(rot);   // run_fwd_f32 synchronises
    if (rc != 0) {
        set_error("Attention failed: %s", rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported shape");
        return -3;
    }
    return 0;
}

/* ------------------------------------------------------ host-pointer paths */
static int32_t forward_host(const float* query, const float* key, const float* value, float* output, float* lse,
                            uint32_t B, uint32_t H, uint32_t S, uint32_t D, int32_t causal) {
    if (!initialised()) return -1;
    if (D > 256) {
        set_error("Attention failed: error.HeadDimTooLarge (head_dim %u > 256)", D);
        return -4;
    }
    const size_t rows = (size_t)B * H * S;
    if (rows == 0 || D == 0) return 0;
    const uint32_t Dp = pad_dim(D);
    DeviceGuard g(g_device);
    Temp q, k, v, o, l;
    if (!q.alloc(rows, Dp) || !k.alloc(rows, Dp) || !v.alloc(rows, Dp) || !o.alloc(rows, Dp) ||
        (lse && !l.alloc(rows, 1))) {
        set_error("Create tensor failed: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (!upload_rows(q.ptr, Dp, query, rows, D) || !upload_rows(k.ptr, Dp, key, rows, D) ||
        !upload_rows(v.ptr, Dp, value, rows, D)) {
        set_error("Upload failed: %s", hipGetErrorString(hipGetLastError()));
        return -3;
    }
    int rc = run_fwd_f32(q.ptr, k.ptr, v.ptr, o.ptr, lse ? l.ptr : nullptr, B, H, H, S, S, D, Dp, causal);
    if (rc != 0) {
        set_error("Attention failed: %s", rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported shape");
        return -4;
    }
    if (!download_rows(output, o.ptr, Dp, rows, D) ||
        (lse && hipMemcpy(lse, l.ptr, rows * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) {
        set_error("Download failed: %s", hipGetErrorString(hipGetLastError()));
        return -5;
    }
    return 0;
}

int32_t aule_attention_forward(const float* query, const float* key, const float* value, float* output,
                               uint32_t B, uint32_t H, uint32_t S, uint32_t D, int32_t causal) {
    std::lock_guard<std::mutex> lk(g_mu);
    return forward_host(query, key, value, output, nullptr, B, H, S, D, causal);
}

int32_t aule_attention_forward_with_lse(const float* query, const float* key, const float* value, float* output,
                                        float* lse, uint32_t B, uint32_t H, uint32_t S, uint32_t D,
                                        int32_t causal) {
    std::lock_guard<std::mutex> lk(g_mu);
    return forward_host(query, key, value, output, lse, B, H, S, D, causal);
}

int32_t aule_attention_backward(const float* query, const float* key, const float* value, const float* output,
                                const float* grad_output, const float* lse, float* grad_query, float* grad_key,
                                float* grad_value, uint32_t B, uint32_t H, uint32_t S, uint32_t D,
                                int32_t causal) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    if (D > 256) {
        set_error("Backward failed: error.HeadDimTooLarge (head_dim %u > 256)", D);
        return -4;
    }
    const size_t rows = (size_t)B * H * S;
    if (rows == 0 || D == 0) return 0;
    const uint32_t Dp = pad_dim(D);
    DeviceGuard g(g_device);
    BwdArgs a{};
    a.B = (int)B; a.Hq = (int)H; a.Hkv = (int)H; a.Sq = (int)S; a.Sk = (int)S; a.D = (int)Dp;
    a.scale = 1.0f / std::sqrt((float)D);
    a.causal = causal != 0;
    a.dtype = aule_hip::kF32;
    a.window = -1; a.device = -1;
    Temp q, k, v, o, go, l, dq, dk, dv, ws;
    const uint64_t wsb = aule_hip::bwd_plan(a).want_bytes;
    if (!q.alloc(rows, Dp) || !k.alloc(rows, Dp) || !v.alloc(rows, Dp) || !o.alloc(rows, Dp) ||
        !go.alloc(rows, Dp) || !l.alloc(rows, 1) || !dq.alloc(rows, Dp) || !dk.alloc(rows, Dp) ||
        !dv.alloc(rows, Dp) || !ws.alloc((wsb + 3) / 4, 1)) {
        set_error("Create tensor failed: %s", hipGetErrorString(hipGetLastError()));
        return -2;
    }
    if (!upload_rows(q.ptr, Dp, query, rows, D) || !upload_rows(k.ptr, Dp, key, rows, D) ||
        !upload_rows(v.ptr, Dp, value, rows, D) || !upload_rows(o.ptr, Dp, output, rows, D) ||
        !upload_rows(go.ptr, Dp, grad_output, rows, D) ||
        hipMemcpy(l.ptr, lse, rows * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("Upload failed: %s", hipGetErrorString(hipGetLastError()));
        return -3;
    }
    a.q = q.ptr; a.k = k.ptr; a.v = v.ptr; a.o = o.ptr; a.dout = go.ptr; a.lse = l.ptr;
    a.dq = dq.ptr; a.dk = dk.ptr; a.dv = dv.ptr; a.delta = ws.ptr;
    int rc = aule_hip::launch_bwd(a, nullptr);
    if (rc == 0) rc = (int)hipDeviceSynchronize();
    if (rc != 0) {
        set_error("Backward failed: %s", rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported shape");
        return -4;
    }
    if (!download_rows(grad_query, dq.ptr, Dp, rows, D) || !download_rows(grad_key, dk.ptr, Dp, rows, D) ||
        !download_rows(grad_value, dv.ptr, Dp, rows, D)) {
        set_error("Download failed: %s", hipGetErrorString(hipGetLastError()));
        return -5;
    }
    return 0;
}

/* ------------------------------------------------------ out-of-scope stubs */
int32_t aule_attention_forward_paged(aule_tensor_handle, aule_tensor_handle, aule_tensor_handle,
                                     aule_tensor_handle, aule_tensor_handle, aule_tensor_handle, int32_t,
                                     int32_t) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    set_error("PagedAttention failed: not supported by the HIP backend");
    return -3;
}

int32_t aule_spatial_sort(aule_tensor_handle, aule_tensor_handle, aule_tensor_handle, uint32_t) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    set_error("Spatial sort failed: not supported by the HIP backend");
    return -3;
}

int32_t aule_attention_forward_gravity(aule_tensor_handle, aule_tensor_handle, aule_tensor_handle,
                                       aule_tensor_handle, aule_tensor_handle, aule_tensor_handle,
                                       aule_tensor_handle, int32_t, uint32_t, int32_t) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init) return -1;
    set_error("Gravity Attention failed: not supported by the HIP backend");
    return -3;
}

/* ------------------------------------------------------------ _ex entries */
// The descriptor checkers, one per kind: pure host logic (no lock, no g_init, no pointer dereferenced).  Each answers nullptr
// or the reason the descriptor is refused (kv_append_error further down is the model); a reason that carries values is
// formatted into the caller's Reason.  What has nothing to do is a predicate of its own per kind; null pointers, workspace
// sizes and the size limits of the launches are rules of the launch entries (the paged checkers and kv_append_error state the
// pointer rules too, for their launch entries only).  A rule that several kinds have is a function of its own, asked by each.
struct Reason { char text[128]; };
static const char kBadDescriptor[] = "bad descriptor (struct_size mismatch)";

static const char* reasonf(Reason& r, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(r.text, sizeof(r.text), fmt, ap);
    va_end(ap);
    return r.text;
}

// The end of every launch entry: 0, or -4 and "<what> failed: " the HIP error, or that no kernel takes the arguments (rc < 0).
static int32_t launched(const char* what, int rc) {
    if (rc == 0) return 0;
    set_error("%s failed: %s", what, rc > 0 ? hipGetErrorString((hipError_t)rc) : "unsupported configuration");
    return -4;
}

// aule_attn_desc and aule_attn_bwd_desc state the problem in the same leading fields (the layout asserts at the top of this file):
// both are checked and read through the forward descriptor's; `size` is the kind's own sizeof.
static const aule_attn_desc* attn_prefix(const aule_attn_bwd_desc* d) { return reinterpret_cast<const aule_attn_desc*>(d); }

// (the dense and the paged kinds alike)
static const char* head_ratio_error(uint32_t heads_q, uint32_t heads_kv, Reason& why) {
    if (heads_kv == 0 || heads_q % heads_kv != 0) return reasonf(why, "heads_q (%u) must be divisible by heads_kv (%u)", heads_q, heads_kv);
    return nullptr;
}

// plan_hook: the three forward plan hooks still answer for a bottom-right mask with seq_k < seq_q (tests/test_capi_sanitizers.py
// pins what they say there); every other reader refuses it like the launch.
static const char* attn_desc_error(const aule_attn_desc* d, size_t size, Reason& why, bool plan_hook = false) {
    if (d == nullptr || d->struct_size != size) return kBadDescriptor;
    if (d->causal < 0 || d->causal > AULE_CAUSAL_BOTTOM_RIGHT)
        return reasonf(why, "unknown causal mode %d (0 none, 1 top-left, 2 bottom-right)", d->causal);
    if (d->causal == AULE_CAUSAL_BOTTOM_RIGHT && d->seq_k < d->seq_q && !plan_hook)
        return reasonf(why, "bottom-right causal alignment needs seq_k (%u) >= seq_q (%u)", d->seq_k, d->seq_q);
    if (d->dtype < 0 || d->dtype > 2) return reasonf(why, "unknown dtype %d", d->dtype);
    if (d->head_dim != 32 && d->head_dim != 64 && d->head_dim != 128 && d->head_dim != 256)
        return reasonf(why, "head_dim %u unsupported (32, 64, 128 or 256; pad to the next size)", d->head_dim);
    return head_ratio_error(d->heads_q, d->heads_kv, why);   // (window_size: any value is accepted, <= 0 means full attention)
}

static bool fwd_nothing_to_do(const aule_attn_desc* d) { return (uint64_t)d->batch * d->heads_q * d->seq_q == 0; }  // no output element
static bool bwd_nothing_to_do(const aule_attn_desc* d) { return fwd_nothing_to_do(d) && (uint64_t)d->batch * d->heads_kv * d->seq_k == 0; }  // ... and no key element

// The launches' size limit: per-head K/V/Q slabs are addressed through 32-bit buffer descriptors (raw SRD, byte offsets).
static bool attn_too_large(const aule_attn_desc* d) {
    return (uint64_t)d->batch * d->heads_q * d->seq_q * d->head_dim >= (1ull << 40) || (uint64_t)d->seq_q * d->head_dim * 4 >= (1ull << 31) ||
           (uint64_t)d->seq_k * d->head_dim * 4 >= (1ull << 31);
}

// aule_attention_forward_rope_fusable's own limit (it answers without the launch's): extents the plan's int arithmetic holds.
static bool rope_fusable_too_large(const aule_attn_desc* d) {
    return d->batch >= (1u << 24) || d->heads_q >= (1u << 24) || d->seq_q >= (1u << 30) || d->seq_k >= (1u << 30);
}

// roctx ranges around the launches (the reference has no tracing at all), so that
// `rocprofv3 --marker-trace` shows "aule.forward" / "aule.backward" / "aule.paged_decode" / "aule.rope" next to the kernels.
// Opt-in (AULE_ROCTX=1) and loaded lazily with dlopen: the library keeps its single link dependency (libamdhip64).
struct RoctxRange {
    using PushFn = int (*)(const char*);
    using PopFn = int (*)();
    static PushFn push_fn() {
        static const PushFn fn = [] {
            if (!aule_hip::switches().roctx) return (PushFn) nullptr;
            // rocprofv3 intercepts the rocprofiler-sdk flavour; libroctx64 is the legacy (roctracer) one
            void* h = nullptr;
            for (const char* name : {"librocprofiler-sdk-roctx.so", "/opt/rocm/lib/librocprofiler-sdk-roctx.so", "libroctx64.so",
                                     "/opt/rocm/lib/libroctx64.so"}) {
                h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
                if (h != nullptr) break;
            }
            if (h == nullptr) return (PushFn) nullptr;
            // both or neither: a push whose pop did not resolve would leave a range open on every API call
            const PopFn pop = reinterpret_cast<PopFn>(dlsym(h, "roctxRangePop"));
            const PushFn push = reinterpret_cast<PushFn>(dlsym(h, "roctxRangePushA"));
            if (pop == nullptr || push == nullptr) return (PushFn) nullptr;
            pop_slot() = pop;
            return push;
        }();
        return fn;
    }
    static PopFn& pop_slot() {
        static PopFn fn = nullptr;
        return fn;
    }
    bool on = false;
    explicit RoctxRange(const char* name) {
        if (PushFn f = push_fn()) {
            f(name);
            on = pop_slot() != nullptr;
        }
    }
    ~RoctxRange() {
        if (on) pop_slot()();
    }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};

// Descriptor -> launch arguments, once per direction (every entry point that reads a descriptor; no device work, no pointer dereferenced).
static void fill_fwd_args(const aule_attn_desc* d, FwdArgs& a) {
    a.q = d->q; a.k = d->k; a.v = d->v; a.o = d->out; a.lse = d->lse;
    fill_problem(d, a, true);
    a.ws = d->workspace; a.ws_bytes = d->workspace ? d->workspace_bytes : 0;
}

// as_launched = false: the problem as the descriptor states it (what aule_attention_backward_workspace_size sizes the workspace for); true: the
// problem the launch runs inside that workspace -- a causal mask that masks nothing dropped: never more partials, the same dS per element -- with
// the stated minimum in ws_floor: the call is checked against it and the dS room lies behind it (just the minimum never looks like dS room).
static void fill_bwd_args(const aule_attn_bwd_desc* d, BwdArgs& a, bool as_launched) {
    a.q = d->q; a.k = d->k; a.v = d->v; a.o = d->out; a.dout = d->dout; a.lse = d->lse;
    a.dq = d->dq; a.dk = d->dk; a.dv = d->dv; a.delta = (float*)d->workspace;
    a.ws_bytes = d->workspace_bytes;
    fill_problem(attn_prefix(d), a, false);
    if (!as_launched) return;
    a.ws_floor = aule_hip::bwd_plan(a).min_bytes;
    set_mask(a, d->causal, d->window_size);
}

static bool fill_rope_args(const aule_attn_rope* r, uint32_t head_dim, FwdArgs& a) {
    if (r == nullptr || r->struct_size != sizeof(aule_attn_rope) || r->layout != AULE_ROPE_HALF) return false;
    if (r->table_len >= (1u << 30) || r->table_pitch >= (1u << 20) || r->q_pos_offset >= (1u << 30)) return false;
    a.rope_cos = r->cos; a.rope_sin = r->sin;
    a.rope_rows = (int)r->table_len;
    a.rope_pitch = (int)(r->table_pitch ? r->table_pitch : head_dim / 2);
    a.rope_pos = (int)r->q_pos_offset;
    return true;
}

static int32_t forward_impl(const aule_attn_desc* d, const aule_attn_rope* rope) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    Reason text;
    const char* why = attn_desc_error(d, sizeof(aule_attn_desc), text);
    if (why == nullptr && attn_too_large(d)) why = "problem too large";
    if (why != nullptr) {
        set_error("Attention failed: %s", why);
        return -3;
    }
    if (fwd_nothing_to_do(d)) return 0;
    if (d->seq_k == 0) {
        set_error("Attention failed: empty key sequence");
        return -3;
    }
    if (!d->q || !d->k || !d->v || !d->out) {
        set_error("Attention failed: null tensor pointer");
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    FwdArgs a;
    fill_fwd_args(d, a);
    if (rope != nullptr) {
        if (!fill_rope_args(rope, d->head_dim, a) || !aule_hip::fwd_rope_fusable(a)) {
            set_error("Attention failed: the query rotation is not fused for this configuration "
                      "(aule_attention_forward_rope_fusable() == 0): rotate Q with aule_rope_ex() and call aule_attention_forward_ex()");
            return -3;
        }
    }
    return launched("Attention", aule_hip::launch_fwd(a, (hipStream_t)d->stream));
}

int32_t aule_attention_forward_ex(const aule_attn_desc* d) {
    RoctxRange range("aule.forward");
    return forward_impl(d, nullptr);
}

int32_t aule_attention_forward_rope_ex(const aule_attn_desc* d, const aule_attn_rope* rope) {
    RoctxRange range("aule.forward_rope");
    if (rope == nullptr) {
        std::lock_guard<std::mutex> lk(g_mu);
        set_error("Attention failed: null rotation descriptor");
        return -3;
    }
    return forward_impl(d, rope);
}

int32_t aule_attention_forward_rope_fusable(const aule_attn_desc* d, const aule_attn_rope* rope) {
    Reason text;
    if (rope == nullptr || attn_desc_error(d, sizeof(aule_attn_desc), text)) return 0;
    if (fwd_nothing_to_do(d) || d->seq_k == 0 || rope_fusable_too_large(d)) return 0;
    FwdArgs a;
    fill_fwd_args(d, a);
    return fill_rope_args(rope, d->head_dim, a) && aule_hip::fwd_rope_fusable(a) ? 1 : 0;
}

// The paged entry points.  Each rule of their descriptors -- its condition and its message -- is stated once, in the pieces below, and
// the checker of a kind is the pieces in that kind's order.  The kinds name their fields alike (the pieces are templates over the
// descriptor); aule_paged_fp8_desc is aule_paged_desc field for field plus the two scale pointers, aule_paged_query_desc that plus
// lse, seq_q and cache_dtype, and aule_paged_cascade_desc is aule_paged_prefill_desc but for the word at 48 plus the prefix and the
// workspace (the layout asserts at the top of this file), so those kinds are read through the common prefix.
static const aule_paged_desc* paged_prefix(const aule_paged_fp8_desc* d) { return reinterpret_cast<const aule_paged_desc*>(d); }
static const aule_paged_prefill_desc* prefill_prefix(const aule_paged_cascade_desc* d) { return reinterpret_cast<const aule_paged_prefill_desc*>(d); }

static bool is_16_bit(int32_t dtype) { return dtype == AULE_DTYPE_F16 || dtype == AULE_DTYPE_BF16; }
static const char kDtypeOfQ[] = "dtype (of q / out) must be fp16 or bf16";
static bool misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

static const char* cache_dtype_error(int32_t cache_dtype) {
    if (cache_dtype != AULE_KV_CACHE_SAME && cache_dtype != AULE_KV_CACHE_FP8_E4M3) return "cache_dtype must be AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3";
    return nullptr;
}

static const char* scale_pointer_error(bool fp8, const float* k_scale, const float* v_scale) {
    if (fp8 && (!k_scale || !v_scale)) return "null scale pointer (k_scale and v_scale are [heads_kv] fp32 device arrays)";
    if (!fp8 && (k_scale || v_scale)) return "k_scale / v_scale apply to FP8 caches only; a 16-bit cache holds the values themselves";
    return nullptr;
}

extern "C++" {   // (templates, inside this file's extern "C")
// the kinds with a cache_dtype field (every one but the decode's two)
template <class Desc>
static const char* paged_dtype_error(const Desc* d) {
    if (!is_16_bit(d->dtype)) return kDtypeOfQ;
    return cache_dtype_error(d->cache_dtype);
}

template <class Desc>
static const char* paged_heads_error(const Desc* d, Reason& why) {
    if (d->head_dim != 32 && d->head_dim != 64 && d->head_dim != 128) return reasonf(why, "head_dim %u unsupported (32, 64 or 128)", d->head_dim);
    return head_ratio_error(d->heads_q, d->heads_kv, why);
}

static bool bad_block_table(uint32_t block_size, uint32_t blocks) { return block_size == 0 || blocks == 0 || (uint64_t)block_size * blocks >= (1ull << 30); }

template <class Desc>
static const char* paged_blocks_error(const Desc* d) { return bad_block_table(d->block_size, d->max_blocks) ? "bad block_size / max_blocks" : nullptr; }

// the packed ragged queries of the prefill and the cascade
template <class Desc>
static const char* ragged_query_error(const Desc* d, Reason& why) {
    if (d->max_seqlen_q == 0) return "max_seqlen_q must be at least 1";
    if (d->q_token_stride < (int64_t)d->heads_q * d->head_dim)
        return reasonf(why, "q_token_stride (%lld) is smaller than a token (heads_q * head_dim = %llu elements)", (long long)d->q_token_stride,
                       (unsigned long long)d->heads_q * d->head_dim);
    if (d->q_token_stride % 8 != 0) return reasonf(why, "q_token_stride (%lld) must be a multiple of 8 elements (16-byte loads)", (long long)d->q_token_stride);
    if (d->batch >= (1u << 30) || d->total_tokens >= (1u << 30)) return "batch / total_tokens too large";
    if (((uint64_t)d->total_tokens + 128) * (d->heads_q / d->heads_kv) > 0x7fffffffull) return "total_tokens * (heads_q / heads_kv) too large (packed rows are counted in 32 bits)";
    return nullptr;
}

template <class Desc>
static bool ragged_nothing_to_do(const Desc* d) { return d->total_tokens == 0 || (uint64_t)d->batch * d->heads_q == 0; }

// The pointers of a call that has something to do: the six tensors every kind has (`more_tensors`: whether the kind's own are all
// there), then the scale pair; paged_alignment_error: for the kernels that load 16 bytes at a time.
template <class Desc>
static const char* paged_pointer_error(const Desc* d, bool more_tensors, bool fp8, const float* k_scale, const float* v_scale) {
    if (!d->q || !d->k_cache || !d->v_cache || !d->block_tables || !d->context_lens || !d->out || !more_tensors) return "null tensor pointer";
    return scale_pointer_error(fp8, k_scale, v_scale);
}

template <class Desc>
static const char* paged_alignment_error(const Desc* d) {
    if (misaligned(d->q) || misaligned(d->out) || misaligned(d->k_cache) || misaligned(d->v_cache)) return "q, out and the caches must be 16-byte aligned";
    return nullptr;
}

// what the prefill and the cascade share, before and after their own rules
template <class Desc>
static const char* ragged_desc_error(const Desc* d, Reason& why) {
    if (const char* e = paged_dtype_error(d)) return e;
    if (const char* e = paged_heads_error(d, why)) return e;
    return paged_blocks_error(d);
}

template <class Desc>
static const char* ragged_pointer_error(const Desc* d, bool more_tensors) {
    if (const char* e = paged_pointer_error(d, d->cu_seqlens_q && more_tensors, d->cache_dtype == AULE_KV_CACHE_FP8_E4M3, d->k_scale, d->v_scale)) return e;
    return paged_alignment_error(d);
}
}   // extern "C++"

static bool paged_nothing_to_do(const aule_paged_desc* d) { return (uint64_t)d->batch * d->heads_q == 0; }

// The decode's two kinds (no cache_dtype: the kind says it, and names the dtype in its own words).  One checker for their two readers;
// `launch`: the pointer rules of a call that has something to do as well (the size queries read no pointer).
static const char* paged_desc_error(const aule_paged_desc* d, bool fp8, bool launch, Reason& why) {
    if (d == nullptr || d->struct_size != (fp8 ? sizeof(aule_paged_fp8_desc) : sizeof(aule_paged_desc))) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return fp8 ? kDtypeOfQ : "dtype must be fp16 or bf16";
    if (const char* e = paged_heads_error(d, why)) return e;
    if (const char* e = paged_blocks_error(d)) return e;
    if (!launch || paged_nothing_to_do(d)) return nullptr;
    const aule_paged_fp8_desc* d8 = reinterpret_cast<const aule_paged_fp8_desc*>(d);   // (read where `d` is one)
    return paged_pointer_error(d, true, fp8, fp8 ? d8->k_scale : nullptr, fp8 ? d8->v_scale : nullptr);
}

// (`d` passed paged_desc_error: an FP8 descriptor really is one)
static void fill_paged_args(const aule_paged_desc* d, bool fp8, aule_hip::PagedArgs& a) {
    a.q = d->q; a.k_cache = d->k_cache; a.v_cache = d->v_cache; a.out = d->out;
    a.block_tables = d->block_tables; a.context_lens = d->context_lens;
    a.B = (int)d->batch; a.Hq = (int)d->heads_q; a.Hkv = (int)d->heads_kv; a.D = (int)d->head_dim;
    a.block_size = (int)d->block_size; a.max_blocks = (int)d->max_blocks;
    a.scale = resolve_scale(d->scale, d->head_dim);
    a.window = d->window_size;
    a.dtype = d->dtype;
    a.ws = d->workspace; a.ws_bytes = d->workspace ? d->workspace_bytes : 0;
    if (fp8) {
        const aule_paged_fp8_desc* d8 = reinterpret_cast<const aule_paged_fp8_desc*>(d);
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.k_scale = d8->k_scale; a.v_scale = d8->v_scale;
    }
}

static int32_t paged_decode_impl(const aule_paged_desc* d, bool fp8) {
    const char* const what = fp8 ? "Paged FP8 attention" : "Paged attention";
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    Reason text;
    if (const char* why = paged_desc_error(d, fp8, true, text)) {
        set_error("%s failed: %s", what, why);
        return -3;
    }
    if (paged_nothing_to_do(d)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_args(d, fp8, a);
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched(what, aule_hip::launch_paged_decode(a, (hipStream_t)d->stream));
}

int32_t aule_attention_paged_decode_ex(const aule_paged_desc* d) {
    RoctxRange range("aule.paged_decode");
    return paged_decode_impl(d, false);
}

int32_t aule_attention_paged_decode_fp8_ex(const aule_paged_fp8_desc* d) {
    RoctxRange range("aule.paged_decode_fp8");
    return paged_decode_impl(paged_prefix(d), true);
}

// The paged query.  One checker for its two readers; `launch`: the pointer rules of a call that has something to do as well (the
// size query reads no pointer).
static bool paged_query_nothing_to_do(const aule_paged_query_desc* d) { return (uint64_t)d->batch * d->heads_q == 0; }

// (`size`: the kind's own sizeof -- aule_paged_query_sink_desc is read through this type)
static const char* paged_query_desc_error(const aule_paged_query_desc* d, bool launch, Reason& why, size_t size = sizeof(aule_paged_query_desc)) {
    if (d == nullptr || d->struct_size != size) return kBadDescriptor;
    if (const char* e = paged_dtype_error(d)) return e;
    if (const char* e = paged_heads_error(d, why)) return e;
    if (d->seq_q == 0 || d->seq_q > 64) return reasonf(why, "seq_q %u unsupported (1 to 64 query tokens per sequence)", d->seq_q);
    if (const char* e = paged_blocks_error(d)) return e;
    if (!launch || paged_query_nothing_to_do(d)) return nullptr;
    return paged_pointer_error(d, true, d->cache_dtype == AULE_KV_CACHE_FP8_E4M3, d->k_scale, d->v_scale);
}

// (`d` passed paged_query_desc_error)
static void fill_paged_query_args(const aule_paged_query_desc* d, aule_hip::PagedArgs& a) {
    fill_paged_args(reinterpret_cast<const aule_paged_desc*>(d), d->cache_dtype == AULE_KV_CACHE_FP8_E4M3, a);
    a.Sq = (int)d->seq_q;
    a.lse = d->lse;
}

int32_t aule_attention_paged_query_ex(const aule_paged_query_desc* d) {
    RoctxRange range("aule.paged_query");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    Reason text;
    if (const char* why = paged_query_desc_error(d, true, text)) {
        set_error("Paged query attention failed: %s", why);
        return -3;
    }
    if (paged_query_nothing_to_do(d)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_query_args(d, a);
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched("Paged query attention", aule_hip::launch_paged_query(a, (hipStream_t)d->stream));
}

// The sink kinds (attention sinks: include/aule.h): each is its twin's descriptor plus pointers, checked by the twin's checker with its
// own size and read through the twin's type (the layout asserts at the top of this file); a null sinks is refused once there is
// something to do.  Host logic first: a refusal and a call with nothing to do are answered before the device is needed.
static const char kNullSinks[] = "null sinks pointer (sinks is a [heads_q] fp32 device array; -inf entries mean no sink)";
static const aule_paged_query_desc* query_prefix(const aule_paged_query_sink_desc* d) { return reinterpret_cast<const aule_paged_query_desc*>(d); }
static const aule_paged_prefill_desc* prefill_sink_prefix(const aule_paged_prefill_sink_desc* d) { return reinterpret_cast<const aule_paged_prefill_desc*>(d); }

int32_t aule_attention_paged_query_sink_ex(const aule_paged_query_sink_desc* d) {
    RoctxRange range("aule.paged_query_sink");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const aule_paged_query_desc* x = query_prefix(d);
    const char* why = paged_query_desc_error(x, true, text, sizeof(aule_paged_query_sink_desc));
    if (why == nullptr && !paged_query_nothing_to_do(x) && d->sinks == nullptr) why = kNullSinks;
    if (why != nullptr) {
        set_error("Paged query sink attention failed: %s", why);
        return -3;
    }
    if (paged_query_nothing_to_do(x)) return 0;
    if (!initialised()) return -1;
    aule_hip::PagedArgs a;
    fill_paged_query_args(x, a);
    a.sinks = d->sinks;
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched("Paged query sink attention", aule_hip::launch_paged_query(a, (hipStream_t)d->stream));
}

// The paged prefill and the paged cascade: packed ragged queries, a descriptor family of its own.  `launch`: the pointer rules of a
// call that has something to do as well (the cascade's size query and plan hook read no pointer).  Host logic only, and the launch
// entries ask before they need the device.
// (`size`: the kind's own sizeof -- aule_paged_prefill_sink_desc is read through this type)
static const char* paged_prefill_desc_error(const aule_paged_prefill_desc* d, Reason& why, size_t size = sizeof(aule_paged_prefill_desc)) {
    if (d == nullptr || d->struct_size != size) return kBadDescriptor;
    if (const char* e = ragged_desc_error(d, why)) return e;
    if (const char* e = ragged_query_error(d, why)) return e;
    return ragged_nothing_to_do(d) ? nullptr : ragged_pointer_error(d, true);
}

static const char* paged_cascade_desc_error(const aule_paged_cascade_desc* d, bool launch, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_paged_cascade_desc)) return kBadDescriptor;
    if (const char* e = ragged_desc_error(d, why)) return e;
    if (bad_block_table(d->block_size, d->max_prefix_blocks)) return "bad block_size / max_prefix_blocks";
    if (const char* e = ragged_query_error(d, why)) return e;
    return !launch || ragged_nothing_to_do(d) ? nullptr : ragged_pointer_error(d, d->prefix_block_table && d->prefix_len);
}

// (`d` passed paged_prefill_desc_error, or is the prefix of a cascade descriptor that passed its checker: then the window is not `d`'s to state)
static void fill_paged_prefill_args(const aule_paged_prefill_desc* d, aule_hip::PagedPrefillArgs& a) {
    a.q = d->q; a.k_cache = d->k_cache; a.v_cache = d->v_cache; a.out = d->out; a.lse = d->lse;
    a.block_tables = d->block_tables; a.context_lens = d->context_lens; a.cu_seqlens_q = d->cu_seqlens_q;
    a.T = (int)d->total_tokens; a.B = (int)d->batch; a.Hq = (int)d->heads_q; a.Hkv = (int)d->heads_kv; a.D = (int)d->head_dim;
    a.max_seqlen_q = aule_hip::seqlen_cut(d->max_seqlen_q, d->total_tokens);
    a.q_token_stride = d->q_token_stride;
    a.block_size = (int)d->block_size; a.max_blocks = (int)d->max_blocks;
    a.scale = resolve_scale(d->scale, d->head_dim);
    a.window = d->window_size;
    a.dtype = d->dtype;
    if (d->cache_dtype == AULE_KV_CACHE_FP8_E4M3) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.k_scale = d->k_scale; a.v_scale = d->v_scale;
    }
}

// (`d` passed paged_prefill_desc_error with its kind's size; `sinks` / `tree_mask`: the sink kind's logits and the tree kind's words, checked
// by the caller)
// `launch`: the kernel family behind the entry (the FP8-product twin passes its own)
using PagedPrefillLauncher = int (*)(const aule_hip::PagedPrefillArgs&, hipStream_t);
static int32_t paged_prefill_launch(const aule_paged_prefill_desc* d, const float* sinks, const char* what, const int64_t* tree_mask = nullptr,
                                    PagedPrefillLauncher launch = aule_hip::launch_paged_prefill) {
    if (!initialised()) return -1;
    aule_hip::PagedPrefillArgs a;
    fill_paged_prefill_args(d, a);
    a.sinks = sinks;
    a.tree_mask = reinterpret_cast<const long long*>(tree_mask);
    if (aule_hip::paged_prefill_grid(a) > 0x7fffffffll) {
        set_error("%s failed: the grid (blocks * heads_kv * batch) exceeds 2^31 - 1 workgroups", what);
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched(what, launch(a, (hipStream_t)d->stream));
}

int32_t aule_attention_paged_prefill_ex(const aule_paged_prefill_desc* d) {
    RoctxRange range("aule.paged_prefill");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = paged_prefill_desc_error(d, text)) {
        set_error("Paged prefill attention failed: %s", why);
        return -3;
    }
    if (ragged_nothing_to_do(d)) return 0;
    return paged_prefill_launch(d, nullptr, "Paged prefill attention");
}

int32_t aule_attention_paged_prefill_sink_ex(const aule_paged_prefill_sink_desc* d) {
    RoctxRange range("aule.paged_prefill_sink");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const aule_paged_prefill_desc* x = prefill_sink_prefix(d);
    const char* why = paged_prefill_desc_error(x, text, sizeof(aule_paged_prefill_sink_desc));
    if (why == nullptr && !ragged_nothing_to_do(x) && d->sinks == nullptr) why = kNullSinks;
    if (why != nullptr) {
        set_error("Paged prefill sink attention failed: %s", why);
        return -3;
    }
    if (ragged_nothing_to_do(x)) return 0;
    return paged_prefill_launch(x, d->sinks, "Paged prefill sink attention");
}

// The tree kinds (tree masks: include/aule.h), read like the sink kinds: the twin's checker with the kind's own size, then the two rules of
// their own -- a window is not defined over a tree, and a null tree_mask is refused once there is something to do.  Host logic first.
static const char kNullTreeMask[] = "null tree_mask pointer (tree_mask is an int64 device array, one word per new token)";
static const char kTreeWindow[] = "window_size > 0: a sliding window is not defined over a tree";
static const aule_paged_query_desc* query_tree_prefix(const aule_paged_query_tree_desc* d) { return reinterpret_cast<const aule_paged_query_desc*>(d); }
static const aule_paged_prefill_desc* prefill_tree_prefix(const aule_paged_prefill_tree_desc* d) { return reinterpret_cast<const aule_paged_prefill_desc*>(d); }

int32_t aule_attention_paged_query_tree_ex(const aule_paged_query_tree_desc* d) {
    RoctxRange range("aule.paged_query_tree");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const aule_paged_query_desc* x = query_tree_prefix(d);
    const char* why = paged_query_desc_error(x, true, text, sizeof(aule_paged_query_tree_desc));
    if (why == nullptr && x->window_size > 0) why = kTreeWindow;
    if (why == nullptr && !paged_query_nothing_to_do(x) && d->tree_mask == nullptr) why = kNullTreeMask;
    if (why != nullptr) {
        set_error("Paged query tree attention failed: %s", why);
        return -3;
    }
    if (paged_query_nothing_to_do(x)) return 0;
    if (!initialised()) return -1;
    aule_hip::PagedArgs a;
    fill_paged_query_args(x, a);
    a.tree_mask = reinterpret_cast<const long long*>(d->tree_mask);
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched("Paged query tree attention", aule_hip::launch_paged_query(a, (hipStream_t)d->stream));
}

int32_t aule_attention_paged_prefill_tree_ex(const aule_paged_prefill_tree_desc* d) {
    RoctxRange range("aule.paged_prefill_tree");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const aule_paged_prefill_desc* x = prefill_tree_prefix(d);
    const char* why = paged_prefill_desc_error(x, text, sizeof(aule_paged_prefill_tree_desc));
    if (why == nullptr && x->window_size > 0) why = kTreeWindow;
    if (why == nullptr && !ragged_nothing_to_do(x) && d->tree_mask == nullptr) why = kNullTreeMask;
    if (why != nullptr) {
        set_error("Paged prefill tree attention failed: %s", why);
        return -3;
    }
    if (ragged_nothing_to_do(x)) return 0;
    return paged_prefill_launch(x, nullptr, "Paged prefill tree attention", d->tree_mask);
}

// The FP8-product twin of the paged prefill: the same descriptor through the same checker, then this kind's own two
// rules -- an FP8 cache is the only kind, head_dim 64 or 128 -- and its own launcher.  Host logic first, as above.
static const char kFp8mmaCache[] = "cache_dtype must be AULE_KV_CACHE_FP8_E4M3: this entry multiplies the cache's e4m3fn codes as they are "
                                   "(a 16-bit cache: aule_attention_paged_prefill_ex)";

int32_t aule_attention_paged_prefill_fp8mma_ex(const aule_paged_prefill_desc* d) {
    RoctxRange range("aule.paged_prefill_fp8mma");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const char* why = paged_prefill_desc_error(d, text);
    if (why == nullptr && d->cache_dtype != AULE_KV_CACHE_FP8_E4M3) why = kFp8mmaCache;
    if (why == nullptr && d->head_dim != 64 && d->head_dim != 128)
        why = reasonf(text, "head_dim %u unsupported by the FP8-product prefill (64 or 128; head_dim 32: aule_attention_paged_prefill_ex)", d->head_dim);
    if (why != nullptr) {
        set_error("Paged prefill FP8-product attention failed: %s", why);
        return -3;
    }
    if (ragged_nothing_to_do(d)) return 0;
    return paged_prefill_launch(d, nullptr, "Paged prefill FP8-product attention", nullptr, aule_hip::launch_paged_prefill_fp8mma);
}

// (`d` passed paged_cascade_desc_error) the two kernels' arguments: the suffix pass is the prefill's, read through the common prefix,
// without a window (the word at 48 is max_prefix_blocks here); the prefix pass is derived from it.  part / lse of the workspace are the
// launch entry's to set.
static void fill_paged_cascade_args(const aule_paged_cascade_desc* d, aule_hip::SharedPrefixArgs& x, aule_hip::PagedPrefillArgs& a) {
    fill_paged_prefill_args(prefill_prefix(d), a);
    a.window = -1;
    x.q = a.q; x.k_cache = a.k_cache; x.v_cache = a.v_cache;
    x.prefix_block_table = d->prefix_block_table; x.prefix_len = d->prefix_len;
    x.T = a.T; x.Hq = a.Hq; x.Hkv = a.Hkv; x.D = a.D;
    x.q_token_stride = a.q_token_stride;
    x.block_size = a.block_size; x.max_prefix_blocks = (int)d->max_prefix_blocks;
    x.scale = a.scale; x.dtype = a.dtype;
    x.cache_kind = a.cache_kind; x.k_scale = a.k_scale; x.v_scale = a.v_scale;
    x.device = d->device;
}

int32_t aule_attention_paged_cascade_ex(const aule_paged_cascade_desc* d) {
    RoctxRange range("aule.paged_cascade");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = paged_cascade_desc_error(d, true, text)) {
        set_error("Paged cascade attention failed: %s", why);
        return -3;
    }
    if (ragged_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::SharedPrefixArgs x;
    aule_hip::PagedPrefillArgs a;
    fill_paged_cascade_args(d, x, a);
    const aule_hip::SharedPrefixPlan plan = aule_hip::shared_prefix_plan(x);
    aule_hip::CascadeMergeArgs m;
    m.nsplit = plan.nsplit; m.out = a.out;
    m.context_lens = a.context_lens; m.cu_seqlens_q = a.cu_seqlens_q;
    m.T = a.T; m.B = a.B; m.Hq = a.Hq; m.D = a.D;
    m.max_seqlen_q = a.max_seqlen_q; m.own_capacity = a.block_size * a.max_blocks; m.dtype = a.dtype;
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll || aule_hip::paged_prefill_grid(a) > 0x7fffffffll || aule_hip::cascade_merge_grid(m) > 0x7fffffffll) {
        set_error("Paged cascade attention failed: a grid exceeds 2^31 - 1 workgroups");
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)d->stream;
    aule_hip::ScopedWorkspace ws(plan.ws_bytes, d->workspace, d->workspace ? d->workspace_bytes : 0, stream);
    if (ws.err != hipSuccess) {
        set_error("Paged cascade attention failed: workspace allocation (%llu bytes): %s", (unsigned long long)plan.ws_bytes, hipGetErrorString(ws.err));
        return -4;
    }
    x.part = static_cast<float*>(ws.ptr);
    if (a.lse == nullptr) a.lse = reinterpret_cast<float*>(static_cast<char*>(ws.ptr) + plan.lse_offset);
    m.part = x.part; m.lse = a.lse;
    rc = aule_hip::launch_shared_prefix(x, plan, stream);
    if (rc == 0) rc = aule_hip::launch_paged_prefill(a, stream);
    if (rc == 0) rc = aule_hip::launch_cascade_merge(m, stream);
    return launched("Paged cascade attention", rc);
}

// The paged MLA: one latent cache, 576 / 512, ragged queries as the prefill's or plain decode (null cu_seqlens_q).  Three kinds:
// aule_mla_paged_fp8_desc is aule_mla_paged_desc field for field plus kv_scale, aule_mla_paged_tree_desc is that plus tree_mask and
// cache_dtype (the layout asserts at the top of this file), so all are checked and read through that prefix; `kind` says which one
// `d` is.  One checker for all their readers, built from the paged kinds'
// pieces where the fields are alike; `launch`: the pointer rules of a call that has something to do as well (the size queries and the
// plan hook read no pointer).  Host logic only, asked before the device is needed.
extern "C++" {
// (the kinds whose cu_seqlens_q may be null -- plain decode, sequence b owns row b -- read max_seqlen_q as 1 then; else the cut)
template <class Desc>
static int max_sq_or_one(const Desc* d) { return d->cu_seqlens_q == nullptr ? 1 : aule_hip::seqlen_cut(d->max_seqlen_q, d->total_tokens); }

// (the tail of both MLA launch entries: the device, the workspace of a split plan -- the caller's buffer when it is large enough, else a
// stream-ordered allocation -- and the launch; `launch(ws, stream)`: the kind's launcher with its arguments and `plan`)
template <class Desc, class Launch>
static int32_t mla_launch_tail(const Desc* d, const aule_hip::MlaPlan& plan, const char* what, Launch&& launch) {
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)d->stream;
    if (plan.nsplit == 1) return launched(what, launch(nullptr, stream));
    aule_hip::ScopedWorkspace ws(plan.ws_bytes, d->workspace, d->workspace ? d->workspace_bytes : 0, stream);
    if (ws.err != hipSuccess) {
        set_error("%s failed: workspace allocation (%llu bytes): %s", what, (unsigned long long)plan.ws_bytes, hipGetErrorString(ws.err));
        return -4;
    }
    return launched(what, launch(ws.ptr, stream));
}
}   // extern "C++"

enum MlaKind { kMla16, kMlaFp8, kMlaTree };
static const aule_mla_paged_desc* mla_prefix(const aule_mla_paged_fp8_desc* d) { return reinterpret_cast<const aule_mla_paged_desc*>(d); }
static const aule_mla_paged_desc* mla_tree_prefix(const aule_mla_paged_tree_desc* d) { return reinterpret_cast<const aule_mla_paged_desc*>(d); }
// (`d` read as the larger kinds, where `kind` says it is one)
static const aule_mla_paged_tree_desc* mla_tree(const aule_mla_paged_desc* d) { return reinterpret_cast<const aule_mla_paged_tree_desc*>(d); }
static size_t mla_desc_size(MlaKind kind) {
    return kind == kMlaTree ? sizeof(aule_mla_paged_tree_desc) : kind == kMlaFp8 ? sizeof(aule_mla_paged_fp8_desc) : sizeof(aule_mla_paged_desc);
}
// (the cache holds e4m3fn codes: the FP8 kind, or the tree kind with that cache_dtype; `d` has its kind's size)
static bool mla_cache_is_fp8(const aule_mla_paged_desc* d, MlaKind kind) {
    return kind == kMlaFp8 || (kind == kMlaTree && mla_tree(d)->cache_dtype == AULE_KV_CACHE_FP8_E4M3);
}
static const char* varlen_stride_error(const char* name, int64_t stride, uint64_t token, const char* heads, Reason& why);   // (the token stride rule, below)
static const char* mla_paged_desc_error(const aule_mla_paged_desc* d, MlaKind kind, bool launch, Reason& why) {
    if (d == nullptr || d->struct_size != mla_desc_size(kind)) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return kind != kMla16 ? kDtypeOfQ : "dtype (of q / out / kv_cache) must be fp16 or bf16";
    if (kind == kMlaTree && cache_dtype_error(mla_tree(d)->cache_dtype))
        return reasonf(why, "cache_dtype %d must be AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3", mla_tree(d)->cache_dtype);
    const bool fp8 = mla_cache_is_fp8(d, kind);
    if (d->qk_dim != 576 || d->v_dim != 512) return reasonf(why, "qk_dim %u / v_dim %u unsupported (576 / 512 only)", d->qk_dim, d->v_dim);
    if (const char* e = paged_blocks_error(d)) return e;
    if (d->max_seqlen_q == 0) return "max_seqlen_q must be at least 1";
    if (const char* e = varlen_stride_error("q", d->q_token_stride, (uint64_t)d->heads_q * d->qk_dim, "heads_q", why)) return e;
    if (d->batch >= (1u << 30) || d->total_tokens >= (1u << 30)) return "batch / total_tokens too large";
    if (((uint64_t)d->total_tokens + 64) * d->heads_q > 0x7fffffffull) return "total_tokens * heads_q too large (packed rows are counted in 32 bits)";
    if (ragged_nothing_to_do(d)) return nullptr;
    if (kind == kMlaTree && d->cu_seqlens_q == nullptr)
        return "null cu_seqlens_q (a tree of one node per sequence is the decode call: aule_attention_mla_paged_ex / _fp8_ex)";
    if (d->cu_seqlens_q == nullptr && d->total_tokens < d->batch) return "cu_seqlens_q is null (plain decode: sequence b owns row b) and total_tokens < batch";
    if (!launch) return nullptr;
    if (!d->q || !d->kv_cache || !d->block_tables || !d->context_lens || !d->out) return "null tensor pointer";
    if (misaligned(d->q) || misaligned(d->out) || misaligned(d->kv_cache)) return "q, out and kv_cache must be 16-byte aligned";
    if (fp8) {
        const float* kv_scale = reinterpret_cast<const aule_mla_paged_fp8_desc*>(d)->kv_scale;   // (read where `d` is one)
        if (kv_scale == nullptr) return "null kv_scale (one fp32 value on the device)";
        if ((reinterpret_cast<uintptr_t>(kv_scale) & 3) != 0) return "kv_scale must be 4-byte aligned";
    }
    if (kind == kMlaTree) {
        if (!fp8 && mla_tree(d)->kv_scale != nullptr) return "kv_scale applies to an FP8 cache only (cache_dtype AULE_KV_CACHE_FP8_E4M3)";
        if (mla_tree(d)->tree_mask == nullptr) return kNullTreeMask;
        if ((reinterpret_cast<uintptr_t>(mla_tree(d)->tree_mask) & 7) != 0) return "tree_mask must be 8-byte aligned";
    }
    return nullptr;
}

// (`d` passed mla_paged_desc_error with the same `kind`)
static void fill_mla_paged_args(const aule_mla_paged_desc* d, MlaKind kind, aule_hip::MlaArgs& a) {
    a.q = d->q; a.kv_cache = d->kv_cache; a.out = d->out; a.lse = d->lse;
    a.block_tables = d->block_tables; a.context_lens = d->context_lens; a.cu_seqlens_q = d->cu_seqlens_q;
    a.T = (int)d->total_tokens; a.B = (int)d->batch; a.Hq = (int)d->heads_q;
    a.max_seqlen_q = max_sq_or_one(d);
    a.q_token_stride = d->q_token_stride;
    a.block_size = (int)d->block_size; a.max_blocks = (int)d->max_blocks;
    a.scale = resolve_scale(d->scale, d->qk_dim);
    a.dtype = d->dtype;
    a.device = d->device;
    if (mla_cache_is_fp8(d, kind)) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.kv_scale = reinterpret_cast<const aule_mla_paged_fp8_desc*>(d)->kv_scale;
    }
    if (kind == kMlaTree) a.tree_mask = reinterpret_cast<const long long*>(mla_tree(d)->tree_mask);
}

// (every kind's launch entry; `what`: the kind's error prefix)
static int32_t mla_paged_launch(const aule_mla_paged_desc* d, MlaKind kind, const char* what) {
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_paged_desc_error(d, kind, true, text)) {
        set_error("%s failed: %s", what, why);
        return -3;
    }
    if (ragged_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaArgs a;
    fill_mla_paged_args(d, kind, a);
    const aule_hip::MlaPlan plan = aule_hip::mla_plan(a);
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll) {
        set_error("%s failed: the grid (row blocks * nsplit * batch) exceeds 2^31 - 1 workgroups", what);
        return -3;
    }
    return mla_launch_tail(d, plan, what, [&](void* ws, hipStream_t stream) { return aule_hip::launch_mla_paged(a, plan, ws, stream); });
}

int32_t aule_attention_mla_paged_ex(const aule_mla_paged_desc* d) {
    RoctxRange range("aule.mla_paged");
    return mla_paged_launch(d, kMla16, "Paged MLA attention");
}

int32_t aule_attention_mla_paged_fp8_ex(const aule_mla_paged_fp8_desc* d) {
    RoctxRange range("aule.mla_paged_fp8");
    return mla_paged_launch(mla_prefix(d), kMlaFp8, "Paged MLA FP8 attention");
}

int32_t aule_attention_mla_paged_tree_ex(const aule_mla_paged_tree_desc* d) {
    RoctxRange range("aule.mla_paged_tree");
    return mla_paged_launch(mla_tree_prefix(d), kMlaTree, "Paged MLA tree attention");
}

// The sparse MLA: per-token key lists over the latent cache, both cache kinds in one descriptor.  One checker for all its readers;
// `launch`: the pointer and workspace rules of a call that has something to do as well (the size query and the plan hook read no
// pointer).  Host logic only, asked before the device is needed.
static bool mla_sparse_nothing_to_do(const aule_mla_sparse_desc* d) { return d->total_tokens == 0; }

// (`d` passed the field rules of mla_sparse_desc_error: mla_sparse_plan reads the shape, none of the pointers)
// (force_nsplit > 0: the bench's debug launch alone, aule_hip_debug_mla_sparse_launch_nsplit)
static aule_hip::MlaPlan mla_sparse_plan_of(const aule_mla_sparse_desc* d, int force_nsplit = 0) {
    return aule_hip::mla_sparse_plan((int)d->total_tokens, (int)d->heads_q, (int)d->topk, d->device, force_nsplit);
}

static const char* mla_sparse_desc_error(const aule_mla_sparse_desc* d, bool launch, Reason& why, int force_nsplit = 0) {
    if (d == nullptr || d->struct_size != sizeof(aule_mla_sparse_desc)) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return reasonf(why, "dtype %d (of q / out) must be fp16 or bf16", d->dtype);
    if (cache_dtype_error(d->cache_dtype)) return reasonf(why, "cache_dtype %d must be AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3", d->cache_dtype);
    if (d->heads_q < 1) return reasonf(why, "heads_q (%d) must be at least 1", d->heads_q);
    if (d->topk < 1 || d->topk > aule_hip::kMlaSparseMaxTopk) return reasonf(why, "topk (%d) must be in 1 .. %d", d->topk, aule_hip::kMlaSparseMaxTopk);
    const uint64_t slots = (uint64_t)d->num_blocks * d->block_size;
    if (slots < 1 || slots > 0x7fffffffull)
        return reasonf(why, "num_blocks * block_size (%u * %u) must be in 1 .. 2^31 - 1 (slots are int32)", d->num_blocks, d->block_size);
    if (d->total_tokens < 0) return reasonf(why, "total_tokens (%d) must not be negative", d->total_tokens);
    if (const char* e = varlen_stride_error("q", d->q_token_stride, (uint64_t)d->heads_q * 576, "heads_q", why)) return e;
    if (((uint64_t)d->total_tokens + 64) * (uint64_t)d->heads_q > 0x7fffffffull)
        return reasonf(why, "total_tokens * heads_q (%d * %d) too large (packed rows are counted in 32 bits)", d->total_tokens, d->heads_q);
    if (mla_sparse_nothing_to_do(d)) return nullptr;
    const aule_hip::MlaPlan plan = mla_sparse_plan_of(d, force_nsplit);
    // (not reachable while (total_tokens + 64) * heads_q fits 32 bits and nsplit > 1 needs total_tokens * row blocks below the CU
    // count: kept as the statement of the rule, should either bound move)
    if (plan.grid > 0x7fffffffll || (long long)plan.row_blocks * d->total_tokens * 16 > 0x7fffffffll)
        return reasonf(why, "the grid (total_tokens %d * row blocks %d * nsplit %d, or * 16 for the combine) exceeds 2^31 - 1 workgroups",
                       d->total_tokens, plan.row_blocks, plan.nsplit);
    if (!launch) return nullptr;
    if (!d->q || !d->kv_cache || !d->indices || !d->out) return "null tensor pointer (q, kv_cache, indices and out are required)";
    if (misaligned(d->q) || misaligned(d->out) || misaligned(d->kv_cache)) return "q, out and kv_cache must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(d->indices) & 3) != 0) return "indices must be 4-byte aligned";
    const bool fp8 = d->cache_dtype == AULE_KV_CACHE_FP8_E4M3;
    if (fp8 && !d->kv_scale) return "null kv_scale (an FP8 cache needs one fp32 value on the device)";
    if (!fp8 && d->kv_scale) return "kv_scale applies to an FP8 cache only; a 16-bit cache holds the values themselves";
    if ((reinterpret_cast<uintptr_t>(d->kv_scale) & 3) != 0) return "kv_scale must be 4-byte aligned";
    if (d->workspace != nullptr) {
        if (d->workspace_bytes < plan.ws_bytes)
            return reasonf(why, "workspace_bytes (%llu) is smaller than the plan's %llu", (unsigned long long)d->workspace_bytes, (unsigned long long)plan.ws_bytes);
        if (misaligned(d->workspace)) return "workspace must be 16-byte aligned";
    }
    return nullptr;
}

// (the launch entry, and with force_nsplit > 0 the bench's debug launch)
static int32_t mla_sparse_launch(const aule_mla_sparse_desc* d, int force_nsplit) {
    const char* what = "Sparse MLA attention";
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_sparse_desc_error(d, true, text, force_nsplit)) {
        set_error("%s failed: %s", what, why);
        return -3;
    }
    if (mla_sparse_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaSparseArgs a;
    a.q = d->q; a.kv_cache = d->kv_cache; a.out = d->out; a.lse = d->lse;
    a.indices = d->indices;
    a.T = (int)d->total_tokens; a.Hq = (int)d->heads_q;
    a.topk = (int)d->topk;
    a.slots = (int)((uint64_t)d->num_blocks * d->block_size);
    a.q_token_stride = d->q_token_stride;
    a.scale = resolve_scale(d->scale, 576);
    a.dtype = d->dtype;
    a.device = d->device;
    if (d->cache_dtype == AULE_KV_CACHE_FP8_E4M3) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.kv_scale = d->kv_scale;
    }
    const aule_hip::MlaPlan plan = mla_sparse_plan_of(d, force_nsplit);
    return mla_launch_tail(d, plan, what, [&](void* ws, hipStream_t stream) { return aule_hip::launch_mla_sparse(a, plan, ws, stream); });
}

int32_t aule_attention_mla_sparse_ex(const aule_mla_sparse_desc* d) {
    RoctxRange range("aule.mla_sparse");
    return mla_sparse_launch(d, 0);
}

// The MLA indexer: index logits and top-k key lists, one checker per kind; `launch`: the pointer rules of a call that has something to
// do as well (the plan hook reads no pointer).  Host logic only, asked before the device is needed.  What the two kinds share -- the
// table, the ragged queries, the logits' row stride -- is stated once.
extern "C++" {
template <class Desc>
static bool indexer_nothing_to_do(const Desc* d) { return d->total_tokens == 0 || d->batch == 0; }

template <class Desc>
static const char* indexer_shape_error(const Desc* d, Reason& why) {
    if (bad_block_table(d->block_size, d->max_blocks))
        return reasonf(why, "block_size (%u) and max_blocks (%u) must be positive and block_size * max_blocks below 2^30", d->block_size, d->max_blocks);
    if (d->max_seqlen_q == 0) return "max_seqlen_q must be at least 1";
    const int64_t W = (int64_t)d->block_size * d->max_blocks;
    if (d->logits_stride < W)
        return reasonf(why, "logits_stride (%lld) is smaller than a row (max_blocks * block_size = %lld columns)", (long long)d->logits_stride, (long long)W);
    if (d->batch >= (1u << 30)) return reasonf(why, "batch (%u) too large", d->batch);
    if (d->total_tokens >= (1u << 30)) return reasonf(why, "total_tokens (%u) too large", d->total_tokens);
    if (indexer_nothing_to_do(d)) return nullptr;
    if (d->cu_seqlens_q == nullptr && d->total_tokens < d->batch)
        return reasonf(why, "cu_seqlens_q is null (plain decode: sequence b owns row b) and total_tokens (%u) < batch (%u)", d->total_tokens, d->batch);
    return nullptr;
}
}   // extern "C++"

// (`d` passed the field rules of mla_indexer_logits_desc_error: the plan reads the shape, none of the pointers but whether cu_seqlens_q is there)
static aule_hip::MlaIndexerPlan mla_indexer_plan_of(const aule_mla_indexer_logits_desc* d) {
    return aule_hip::mla_indexer_plan((int)d->batch, max_sq_or_one(d), (long long)d->block_size * d->max_blocks, d->device);
}

static const char* mla_indexer_logits_desc_error(const aule_mla_indexer_logits_desc* d, bool launch, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_mla_indexer_logits_desc)) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return reasonf(why, "dtype %d (of q) must be fp16 or bf16", d->dtype);
    if (cache_dtype_error(d->cache_dtype)) return reasonf(why, "cache_dtype %d must be AULE_KV_CACHE_SAME or AULE_KV_CACHE_FP8_E4M3", d->cache_dtype);
    if (d->heads < 1 || d->heads > (uint32_t)aule_hip::kMlaIndexerMaxHeads) return reasonf(why, "heads (%u) must be in 1 .. %d", d->heads, aule_hip::kMlaIndexerMaxHeads);
    if (d->head_dim != 128) return reasonf(why, "head_dim (%u) must be 128", d->head_dim);
    if (d->num_blocks == 0 || (uint64_t)d->num_blocks * d->block_size > 0x7fffffffull)
        return reasonf(why, "num_blocks * block_size (%u * %u) must be in 1 .. 2^31 - 1", d->num_blocks, d->block_size);
    if (const char* e = indexer_shape_error(d, why)) return e;
    if (const char* e = varlen_stride_error("q", d->q_token_stride, (uint64_t)d->heads * 128, "heads", why)) return e;
    if (indexer_nothing_to_do(d)) return nullptr;
    const aule_hip::MlaIndexerPlan plan = mla_indexer_plan_of(d);
    if (plan.grid > 0x7fffffffll)
        return reasonf(why, "the grid (batch %u * token groups %d * key chunks %d) exceeds 2^31 - 1 workgroups", d->batch, plan.token_groups, plan.key_chunks);
    if (!launch) return nullptr;
    if (!d->q || !d->weights || !d->k_cache || !d->block_tables || !d->context_lens || !d->logits)
        return "null tensor pointer (q, weights, k_cache, block_tables, context_lens and logits are required)";
    if (misaligned(d->q) || misaligned(d->k_cache)) return "q and k_cache must be 16-byte aligned";
    const bool fp8 = d->cache_dtype == AULE_KV_CACHE_FP8_E4M3;
    if (fp8 && !d->k_scale) return "null k_scale (an FP8 cache needs [num_blocks, block_size] fp32 values on the device)";
    if (!fp8 && d->k_scale) return "k_scale applies to an FP8 cache only; a 16-bit cache holds the values themselves";
    if (((reinterpret_cast<uintptr_t>(d->weights) | reinterpret_cast<uintptr_t>(d->k_scale) | reinterpret_cast<uintptr_t>(d->logits) |
          reinterpret_cast<uintptr_t>(d->block_tables) | reinterpret_cast<uintptr_t>(d->context_lens) | reinterpret_cast<uintptr_t>(d->cu_seqlens_q)) & 3) != 0)
        return "weights, k_scale, logits, block_tables, context_lens and cu_seqlens_q must be 4-byte aligned";
    return nullptr;
}

int32_t aule_mla_indexer_logits_ex(const aule_mla_indexer_logits_desc* d) {
    RoctxRange range("aule.mla_indexer_logits");
    const char* what = "MLA indexer logits";
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_indexer_logits_desc_error(d, true, text)) {
        set_error("%s failed: %s", what, why);
        return -3;
    }
    if (indexer_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaIndexerArgs a;
    a.q = d->q; a.weights = d->weights; a.k_cache = d->k_cache; a.logits = d->logits;
    a.block_tables = d->block_tables; a.context_lens = d->context_lens; a.cu_seqlens_q = d->cu_seqlens_q;
    a.T = (int)d->total_tokens; a.B = (int)d->batch; a.H = (int)d->heads;
    a.num_blocks = (int)d->num_blocks; a.block_size = (int)d->block_size; a.max_blocks = (int)d->max_blocks;
    a.max_seqlen_q = max_sq_or_one(d);
    a.q_token_stride = d->q_token_stride; a.logits_stride = d->logits_stride;
    a.dtype = d->dtype;
    a.device = d->device;
    if (d->cache_dtype == AULE_KV_CACHE_FP8_E4M3) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.k_scale = d->k_scale;
    }
    const aule_hip::MlaIndexerPlan plan = mla_indexer_plan_of(d);
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched(what, aule_hip::launch_mla_indexer_logits(a, plan, (hipStream_t)d->stream));
}

static const char* mla_indexer_topk_desc_error(const aule_mla_indexer_topk_desc* d, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_mla_indexer_topk_desc)) return kBadDescriptor;
    if (d->output != AULE_INDEXER_SLOTS && d->output != AULE_INDEXER_POSITIONS)
        return reasonf(why, "output %d must be AULE_INDEXER_SLOTS or AULE_INDEXER_POSITIONS", d->output);
    if (d->topk < 1 || d->topk > aule_hip::kMlaIndexerMaxTopk) return reasonf(why, "topk (%d) must be in 1 .. %d", d->topk, aule_hip::kMlaIndexerMaxTopk);
    if (d->reserved != 0) return reasonf(why, "reserved (%u) must be 0", d->reserved);
    if (const char* e = indexer_shape_error(d, why)) return e;
    if (indexer_nothing_to_do(d)) return nullptr;
    if ((uint64_t)d->batch * (uint64_t)max_sq_or_one(d) > 0x7fffffffull)
        return reasonf(why, "the grid (batch %u * max_seqlen_q %d) exceeds 2^31 - 1 workgroups", d->batch, max_sq_or_one(d));
    if (!d->logits || !d->block_tables || !d->context_lens || !d->indices)
        return "null tensor pointer (logits, block_tables, context_lens and indices are required)";
    if (((reinterpret_cast<uintptr_t>(d->logits) | reinterpret_cast<uintptr_t>(d->indices) | reinterpret_cast<uintptr_t>(d->block_tables) |
          reinterpret_cast<uintptr_t>(d->context_lens) | reinterpret_cast<uintptr_t>(d->cu_seqlens_q)) & 3) != 0)
        return "logits, indices, block_tables, context_lens and cu_seqlens_q must be 4-byte aligned";
    return nullptr;
}

int32_t aule_mla_indexer_topk_ex(const aule_mla_indexer_topk_desc* d) {
    RoctxRange range("aule.mla_indexer_topk");
    const char* what = "MLA indexer top-k";
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_indexer_topk_desc_error(d, text)) {
        set_error("%s failed: %s", what, why);
        return -3;
    }
    if (indexer_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaIndexerTopkArgs a;
    a.logits = d->logits; a.indices = d->indices;
    a.block_tables = d->block_tables; a.context_lens = d->context_lens; a.cu_seqlens_q = d->cu_seqlens_q;
    a.T = (int)d->total_tokens; a.B = (int)d->batch; a.topk = (int)d->topk;
    a.block_size = (int)d->block_size; a.max_blocks = (int)d->max_blocks;
    a.max_seqlen_q = max_sq_or_one(d);
    a.logits_stride = d->logits_stride;
    a.positions = d->output == AULE_INDEXER_POSITIONS;
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched(what, aule_hip::launch_mla_indexer_topk(a, (hipStream_t)d->stream));
}

// The variable-length kinds: aule_varlen_bwd_desc states the problem in aule_varlen_desc's fields up to cu_seqlens_k (the layout asserts
// at the top of this file), so both are checked and read through that prefix; what follows it is each kind's own.  One checker per
// kind; `launch`: the pointer and workspace rules of a call that has something to do as well (the size query reads no pointer).  Host
// logic only, and the launch entries ask before they need the device.
static const aule_varlen_desc* varlen_prefix(const aule_varlen_bwd_desc* d) { return reinterpret_cast<const aule_varlen_desc*>(d); }

static const char* varlen_stride_error(const char* name, int64_t stride, uint64_t token, const char* heads, Reason& why) {
    if (stride < (int64_t)token)
        return reasonf(why, "%s_token_stride (%lld) is smaller than a token (%s * head_dim = %llu elements)", name, (long long)stride, heads, (unsigned long long)token);
    if (stride % 8 != 0) return reasonf(why, "%s_token_stride (%lld) must be a multiple of 8 elements (16-byte loads)", name, (long long)stride);
    return nullptr;
}

// the problem statement (`size`: the kind's own sizeof)
static const char* varlen_problem_error(const aule_varlen_desc* d, size_t size, Reason& why) {
    if (d == nullptr || d->struct_size != size) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return "dtype must be fp16 or bf16 (fp32 is not built for variable-length batches)";
    if (const char* e = paged_heads_error(d, why)) return e;
    if (d->causal < 0 || d->causal > AULE_CAUSAL_BOTTOM_RIGHT) return reasonf(why, "unknown causal mode %d (0 none, 1 top-left, 2 bottom-right)", d->causal);
    if (d->max_seqlen_q == 0) return "max_seqlen_q must be at least 1";
    if (d->max_seqlen_k == 0) return "max_seqlen_k must be at least 1";
    if (const char* e = varlen_stride_error("q", d->q_token_stride, (uint64_t)d->heads_q * d->head_dim, "heads_q", why)) return e;
    if (const char* e = varlen_stride_error("k", d->k_token_stride, (uint64_t)d->heads_kv * d->head_dim, "heads_kv", why)) return e;
    if (const char* e = varlen_stride_error("v", d->v_token_stride, (uint64_t)d->heads_kv * d->head_dim, "heads_kv", why)) return e;
    if (d->batch >= (1u << 30) || d->total_q >= (1u << 30) || d->total_k >= (1u << 30)) return "batch / total_q / total_k too large";
    if (((uint64_t)d->total_q + 128) * (d->heads_q / d->heads_kv) > 0x7fffffffull) return "(total_q + 128) * (heads_q / heads_kv) too large (packed rows are counted in 32 bits)";
    return nullptr;
}

static bool varlen_fwd_nothing_to_do(const aule_varlen_desc* d) { return d->total_q == 0 || (uint64_t)d->batch * d->heads_q == 0; }
static bool varlen_bwd_nothing_to_do(const aule_varlen_desc* d) { return (uint64_t)d->batch * d->heads_q == 0 || (d->total_q == 0 && d->total_k == 0); }

// the pointers both kinds have: the offsets always, q with any query row, k and v with any key row
static const char* varlen_input_error(const aule_varlen_desc* d) {
    if (!d->cu_seqlens_q || !d->cu_seqlens_k) return "null cu_seqlens pointer";
    if (d->total_q > 0 && !d->q) return "null tensor pointer";
    if (d->total_k > 0 && (!d->k || !d->v)) return "null tensor pointer";
    if (misaligned(d->q) || misaligned(d->k) || misaligned(d->v)) return "q, k and v must be 16-byte aligned";
    return nullptr;
}

// (`size`: the kind's own sizeof -- the sink kinds are read through their twins' types)
static const char* varlen_desc_error(const aule_varlen_desc* d, Reason& why, size_t size = sizeof(aule_varlen_desc)) {
    if (const char* e = varlen_problem_error(d, size, why)) return e;
    if (varlen_fwd_nothing_to_do(d)) return nullptr;
    if (const char* e = varlen_input_error(d)) return e;
    if (!d->out) return "null tensor pointer";
    if (misaligned(d->out)) return "out must be 16-byte aligned";
    return nullptr;
}

static uint64_t varlen_bwd_workspace(const aule_varlen_desc* d) { return aule_hip::varlen_bwd_workspace_bytes(d->total_q, (int)d->heads_q); }

// (`more`: the bytes the kind's workspace holds beyond delta)
static const char* varlen_bwd_desc_error(const aule_varlen_bwd_desc* d, bool launch, Reason& why, size_t size = sizeof(aule_varlen_bwd_desc), uint64_t more = 0) {
    const aule_varlen_desc* x = varlen_prefix(d);
    if (const char* e = varlen_problem_error(x, size, why)) return e;
    if (!launch || varlen_bwd_nothing_to_do(x)) return nullptr;
    if (const char* e = varlen_input_error(x)) return e;
    if (d->total_q > 0 && (!d->out || !d->lse || !d->dout || !d->dq)) return "null tensor pointer";
    if (d->total_k > 0 && (!d->dk || !d->dv)) return "null tensor pointer";
    if (misaligned(d->out) || misaligned(d->dout) || misaligned(d->dq) || misaligned(d->dk) || misaligned(d->dv)) return "out, dout, dq, dk and dv must be 16-byte aligned";
    if (d->workspace != nullptr) {
        if (misaligned(d->workspace)) return "workspace must be 16-byte aligned";
        if (d->workspace_bytes < varlen_bwd_workspace(x) + more)
            return reasonf(why, "workspace too small (%llu bytes, need %llu)", (unsigned long long)d->workspace_bytes, (unsigned long long)(varlen_bwd_workspace(x) + more));
    }
    return nullptr;
}

// (`d` passed its kind's checker) the problem statement; the tensors behind the prefix are the entry's to set
static void fill_varlen_args(const aule_varlen_desc* d, aule_hip::VarlenArgs& a) {
    a.q = d->q; a.k = d->k; a.v = d->v;
    a.cu_seqlens_q = d->cu_seqlens_q; a.cu_seqlens_k = d->cu_seqlens_k;
    a.Tq = (int)d->total_q; a.Tk = (int)d->total_k; a.B = (int)d->batch; a.Hq = (int)d->heads_q; a.Hkv = (int)d->heads_kv; a.D = (int)d->head_dim;
    a.max_seqlen_q = aule_hip::seqlen_cut(d->max_seqlen_q, d->total_q);
    a.max_seqlen_k = aule_hip::seqlen_cut(d->max_seqlen_k, d->total_k);
    a.q_token_stride = d->q_token_stride; a.k_token_stride = d->k_token_stride; a.v_token_stride = d->v_token_stride;
    a.scale = resolve_scale(d->scale, d->head_dim);
    a.causal = d->causal;
    a.window = d->window_size;
    a.dtype = d->dtype;
}

// (`d` passed varlen_desc_error with its kind's size and has something to do; `sinks`: the sink kind's logits, checked by the caller)
static int32_t varlen_forward_launch(const aule_varlen_desc* d, const float* sinks, const char* what) {
    if (!initialised()) return -1;
    aule_hip::VarlenArgs a;
    fill_varlen_args(d, a);
    a.out = d->out; a.lse = d->lse; a.sinks = sinks;
    if (aule_hip::varlen_fwd_grid(a) > 0x7fffffffll) {
        set_error("%s failed: the grid (blocks * heads_kv * batch) exceeds 2^31 - 1 workgroups", what);
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched(what, aule_hip::launch_varlen_fwd(a, (hipStream_t)d->stream));
}

int32_t aule_attention_varlen_forward_ex(const aule_varlen_desc* d) {
    RoctxRange range("aule.varlen_forward");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = varlen_desc_error(d, text)) {
        set_error("Variable-length attention failed: %s", why);
        return -3;
    }
    if (varlen_fwd_nothing_to_do(d)) return 0;
    return varlen_forward_launch(d, nullptr, "Variable-length attention");
}

int32_t aule_attention_varlen_sink_forward_ex(const aule_varlen_sink_desc* d) {
    RoctxRange range("aule.varlen_sink_forward");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    const aule_varlen_desc* x = reinterpret_cast<const aule_varlen_desc*>(d);
    const char* why = varlen_desc_error(x, text, sizeof(aule_varlen_sink_desc));
    if (why == nullptr && !varlen_fwd_nothing_to_do(x) && d->sinks == nullptr) why = kNullSinks;
    if (why != nullptr) {
        set_error("Variable-length sink attention failed: %s", why);
        return -3;
    }
    if (varlen_fwd_nothing_to_do(x)) return 0;
    return varlen_forward_launch(x, d->sinks, "Variable-length sink attention");
}

// (`d` passed varlen_bwd_desc_error with its kind's size and has something to do; sinks / dsinks: the sink kind's, checked by the caller,
// the partials of its reduction behind delta in the workspace)
static int32_t varlen_backward_launch(const aule_varlen_bwd_desc* d, const float* sinks, float* dsinks, const char* what) {
    const aule_varlen_desc* x = varlen_prefix(d);
    if (!initialised()) return -1;
    aule_hip::VarlenArgs a;
    fill_varlen_args(x, a);
    a.o = d->out; a.lse = const_cast<float*>(d->lse); a.dout = d->dout;
    a.dq = d->dq; a.dk = d->dk; a.dv = d->dv; a.sinks = sinks;
    if (aule_hip::varlen_fwd_grid(a) > 0x7fffffffll || aule_hip::varlen_dkdv_grid(a) > 0x7fffffffll) {
        set_error("%s failed: a grid exceeds 2^31 - 1 workgroups", what);
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)d->stream;
    const uint64_t delta_bytes = varlen_bwd_workspace(x);
    const uint64_t need = delta_bytes + (sinks ? aule_hip::varlen_dsinks_partial_bytes(a) : 0);
    if (need == 0) {
        rc = aule_hip::launch_varlen_bwd(a, stream);
        if (rc == 0 && sinks) rc = aule_hip::launch_varlen_dsinks(a, dsinks, nullptr, stream);
        return launched(what, rc);
    }
    aule_hip::ScopedWorkspace ws(need, d->workspace, d->workspace ? d->workspace_bytes : 0, stream);
    if (ws.err != hipSuccess) {
        set_error("%s failed: workspace allocation (%llu bytes): %s", what, (unsigned long long)need, hipGetErrorString(ws.err));
        return -4;
    }
    a.delta = static_cast<float*>(ws.ptr);
    rc = aule_hip::launch_varlen_bwd(a, stream);
    if (rc == 0 && sinks) rc = aule_hip::launch_varlen_dsinks(a, dsinks, reinterpret_cast<float*>(static_cast<char*>(ws.ptr) + delta_bytes), stream);
    return launched(what, rc);
}

int32_t aule_attention_varlen_backward_ex(const aule_varlen_bwd_desc* d) {
    RoctxRange range("aule.varlen_backward");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = varlen_bwd_desc_error(d, true, text)) {
        set_error("Variable-length backward failed: %s", why);
        return -3;
    }
    if (varlen_bwd_nothing_to_do(varlen_prefix(d))) return 0;
    return varlen_backward_launch(d, nullptr, nullptr, "Variable-length backward");
}

uint64_t aule_attention_varlen_backward_workspace_size(const aule_varlen_bwd_desc* d) {
    Reason text;
    if (varlen_bwd_desc_error(d, false, text)) return 0;
    return varlen_bwd_nothing_to_do(varlen_prefix(d)) ? 0 : varlen_bwd_workspace(varlen_prefix(d));
}

// the partials of the dsinks reduction for the problem `x` states (`x` passed varlen_problem_error)
static uint64_t varlen_sink_partials(const aule_varlen_desc* x) {
    aule_hip::VarlenArgs a;
    fill_varlen_args(x, a);
    return aule_hip::varlen_dsinks_partial_bytes(a);
}

static const char* varlen_sink_bwd_desc_error(const aule_varlen_sink_bwd_desc* d, bool launch, Reason& why) {
    const aule_varlen_bwd_desc* y = reinterpret_cast<const aule_varlen_bwd_desc*>(d);
    if (const char* e = varlen_problem_error(varlen_prefix(y), sizeof(aule_varlen_sink_bwd_desc), why)) return e;
    if (const char* e = varlen_bwd_desc_error(y, launch, why, sizeof(aule_varlen_sink_bwd_desc), varlen_sink_partials(varlen_prefix(y)))) return e;
    if (!launch || varlen_bwd_nothing_to_do(varlen_prefix(y))) return nullptr;
    if (d->sinks == nullptr) return kNullSinks;
    if (d->dsinks == nullptr) return "null dsinks pointer (dsinks is a [heads_q] fp32 device array)";
    return nullptr;
}

int32_t aule_attention_varlen_sink_backward_ex(const aule_varlen_sink_bwd_desc* d) {
    RoctxRange range("aule.varlen_sink_backward");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = varlen_sink_bwd_desc_error(d, true, text)) {
        set_error("Variable-length sink backward failed: %s", why);
        return -3;
    }
    const aule_varlen_bwd_desc* y = reinterpret_cast<const aule_varlen_bwd_desc*>(d);
    if (varlen_bwd_nothing_to_do(varlen_prefix(y))) return 0;
    return varlen_backward_launch(y, d->sinks, d->dsinks, "Variable-length sink backward");
}

uint64_t aule_attention_varlen_sink_backward_workspace_size(const aule_varlen_sink_bwd_desc* d) {
    Reason text;
    if (varlen_sink_bwd_desc_error(d, false, text)) return 0;
    const aule_varlen_desc* x = varlen_prefix(reinterpret_cast<const aule_varlen_bwd_desc*>(d));
    return varlen_bwd_nothing_to_do(x) ? 0 : varlen_bwd_workspace(x) + varlen_sink_partials(x);
}

// The MLA prefill (the non-absorbed 192 / 128 form over a packed batch): one checker, one reader (the launch entry).  Host logic
// only, asked before the device is needed.  The stride rule: at least `least` elements and a multiple of 8.
static const char* mla_prefill_stride_error(const char* field, int64_t stride, uint64_t least, const char* what, Reason& why) {
    if (stride < 0 || (uint64_t)stride < least)
        return reasonf(why, "%s (%lld) is smaller than %s = %llu elements", field, (long long)stride, what, (unsigned long long)least);
    if (stride % 8 != 0) return reasonf(why, "%s (%lld) must be a multiple of 8 elements (16-byte loads)", field, (long long)stride);
    return nullptr;
}

static bool mla_prefill_nothing_to_do(const aule_mla_prefill_desc* d) { return d->total_q == 0 || (uint64_t)d->batch * d->heads == 0; }

// the problem statement, shared with the backward descriptor (`size`: the kind's own sizeof)
static const char* mla_prefill_problem_error(const aule_mla_prefill_desc* d, size_t size, Reason& why) {
    if (d == nullptr || d->struct_size != size) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return "dtype must be fp16 or bf16";
    if (d->qk_dim != 192 || d->v_dim != 128) return reasonf(why, "qk_dim %u / v_dim %u unsupported (192 / 128 only)", d->qk_dim, d->v_dim);
    if (d->causal < 0 || d->causal > AULE_CAUSAL_BOTTOM_RIGHT) return reasonf(why, "unknown causal mode %d (0 none, 1 top-left, 2 bottom-right)", d->causal);
    if (d->max_seqlen_q == 0) return "max_seqlen_q must be at least 1";
    if (d->max_seqlen_k == 0) return "max_seqlen_k must be at least 1";
    if (d->batch >= (1u << 30) || d->heads >= (1u << 30) || d->total_q >= (1u << 30) || d->total_k >= (1u << 30)) return "batch / heads / total_q / total_k too large";
    const uint64_t more = d->heads > 0 ? d->heads - 1 : 0;   // heads after the first
    if (const char* e = mla_prefill_stride_error("q_token_stride", d->q_token_stride, (uint64_t)d->heads * 192, "a token, heads * 192", why)) return e;
    if (const char* e = mla_prefill_stride_error("k_nope_head_stride", d->k_nope_head_stride, 128, "a head", why)) return e;
    if (const char* e = mla_prefill_stride_error("v_head_stride", d->v_head_stride, 128, "a head", why)) return e;
    if (d->k_nope_head_stride >= (1ll << 30) || d->v_head_stride >= (1ll << 30)) return "k_nope_head_stride / v_head_stride too large (below 2^30 elements)";
    if (const char* e = mla_prefill_stride_error("k_nope_token_stride", d->k_nope_token_stride, more * (uint64_t)d->k_nope_head_stride + 128,
                                                 "a token, (heads - 1) * k_nope_head_stride + 128", why)) return e;
    if (const char* e = mla_prefill_stride_error("v_token_stride", d->v_token_stride, more * (uint64_t)d->v_head_stride + 128,
                                                 "a token, (heads - 1) * v_head_stride + 128", why)) return e;
    if (const char* e = mla_prefill_stride_error("k_pe_token_stride", d->k_pe_token_stride, 64, "a token", why)) return e;
    return nullptr;
}

static const char* mla_prefill_desc_error(const aule_mla_prefill_desc* d, Reason& why) {
    if (const char* e = mla_prefill_problem_error(d, sizeof(aule_mla_prefill_desc), why)) return e;
    if (mla_prefill_nothing_to_do(d)) return nullptr;
    if (!d->cu_seqlens_q || !d->cu_seqlens_k) return "null cu_seqlens pointer";
    if (!d->q || !d->out) return "null tensor pointer";
    if (d->total_k > 0 && (!d->k_nope || !d->k_pe || !d->v)) return "null tensor pointer";
    if (misaligned(d->q) || misaligned(d->k_nope) || misaligned(d->k_pe) || misaligned(d->v)) return "q, k_nope, k_pe and v must be 16-byte aligned";
    if (misaligned(d->out)) return "out must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(d->lse) & 3) != 0) return "lse must be 4-byte aligned";
    return nullptr;
}

// (`d` passed its kind's checker) the problem statement; the tensors behind the prefix are the entry's to set
static void fill_mla_prefill_args(const aule_mla_prefill_desc* d, aule_hip::MlaPrefillArgs& a) {
    a.q = d->q; a.k_nope = d->k_nope; a.k_pe = d->k_pe; a.v = d->v;
    a.cu_seqlens_q = d->cu_seqlens_q; a.cu_seqlens_k = d->cu_seqlens_k;
    a.Tq = (int)d->total_q; a.Tk = (int)d->total_k; a.B = (int)d->batch; a.H = (int)d->heads;
    a.max_seqlen_q = aule_hip::seqlen_cut(d->max_seqlen_q, d->total_q);
    a.max_seqlen_k = aule_hip::seqlen_cut(d->max_seqlen_k, d->total_k);
    a.q_token_stride = d->q_token_stride;
    a.k_nope_token_stride = d->k_nope_token_stride; a.k_nope_head_stride = d->k_nope_head_stride;
    a.v_token_stride = d->v_token_stride; a.v_head_stride = d->v_head_stride;
    a.k_pe_token_stride = d->k_pe_token_stride;
    a.scale = resolve_scale(d->scale, d->qk_dim);
    a.causal = d->causal;
    a.dtype = d->dtype;
}

int32_t aule_attention_mla_prefill_ex(const aule_mla_prefill_desc* d) {
    RoctxRange range("aule.mla_prefill");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_prefill_desc_error(d, text)) {
        set_error("MLA prefill failed: %s", why);
        return -3;
    }
    if (mla_prefill_nothing_to_do(d)) return 0;
    aule_hip::MlaPrefillArgs a;
    fill_mla_prefill_args(d, a);
    a.out = d->out; a.lse = d->lse;
    if (aule_hip::mla_prefill_grid(a) > 0x7fffffffll) {
        set_error("MLA prefill failed: the grid (blocks * heads * batch) exceeds 2^31 - 1 workgroups (sizes beyond 32 bits)");
        return -3;
    }
    if (!initialised()) return -1;
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched("MLA prefill", aule_hip::launch_mla_prefill(a, (hipStream_t)d->stream));
}

// The MLA prefill backward: aule_mla_prefill_bwd_desc states the problem in aule_mla_prefill_desc's fields up to cu_seqlens_k (the
// layout asserts at the top of this file), so it is checked and read through that prefix.  `launch`: the pointer and workspace rules
// of a call that has something to do as well (the size query and the plan hook read no pointer).
static const aule_mla_prefill_desc* mla_prefill_prefix(const aule_mla_prefill_bwd_desc* d) { return reinterpret_cast<const aule_mla_prefill_desc*>(d); }

static bool mla_prefill_bwd_nothing_to_do(const aule_mla_prefill_bwd_desc* d) {
    return (uint64_t)d->batch * d->heads == 0 || (d->total_q == 0 && d->total_k == 0);
}

static aule_hip::MlaPrefillBwdPlan mla_prefill_bwd_plan_of(const aule_mla_prefill_bwd_desc* d) {
    return aule_hip::mla_prefill_bwd_plan((int)d->total_q, (int)d->total_k, (int)d->batch, (int)d->heads,
                                          aule_hip::seqlen_cut(d->max_seqlen_q, d->total_q), aule_hip::seqlen_cut(d->max_seqlen_k, d->total_k), d->device);
}

static const char* mla_prefill_bwd_desc_error(const aule_mla_prefill_bwd_desc* d, bool launch, Reason& why) {
    if (const char* e = mla_prefill_problem_error(mla_prefill_prefix(d), sizeof(aule_mla_prefill_bwd_desc), why)) return e;
    const uint64_t more = d->heads > 0 ? d->heads - 1 : 0;
    if (const char* e = mla_prefill_stride_error("dk_nope_head_stride", d->dk_nope_head_stride, 128, "a head", why)) return e;
    if (const char* e = mla_prefill_stride_error("dv_head_stride", d->dv_head_stride, 128, "a head", why)) return e;
    if (d->dk_nope_head_stride >= (1ll << 30) || d->dv_head_stride >= (1ll << 30)) return "dk_nope_head_stride / dv_head_stride too large (below 2^30 elements)";
    if (const char* e = mla_prefill_stride_error("dk_nope_token_stride", d->dk_nope_token_stride, more * (uint64_t)d->dk_nope_head_stride + 128,
                                                 "a token, (heads - 1) * dk_nope_head_stride + 128", why)) return e;
    if (const char* e = mla_prefill_stride_error("dv_token_stride", d->dv_token_stride, more * (uint64_t)d->dv_head_stride + 128,
                                                 "a token, (heads - 1) * dv_head_stride + 128", why)) return e;
    if (mla_prefill_bwd_nothing_to_do(d)) return nullptr;
    if (!mla_prefill_bwd_plan_of(d).ok) return "a grid exceeds 2^31 - 1 workgroups (sizes beyond 32 bits)";
    if (!launch) return nullptr;
    if (!d->cu_seqlens_q || !d->cu_seqlens_k) return "null cu_seqlens pointer";
    if (d->total_q > 0 && (!d->q || !d->out || !d->lse || !d->dout || !d->dq)) return "null tensor pointer";
    if (d->total_k > 0 && (!d->k_nope || !d->k_pe || !d->v || !d->dk_nope || !d->dk_pe || !d->dv)) return "null tensor pointer";
    if (misaligned(d->q) || misaligned(d->k_nope) || misaligned(d->k_pe) || misaligned(d->v)) return "q, k_nope, k_pe and v must be 16-byte aligned";
    if (misaligned(d->out) || misaligned(d->dout) || misaligned(d->dq) || misaligned(d->dk_nope) || misaligned(d->dk_pe) || misaligned(d->dv))
        return "out, dout, dq, dk_nope, dk_pe and dv must be 16-byte aligned";
    if ((reinterpret_cast<uintptr_t>(d->lse) & 3) != 0) return "lse must be 4-byte aligned";
    if (d->workspace != nullptr) {
        if (misaligned(d->workspace)) return "workspace must be 16-byte aligned";
        const uint64_t need = mla_prefill_bwd_plan_of(d).ws_bytes;
        if (d->workspace_bytes < need)
            return reasonf(why, "workspace too small (%llu bytes, need %llu)", (unsigned long long)d->workspace_bytes, (unsigned long long)need);
    }
    return nullptr;
}

int32_t aule_attention_mla_prefill_backward_ex(const aule_mla_prefill_bwd_desc* d) {
    RoctxRange range("aule.mla_prefill_backward");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_prefill_bwd_desc_error(d, true, text)) {
        set_error("MLA prefill backward failed: %s", why);
        return -3;
    }
    if (mla_prefill_bwd_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaPrefillBwdArgs a;
    fill_mla_prefill_args(mla_prefill_prefix(d), a.fwd);
    a.o = d->out; a.lse = d->lse; a.dout = d->dout;
    a.dq = d->dq; a.dk_nope = d->dk_nope; a.dk_pe = d->dk_pe; a.dv = d->dv;
    a.dk_nope_token_stride = d->dk_nope_token_stride; a.dk_nope_head_stride = d->dk_nope_head_stride;
    a.dv_token_stride = d->dv_token_stride; a.dv_head_stride = d->dv_head_stride;
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)d->stream;
    const aule_hip::MlaPrefillBwdPlan plan = mla_prefill_bwd_plan_of(d);
    if (d->workspace != nullptr && d->workspace_bytes < plan.ws_bytes) {   // (the plan asks the device now selected: the same one, stated again)
        set_error("MLA prefill backward failed: workspace too small (%llu bytes, need %llu)", (unsigned long long)d->workspace_bytes, (unsigned long long)plan.ws_bytes);
        return -3;
    }
    if (plan.ws_bytes == 0) return launched("MLA prefill backward", aule_hip::launch_mla_prefill_bwd(a, plan, nullptr, stream));
    aule_hip::ScopedWorkspace ws(plan.ws_bytes, d->workspace, d->workspace ? d->workspace_bytes : 0, stream);
    if (ws.err != hipSuccess) {
        set_error("MLA prefill backward failed: workspace allocation (%llu bytes): %s", (unsigned long long)plan.ws_bytes, hipGetErrorString(ws.err));
        return -4;
    }
    return launched("MLA prefill backward", aule_hip::launch_mla_prefill_bwd(a, plan, ws.ptr, stream));
}

uint64_t aule_attention_mla_prefill_backward_workspace_size(const aule_mla_prefill_bwd_desc* d) {
    Reason text;
    if (mla_prefill_bwd_desc_error(d, false, text)) return 0;
    return mla_prefill_bwd_nothing_to_do(d) ? 0 : mla_prefill_bwd_plan_of(d).ws_bytes;
}

// The two-state merge.  One checker, one reader (the launch entry: the pointer rules are stated here too).
static bool merge_states_nothing_to_do(const aule_merge_states_desc* d) { return (uint64_t)d->rows * d->heads == 0; }

static const char* merge_states_desc_error(const aule_merge_states_desc* d, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_merge_states_desc)) return kBadDescriptor;
    if (d->dtype != AULE_DTYPE_F16 && d->dtype != AULE_DTYPE_BF16) return "dtype must be fp16 or bf16";
    if (d->head_dim == 0 || d->head_dim % 8 != 0 || d->head_dim > 1024) return reasonf(why, "head_dim %u unsupported (a multiple of 8, at most 1024)", d->head_dim);
    if ((uint64_t)d->rows * d->heads >= (1ull << 31)) return "rows * heads too large";
    if (merge_states_nothing_to_do(d)) return nullptr;
    if (!d->out_a || !d->lse_a || !d->out_b || !d->lse_b || !d->out || !d->lse) return "null tensor pointer";
    if (misaligned(d->out_a) || misaligned(d->out_b) || misaligned(d->out)) return "out_a, out_b and out must be 16-byte aligned";
    // every thread of a row reads lse_a and lse_b, one of them writes lse: an lse inside either input would be read after it was written
    const uint64_t lse_bytes = (uint64_t)d->rows * d->heads * 4;
    const auto overlaps = [lse_bytes](const float* x, const float* y) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(x), b = reinterpret_cast<uintptr_t>(y);
        return a < b + lse_bytes && b < a + lse_bytes;
    };
    if (overlaps(d->lse, d->lse_a) || overlaps(d->lse, d->lse_b)) return "lse must not overlap lse_a or lse_b (only out may alias an input)";
    return nullptr;
}

int32_t aule_attention_merge_states_ex(const aule_merge_states_desc* d) {
    RoctxRange range("aule.merge_states");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = merge_states_desc_error(d, text)) {
        set_error("Merge of attention states failed: %s", why);
        return -3;
    }
    if (merge_states_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MergeStatesArgs a;
    a.out_a = d->out_a; a.lse_a = d->lse_a; a.out_b = d->out_b; a.lse_b = d->lse_b; a.out = d->out; a.lse = d->lse;
    a.rows = (long long)d->rows * d->heads; a.D = (int)d->head_dim; a.dtype = d->dtype;
    DeviceGuard g(d->device);
    return launched("Merge of attention states", aule_hip::launch_merge_states(a, (hipStream_t)d->stream));
}

static const char* rope_desc_error(const aule_rope_desc* d, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_rope_desc)) return kBadDescriptor;
    if (d->dtype < 0 || d->dtype > 2) return reasonf(why, "unknown dtype %d", d->dtype);
    if (d->head_dim == 0 || (d->head_dim & 1) || d->row_pitch < d->head_dim)
        return reasonf(why, "head_dim (%u) must be even and <= row_pitch (%u)", d->head_dim, d->row_pitch);
    if (d->layout != AULE_ROPE_HALF && d->layout != AULE_ROPE_INTERLEAVED) return reasonf(why, "unknown layout %d", d->layout);
    if ((uint64_t)d->seq + d->pos_offset > d->table_len)
        return reasonf(why, "table too short (%u rows < seq %u + pos_offset %u)", d->table_len, d->seq, d->pos_offset);
    if (d->table_pitch != 0 && d->table_pitch < d->head_dim / 2) return reasonf(why, "table_pitch (%u) < head_dim/2", d->table_pitch);
    return nullptr;
}

static bool rope_nothing_to_do(const aule_rope_desc* d) { return d->rows_bh == 0 || d->seq == 0; }

int32_t aule_rope_ex(const aule_rope_desc* d) {
    RoctxRange range("aule.rope");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    Reason text;
    if (const char* why = rope_desc_error(d, text)) {
        set_error("RoPE failed: %s", why);
        return -3;
    }
    if (rope_nothing_to_do(d)) return 0;
    if (d->rows_bh * d->seq >= (1ull << 40) || d->seq >= (1u << 30)) {
        set_error("RoPE failed: problem too large");
        return -3;
    }
    if (!d->in || !d->out || !d->cos || !d->sin) {
        set_error("RoPE failed: null pointer");
        return -3;
    }
    DeviceGuard g(d->device);
    aule_hip::RopeArgs r;
    r.in = d->in; r.out = d->out; r.cos = d->cos; r.sin = d->sin;
    r.nheads = (long long)d->rows_bh; r.S = (int)d->seq; r.D = (int)d->head_dim; r.pitch = (int)d->row_pitch;
    r.layout = d->layout; r.inverse = d->inverse != 0; r.pos_offset = (int)d->pos_offset; r.dtype = d->dtype;
    r.table_pitch = (int)d->table_pitch;
    return launched("RoPE", aule_hip::launch_rope(r, (hipStream_t)d->stream));
}

static bool kv_append_nothing_to_do(const aule_kv_append_desc* d) { return d->num_tokens == 0; }

// 0 fine, else the reason the descriptor is refused (host logic only: no pointer is dereferenced; its only reader is the launch
// entry, so the pointer rules of a call that has something to do are stated here too)
static const char* kv_append_error(const aule_kv_append_desc* d) {
    if (d == nullptr || d->struct_size != sizeof(aule_kv_append_desc)) return kBadDescriptor;
    if (d->dtype != AULE_DTYPE_F16 && d->dtype != AULE_DTYPE_BF16) return "dtype (of key / value) must be fp16 or bf16";
    if (const char* e = cache_dtype_error(d->cache_dtype)) return e;
    if (d->head_dim != 32 && d->head_dim != 64 && d->head_dim != 128) return "head_dim unsupported (32, 64 or 128)";
    if (d->heads_kv == 0 || d->block_size == 0) return "heads_kv and block_size must be positive";
    const int64_t D = (int64_t)d->head_dim;
    const int64_t strides[4] = {d->key_token_stride, d->key_head_stride, d->value_token_stride, d->value_head_stride};
    for (int64_t st : strides) {
        if (st < D) return "a token / head stride is smaller than a row (head_dim elements)";
        if (st % 8 != 0) return "token / head strides must be multiples of 8 elements (16-byte loads)";
    }
    const bool any_rope = d->cos || d->sin || d->positions || d->table_len || d->table_pitch;
    const bool all_rope = d->cos && d->sin && d->positions && d->table_len;
    if (any_rope && !all_rope) return "RoPE group only partly given (cos, sin, positions and table_len go together)";
    if (all_rope) {
        if (d->head_dim & 1) return "head_dim must be even for RoPE";
        if (d->table_pitch != 0 && (d->table_pitch < d->head_dim / 2 || d->table_pitch % 4 != 0))
            return "table_pitch must be 0 or a multiple of 4 that is >= head_dim/2";
    }
    if (kv_append_nothing_to_do(d)) return nullptr;
    if (!d->key || !d->value || !d->k_cache || !d->v_cache || !d->slot_mapping) return "null tensor pointer";
    if (const char* e = scale_pointer_error(d->cache_dtype == AULE_KV_CACHE_FP8_E4M3, d->k_scale, d->v_scale)) return e;
    if (misaligned(d->key) || misaligned(d->value) || misaligned(d->k_cache) || misaligned(d->v_cache) || misaligned(d->cos) || misaligned(d->sin))
        return "key, value, the caches and the tables must be 16-byte aligned";
    return nullptr;
}

int32_t aule_kv_cache_append_ex(const aule_kv_append_desc* d) {
    RoctxRange range("aule.kv_cache_append");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    if (const char* why = kv_append_error(d)) {
        set_error("KV cache append failed: %s", why);
        return -3;
    }
    if (kv_append_nothing_to_do(d)) return 0;
    aule_hip::KvAppendArgs a;
    a.key = d->key; a.value = d->value; a.k_cache = d->k_cache; a.v_cache = d->v_cache;
    a.slot_mapping = reinterpret_cast<const long long*>(d->slot_mapping);
    a.T = (int)d->num_tokens; a.Hkv = (int)d->heads_kv; a.D = (int)d->head_dim;
    a.num_blocks = (long long)d->num_blocks; a.block_size = (int)d->block_size;
    a.k_token_stride = d->key_token_stride; a.k_head_stride = d->key_head_stride;
    a.v_token_stride = d->value_token_stride; a.v_head_stride = d->value_head_stride;
    a.dtype = d->dtype;
    if (d->cache_dtype == AULE_KV_CACHE_FP8_E4M3) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.k_scale = d->k_scale; a.v_scale = d->v_scale;
    }
    a.cos = d->cos; a.sin = d->sin; a.positions = reinterpret_cast<const long long*>(d->positions);
    a.table_len = (long long)d->table_len; a.table_pitch = (int)d->table_pitch;
    DeviceGuard g(d->device);
    return launched("KV cache append", aule_hip::launch_kv_append(a, (hipStream_t)d->stream));
}

static bool mla_kv_append_nothing_to_do(const aule_mla_kv_append_desc* d) { return d->total_tokens == 0; }

// 0 fine, else the reason the descriptor is refused (host logic only: no pointer is dereferenced; its only reader is the launch
// entry, so the pointer rules of a call that has something to do are stated here too)
static const char* mla_kv_append_error(const aule_mla_kv_append_desc* d, Reason& why) {
    if (d == nullptr || d->struct_size != sizeof(aule_mla_kv_append_desc)) return kBadDescriptor;
    if (!is_16_bit(d->dtype)) return "dtype (of c_kv / k_pe) must be fp16 or bf16";
    if (const char* e = cache_dtype_error(d->cache_dtype)) return e;
    if (d->rope_layout != AULE_ROPE_HALF && d->rope_layout != AULE_ROPE_INTERLEAVED)
        return reasonf(why, "unknown rope_layout %d (AULE_ROPE_HALF or AULE_ROPE_INTERLEAVED)", d->rope_layout);
    if (d->block_size == 0) return "block_size must be positive";
    if (d->c_kv_token_stride < 512) return reasonf(why, "c_kv_token_stride (%lld) is smaller than a row (512 elements)", (long long)d->c_kv_token_stride);
    if (d->k_pe_token_stride < 64) return reasonf(why, "k_pe_token_stride (%lld) is smaller than a row (64 elements)", (long long)d->k_pe_token_stride);
    if (d->c_kv_token_stride % 8 != 0 || d->k_pe_token_stride % 8 != 0) return "token strides must be multiples of 8 elements (16-byte loads)";
    const bool any_rope = d->cos || d->sin || d->positions || d->table_len || d->table_pitch;
    const bool all_rope = d->cos && d->sin && d->positions && d->table_len;
    if (any_rope && !all_rope) return "RoPE group only partly given (cos, sin, positions and table_len go together)";
    if (all_rope && d->table_pitch != 0 && (d->table_pitch < 32 || d->table_pitch % 4 != 0)) return "table_pitch must be 0 or a multiple of 4 that is >= 32";
    if (mla_kv_append_nothing_to_do(d)) return nullptr;
    if (!d->c_kv || !d->k_pe || !d->kv_cache || !d->slot_mapping) return "null tensor pointer";
    const bool fp8 = d->cache_dtype == AULE_KV_CACHE_FP8_E4M3;
    if (fp8 && !d->kv_scale) return "null kv_scale (one fp32 value on the device)";
    if (!fp8 && d->kv_scale) return "kv_scale applies to an FP8 cache only; a 16-bit cache holds the values themselves";
    if ((reinterpret_cast<uintptr_t>(d->kv_scale) & 3) != 0) return "kv_scale must be 4-byte aligned";
    if (misaligned(d->c_kv) || misaligned(d->k_pe) || misaligned(d->kv_cache) || misaligned(d->cos) || misaligned(d->sin))
        return "c_kv, k_pe, kv_cache and the tables must be 16-byte aligned";
    return nullptr;
}

int32_t aule_mla_kv_append_ex(const aule_mla_kv_append_desc* d) {
    RoctxRange range("aule.mla_kv_append");
    std::lock_guard<std::mutex> lk(g_mu);
    Reason text;
    if (const char* why = mla_kv_append_error(d, text)) {
        set_error("MLA KV append failed: %s", why);
        return -3;
    }
    if (mla_kv_append_nothing_to_do(d)) return 0;
    if (!initialised()) return -1;
    aule_hip::MlaKvAppendArgs a;
    a.c_kv = d->c_kv; a.k_pe = d->k_pe; a.kv_cache = d->kv_cache;
    a.slot_mapping = reinterpret_cast<const long long*>(d->slot_mapping);
    a.T = (int)d->total_tokens;
    a.num_blocks = (long long)d->num_blocks; a.block_size = (int)d->block_size;
    a.c_kv_token_stride = d->c_kv_token_stride; a.k_pe_token_stride = d->k_pe_token_stride;
    a.dtype = d->dtype;
    if (d->cache_dtype == AULE_KV_CACHE_FP8_E4M3) {
        a.cache_kind = aule_hip::kCacheFp8E4M3;
        a.kv_scale = d->kv_scale;
    }
    a.cos = d->cos; a.sin = d->sin; a.positions = reinterpret_cast<const long long*>(d->positions);
    a.table_len = (long long)d->table_len; a.table_pitch = (int)d->table_pitch;
    a.rope_layout = d->rope_layout;
    DeviceGuard g(d->device);
    return launched("MLA KV append", aule_hip::launch_mla_kv_append(a, (hipStream_t)d->stream));
}

uint64_t aule_attention_backward_workspace_size(const aule_attn_bwd_desc* d) {
    Reason text;
    if (attn_desc_error(attn_prefix(d), sizeof(aule_attn_bwd_desc), text)) return 0;
    BwdArgs a;
    fill_bwd_args(d, a, false);
    return aule_hip::bwd_plan(a).want_bytes;
}

int32_t aule_attention_backward_ex(const aule_attn_bwd_desc* d) {
    RoctxRange range("aule.backward");
    std::lock_guard<std::mutex> lk(g_mu);
    if (!initialised()) return -1;
    const aule_attn_desc* p = attn_prefix(d);
    Reason text;
    const char* why = attn_desc_error(p, sizeof(aule_attn_bwd_desc), text);
    if (why == nullptr && attn_too_large(p)) why = "problem too large";
    if (why != nullptr) {   // (the shared rules say "Attention failed" in both directions; only the struct_size text names this one)
        set_error("%s failed: %s", why == kBadDescriptor ? "Backward" : "Attention", why);
        return -3;
    }
    if (bwd_nothing_to_do(p)) return 0;
    if (d->seq_k == 0 || d->seq_q == 0) {
        set_error("Backward failed: empty sequence");
        return -3;
    }
    if (!d->q || !d->k || !d->v || !d->out || !d->dout || !d->lse || !d->dq || !d->dk || !d->dv) {
        set_error("Backward failed: null tensor pointer");
        return -3;
    }
    // (aule_attention_backward_workspace_size() also asks for the dS workspace of the 5-matmul backward; a smaller buffer that
    // still holds delta / L' / the partials is accepted and runs the recompute pair)
    BwdArgs a;
    fill_bwd_args(d, a, true);
    const uint64_t need = a.ws_floor;
    if (!d->workspace || d->workspace_bytes < need) {
        set_error("Backward failed: workspace too small (%llu < %llu bytes)",
                  (unsigned long long)d->workspace_bytes, (unsigned long long)need);
        return -3;
    }
    DeviceGuard g(d->device);
    int rc = ensure_configured();
    if (rc) return rc;
    return launched("Backward", aule_hip::launch_bwd(a, (hipStream_t)d->stream));
}

// ---- direct peer exchange (include/aule.h; consumer: aule/dist.py, transport="peer")
static_assert(sizeof(aule_ipc_handle) == sizeof(hipIpcMemHandle_t), "aule_ipc_handle must carry a hipIpcMemHandle_t");

int32_t aule_peer_alloc(int32_t device, uint64_t bytes, void** ptr, aule_ipc_handle* handle) {
    if (ptr == nullptr || handle == nullptr || bytes == 0) { set_error("aule_peer_alloc: bad argument"); return -1; }
    DeviceGuard g(device);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) { set_error("aule_peer_alloc: hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e)); return -2; }
    hipIpcMemHandle_t h;
    e = hipIpcGetMemHandle(&h, p);
    if (e != hipSuccess) {
        set_error("aule_peer_alloc: hipIpcGetMemHandle: %s (HSA_ENABLE_IPC_MODE_LEGACY=0 set?)", hipGetErrorString(e));
        (void)hipFree(p);
        return -4;
    }
    std::memcpy(handle->bytes, &h, sizeof(h));
    *ptr = p;
    return 0;
}

int32_t aule_peer_free(int32_t device, void* ptr) {
    if (ptr == nullptr) return 0;
    DeviceGuard g(device);
    const hipError_t e = hipFree(ptr);
    if (e != hipSuccess) { set_error("aule_peer_free: %s", hipGetErrorString(e)); return -4; }
    return 0;
}

int32_t aule_peer_open(int32_t device, const aule_ipc_handle* handle, void** ptr) {
    if (ptr == nullptr || handle == nullptr) { set_error("aule_peer_open: bad argument"); return -1; }
    DeviceGuard g(device);
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle->bytes, sizeof(h));
    void* p = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { set_error("aule_peer_open: hipIpcOpenMemHandle: %s", hipGetErrorString(e)); return -4; }
    *ptr = p;
    return 0;
}

int32_t aule_peer_close(int32_t device, void* ptr) {
    if (ptr == nullptr) return 0;
    DeviceGuard g(device);
    const hipError_t e = hipIpcCloseMemHandle(ptr);
    if (e != hipSuccess) { set_error("aule_peer_close: %s", hipGetErrorString(e)); return -4; }
    return 0;
}

int32_t aule_peer_copy_async(int32_t device, void* dst, const void* src, uint64_t bytes, void* stream) {
    if (bytes == 0) return 0;
    if (dst == nullptr || src == nullptr) { set_error("aule_peer_copy_async: bad argument"); return -1; }
    DeviceGuard g(device);
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { set_error("aule_peer_copy_async: %s", hipGetErrorString(e)); return -4; }
    return 0;
}

const char* aule_hip_build_info(void) { return "aule-hip gfx950 abi2"; }   // abi2: workspace fields in the fwd / paged descriptors

uint64_t aule_attention_forward_workspace_size(const aule_attn_desc* d) {
    Reason text;
    if (attn_desc_error(d, sizeof(aule_attn_desc), text) || fwd_nothing_to_do(d) || d->seq_k == 0) return 0;
    FwdArgs a;
    fill_fwd_args(d, a);
    return aule_hip::fwd_workspace_bytes(a);
}

// (the launcher's plan: it reads the shape, none of the pointers)
static uint64_t paged_workspace_impl(const aule_paged_desc* d, bool fp8) {
    Reason text;
    if (paged_desc_error(d, fp8, false, text) || paged_nothing_to_do(d)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_args(d, fp8, a);
    return aule_hip::paged_workspace_bytes(a);
}

uint64_t aule_attention_paged_decode_workspace_size(const aule_paged_desc* d) { return paged_workspace_impl(d, false); }

uint64_t aule_attention_paged_decode_fp8_workspace_size(const aule_paged_fp8_desc* d) {
    return paged_workspace_impl(paged_prefix(d), true);
}

// (the same plan as the launch: paged_workspace_bytes reads PagedArgs::Sq)
uint64_t aule_attention_paged_query_workspace_size(const aule_paged_query_desc* d) {
    Reason text;
    if (paged_query_desc_error(d, false, text) || paged_query_nothing_to_do(d)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_query_args(d, a);
    return aule_hip::paged_workspace_bytes(a);
}

// (the sink is merged by the combine pass: the sinkless plan's bytes)
uint64_t aule_attention_paged_query_sink_workspace_size(const aule_paged_query_sink_desc* d) {
    Reason text;
    const aule_paged_query_desc* x = query_prefix(d);
    if (paged_query_desc_error(x, false, text, sizeof(aule_paged_query_sink_desc)) || paged_query_nothing_to_do(x)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_query_args(x, a);
    return aule_hip::paged_workspace_bytes(a);
}

// (the tree kernel writes the twin's partials: the twin's plan and bytes; a window is refused as by the launch)
uint64_t aule_attention_paged_query_tree_workspace_size(const aule_paged_query_tree_desc* d) {
    Reason text;
    const aule_paged_query_desc* x = query_tree_prefix(d);
    if (paged_query_desc_error(x, false, text, sizeof(aule_paged_query_tree_desc)) || x->window_size > 0 || paged_query_nothing_to_do(x)) return 0;
    aule_hip::PagedArgs a;
    fill_paged_query_args(x, a);
    return aule_hip::paged_workspace_bytes(a);
}

// (the launch's plan: shared_prefix_plan reads the shape, none of the pointers)
static bool cascade_plan(const aule_paged_cascade_desc* d, aule_hip::SharedPrefixPlan& plan) {
    Reason text;
    if (paged_cascade_desc_error(d, false, text)) return false;
    plan = aule_hip::SharedPrefixPlan();
    if (ragged_nothing_to_do(d)) return true;
    aule_hip::SharedPrefixArgs x;
    aule_hip::PagedPrefillArgs a;
    fill_paged_cascade_args(d, x, a);
    plan = aule_hip::shared_prefix_plan(x);
    return true;
}

uint64_t aule_attention_paged_cascade_workspace_size(const aule_paged_cascade_desc* d) {
    aule_hip::SharedPrefixPlan plan;
    return cascade_plan(d, plan) ? plan.ws_bytes : 0;
}

// (the launch's plan: mla_plan reads the shape, none of the pointers)
static bool mla_paged_plan(const aule_mla_paged_desc* d, MlaKind kind, aule_hip::MlaPlan& plan) {
    Reason text;
    if (mla_paged_desc_error(d, kind, false, text)) return false;
    plan = aule_hip::MlaPlan();
    if (ragged_nothing_to_do(d)) return true;
    aule_hip::MlaArgs a;
    fill_mla_paged_args(d, kMla16, a);   // (the plan reads the shape: no pointer, not the cache kind, not the words)
    plan = aule_hip::mla_plan(a);
    return plan.grid <= 0x7fffffffll;
}

uint64_t aule_attention_mla_paged_workspace_size(const aule_mla_paged_desc* d) {
    aule_hip::MlaPlan plan;
    return mla_paged_plan(d, kMla16, plan) ? plan.ws_bytes : 0;
}

uint64_t aule_attention_mla_paged_fp8_workspace_size(const aule_mla_paged_fp8_desc* d) {
    aule_hip::MlaPlan plan;
    return mla_paged_plan(mla_prefix(d), kMlaFp8, plan) ? plan.ws_bytes : 0;
}

uint64_t aule_attention_mla_paged_tree_workspace_size(const aule_mla_paged_tree_desc* d) {
    aule_hip::MlaPlan plan;
    return mla_paged_plan(mla_tree_prefix(d), kMlaTree, plan) ? plan.ws_bytes : 0;
}

uint64_t aule_attention_mla_sparse_workspace_size(const aule_mla_sparse_desc* d) {
    Reason text;
    if (mla_sparse_desc_error(d, false, text)) return 0;
    return mla_sparse_nothing_to_do(d) ? 0 : mla_sparse_plan_of(d).ws_bytes;
}

#ifdef AULE_DEBUG_HOOKS
/* The timeline hooks exist only in the debug library (`make dbg` -> build/variants/libaule_dbg.so, -DAULE_DEBUG_HOOKS):
 * they launch instrumented kernel instances on caller-supplied pointers and are not part of the product libaule.so. */
/* Debug hook (not part of the drop-in ABI): aule_attention_backward_ex with the dK/dV kernel's timeline build --
 * per-phase s_memtime stamps of its workgroup 0 into `stamps` (device pointer, 8 * 384 uint64; bf16 D128 causal only,
 * otherwise the ordinary kernels run and nothing is written).  Used by tools/timeline_bwd.py. */
static int32_t backward_timeline(const aule_attn_bwd_desc* d, unsigned long long* stamps, bool dq) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init || stamps == nullptr) return -1;
    Reason text;
    if (const char* why = attn_desc_error(attn_prefix(d), sizeof(aule_attn_bwd_desc), text)) return why == kBadDescriptor ? -1 : -3;
    if (d->dtype != AULE_DTYPE_BF16 || (d->head_dim != 128 && !(d->head_dim == 64 && !dq))) return -3;   // the instrumented instances (D = 64: the dK/dV timeline only)
    BwdArgs a;
    fill_bwd_args(d, a, true);
    if (dq) a.dbg_dq = stamps; else a.dbg = stamps;
    return aule_hip::launch_bwd(a, (hipStream_t)d->stream);
}
int32_t aule_hip_debug_backward_timeline(const aule_attn_bwd_desc* d, unsigned long long* stamps) {
    return backward_timeline(d, stamps, false);
}
/* ... the same for the dQ kernel (8 stamps per tile). */
int32_t aule_hip_debug_backward_timeline_dq(const aule_attn_bwd_desc* d, unsigned long long* stamps) {
    return backward_timeline(d, stamps, true);
}
#endif  // AULE_DEBUG_HOOKS

/* Debug hook (not part of the drop-in ABI): the forward kernel aule_attention_forward_ex would launch for `d`
 * -- the codes of fwd_route() (fa_kernels.h; include/aule.h lists them); -3 for a bad descriptor.  Pure host logic: no
 * device, no aule_init() needed.  Used by the tests to pin which kernel a shape exercises. */
static bool plan_hook_args(const aule_attn_desc* d, FwdArgs& a) {   // (the three forward plan hooks)
    Reason text;
    if (attn_desc_error(d, sizeof(aule_attn_desc), text, /*plan_hook=*/true)) return false;
    fill_fwd_args(d, a);   // (the sign of the scale picks the kernel: negative scales stay off route 8)
    return true;
}

int32_t aule_hip_debug_forward_route(const aule_attn_desc* d) {
    FwdArgs a;
    return plan_hook_args(d, a) ? aule_hip::fwd_route(a) : -3;
}

/* Debug hook: the route of the most recent forward launch of this process (0 before the first): what ran, where
 * aule_hip_debug_forward_route says what would. */
int32_t aule_hip_debug_last_forward_route(void) { return aule_hip::fwd_last_route(); }

/* Debug hook: the whole launch plan of aule_attention_forward_ex(d) as integers (include/aule.h lists them); the contract of
 * aule_hip_debug_forward_split_plan.  Pure host logic like the route hook. */
int32_t aule_hip_debug_forward_plan(const aule_attn_desc* d, int32_t* out, int32_t cap) {
    FwdArgs a;
    return plan_hook_args(d, a) ? aule_hip::fwd_plan_dump(a, out, cap) : -3;
}

/* What the plan hooks below answer: the integers of `v`, then the low and the high word of *ws_bytes where the plan has a workspace; their
 * count, or minus their count when `out` cannot hold them. */
static int32_t dump_plan(std::initializer_list<int32_t> v, const uint64_t* ws_bytes, int32_t* out, int32_t cap) {
    const int32_t n = (int32_t)v.size() + (ws_bytes != nullptr ? 2 : 0);
    if (out == nullptr || cap < n) return -n;
    out = std::copy(v.begin(), v.end(), out);
    if (ws_bytes != nullptr) {
        out[0] = (int32_t)(uint32_t)(*ws_bytes & 0xffffffffull);
        out[1] = (int32_t)(uint32_t)(*ws_bytes >> 32);
    }
    return n;
}

/* Debug hook: the launch plan of the paged cascade's shared-prefix kernel as integers (include/aule.h lists them): the plan the launch
 * and the workspace query read.  Pure host logic like the forward hook. */
int32_t aule_hip_debug_shared_prefix_plan(const aule_paged_cascade_desc* d, int32_t* out, int32_t cap) {
    aule_hip::SharedPrefixPlan plan;
    if (!cascade_plan(d, plan)) return -3;
    if (plan.grid <= 0) return 0;
    return dump_plan({plan.row_blocks, plan.tiles, plan.nsplit, plan.tiles_per_split, (int32_t)(plan.grid > 0x7fffffffll ? 0x7fffffff : plan.grid)}, &plan.ws_bytes, out, cap);
}

/* Debug hook: the launch plan of aule_attention_mla_paged_ex(d) as integers (include/aule.h lists them): the plan the launch and the
 * workspace query read.  Pure host logic like the forward hook. */
int32_t aule_hip_debug_mla_plan(const aule_mla_paged_desc* d, int32_t* out, int32_t cap) {
    aule_hip::MlaPlan plan;
    if (!mla_paged_plan(d, kMla16, plan)) return -3;
    if (plan.grid <= 0) return 0;
    return dump_plan({plan.row_blocks, plan.rows_per_block, plan.nsplit, (int32_t)plan.grid}, &plan.ws_bytes, out, cap);
}

/* Debug hook: the launch plan of aule_attention_mla_sparse_ex(d) as integers (include/aule.h lists them): the plan the launch and the
 * workspace query read.  Pure host logic like the forward hook. */
int32_t aule_hip_debug_mla_sparse_plan(const aule_mla_sparse_desc* d, int32_t* out, int32_t cap) {
    Reason text;
    if (mla_sparse_desc_error(d, false, text)) return -3;
    if (mla_sparse_nothing_to_do(d)) return 0;
    const aule_hip::MlaPlan plan = mla_sparse_plan_of(d);
    return dump_plan({plan.row_blocks, plan.rows_per_block, plan.nsplit, (int32_t)plan.grid}, &plan.ws_bytes, out, cap);
}

/* Debug hook (not part of the drop-in ABI): aule_attention_mla_sparse_ex(d) with `nsplit` key ranges (within 1 .. min(64, tiles)) instead
 * of the plan's -- what tools/bench_mla_sparse.py measures the plan's "one split per two tiles" cap with.  Every rule of the entry
 * holds; a caller workspace is sized for THIS nsplit (round16(nsplit * total_tokens * heads_q * 514 * 4)).  nsplit < 1: -3. */
int32_t aule_hip_debug_mla_sparse_launch_nsplit(const aule_mla_sparse_desc* d, int32_t nsplit) {
    if (nsplit < 1) {
        set_error("Sparse MLA attention failed: nsplit (%d) must be at least 1", nsplit);
        return -3;
    }
    return mla_sparse_launch(d, nsplit);
}

/* Debug hook: the launch plan of aule_mla_indexer_logits_ex(d) as integers (include/aule.h lists them): the plan the launch reads.
 * Pure host logic like the forward hook. */
int32_t aule_hip_debug_mla_indexer_plan(const aule_mla_indexer_logits_desc* d, int32_t* out, int32_t cap) {
    Reason text;
    if (mla_indexer_logits_desc_error(d, false, text)) return -3;
    if (indexer_nothing_to_do(d)) return 0;
    const aule_hip::MlaIndexerPlan plan = mla_indexer_plan_of(d);
    return dump_plan({plan.group_tokens, plan.token_groups, plan.chunk_keys, plan.key_chunks, (int32_t)plan.grid}, nullptr, out, cap);
}

/* Debug hook: the launch plan of aule_attention_mla_prefill_backward_ex(d) as integers (include/aule.h lists them): the plan the launch
 * and the workspace query read.  Pure host logic like the forward hook. */
int32_t aule_hip_debug_mla_prefill_backward_plan(const aule_mla_prefill_bwd_desc* d, int32_t* out, int32_t cap) {
    Reason text;
    if (mla_prefill_bwd_desc_error(d, false, text)) return -3;
    if (mla_prefill_bwd_nothing_to_do(d)) return 0;
    const aule_hip::MlaPrefillBwdPlan plan = mla_prefill_bwd_plan_of(d);
    return dump_plan({plan.heads_per_chunk, plan.n_chunks, plan.max_chunks, (int32_t)plan.delta_grid, (int32_t)plan.dq_grid, (int32_t)plan.dkdv_grid,
                      (int32_t)plan.reduce_grid, plan.reduce ? 1 : 0}, &plan.ws_bytes, out, cap);
}

/* Debug hook: what the most recent backward launch of this process ran (bit mask, include/aule.h). */
int32_t aule_hip_debug_last_backward_route(void) { return aule_hip::bwd_last_route(); }

/* Debug hook: the same mask for the call aule_attention_backward_ex(d) would make with d->workspace_bytes bytes of workspace; -3 for a
 * descriptor it would refuse on shape grounds.  Pure host logic like the forward hook: the plan of the launch, not a launch. */
int32_t aule_hip_debug_backward_route(const aule_attn_bwd_desc* d) {
    Reason text;
    if (attn_desc_error(attn_prefix(d), sizeof(aule_attn_bwd_desc), text)) return -3;
    if (bwd_nothing_to_do(attn_prefix(d))) return 0;   // (nothing runs)
    if (d->seq_k == 0 || d->seq_q == 0) return -3;
    BwdArgs a;
    fill_bwd_args(d, a, true);
    if (d->workspace_bytes < a.ws_floor) return -3;
    return aule_hip::bwd_plan(a).route;
}

int32_t aule_hip_debug_forward_split_plan(const aule_attn_desc* d, int32_t* out, int32_t cap) {
    FwdArgs a;
    return plan_hook_args(d, a) ? aule_hip::fwd_split_plan_dump(a, out, cap) : -3;   // (0 unless the plan's route is 7)
}

int32_t aule_hip_debug_work_order(int32_t ranked, int32_t bid, int32_t batch, int32_t heads_q, int32_t heads_kv, int32_t nblk, int32_t flag, int32_t* out4) {
    if (out4 == nullptr || batch <= 0 || heads_kv <= 0 || heads_q <= 0 || heads_q % heads_kv != 0 || nblk <= 0) return -3;
    if (bid < 0 || (int64_t)bid >= (int64_t)batch * heads_q * nblk) return -3;
    int o[4];
    aule_hip::work_order_dump(ranked, bid, batch, heads_q, heads_kv, nblk, flag, o);
    for (int i = 0; i < 4; ++i) out4[i] = o[i];
    return 0;
}

/* Debug hook: the run-time switches this process runs under (csrc/fa_switches.h), one line per name, NAME=<resolved value>, the unset
 * default spelt like a set one.  Returns the bytes the text needs (NUL included) and writes at most `cap` of them.  No lock, no device,
 * no aule_init() needed; the first call of this or of any plan reads the environment, once. */
uint64_t aule_hip_debug_switches(char* buf, uint64_t cap) { return aule_hip::print_switches(aule_hip::switches(), buf, cap); }

#ifdef AULE_DEBUG_HOOKS
/* Debug hook (debug library only): bf16 D=128 forward with per-phase s_memtime stamps of workgroup 0 written to
 * `stamps` (device pointer; 8 * 256 uint64 for the ping-pong kernel, 8 * 2048 with AULE_TL=ps for the tile stream).
 * Used by tools/timeline.py / tools/timeline_w4.py. */
int32_t aule_hip_debug_forward_timeline(const aule_attn_desc* d, unsigned long long* stamps) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_init || stamps == nullptr) return -1;
    Reason text;
    if (const char* why = attn_desc_error(d, sizeof(aule_attn_desc), text)) return why == kBadDescriptor ? -1 : -3;
    if (d->dtype != AULE_DTYPE_BF16 || (d->head_dim != 128 && d->head_dim != 64)) return -3;   // the instrumented instances
    FwdArgs a;
    fill_fwd_args(d, a);
    if (aule_hip::switches().tl == aule_hip::Timeline::w4)   // AULE_TL=w4, one wave per SIMD: 4 waves x 2048 tagged stamps (tools/timeline_w4.py)
        return aule_hip::launch_fwd_w4_timeline(a, stamps, (hipStream_t)d->stream);
    return aule_hip::launch_fwd_pp_timeline(a, stamps, (hipStream_t)d->stream);
}
#endif  // AULE_DEBUG_HOOKS

}  // extern "C"
