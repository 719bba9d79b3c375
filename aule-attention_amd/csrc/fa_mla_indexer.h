// fa_mla_indexer.h -- what the two logits kernels of the MLA indexer share on the host: the kernel parameters and their one fill
// (fa_mla_indexer_gfx950.hip holds both; fa_mla_indexer_fp8mma_gfx950.hip is the second reader).
#pragma once

#include "fa_kernels.h"

namespace aule_hip {

struct IdxParams {
    const char* q;
    const float* w;
    const char* k;
    const float* ks;     // FP8 cache: [num_blocks * block_size] fp32; else null
    const int* table;
    const int* ctx;
    const int* cu;       // null: sequence b owns row b
    float* out;
    long long q_stride, out_stride;
    int T, B, H;
    int nb, bs, bs_shift;
    int max_blocks, max_sq;
    int W;               // max_blocks * bs
    int groups, chunks, chunk_keys;
};

// mla_indexer_plan's rule for work items of group_tokens tokens
MlaIndexerPlan mla_indexer_plan_grouped(int B, int max_seqlen_q, long long W, int device, int group_tokens);
// The rules of the shape every logits launch checks, and `p` from (a, plan); -1: unsupported.  What depends on q's type (its stride
// rule, the cache kinds it goes with) is the caller's.
int mla_indexer_params(const MlaIndexerArgs& a, const MlaIndexerPlan& plan, IdxParams& p);

}  // namespace aule_hip
