// fa_fwd_mla_sparse_ds_gfx950.hip -- sparse multi-head latent attention over the per-128-scaled FP8 latent cache (the
// contract is aule_mla_sparse_ds_desc in include/aule.h): fa_fwd_mla_sparse_gfx950.hip's call in every respect but where a key row
// comes from.  q [T, Hq, 576] bf16, indices [T, topk] int32 slots, the cache read as a flat array of 656-byte rows [S][656]
// (fa_mla_ds.h: 512 e4m3fn codes, 4 fp32 scales, 64 bf16 rotary elements), key = bf16(code * its group's scale) | the rotary
// elements as stored, value = the key's first 512 elements.  out [T, Hq, 512], lse [T, Hq].
//
// The kernel is the paged MLA's body (fa_mla_common.h) with the list as its key source and fa_mla_ds.h's tile: the tile dequantises
// on its way into the LDS image, so the image, and with it every score, weight and accumulator, is what the 16-bit sparse kernel
// computes over the dequantised cache -- bit for bit, since plan, launch, split, partials and combine are that call's too
// (launch_mla_sparse with MlaSparseArgs::ds_rows).  No scale reaches the score scale or the accumulators.  bf16 only: the rotary
// part of a row is bf16.
#include "fa_mla_ds.h"

namespace aule_hip {
namespace {

__global__ void __launch_bounds__(256, 1) fa_fwd_mla_sparse_ds_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<Bf16Traits, KvFp8Ds, true>(p, Ls, Xs);
}

}  // namespace

// (`p` as launch_mla_sparse fills it for MlaSparseArgs::ds_rows: kv the [slots][656] rows, no kv_scale; grid: the plan's)
int launch_mla_sparse_ds_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream) {
    if (p.kv_scale != nullptr || p.list == nullptr || dtype != kBF16 || grid <= 0 || grid > 0x7fffffffll) return -1;
    hipLaunchKernelGGL(fa_fwd_mla_sparse_ds_kernel, dim3((unsigned)grid), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace aule_hip
