// fa_fwd_mla_verify_gfx950.hip -- the paged MLA attention kernel with TREE MASKS: the verify step of tree drafters (MTP heads, EAGLE,
// Medusa) over the latent KV cache (the contract is aule_mla_paged_tree_desc in include/aule.h).
//
// The dense call of fa_fwd_mla_paged_gfx950.hip with one int64 word per packed token: a sequence with n <= 64 new tokens carries a
// tree -- its token i sees key j < L iff j < L - n or bit j - (L - n) of tree_mask[s + i] is set -- and a longer one keeps the causal
// rule, decided per sequence on the device.  The body is fa_mla_common.h's, the one of the dense kernels, instantiated with kTree:
// what differs is stated there (MlaTreeKeys: the key range of a sequence with a tree is not cut at the block's last position, and a
// score counts by the row's visibility word of the tile).  Both cache kinds live here, four instances; plan, launch, workspace,
// partials and combine are fa_fwd_mla_paged_gfx950.hip's.
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

template <class T, class KV>
__global__ void __launch_bounds__(256, 1) fa_mla_verify_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, KV, false, true>(p, Ls, Xs);
}

}  // namespace

// (`p` as launch_mla_paged fills it, tree_mask and cu set, kv_scale set for an FP8 cache; grid: the plan's)
int launch_mla_verify_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream) {
    if (p.tree_mask == nullptr || p.cu == nullptr || grid <= 0 || grid > 0x7fffffffll) return -1;
    return dispatch_16bit(dtype, [&](auto t) {
        if (p.kv_scale != nullptr) hipLaunchKernelGGL((fa_mla_verify_kernel<decltype(t), KvFp8>), dim3((unsigned)grid), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_mla_verify_kernel<decltype(t), Kv16>), dim3((unsigned)grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
