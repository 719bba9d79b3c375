// fa_fwd_mla_paged_fp8_gfx950.hip -- the paged MLA attention kernel over an FP8 latent cache (the contract is
// aule_mla_paged_fp8_desc in include/aule.h): kv_cache [num_blocks, block_size, 576] OCP e4m3fn codes and ONE fp32 scale on the
// device, key = kv_scale * float(code row), value = its first 512 elements.
//
// The body is fa_mla_common.h's, the one of the 16-bit kernel, with the other tile: a latent row is read from HBM as 576 bytes
// instead of 1152 (8 threads x 8 bytes per request, 36 prefetch registers per thread instead of 72) and converted EXACTLY to q's
// 16-bit type (cvt8: every e4m3fn value is a bf16 and an fp16 value) on its way into the same LDS image; everything downstream of
// the image -- score MFMAs, exchange, softmax, transposed V reads, PV, partials -- is the same instruction stream.  The scale is
// never applied per element: it multiplies the score scale (so m, l and lse include it) and the fp32 accumulators on their way
// out, the un-normalised partials of a split call included.  Plan, launch, workspace and combine are fa_fwd_mla_paged_gfx950.hip's.
// The sparse call's FP8 instances (keys from a per-token list; plan and launch in fa_fwd_mla_sparse_gfx950.hip) live here too: this
// unit holds every instance of the body that converts codes, the other two those that do not, which keeps compile times even.
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_mla_fp8_latent_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, KvFp8>(p, Ls, Xs);
}

// The sparse call over the same codes (fa_fwd_mla_sparse_gfx950.hip): the body with the list as its key source.
template <class T>
__global__ void __launch_bounds__(256, 1) fa_mla_sparse_fp8_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, KvFp8, true>(p, Ls, Xs);
}

}  // namespace

// (`p` as launch_mla_paged fills it, kv_scale set; grid: the plan's)
int launch_mla_fp8_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream) {
    if (p.kv_scale == nullptr || grid <= 0 || grid > 0x7fffffffll) return -1;
    return dispatch_16bit(dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_mla_fp8_latent_kernel<decltype(t)>), dim3((unsigned)grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

// (`p` as launch_mla_sparse fills it, kv_scale set; grid: the plan's)
int launch_mla_sparse_fp8_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream) {
    if (p.kv_scale == nullptr || p.list == nullptr || grid <= 0 || grid > 0x7fffffffll) return -1;
    return dispatch_16bit(dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_mla_sparse_fp8_kernel<decltype(t)>), dim3((unsigned)grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
