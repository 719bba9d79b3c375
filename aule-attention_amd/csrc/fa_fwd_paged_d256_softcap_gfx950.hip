// fa_fwd_paged_d256_softcap_gfx950.hip -- paged attention at head_dim 256 with logit soft-capping (Gemma-2: softcap = 50;
// DESIGN.md 3.22): decode, short verify and prompt chunks against the paged KV cache, 16-bit or FP8,
//     s_ij = softcap tanh(scale q_i.k_j / softcap),  P = softmax_j(s_ij over visible j),  out = P.V,  lse_i = ln sum_j exp(s_ij),
// everything else -- the contract, the work items, the key ranges the device derives, the partials and the combine -- as
// fa_fwd_paged_d256_gfx950.hip.  The mask is applied after the cap.
//
// The kernel is the kCap = true instance of paged_d256_body (fa_paged_d256_body.h) under a name of its own, in a translation unit of
// its own, so the plain kernel's four instances stay as they were.  The two waves of a row half exchange their partial products through
// LDS as before; each then caps own + other in place, y = cc - 2 cc rcp(1 + exp2(raw ci)) in log2 units (fa_softcap.h), and runs the
// online softmax on y -- the running max stays (a fixed maximum cc would underflow a row whose scores all sit near -softcap).  The host
// folds ci = 2 log2(e) scale / softcap into the parameter block's c; with an FP8 cache the kernel multiplies it by k_scale[hk] where the
// plain kernel multiplies scale log2(e), which puts the key scale inside the tanh.  The partials of a split launch carry m and l in
// the same log2 units, so the combine kernel is the plain file's, launched through launch_paged_d256_combine.
#include "fa_paged_d256_body.h"

namespace aule_hip {
namespace {

template <class T, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_d256_cap_kernel(const D256Params p, const float cc) {
    paged_d256_body<T, KV, true>(p, cc);
}

}  // namespace

// (`plan`: paged_d256_plan(a), the plain launch's; `ws` as launch_paged_d256's)  -1: unsupported arguments
int launch_paged_d256_softcap(const PagedD256Args& a, float softcap, const PagedD256Plan& plan, void* ws, hipStream_t stream) {
    if (!(softcap > 0.f && softcap <= 3.4e38f)) return -1;   // (finite, and not NaN)
    D256Params p(a.block_size);
    if (paged_d256_params(a, plan, ws, p) != 0) return -1;
    const SoftcapConsts k = softcap_consts(a.scale, softcap);
    p.c = k.ci;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    const int rc = dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (fp8) hipLaunchKernelGGL((fa_fwd_paged_d256_cap_kernel<T, KvFp8>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p, k.cc);
        else hipLaunchKernelGGL((fa_fwd_paged_d256_cap_kernel<T, Kv16>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p, k.cc);
        return (int)hipGetLastError();
    });
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_paged_d256_combine(p, a.dtype, stream);
}

}  // namespace aule_hip
