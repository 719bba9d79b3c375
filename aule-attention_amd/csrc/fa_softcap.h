// fa_softcap.h -- the logit soft-cap of the head_dim 256 kernels: s = softcap tanh(scale q.k / softcap).
//
// gfx950 has no tanh instruction.  tanh(x) = 1 - 2 / (1 + e^(2x)), so with the constants the host folds once,
//     ci = 2 log2(e) scale / softcap      (an FP8 cache's k_scale[hk] multiplies ci: it belongs inside the tanh)
//     cc = softcap log2(e)
// the capped score in the log2 units of the online softmax is  cc - 2 cc rcp(1 + exp2(raw ci)): two quarter-rate instructions per
// score.  The form is exact at both saturations -- exp2 -> inf gives rcp(inf) = 0 and +cc, exp2 -> 0 gives rcp(1) = 1 and -cc -- and
// carries a few ulp of cc near 0.  The backward takes r = rcp(1 + exp2(raw ci)) itself: t = 1 - 2 r and d s / d raw = scale (1 - t^2)
// = scale 4 r (1 - r), which has no cancellation at either saturation.
#pragma once
#include "fa_device.h"

namespace aule_hip {

struct SoftcapConsts {
    float ci, cc;
};
// (`softcap` finite and > 0: the entries check)
inline SoftcapConsts softcap_consts(float scale, float softcap) { return SoftcapConsts{2.f * kLog2e * scale / softcap, softcap * kLog2e}; }

namespace {

// the score in log2 units: the capped one (c = ci), or the plain product raw c (c = scale log2 e)
template <bool kCap>
__device__ __forceinline__ float score_log2(float raw, float c, float cc) {
    if constexpr (kCap) return cc - 2.f * cc * __builtin_amdgcn_rcpf(1.f + fast_exp2(raw * c));
    else return raw * c;
}

}  // namespace
}  // namespace aule_hip
