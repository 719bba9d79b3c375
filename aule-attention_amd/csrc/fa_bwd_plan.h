// fa_bwd_plan.h -- the backward decided once, as a value (host only; the backward's counterpart of fa_fwd_plan.h).
// bwd_plan() is everything launch_bwd and the workspace-size queries need to know about a call.  Pure host logic: it reads the shape,
// the mask, BwdArgs::ws_bytes / ws_floor, the debug inputs (dbg / dbg_dq; AULE_TL=dkv4, AULE_DBG_BWD_ONLY) and the once-per-process
// AULE_HIP_BWD_* switches; it dereferences no pointer and asks the device nothing but its (cached) CU count.
#pragma once
#include "fa_kernels.h"

namespace aule_hip {

// BwdPlan::route (aule_hip_debug_backward_route / _last_backward_route, include/aule.h): 1 the 5-matmul mode (delta pass + dK/dV kernel
// that spills its packed dS + dQ = dS K; always with 4), 2 / 4 the one-wave-per-SIMD dQ / dK/dV kernel, 8 / 16 their two-waves-per-SIMD
// predecessors, 32 the fp32 kernels, 64 (with 4) the D = 64 dK/dV instance with two key blocks per wave, 128 head_dim 256 (with 32: fp32)
enum BwdRoute : int { kRouteSpill = 1, kRouteDq4 = 2, kRouteDkv4 = 4, kRouteDqOld = 8, kRouteDkvOld = 16, kRouteF32 = 32, kRouteDkv4K2 = 64, kRouteD256 = 128 };

struct BwdPlan {
    int route = 0;
    // The 16-bit workspace as byte offsets from its base (BwdArgs::delta): delta [B,Hq,Sq] fp32 at 0 | L' = LSE log2(e) | - delta | fp32
    // dK / dV partials of the head split [2][gsplit][B,Hkv,Sk,D] (gsplit > 1) | dS of one batch chunk (DsLayout; the 5-matmul mode).
    // (fp32, D = 256: delta at 0, then what their own launchers lay out -- only the sizes below are theirs here.)
    uint64_t lse2_off = 0, ndelta_off = 0, part_off = 0, ds_off = 0;
    uint64_t min_bytes = 0;    // what the call cannot do without (everything but the dS room)
    uint64_t want_bytes = 0;   // ... plus dS room for as many batch elements as AULE_HIP_BWD_DS_CAP_MB holds: what the size query answers
    int gsplit = 1;            // two-waves-per-SIMD dK/dV kernel: workgroups that share the query heads of a GQA group
    int nb = 0;                // kRouteSpill: batch elements per chunk (the dS room behind ds_off holds that many)
    bool k2 = false;           // kRouteDkv4K2
};

BwdPlan bwd_plan(const BwdArgs& a);   // fa_bwd_gfx950.hip

}  // namespace aule_hip
