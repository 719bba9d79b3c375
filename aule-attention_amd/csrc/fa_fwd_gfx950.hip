// fa_fwd_gfx950.hip -- forward dispatch for MI355X (gfx950 / CDNA4).
//
// Replaces, behind aule_attention_forward_ex, the Triton launch of the reference
// (python/aule/triton_flash_amd.py:393-445 FlashAttentionAMDFunc.forward and its
// kernel :97-240) and the HIP stub slot (src/backends/attention_hip.cpp:22-119).
// Numerics contract: s = scale * q.k ; top-left causal
// mask (j <= i) ; online softmax with fp32 m, l, acc ; P cast to the V dtype
// before the PV product (triton_flash_amd.py:222) ; LSE = m + ln(l) (:237).
//
// The kernels live in their own files; this one only picks among them: fwd_plan() (fa_fwd_plan.h) states once which kernel a call
// runs, its workspace and that kernel's launch plan, and launch_fwd() executes that plan (host logic):
//   fa_fwd_w4_gfx950.hip       16-bit, one wave per SIMD (4 x 64 query rows), persistent part lists: the default for tiled problems;
//                              small grids as key-range pieces + merge (fa_fwd_split.h)
//   fa_fwd_pp_gfx950.hip       16-bit, two waves per SIMD, one workgroup per Q-block pair: sliding windows below 128 keys or without the causal rule, fewer
//                              than four KV tiles per Q block, D = 32, scale = 0, and the SPLIT instances (packed rows + KV splits) for short queries
//   fa_fwd_splitkv_gfx950.hip  16-bit, wave-per-chunk split-KV (decode streaming corner) and paged decode
//   fa_fwd_f32.hip             fp32 I/O
// Common to the 16-bit kernels: "swapped" S^T = K.Q^T so that a lane owns one query row; P stays in registers as
// the B operand of O^T += V^T.P^T; K row-major and V sub-tiled in LDS; all blocks of one (batch, kv-head) on one XCD.
// (Retired, in the history: the lock-step kernel of round 1 and the in-wave pipelined variants -- fa_fwd_iw_gfx950.hip -- in
// round 2; the two-waves-per-SIMD persistent tile stream -- fa_fwd_ps_gfx950.hip, routes 6 and 7 of rounds 2-3 -- in round 4,
// when the one-wave-per-SIMD kernel took its small-grid split and the ping-pong kernel its remaining shapes.)
#include <cstdio>
#include <cstdlib>

#include "fa_device.h"
#include "fa_fwd_plan.h"
#include "fa_kernels.h"
#include "fa_switches.h"

namespace aule_hip {
int configure_fwd_f32();   // fa_fwd_f32.hip
int configure_fwd_pp();    // fa_fwd_pp_gfx950.hip
int configure_fwd_w4();    // fa_fwd_w4_gfx950.hip

// Non-causal problems that the plain tiled launch would run badly (few workgroups, or Q blocks mostly without rows):
// 4 = wave-per-chunk split-KV kernel, 5 = tiled kernel with packed rows + KV splits (`pp` is its plan then), 0 = neither.
// Measured on one box per comparison (tools/ppsplit_grid.py, tools/ppsplit_decode.py): the tiled variant wins
// almost everywhere, including Sq = 1 (its combine merges <= 32 partials per row, the wave kernel's hundreds); the wave kernel
// keeps the pure streaming corner -- many units, at most half a row tile of packed rows, K+V beyond ~100 MB -- where
// it is 10-15 % ahead at D = 128 and 35-55 % at D = 64.  Differences below ~8 % on these kernels are noise.
static int short_query_route(const FwdArgs& a, PPSplitPlan& pp) {
    if (a.window > 0) return 0;
    const bool wave_ok = !a.causal && switches().fwd_splitkv && splitkv_applicable(a);   // (the wave kernel has no mask; AULE_HIP_FWD_SPLITKV=0: A/B)
    PPSplitPlan s;
    const bool tiled_ok = fwd_pp_split_plan(a, s);
    int route = wave_ok ? 4 : (tiled_ok ? 5 : 0);
    if (wave_ok && tiled_ok) {
        const long long units = (long long)a.B * a.Hkv;
        const long long rows = (long long)(a.Hq / a.Hkv) * a.Sq;
        const double kv_bytes = 2.0 * (double)units * a.Sk * a.D * 2.0;
        route = (units >= 32 && rows <= 16 && kv_bytes >= 100e6) ? 4 : 5;
    }
    if (route == 5) pp = s;
    return route;
}

// The dispatch order, stated once.  FwdPlan::route: 0 fp32, 1 ping-pong, 4 split-KV, 5 ping-pong kernel with packed rows + KV
// splits, 7 one-wave-per-SIMD kernel with every pair of causal Q blocks (every non-causal block) cut into key ranges (small grids;
// partials + merge), 8 one-wave-per-SIMD kernel (4 x 64 rows), 9 the head_dim 256 kernel (2, 3 and 6 were the removed in-wave,
// lock-step and two-waves-per-SIMD stream kernels).  Lets the tests pin the path a shape exercises.
FwdPlan fwd_plan(const FwdArgs& a) {
    FwdPlan p;
    if (a.dtype == kF32) {
        // Route 0 at every head size, on purpose: 0 is "the fp32 path" to callers (include/aule.h).  At head_dim 256 that is the
        // fp32 instance of the head_dim 256 file (launch_fwd, case 0), a single launch.
        p.f32_pieces = a.D == 256 ? 1 : fwd_f32_pieces(a);
        p.ws_bytes = fwd_f32_workspace_bytes(a, p.f32_pieces);
        return p;
    }
    if (a.D == 256) {
        p.route = 9;
        return p;
    }
    p.route = short_query_route(a, p.pp);
    if (p.route == 4) {
        p.wave = wave_chunk_plan(a.B, a.Hq, a.Hkv, a.Sq, a.Sk);
        p.ws_bytes = p.wave.bytes(a.D);
    } else if (p.route == 5) {
        p.ws_bytes = p.pp.bytes(a.B * a.Hkv, a.D);
    } else {
        // short / non-causal windows, fewer than four KV tiles per Q block, D = 32, scale = 0, AULE_HIP_FWD_KERNEL=pp (A/B against the
        // one-wave-per-SIMD kernel) and the online softmax stay on the ping-pong kernel.  (AULE_HIP_FWD_SOFTMAX=classic asks for the
        // online softmax throughout, default "raw" for bf16: the ping-pong kernel then runs its online instances; the one-wave-per-SIMD
        // kernel has no online form -- its fall-back is a second pass with the exact row maximum.)
        const bool w4 = switches().fwd_kernel != FwdKernel::pp && !switches().fwd_softmax_classic;
        if (w4 && fwd_w4_split_plan(a, p.split)) {
            p.route = 7;
            p.ws_bytes = p.split.bytes;
        } else if (w4 && fwd_w4_applicable(a)) {
            p.route = 8;
            p.w4 = fwd_w4_grid(a);
        } else {
            p.route = 1;
        }
    }
    return p;
}

int fwd_route(const FwdArgs& a) { return fwd_plan(a).route; }

// Which problems the forward rotates Q for by itself (half-split pairs, K already rotated): what the one-wave-per-SIMD kernel
// takes (its applicability rule looks at the table geometry too).
bool fwd_rope_fusable(const FwdArgs& a) { return fwd_plan(a).route == 8; }

uint64_t fwd_workspace_bytes(const FwdArgs& a) { return fwd_plan(a).ws_bytes; }

static std::atomic<int> g_last_fwd_route{0};
int fwd_last_route() { return g_last_fwd_route.load(); }

int launch_fwd(const FwdArgs& a, hipStream_t stream) {
    const FwdPlan p = fwd_plan(a);
    if (a.rope_cos != nullptr && p.route != 8) return -1;   // only the one-wave-per-SIMD kernel rotates Q itself
    g_last_fwd_route.store(p.route);
    switch (p.route) {
        case 0: return a.D == 256 ? launch_fwd_d256(a, stream) : launch_fwd_f32(a, p.f32_pieces, stream);
        case 4: return launch_fwd_splitkv(a, p.wave, stream);
        case 5: return launch_fwd_pp_split(a, p.pp, stream);
        case 7: return launch_fwd_w4_split(a, p.split, stream);
        case 8: return launch_fwd_w4(a, p.w4, stream);
        case 9: return launch_fwd_d256(a, stream);
        default: return launch_fwd_pp(a, stream);
    }
}

// The plan as integers (aule_hip_debug_forward_plan): route, ws_bytes low / high, then the chosen route's sub-plan.
int fwd_plan_dump(const FwdArgs& a, int* out, int cap) {
    const FwdPlan p = fwd_plan(a);
    const int sub[10][8] = {{p.f32_pieces}, {}, {}, {}, {p.wave.nrt, p.wave.chunk_tiles, p.wave.nsplit, p.wave.npart, p.wave.rows_total},
                            {p.pp.g, p.pp.rows, p.pp.nqb, p.pp.nbase, p.pp.ntiles, p.pp.nsplit, p.pp.chunk, p.pp.nrt}, {},
                            {p.split.n, p.split.nwork, p.split.nqb, (int)p.split.nitems}, {p.w4.pair, p.w4.nwork, p.w4.nitems, p.w4.G, p.w4.rounds, p.w4.mper}, {}};
    static const int nsub[10] = {1, 0, 0, 0, 5, 8, 0, 4, 6, 0};
    const int n = 3 + nsub[p.route];
    if (out == nullptr || cap < n) return -n;
    out[0] = p.route; out[1] = (int)(uint32_t)p.ws_bytes; out[2] = (int)(uint32_t)(p.ws_bytes >> 32);
    for (int i = 3; i < n; ++i) out[i] = sub[p.route][i - 3];
    return n;
}

int configure_fwd() {
    int rc = 0;
    rc |= configure_fwd_f32();
    rc |= configure_fwd_pp();
    rc |= configure_fwd_w4();
    return rc;
}

}  // namespace aule_hip
