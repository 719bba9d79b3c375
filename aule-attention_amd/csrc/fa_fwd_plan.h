// fa_fwd_plan.h -- the forward decided once, as a value (host only; the forward's counterpart of fa_bwd_plan.h).
// fwd_plan() is everything launch_fwd and the workspace-size query need to know about a call: which kernel runs, the bytes of its
// partials and the chosen kernel's own launch plan.  Pure host logic: it reads the shape, the mask, the scale's sign, the rope table
// geometry (the pointers for null and alignment only) and the once-per-process AULE_HIP_FWD_* / AULE_HIP_W4_* / AULE_HIP_F32_SPLIT
// switches; it dereferences no pointer and asks the device nothing but its (cached) CU count.  The dispatch order is fwd_plan() in
// fa_fwd_gfx950.hip; what a kernel can take and its sub-plan are stated in the kernel's own file.  (A rope request the plan cannot
// fuse is refused by launch_fwd; ws_bytes is then what the same call without the tables would use.)
#pragma once
#include "fa_kernels.h"
#include "fa_switches.h"

namespace aule_hip {

// Route 8, the grid of the one-wave-per-SIMD kernel: causal Q blocks paired or not, work items per head and in all, workgroups (one
// per CU; more only when a workgroup's list would not fit its part table), the round order (rounds = 0: item order; heads per round)
struct W4Grid { int pair, nwork, nitems, G, rounds, mper; };
// Route 7: the same kernel with every pair of causal Q blocks (every non-causal block) cut into n key ranges (fa_fwd_split.h)
struct SplitPlan {
    bool ok;
    int nqb, nwork, n;
    long long nitems;
    size_t bytes;
};
// Route 5: the ping-pong kernel's SPLIT instances, packed rows + KV splits (fa_fwd_pp_gfx950.hip)
struct PPSplitPlan {
    int g, rows, nqb, nbase, ntiles, nsplit, chunk, nrt;
    uint64_t bytes(int units, int D) const { return (uint64_t)nsplit * units * nrt * 32 * (D + 2) * sizeof(float); }   // units = B * Hkv
};
// Route 4 and the paged decode, the wave-per-chunk launch: 32-row tiles per unit, 32-key tiles per wave, workgroups along the keys
// (four waves each), partials per row (nsplit * 4), partial rows (B * Hkv * nrt * 32)
struct WaveChunkPlan {
    int nrt, chunk_tiles, nsplit, npart, rows_total;
    uint64_t bytes(int D) const { return (uint64_t)npart * rows_total * (D + 2) * sizeof(float); }
};

struct FwdPlan {
    int route = 0;            // fwd_route()'s codes (fa_kernels.h, include/aule.h)
    uint64_t ws_bytes = 0;    // partials of the two-launch routes (0: single launch)
    W4Grid w4 = {};           // the chosen route's sub-plan (the others stay zero): 8
    SplitPlan split = {};     // 7
    PPSplitPlan pp = {};      // 5
    WaveChunkPlan wave = {};  // 4
    int f32_pieces = 0;       // 0: key-range pieces per Q block (1 = single launch)
};
FwdPlan fwd_plan(const FwdArgs& a);   // fa_fwd_gfx950.hip

// What each kernel file states about itself (a bool answer: the route can take `a`, and s is its plan then) ...
bool fwd_w4_applicable(const FwdArgs& a);                  // fa_fwd_w4_gfx950.hip
bool fwd_w4_split_plan(const FwdArgs& a, SplitPlan& s);
W4Grid fwd_w4_grid(const FwdArgs& a);
bool fwd_pp_split_plan(const FwdArgs& a, PPSplitPlan& s);  // fa_fwd_pp_gfx950.hip
bool splitkv_applicable(const FwdArgs& a);                 // fa_fwd_splitkv_gfx950.hip
WaveChunkPlan wave_chunk_plan(int B, int Hq, int Hkv, int Sq, int Sk);
int fwd_f32_pieces(const FwdArgs& a);                      // fa_fwd_f32.hip
uint64_t fwd_f32_workspace_bytes(const FwdArgs& a, int pieces);
// ... and its launcher, which executes a plan and never plans again
int launch_fwd_f32(const FwdArgs& a, int pieces, hipStream_t stream);
int launch_fwd_pp(const FwdArgs& a, hipStream_t stream);
int launch_fwd_pp_split(const FwdArgs& a, const PPSplitPlan& s, hipStream_t stream);
int launch_fwd_w4(const FwdArgs& a, const W4Grid& g, hipStream_t stream);
int launch_fwd_w4_split(const FwdArgs& a, const SplitPlan& s, hipStream_t stream);
int launch_fwd_splitkv(const FwdArgs& a, const WaveChunkPlan& w, hipStream_t stream);
int launch_fwd_d256(const FwdArgs& a, hipStream_t stream);   // fa_fwd_d256_gfx950.hip (every dtype)

}  // namespace aule_hip
