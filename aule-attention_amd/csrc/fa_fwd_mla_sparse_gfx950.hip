// fa_fwd_mla_sparse_gfx950.hip -- sparse multi-head LATENT attention (DeepSeek-V3.2 "DSA", absorbed form): every query token attends to
// the rows of the latent cache that ITS list names, in decode and in prefill (the contract is aule_mla_sparse_desc in
// include/aule.h).
//
// q [T, Hq, 576], the cache read as a flat array of slots [S, 576] (16-bit of q's dtype, or e4m3fn codes with one fp32 scale: those
// instances sit beside the dense FP8 kernel in fa_fwd_mla_paged_fp8_gfx950.hip), indices [T, topk] int32.  Token t's keys are the
// multiset { cache[indices[t][i]] : 0 <= indices[t][i] < S }: an entry outside the cache is skipped, a slot listed twice counts
// twice, nothing is causal.  out [T, Hq, 512], lse [T, Hq].
//
// The kernel is the paged MLA's body (fa_mla_common.h: image, split reduction, score exchange, online softmax, PV from the same image,
// partial / final store) instantiated with the list as its key source (kList; MlaListKeys there):
//   work item (split, row block, token): a row block is 64 heads of ONE token (tokens cannot share a block: their lists differ);
//   tile source: key k of the list is the row at slot indices[t][k], looked up one tile ahead; a row past topk or with an invalid
//     slot is not read but zero-filled, so a NaN in a row nobody names cannot reach P.V through p = 0;
//   mask: one wave-uniform validity word per tile, tested at compile-time bit positions (fa_mla_common.h, MlaListKeys).
//
// Key ranges: mla_sparse_plan below states row blocks, nsplit, grid and workspace by the dense rule (mla_split_plan) applied to the
// list: tiles = ceil(topk / 64), nsplit covers the compute units with T * row blocks * nsplit workgroups, at most kMlaMaxSplit and at
// most one split per two tiles.  Split k owns tiles [k * ceil(tiles / nsplit), ...); the partials have the dense layout and the dense
// combine kernel adds them in split order (no atomics: two runs give the same bits).  A split whose tiles hold no valid entry writes
// O = 0, m = -inf, l = 0.  Every one of the T rows is written.
#include <algorithm>

#include "fa_mla_common.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_mla_sparse_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, Kv16, true>(p, Ls, Xs);
}

}  // namespace

// The sparse call: row blocks of ONE token's heads, the tiles of its list.
MlaPlan mla_sparse_plan(int T, int Hq, int topk, int device, int force_nsplit) {
    if (T <= 0 || Hq <= 0 || topk <= 0) return MlaPlan();
    const long long tiles = ((long long)topk + kMlaKeys - 1) / kMlaKeys;
    const long long forced = force_nsplit > 0 ? std::min<long long>({force_nsplit, kMlaMaxSplit, tiles}) : 0;
    return mla_split_plan(((long long)Hq + kMlaRows - 1) / kMlaRows, T, tiles, T, Hq, device, forced);
}

// (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1)
int launch_mla_sparse(const MlaSparseArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream) {
    if ((long long)plan.row_blocks * a.T * 16 > 0x7fffffffll) return -1;   // (the combine's grid)
    if (a.topk < 1 || a.topk > kMlaSparseMaxTopk || a.slots < 1) return -1;
    if (a.indices == nullptr) return -1;
    MlaParams p;
    if (mla_common_params(a, plan, ws, p) != 0) return -1;
    p.table = nullptr; p.ctx = nullptr; p.cu = nullptr;
    p.B = a.T;
    p.bs = 1; p.bs_shift = 0;
    p.max_blocks = 0; p.max_sq = 1;
    p.list = a.indices; p.topk = a.topk; p.slots = a.slots;
    int rc;
    if (p.kv_scale != nullptr) {
        rc = launch_mla_sparse_fp8_kernel(p, plan.grid, a.dtype, stream);
    } else {
        rc = dispatch_16bit(a.dtype, [&](auto t) {
            hipLaunchKernelGGL((fa_fwd_mla_sparse_kernel<decltype(t)>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
            return (int)hipGetLastError();
        });
    }
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_mla_combine(p, plan.row_blocks, a.dtype, stream);
}

}  // namespace aule_hip
