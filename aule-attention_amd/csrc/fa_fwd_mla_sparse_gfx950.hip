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
// Key ranges: mla_sparse_plan below is the one statement of row blocks, nsplit, grid and workspace -- the dense rule applied to the
// list: tiles = ceil(topk / 64), nsplit covers the compute units with T * row blocks * nsplit workgroups, at most kMlaMaxSplit and at
// most one split per two tiles.  Split k owns tiles [k * ceil(tiles / nsplit), ...); the partials have the dense layout and the dense
// combine kernel adds them in split order (no atomics: two runs give the same bits).  A split whose tiles hold no valid entry writes
// O = 0, m = -inf, l = 0.  Every one of the T rows is written.
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_mla_sparse_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, Kv16, true>(p, Ls, Xs);
}

int launch_16(const MlaParams& p, long long grid, int dtype, hipStream_t stream) {
    if (dtype == kBF16) {
        hipLaunchKernelGGL((fa_fwd_mla_sparse_kernel<Bf16Traits>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    } else if (dtype == kF16) {
        hipLaunchKernelGGL((fa_fwd_mla_sparse_kernel<F16Traits>), dim3((unsigned)grid), dim3(256), 0, stream, p);
    } else {
        return -1;
    }
    return (int)hipGetLastError();
}

}  // namespace

MlaPlan mla_sparse_plan(int T, int Hq, int topk, int device, int force_nsplit) {
    MlaPlan plan;
    if (T <= 0 || Hq <= 0 || topk <= 0) return plan;
    const long long rb = ((long long)Hq + kMlaRows - 1) / kMlaRows;
    const long long base = rb * T;
    const long long cus = device_cu_count(device);
    const long long tiles = ((long long)topk + kMlaKeys - 1) / kMlaKeys;
    long long ns = (cus + base - 1) / base;
    if (ns > kMlaMaxSplit) ns = kMlaMaxSplit;
    if (ns > tiles / 2) ns = tiles / 2;
    if (ns < 1) ns = 1;
    if (force_nsplit > 0) ns = force_nsplit < kMlaMaxSplit ? (force_nsplit < tiles ? force_nsplit : tiles) : (kMlaMaxSplit < tiles ? kMlaMaxSplit : tiles);
    plan.row_blocks = (int)rb;
    plan.rows_per_block = kMlaRows;
    plan.nsplit = (int)ns;
    plan.grid = base * ns;
    plan.ws_bytes = ns > 1 ? ((uint64_t)ns * (uint64_t)T * (uint64_t)Hq * (kMlaV + 2) * 4 + 15) & ~15ull : 0;
    return plan;
}

// (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1)
int launch_mla_sparse(const MlaSparseArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream) {
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll || (long long)plan.row_blocks * a.T * 16 > 0x7fffffffll) return -1;   // (attention and combine grids)
    if (a.topk < 1 || a.topk > kMlaSparseMaxTopk || a.slots < 1) return -1;
    if (a.q_token_stride < (long long)a.Hq * kMlaQK || a.q_token_stride % 8 != 0) return -1;
    if (((long long)a.T + kMlaRows) * a.Hq > 0x7fffffffll) return -1;   // the kernels count packed rows in 32 bits
    if (plan.nsplit > 1 && ws == nullptr) return -1;
    if (a.indices == nullptr) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 ? a.kv_scale == nullptr : a.cache_kind != kCache16) return -1;
    MlaParams p;
    p.q = static_cast<const char*>(a.q); p.kv = static_cast<const char*>(a.kv_cache);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    p.rows_total = (long long)a.T * a.Hq;
    p.part_o = static_cast<float*>(ws);
    p.part_ml = p.part_o != nullptr ? p.part_o + (long long)plan.nsplit * p.rows_total * kMlaV : nullptr;
    p.table = nullptr; p.ctx = nullptr; p.cu = nullptr;
    p.q_stride = a.q_token_stride;
    p.T = a.T; p.B = a.T; p.Hq = a.Hq;
    p.bs = 1; p.bs_shift = 0;
    p.max_blocks = 0; p.max_sq = 1;
    p.row_blocks = plan.row_blocks; p.nsplit = plan.nsplit;
    p.c = a.scale * kLog2e;
    p.kv_scale = fp8 ? a.kv_scale : nullptr;
    p.list = a.indices; p.topk = a.topk; p.slots = a.slots;
    const int rc = fp8 ? launch_mla_sparse_fp8_kernel(p, plan.grid, a.dtype, stream) : launch_16(p, plan.grid, a.dtype, stream);
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_mla_combine(p, plan.row_blocks, a.dtype, stream);
}

}  // namespace aule_hip
