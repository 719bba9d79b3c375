// fa_fwd_mla_paged_gfx950.hip -- paged multi-head LATENT attention (DeepSeek-V2 / V3 / R1, absorbed form): decode and short
// verify over a latent KV cache (the contract is aule_mla_paged_desc in include/aule.h).
//
// One cache [num_blocks, block_size, 576] of q's dtype: row `pos` of a sequence is the key of ALL query heads (576 elements: 512
// compressed dimensions, then 64 rotary ones) and its first 512 elements are the value.  q [T, Hq, 576], out [T, Hq, 512].
// (Or a cache of e4m3fn codes with one fp32 scale: its attention kernel is the same body, fa_mla_common.h, instantiated in
// fa_fwd_mla_paged_fp8_gfx950.hip; plan, launch and combine are the ones here.  With tree masks -- a tree of new tokens per sequence
// instead of the chain -- the same body once more, fa_fwd_mla_verify_gfx950.hip, behind the same plan, launch and combine.)
// Per sequence, read and clamped HERE exactly as the paged prefill does:
//     L = clamp(context_lens[b], 0, max_blocks * block_size)        s = clamp(cu[b], 0, T)      e = clamp(cu[b + 1], s, T)
//     n = min(e - s, max_seqlen_q)  (cu == null: s = b, n = 1);   token i < n is row s + i, sits at p = L - n + i, sees key j iff j <= p.
//
// Layout.  The packed rows of a sequence are token-major (row r = token r / Hq, head r % Hq) and all share the latent, so a
// workgroup owns a block of 64 rows and one key range, 4 waves, one per SIMD.  A tile of 64 latent rows (72 KB) is fetched from
// global memory ONCE, into one LDS image (pitch 1152 + 80 bytes: fa_d256_common.h, "rows read both ways"), and serves both products:
//   wave w = (rh = w & 1, ch = w >> 1) owns rows 32 rh .. 32 rh + 31 of the block.
//   S^T[key][row] = K.Q^T: the wave sums over elements 288 ch .. 288 ch + 287 only (18 operand chunk pairs, its Q chunks in 72
//     registers, 36 MFMAs of 32x32x16 per tile); the two waves of a row half exchange their partial sums through LDS (8 KB each,
//     lane to lane: no layout involved) and both add own + other -- the same two numbers, so both hold the same bits;
//   both do the rows' online softmax (log2 units, fp32 m / l), identically, and pack P^T as the B operand with no lane movement;
//   O^T[d][row] += V^T.P^T: the wave accumulates value columns 256 ch .. 256 ch + 255 (8 accumulators, 32 MFMAs per tile), V read
//     transposed (ds_read_b64_tr_b16) from the SAME image -- there is no second read of the cache for V.
// 68 MFMAs per wave and 64-key tile with no product computed twice; LDS 78 848 + 32 768 = 111 616 bytes; the next tile sits in
// 72 registers per thread while this one is computed (8 threads x 16 bytes = one 128-byte line of a latent row per request).
//
// Key ranges.  The host fixes nsplit from the shape alone (mla_split_plan below: the one place that decides row blocks, nsplit, grid and
// workspace); every workgroup derives ITS sequence's range on the device from the clamped L: split k owns the 64-key tiles
// [k * ceil(tiles(L) / nsplit), ...), so the work is balanced whatever the table's capacity.  nsplit == 1: one launch writes out /
// lse.  nsplit > 1: fp32 partials in the workspace -- un-normalised O [nsplit][T * Hq][512], then {m (log2 units), l}
// [nsplit][T * Hq][2], 514 floats per (split, token, head) -- and a combine kernel, one wave per row, that adds them in split order (no
// atomics: two runs give the same bits).  A split with no tile, or whose rows see none of its keys, writes O = 0, m = -inf, l = 0.
// Rows of no sequence are never written, by either kernel; a workspace is read only where this call wrote it.
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_mla_paged_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ls[kMlaLdsImage];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];
    mla_paged_body<T, Kv16>(p, Ls, Xs);
}

// The combine: workgroup (rank, sequence, sixteenth) takes four rows of the block the attention kernel's workgroups of that (rank,
// sequence) wrote, one row per wave: lane k holds split k's {m, l} (nsplit <= 64 = a wave), the weights come from one wave
// reduction, and the partial rows are added in split order with lane x on value columns 8 x .. 8 x + 7 (independent loads: the
// splits are in flight together).  merge_attention_states' rule for empty sides: a split with m = -inf weighs nothing; all of
// them empty gives zeros and lse = -inf.
constexpr int kMlaCombineParts = kMlaRows / 4;
static_assert(kMlaMaxSplit <= 64, "a lane per split");

template <class T>
__global__ void __launch_bounds__(256) fa_mla_combine_kernel(const MlaParams p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = (int)blockIdx.x;
    const int sub = bid % kMlaCombineParts, rest = bid / kMlaCombineParts;
    const int b = rest % p.B, rank = rest / p.B;
    const MlaBlock blk = p.list != nullptr ? MlaBlock(p, b, rank, MlaBlock::ListRows{}) : MlaBlock(p, b, rank);   // (the sparse call's partials)
    const int rl = 4 * sub + wave;
    if (rl >= blk.rows) return;
    const int r = blk.r0 + rl;
    const int tok = r / p.Hq, head = r - tok * p.Hq;
    const long long orow = ((long long)blk.s + tok) * p.Hq + head;
    float mk = -__builtin_inff(), lk = 0.f;
    if (lane < p.nsplit) {
        const f32x2_t ml = *reinterpret_cast<const f32x2_t*>(p.part_ml + ((long long)lane * p.rows_total + orow) * 2);
        mk = ml[0];
        lk = ml[1];
    }
    float mm = mk;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mm = fmaxf(mm, __shfl_xor(mm, off, 64));
    const float wk = mk == -__builtin_inff() ? 0.f : fast_exp2(mk - mm);
    float ls = wk * lk;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ls += __shfl_xor(ls, off, 64);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* po = p.part_o + orow * kMlaV + 8 * lane;
    for (int k = 0; k < p.nsplit; k += 4) {   // four splits in flight; lanes at or past nsplit hold weight 0
        f32x4_t a[4], c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* src = po + (long long)min(k + i, p.nsplit - 1) * p.rows_total * kMlaV;
            a[i] = *reinterpret_cast<const f32x4_t*>(src);
            c[i] = *reinterpret_cast<const f32x4_t*>(src + 4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float w = __shfl(wk, k + i, 64);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[e] += w == 0.f ? 0.f : w * a[i][e];
                acc[4 + e] += w == 0.f ? 0.f : w * c[i][e];
            }
        }
    }
    const float inv = ls > 0.f ? 1.f / ls : 0.f;
    *reinterpret_cast<u32x4_t*>(p.o + (orow * kMlaV + 8 * lane) * 2) =
        u32x4_t{T::pack2(acc[0] * inv, acc[1] * inv), T::pack2(acc[2] * inv, acc[3] * inv), T::pack2(acc[4] * inv, acc[5] * inv),
                T::pack2(acc[6] * inv, acc[7] * inv)};
    if (p.lse != nullptr && lane == 0) p.lse[orow] = ls > 0.f ? (mm + fast_log2(ls)) * kLn2 : -__builtin_inff();
}

}  // namespace

int launch_mla_combine(const MlaParams& p, int row_blocks, int dtype, hipStream_t stream) {
    const long long grid = (long long)row_blocks * p.B * kMlaCombineParts;
    if (grid <= 0 || grid > 0x7fffffffll) return -1;
    return dispatch_16bit(dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_mla_combine_kernel<decltype(t)>), dim3((unsigned)grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

// The launch plans: the one place that decides row blocks, nsplit, grid and workspace (launch, size query, debug hook), from the
// shape alone; WHICH tiles a split owns is decided on the device from each sequence's own length.  The rule is fa_mla_common.h's.
MlaPlan mla_split_plan(long long row_blocks, long long units, long long tiles, int T, int Hq, int device, long long nsplit) {
    const long long base = row_blocks * units;
    long long ns = nsplit;
    if (ns <= 0) {
        ns = (device_cu_count(device) + base - 1) / base;
        if (ns > kMlaMaxSplit) ns = kMlaMaxSplit;
        if (ns > tiles / 2) ns = tiles / 2;
        if (ns < 1) ns = 1;
    }
    MlaPlan plan;
    plan.row_blocks = (int)row_blocks;
    plan.rows_per_block = kMlaRows;
    plan.nsplit = (int)ns;
    plan.grid = base * ns;
    plan.ws_bytes = ns > 1 ? ((uint64_t)ns * (uint64_t)T * (uint64_t)Hq * (kMlaV + 2) * 4 + 15) & ~15ull : 0;
    return plan;
}

// The dense call: row blocks of a sequence's packed rows, the tiles of the table's capacity.
MlaPlan mla_plan(const MlaArgs& a) {
    if (a.T <= 0 || a.B <= 0 || a.Hq <= 0 || a.max_seqlen_q <= 0 || a.block_size <= 0 || a.max_blocks <= 0) return MlaPlan();
    const long long rb = ((long long)seqlen_cut(a.max_seqlen_q, a.T) * a.Hq + kMlaRows - 1) / kMlaRows;
    return mla_split_plan(rb, a.B, ((long long)a.block_size * a.max_blocks + kMlaKeys - 1) / kMlaKeys, a.T, a.Hq, a.device);
}

// (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1)
int launch_mla_paged(const MlaArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream) {
    if ((long long)plan.row_blocks * a.B * kMlaCombineParts > 0x7fffffffll) return -1;
    if ((long long)a.block_size * a.max_blocks >= (1ll << 30)) return -1;
    if (a.cu_seqlens_q == nullptr && a.T < a.B) return -1;
    MlaParams p;   // (list stays null, its default: that is what tells the combine kernel that these are a dense call's partials)
    if (mla_common_params(a, plan, ws, p) != 0) return -1;
    p.table = a.block_tables; p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.B = a.B;
    p.bs = a.block_size;
    p.bs_shift = shift_of(a.block_size);
    p.max_blocks = a.max_blocks;
    p.max_sq = seqlen_cut(a.max_seqlen_q, a.T);
    int rc;
    if (a.tree_mask != nullptr) {   // (either cache kind; fa_fwd_mla_verify_gfx950.hip)
        if (a.cu_seqlens_q == nullptr) return -1;
        p.tree_mask = a.tree_mask;
        rc = launch_mla_verify_kernel(p, plan.grid, a.dtype, stream);
    } else if (p.kv_scale != nullptr) {
        rc = launch_mla_fp8_kernel(p, plan.grid, a.dtype, stream);
    } else {
        rc = dispatch_16bit(a.dtype, [&](auto t) {
            hipLaunchKernelGGL((fa_fwd_mla_paged_kernel<decltype(t)>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
            return (int)hipGetLastError();
        });
    }
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_mla_combine(p, plan.row_blocks, a.dtype, stream);
}

}  // namespace aule_hip
