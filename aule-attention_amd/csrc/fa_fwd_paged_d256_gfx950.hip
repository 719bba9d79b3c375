// fa_fwd_paged_d256_gfx950.hip -- paged attention at head_dim 256 (Gemma-2 / Gemma-3 / Qwen3-Next heads): decode, short verify and
// prompt chunks of ragged sequences against the paged KV cache, 16-bit or FP8 (the contract is aule_paged_d256_desc
// in include/aule.h).  q [T, Hq, 256], k_cache / v_cache [num_blocks, block_size, Hkv, 256], out [T, Hq, 256].
// Per sequence, read and clamped HERE with the rules of fa_device.h (seq_len, seq_range, block_of), as the paged prefill does:
//     L = clamp(context_lens[b], 0, max_blocks * block_size)        s = clamp(cu[b], 0, T)      e = clamp(cu[b + 1], s, T)
//     n = min(e - s, max_seqlen_q)  (cu == null: s = b, n = 1);   token i < n is row s + i, sits at p = L - n + i, sees key j iff
//     j <= p and, with a window W > 0, p - j < W.
//
// Work item: (sequence, KV head, block of 64 packed rows, key range).  The rows of a (sequence, KV head) are packed token-major (row r
// = token r / g, head hk g + r % g, g = Hq / Hkv): positions are monotone in r, so the keys a block sees are ONE interval.  256 threads,
// 4 waves, one per SIMD; wave w = (rh = w & 1, ch = w >> 1) owns rows 32 rh .. 32 rh + 31 of the block and HALF of the head dimension:
//   S^T[key][row] = K.Q^T: the wave sums over elements 128 ch .. 128 ch + 127 only (8 operand chunk pairs, its Q chunks in 32
//     registers, 16 MFMAs of 32x32x16 per 64-key tile); the two waves of a row half exchange their partial sums through LDS (8 KB each,
//     lane to lane: no layout involved) and both add own + other -- the same two numbers, so both hold the same bits;
//   both do the rows' online softmax (log2 units, fp32 m / l), identically, and pack P^T as the B operand with no lane movement;
//   O^T[d][row] += V^T.P^T: the wave accumulates value columns 128 ch .. 128 ch + 127 (4 accumulators, 16 MFMAs per tile), V read
//     transposed (ds_read_b64_tr_b16).
// 32 MFMAs per wave and tile, no product computed twice; a decode block of <= 32 rows has both waves of rh = 0 on the MFMAs and all
// four waves staging; a wave without a live row skips the arithmetic, not the barriers.
// Tiles: 64 keys of K (pitch 528) and V (pitch 576) in two LDS images, 33 792 + 36 864 bytes, plus 32 768 of partial scores = 103 424;
// the next tile sits in registers (PagedTile: 64 per thread for a 16-bit cache, 32 for FP8, whose codes become 16-bit chunks on the
// way into LDS -- k_scale[hk] joins the score scale, v_scale[hk] the epilogue, so the MFMA loop is one for both cache kinds), the table
// is walked one tile ahead of the loads.
//
// Key ranges.  The host fixes nsplit from the shape alone (paged_d256_plan below: the one place that decides row blocks, nsplit, grid and
// workspace); every workgroup derives ITS range on the device: the block's visible keys [vbeg, vend) -- from the clamped L, the block's
// first and last position and the window -- cover the 64-key tiles [tb, te), and split k owns tiles [tb + k ceil((te - tb) / nsplit), ...).
// So a short context behind a large table is balanced, and so is a window over a long context.  nsplit == 1: one launch writes out /
// lse.  nsplit > 1: fp32 partials in the workspace -- un-normalised O [nsplit][T * Hq][256], then {m (log2 units), l}
// [nsplit][T * Hq][2] -- and a combine kernel, one wave per row, that adds them in split order (no atomics: two runs give the same
// bits).  A split with no tile, or whose rows see none of its keys, writes O = 0, m = -inf, l = 0.  Rows of no sequence are never
// written, by either kernel; the workspace is read only where this call wrote it.
#include "fa_paged_d256_body.h"

namespace aule_hip {
namespace {

template <class T, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_d256_kernel(const D256Params p) {
    paged_d256_body<T, KV, false>(p, 0.f);   // (the body: fa_paged_d256_body.h)
}

// The combine: workgroup (sixteenth, sequence, KV head, rank) takes four rows of the block the attention kernel's workgroups of that
// (sequence, KV head, rank) wrote, one row per wave: lane k holds split k's {m, l} (nsplit <= 64 = a wave), the weights come from one
// wave reduction, and the partial rows are added in split order with lane x on value columns 4 x .. 4 x + 3 (independent loads: four
// splits are in flight together).  A split with m = -inf weighs nothing; all of them empty gives zeros and lse = -inf.
template <class T>
__global__ void __launch_bounds__(256) fa_paged_d256_combine_kernel(const D256Params p) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bid = (int)blockIdx.x;
    const int sub = bid % kCombineParts, rest = bid / kCombineParts;
    const int units = p.B * p.Hkv;
    const int unit = rest % units, rank = rest / units;
    const int b = unit / p.Hkv, hk = unit - b * p.Hkv;
    const D256Block blk(p, b, rank);
    const int rl = 4 * sub + wave;
    if (rl >= blk.rows) return;
    const int r = blk.r0 + rl;
    const int tok = r / p.g, head = hk * p.g + (r - tok * p.g);
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
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const float* po = p.part_o + orow * kD + 4 * lane;
    for (int k = 0; k < p.nsplit; k += 4) {   // four splits in flight; lanes at or past nsplit hold weight 0
        f32x4_t a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const f32x4_t*>(po + (long long)min(k + i, p.nsplit - 1) * p.rows_total * kD);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float w = __shfl(wk, k + i, 64);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] += w == 0.f ? 0.f : w * a[i][e];
        }
    }
    const float inv = ls > 0.f ? 1.f / ls : 0.f;
    *reinterpret_cast<u32x2_t*>(p.o + (orow * kD + 4 * lane) * 2) = u32x2_t{T::pack2(acc[0] * inv, acc[1] * inv), T::pack2(acc[2] * inv, acc[3] * inv)};
    if (p.lse != nullptr && lane == 0) p.lse[orow] = ls > 0.f ? (mm + fast_log2(ls)) * kLn2 : -__builtin_inff();
}

}  // namespace

// The launch plan.  Row blocks from the longest sequence the grid is sized for; nsplit covers the device's compute units with
// row_blocks * Hkv * B * nsplit workgroups (one workgroup per compute unit: 103 KB of LDS), at most kPagedD256MaxSplit and at most one
// split per 128 keys a block can see (a split is worth a launch slot only with two tiles to read) -- the table's capacity, or the window
// plus the block's token span when a window is set.
PagedD256Plan paged_d256_plan(const PagedD256Args& a, int force_nsplit) {
    if (a.T <= 0 || a.B <= 0 || a.Hq <= 0 || a.Hkv <= 0 || a.Hq % a.Hkv != 0 || a.max_seqlen_q <= 0 || a.block_size <= 0 || a.max_blocks <= 0)
        return PagedD256Plan();
    const long long g = a.Hq / a.Hkv;
    const long long sq = a.cu_seqlens_q == nullptr ? 1 : seqlen_cut(a.max_seqlen_q, a.T);
    const long long rb = (sq * g + kRows - 1) / kRows;
    long long keys = (long long)a.block_size * a.max_blocks;
    if (a.window > 0) {
        const long long span = (kRows + g - 1) / g < sq ? (kRows + g - 1) / g : sq;   // tokens of a block
        if ((long long)a.window + span < keys) keys = (long long)a.window + span;
    }
    const long long most = keys / (2 * kKeys);
    const long long base = rb * a.Hkv * a.B;
    long long ns = force_nsplit;
    if (ns <= 0) {
        ns = (device_cu_count(a.device) + base - 1) / base;
        if (ns > most) ns = most;
    }
    if (ns > kPagedD256MaxSplit) ns = kPagedD256MaxSplit;
    if (ns < 1) ns = 1;
    PagedD256Plan plan;
    plan.row_blocks = (int)rb;
    plan.rows_per_block = kRows;
    plan.nsplit = (int)ns;
    plan.grid = base * ns;
    plan.ws_bytes = ns > 1 ? ((uint64_t)ns * (uint64_t)a.T * (uint64_t)a.Hq * kPagedD256PartFloats * 4 + 15) & ~15ull : 0;
    return plan;
}

// (the one statement of the argument rules and of the parameter block: the plain launch below and the capped one's,
// fa_fwd_paged_d256_softcap_gfx950.hip)
int paged_d256_params(const PagedD256Args& a, const PagedD256Plan& plan, void* ws, D256Params& p) {
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (a.cache_kind != kCache16 && !fp8) return -1;
    if (fp8 ? (a.k_scale == nullptr || a.v_scale == nullptr) : (a.k_scale != nullptr || a.v_scale != nullptr)) return -1;
    if (a.T <= 0 || a.B <= 0 || a.Hkv <= 0 || a.Hq <= 0 || a.Hq % a.Hkv != 0 || a.block_size <= 0 || a.max_blocks <= 0) return -1;
    if ((long long)a.block_size * a.max_blocks >= (1ll << 30)) return -1;
    if (a.q_token_stride < (long long)a.Hq * kD || a.q_token_stride % 8 != 0) return -1;
    if (a.cu_seqlens_q == nullptr && a.T < a.B) return -1;
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll || plan.nsplit < 1 || plan.nsplit > kPagedD256MaxSplit || plan.row_blocks < 1) return -1;
    if (plan.grid != (long long)plan.row_blocks * plan.nsplit * a.Hkv * a.B) return -1;
    if ((long long)plan.row_blocks * a.Hkv * a.B * kCombineParts > 0x7fffffffll) return -1;   // (the combine's grid)
    if (((long long)a.T + kRows) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;   // the kernels count packed rows in 32 bits
    if (plan.nsplit > 1 && (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)) return -1;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k_cache); p.v = static_cast<const char*>(a.v_cache);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    p.rows_total = (long long)a.T * a.Hq;
    p.part_o = plan.nsplit > 1 ? static_cast<float*>(ws) : nullptr;
    p.part_ml = plan.nsplit > 1 ? p.part_o + (long long)plan.nsplit * p.rows_total * kD : nullptr;
    p.table = a.block_tables; p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.q_stride = a.q_token_stride;
    p.T = a.T; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv;
    p.max_blocks = a.max_blocks;
    p.max_sq = a.cu_seqlens_q == nullptr ? 1 : seqlen_cut(a.max_seqlen_q, a.T);
    p.row_blocks = plan.row_blocks; p.nsplit = plan.nsplit;
    p.window = a.window > 0 ? a.window : 0;
    p.c = a.scale * kLog2e;
    return 0;
}

int launch_paged_d256_combine(const D256Params& p, int dtype, hipStream_t stream) {
    const long long combine_grid = (long long)p.row_blocks * p.Hkv * p.B * kCombineParts;   // (< 2^31: paged_d256_params)
    return dispatch_16bit(dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_paged_d256_combine_kernel<decltype(t)>), dim3((unsigned)combine_grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

int launch_paged_d256(const PagedD256Args& a, const PagedD256Plan& plan, void* ws, hipStream_t stream) {
    D256Params p(a.block_size);
    if (paged_d256_params(a, plan, ws, p) != 0) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    int rc = dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (fp8) hipLaunchKernelGGL((fa_fwd_paged_d256_kernel<T, KvFp8>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_paged_d256_kernel<T, Kv16>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_paged_d256_combine(p, a.dtype, stream);
}

}  // namespace aule_hip
