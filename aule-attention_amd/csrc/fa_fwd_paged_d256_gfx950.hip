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
#include "fa_paged_d256.h"
#include "fa_paged_tile.h"

namespace aule_hip {
namespace {

constexpr int kD = 256;
using C256 = PrefillCfg<kD>;
constexpr int kKeys = kPK;                          // keys per tile: 64
constexpr int kRows = kPagedD256Rows;
constexpr int kHalfBytes = C256::RB / 2;             // a wave's half of a 16-bit row
constexpr int kHalfG = C256::G / 2;                  // ... in operand chunk pairs: 8
constexpr int kHalfDT = C256::DT / 2;                // O accumulators of a wave's half of the value columns: 4
constexpr int kLdsK = kKeys * C256::PA;              // 33 792
constexpr int kLdsV = kKeys * C256::PT;              // 36 864
constexpr int kLdsScores = 4 * 8 * 1024;            // partial scores: [wave][register quad][lane] 16 bytes
constexpr int kCombineParts = kRows / 4;            // combine workgroups per row block: four rows each, one per wave
static_assert(kPagedD256MaxSplit <= 64, "a lane per split");

struct D256Params {
    const char* q;
    const char* k;
    const char* v;
    char* o;
    float* lse;
    float* part_o;    // nsplit > 1: [nsplit][T * Hq][256]
    float* part_ml;   //             [nsplit][T * Hq][2]
    const int* table;
    const int* ctx;
    const int* cu;    // null: sequence b owns row b
    const float* k_scale;
    const float* v_scale;
    long long q_stride;
    long long rows_total;   // T * Hq
    int T, B, Hq, Hkv, g;
    int bs, bs_shift;       // bs_shift >= 0: bs = 1 << bs_shift
    int max_blocks, max_sq;
    int row_blocks, nsplit;
    int window;             // > 0: on
    float c;
    // (the block size and the shift block_of takes are stated together)
    explicit D256Params(int block_size) : bs(block_size), bs_shift(shift_of(block_size)) {}
};

// what both kernels derive for (sequence b, rank): the clamps of the contract and the block of packed rows of ONE KV head
struct D256Block {
    int L, s, n;
    int r0, rows;   // rows == 0: nothing to do
    __device__ __forceinline__ D256Block(const D256Params& p, int b, int rank) {
        L = seq_len(p.ctx, b, p.max_blocks * p.bs);   // (the capacity < 2^30: the host checks)
        const SeqRange q = seq_range_or_row(p.cu, b, p.T, p.max_sq);   // (a null cu: b < T, the host checks)
        s = q.s;
        n = q.n;
        const int R = n * p.g;   // (T + 64) * g < 2^31: the host checks
        const int own = (R + kRows - 1) / kRows;
        r0 = 0;
        rows = 0;
        if (rank < own) {
            r0 = (own - 1 - rank) * kRows;   // rank 0 is the sequence's last block, as in the paged prefill
            rows = min(kRows, R - r0);
        }
    }
};

template <class T, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_d256_kernel(const D256Params p) {
    constexpr bool FP8 = std::is_same<KV, KvFp8>::value;
    __shared__ __attribute__((aligned(16))) char Ks[kLdsK];
    __shared__ __attribute__((aligned(16))) char Vs[kLdsV];
    __shared__ __attribute__((aligned(16))) char Xs[kLdsScores];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rh = wave & 1, ch = wave >> 1;
    // work item: (split, rank, sequence, KV head), the KV heads of a sequence side by side
    const int bid = (int)blockIdx.x;
    const int units = p.B * p.Hkv;
    const int unit = bid % units, rest = bid / units;
    const int b = unit / p.Hkv, hk = unit - b * p.Hkv;
    const int rank = rest % p.row_blocks, split = rest / p.row_blocks;

    const D256Block blk(p, b, rank);
    if (blk.rows == 0) return;
    const int L = blk.L, n = blk.n, r0 = blk.r0, rows = blk.rows;

    // this lane's row (a lane past the end works on the block's last row and stores nothing)
    const int rl = rh * 32 + l31;
    const bool live = rl < rows;
    const int r = r0 + min(rl, rows - 1);
    const int tok = r / p.g, head = hk * p.g + (r - tok * p.g);
    const int pos = L - n + tok;
    // wave-uniform position ranges: the block's decide the tiles, the wave's the tiles it computes and the unmasked path
    const int bpos_lo = L - n + r0 / p.g, bpos_hi = L - n + (r0 + rows - 1) / p.g;
    const bool wave_live = rh * 32 < rows;
    const int wpos_lo = L - n + (r0 + min(rh * 32, rows - 1)) / p.g;
    const int wpos_hi = L - n + (r0 + min(rh * 32 + 31, rows - 1)) / p.g;

    // the block's visible keys [vbeg, vend) (vend <= L: the last token sits at L - 1), their tiles [tb, te), and this split's share
    const int vend = bpos_hi + 1;
    const int vbeg = p.window > 0 ? max(0, bpos_lo - p.window + 1) : 0;
    const int tb = vbeg / kKeys;
    const int te = vend > vbeg ? (vend + kKeys - 1) / kKeys : tb;
    const int per = (te - tb + p.nsplit - 1) / p.nsplit;
    const int kbeg = (tb + split * per) * kKeys;
    const int kend = min(min(tb + (split + 1) * per, te) * kKeys, vend);
    const int ntiles = kend > kbeg ? (kend - kbeg + kKeys - 1) / kKeys : 0;
    const int* tab = p.table + (long long)b * p.max_blocks;

    // Q operand chunks of this lane's row, the wave's half of the reduction
    const char* qrow = p.q + (((long long)blk.s + tok) * p.q_stride + (long long)head * kD) * 2 + ch * kHalfBytes;
    u32x4_t qf[kHalfG];
#pragma unroll
    for (int g = 0; g < kHalfG; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    // An FP8 cache's scales are never applied per element: k_scale multiplies the score scale here, v_scale the accumulators on their
    // way out; vs is 1.0f for a 16-bit cache, where the product is exact.
    float c = p.c, vs = 1.0f;
    if constexpr (FP8) {
        c *= p.k_scale[hk];
        vs = p.v_scale[hk];
    }

    f32x16_t o[kHalfDT];
#pragma unroll
    for (int i = 0; i < kHalfDT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    PagedTile<T, kD, FP8> kt;
    if (ntiles > 0) {
        kt.lookup(p, tab, kbeg, kend, tid);
        kt.load(p, hk, kbeg, kend, tid);
        kt.lookup(p, tab, kbeg + kKeys, kend, tid);
    }
    char* xmine = Xs + wave * 8192 + lane * 16;
    const char* xother = Xs + (wave ^ 2) * 8192 + lane * 16;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kKeys;
        __syncthreads();   // every wave is done with the previous tile and the previous partial scores
        kt.store(Ks, Vs, tid);
        __syncthreads();
        if (t + 1 < ntiles) {
            kt.load(p, hk, k0 + kKeys, kend, tid);
            kt.lookup(p, tab, k0 + 2 * kKeys, kend, tid);
        }
        // a wave computes the tiles some row of it sees: not those after its last position, not those before its window.  Both waves
        // of a row half decide alike, so the exchange below always has its two sides.
        const bool work = wave_live && k0 <= wpos_hi && !(p.window > 0 && k0 + kKeys - 1 < wpos_lo - p.window + 1);
        // partial S^T[key][row] over the wave's 128 elements
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
        if (work) {
            const char* kimg = Ks + l31 * C256::PA + ch * kHalfBytes + 16 * hi;
#pragma unroll
            for (int g = 0; g < kHalfG; ++g)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) sc[kk] = mfma16<T>(lds_b128(kimg + 32 * kk * C256::PA + 32 * g), qf[g], sc[kk]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    *reinterpret_cast<f32x4_t*>(xmine + (4 * kk + q4) * 1024) = f32x4_t{sc[kk][4 * q4], sc[kk][4 * q4 + 1], sc[kk][4 * q4 + 2], sc[kk][4 * q4 + 3]};
        }
        __syncthreads();
        if (!work) continue;
        // own + other, scale to log2 units, mask, running max over the lane pair (lanes l and l + 32 hold the same row)
        float mx = -__builtin_inff();
        // every row of the wave sees every key of the tile
        const bool full = k0 + kKeys - 1 <= wpos_lo && k0 + kKeys <= kend && (p.window <= 0 || wpos_hi - k0 < p.window);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const f32x4_t y = *reinterpret_cast<const f32x4_t*>(xother + (4 * kk + q4) * 1024);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = 4 * q4 + i;
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const bool see = full || (j <= pos && j < kend && (p.window <= 0 || pos - j < p.window));
                    const float x = see ? (sc[kk][rr] + y[i]) * c : -__builtin_inff();
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
                }
            }
        mx = fmaxf(mx, xhalf(mx));
        const float mn = fmaxf(m, mx);
        const float top = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(m - top);   // m = -inf: 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < kHalfDT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - top);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T over the wave's 128 value columns
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < kHalfDT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, C256::PT, 16 * st, 128 * ch + 32 * dt, lane), pb, o[dt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    l += xhalf(l);
    if (!live) return;
    const long long orow = ((long long)blk.s + tok) * p.Hq + head;
    if (p.nsplit > 1) {
        const long long prow = (long long)split * p.rows_total + orow;
        float* po = p.part_o + prow * kD + 128 * ch;
#pragma unroll
        for (int dt = 0; dt < kHalfDT; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<f32x4_t*>(po + 32 * dt + 8 * g4 + 4 * hi) =
                    f32x4_t{o[dt][4 * g4] * vs, o[dt][4 * g4 + 1] * vs, o[dt][4 * g4 + 2] * vs, o[dt][4 * g4 + 3] * vs};
        if (ch == 0 && hi == 0) *reinterpret_cast<f32x2_t*>(p.part_ml + prow * 2) = f32x2_t{m, l};
        return;
    }
    const float inv = (l > 0.f ? 1.f / l : 0.f) * vs;
    char* og = p.o + (orow * kD + 128 * ch) * 2;
#pragma unroll
    for (int dt = 0; dt < kHalfDT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && ch == 0 && hi == 0) {
        const float top = m == -__builtin_inff() ? 0.f : m;
        p.lse[orow] = l > 0.f ? (top + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
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

int launch_paged_d256(const PagedD256Args& a, const PagedD256Plan& plan, void* ws, hipStream_t stream) {
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (a.cache_kind != kCache16 && !fp8) return -1;
    if (fp8 ? (a.k_scale == nullptr || a.v_scale == nullptr) : (a.k_scale != nullptr || a.v_scale != nullptr)) return -1;
    if (a.T <= 0 || a.B <= 0 || a.Hkv <= 0 || a.Hq <= 0 || a.Hq % a.Hkv != 0 || a.block_size <= 0 || a.max_blocks <= 0) return -1;
    if ((long long)a.block_size * a.max_blocks >= (1ll << 30)) return -1;
    if (a.q_token_stride < (long long)a.Hq * kD || a.q_token_stride % 8 != 0) return -1;
    if (a.cu_seqlens_q == nullptr && a.T < a.B) return -1;
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll || plan.nsplit < 1 || plan.nsplit > kPagedD256MaxSplit || plan.row_blocks < 1) return -1;
    if (plan.grid != (long long)plan.row_blocks * plan.nsplit * a.Hkv * a.B) return -1;
    const long long combine_grid = (long long)plan.row_blocks * a.Hkv * a.B * kCombineParts;
    if (combine_grid > 0x7fffffffll) return -1;
    if (((long long)a.T + kRows) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;   // the kernels count packed rows in 32 bits
    if (plan.nsplit > 1 && (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)) return -1;
    D256Params p(a.block_size);
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
    int rc = dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (fp8) hipLaunchKernelGGL((fa_fwd_paged_d256_kernel<T, KvFp8>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_paged_d256_kernel<T, Kv16>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
    if (rc != 0 || plan.nsplit == 1) return rc;
    return dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_paged_d256_combine_kernel<decltype(t)>), dim3((unsigned)combine_grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
