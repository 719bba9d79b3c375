// fa_mla_indexer_fp8mma_gfx950.hip -- the index logits of the sparse MLA's indexer with e4m3 queries over the e4m3 index-key cache,
// the products on FP8 matrix instructions (the contract is aule_mla_indexer_logits_fp8mma_desc in include/aule.h).
//
//   I[t, s] = ks[row(s)] * sum_h (w[t, h] * qs[t, h]) * relu(sum_d qc[t, h, d] * kc[row(s), d])
//
// No element is ever scaled: a token's weights take its query scales once, when they are loaded, and a key's scale multiplies the
// finished sum (relu commutes with a positive factor).  The clamps, the visibility rule (j <= p), the -inf columns and the rows that
// are never written are fa_mla_indexer_gfx950.hip's, through the same fa_device.h helpers; the grid is its plan rule with this
// kernel's tokens per work item (mla_indexer_fp8mma_plan below).
//
// PRODUCTS.  v_mfma_scale_f32_32x32x64_f8f6f4, e4m3 x e4m3, both block scales 1.0, the HEADS as rows (A: the query codes, 32 heads per
// accumulator, two accumulators for H > 32) and the KEYS as columns (B: 32 keys per tile).  Lane (l, half h) of either operand holds
// bytes 64 g + 32 h .. + 31 of its row for instruction g < 2, so the instruction's internal k order cancels (the rule of the other
// two fp8mma kernels).  The 128-wide reduction is 2 instructions per accumulator; the result layout is the 16-bit kernel's (register
// r of half h: head crow(r, h)), and so is the epilogue: relu, weight and head sum as in-lane v_max / v_fma over the accumulator
// registers in one fixed order, the lane halves met by one cross-lane add.  A token's operands are 16 + 16 dwords of codes and 32
// weights: half the 16-bit kernel's query registers.
//
// Work item (sequence b, group of kGroup tokens, chunk of chunk_keys keys), 4 waves.  kGroup is a compile-time constant, 4 or 8: one
// or two tokens per wave.  At 8 and H > 32 the compile misses this kernel's rule (no spill: 216 VGPRs and 20 SGPRs spilled to lanes);
// at H = 32, where both fit, 8 was timed and is slower on every leg that is not launch-bound.  The shipped value is
// 4 (148 VGPRs, three waves per SIMD); the two-token path is compiled only by that A/B build and is not tested.
//   * SEVERAL live tokens: wave w owns token w (and w + 4) of the group.  The K tile is 128 keys of RAW codes, staged once in LDS for
//     the four waves with its 128 row scales beside it, the next tile's rows held in registers meanwhile.  A wave reads a 32-key B
//     operand from LDS ONCE for all its tokens and both head blocks.  The epilogue is NOT hidden under MFMAs: as compiled (H > 32), each
//     32-key tile is a basic block of its own (the kstop / visibility / store branches separate the tiles), both head blocks use one
//     accumulator, and the order is 2 MFMAs, a stall, 32 v_max (the relu is a canonicalising max plus the max with 0), a chain of 16
//     fused multiply-adds of which 15 overlap the second block's first MFMA, then that block's second MFMA, a stall and a fully exposed
//     epilogue.  What covers it is the other waves of the SIMD (three per SIMD).  A pipeline over the 32-key tiles with two live
//     accumulator sets and the branches hoisted was not built.
//       128 keys and one buffer, not 64 and two: at 128 bytes a row the tile is 18 KB, the barrier pair comes once per 128 keys (half
//       as often as in the 16-bit kernel), and the global latency is already hidden by the register prefetch, which a second LDS
//       buffer would not shorten; two workgroups per compute unit-SIMD cover each other's barriers.
//       LDS pitch 144 bytes = 9 sixteen-byte slots.  The B operand is read as two ds_read_b128 per instruction g at row * 144 +
//       64 g + 32 h (+ 16); a ds_read_b128 is served 16 lanes at a time, rows l .. l + 15 of one column: their slots are 9 l mod 16,
//       sixteen different ones, so all 64 banks are hit once -- an odd slot count is what makes that so, and 9 is the smallest one.
//   * ONE live token (decode, the odd last token of a group): the four waves share the token and take DIFFERENT 32-key tiles, each
//     lane reading its key's 128-byte row straight from the cache as the B operand.  No LDS, no barrier.
// The epilogue stays on single-issue fp32 forms: packed fp32 arithmetic runs slower beside a SIMD's MFMA stream (tools/probe_issue.hip),
// and there is no packed max.  No workspace, no atomics; every column of an owned row is written by exactly one item.
#include "fa_device.h"
#include "fa_kernels.h"
#include "fa_mla_indexer.h"

namespace aule_hip {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr int kD = 128;                  // index head width = bytes of a row of codes
constexpr int kG = kD / 64;              // MFMAs per accumulator
#ifndef AULE_IDX_FP8MMA_GROUP
#define AULE_IDX_FP8MMA_GROUP 4          // (8: the A/B build timed at H = 32)
#endif
constexpr int kGroup = AULE_IDX_FP8MMA_GROUP;   // tokens per work item (4: one per wave; 8: two per wave)
constexpr int kSub = 32;                 // keys per MFMA tile
constexpr int kTile = 128;               // keys per staged LDS tile
constexpr int kPitch = kD + 16;          // LDS pitch: 9 slots of 16 bytes (header comment)
static_assert(kGroup == 4 || kGroup == 8, "one or two tokens per wave");

// e4m3 x e4m3 with both E8M0 block scales 127 (1.0) in every byte of the scale registers
__device__ __forceinline__ f32x16_t mfma_fp8(i32x8_t a, i32x8_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

__device__ __forceinline__ i32x8_t join(u32x4_t a, u32x4_t b) {
    return i32x8_t{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}
// 32 bytes at p (16-byte aligned) as one operand; absent: zeros, nothing read
__device__ __forceinline__ i32x8_t row32(const char* p, bool there) {
    if (!there) return i32x8_t{};
    return join(*reinterpret_cast<const u32x4_t*>(p), *reinterpret_cast<const u32x4_t*>(p + 16));
}

// the cache row of position j of the sequence whose table row is `tab` (j < L_b); the entry is clamped into the cache
__device__ __forceinline__ long long cache_row(const IdxParams& p, const int* tab, int j) {
    const int lb = block_of(j, p.bs, p.bs_shift);
    const unsigned blk = min((unsigned)tab[lb], (unsigned)(p.nb - 1));
    return (long long)blk * p.bs + (j - lb * p.bs);
}

// A token's operands: the codes of head (lane & 31) + 32 hb, bytes 64 g + 32 hi .. + 31, and the weights (times the query scales) of
// the heads whose scores this lane's accumulator registers hold.  Heads at or past H: zeros, never read.
struct Fp8Token {
    i32x8_t qf[2][kG];
    float w[2][16];
    __device__ __forceinline__ void load(const IdxParams& p, const float* qs, long long row, int l31, int hi) {
        const char* qrow = p.q + row * p.q_stride;
        const float* wrow = p.w + row * p.H;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int head = l31 + 32 * hb;
#pragma unroll
            for (int g = 0; g < kG; ++g) qf[hb][g] = row32(qrow + head * kD + 64 * g + 32 * hi, head < p.H);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int h = crow(r, hi) + 32 * hb;
                w[hb][r] = h < p.H ? (qs != nullptr ? wrow[h] * qs[row * p.H + h] : wrow[h]) : 0.f;
            }
        }
    }
};

// the scores of 32 keys (B operand kf) for the token's heads 32 hb ..
__device__ __forceinline__ f32x16_t scores(const Fp8Token& t, int hb, const i32x8_t (&kf)[kG]) {
    f32x16_t a = {};
#pragma unroll
    for (int g = 0; g < kG; ++g) a = mfma_fp8(t.qf[hb][g], kf[g], a);
    return a;
}
// relu, weight and sum over the 32 heads of block hb of this lane's key, onto s.  One fixed order of operations for every path: block
// 0 then block 1, registers in order, then the two lane halves (s + xhalf(s)).
__device__ __forceinline__ float head_sum(const Fp8Token& t, int hb, const f32x16_t& a, float s) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s = __builtin_fmaf(fmaxf(a[r], 0.f), t.w[hb][r], s);
    return s;
}

template <int GROUP, bool two>
__global__ void __launch_bounds__(256, 2) fa_mla_indexer_logits_fp8mma_kernel(const IdxParams p, const float* qs) {
    constexpr int TW = GROUP / 4;   // tokens per wave
    __shared__ __attribute__((aligned(16))) char Ks[kTile * kPitch];
    __shared__ float Ss[kTile];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int chunk = bid % p.chunks, rest = bid / p.chunks;
    const int grp = rest % p.groups, b = rest / p.groups;

    // aule_mla_paged_desc's clamps (fa_device.h): L_b, s_b, n_b
    const int L = seq_len(p.ctx, b, p.W);
    const SeqRange own_rows = seq_range_or_row(p.cu, b, p.T, p.max_sq);   // (a null cu: b < T, the host checks)
    const int s = own_rows.s, n = own_rows.n;
    const int i0 = grp * GROUP;
    const int live = min(GROUP, n - i0);
    if (live <= 0) return;
    const int kbeg = chunk * p.chunk_keys;
    const int kstop = min(kbeg + p.chunk_keys, p.W);                 // columns this item writes
    const int kend = min(kstop, L - n + i0 + live);                  // keys this item reads: up to its last token's position
    const int* tab = p.table + (long long)b * p.max_blocks;
    const float ninf = -__builtin_inff();

    if (live == 1) {
        // one token, the waves on different tiles, the B operand straight from the cache
        const int pos = L - n + i0;
        float* orow = p.out + (long long)(s + i0) * p.out_stride;
        Fp8Token tk;
        if (kbeg < kend) tk.load(p, qs, s + i0, l31, hi);
        for (int j0 = kbeg + kSub * wave; j0 < kstop; j0 += kSub * 4) {
            const int j = j0 + l31;
            float v = ninf;
            if (j0 < kend) {
                const bool vis = j <= pos;
                const long long at = vis ? cache_row(p, tab, j) : 0;
                i32x8_t kf[kG];
#pragma unroll
                for (int g = 0; g < kG; ++g) kf[g] = row32(p.k + at * kD + 64 * g + 32 * hi, vis);
                float sum = 0.f;
#pragma unroll
                for (int hb = 0; hb < (two ? 2 : 1); ++hb) sum = head_sum(tk, hb, scores(tk, hb, kf), sum);
                sum += xhalf(sum);
                if (vis) v = sum * p.ks[at];
            }
            if (hi == 0 && j < kstop) orow[j] = v;
        }
        return;
    }

    // several tokens: wave w owns tokens i0 + w (+ 4), the K tile staged once for all of them
    Fp8Token tk[TW];
    int pos[TW];
    bool alive[TW];
    float* orow[TW];
#pragma unroll
    for (int u = 0; u < TW; ++u) {
        const int ti = wave + 4 * u;
        alive[u] = ti < live;
        pos[u] = L - n + i0 + ti;
        orow[u] = p.out + (long long)(s + i0 + min(ti, live - 1)) * p.out_stride;
        if (alive[u] && kbeg <= pos[u]) tk[u].load(p, qs, s + i0 + ti, l31, hi);
    }

    // thread t stages 16-byte chunks (t & 3) + 4 i of tile rows (t >> 2) + 64 r
    const int srow = tid >> 2, sc0 = tid & 3;
    u32x4_t d[2][2];
    float dscale[2] = {0.f, 0.f};
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = k0 + srow + 64 * r;
            const bool ok = j < kend;
            const long long at = ok ? cache_row(p, tab, j) : 0;
#pragma unroll
            for (int i = 0; i < 2; ++i) d[r][i] = ok ? *reinterpret_cast<const u32x4_t*>(p.k + at * kD + (sc0 + 4 * i) * 16) : u32x4_t{};
            dscale[r] = ok && sc0 == 0 ? p.ks[at] : 0.f;
        }
    };
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kstop; k0 += kTile) {
        if (k0 < kend) {   // (uniform over the workgroup)
            __syncthreads();   // every wave is done with the previous tile
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4_t*>(Ks + (srow + 64 * r) * kPitch + (sc0 + 4 * i) * 16) = d[r][i];
                if (sc0 == 0) Ss[srow + 64 * r] = dscale[r];
            }
            __syncthreads();
            if (k0 + kTile < kend) fetch(k0 + kTile);
        }
        if (!alive[0]) continue;   // (token w + 4 is live only if token w is)
#pragma unroll
        for (int kk = 0; kk < kTile / kSub; ++kk) {
            const int j0 = k0 + kSub * kk, j = j0 + l31;
            if (j0 >= kstop) break;
            // (uniform over the wave; j0 <= pos < kend: the tile is staged)
            bool need[TW], any = false;
#pragma unroll
            for (int u = 0; u < TW; ++u) {
                need[u] = alive[u] && j0 <= pos[u];
                any = any || need[u];
            }
            float sum[TW] = {};
            float ksc = 0.f;
            if (any) {
                i32x8_t kf[kG];
                const char* krow = Ks + (kSub * kk + l31) * kPitch + 32 * hi;
#pragma unroll
                for (int g = 0; g < kG; ++g) kf[g] = row32(krow + 64 * g, true);
                ksc = Ss[kSub * kk + l31];
                // per block of 32 heads: the MFMAs of every token that sees the tile, then their epilogues
#pragma unroll
                for (int hb = 0; hb < (two ? 2 : 1); ++hb) {
                    f32x16_t a[TW];
#pragma unroll
                    for (int u = 0; u < TW; ++u)
                        if (need[u]) a[u] = scores(tk[u], hb, kf);
#pragma unroll
                    for (int u = 0; u < TW; ++u)
                        if (need[u]) sum[u] = head_sum(tk[u], hb, a[u], sum[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < TW; ++u) {
                if (!alive[u]) continue;
                float v = ninf;
                if (need[u] && j <= pos[u]) v = (sum[u] + xhalf(sum[u])) * ksc;
                if (hi == 0 && j < kstop) orow[u][j] = v;
            }
        }
    }
}

}  // namespace

MlaIndexerPlan mla_indexer_fp8mma_plan(int B, int max_seqlen_q, long long W, int device) {
    return mla_indexer_plan_grouped(B, max_seqlen_q, W, device, kGroup);
}

int launch_mla_indexer_logits_fp8mma(const MlaIndexerArgs& a, const MlaIndexerPlan& plan, hipStream_t stream) {
    IdxParams p;
    if (mla_indexer_params(a, plan, p) != 0) return -1;
    if (a.cache_kind != kCacheFp8E4M3 || a.q_token_stride % 16 != 0 || plan.group_tokens != kGroup) return -1;
    if (a.H > 32) hipLaunchKernelGGL((fa_mla_indexer_logits_fp8mma_kernel<kGroup, true>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p, a.q_scale);
    else hipLaunchKernelGGL((fa_mla_indexer_logits_fp8mma_kernel<kGroup, false>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p, a.q_scale);
    return (int)hipGetLastError();
}

}  // namespace aule_hip
