// fa_paged_d256_body.h -- the body of the paged attention kernel at head_dim 256, once for the plain kernel (kCap = false:
// fa_fwd_paged_d256_gfx950.hip, whose header describes the layout) and the soft-capped one (kCap = true:
// fa_fwd_paged_d256_softcap_gfx950.hip), with the parameter block both read and the host functions the plain file
// exports to the capped one: the one fill of the block and the launch of the combine kernel, which is instantiated once.
// Capped, p.c is ci and `cc` the cap in log2 units (fa_softcap.h); plain, `cc` is not read.
#pragma once
#include "fa_paged_d256.h"
#include "fa_paged_tile.h"
#include "fa_softcap.h"

namespace aule_hip {

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


// -1: unsupported arguments; else `p` holds the launch's parameters (`ws` as launch_paged_d256's)
int paged_d256_params(const PagedD256Args& a, const PagedD256Plan& plan, void* ws, D256Params& p);
// the combine of a launch with p.nsplit > 1 (`p` from paged_d256_params): one wave per row adds the partials in split order
int launch_paged_d256_combine(const D256Params& p, int dtype, hipStream_t stream);

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

template <class T, class KV, bool kCap>
__device__ __forceinline__ void paged_d256_body(const D256Params p, const float cc) {
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

    // An FP8 cache's scales are never applied per element: k_scale multiplies the score scale here (capped: ci, so it ends up inside the
    // tanh), v_scale the accumulators on their way out; vs is 1.0f for a 16-bit cache, where the product is exact.
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
        // own + other, scale to log2 units (capped: through the tanh), mask, running max over the lane pair (lanes l and l + 32 hold the same row)
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
                    const float x = see ? score_log2<kCap>(sc[kk][rr] + y[i], c, cc) : -__builtin_inff();
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

}  // namespace
}  // namespace aule_hip
