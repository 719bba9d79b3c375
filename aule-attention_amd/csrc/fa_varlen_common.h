// fa_varlen_common.h -- what the variable-length kernels share (fa_fwd_varlen_gfx950.hip, fa_bwd_varlen_gfx950.hip):
// the LDS pitches per head_dim, a tile of rows on its way from global memory to LDS, and the work
// decomposition and K / V tile source of the forward and the dQ kernel (QueryBlock, KeyTiles), and the dQ kernel's body
// (ragged_dq_body), which the MLA 192 / 128 backward runs too.  The body is parameterised by a shape S: widths DQK (q / key rows)
// and DV (value / output rows), the key-tile source S::Tiles(p, x, hk) with load(k0, tid) and store(Ks, kpitch, Vs, vpitch, tid),
// and the head counts q_heads(p), kv_heads(p).
// The layout is the plain one of fa_fwd_paged_prefill_gfx950.hip (tile sizes and pitches of fa_paged_tile.h) with a contiguous
// tile source: row kv of a sequence's keys is row s_k + kv of k, k_token_stride elements from one token to the next.
// Device code only.
#pragma once
#include "fa_tile_attention.h"

namespace aule_hip {
namespace {

constexpr int kVQT = 32;    // dK/dV: packed query rows per tile
constexpr int kVKB = 128;   // dK/dV: keys per workgroup

template <int D>
struct VarlenCfg : PrefillCfg<D> {
    // rows read both as ds_read_b128 A operands and transposed (the PAT idea of D256Cfg: an odd number of 16-byte slots on top of
    // the transposed pitch)
    static constexpr int PAT = PrefillCfg<D>::PT + 16;
};

// (the clamp of a sequence's bounds, seq_range: fa_device.h, beside the other clamps of the contract)

// key j < L visible to the query at position pos
__device__ __forceinline__ bool varlen_visible(int pos, int j, int L, bool causal, int window) {
    return j < L && (!causal || j <= pos) && (window <= 0 || pos - j < window);
}

// ROWS rows of D 16-bit elements on their way to LDS: 16-byte chunk i of thread t is chunk t + 256 i of the tile (row
// (t + 256 i) / CPR).  addr(row) is the row's first byte, or nullptr for a row that is not read (zeros in LDS).
template <int D, int ROWS>
struct RowTile {
    static constexpr int CPR = D / 8;
    static constexpr int CH = ROWS * CPR;
    static constexpr int N = (CH + 255) / 256;
    static constexpr bool kWhole = CH % 256 == 0;
    u32x4_t r[N];
    template <class F>
    __device__ __forceinline__ void load(F&& addr, int tid) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int idx = tid + 256 * i;
            u32x4_t x = u32x4_t{};
            if (kWhole || idx < CH) {
                const char* p = addr(idx / CPR);
                if (p != nullptr) x = *reinterpret_cast<const u32x4_t*>(p + (idx % CPR) * 16);
            }
            r[i] = x;
        }
    }
    __device__ __forceinline__ void store(char* lds, int pitch, int tid) const {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int idx = tid + 256 * i;
            if (kWhole || idx < CH) *reinterpret_cast<u32x4_t*>(lds + (idx / CPR) * pitch + (idx % CPR) * 16) = r[i];
        }
    }
};

// The work of one workgroup of the forward and of the dQ kernel -- block `rank` of (sequence b, KV head hk), rank 0 the sequence's last
// (heaviest) block of 128 token-major packed rows -- and this lane's row of it.  P supplies cu_q, cu_k, Tq, Tk, max_sq, max_sk, g,
// causal (0, 1, 2) and window (> 0: on).
struct QueryBlock {
    int sq, n, sk, L;          // the sequence after the clamps: first query row, queries, first key row, keys
    int rows;                  // of the block (0: the sequence has no block of this rank)
    int tok, head, pos;        // this lane's row: token of the sequence, query head, position (a lane past the end works on the block's
    bool live;                 // last row and stores nothing)
    bool causal, wave_live;    // wave-uniform from here on: the wave's position range decides the tiles it computes and the unmasked
    int wpos_lo, wpos_hi;      // path, the block's the tiles that are loaded
    int kbeg, kend, ntiles;    // keys kbeg .. kend - 1 in tiles of 64
    int window;
    // none of the wave's rows sees a key of the tile at k0: all keys after its last position, or all before its window
    __device__ __forceinline__ bool skips(int k0) const {
        return !wave_live || (causal && k0 > wpos_hi) || (window > 0 && k0 + kPK - 1 < (long long)wpos_lo - window + 1);   // (64-bit: positions may be negative)
    }
    // every row of the wave sees every key of the tile at k0
    __device__ __forceinline__ bool sees_all(int k0) const {
        return k0 + kPK <= L && (!causal || k0 + kPK - 1 <= wpos_lo) && (window <= 0 || wpos_hi - k0 < window);
    }
    __device__ __forceinline__ bool visible(int j) const { return varlen_visible(pos, j, L, causal, window); }
};

template <class P>
__device__ __forceinline__ QueryBlock query_block(const P& p, int rank, int b, int hk, int wave, int l31) {
    QueryBlock x;
    const SeqRange q = seq_range(p.cu_q, b, p.Tq, p.max_sq);
    const SeqRange k = seq_range(p.cu_k, b, p.Tk, p.max_sk);
    x.sq = q.s; x.n = q.n; x.sk = k.s; x.L = k.n;
    const int R = x.n * p.g;   // packed rows of this (sequence, KV head); (Tq + 128) g < 2^31: the host checks
    const int own = (R + kPQ - 1) / kPQ;
    x.rows = 0;
    if (rank >= own) return x;
    const int r0 = (own - 1 - rank) * kPQ;
    x.rows = min(kPQ, R - r0);
    const int rl = wave * 32 + l31;
    x.live = rl < x.rows;
    const int r = r0 + min(rl, x.rows - 1);
    x.tok = r / p.g;
    x.head = hk * p.g + r % p.g;
    x.causal = p.causal != 0;
    x.window = p.window;
    const int coff = p.causal == 2 ? x.L - x.n : 0;
    x.pos = x.tok + coff;
    const int bpos_lo = coff + r0 / p.g, bpos_hi = coff + (r0 + x.rows - 1) / p.g;
    x.wave_live = wave * 32 < x.rows;
    x.wpos_lo = coff + (r0 + min(wave * 32, x.rows - 1)) / p.g;
    x.wpos_hi = coff + (r0 + min(wave * 32 + 31, x.rows - 1)) / p.g;
    x.kend = x.causal ? min(x.L, bpos_hi + 1) : x.L;
    x.kbeg = p.window > 0 ? (int)max(0ll, (long long)bpos_lo - p.window + 1) / kPK * kPK : 0;   // (64-bit: bpos_lo may be negative; the result is <= bpos_lo + 1)
    x.ntiles = x.kend > x.kbeg ? (x.kend - x.kbeg + kPK - 1) / kPK : 0;
    return x;
}

// One K and one V tile of 64 keys of sequence rows sk .. on their way to LDS: key row kv (< kend <= L: inside k / v) is at byte
// ((sk + kv) token stride + hk D) 2, 64-bit; rows at or beyond kend are not read.
template <int D>
struct KeyTiles {
    RowTile<D, kPK> k, v;
    const char* kbase;
    const char* vbase;
    long long kpitch, vpitch;
    int kend;
    template <class P>
    __device__ __forceinline__ KeyTiles(const P& p, const QueryBlock& x, int hk)
        : kbase(p.k + ((long long)x.sk * p.k_stride + (long long)hk * D) * 2), vbase(p.v + ((long long)x.sk * p.v_stride + (long long)hk * D) * 2),
          kpitch(p.k_stride * 2), vpitch(p.v_stride * 2), kend(x.kend) {}
    __device__ __forceinline__ void load(int k0, int tid) {
        k.load([&](int row) { return k0 + row < kend ? kbase + (long long)(k0 + row) * kpitch : nullptr; }, tid);
        v.load([&](int row) { return k0 + row < kend ? vbase + (long long)(k0 + row) * vpitch : nullptr; }, tid);
    }
    __device__ __forceinline__ void store(char* Ks, int kp, char* Vs, int vp, int tid) const {
        k.store(Ks, kp, tid);
        v.store(Vs, vp, tid);
    }
};

// The shape of the variable-length kernels: q, k, v rows of D elements, the query heads of a KV head packed together
template <int D>
struct VarlenShape {
    static constexpr int DQK = D, DV = D;
    using Tiles = KeyTiles<D>;
    template <class P>
    static __device__ __forceinline__ int q_heads(const P& p) { return p.Hq; }
    template <class P>
    static __device__ __forceinline__ int kv_heads(const P& p) { return p.Hkv; }
};

// The dQ kernel: the forward's work decomposition and tile walk with Q and dO of the lane's row in registers; K tiles through Ks at
// pitch VarlenCfg<DQK>::PAT (read as b128 rows AND transposed), V tiles through Vs at PrefillCfg<DV>::PA; S^T = K.Q^T,
// dP^T = V.dO^T, dS^T = P^T (dP^T - delta) with P = exp2(S c - L log2 e) on visible keys only, dQ^T[d][q] += K^T.dS^T.
// dq = scale * acc.  P supplies, beside the forward's, dout, lse, delta, dq and scale.
template <class T, class S, class P>
__device__ __forceinline__ void ragged_dq_body(const P& p, char* Ks, char* Vs) {
    constexpr int GQ = S::DQK / 16, GV = S::DV / 16, DT = S::DQK / 32;
    constexpr int KP = VarlenCfg<S::DQK>::PAT, VP = PrefillCfg<S::DV>::PA;
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int units = S::kv_heads(p) * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int hk = unit % S::kv_heads(p), b = unit / S::kv_heads(p);

    const QueryBlock x = query_block(p, rank, b, hk, wave, l31);
    if (x.rows == 0) return;
    const int ntiles = x.ntiles;

    // Q and dO operand chunks of this lane's row, its lse (log2 units) and delta
    const long long orow = ((long long)x.sq + x.tok) * S::q_heads(p) + x.head;
    const char* qrow = p.q + (((long long)x.sq + x.tok) * p.q_stride + (long long)x.head * S::DQK) * 2;
    const char* dorow = p.dout + orow * (long long)(S::DV * 2);
    u32x4_t qf[GQ], of[GV];
#pragma unroll
    for (int g = 0; g < GQ; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);
#pragma unroll
    for (int g = 0; g < GV; ++g) of[g] = *reinterpret_cast<const u32x4_t*>(dorow + 32 * g + 16 * hi);
    const float l2 = p.lse[orow] * kLog2e;
    const float dl = p.delta[orow];

    f32x16_t acc[DT];
#pragma unroll
    for (int i = 0; i < DT; ++i) acc[i] = f32x16_t{};

    typename S::Tiles kt(p, x, hk);
    if (ntiles > 0) kt.load(x.kbeg, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = x.kbeg + t * kPK;
        __syncthreads();
        kt.store(Ks, KP, Vs, VP, tid);
        __syncthreads();
        if (t + 1 < ntiles) kt.load(k0 + kPK, tid);
        if (x.skips(k0)) continue;
        // S^T[key][row] = K.Q^T, dP^T[key][row] = V.dO^T
        f32x16_t s[2], dp[2];
        tile_scores<T, GQ>(s, Ks, KP, qf, l31, hi);
        tile_scores<T, GV>(dp, Vs, VP, of, l31, hi);
        // dS^T = P^T (dP^T - delta), P^T = exp2(S^T c - L log2 e) on visible keys
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int j = k0 + 32 * kk + crow(rr, hi);
                const float pr = x.visible(j) ? fast_exp2(s[kk][rr] * p.c - l2) : 0.f;
                s[kk][rr] = pr * (dp[kk][rr] - dl);
            }
        // dQ^T[d][q] += K^T.dS^T
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t bs = pack_step<T>(s[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) acc[dt] = mfma16<T>(lds_tr_step(Ks, KP, 16 * st, 32 * dt, lane), bs, acc[dt]);
        }
    }
    if (!x.live) return;
    store_row16<T, DT>(p.dq + orow * (long long)(S::DQK * 2), acc, p.scale, hi);
}

}  // namespace
}  // namespace aule_hip
