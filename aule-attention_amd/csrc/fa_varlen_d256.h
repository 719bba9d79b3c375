// fa_varlen_d256.h -- what the head_dim 256 variable-length kernels share (fa_fwd_varlen_d256_gfx950.hip, fa_bwd_varlen_d256_gfx950.hip;
// DESIGN.md 3.21): the parameter block the kernels read and the one place that fills it from VarlenArgs.  The decomposition, the
// clamps, the tile source and the mask predicates are fa_varlen_common.h's; the pitches PrefillCfg<256> (PA 528, PT 576) and
// VarlenCfg<256>::PAT = D256Cfg::PAT (592).
#pragma once
#include "fa_kernels.h"
#include "fa_varlen_common.h"
#include "fa_softcap.h"

namespace aule_hip {
namespace {

constexpr int kVD = 256;
using CV256 = VarlenCfg<kVD>;
static_assert(CV256::PA == 528 && CV256::PT == 576 && CV256::PAT == D256Cfg<Bf16Traits>::PAT, "the pitches of the 256-wide kernels");

struct VarlenD256Params {
    const char* q;
    const char* k;
    const char* v;
    char* o;              // forward: written
    float* lse_out;       // forward: written (null: skipped)
    const char* dout;     // backward from here on
    const float* lse;
    const float* delta;
    char* dq;
    char* dk;
    char* dv;
    const int* cu_q;
    const int* cu_k;
    long long q_stride, k_stride, v_stride;   // elements between tokens
    int Tq, Tk, B, Hq, Hkv, g;
    int max_sq, max_sk;
    float c;       // scale * log2(e)
    float scale;
    int causal;    // 0, 1, 2
    int window;    // > 0: on
};

// (`a` passed varlen_args_ok)
inline VarlenD256Params varlen_d256_params(const VarlenArgs& a) {
    VarlenD256Params p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k); p.v = static_cast<const char*>(a.v);
    p.o = static_cast<char*>(a.out); p.lse_out = a.lse;
    p.dout = static_cast<const char*>(a.dout); p.lse = a.lse; p.delta = a.delta;
    p.dq = static_cast<char*>(a.dq); p.dk = static_cast<char*>(a.dk); p.dv = static_cast<char*>(a.dv);
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k;
    p.q_stride = a.q_token_stride; p.k_stride = a.k_token_stride; p.v_stride = a.v_token_stride;
    p.Tq = a.Tq; p.Tk = a.Tk; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv;
    p.max_sq = varlen_max_sq(a);
    p.max_sk = varlen_max_sk(a);
    p.c = a.scale * kLog2e;
    p.scale = a.scale;
    p.causal = a.causal;
    p.window = varlen_window(a);
    return p;
}

// The forward's and the dK / dV kernel's bodies, once for the plain kernels (kCap = false: fa_fwd_varlen_d256_gfx950.hip, fa_bwd_varlen_d256_gfx950.hip) and
// the soft-capped ones (kCap = true: fa_varlen_d256_softcap_gfx950.hip).  Capped, p.c is ci and `cc` the cap in log2
// units (fa_softcap.h); plain, `cc` is not read.  The files' headers describe the layouts.
// (The dQ kernels are two texts: DESIGN.md 3.22.)
constexpr int kVHalfDT = CV256::DT / 2;   // accumulators of a column half of the dK / dV kernel: 4

template <class T, bool kCap>
__device__ __forceinline__ void varlen_d256_fwd_body(const VarlenD256Params& p, const float cc) {
    using C = CV256;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PA];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int hk = unit % p.Hkv, b = unit / p.Hkv;

    const QueryBlock x = query_block(p, rank, b, hk, wave, l31);   // the sequence, clamped; this block of it; this lane's row
    if (x.rows == 0) return;
    const int ntiles = x.ntiles;

    const char* qrow = p.q + (((long long)x.sq + x.tok) * p.q_stride + (long long)x.head * kVD) * 2;
    u32x4_t qf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    const float c = p.c;
    f32x16_t o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    KeyTiles<kVD> kt(p, x, hk);
    if (ntiles > 0) kt.load(x.kbeg, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = x.kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, C::PA, Vs, C::PT, tid);
        __syncthreads();
        if (t + 1 < ntiles) kt.load(k0 + kPK, tid);
        if (x.skips(k0)) continue;
        f32x16_t sc[2];
        tile_scores<T, C::G>(sc, Ks, C::PA, qf, l31, hi);
        __builtin_amdgcn_sched_barrier(0);
        // scale to log2 units (capped: through the tanh, in place), mask, running max over the lane pair
        float mx = -__builtin_inff();
        if (x.sees_all(k0)) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float y = score_log2<kCap>(sc[kk][rr], c, cc);
                    sc[kk][rr] = y;
                    mx = fmaxf(mx, y);
                }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const float y = x.visible(j) ? score_log2<kCap>(sc[kk][rr], c, cc) : -__builtin_inff();
                    sc[kk][rr] = y;
                    mx = fmaxf(mx, y);
                }
        }
        mx = fmaxf(mx, xhalf(mx));
        const float mn = fmaxf(m, mx);
        const float top = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(m - top);   // m = -inf: 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < C::DT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - top);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, C::PT, 16 * st, 32 * dt, lane), pb, o[dt]);
            __builtin_amdgcn_sched_barrier(0);   // (the transposed reads of one step at a time: hoisted further they cost registers)
        }
    }
    l += xhalf(l);
    if (!x.live) return;
    const long long orow = ((long long)x.sq + x.tok) * p.Hq + x.head;
    store_row16<T, C::DT>(p.o + orow * (long long)C::RB, o, l > 0.f ? 1.f / l : 0.f, hi);
    if (p.lse_out != nullptr && hi == 0) {
        const float top = m == -__builtin_inff() ? 0.f : m;
        p.lse_out[orow] = l > 0.f ? (top + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

// The capped P of one score from its raw product `s` (c = ci): t = tanh by the forward's expression, P = exp2(cc t - L log2 e) on a
// visible key, and `onem` = 1 - t^2 for dS = P (dP - delta) (1 - t^2) -- the scale of d s / d raw = scale (1 - t^2) stays with the store.
// Called element by element, in place: no array beside the caller's.
__device__ __forceinline__ float varlen_d256_capped_p(float s, float c, float cc, float l2, bool vis, float& onem) {
    const float r = __builtin_amdgcn_rcpf(1.f + fast_exp2(s * c));   // t = 1 - 2 r
    onem = 4.f * r * (1.f - r);                                       // 1 - t^2 with no cancellation at either saturation
    return vis ? fast_exp2(cc - 2.f * cc * r - l2) : 0.f;
}

// The twin of fa_bwd_varlen_dkdv_kernel (fa_bwd_varlen_gfx950.hip) over a column half: the clamps, the row range, the per-wave skips and the
// mask are that kernel's statements, and a fix to them there belongs here too.  (Shared as one template the D <= 128 instances would have to
// be recompiled from changed text; fa_tile_attention.h says what that has cost before.)
template <class T, bool kCap>
__device__ __forceinline__ void varlen_d256_dkdv_body(const VarlenD256Params& p, const float cc) {
    using C = CV256;
    __shared__ __attribute__((aligned(16))) char Qs[kVQT * C::PAT];
    __shared__ __attribute__((aligned(16))) char Os[kVQT * C::PAT];
    __shared__ float Ls[kVQT], Dl[kVQT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> (key block, column half, sequence, KV head): the two halves of a key block side by side (they read the same rows),
    // key block 0 first (under the top-left rule it sees the most queries)
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int kbh = bid / units, unit = bid - kbh * units;
    const int kb = kbh >> 1, ch = kbh & 1;
    const int hk = unit % p.Hkv, b = unit / p.Hkv;

    const SeqRange sk = seq_range(p.cu_k, b, p.Tk, p.max_sk);
    const int L = sk.n;
    const int k0 = kb * kVKB;
    if (k0 >= L) return;
    const SeqRange sq = seq_range(p.cu_q, b, p.Tq, p.max_sq);
    const int n = sq.n;
    const bool causal = p.causal != 0;
    const int coff = p.causal == 2 ? L - n : 0;

    // this lane's key (a lane past the end works on the sequence's last key and stores nothing)
    const int kj = k0 + wave * 32 + l31;
    const bool live = kj < L;
    const int kjc = min(kj, L - 1);
    const int wkey_lo = k0 + wave * 32, wkey_hi = min(wkey_lo + 31, L - 1);   // (wave-uniform)

    // tokens that see any key of the block, as packed rows
    const int klast = min(k0 + kVKB, L) - 1;
    int tbeg = 0, tend = n;
    if (causal) tbeg = min(n, max(0, k0 - coff));
    if (p.window > 0) tend = (int)min((long long)n, max(0ll, (long long)klast + p.window - coff));   // (64-bit: the sum may pass 2^31)
    const int rbeg = (int)((long long)tbeg * p.g / kVQT * kVQT);
    const int rend = tend * p.g;
    const int ntiles = rend > rbeg ? (rend - rbeg + kVQT - 1) / kVQT : 0;

    const char* krow = p.k + (((long long)sk.s + kjc) * p.k_stride + (long long)hk * kVD) * 2;
    const char* vrow = p.v + (((long long)sk.s + kjc) * p.v_stride + (long long)hk * kVD) * 2;
    u32x4_t kf[C::G], vf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) {
        kf[g] = *reinterpret_cast<const u32x4_t*>(krow + 32 * g + 16 * hi);
        vf[g] = *reinterpret_cast<const u32x4_t*>(vrow + 32 * g + 16 * hi);
    }
    f32x16_t dk[kVHalfDT], dv[kVHalfDT];
#pragma unroll
    for (int i = 0; i < kVHalfDT; ++i) dk[i] = dv[i] = f32x16_t{};

    // packed row rr of the sequence (rr < rend <= n g): token rr / g, head hk g + rr % g
    const int hq0 = hk * p.g;
    RowTile<kVD, kVQT> qt, ot;
    float pl = 0.f, pd = 0.f;   // threads 0 .. 31: lse log2 e and delta of row tid of the tile in flight
    const auto load_tile = [&](int t0) {
        qt.load([&](int row) -> const char* {
            const int rr = t0 + row;
            if (rr >= rend) return nullptr;
            return p.q + (((long long)sq.s + rr / p.g) * p.q_stride + (long long)(hq0 + rr % p.g) * kVD) * 2;
        }, tid);
        ot.load([&](int row) -> const char* {
            const int rr = t0 + row;
            if (rr >= rend) return nullptr;
            return p.dout + (((long long)sq.s + rr / p.g) * p.Hq + hq0 + rr % p.g) * (long long)C::RB;
        }, tid);
        if (tid < kVQT) {
            const int rr = t0 + tid;
            pl = 0.f;
            pd = 0.f;
            if (rr < rend) {
                const long long at = ((long long)sq.s + rr / p.g) * p.Hq + hq0 + rr % p.g;
                pl = p.lse[at] * kLog2e;
                pd = p.delta[at];
            }
        }
    };
    const int c0 = 128 * ch;   // the first column of this workgroup's half
    if (ntiles > 0) load_tile(rbeg);
    for (int t = 0; t < ntiles; ++t) {
        const int t0 = rbeg + t * kVQT;
        __syncthreads();
        qt.store(Qs, C::PAT, tid);
        ot.store(Os, C::PAT, tid);
        if (tid < kVQT) {
            Ls[tid] = pl;
            Dl[tid] = pd;
        }
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t0 + kVQT);
        // a wave skips the tiles whose rows see none of its keys: every position before its first key, or its last key outside every window
        const int tpos_lo = coff + t0 / p.g, tpos_hi = coff + (min(t0 + kVQT, rend) - 1) / p.g;
        if (wkey_lo >= L || (causal && tpos_hi < wkey_lo) || (p.window > 0 && tpos_lo - wkey_hi >= p.window)) continue;
        // S[row][key] = Q.K^T, dP[row][key] = dO.V^T over the full width
        f32x16_t s = f32x16_t{}, dp = f32x16_t{};
#pragma unroll
        for (int g = 0; g < C::G; ++g) {
            s = mfma16<T>(lds_b128(Qs + l31 * C::PAT + 32 * g + 16 * hi), kf[g], s);
            dp = mfma16<T>(lds_b128(Os + l31 * C::PAT + 32 * g + 16 * hi), vf[g], dp);
        }
        // P and dS (rows crow(r, hi) of the tile)
        f32x16_t ds;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qr = crow(r, hi);
            const int rr = t0 + qr;
            const bool vis = rr < rend && varlen_visible(coff + rr / p.g, kj, L, causal, p.window);
            if constexpr (kCap) {
                float onem;
                const float pr = varlen_d256_capped_p(s[r], p.c, cc, Ls[qr], vis, onem);
                s[r] = pr;
                ds[r] = pr * (dp[r] - Dl[qr]) * onem;
            } else {
                const float pr = vis ? fast_exp2(s[r] * p.c - Ls[qr]) : 0.f;
                s[r] = pr;
                ds[r] = pr * (dp[r] - Dl[qr]);
            }
        }
        // dV^T[d][key] += dO^T.P, dK^T[d][key] += Q^T.dS over the half's columns
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const u32x4_t pb = pack_step<T>(s, st), db = pack_step<T>(ds, st);
#pragma unroll
            for (int dt = 0; dt < kVHalfDT; ++dt) {
                dv[dt] = mfma16<T>(lds_tr_step(Os, C::PAT, 16 * st, c0 + 32 * dt, lane), pb, dv[dt]);
                dk[dt] = mfma16<T>(lds_tr_step(Qs, C::PAT, 16 * st, c0 + 32 * dt, lane), db, dk[dt]);
            }
        }
    }
    if (!live) return;
    const long long at = (((long long)sk.s + kj) * p.Hkv + hk) * (long long)C::RB + c0 * 2;
    store_row16<T, kVHalfDT>(p.dk + at, dk, p.scale, hi);
    store_row16<T, kVHalfDT>(p.dv + at, dv, 1.f, hi);
}

}  // namespace
}  // namespace aule_hip
