// fa_bwd_varlen_d256_gfx950.hip -- backward over a variable-length packed batch at head_dim 256.
//
// The tensors, the clamps and the visibility rule are those of fa_fwd_varlen_d256_gfx950.hip; out, lse, dout, dq [Tq, Hq, 256] /
// [Tq, Hq] and dk, dv [Tk, Hkv, 256] are contiguous.  Three launches on the stream:
//   delta     launch_varlen_delta (fa_bwd_varlen_gfx950.hip): delta = rowsum(dO * O), fp32, the workspace [Tq, Hq]
//   dQ        the walk of ragged_dq_body (fa_varlen_common.h) in a body of its own -- instantiated at 256 the shared body spills 8
//             registers: the forward's decomposition and tile walk, the 16 Q chunks of the lane's row in registers (64), its 16 dO
//             chunks in the lane's own row of a third LDS image (128 x 528 = 67 584 bytes, written and read by the same lane), 8 dQ
//             accumulators (128, accumulation registers), S / dP (64) and the next K / V tile (64); K through one LDS tile at pitch
//             592, read plain and transposed, V at 528: 139 264 bytes of the compute unit's 160 KB.
//   dK / dV   workgroup = (key block of 128, column half ch, sequence, KV head), 4 waves x 32 keys, the 16 K and 16 V chunks of the
//             lane's key in registers (64 + 64).  A wave cannot hold 8 + 8 accumulators beside them, so the two workgroups of a key
//             block each accumulate HALF of the columns -- dK and dV columns 128 ch .. 128 ch + 127, four accumulators each (128
//             registers) -- and both recompute S = Q.K^T and dP = dO.V^T over the full width (32 MFMAs) before their 32 MFMAs of
//             accumulation, as the dense head_dim 256 kernel does.  The sequence's packed rows are walked token-major in 32-row tiles
//             of Q and dO through LDS (pitch 592, 2 x 18 944 bytes) with their lse log2 e and delta, the next tile in 32 registers;
//             the g heads of a token are adjacent rows, so the GQA sum happens here: no partial planes, no reduce pass, no atomics.
//             The row range is cut to the tokens that can see the block, tile skips are per wave (3.8).  A workgroup past its
//             sequence's blocks returns before it touches memory.
// Every owned row of dq, dk and dv is written (zeros where nothing is seen, n = 0 included); rows that belong to no sequence never.
#include "fa_varlen_d256.h"

namespace aule_hip {
namespace {

constexpr int kHalfDT = CV256::DT / 2;   // accumulators of a column half: 4

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_d256_dq_kernel(const VarlenD256Params p) {
    using C = CV256;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PAT];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PA];
    __shared__ __attribute__((aligned(16))) char Os[kPQ * C::PA];
    // ragged_dq_body's walk and arithmetic (fa_varlen_common.h) with the dO chunks in LDS.  64 Q + 64 dO operand, 64 S / dP and 64
    // prefetch registers are all 256 plain registers before an address is computed (the shared body spills 8 at this width).  Every
    // lane therefore parks the 16 dO chunks of its row in LDS -- the bytes it wrote are the bytes it reads back as the B operand of
    // dP, 16 ds_read_b128 per tile beside the 128 of the tile itself, so no barrier is involved -- and the MFMA groups are fenced so
    // that their LDS reads stay with them.
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int hk = unit % p.Hkv, b = unit / p.Hkv;

    const QueryBlock x = query_block(p, rank, b, hk, wave, l31);
    if (x.rows == 0) return;
    const int ntiles = x.ntiles;

    // Q operand chunks of this lane's row in registers, its dO chunks in its own LDS row, its lse (log2 units) and delta
    const long long orow = ((long long)x.sq + x.tok) * p.Hq + x.head;
    const char* qrow = p.q + (((long long)x.sq + x.tok) * p.q_stride + (long long)x.head * kVD) * 2;
    const char* dorow = p.dout + orow * (long long)C::RB;
    char* mine = Os + (wave * 32 + l31) * C::PA + 16 * hi;
    u32x4_t qf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) {
        qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);
        *reinterpret_cast<u32x4_t*>(mine + 32 * g) = *reinterpret_cast<const u32x4_t*>(dorow + 32 * g + 16 * hi);
    }
    const float l2 = p.lse[orow] * kLog2e;
    const float dl = p.delta[orow];

    f32x16_t acc[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) acc[i] = f32x16_t{};

    KeyTiles<kVD> kt(p, x, hk);
    if (ntiles > 0) kt.load(x.kbeg, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = x.kbeg + t * kPK;
        __syncthreads();
        kt.store(Ks, C::PAT, Vs, C::PA, tid);
        __syncthreads();
        if (t + 1 < ntiles) kt.load(k0 + kPK, tid);
        if (x.skips(k0)) continue;
        // S^T[key][row] = K.Q^T, dP^T[key][row] = V.dO^T
        f32x16_t s[2], dp[2] = {f32x16_t{}, f32x16_t{}};
        tile_scores<T, C::G>(s, Ks, C::PAT, qf, l31, hi);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < C::G; ++g) {
            const u32x4_t of = lds_b128(mine + 32 * g);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) dp[kk] = mfma16<T>(lds_b128(Vs + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), of, dp[kk]);
        }
        __builtin_amdgcn_sched_barrier(0);
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
            for (int dt = 0; dt < C::DT; ++dt) acc[dt] = mfma16<T>(lds_tr_step(Ks, C::PAT, 16 * st, 32 * dt, lane), bs, acc[dt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (!x.live) return;
    store_row16<T, C::DT>(p.dq + orow * (long long)C::RB, acc, p.scale, hi);
}

// The twin of fa_bwd_varlen_dkdv_kernel (fa_bwd_varlen_gfx950.hip) over a column half: the clamps, the row range, the per-wave skips and the
// mask are that kernel's statements, and a fix to them there belongs here too.  (Shared as one template the D <= 128 instances would have to
// be recompiled from changed text; fa_tile_attention.h says what that has cost before.)
template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_d256_dkdv_kernel(const VarlenD256Params p) {
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
    f32x16_t dk[kHalfDT], dv[kHalfDT];
#pragma unroll
    for (int i = 0; i < kHalfDT; ++i) dk[i] = dv[i] = f32x16_t{};

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
            const float pr = vis ? fast_exp2(s[r] * p.c - Ls[qr]) : 0.f;
            s[r] = pr;
            ds[r] = pr * (dp[r] - Dl[qr]);
        }
        // dV^T[d][key] += dO^T.P, dK^T[d][key] += Q^T.dS over the half's columns
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const u32x4_t pb = pack_step<T>(s, st), db = pack_step<T>(ds, st);
#pragma unroll
            for (int dt = 0; dt < kHalfDT; ++dt) {
                dv[dt] = mfma16<T>(lds_tr_step(Os, C::PAT, 16 * st, c0 + 32 * dt, lane), pb, dv[dt]);
                dk[dt] = mfma16<T>(lds_tr_step(Qs, C::PAT, 16 * st, c0 + 32 * dt, lane), db, dk[dt]);
            }
        }
    }
    if (!live) return;
    const long long at = (((long long)sk.s + kj) * p.Hkv + hk) * (long long)C::RB + c0 * 2;
    store_row16<T, kHalfDT>(p.dk + at, dk, p.scale, hi);
    store_row16<T, kHalfDT>(p.dv + at, dv, 1.f, hi);
}

}  // namespace

// two column halves per key block of 128: 2 ceil(min(max_seqlen_k, Tk) / 128) x Hkv x B
long long varlen_d256_dkdv_grid(const VarlenArgs& a) { return 2 * varlen_dkdv_grid(a); }

int launch_varlen_d256_bwd(const VarlenArgs& a, hipStream_t stream) {
    if (a.D != kVD || a.sinks != nullptr || !varlen_args_ok(a)) return -1;
    const long long dq_grid = varlen_fwd_grid(a), dkdv_grid = varlen_d256_dkdv_grid(a);
    if (dq_grid <= 0 && dkdv_grid <= 0) return 0;
    if (dq_grid > 0x7fffffffll || dkdv_grid > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;
    if (dq_grid > 0) {
        if (const int rc = launch_varlen_delta(a, stream)) return rc;
    }
    const VarlenD256Params p = varlen_d256_params(a);
    return dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (dq_grid > 0) hipLaunchKernelGGL((fa_bwd_varlen_d256_dq_kernel<T>), dim3((unsigned)dq_grid), dim3(256), 0, stream, p);
        if (dkdv_grid > 0) hipLaunchKernelGGL((fa_bwd_varlen_d256_dkdv_kernel<T>), dim3((unsigned)dkdv_grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
