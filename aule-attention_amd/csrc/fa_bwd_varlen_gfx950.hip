// fa_bwd_varlen_gfx950.hip -- backward over a variable-length packed batch.
//
// The tensors, the clamps of cu_seqlens_q / cu_seqlens_k and the visibility rule are those of fa_fwd_varlen_gfx950.hip; out, lse,
// dout, dq [Tq, Hq, D] / [Tq, Hq] and dk, dv [Tk, Hkv, D] are contiguous.  Three launches, the plain backward of
// fa_bwd_d256_gfx950.hip generalised over D = 32, 64, 128, the dQ kernel and the row stores from fa_varlen_common.h and fa_tile_attention.h:
//   delta     delta = rowsum(dO * O) in fp32, one wave per (token, head) row, all Tq rows (the workspace: [Tq, Hq] fp32)
//   dQ        ragged_dq_body: the forward's work decomposition and tile walk: workgroup = (rank, sequence, KV head), 128 token-major packed rows,
//             4 waves x 32 rows, Q and dO of the lane's row in registers; K / V tiles of 64 keys through LDS, the next one prefetched
//             into registers; S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T (dP^T - delta) with P = exp2(S c - L log2 e) on visible keys
//             only, dQ^T[d][q] += K^T.dS^T with K read transposed from the same LDS tile (pitch PAT).  dq = scale * acc.
//   dK / dV   workgroup = (sequence, KV head, 128 keys), 4 waves x 32 keys, K and V of the lane's key in registers; dK and dV
//             accumulate UNSPLIT (2 D / 32 accumulators per wave: 128 registers at D = 128).  The workgroup walks the sequence's
//             packed rows -- token-major, the g heads of a token adjacent, so the GQA sum happens here: no partial planes, no
//             reduce pass -- in 32-row tiles of Q and dO through LDS with the rows' lse log2 e and delta; the range is cut to the
//             tokens that can see the block (from token k0 - coff under the causal rule, up to klast + W - coff with a window).
//             A workgroup past its sequence's blocks returns before it touches memory.
// Every owned row of dq, dk and dv is written (zeros where nothing is seen, n = 0 included); rows that belong to no sequence never.
#include "fa_kernels.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

struct VarlenBwdParams {
    const char* q;
    const char* k;
    const char* v;
    const char* o;
    const char* dout;
    const float* lse;
    float* delta;
    char* dq;
    char* dk;
    char* dv;
    const int* cu_q;
    const int* cu_k;
    long long q_stride, k_stride, v_stride;   // elements between tokens
    int Tq, Tk, B, Hq, Hkv, g, D;
    int max_sq, max_sk;
    float c;       // scale * log2(e)
    float scale;
    int causal;    // 0, 1, 2
    int window;    // > 0: on
};

// one wave per (token, head) row of the contiguous out / dout; D: any multiple of 8
template <class T>
__global__ void __launch_bounds__(256) fa_bwd_varlen_delta_kernel(const VarlenBwdParams p, long long rows) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const char* a = p.o + row * p.D * 2;
    const char* b = p.dout + row * p.D * 2;
    float acc = 0.f;
    for (int ch = lane; ch < p.D / 8; ch += 64) {
        const u32x4_t x = *reinterpret_cast<const u32x4_t*>(a + 16 * ch);
        const u32x4_t y = *reinterpret_cast<const u32x4_t*>(b + 16 * ch);
#pragma unroll
        for (int w = 0; w < 4; ++w) acc += T::lo(x[w]) * T::lo(y[w]) + T::hi(x[w]) * T::hi(y[w]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) p.delta[row] = acc;
}

template <class T, int D>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_dq_kernel(const VarlenBwdParams p) {
    using C = VarlenCfg<D>;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PAT];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PA];
    ragged_dq_body<T, VarlenShape<D>>(p, Ks, Vs);
}

template <class T, int D>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_dkdv_kernel(const VarlenBwdParams p) {
    using C = VarlenCfg<D>;
    __shared__ __attribute__((aligned(16))) char Qs[kVQT * C::PAT];
    __shared__ __attribute__((aligned(16))) char Os[kVQT * C::PAT];
    __shared__ float Ls[kVQT], Dl[kVQT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> (key block, sequence, KV head): key block 0 first (under the top-left rule it sees the most queries)
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int kb = bid / units, unit = bid - kb * units;
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

    const char* krow = p.k + (((long long)sk.s + kjc) * p.k_stride + (long long)hk * D) * 2;
    const char* vrow = p.v + (((long long)sk.s + kjc) * p.v_stride + (long long)hk * D) * 2;
    u32x4_t kf[C::G], vf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) {
        kf[g] = *reinterpret_cast<const u32x4_t*>(krow + 32 * g + 16 * hi);
        vf[g] = *reinterpret_cast<const u32x4_t*>(vrow + 32 * g + 16 * hi);
    }
    f32x16_t dk[C::DT], dv[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) dk[i] = dv[i] = f32x16_t{};

    // packed row rr of the sequence (rr < rend <= R): token rr / g, head hk g + rr % g
    const int hq0 = hk * p.g;
    RowTile<D, kVQT> qt, ot;
    float pl = 0.f, pd = 0.f;   // threads 0 .. 31: lse log2 e and delta of row tid of the tile in flight
    const auto load_tile = [&](int t0) {
        qt.load([&](int row) -> const char* {
            const int rr = t0 + row;
            if (rr >= rend) return nullptr;
            return p.q + (((long long)sq.s + rr / p.g) * p.q_stride + (long long)(hq0 + rr % p.g) * D) * 2;
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
        // S[row][key] = Q.K^T, dP[row][key] = dO.V^T
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
        // dV^T[d][key] += dO^T.P, dK^T[d][key] += Q^T.dS
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const u32x4_t pb = pack_step<T>(s, st), db = pack_step<T>(ds, st);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) {
                dv[dt] = mfma16<T>(lds_tr_step(Os, C::PAT, 16 * st, 32 * dt, lane), pb, dv[dt]);
                dk[dt] = mfma16<T>(lds_tr_step(Qs, C::PAT, 16 * st, 32 * dt, lane), db, dk[dt]);
            }
        }
    }
    if (!live) return;
    const long long krow_out = ((long long)sk.s + kj) * p.Hkv + hk;
    store_row16<T, C::DT>(p.dk + krow_out * (long long)C::RB, dk, p.scale, hi);
    store_row16<T, C::DT>(p.dv + krow_out * (long long)C::RB, dv, 1.f, hi);
}

}  // namespace

// ceil(min(max_seqlen_k, Tk) / 128) key blocks per (sequence, KV head)
long long varlen_dkdv_grid(const VarlenArgs& a) {
    if (a.Hkv <= 0 || a.max_seqlen_k <= 0 || a.Tk <= 0) return 0;
    return ((long long)varlen_max_sk(a) + kVKB - 1) / kVKB * a.Hkv * a.B;
}

// delta [Tq, Hq] fp32, on a 256-byte boundary
uint64_t varlen_bwd_workspace_bytes(long long Tq, int Hq) {
    return ((uint64_t)Tq * Hq * sizeof(float) + 255) / 256 * 256;
}

int launch_varlen_bwd(const VarlenArgs& a, hipStream_t stream) {
    if (!varlen_args_ok(a)) return -1;
    const long long dq_grid = varlen_fwd_grid(a), dkdv_grid = varlen_dkdv_grid(a);
    if (dq_grid <= 0 && dkdv_grid <= 0) return 0;
    if (dq_grid > 0x7fffffffll || dkdv_grid > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;
    const long long rows = (long long)a.Tq * a.Hq;
    if ((rows + 3) / 4 > 0x7fffffffll) return -1;
    VarlenBwdParams p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k); p.v = static_cast<const char*>(a.v);
    p.o = static_cast<const char*>(a.o); p.dout = static_cast<const char*>(a.dout); p.lse = a.lse; p.delta = a.delta;
    p.dq = static_cast<char*>(a.dq); p.dk = static_cast<char*>(a.dk); p.dv = static_cast<char*>(a.dv);
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k;
    p.q_stride = a.q_token_stride; p.k_stride = a.k_token_stride; p.v_stride = a.v_token_stride;
    p.Tq = a.Tq; p.Tk = a.Tk; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv; p.D = a.D;
    p.max_sq = varlen_max_sq(a);
    p.max_sk = varlen_max_sk(a);
    p.c = a.scale * kLog2e;
    p.scale = a.scale;
    p.causal = a.causal;
    p.window = varlen_window(a);
    return dispatch_tile_instance(a.dtype, a.D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int D = decltype(d)::value;
        if (dq_grid > 0) {
            hipLaunchKernelGGL((fa_bwd_varlen_delta_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, p, rows);
            hipLaunchKernelGGL((fa_bwd_varlen_dq_kernel<T, D>), dim3((unsigned)dq_grid), dim3(256), 0, stream, p);
        }
        if (dkdv_grid > 0) hipLaunchKernelGGL((fa_bwd_varlen_dkdv_kernel<T, D>), dim3((unsigned)dkdv_grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
