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

// (the body: fa_varlen_d256.h)
template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_d256_dkdv_kernel(const VarlenD256Params p) {
    varlen_d256_dkdv_body<T, false>(p, 0.f);
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
