// fa_varlen_d256_softcap_gfx950.hip -- variable-length packed attention at head_dim 256 with logit soft-capping, forward and backward
// (Gemma-2: softcap = 50):
//     s_ij = softcap tanh(scale q_i.k_j / softcap),  P = softmax_j(s_ij over visible j),  out = P.V,  lse_i = ln sum_j exp(s_ij).
// The mask is applied after the cap (an invisible key stays -inf; a row without a key writes zeros and lse = -inf).
//
// The forward and the dK / dV kernel are the kCap = true instances of the bodies of fa_varlen_d256.h, the dQ kernel a twin of the plain
// one (below) -- the layouts, the tile walk, the LDS images and the register budget are those of fa_fwd_varlen_d256_gfx950.hip /
// fa_bwd_varlen_d256_gfx950.hip -- under names of their own, in a translation unit of their own, so that the plain kernels'
// instances stay as they were.  What differs is the score step (fa_softcap.h), computed in place on the score registers:
//   forward   y = cc - 2 cc rcp(1 + exp2(raw ci)) in log2 units; the running max, the rescale and the lane-pair exchange as before (a
//             fixed maximum cc would underflow a row whose scores all sit near -softcap)
//   dQ, dK/dV r = rcp(1 + exp2(raw ci)), t = 1 - 2 r: P = exp2(cc t - lse log2 e), dS = P (dP - delta) (1 - t^2) with
//             1 - t^2 = 4 r (1 - r); the scale of d s / d raw = scale (1 - t^2) is the one the dq / dk store applies already
// The host folds ci = 2 log2(e) scale / softcap into the parameter block's c and passes cc = softcap log2(e) beside it.  delta is the
// plain backward's launch (launch_varlen_delta): it does not depend on the scores.
#include "fa_varlen_d256.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_varlen_d256_cap_kernel(const VarlenD256Params p, const float cc) {
    varlen_d256_fwd_body<T, true>(p, cc);
}

// The dQ kernel with a body of its own: moved into a shared template, the plain kernel's register allocation changed,
// so fa_bwd_varlen_d256_dq_kernel keeps its text and this is its walk with the capped dS.  It sits at 256 plain registers like the
// plain one: t, P and dS are computed element by element in place of the score.
template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_d256_cap_dq_kernel(const VarlenD256Params p, const float cc) {
    using C = CV256;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PAT];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PA];
    __shared__ __attribute__((aligned(16))) char Os[kPQ * C::PA];
    // (the dO chunks of the lane's row in its own LDS row, the MFMA groups fenced: fa_bwd_varlen_d256_gfx950.hip says why)
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
        // dS^T = P^T (dP^T - delta) (1 - t^2), P^T = exp2(cc t - L log2 e) on visible keys
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const int j = k0 + 32 * kk + crow(rr, hi);
                float onem;
                const float pr = varlen_d256_capped_p(s[kk][rr], p.c, cc, l2, x.visible(j), onem);
                s[kk][rr] = pr * (dp[kk][rr] - dl) * onem;
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

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_varlen_d256_cap_dkdv_kernel(const VarlenD256Params p, const float cc) {
    varlen_d256_dkdv_body<T, true>(p, cc);
}

// the plain kernels' parameter block with ci in the place of scale log2(e)
VarlenD256Params capped_params(const VarlenArgs& a, const SoftcapConsts& k) {
    VarlenD256Params p = varlen_d256_params(a);
    p.c = k.ci;
    return p;
}

bool softcap_ok(float softcap) { return softcap > 0.f && softcap <= 3.4e38f; }   // (finite, and not NaN: both comparisons fail on it)

}  // namespace

// (the argument and grid rules of launch_varlen_d256_fwd)
int launch_varlen_d256_softcap_fwd(const VarlenArgs& a, float softcap, hipStream_t stream) {
    if (a.D != kVD || a.sinks != nullptr || !softcap_ok(softcap) || !varlen_args_ok(a)) return -1;
    const long long nwg = varlen_fwd_grid(a);
    if (nwg <= 0) return 0;
    if (nwg > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll || a.Tk < 0) return -1;
    const SoftcapConsts k = softcap_consts(a.scale, softcap);
    const VarlenD256Params p = capped_params(a, k);
    return dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_fwd_varlen_d256_cap_kernel<decltype(t)>), dim3((unsigned)nwg), dim3(256), 0, stream, p, k.cc);
        return (int)hipGetLastError();
    });
}

// (the argument and grid rules of launch_varlen_d256_bwd; delta, dQ, dK/dV on `stream`)
int launch_varlen_d256_softcap_bwd(const VarlenArgs& a, float softcap, hipStream_t stream) {
    if (a.D != kVD || a.sinks != nullptr || !softcap_ok(softcap) || !varlen_args_ok(a)) return -1;
    const long long dq_grid = varlen_fwd_grid(a), dkdv_grid = varlen_d256_dkdv_grid(a);
    if (dq_grid <= 0 && dkdv_grid <= 0) return 0;
    if (dq_grid > 0x7fffffffll || dkdv_grid > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;
    if (dq_grid > 0) {
        if (const int rc = launch_varlen_delta(a, stream)) return rc;
    }
    const SoftcapConsts k = softcap_consts(a.scale, softcap);
    const VarlenD256Params p = capped_params(a, k);
    return dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (dq_grid > 0) hipLaunchKernelGGL((fa_bwd_varlen_d256_cap_dq_kernel<T>), dim3((unsigned)dq_grid), dim3(256), 0, stream, p, k.cc);
        if (dkdv_grid > 0) hipLaunchKernelGGL((fa_bwd_varlen_d256_cap_dkdv_kernel<T>), dim3((unsigned)dkdv_grid), dim3(256), 0, stream, p, k.cc);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
