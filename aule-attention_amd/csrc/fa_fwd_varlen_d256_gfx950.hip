// fa_fwd_varlen_d256_gfx950.hip -- forward over a variable-length packed batch at head_dim 256.
//
// The tensors, the clamps of cu_seqlens_q / cu_seqlens_k, the positions and the visibility rule are those of fa_fwd_varlen_gfx950.hip
// (VarlenArgs, fa_kernels.h); q [Tq, Hq, 256], k, v [Tk, Hkv, 256], 16-bit, each with its own token stride.
//
// Layout: workgroup = (rank, sequence, KV head), rank 0 the sequence's last block of 128 token-major PACKED rows (QueryBlock), 4 waves
// x 32 rows, one workgroup per compute unit.  A lane keeps the 16 operand chunks of its Q row (64 registers), 8 output accumulators
// (128 registers, accumulation registers) and the row's m / l; lanes l and l + 32 hold the two halves of one row's chunks.
// K and V tiles of 64 keys go through LDS at pitches 528 and 576 (33 792 + 36 864 = 70 656 bytes); the next tile sits in 64 registers
// per thread while this one is multiplied:
//   S^T[key][row] = K.Q^T   32 MFMAs of 32x32x16 (tile_scores, K read as ds_read_b128 rows)
//   online softmax in log2 units over the lane pair, P^T packed as the B operand with no lane movement
//   O^T[d][row] += V^T.P^T  32 MFMAs, V read transposed (ds_read_b64_tr_b16)
// 64 MFMAs per wave and tile, no product computed twice and no exchange between waves -- the 128-row block, not the split-head
// 64-row block of the paged kernel (3.20), which pays an LDS round trip per tile that long sequences do not amortise.
// A wave skips a tile none of its rows sees and runs unmasked where every row sees all of it (3.8).  A row without a visible key
// writes O = 0 and LSE = -inf.  One launch, no workspace: grid = ceil(min(max_seqlen_q, Tq) g / 128) x Hkv x B.
#include "fa_varlen_d256.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_varlen_d256_kernel(const VarlenD256Params p) {
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
        // scale to log2 units, mask, running max over the lane pair
        float mx = -__builtin_inff();
        if (x.sees_all(k0)) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float y = sc[kk][rr] * c;
                    sc[kk][rr] = y;
                    mx = fmaxf(mx, y);
                }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const float y = x.visible(j) ? sc[kk][rr] * c : -__builtin_inff();
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

}  // namespace

int launch_varlen_d256_fwd(const VarlenArgs& a, hipStream_t stream) {
    if (a.D != kVD || a.sinks != nullptr || !varlen_args_ok(a)) return -1;
    const long long nwg = varlen_fwd_grid(a);   // (the grid rule does not depend on the head dimension)
    if (nwg <= 0) return 0;
    // the kernel counts packed rows in 32 bits
    if (nwg > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll || a.Tk < 0) return -1;
    const VarlenD256Params p = varlen_d256_params(a);
    return dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_fwd_varlen_d256_kernel<decltype(t)>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
