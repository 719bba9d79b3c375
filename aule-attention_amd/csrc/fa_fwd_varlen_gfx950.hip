// fa_fwd_varlen_gfx950.hip -- forward over a variable-length packed batch.
//
// Sequences of different lengths packed along one token axis: q [Tq, Hq, D] and k, v [Tk, Hkv, D], the heads of a token contiguous,
// each with its own token stride; cu_seqlens_q / cu_seqlens_k [B + 1] on the device.  Everything per sequence is read and clamped HERE:
//     s_q = clamp(cu_q[b], 0, Tq)   e_q = clamp(cu_q[b + 1], s_q, Tq)   n = min(e_q - s_q, max_seqlen_q)
//     s_k = clamp(cu_k[b], 0, Tk)   e_k = clamp(cu_k[b + 1], s_k, Tk)   L = min(e_k - s_k, max_seqlen_k)
// query i < n is row s_q + i at position pos = i (no mask, top-left) or i + L - n (bottom-right; L < n allowed, pos < 0 sees nothing);
// key j < L is row s_k + j, visible iff (!causal || j <= pos) and, with a window W > 0, pos - j < W.  A stale offset cannot index
// outside a buffer, and rows of out / lse outside every [s_q, s_q + n) are never written.
//
// Layout: the loop of fa_fwd_paged_prefill_gfx950.hip with a contiguous tile source and the three causal modes:
//   workgroup = (rank, sequence, KV head), rank 0 the sequence's last block of 128 token-major PACKED rows (row r = token r / g, head
//   hk g + r % g), 4 waves x 32 rows; Q of the lane's row in registers, K / V tiles of 64 keys in LDS, the next tile prefetched into
//   registers while this one is computed; a wave skips a tile none of its rows sees and runs unmasked where every row sees all of it.
// Key row kv of the sequence is at byte ((s_k + kv) k_token_stride + hk D) 2 of k (64-bit); rows at or beyond the block's last
// visible key are not read (zeros in LDS).  Online softmax in log2 units with fp32 m, l, acc; a row without a visible key writes
// O = 0 and LSE = -inf (VarlenArgs::sinks given: LSE = the head's sink logit).  One launch, no workspace:
// grid = ceil(min(max_seqlen_q, Tq) g / 128) x Hkv x B.
#include "fa_kernels.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

struct VarlenFwdParams {
    const char* q;
    const char* k;
    const char* v;
    char* o;
    float* lse;
    const int* cu_q;
    const int* cu_k;
    const float* sinks;   // [Hq] fp32 sink logits or null
    long long q_stride, k_stride, v_stride;   // elements between tokens
    int Tq, Tk, B, Hq, Hkv, g;
    int max_sq, max_sk;
    float c;        // scale * log2(e) (sign kept)
    int causal;     // 0, 1, 2
    int window;     // > 0: on
};

template <class T, int D>
__global__ void __launch_bounds__(256, 1) fa_fwd_varlen_kernel(const VarlenFwdParams p) {
    using C = VarlenCfg<D>;
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

    // Q operand chunks of this lane's row
    const char* qrow = p.q + (((long long)x.sq + x.tok) * p.q_stride + (long long)x.head * D) * 2;
    u32x4_t qf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    const float c = p.c;
    f32x16_t o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    KeyTiles<D> kt(p, x, hk);
    if (ntiles > 0) kt.load(x.kbeg, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = x.kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.k.store(Ks, C::PA, tid);
        kt.v.store(Vs, C::PT, tid);
        __syncthreads();
        if (t + 1 < ntiles) kt.load(k0 + kPK, tid);
        if (x.skips(k0)) continue;
        // S^T[key][row] = K.Q^T over the 64 keys of the tile
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int g = 0; g < C::G; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                sc[kk] = mfma16<T>(lds_b128(Ks + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), qf[g], sc[kk]);
        // scale to log2 units, mask, running max over the lane pair (lanes l and l + 32 hold the same row)
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
        const float mu = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(m - mu);   // m = -inf: 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < C::DT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - mu);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, C::PT, 16 * st, 32 * dt, lane), pb, o[dt]);
        }
    }
    l += xhalf(l);
    if (!x.live) return;
    float inv = l > 0.f ? 1.f / l : 0.f;
    // sink logits (a wave-uniform pointer; null: the line above is the whole story): the head's logit joins the denominator
    const bool sink = p.sinks != nullptr;
    float sink_lse = 0.f;
    if (sink) sink_lse = sink_epilogue(p.sinks[x.head], m, l, inv);
    const long long orow = ((long long)x.sq + x.tok) * p.Hq + x.head;
    char* og = p.o + orow * (long long)C::RB;
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && hi == 0) {
        if (sink) {
            p.lse[orow] = sink_lse;
        } else {
            const float mu = m == -__builtin_inff() ? 0.f : m;
            p.lse[orow] = l > 0.f ? (mu + fast_log2(l)) * kLn2 : -__builtin_inff();
        }
    }
}

}  // namespace

// The grid rule: ceil(min(max_seqlen_q, Tq) * g / 128) blocks per (sequence, KV head); the kernel decodes (rank, sequence, KV head)
// from the 1-D index, KV head fastest, rank r = the sequence's own block count - 1 - r.
long long varlen_fwd_grid(const VarlenArgs& a) {
    if (a.Hkv <= 0 || a.max_seqlen_q <= 0 || a.Tq <= 0) return 0;
    return ((long long)varlen_max_sq(a) * (a.Hq / a.Hkv) + kPQ - 1) / kPQ * a.Hkv * a.B;
}

int launch_varlen_fwd(const VarlenArgs& a, hipStream_t stream) {
    if (!varlen_args_ok(a)) return -1;
    const long long nwg = varlen_fwd_grid(a);
    if (nwg <= 0) return 0;
    // the kernel counts packed rows in 32 bits
    if (nwg > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll || a.Tk < 0) return -1;
    VarlenFwdParams p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k); p.v = static_cast<const char*>(a.v);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k; p.sinks = a.sinks;
    p.q_stride = a.q_token_stride; p.k_stride = a.k_token_stride; p.v_stride = a.v_token_stride;
    p.Tq = a.Tq; p.Tk = a.Tk; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv;
    p.max_sq = varlen_max_sq(a);
    p.max_sk = varlen_max_sk(a);
    p.c = a.scale * kLog2e;
    p.causal = a.causal;
    p.window = varlen_window(a);
    return dispatch_tile_instance(a.dtype, a.D, [&](auto t, auto d) {
        hipLaunchKernelGGL((fa_fwd_varlen_kernel<decltype(t), decltype(d)::value>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
