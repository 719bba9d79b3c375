// fa_fwd_mla_prefill_gfx950.hip -- MLA prefill, the non-absorbed form, over a variable-length packed batch.
//
// Multi-head latent attention as the prompt runs it: every head has its own 128-wide k_nope and 128-wide v (slices of the kv_b
// up-projection), all heads of a token share one 64-wide rotated k_pe, queries are 192 wide (q_nope | q_pe), the output 128 wide.
//     q [Tq, H, 192]   k_nope, v [Tk, H, 128] with their own token AND head strides   k_pe [Tk, 64] with its own token stride
//     out [Tq, H, 128] contiguous   lse [Tq, H] fp32 or null   cu_seqlens_q / cu_seqlens_k [B + 1] on the device
// The sequence bounds, their clamps, the cuts by max_seqlen_*, the positions and the visibility rule are the variable-length
// forward's (fa_fwd_varlen_gfx950.hip; seq_range, query_block of fa_varlen_common.h) with heads_kv = heads_q (g = 1) and no window.
//
// Layout: that kernel's loop with a 192-wide score reduction, a 128-wide value and a K tile assembled from two sources:
//   workgroup = (rank, sequence, head), rank 0 the sequence's last block of 128 tokens, 4 waves x 32 rows, head fastest in the 1-D
//   grid (the heads of one (block, sequence) run together and find the k_pe rows of their tiles in L2); Q of the lane's row in
//   registers (12 chunk pairs), K tiles of 64 keys in LDS at pitch 384 + 16 bytes (25 sixteen-byte slots), V tiles at the D = 128
//   pitch of PrefillCfg, the next tile prefetched into registers (24 + 16) while this one is computed.
// 16-byte chunk c of key row kv of the sequence: c < 16 is at byte ((s_k + kv) k_nope_token_stride + head k_nope_head_stride) 2 + 16 c
// of k_nope, 16 <= c < 24 at byte ((s_k + kv) k_pe_token_stride) 2 + 16 (c - 16) of k_pe (64-bit); rows at or beyond the block's
// last visible key are not read (zeros in LDS).  Online softmax in log2 units with fp32 m, l, acc; a row without a visible key
// writes O = 0 and LSE = -inf; rows of no sequence are never written.  One launch, no workspace:
// grid = ceil(min(max_seqlen_q, Tq) / 128) x H x B.  LDS 64 (400 + 320) = 46080 bytes.
#include "fa_kernels.h"
#include "fa_mla_prefill_common.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

struct MlaPrefillParams {
    const char* q;
    const char* k_nope;
    const char* k_pe;
    const char* v;
    char* o;
    float* lse;
    const int* cu_q;
    const int* cu_k;
    long long q_stride;                  // elements between tokens
    long long kn_stride, kn_hstride;     // elements between tokens / heads of k_nope
    long long v_stride, v_hstride;
    long long kp_stride;                 // elements between tokens of k_pe
    int Tq, Tk, B, H;
    int max_sq, max_sk;
    float c;        // scale * log2(e) (sign kept)
    int causal;     // 0, 1, 2
    // what query_block reads beside the above: MHA, no window
    static constexpr int g = 1;
    static constexpr int window = 0;
};

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_mla_prefill_kernel(const MlaPrefillParams p) {
    using CV = PrefillCfg<kDV>;
    constexpr int PA = PrefillCfg<kDQK>::PA;   // 400: 25 slots
    constexpr int G = PrefillCfg<kDQK>::G;     // 12
    static_assert(PA == 400 && G == 12 && CV::PT == 320 && CV::DT == 4, "the budget of DESIGN.md 3.10");
    __shared__ __attribute__((aligned(16))) char Ks[kPK * PA];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * CV::PT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int units = p.H * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int head = unit % p.H, b = unit / p.H;

    const QueryBlock x = query_block(p, rank, b, head, wave, l31);   // the sequence, clamped; this block of it; this lane's row
    if (x.rows == 0) return;
    const int ntiles = x.ntiles;

    // Q operand chunks of this lane's row
    const char* qrow = p.q + (((long long)x.sq + x.tok) * p.q_stride + (long long)head * kDQK) * 2;
    u32x4_t qf[G];
#pragma unroll
    for (int g = 0; g < G; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    const float c = p.c;
    f32x16_t o[CV::DT];
#pragma unroll
    for (int i = 0; i < CV::DT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    MlaKeyTiles kt(p, x, head);
    if (ntiles > 0) kt.load(x.kbeg, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = x.kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, PA, Vs, CV::PT, tid);
        __syncthreads();
        if (t + 1 < ntiles) kt.load(k0 + kPK, tid);
        if (x.skips(k0)) continue;
        // S^T[key][row] = K.Q^T over the 64 keys of the tile, 192 elements deep
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                sc[kk] = mfma16<T>(lds_b128(Ks + (32 * kk + l31) * PA + 32 * g + 16 * hi), qf[g], sc[kk]);
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
        for (int i = 0; i < CV::DT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - mu);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T over the 128 value columns
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < CV::DT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, CV::PT, 16 * st, 32 * dt, lane), pb, o[dt]);
        }
    }
    l += xhalf(l);
    if (!x.live) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    const long long orow = ((long long)x.sq + x.tok) * p.H + head;
    char* og = p.o + orow * (long long)CV::RB;
#pragma unroll
    for (int dt = 0; dt < CV::DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && hi == 0) {
        const float mu = m == -__builtin_inff() ? 0.f : m;
        p.lse[orow] = l > 0.f ? (mu + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

}  // namespace

// The grid rule: ceil(min(max_seqlen_q, Tq) / 128) blocks per (sequence, head); the kernel decodes (rank, sequence, head) from the
// 1-D index, head fastest, rank r = the sequence's own block count - 1 - r.
long long mla_prefill_grid(const MlaPrefillArgs& a) {
    if (a.H <= 0 || a.B <= 0 || a.max_seqlen_q <= 0 || a.Tq <= 0) return 0;
    return ((long long)seqlen_cut(a.max_seqlen_q, a.Tq) + kPQ - 1) / kPQ * a.H * a.B;
}

int launch_mla_prefill(const MlaPrefillArgs& a, hipStream_t stream) {
    if (a.causal < 0 || a.causal > 2) return -1;
    if (a.q_token_stride < (long long)a.H * kDQK || a.q_token_stride % 8 != 0) return -1;
    if (a.k_nope_head_stride < kDN || a.k_nope_head_stride % 8 != 0 || a.k_nope_token_stride < kDN || a.k_nope_token_stride % 8 != 0) return -1;
    if (a.v_head_stride < kDV || a.v_head_stride % 8 != 0 || a.v_token_stride < kDV || a.v_token_stride % 8 != 0) return -1;
    if (a.k_pe_token_stride < kDR || a.k_pe_token_stride % 8 != 0) return -1;
    const long long nwg = mla_prefill_grid(a);
    if (nwg <= 0) return 0;
    // the kernel counts rows in 32 bits
    if (nwg > 0x7fffffffll || (long long)a.Tq + kPQ > 0x7fffffffll || a.Tk < 0) return -1;
    MlaPrefillParams p;
    mla_inputs(p, a);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    const dim3 grid((unsigned)nwg), block(256);
    if (a.dtype == kBF16) hipLaunchKernelGGL((fa_fwd_mla_prefill_kernel<Bf16Traits>), grid, block, 0, stream, p);
    else if (a.dtype == kF16) hipLaunchKernelGGL((fa_fwd_mla_prefill_kernel<F16Traits>), grid, block, 0, stream, p);
    else return -1;
    return (int)hipGetLastError();
}

}  // namespace aule_hip
