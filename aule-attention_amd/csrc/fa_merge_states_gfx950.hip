// fa_merge_states_gfx950.hip -- merges of attention states.
//
// An attention state is the output of a query row over SOME keys together with the log of its softmax denominator; the states of
// two disjoint key sets merge into the state of their union by weighting each with exp(lse - max).  Two kernels:
//   fa_merge_states_kernel    the public two-state merge: out_a, out_b [rows, D] 16-bit, lse_a, lse_b [rows] fp32 (natural log);
//       M = max(lse_a, lse_b), w_x = exp(lse_x - M), out = (w_a out_a + w_b out_b) / (w_a + w_b), lse = M + log(w_a + w_b).
//       A side with lse = -inf holds no key: the result is the other side bit for bit; both: zeros and -inf.  The products are
//       formed before they are added (no contraction), so the result does not depend on the order of the pair.  out may alias
//       either input: a thread reads the 16 bytes it writes.  lse may not: the D / 8 threads of a row all read lse_a / lse_b and
//       for a D / 8 that does not divide 64 they sit in different waves or workgroups (the C entry refuses an overlap).
//   fa_cascade_merge_kernel   the paged cascade's: the nsplit fp32 partials of fa_fwd_paged_shared_prefix_gfx950.hip
//       (part [nsplit][T Hq][D + 2]: un-normalised O, m in log2 units, l) into the per-sequence state (out 16-bit, lse) the
//       paged prefill left, in place.  Gridded per (sequence, chunk of 8 tokens) with the prefill's clamps, so it touches exactly the
//       rows the prefill wrote: rows of no sequence are neither read nor written, whatever their partials hold.  A token at a
//       negative own position keeps its zeros and -inf; a row whose partials hold no key keeps its bits.
// One thread owns 8 elements of a row and forms the row's weights itself.  In the cascade merge (D 32 / 64 / 128: D / 8 divides 64,
// items dealt 256 at a time) the threads of a row are neighbours in one wave, so all of them have read the row's lse before one
// of them overwrites it.
#include "fa_device.h"
#include "fa_kernels.h"

namespace aule_hip {
namespace {

constexpr int kMergeTokens = 8;   // tokens per workgroup of the cascade merge

struct MergeParams {
    const char* out_a;
    const float* lse_a;
    const char* out_b;
    const float* lse_b;
    char* out;
    float* lse;
    long long rows;
    int cpr;   // 16-byte chunks per row: D / 8
};

template <class T>
__global__ void __launch_bounds__(256) fa_merge_states_kernel(const MergeParams p) {
#pragma clang fp contract(off)
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = item / p.cpr;
    if (row >= p.rows) return;
    const long long at = item * 16;   // (row * cpr + chunk) * 16 bytes
    const float la = p.lse_a[row], lb = p.lse_b[row];
    const u32x4_t a = *reinterpret_cast<const u32x4_t*>(p.out_a + at);
    const u32x4_t b = *reinterpret_cast<const u32x4_t*>(p.out_b + at);
    const float ninf = -__builtin_inff();
    u32x4_t r;
    float lo;
    if (la == ninf && lb == ninf) {
        r = u32x4_t{0u, 0u, 0u, 0u};
        lo = ninf;
    } else if (la == ninf) {
        r = b;
        lo = lb;
    } else if (lb == ninf) {
        r = a;
        lo = la;
    } else {
        const float M = fmaxf(la, lb);
        const float wa = fast_exp2((la - M) * kLog2e), wb = fast_exp2((lb - M) * kLog2e);
        const float s = wa + wb;
        const float inv = 1.f / s;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float x0 = T::lo(a[i]) * wa, y0 = T::lo(b[i]) * wb;
            const float x1 = T::hi(a[i]) * wa, y1 = T::hi(b[i]) * wb;
            r[i] = T::pack2((x0 + y0) * inv, (x1 + y1) * inv);
        }
        lo = M + fast_log2(s) * kLn2;
    }
    *reinterpret_cast<u32x4_t*>(p.out + at) = r;
    if (item % p.cpr == 0) p.lse[row] = lo;
}

struct CascadeParams {
    const float* part;
    char* out;
    float* lse;
    const int* ctx;
    const int* cu;
    long long part_stride;   // floats between the partials of two splits: T * Hq * (D + 2)
    int nsplit, nchunk;
    int T, Hq;
    int max_sq, cap;         // the prefill's clamps: n <= max_sq, L <= cap (its own table's capacity)
};

template <class T, int D>
__global__ void __launch_bounds__(256) fa_cascade_merge_kernel(const CascadeParams p) {
    constexpr int CPR = D / 8;
    const int b = (int)blockIdx.x / p.nchunk, chunk = (int)blockIdx.x % p.nchunk;
    // the sequence, clamped as the prefill clamps it (fa_device.h)
    const int L = seq_len(p.ctx, b, p.cap);
    const SeqRange own_rows = seq_range(p.cu, b, p.T, p.max_sq);
    const int s = own_rows.s, n = own_rows.n;
    const int i0 = chunk * kMergeTokens;
    if (i0 >= n) return;
    const int items = (min(n, i0 + kMergeTokens) - i0) * p.Hq * CPR;
    const float ninf = -__builtin_inff();
    for (int it = threadIdx.x; it < items; it += 256) {
        const int c = it % CPR, rr = it / CPR;
        const int i = i0 + rr / p.Hq;
        if (L - n + i < 0) continue;   // a negative own position: the prefill's zeros and -inf stay, whatever the prefix holds
        const long long row = ((long long)s + i) * p.Hq + rr % p.Hq;
        const float* pr = p.part + row * (D + 2);
        float M = ninf;
        for (int k = 0; k < p.nsplit; ++k) M = fmaxf(M, pr[k * p.part_stride + D]);
        if (M == ninf) continue;       // the prefix holds no key: the suffix state stays, bit for bit
        const float s2 = p.lse[row] * kLog2e;
        const float Mt = fmaxf(M, s2);
        // the suffix state is normalised: weight ws, denominator 1
        const float ws = s2 == ninf ? 0.f : fast_exp2(s2 - Mt);
        char* og = p.out + (row * D + 8 * c) * 2;
        const u32x4_t x = *reinterpret_cast<const u32x4_t*>(og);
        float acc[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[2 * j] = ws * T::lo(x[j]);
            acc[2 * j + 1] = ws * T::hi(x[j]);
        }
        float Lt = ws;
        for (int k = 0; k < p.nsplit; ++k) {
            const float* pk = pr + k * p.part_stride;
            const float mk = pk[D];
            if (mk == ninf) continue;   // an empty split wrote no O
            const float w = fast_exp2(mk - Mt);
            Lt += w * pk[D + 1];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2_t v = *reinterpret_cast<const f32x2_t*>(pk + 8 * c + 2 * j);   // (rows of the partial are 8-byte aligned)
                acc[2 * j] += w * v[0];
                acc[2 * j + 1] += w * v[1];
            }
        }
        const float inv = 1.f / Lt;   // (Lt >= 1: the largest m has weight 1 and l >= 1)
        *reinterpret_cast<u32x4_t*>(og) = u32x4_t{T::pack2(acc[0] * inv, acc[1] * inv), T::pack2(acc[2] * inv, acc[3] * inv),
                                                   T::pack2(acc[4] * inv, acc[5] * inv), T::pack2(acc[6] * inv, acc[7] * inv)};
        if (c == 0) p.lse[row] = (Mt + fast_log2(Lt)) * kLn2;
    }
}

template <class T>
int launch_cascade_dim(const CascadeParams& p, int D, long long nwg, hipStream_t stream) {
    if (D == 32) hipLaunchKernelGGL((fa_cascade_merge_kernel<T, 32>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else if (D == 64) hipLaunchKernelGGL((fa_cascade_merge_kernel<T, 64>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else if (D == 128) hipLaunchKernelGGL((fa_cascade_merge_kernel<T, 128>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
    else return -1;
    return (int)hipGetLastError();
}

}  // namespace

int launch_merge_states(const MergeStatesArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.D <= 0) return 0;
    if (a.D % 8 != 0) return -1;
    MergeParams p;
    p.out_a = static_cast<const char*>(a.out_a); p.lse_a = a.lse_a;
    p.out_b = static_cast<const char*>(a.out_b); p.lse_b = a.lse_b;
    p.out = static_cast<char*>(a.out); p.lse = a.lse;
    p.rows = a.rows; p.cpr = a.D / 8;
    const long long nwg = (a.rows * p.cpr + 255) / 256;
    if (nwg > 0x7fffffffll) return -1;
    return dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL(fa_merge_states_kernel<decltype(t)>, dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

// one workgroup per (sequence, chunk of kMergeTokens tokens); a chunk past the sequence's tokens leaves at once
long long cascade_merge_grid(const CascadeMergeArgs& a) {
    if (a.B <= 0 || a.max_seqlen_q <= 0 || a.T <= 0) return 0;
    return ((long long)seqlen_cut(a.max_seqlen_q, a.T) + kMergeTokens - 1) / kMergeTokens * a.B;
}

int launch_cascade_merge(const CascadeMergeArgs& a, hipStream_t stream) {
    const long long nwg = cascade_merge_grid(a);
    if (nwg <= 0 || a.Hq <= 0) return 0;
    if (nwg > 0x7fffffffll || a.nsplit <= 0 || a.part == nullptr || a.lse == nullptr) return -1;
    CascadeParams p;
    p.part = a.part; p.out = static_cast<char*>(a.out); p.lse = a.lse;
    p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.part_stride = (long long)a.T * a.Hq * (a.D + 2);
    p.nsplit = a.nsplit; p.nchunk = (int)(nwg / a.B);
    p.T = a.T; p.Hq = a.Hq;
    p.max_sq = seqlen_cut(a.max_seqlen_q, a.T); p.cap = a.own_capacity;
    return dispatch_16bit(a.dtype, [&](auto t) { return launch_cascade_dim<decltype(t)>(p, a.D, nwg, stream); });
}

}  // namespace aule_hip
