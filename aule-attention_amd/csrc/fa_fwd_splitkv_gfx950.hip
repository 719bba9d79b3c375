// fa_fwd_splitkv_gfx950.hip -- forward for SHORT query sequences against long K/V (decode-like cross-attention,
// SURVEY.md 8d points C5b / C5c): the regime where the tiled kernels cannot fill the chip -- a 256-row Q block per
// workgroup leaves B*Hq*ceil(Sq/256) workgroups, 32 for C5b -- and the bound is HBM (K and V are read once,
// arithmetic intensity ~32 FLOP/B at Sq = 1).
//
//   * GQA/MQA packing: the Hq/Hkv query heads that share one K/V head are stacked into the ROW dimension
//     (row r of a (batch, kv-head) unit = (head r / Sq of the group, query r % Sq)), so MQA decode with 32 heads
//     is exactly one 32-row MFMA tile instead of 32 one-row problems, and K/V are streamed once per unit.
//   * split-KV: the key range is cut into chunks of `chunk_tiles` 32-key tiles, ONE WAVE per chunk (4 waves per
//     workgroup); every wave keeps its own online-softmax state and writes an un-normalised partial
//     (m, l, O) in fp32; fa_fwd_splitkv_combine merges the partials of a row (log-sum-exp merge), casts O and
//     writes LSE.  ~2048 waves are launched whatever the shape.
//   * per wave and 32-key tile: K fragments go from global memory straight into the MFMA A operand (row = key,
//     16 contiguous bytes per lane: no LDS), V goes through a wave-private LDS tile in the [kv/4][d/16][4][16]
//     sub-tile layout for ds_read_b64_tr_b16 (same layout and operand maps as fa_fwd_pp_gfx950.hip), S^T = K.Q^T
//     with a lane owning one packed row, O^T += V^T.P^T.
// Non-causal only (with the reference's top-left causal rule a short query sequence sees only its first Sq keys,
// which the tiled kernels handle).  Reference semantics: python/aule/triton_flash_amd.py:97-240 (same math,
// GQA head map :126-127).
//
// ONE kernel body serves three K/V sources: contiguous 16-bit K/V (route 4), a paged 16-bit cache and a paged cache of
// OCP FP8 e4m3fn codes (one byte per element, what gfx950 speaks; MI300X's e4m3fnuz is a different encoding) with one
// fp32 dequantisation scale per KV head:  K[pos, hk, :] = k_scale[hk] * float(k_cache[block, off, hk, :]), V likewise.
// Where the rows come from (PAGED: block table, context_lens, window) and what a row holds (Kv16 / KvFp8 below: K load
// -> MFMA operands with the matching order of d in the Q fragments, V load -> LDS image, the two scale factors) are
// the only per-source pieces; indexing, softmax step, PV step and the partial store are written once.
//
// MQ instances (fa_fwd_paged_query_kernel: both paged sources): 1 <= Sq <= 64 query tokens per sequence, the LAST Sq positions of
// the cache (speculative verify, multi-token heads, a short prompt tail).  Query qi sits at position pos = Sk - Sq + qi and sees
// key kv iff kv <= pos (and pos - kv < window): a per-lane limit, since a lane owns one packed row.  A row may see nothing of a
// tile -- or nothing at all (pos < 0) -- so the softmax step keeps m = -inf, l = 0, O = 0 for it: an empty partial.
//
// TREE instances (fa_fwd_paged_tree_kernel: the MQ instances with a tree of draft tokens instead of a chain): the row
// of query qi carries one 64-bit word; it sees every context key (kv < Sk - Sq) and new token t (key Sk - Sq + t < Sk) iff bit t of
// its word is set.  The tiles run to Sk for every row, no window; only the tiles that reach Sk - Sq test the word.  Plan, workspace
// and combine are the MQ instances'.
#include <type_traits>

#include "fa_device.h"
#include "fa_fwd_plan.h"
#include "fa_kernels.h"
#include "fa_switches.h"

namespace aule_hip {
namespace {

struct SplitParams {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;
    float* part;   // [npart][rows_total][D + 2] fp32: O (un-normalised, v_scale applied), m (log2 units), l
    int B, Hq, Hkv, Sq, Sk;
    float c;       // softmax factor in log2 units: |scale| log2(e) with the sign in Q (KV::kSignInQ), or the signed product
    int negq;
    int nrt;          // 32-row tiles per (batch, kv-head) unit
    int chunk_tiles;  // 32-key tiles per wave
    int npart;        // partials per row = 4 * gridDim.x
    int rows_total;   // B * Hkv * nrt * 32
    // paged KV cache (decode, Sq = 1; python/aule/triton_flash_amd.py:543-737): K/V = [num_blocks, block_size, Hkv, D]
    const int* block_tables;   // [B, max_blocks] physical block of each logical block
    const int* context_lens;   // [B] keys per sequence
    int block_size, max_blocks;
    int window;                // > 0: only the last `window` positions (context_len - 1 - pos < window; MQ: query position - pos < window)
    const float* k_scale;      // [Hkv] fp32, KvFp8 only
    const float* v_scale;
    const float* sinks;        // the combine's SINK instances: [Hq] fp32 sink logits; null: the plain instances
    const long long* tree_mask;   // the TREE instances: [B, Sq] words, bit t of row (b, qi) = new token t is visible
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t skv_srd(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// ---- what a K/V row holds.  A lane always loads 16 bytes; EB bytes per element decide how many elements that is. ----

// K and V in the query's 16-bit type: a 16-byte load is one MFMA operand (8 elements) and one chunk of the LDS image.
struct Kv16 {
    static constexpr int EB = 2;
    static constexpr bool kSignInQ = true;    // softmax factor |scale| log2(e), a negative scale flips the sign of Q
    // first d of Q fragment ks in lane half hi
    static __device__ __forceinline__ int q_d0(int ks, int hi) { return 16 * ks + 8 * hi; }
    // S^T += K.Q^T for one load: 8 elements, one MFMA step against the load's one Q fragment
    template <class T>
    static __device__ __forceinline__ f32x16_t qk(u32x4_t kx, const typename T::v8* qf, f32x16_t acc) {
        return T::mfma(as_v8<T>(kx), qf[0], acc);
    }
    template <class T>
    static __device__ __forceinline__ void stage_v(char* img, u32x4_t x) { *reinterpret_cast<u32x4_t*>(img) = x; }
    static __device__ __forceinline__ float k_factor(const SplitParams&, int) { return 1.f; }
    static __device__ __forceinline__ float v_factor(const SplitParams&, int) { return 1.f; }
};

// sixteen e4m3fn codes (four dwords) -> elements 0..7 and 8..15 in the 16-bit type, exact
template <class T>
__device__ __forceinline__ void cvt16(u32x4_t x, u32x4_t& e0, u32x4_t& e1) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], false);
        const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], true);
        const unsigned lo = T::pack2(a[0], a[1]), hi = T::pack2(b[0], b[1]);
        if (w < 2) {
            e0[2 * w] = lo;
            e0[2 * w + 1] = hi;
        } else {
            e1[2 * w - 4] = lo;
            e1[2 * w - 3] = hi;
        }
    }
}

// K and V as OCP e4m3fn codes.  Every finite code is exactly representable in fp16 and in bf16, so a code is converted
// to the query's 16-bit type WITHOUT its scale (v_cvt_pk_f32_fp8 + one pack: exact, NaN codes stay NaN) and the 16-bit
// MFMAs are kept -- no FP8 MFMA, no quantisation of Q or P.  The scales stay out of the loop: k_scale[hk] multiplies
// the logits, so it goes into the softmax factor (a unit is one (batch, kv-head)); v_scale[hk] multiplies the
// un-normalised O, so it is applied once where the partial is written.  Both are fp32 device values: no host
// synchronisation, capturable.
struct KvFp8 {
    static constexpr int EB = 1;
    static constexpr bool kSignInQ = false;   // softmax factor = the signed scale log2(e) * k_scale[hk]
    // A 16-byte load carries 16 elements = two MFMA k-slices, so K needs half as many loads: lane (key, hi) loads chunk
    // 2j + hi and feeds its low / high 8 elements to MFMA steps 2j / 2j + 1 -- the order of d inside the k dimension is
    // free as long as the Q fragments use the same permutation: qf[2j + e] holds d = 32j + 16hi + 8e .. +7.
    static __device__ __forceinline__ int q_d0(int ks, int hi) { return 32 * (ks >> 1) + 16 * hi + 8 * (ks & 1); }
    template <class T>
    static __device__ __forceinline__ f32x16_t qk(u32x4_t kx, const typename T::v8* qf, f32x16_t acc) {
        u32x4_t e0, e1;
        cvt16<T>(kx, e0, e1);
        return T::mfma(as_v8<T>(e1), qf[1], T::mfma(as_v8<T>(e0), qf[0], acc));
    }
    // V is converted before the LDS write (16 bytes of codes -> 32 bytes = two adjacent chunks of the sub-tiled image),
    // so the image, the transpose reads and the operand maps are the 16-bit ones.
    template <class T>
    static __device__ __forceinline__ void stage_v(char* img, u32x4_t x) {
        u32x4_t e0, e1;
        cvt16<T>(x, e0, e1);
        *reinterpret_cast<u32x4_t*>(img) = e0;
        *reinterpret_cast<u32x4_t*>(img + 16) = e1;
    }
    static __device__ __forceinline__ float k_factor(const SplitParams& p, int hk) { return p.k_scale[hk]; }
    static __device__ __forceinline__ float v_factor(const SplitParams& p, int hk) { return p.v_scale[hk]; }
};

// The body is fa_fwd_splitkv_body.inc, included by the two kernels: fa_fwd_splitkv_kernel (route 4 and the paged decode) and
// fa_fwd_paged_query_kernel (the MQ instances, a kernel name of their own).  Text, not a shared inline function: behind a call
// the compiler optimises the body before it knows the kernel arguments and schedules the decode instances differently; included,
// they stay the code they were, instruction for instruction.
template <class T, int D, class KV, bool PAGED>
__global__ void __launch_bounds__(256) fa_fwd_splitkv_kernel(const SplitParams p) {
    constexpr bool MQ = false, TREE = false;
#include "fa_fwd_splitkv_body.inc"
}

template <class T, int D, class KV>
__global__ void __launch_bounds__(256) fa_fwd_paged_query_kernel(const SplitParams p) {
    constexpr bool PAGED = true, MQ = true, TREE = false;
#include "fa_fwd_splitkv_body.inc"
}

template <class T, int D, class KV>
__global__ void __launch_bounds__(256) fa_fwd_paged_tree_kernel(const SplitParams p) {
    constexpr bool PAGED = true, MQ = true, TREE = true;
#include "fa_fwd_splitkv_body.inc"
}

// One workgroup per packed row: log-sum-exp merge of the row's partials (there can be hundreds -- a serial loop per
// thread made this kernel, not the split kernel, the bottleneck: 230 us for C5b), cast, LSE.  Threads are arranged as
// G groups x D/4 column chunks; group j merges partials j, j+G, ...; the groups are then summed through LDS.
// SINK: the head's sink logit is one more partial with m = sinks[head] log2 e, l = 1 and O = 0: it enters the maximum M and the sum;
// a logit of -inf leaves M and the sum their bits, and a row whose partials hold no key gets lse = the logit itself.
template <class T, int D, bool SINK>
__global__ void __launch_bounds__(256) fa_fwd_splitkv_combine(const SplitParams p) {
    constexpr int C4 = D / 4, G = 256 / C4;
    __shared__ float red[256];
    __shared__ __attribute__((aligned(16))) float accs[G][D];
    __shared__ float lsum[G];
    const int prow = blockIdx.x, tid = threadIdx.x;
    const int g = p.Hq / p.Hkv;
    const int unit = prow / (p.nrt * 32), row = prow % (p.nrt * 32);
    if (row >= g * p.Sq) return;
    const int b = unit / p.Hkv, hk = unit % p.Hkv, head = hk * g + row / p.Sq, qi = row % p.Sq;
    const float* base = p.part + (size_t)prow * (D + 2);
    const size_t pstride = (size_t)p.rows_total * (D + 2);
    // M = max over the partials' maxima
    float mx = -INFINITY;
    for (int i = tid; i < p.npart; i += 256) mx = fmaxf(mx, base[i * pstride + D]);
    red[tid] = mx;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] = fmaxf(red[tid], red[tid + st]);
        __syncthreads();
    }
    const float Mk = red[0];   // of the keys
    float M = Mk, s2 = -INFINITY, sink = -INFINITY;
    if constexpr (SINK) {
        sink = p.sinks[head];
        s2 = sink * kLog2e;
        M = fmaxf(Mk, s2);
    }
    const int grp = tid / C4, c4 = tid % C4;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
#pragma unroll 8
    for (int i = grp; i < p.npart; i += G) {
        const float* src = base + i * pstride;
        const float w = (M == -INFINITY) ? 0.f : fast_exp2(src[D] - M);   // empty partial: m = -inf -> 0
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(src + 4 * c4);
        acc += x * w;
        if (c4 == 0) L += w * src[D + 1];
    }
    *reinterpret_cast<f32x4_t*>(&accs[grp][4 * c4]) = acc;
    if (c4 == 0) lsum[grp] = L;
    __syncthreads();
    if (tid < C4) {
        f32x4_t t = {0.f, 0.f, 0.f, 0.f};
        float Lt = 0.f;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            t += *reinterpret_cast<const f32x4_t*>(&accs[j][4 * tid]);
            Lt += lsum[j];
        }
        if constexpr (SINK) Lt += (M == -INFINITY) ? 0.f : fast_exp2(s2 - M);
        const float inv = Lt > 0.f ? 1.0f / Lt : 0.f;   // paged: a sequence with context_len 0 has no key -> O = 0
        const size_t orow = ((size_t)(b * p.Hq + head) * p.Sq + qi);
        u32x2_t u;
        u[0] = T::pack2(t[0] * inv, t[1] * inv);
        u[1] = T::pack2(t[2] * inv, t[3] * inv);
        *reinterpret_cast<u32x2_t*>(reinterpret_cast<char*>(p.o) + orow * (D * 2) + tid * 8) = u;
        if (tid == 0 && p.lse != nullptr) {
            if (SINK && Mk == -INFINITY) p.lse[orow] = sink;   // (no key: the logit itself)
            else p.lse[orow] = Lt > 0.f ? (M + fast_log2(Lt)) * kLn2 : -INFINITY;   // (a row that sees no key)
        }
    }
}

// Combine for FEW partials per row (the tiled kernel's SPLIT instances leave at most a few dozen): one WAVE per packed
// row, four rows per workgroup, no LDS and no block-wide reduction.  Lane i first weighs partial i (w_i = 2^(m_i - M),
// M the row's maximum; wave reductions), then every lane accumulates its D/64 columns over the partials with w_i
// broadcast from lane i.  The one-workgroup-per-row kernel above spends 256 threads and two block reductions on a row
// with 4 partials: 26 us for B8 Hq32 Hkv8 Sq64 (34 MB, 1.3 TB/s) -- a quarter of that shape's time.  Used for <= 16
// partials per row only: beyond that the serial walk over the partials is slower than the kernel above.  SINK: as above, the sink
// merged after the last trip.
template <class T, int D, bool SINK>
__global__ void __launch_bounds__(256) fa_fwd_splitkv_combine_rows(const SplitParams p) {
    constexpr int CPL = (D + 63) / 64;            // columns per lane (D = 32: lanes 32..63 carry no column)
    const int lane = threadIdx.x & 63;
    const int prow = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (prow >= p.rows_total) return;
    const int g = p.Hq / p.Hkv;
    const int unit = prow / (p.nrt * 32), row = prow % (p.nrt * 32);
    if (row >= g * p.Sq) return;
    const int b = unit / p.Hkv, hk = unit % p.Hkv, head = hk * g + row / p.Sq, qi = row % p.Sq;
    const float* base = p.part + (size_t)prow * (D + 2);
    const size_t pstride = (size_t)p.rows_total * (D + 2);
    float acc[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
    float L = 0.f, M = -INFINITY;
    const bool has_col = lane * CPL < D;
    for (int i0 = 0; i0 < p.npart; i0 += 64) {     // (one trip unless there are more than 64 partials)
        const int n = min(64, p.npart - i0);
        const float mi = lane < n ? base[(size_t)(i0 + lane) * pstride + D] : -INFINITY;
        const float li = lane < n ? base[(size_t)(i0 + lane) * pstride + D + 1] : 0.f;
        float mx = mi;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float Mn = fmaxf(M, mx);
        const float rescale = (M == -INFINITY) ? 0.f : fast_exp2(M - Mn);   // earlier trips (if any) move to the new maximum
        const float w = (mi == -INFINITY) ? 0.f : fast_exp2(mi - Mn);       // empty partial: weight 0
        float wl = w * li;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) wl += __shfl_xor(wl, o, 64);
        L = L * rescale + wl;
#pragma unroll
        for (int c = 0; c < CPL; ++c) acc[c] *= rescale;
        M = Mn;
        for (int i = 0; i < n; ++i) {
            const float wi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), i));
            if (has_col) {
                const float* src = base + (size_t)(i0 + i) * pstride + lane * CPL;
#pragma unroll
                for (int c = 0; c < CPL; ++c) acc[c] += wi * src[c];
            }
        }
    }
    const bool no_key = M == -INFINITY;
    float sink = -INFINITY;
    if constexpr (SINK) {
        sink = p.sinks[head];
        const float s2 = sink * kLog2e;
        const float Mn = fmaxf(M, s2);
        const float rescale = (M == -INFINITY) ? 0.f : fast_exp2(M - Mn);   // s2 = -inf: exactly 1
        L = L * rescale + ((Mn == -INFINITY) ? 0.f : fast_exp2(s2 - Mn));
#pragma unroll
        for (int c = 0; c < CPL; ++c) acc[c] *= rescale;
        M = Mn;
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
    const size_t orow = ((size_t)(b * p.Hq + head) * p.Sq + qi);
    if (has_col) {
        if constexpr (CPL == 2) {
            reinterpret_cast<unsigned*>(p.o)[orow * (D / 2) + lane] = T::pack2(acc[0] * inv, acc[1] * inv);
        } else {
            const unsigned u = T::pack2(acc[0] * inv, 0.f);
            reinterpret_cast<unsigned short*>(p.o)[orow * D + lane] = (unsigned short)(u & 0xffffu);
        }
    }
    if (lane == 0 && p.lse != nullptr) {
        if (SINK && no_key) p.lse[orow] = sink;   // (no key: the logit itself)
        else p.lse[orow] = L > 0.f ? (M + fast_log2(L)) * kLn2 : -INFINITY;
    }
}

// ---- host side ----

// (dtype, D) -> instance: f(traits, std::integral_constant<int, D>), or -1 for a combination this family does not have
template <class F>
int for_dtype_d(int dtype, int D, F&& f) {
    auto by_d = [&](auto t) -> int {
        if (D == 128) return f(t, std::integral_constant<int, 128>{});
        if (D == 64) return f(t, std::integral_constant<int, 64>{});
        if (D == 32) return f(t, std::integral_constant<int, 32>{});
        return -1;
    };
    if (dtype == kBF16) return by_d(Bf16Traits{});
    if (dtype == kF16) return by_d(F16Traits{});
    return -1;
}

// Merge the partials `p` describes.  Same-box A/B (tools/combine_ab.py, two passes): with <= 16 partials per row the
// wave-per-row kernel is ahead or level (B8 Hq32 Hkv8 Sq64 Sk8192 101 -> 87 us, B4 Sq128 Sk4096 65.5 -> 52.4 us); with
// >= 32 its serial walk over the partials loses to the kernel that spreads them over thread groups (C5b 21.7 -> 29.0 us,
// C5c 29.8 -> 36.2 us).  `by_count` = false: the workgroup-per-row kernel whatever the count.
template <class T, int D>
int launch_combine(const SplitParams& p, bool by_count, hipStream_t stream) {
    // (AULE_HIP_FWD_COMBINE=wg selects the workgroup-per-row kernel: A/B measurements)
    const bool rows = by_count && !switches().fwd_combine_wg && p.npart <= 16;
    const dim3 grid(rows ? (unsigned)((p.rows_total + 3) / 4) : (unsigned)p.rows_total);
    if (p.sinks != nullptr) {   // (the paged query with sink logits)
        if (rows) hipLaunchKernelGGL((fa_fwd_splitkv_combine_rows<T, D, true>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_splitkv_combine<T, D, true>), grid, dim3(256), 0, stream, p);
    } else {
        if (rows) hipLaunchKernelGGL((fa_fwd_splitkv_combine_rows<T, D, false>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_splitkv_combine<T, D, false>), grid, dim3(256), 0, stream, p);
    }
    return (int)hipGetLastError();
}

// The wave-per-chunk launch: workspace, split kernel, combine.  `p` arrives with the tensors, B / Hq / Hkv / Sq, the scale and
// the paged fields set; `w` is wave_chunk_plan() of the problem.
template <class T, int D, class KV, bool PAGED, bool MQ = false>
int launch_wave_chunk(SplitParams p, const WaveChunkPlan& w, void* user_ws, uint64_t user_ws_bytes, bool combine_by_count, hipStream_t stream) {
    p.nrt = w.nrt; p.chunk_tiles = w.chunk_tiles; p.npart = w.npart; p.rows_total = w.rows_total;
    ScopedWorkspace ws(w.bytes(D), user_ws, user_ws_bytes, stream);   // caller's buffer, or stream-ordered (safe with concurrent streams)
    if (ws.err != hipSuccess) return (int)ws.err;
    p.part = static_cast<float*>(ws.ptr);
    const dim3 grid((unsigned)w.nsplit, (unsigned)(w.rows_total / 32));
    if constexpr (MQ) {
        if (p.tree_mask != nullptr) hipLaunchKernelGGL((fa_fwd_paged_tree_kernel<T, D, KV>), grid, dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_paged_query_kernel<T, D, KV>), grid, dim3(256), 0, stream, p);
    }
    else hipLaunchKernelGGL((fa_fwd_splitkv_kernel<T, D, KV, PAGED>), grid, dim3(256), 0, stream, p);
    const int rc = (int)hipGetLastError();
    return rc != 0 ? rc : launch_combine<T, D>(p, combine_by_count, stream);
}

// Scale convention of the 16-bit sources: |scale| log2(e) in the kernel, the sign in Q, 0 replaced by 1e-30.
void set_abs_scale(SplitParams& p, float scale) {
    const float c = scale * kLog2e;
    p.negq = c < 0.f;
    p.c = c < 0.f ? -c : c;
    if (p.c == 0.f) p.c = 1e-30f;
}

template <class T, int D>
int launch_split(const FwdArgs& a, const WaveChunkPlan& w, hipStream_t stream) {
    SplitParams p = {};
    p.q = a.q; p.k = a.k; p.v = a.v; p.o = a.o; p.lse = a.lse;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = a.Sq; p.Sk = a.Sk;
    set_abs_scale(p, a.scale);
    return launch_wave_chunk<T, D, Kv16, false>(p, w, a.ws, a.ws_bytes, false, stream);
}

// (PagedArgs::Sq is 1 for the decode; the launch and the size query of either paged call plan here)
static WaveChunkPlan paged_plan(const PagedArgs& a) { return wave_chunk_plan(a.B, a.Hq, a.Hkv, a.Sq, a.max_blocks * a.block_size); }

// Paged decode: one query token per sequence, K/V gathered through the block table; the key range is bounded by
// max_blocks * block_size on the host (no device->host sync for max(context_lens)); waves past a sequence's
// context_len leave an empty partial.  MQ: the paged query, PagedArgs::Sq tokens per sequence and an optional LSE.
template <class T, int D, class KV, bool MQ>
int launch_paged(const PagedArgs& a, hipStream_t stream) {
    SplitParams p = {};
    p.q = a.q; p.k = a.k_cache; p.v = a.v_cache; p.o = a.out; p.lse = MQ ? a.lse : nullptr;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = MQ ? a.Sq : 1; p.Sk = a.max_blocks * a.block_size;
    p.block_tables = a.block_tables; p.context_lens = a.context_lens;
    p.block_size = a.block_size; p.max_blocks = a.max_blocks; p.window = a.window > 0 ? a.window : 0;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.sinks = MQ ? a.sinks : nullptr;
    p.tree_mask = MQ ? a.tree_mask : nullptr;
    // The two cache kinds differ in two places beyond the data format.  Both differences reach the results (the last
    // bits, or which kernel runs), so each is kept as it was introduced; making them one is a change of its own.
    //  * scale (KV::kSignInQ): the 16-bit cache takes the contiguous kernel's convention (set_abs_scale); the FP8 cache
    //    passes the signed product, which the kernel multiplies by k_scale[hk].
    if (KV::kSignInQ) set_abs_scale(p, a.scale);
    else p.c = a.scale * kLog2e;
    //  * combine: the 16-bit cache always merges with the workgroup-per-row kernel; the FP8 cache picks by the number
    //    of partials (and honours AULE_HIP_FWD_COMBINE), as launch_splitkv_combine does.
    return launch_wave_chunk<T, D, KV, true, MQ>(p, paged_plan(a), a.ws, a.ws_bytes, /*combine_by_count=*/std::is_same<KV, KvFp8>::value, stream);
}

template <bool MQ>
int launch_paged_kind(const PagedArgs& a, hipStream_t stream) {
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 && (a.k_scale == nullptr || a.v_scale == nullptr)) return -1;
    return for_dtype_d(a.dtype, a.D, [&](auto t, auto d) {
        using T = decltype(t);
        constexpr int D = decltype(d)::value;
        return fp8 ? launch_paged<T, D, KvFp8, MQ>(a, stream) : launch_paged<T, D, Kv16, MQ>(a, stream);
    });
}

}  // namespace

// The plan of the wave-per-chunk launch (route 4, the paged decode and its size query): B * Hkv units of Hq / Hkv * Sq packed rows
// each, cut into 32-row tiles; the key tiles are shared out so that about 2048 waves (~8 per CU) are launched whatever the shape
// and whatever the bytes per key.  `Sk` bounds the key range on the host.
WaveChunkPlan wave_chunk_plan(int B, int Hq, int Hkv, int Sq, int Sk) {
    WaveChunkPlan w;
    w.nrt = (Hq / Hkv * Sq + 31) / 32;
    const int units = B * Hkv * w.nrt;
    const int ntiles = (Sk + 31) / 32;
    const int want_waves = (2048 + units - 1) / (units > 0 ? units : 1);   // (units may be 0)
    w.chunk_tiles = (ntiles + want_waves - 1) / want_waves;
    if (w.chunk_tiles < 1) w.chunk_tiles = 1;
    const int nwaves = (ntiles + w.chunk_tiles - 1) / w.chunk_tiles;
    w.nsplit = (nwaves + 3) / 4;
    w.npart = w.nsplit * 4;
    w.rows_total = units * 32;
    return w;
}

int launch_fwd_splitkv(const FwdArgs& a, const WaveChunkPlan& w, hipStream_t stream) {
    return for_dtype_d(a.dtype, a.D, [&](auto t, auto d) { return launch_split<decltype(t), decltype(d)::value>(a, w, stream); });
}

// cache_kind selects the K/V source; an FP8 cache needs its two scale arrays
int launch_paged_decode(const PagedArgs& a, hipStream_t stream) { return launch_paged_kind<false>(a, stream); }

// PagedArgs::Sq query tokens per sequence (1 .. 64: the packed-row bound of this kernel family), PagedArgs::lse optional
int launch_paged_query(const PagedArgs& a, hipStream_t stream) {
    if (a.Sq < 1 || a.Sq > 64) return -1;
    if (a.tree_mask != nullptr && (a.window > 0 || a.sinks != nullptr)) return -1;   // (neither is defined over a tree)
    return launch_paged_kind<true>(a, stream);
}

// the bytes of the plan the two launchers above run (0: a (dtype, D, Sq) they refuse)
uint64_t paged_workspace_bytes(const PagedArgs& a) {
    if ((a.dtype != kBF16 && a.dtype != kF16) || (a.D != 128 && a.D != 64 && a.D != 32) || a.Sq < 1 || a.Sq > 64) return 0;
    return paged_plan(a).bytes(a.D);
}

// The combine pass on its own, for partials written by another kernel (fa_fwd_pp_gfx950.hip SPLIT instances) in
// the same layout: part [npart][B*Hkv*nrt*32][D + 2] fp32, packed row r of a unit = (head r / Sq of the group, query r % Sq).
int launch_splitkv_combine(const FwdArgs& a, float* part, int npart, int nrt, hipStream_t stream) {
    SplitParams p = {};
    p.o = a.o; p.lse = a.lse; p.part = part;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = a.Sq; p.Sk = a.Sk;
    p.nrt = nrt; p.npart = npart;
    p.rows_total = a.B * a.Hkv * nrt * 32;
    return for_dtype_d(a.dtype, a.D, [&](auto t, auto d) { return launch_combine<decltype(t), decltype(d)::value>(p, true, stream); });
}

#ifndef AULE_SPLITKV_MAX_UNITS
#define AULE_SPLITKV_MAX_UNITS 128   // (A/B builds override it: tools/split_ab.py)
#endif
// Shapes the split-KV path takes over from the tiled kernels: 16-bit, non-causal, no window, short queries against
// long K/V -- few enough Q blocks that the tiled kernels would leave most CUs idle.
bool splitkv_applicable(const FwdArgs& a) {
    if (a.dtype != kBF16 && a.dtype != kF16) return false;
    if (a.causal || a.window > 0) return false;
    if (a.D != 32 && a.D != 64 && a.D != 128) return false;
    if (a.Sq > 64 || a.Sk < 1024) return false;
    const long long tiled_wgs = (long long)a.B * a.Hq * ((a.Sq + 255) / 256);
    if (tiled_wgs >= 512) return false;   // two workgroups per CU: the tiled kernel fills the chip
    // K/V is streamed once per 32-row tile of packed rows, so `units` of them re-read it that many times and every
    // one adds partials to combine.  Measured (tools/split_grid.py, bf16 D128, Sk 2048 / 8192): units <= 128 wins
    // in every case (2-8x at B = 1); units = 256 is break-even (-20..25 % at Sk 2048, +4..7 % at 8192); units >= 512
    // loses (B8 Hq32 Hkv8 Sq64 Sk8192: 318 vs 194 us).
    const int g = a.Hq / a.Hkv;
    const long long units = (long long)a.B * a.Hkv * ((g * a.Sq + 31) / 32);
    return units <= AULE_SPLITKV_MAX_UNITS;
}

}  // namespace aule_hip
