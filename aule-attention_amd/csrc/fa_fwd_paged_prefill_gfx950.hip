// fa_fwd_paged_prefill_gfx950.hip -- paged prefill: ragged per-sequence queries against the paged KV cache.
//
// The step of a continuous-batching engine: sequence b brings n_b new tokens (a prompt chunk behind a cached prefix, a short
// verify, a plain decode), packed along the first axis of q [T, Hq, D]; K / V live in the block pool
// [num_blocks, block_size, Hkv, D] behind block_tables [B, max_blocks].  Everything per sequence is read and clamped HERE:
//     L = clamp(context_lens[b], 0, max_blocks * block_size)        s = clamp(cu[b], 0, T)      e = clamp(cu[b + 1], s, T)
//     n = min(e - s, max_seqlen_q);   token i < n is row s + i of q / out and sits at position p = L - n + i;
//     it sees key j iff j <= p (and p - j < window when a window is set): the bottom-right rule of the paged query.
// so a stale length or offset cannot index outside a buffer, and rows of out / lse outside every [s, s + n) are never written.
//
// Layout: the plain one of fa_fwd_d256_gfx950.hip / fa_d256_common.h, generalised over D:
//   workgroup = (sequence, KV head, block of 128 PACKED rows), 4 waves x 32 rows, one wave per SIMD.  Packing is token-major:
//   packed row r = token r / g, head hk g + r % g (g = Hq / Hkv) -- the g heads of a token are contiguous in [T, Hq, D], positions
//   are monotone in r (a block's keys are one interval), K / V of a KV head stream once per 128 / g tokens x g heads;
//   Q of the lane's row in registers, K / V tiles of 64 keys in LDS, the next tile prefetched into registers while this one is
//   computed; S^T[key][row] = K.Q^T (2 accumulators), P^T as the B operand of O^T[d][row] += V^T.P^T (D / 32 accumulators).
// Key row kv of the sequence is row ((table[b][kv / bs] * bs + kv % bs) * Hkv + hk) * D of the cache (64-bit; a shift when bs is a
// power of two); rows at or beyond the block's last visible key are not read (zeros in LDS), table entries past them not touched.
// FP8 caches: eight e4m3fn codes become one 16-byte chunk of q's 16-bit type on the way into LDS (exact), k_scale[hk] goes into the
// log2-unit score factor and v_scale[hk] into the epilogue, so the MFMA loop is one family.
// Online softmax in log2 units with fp32 m, l, acc; a row without a visible key writes O = 0 and LSE = -inf (PagedPrefillArgs::sinks
// given: LSE = the head's sink logit).
// One launch, no workspace: grid = ceil(max_seqlen_q g / 128) x Hkv x B, decoded as (rank, sequence, KV head) with rank 0 the
// sequence's own last (heaviest) block; a workgroup whose rank is past the sequence's blocks leaves before it touches the table or
// the caches.  The table is walked one tile ahead of the K / V loads, which are one tile ahead of the MFMAs.
//
// The kernel body is written ONCE, in the first part of this file, and compiled into two kernels: fa_fwd_paged_prefill_kernel (TREE = false)
// and fa_fwd_paged_prefill_tree_kernel (TREE = true) each include this file again with AULE_PAGED_PREFILL_BODY defined,
// which yields the body alone.  Text, not a shared inline function, for the reason fa_fwd_splitkv_gfx950.hip gives: as a force-inlined
// template the same statements compiled the existing instances to other register counts and schedules; included, they stay the code
// they were, instruction for instruction (profiles/tree_resources.txt).
#ifdef AULE_PAGED_PREFILL_BODY
// ---- the body.  In scope: T, D, KV, the constant TREE and the kernel argument `const PrefillParams p`.
    using C = PrefillCfg<D>;
    constexpr bool FP8 = std::is_same<KV, KvFp8>::value;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PA];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work item: rank i of (sequence, KV head) unit `unit`, the units side by side (with Hkv % 8 == 0 a KV head stays on one XCD)
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int hk = unit % p.Hkv, b = unit / p.Hkv;

    // the sequence, clamped (fa_device.h)
    const int L = seq_len(p.ctx, b, p.max_blocks * p.bs);   // (the capacity < 2^30: the host checks)
    const SeqRange own_rows = seq_range(p.cu, b, p.T, p.max_sq);
    const int s = own_rows.s, n = own_rows.n;
    const int R = n * p.g;   // packed rows of this (sequence, KV head); T * g < 2^31: the host checks
    // rank 0 is the sequence's last (heaviest) block, whatever its length: the one block of a decode starts with the first wave of
    // workgroups, beside the last block of a long chunk
    const int own = (R + kPQ - 1) / kPQ;
    if (rank >= own) return;
    const int r0 = (own - 1 - rank) * kPQ;
    const int rows = min(kPQ, R - r0);   // of this block, >= 1

    // this lane's row (a lane past the end works on the block's last row and stores nothing)
    const int rl = wave * 32 + l31;
    const bool live = rl < rows;
    const int r = r0 + min(rl, rows - 1);
    const int tok = r / p.g, head = hk * p.g + r % p.g;
    const int pos = L - n + tok;
    // wave-uniform position ranges: the block's decide the tiles, the wave's the tiles it computes and the unmasked path
    const int bpos_lo = L - n + r0 / p.g, bpos_hi = L - n + (r0 + rows - 1) / p.g;
    const bool wave_live = wave * 32 < rows;
    const int wpos_lo = L - n + (r0 + min(wave * 32, rows - 1)) / p.g;
    const int wpos_hi = L - n + (r0 + min(wave * 32 + 31, rows - 1)) / p.g;

    // TREE: a sequence of at most 64 new tokens carries a tree (wave-uniform: n is); a longer one keeps the causal rule.  The lane's word,
    // bit t = new token t (key L - n + t) is visible, as two halves; a row at a negative position sees nothing (L < n: no context key)
    bool tree = false;
    unsigned tree_lo = 0u, tree_hi = 0u;
    if constexpr (TREE) {
        tree = n <= 64;
        if (tree && pos >= 0) {
            const unsigned long long w = (unsigned long long)p.tree_mask[(long long)s + tok];
            tree_lo = (unsigned)w;
            tree_hi = (unsigned)(w >> 32);
        }
    }

    const int kend = tree ? L : bpos_hi + 1;   // <= L (a node may see a new token behind its own position)
    const int kbeg = p.window > 0 ? max(0, bpos_lo - p.window + 1) / kPK * kPK : 0;
    const int ntiles = kend > kbeg ? (kend - kbeg + kPK - 1) / kPK : 0;
    const int* tab = p.table + (long long)b * p.max_blocks;

    // Q operand chunks of this lane's row
    const char* qrow = p.q + (((long long)s + tok) * p.q_stride + (long long)head * D) * 2;
    u32x4_t qf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    float c = p.c;
    if constexpr (FP8) c *= p.k_scale[hk];

    f32x16_t o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    PagedTile<T, D, FP8> kt;
    if (ntiles > 0) {
        kt.lookup(p, tab, kbeg, kend, tid);
        kt.load(p, hk, kbeg, kend, tid);
        kt.lookup(p, tab, kbeg + kPK, kend, tid);
    }
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, Vs, tid);
        __syncthreads();
        if (t + 1 < ntiles) {
            kt.load(p, hk, k0 + kPK, kend, tid);
            kt.lookup(p, tab, k0 + 2 * kPK, kend, tid);
        }
        // a wave skips the tiles none of its rows sees: all keys after its last position, or all before its window
        if (!wave_live || (!tree && k0 > wpos_hi) || (p.window > 0 && k0 + kPK - 1 < wpos_lo - p.window + 1)) continue;
        // S^T[key][row] = K.Q^T over the 64 keys of the tile
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int g = 0; g < C::G; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                sc[kk] = mfma16<T>(lds_b128(Ks + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), qf[g], sc[kk]);
        // scale to log2 units, mask, running max over the lane pair (lanes l and l + 32 hold the same row)
        float mx = -__builtin_inff();
        // every row sees every key of the tile (a tree: the tile lies below the new tokens)
        const bool full = tree ? k0 + kPK - 1 < L - n : (k0 + kPK - 1 <= wpos_lo && (p.window <= 0 || wpos_hi - k0 < p.window));
        if (full) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float x = sc[kk][rr] * c;
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
                }
        } else if (tree) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const int bit = j - (L - n);   // of the word: a context key (bit < 0) is visible, a new token iff it lies below L and its bit is set
                    const unsigned half = (bit & 32) ? tree_hi : tree_lo;
                    const bool see = bit < 0 || (j < L && ((half >> (bit & 31)) & 1u) != 0u);
                    const float x = see ? sc[kk][rr] * c : -__builtin_inff();
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
                }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const bool see = j <= pos && (p.window <= 0 || pos - j < p.window);
                    const float x = see ? sc[kk][rr] * c : -__builtin_inff();
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
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
    if (!live) return;
    float inv = l > 0.f ? 1.f / l : 0.f;
    // sink logits (a wave-uniform pointer; null: the line above is the whole story): the head's logit joins the denominator
    const bool sink = p.sinks != nullptr;
    float sink_lse = 0.f;
    if (sink) sink_lse = sink_epilogue(p.sinks[head], m, l, inv);
    if constexpr (FP8) inv *= p.v_scale[hk];
    const long long orow = ((long long)s + tok) * p.Hq + head;
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
#else
// ---- the file proper
#include "fa_kernels.h"
#include "fa_tile_attention.h"

namespace aule_hip {
namespace {

struct PrefillParams {
    const char* q;
    const char* k;
    const char* v;
    char* o;
    float* lse;
    const int* table;
    const int* ctx;
    const int* cu;
    const float* k_scale;
    const float* v_scale;
    const float* sinks;   // [Hq] fp32 sink logits or null
    long long q_stride;   // elements between tokens of q
    int T, B, Hq, Hkv, g;
    int bs, bs_shift;     // bs_shift >= 0: bs = 1 << bs_shift
    int max_blocks, max_sq;
    float c;              // scale * log2(e) (sign kept)
    int window;           // > 0: on
    // (last: the fields above keep the kernel-argument offsets the existing instances were compiled with)
    const long long* tree_mask;   // the TREE instances: [T] words, bit t of token s + i = new token t of its sequence is visible
};

#define AULE_PAGED_PREFILL_BODY
template <class T, int D, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_prefill_kernel(const PrefillParams p) {
    constexpr bool TREE = false;
#include "fa_fwd_paged_prefill_gfx950.hip"
}

// The TREE instances (PagedPrefillArgs::tree_mask given).  A sequence with n <= 64 new tokens carries a tree: every block of it walks the
// keys up to L, the tiles below L - n keep the unmasked path and the others test the lane's word.  A longer sequence is the kernel above.
template <class T, int D, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_prefill_tree_kernel(const PrefillParams p) {
    constexpr bool TREE = true;
#include "fa_fwd_paged_prefill_gfx950.hip"
}
#undef AULE_PAGED_PREFILL_BODY

}  // namespace

// The grid rule: ceil(max_seqlen_q * g / 128) blocks per (sequence, KV head); the kernel decodes (rank, sequence, KV head) from
// the 1-D index, KV head fastest, rank r = the sequence's own block count - 1 - r.
long long paged_prefill_blocks_per_unit(const PagedPrefillArgs& a) {
    if (a.Hkv <= 0 || a.max_seqlen_q <= 0) return 0;
    return ((long long)seqlen_cut(a.max_seqlen_q, a.T) * (a.Hq / a.Hkv) + kPQ - 1) / kPQ;
}

long long paged_prefill_grid(const PagedPrefillArgs& a) {
    return paged_prefill_blocks_per_unit(a) * a.Hkv * a.B;
}

int launch_paged_prefill(const PagedPrefillArgs& a, hipStream_t stream) {
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (a.cache_kind != kCache16 && !fp8) return -1;
    if (fp8 && (a.k_scale == nullptr || a.v_scale == nullptr)) return -1;
    if (a.tree_mask != nullptr && (a.window > 0 || a.sinks != nullptr)) return -1;   // (neither is defined over a tree)
    if (a.Hkv <= 0 || a.Hq % a.Hkv != 0 || a.block_size <= 0 || a.max_blocks <= 0) return -1;
    if ((long long)a.block_size * a.max_blocks >= (1ll << 30)) return -1;
    if (a.q_token_stride < (long long)a.Hq * a.D || a.q_token_stride % 8 != 0) return -1;
    const long long nwg = paged_prefill_grid(a);
    if (nwg <= 0 || a.T <= 0) return 0;
    // the kernel counts packed rows in 32 bits
    if (nwg > 0x7fffffffll || ((long long)a.T + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;
    PrefillParams p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k_cache); p.v = static_cast<const char*>(a.v_cache);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    p.table = a.block_tables; p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale; p.sinks = a.sinks; p.tree_mask = a.tree_mask;
    p.q_stride = a.q_token_stride;
    p.T = a.T; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv;
    p.bs = a.block_size;
    p.bs_shift = shift_of(a.block_size);
    p.max_blocks = a.max_blocks; p.max_sq = seqlen_cut(a.max_seqlen_q, a.T);
    p.c = a.scale * kLog2e;
    p.window = a.window > 0 ? a.window : 0;
    return dispatch_tile_instance(a.dtype, a.D, fp8, [&](auto t, auto d, auto kv) {
        if (a.tree_mask != nullptr) hipLaunchKernelGGL((fa_fwd_paged_prefill_tree_kernel<decltype(t), decltype(d)::value, decltype(kv)>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_paged_prefill_kernel<decltype(t), decltype(d)::value, decltype(kv)>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
#endif   // AULE_PAGED_PREFILL_BODY
