// fa_fwd_mla_paged_fp8mma_gfx950.hip -- paged MLA attention over an FP8 latent cache with BOTH matrix products in FP8.
//
// The twin of fa_fwd_mla_paged_fp8_gfx950.hip (contract: aule_mla_paged_fp8_desc in include/aule.h; the clamps, the block of packed rows,
// the key ranges, the partials and the combine are the twin's: MlaBlock / MlaParams of fa_mla_common.h, launch_mla_combine).  A kernel of
// its own, not an instance of mla_paged_body: the cache's e4m3fn codes go to LDS as they are and both products run on
// v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, both block scales 1.0); the twin converts every tile to 16 bits first.
//   Q   each lane quantises its packed row (token, head) once: a = max |q[d]| over all 576 elements (the lane pair holds the two halves of
//       a wave's part, the two waves of a row half exchange theirs through LDS), s_q = a / 448 (1 when a = 0), codes =
//       e4m3(sat448(q[d] / s_q)) -- kv_quant.h's quant8 rule with a per-row scale, aule.quantize_rows_fp8's; s_q joins the lane's score
//       factor c = scale log2e kv_scale s_q (a row is a lane of S^T).
//   QK  S^T[key][row] = K.Q^T.  Wave (rh = w & 1, ch = w >> 1) owns rows 32 rh .. 32 rh + 31; 576 = 9 x 64 does not halve, so ch = 0 sums
//       over elements 0 .. 319 (5 K-steps, 10 MFMAs, 40 registers of Q codes) and ch = 1 over 320 .. 575 (4 K-steps, 8 MFMAs).  Lane (key,
//       half h) of the A operand and lane (row, half h) of the B operand both hold bytes 64 g + 32 h .. + 31 of the part for step g, so the
//       instruction's internal k order cancels.  The two waves of a row half exchange their fp32 partial sums through LDS (8 KB each, lane
//       to lane) and both add own + other, as the twin does: the same two numbers, the same bits.
//   P   p = exp2((s - m) + 8): the weights carry 2^8, so a row's largest weight is 256 <= 448 and weights down to 2^-14 of it stay normal
//       e4m3 numbers; l sums the fp32 values before rounding.  The factor leaves exactly: it cancels in O / l of a direct write, the LSE
//       takes - 8 log 2, and a partial's un-normalised O and l are multiplied by 2^-8 -- so partials mean what the twin's mean.
//   PV  O^T[d][row] += V^T.P^T, all 64 keys in ONE instruction per 32 value columns: 8 MFMAs for the wave's columns 256 ch .. + 255.  Byte b
//       of dword 4 g0 + i0 of lane half h holds key (8 g0 + 4 h + i0) + 16 b of the tile: for P the lane's own score registers
//       (sc[b >> 1][4 (g0 + 2 (b & 1)) + i0], crow's rule), for V^T what LatentCodes::store wrote.
// One read of the cache per tile, two images.  Thread t holds, of the four keys r + 16 i (r = t >> 4) -- the four whose codes share a dword
// of the PV operands -- the 8-byte units (t & 15) + 16 j, j < 4, of the value part and dword t & 15 of the 64 rotary bytes: 36 registers,
// as the twin's prefetch.  They go to LDS unconverted, twice:
//   Ks  [64 keys][pitch 592]: 37 16-byte slots, odd, so the 16 rows of a ds_read_b128 lane group fall in different slots.   37 888 B
//   Vt  [512 columns][pitch 80]: the first 512 bytes of each row transposed 4 x 4 bytes at a time with v_perm_b32 while staging
//       (DESIGN.md 3.17's scheme; against store conflicts the 16-byte slots of a row are swizzled, code_swizzle below, where 3.17 rotates
//       registers), so a PV operand is two plain ds_read_b128.                                                           40 960 B
//       (ds_read_b64_tr_b8 from Ks alone would save this image and its 32 ds_write_b32 per thread and tile, but needs four transposed
//       reads and a byte shuffle per operand in the PV chain of EVERY wave, where the transposes here are paid once per workgroup, off
//       that chain; 3.17 priced both and this kernel has the LDS: not taken.)
//   Xs  the exchange of partial scores, [wave][register quad][lane] 16 bytes, the twin's.                                  32 768 B
// 111 616 B of LDS: one workgroup per CU, 4 waves, one per SIMD, up to 512 registers each.  Per lane: 128 accumulator registers (8
// MFMA tiles of O^T), 40 of Q codes, 36 + 8 of the next tile and its slots, 32 of scores, 8 of P codes.
// Key rows at or beyond the range's last visible key are zeros in BOTH images and are never read from the cache: a NaN code times a zero
// weight is a NaN in an FP8 MFMA.  At most 18 MFMAs of 64 passes per wave and tile where the twin issues 68 of 32.
// No tree, no list, FP8 caches only.
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;

constexpr int kCodePitchK = kMlaQK + 16;      // Ks: 37 slots of 16 bytes
constexpr int kCodePitchV = kMlaKeys + 16;    // Vt: 64 key bytes + one slot
constexpr int kCodeSplit = 320;               // wave ch = 0 reduces over elements [0, 320), ch = 1 over [320, 576)
constexpr int kCodeSteps = kCodeSplit / 64;   // 5 K-steps at most

// e4m3 x e4m3 with both E8M0 block scales 127 (1.0) in every byte of the scale registers
__device__ __forceinline__ f32x16_t mfma_codes(i32x8_t a, i32x8_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}

// two 16-byte slots of LDS as one operand
__device__ __forceinline__ i32x8_t lds_codes(const char* lo, const char* up) {
    const u32x4_t a = lds_b128(lo), b = lds_b128(up);
    return i32x8_t{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

// V^T row d keeps its four 16-byte slots (16 keys each) at slot ^ code_swizzle(d).  The rows 8 cc + e + 128 j that the 16 units cc of
// a store instruction write lie 32 (cc & 1) banks apart; the swizzle spreads them over four slots more, so a wave's ds_write_b32 meets
// each bank twice (the least for 64 lanes on 32 distinct banks), with no register rotation.  A reader's 16 rows per ds_read_b128 lane
// group share one value, so its reads stay conflict-free (pitch 80: 5 slots, odd).
__device__ __forceinline__ constexpr int code_swizzle(int d) { return (d >> 4) & 3; }

// One latent tile of 64 keys of raw codes on its way from the block pool to the two images (header comment).
struct LatentCodes {
    u32x2_t v[4][4];     // [key i][unit j]: bytes 8 (cc + 16 j) .. + 7 of the row
    unsigned pe[4];      // bytes 512 + 4 cc .. + 3
    long long slot[4];   // cache slot (block * bs + offset) of this thread's rows of the tile load() takes next
    // the table walk for keys k0 .. k0 + 63, one tile ahead of the rows themselves.  A key >= kend takes key kend - 1's slot (kend >= 1:
    // the range has a tile), which load() never reads: no branch, so the four table entries are in flight together.
    __device__ __forceinline__ void lookup(const MlaParams& p, const int* tab, int k0, int kend, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kv = min(k0 + (tid >> 4) + 16 * i, kend - 1);
            const int lb = block_of(kv, p.bs, p.bs_shift);
            slot[i] = (long long)tab[lb] * p.bs + (kv - lb * p.bs);
        }
    }
    // the rows lookup() found (same k0, kend)
    __device__ __forceinline__ void load(const MlaParams& p, int k0, int kend, int tid) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kv = k0 + (tid >> 4) + 16 * i;
            const char* row = p.kv + slot[i] * kMlaQK;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = u32x2_t{};
            pe[i] = 0u;
            if (kv < kend) {   // (one branch per key row: five requests in flight behind it)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[i][j] = *reinterpret_cast<const u32x2_t*>(row + 8 * ((tid & 15) + 16 * j));
                pe[i] = *reinterpret_cast<const unsigned*>(row + kMlaV + 4 * (tid & 15));
            }
        }
    }
    __device__ __forceinline__ void store(char* Ks, char* Vt, int tid) const {
        const int r = tid >> 4, cc = tid & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            char* krow = Ks + (r + 16 * i) * kCodePitchK;
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x2_t*>(krow + 8 * (cc + 16 * j)) = v[i][j];
            *reinterpret_cast<unsigned*>(krow + kMlaV + 4 * cc) = pe[i];
        }
        // the dword of keys r + {0, 16, 32, 48} in V^T row d: lane half (r >> 2) & 1, dword 4 (r >> 3) + (r & 3) of the half -- 16-byte slot
        // 2 (r >> 2 & 1) + (r >> 3) of the row, moved to slot ^ code_swizzle(d), which is one value for all 32 rows of this thread
        char* vt = Vt + 8 * cc * kCodePitchV + 16 * ((2 * ((r >> 2) & 1) + (r >> 3)) ^ code_swizzle(8 * cc)) + 4 * (r & 3);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                // 4 x 4 byte transposes: four dwords of the codes of keys r + {0, 16, 32, 48} at columns 8 (cc + 16 j) + 4 w + (0 .. 3)
                const unsigned a0 = v[0][j][w], a1 = v[1][j][w], a2 = v[2][j][w], a3 = v[3][j][w];
                const unsigned x01l = __builtin_amdgcn_perm(a1, a0, 0x05010400u), x01h = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
                const unsigned x23l = __builtin_amdgcn_perm(a3, a2, 0x05010400u), x23h = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
                char* col = vt + (128 * j + 4 * w) * kCodePitchV;
                *reinterpret_cast<unsigned*>(col) = __builtin_amdgcn_perm(x23l, x01l, 0x05040100u);
                *reinterpret_cast<unsigned*>(col + kCodePitchV) = __builtin_amdgcn_perm(x23l, x01l, 0x07060302u);
                *reinterpret_cast<unsigned*>(col + 2 * kCodePitchV) = __builtin_amdgcn_perm(x23h, x01h, 0x05040100u);
                *reinterpret_cast<unsigned*>(col + 3 * kCodePitchV) = __builtin_amdgcn_perm(x23h, x01h, 0x07060302u);
            }
    }
};

template <class T>
__global__ void __launch_bounds__(256, 1) fa_mla_fp8mma_kernel(const MlaParams p) {
    __shared__ __attribute__((aligned(16))) char Ks[kMlaKeys * kCodePitchK];
    __shared__ __attribute__((aligned(16))) char Vt[kMlaV * kCodePitchV];
    __shared__ __attribute__((aligned(16))) char Xs[kMlaLdsScores];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rh = wave & 1, ch = wave >> 1;
    // work item: (split, rank, sequence), the sequences side by side -- the twin's grid
    const int bid = (int)blockIdx.x;
    const int b = bid % p.B, rest = bid / p.B;
    const int rank = rest % p.row_blocks, split = rest / p.row_blocks;

    const MlaBlock blk(p, b, rank);
    if (blk.rows == 0) return;
    const int L = blk.L, n = blk.n, r0 = blk.r0, rows = blk.rows;

    // this lane's row (a lane past the end works on the block's last row and stores nothing)
    const int rl = rh * 32 + l31;
    const bool live = rl < rows;
    const int r = r0 + min(rl, rows - 1);
    const int tok = r / p.Hq, head = r - tok * p.Hq;
    const int pos = L - n + tok;

    // this split's keys of this block: whole tiles of the sequence's own length, cut at the block's last visible key
    const int tiles = (L + kMlaKeys - 1) / kMlaKeys;
    const int per = (tiles + p.nsplit - 1) / p.nsplit;
    const int kbeg = split * per * kMlaKeys;
    const int kend = min(min((split + 1) * per * kMlaKeys, L), L - n + (r0 + rows - 1) / p.Hq + 1);
    const int ntiles = kend > kbeg ? (kend - kbeg + kMlaKeys - 1) / kMlaKeys : 0;
    const int* tab = p.table + (long long)b * p.max_blocks;

    // Q: the lane's 32 elements of each 64-element step of the wave's part of its row, as they lie in memory ...
    const char* qrow = p.q + (((long long)blk.s + tok) * p.q_stride + (long long)head * kMlaQK + ch * kCodeSplit) * 2 + 64 * hi;
    u32x4_t qraw[kCodeSteps][4];
    float amax = 0.f;
#pragma unroll
    for (int g = 0; g < kCodeSteps; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qraw[g][j] = g < kCodeSteps - 1 || ch == 0 ? *reinterpret_cast<const u32x4_t*>(qrow + 128 * g + 16 * j) : u32x4_t{};
#pragma unroll
            for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(__builtin_fabsf(T::lo(qraw[g][j][e])), __builtin_fabsf(T::hi(qraw[g][j][e]))));
        }
    // ... the row's largest magnitude: the lane pair, then the wave of the other part (a maximum: both hold the same bits)
    amax = fmaxf(amax, xhalf(amax));
    float* ax = reinterpret_cast<float*>(Xs);
    ax[wave * 64 + lane] = amax;
    __syncthreads();
    amax = fmaxf(amax, ax[(wave ^ 2) * 64 + lane]);
    const float sq = amax > 0.f ? amax / kFp8Max : 1.f;
    // ... and quantised with the row's own scale
    i32x8_t qc[kCodeSteps];
#pragma unroll
    for (int g = 0; g < kCodeSteps; ++g)
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const unsigned x0 = qraw[g][w >> 1][2 * (w & 1)], x1 = qraw[g][w >> 1][2 * (w & 1) + 1];
            int word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(T::lo(x0) / sq), sat448(T::hi(x0) / sq), 0, false);
            word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(T::lo(x1) / sq), sat448(T::hi(x1) / sq), word, true);
            qc[g][w] = word;
        }

    // The cache's one scale is never applied per element: it multiplies the score scale here and the accumulators on their way out.
    const float vs = *p.kv_scale;
    const float c = p.c * vs * sq;

    f32x16_t o[kMlaDT];
#pragma unroll
    for (int i = 0; i < kMlaDT; ++i) o[i] = f32x16_t{};
    float mrun = -__builtin_inff(), l = 0.f;   // running maximum (log2 units) and sum of the 2^8-scaled weights

    LatentCodes kt;
    if (ntiles > 0) {
        kt.lookup(p, tab, kbeg, kend, tid);
        kt.load(p, kbeg, kend, tid);
        kt.lookup(p, tab, kbeg + kMlaKeys, kend, tid);
    }
    char* xmine = Xs + wave * 8192 + lane * 16;
    const char* xother = Xs + (wave ^ 2) * 8192 + lane * 16;
    const char* kimg = Ks + l31 * kCodePitchK + ch * kCodeSplit + 32 * hi;
    // V^T rows 256 ch + 32 dt + l31: the swizzle is 2 (dt & 1) + (l31 >> 4); the lane's two slots 2 hi, 2 hi + 1 for either parity of dt
    const char* vrow = Vt + (256 * ch + l31) * kCodePitchV;
    int vslot[2][2];
#pragma unroll
    for (int par = 0; par < 2; ++par)
#pragma unroll
        for (int k = 0; k < 2; ++k) vslot[par][k] = 16 * ((2 * hi + k) ^ code_swizzle(32 * par + l31));
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kMlaKeys;
        __syncthreads();   // every wave is done with the previous tile and the previous partial scores (the first: with the maxima)
        kt.store(Ks, Vt, tid);
        __syncthreads();
        if (t + 1 < ntiles) {
            kt.load(p, k0 + kMlaKeys, kend, tid);
            kt.lookup(p, tab, k0 + 2 * kMlaKeys, kend, tid);
        }
        // partial S^T[key][row] over the wave's part of the reduction
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int g = 0; g < kCodeSteps - 1; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) sc[kk] = mfma_codes(lds_codes(kimg + 32 * kk * kCodePitchK + 64 * g, kimg + 32 * kk * kCodePitchK + 64 * g + 16), qc[g], sc[kk]);
        if (ch == 0) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                sc[kk] = mfma_codes(lds_codes(kimg + 32 * kk * kCodePitchK + 64 * (kCodeSteps - 1), kimg + 32 * kk * kCodePitchK + 64 * (kCodeSteps - 1) + 16), qc[kCodeSteps - 1], sc[kk]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                *reinterpret_cast<f32x4_t*>(xmine + (4 * kk + q4) * 1024) = f32x4_t{sc[kk][4 * q4], sc[kk][4 * q4 + 1], sc[kk][4 * q4 + 2], sc[kk][4 * q4 + 3]};
        __syncthreads();
        // own + other (the same two numbers in both waves: the same bits), scale to log2 units, mask, running max over the lane pair
        float mx = -__builtin_inff();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const f32x4_t y = *reinterpret_cast<const f32x4_t*>(xother + (4 * kk + q4) * 1024);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = 4 * q4 + i;
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const float x = j <= pos && j < kend ? (sc[kk][rr] + y[i]) * c : -__builtin_inff();
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
        for (int i = 0; i < kMlaDT; ++i) o[i] *= alpha;
        // the weights carry 2^8.  (s - mu) + 8 in this order: at the row's maximum the difference is exactly 0 and the weight exactly 256,
        // which s - (mu - 8) is not once mu - 8 rounds
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
        // O^T[d][row] += V^T.P^T over the wave's 256 value columns
#pragma unroll
        for (int dt = 0; dt < kMlaDT; ++dt)
            o[dt] = mfma_codes(lds_codes(vrow + 32 * dt * kCodePitchV + vslot[dt & 1][0], vrow + 32 * dt * kCodePitchV + vslot[dt & 1][1]), pb, o[dt]);
    }
    l += xhalf(l);
    if (!live) return;
    const long long orow = ((long long)blk.s + tok) * p.Hq + head;
    if (p.nsplit > 1) {
        // un-normalised O and l without the 2^8 (an exact product): the twin's partials, for the twin's combine
        const float vp = vs * 0x1p-8f;
        const long long prow = (long long)split * p.rows_total + orow;
        float* po = p.part_o + prow * kMlaV + 256 * ch;
#pragma unroll
        for (int dt = 0; dt < kMlaDT; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<f32x4_t*>(po + 32 * dt + 8 * g4 + 4 * hi) =
                    f32x4_t{o[dt][4 * g4] * vp, o[dt][4 * g4 + 1] * vp, o[dt][4 * g4 + 2] * vp, o[dt][4 * g4 + 3] * vp};
        if (ch == 0 && hi == 0) *reinterpret_cast<f32x2_t*>(p.part_ml + prow * 2) = f32x2_t{mrun, l * 0x1p-8f};
        return;
    }
    const float inv = (l > 0.f ? 1.f / l : 0.f) * vs;   // (2^8 in o over 2^8 in l)
    char* og = p.o + (orow * kMlaV + 256 * ch) * 2;
#pragma unroll
    for (int dt = 0; dt < kMlaDT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && ch == 0 && hi == 0) {
        const float mu = mrun == -__builtin_inff() ? 0.f : mrun;
        p.lse[orow] = l > 0.f ? (mu - 8.f + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

}  // namespace

// (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1; plan: mla_plan's, the twin's grid)
int launch_mla_paged_fp8mma(const MlaArgs& a, const MlaPlan& plan, void* ws, hipStream_t stream) {
    if (a.cache_kind != kCacheFp8E4M3 || a.kv_scale == nullptr || a.tree_mask != nullptr) return -1;
    MlaParams p;
    if (mla_paged_params(a, plan, ws, p) != 0) return -1;
    const int rc = dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_mla_fp8mma_kernel<decltype(t)>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
    if (rc != 0 || plan.nsplit == 1) return rc;
    return launch_mla_combine(p, plan.row_blocks, a.dtype, stream);
}

}  // namespace aule_hip
