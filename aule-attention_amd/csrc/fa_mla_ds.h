// fa_mla_ds.h -- the per-128-scaled FP8 latent row and its tile for the ONE body of the absorbed MLA
// (fa_mla_common.h).  The row of a cached token is 656 bytes:
//     bytes   0 .. 511   512 e4m3fn codes of the compressed latent
//     bytes 512 .. 527   4 fp32 scales, scale g for codes 128 g .. 128 g + 127
//     bytes 528 .. 655   the 64 rotary elements as bf16, not quantised
// and the key the kernels work with is k[c] = bf16_rne(float(code[c]) * scale[c / 128]), c < 512, then the stored bf16.  Its readers:
// fa_fwd_mla_sparse_ds_gfx950.hip (the tile below); its writer: mla_kv_append_ds_gfx950.hip (the sizes alone).  fa_mla_common.h is
// included, not changed: the tile is a specialisation of its MlaTile for a cache kind of this header.  Device code only.
#pragma once
#include "fa_mla_common.h"

namespace aule_hip {
namespace {

constexpr int kDsCodes = 512;                          // quantised columns
constexpr int kDsGroup = 128;                          // columns per scale
constexpr int kDsScaleAt = kDsCodes;                   // byte offset of the 4 scales
constexpr int kDsRopeAt = kDsScaleAt + 16;             // byte offset of the 64 bf16 rotary elements
constexpr int kDsRow = kDsRopeAt + 64 * 2;             // 656 bytes, a multiple of 16
static_assert(kDsRow == 656 && kDsRow % 16 == 0, "rows of the cache are 16-byte aligned");

struct KvFp8Ds {};   // caches of 656-byte rows

// The latent tile for that cache: thread t keeps MlaTile's share of the IMAGE -- rows (t >> 3) and (t >> 3) + 32 of the 64-key tile,
// the 8-element chunks (t & 7) + 8 i, i < 9, of each -- so store() writes the very bytes the 16-bit tile writes for the dequantised
// row and everything downstream of the image is the same instruction stream.  What differs is the way there.  Per row, in flight:
//   i < 8:  8 codes at byte 8 ((t & 7) + 8 i): one 8-byte load (the eight threads of a row cover 64 consecutive bytes per i);
//   scales: ONE 16-byte load at byte 512, the same address in all eight threads of the row.  Every thread needs all four (chunk i
//           is scaled by scale[i / 2], and i runs over 0 .. 7), so the alternatives were a 4-byte load per thread plus three
//           cross-lane moves per row in store(), or this: one request that the memory pipeline serves as a broadcast of a line the
//           row's rotary load touches anyway, and no lane traffic at all.  4 registers per row;
//   i = 8:  16 bytes of bf16 at byte 528 + 16 (t & 7), stored to the image as they are.
// 2 x (16 + 4 + 4) = 48 registers hold a tile, against the 16-bit tile's 72 and the single-scale FP8 tile's 36.  A row without a slot
// is zeros, scales included (0 * 0 = +0, the image row of a skipped key).  store() converts after the next tile's loads are issued:
// v_cvt_pk_f32_fp8 (two codes -> two fp32), one v_mul_f32 each by the group's scale, and the round-to-nearest-even pack to bf16 --
// the rule above spelled out, not folded into the score scale or the accumulators: with four scales per key there is no such fold.
template <class T>
struct MlaTile<T, KvFp8Ds> {
    static_assert(std::is_same<T, Bf16Traits>::value, "the rotary part of the row is bf16 and is multiplied as stored");
    u32x2_t d[2][kMlaN - 1];
    f32x4_t sc[2];
    u32x4_t r[2];
    long long slot[2];
    __device__ __forceinline__ void lookup(const MlaListKeys& keys, int k0, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) slot[j] = keys.slot(k0 + (tid >> 3) + 32 * j);
    }
    __device__ __forceinline__ void load(const MlaParams& p, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* row = p.kv + slot[j] * kDsRow;
            const bool on = slot[j] >= 0;
#pragma unroll
            for (int i = 0; i < kMlaN - 1; ++i) d[j][i] = on ? *reinterpret_cast<const u32x2_t*>(row + (tid & 7) * 8 + 64 * i) : u32x2_t{};
            sc[j] = on ? *reinterpret_cast<const f32x4_t*>(row + kDsScaleAt) : f32x4_t{};
            r[j] = on ? *reinterpret_cast<const u32x4_t*>(row + kDsRopeAt + (tid & 7) * 16) : u32x4_t{};
        }
    }
    __device__ __forceinline__ void store(char* img, int tid) const {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            char* at = img + ((tid >> 3) + 32 * j) * kMlaPitch + (tid & 7) * 16;
#pragma unroll
            for (int i = 0; i < kMlaN - 1; ++i) {
                const float s = sc[j][i >> 1];   // chunk (t & 7) + 8 i covers columns 64 i + 8 (t & 7) ..: group i / 2
                u32x4_t x;
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[j][i][w], false);
                    const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)d[j][i][w], true);
                    x[2 * w] = T::pack2(a[0] * s, a[1] * s);
                    x[2 * w + 1] = T::pack2(b[0] * s, b[1] * s);
                }
                *reinterpret_cast<u32x4_t*>(at + 128 * i) = x;
            }
            *reinterpret_cast<u32x4_t*>(at + 128 * (kMlaN - 1)) = r[j];
        }
    }
};

}  // namespace
}  // namespace aule_hip
