// kv_quant.h -- what the cache append kernels share (kv_append_gfx950.hip, mla_kv_append_gfx950.hip): a 16-byte chunk of eight
// 16-bit elements and its way into a cache, as a copy of the bits or as eight e4m3fn codes.  The quantisation rules are stated in
// kv_append_gfx950.hip's header comment.  The readers of an FP8 cache (fa_paged_tile.h's tiles, fa_mla_indexer_gfx950.hip) take the
// exact way back, cvt8, from here.  Device code only.
#pragma once
#include "fa_device.h"

namespace aule_hip {
namespace {

// eight 16-bit elements = one 16-byte access (register vectors: nothing here is an array the compiler could move to LDS)
template <class E> struct Chunk8;
template <> struct Chunk8<__bf16> { using type = bf16x8_t; };
template <> struct Chunk8<_Float16> { using type = f16x8_t; };
template <class E> using Chunk = typename Chunk8<E>::type;

constexpr float kFp8Max = 448.0f;   // largest finite e4m3fn value

// clamp that keeps NaN: both comparisons are false for it
__device__ __forceinline__ float sat448(float x) {
    x = x > kFp8Max ? kFp8Max : x;
    return x < -kFp8Max ? -kFp8Max : x;
}

// eight 16-bit values -> eight e4m3fn codes (element i in byte i)
template <class E>
__device__ __forceinline__ u32x2_t quant8(const Chunk<E>& x, float scale) {
    u32x2_t out;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const float y0 = sat448((float)x[4 * w] / scale), y1 = sat448((float)x[4 * w + 1] / scale);
        const float y2 = sat448((float)x[4 * w + 2] / scale), y3 = sat448((float)x[4 * w + 3] / scale);
        int word = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);   // low 16 bits
        word = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, word, true);     // high 16 bits
        out[w] = (unsigned)word;
    }
    return out;
}

// the way back, for every reader of an FP8 cache: eight e4m3fn codes -> eight 16-bit elements of T (Bf16Traits / F16Traits), exact
// (every e4m3fn value is a bf16 and an fp16 value)
template <class T>
__device__ __forceinline__ u32x4_t cvt8(u32x2_t x) {
    u32x4_t e;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], false);
        const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], true);
        e[2 * w] = T::pack2(a[0], a[1]);
        e[2 * w + 1] = T::pack2(b[0], b[1]);
    }
    return e;
}

// chunk `x` to element offset `elem` of a cache of E (a copy) or of codes (x / scale)
template <class E, bool FP8>
__device__ __forceinline__ void put(void* cache, size_t elem, const Chunk<E>& x, float scale) {
    if constexpr (FP8) {
        *reinterpret_cast<u32x2_t*>(static_cast<unsigned char*>(cache) + elem) = quant8<E>(x, scale);
    } else {
        *reinterpret_cast<Chunk<E>*>(static_cast<E*>(cache) + elem) = x;
    }
}

}  // namespace
}  // namespace aule_hip
