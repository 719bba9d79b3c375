// fa_tile_attention.h -- what the tiled ragged kernels share beyond their layout (the paged prefill,
// the shared-prefix pass, the variable-length and the MLA 192 / 128 forward and backward): the product of a 64-row LDS image with the lane's row, the 16-bit store of a
// row of MFMA accumulators (lanes l and l + 32 hold the same row) and, on the host, the dtype x head_dim x cache-kind dispatch.
// The forward kernels keep their own copies of the softmax step, and the delta and dK/dV kernels their own bodies: written as shared
// __forceinline__ pieces the same statements compiled to other schedules, which cost registers in some instances and 0.2 .. 0.9 %
// on some shapes (profiles/tile_refactor_resources.txt, profiles/tile_refactor_ab.txt).
#pragma once
#include <type_traits>

#include "fa_kernels.h"
#include "fa_paged_tile.h"

namespace aule_hip {
namespace {

// sc[kk] = rows 32 kk .. 32 kk + 31 of the LDS image `img` (pitch bytes per row, read as ds_read_b128 A operands) times the lane's
// row rf, G operand chunk pairs deep (element rr of sc[kk] is row 32 kk + crow(rr, hi) of the image)
template <class T, int G>
__device__ __forceinline__ void tile_scores(f32x16_t (&sc)[2], const char* img, int pitch, const u32x4_t (&rf)[G], int l31, int hi) {
    sc[0] = sc[1] = f32x16_t{};
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) sc[kk] = mfma16<T>(lds_b128(img + (32 * kk + l31) * pitch + 32 * g + 16 * hi), rf[g], sc[kk]);
}

// DT accumulators of the lane's row (32 DT columns between the lane pair) times f -> the 16-bit row at dst
template <class T, int DT>
__device__ __forceinline__ void store_row16(char* dst, const f32x16_t (&a)[DT], float f, int hi) {
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = a[dt][4 * g4] * f, a1 = a[dt][4 * g4 + 1] * f, a2 = a[dt][4 * g4 + 2] * f, a3 = a[dt][4 * g4 + 3] * f;
            *reinterpret_cast<u32x2_t*>(dst + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
}

// The epilogue of a forward with attention sinks: the row's state (m in log2 units, l) and its head's sink logit -- raw,
// natural units, a term of the denominator that carries no value -> the factor `inv` of the accumulators; returns lse = ln Z.
// sink = -inf ("no sink"): a is exactly 1 and ls exactly l, so inv and the lse are the sinkless epilogue's bits.  A row without a
// visible key (m = -inf): inv = 0 and lse = the logit itself, not its round trip through log2 units.
__device__ __forceinline__ float sink_epilogue(float sink, float m, float l, float& inv) {
    const float s2 = sink * kLog2e;
    const float mn = fmaxf(m, s2);
    const float top = mn == -__builtin_inff() ? 0.f : mn;
    const float a = fast_exp2(m - top);   // m = -inf: 0
    const float ls = l * a + fast_exp2(s2 - top);
    inv = a * (ls > 0.f ? 1.f / ls : 0.f);
    if (m == -__builtin_inff()) return sink;
    return ls > 0.f ? (top + fast_log2(ls)) * kLn2 : -__builtin_inff();
}

// Host: the kernel instance for (dtype, head_dim in {32, 64, 128}): f(T{}, std::integral_constant<int, D>{}), -1 for anything else
template <class F>
int dispatch_tile_instance(int dtype, int D, F&& f) {
    const auto dim = [&](auto t) {
        if (D == 32) return f(t, std::integral_constant<int, 32>{});
        if (D == 64) return f(t, std::integral_constant<int, 64>{});
        if (D == 128) return f(t, std::integral_constant<int, 128>{});
        return -1;
    };
    if (dtype == kBF16) return dim(Bf16Traits{});
    if (dtype == kF16) return dim(F16Traits{});
    return -1;
}

// ... and for (dtype, head_dim, cache kind): f(T{}, std::integral_constant<int, D>{}, Kv16{} or KvFp8{})
template <class F>
int dispatch_tile_instance(int dtype, int D, bool fp8, F&& f) {
    return dispatch_tile_instance(dtype, D, [&](auto t, auto d) { return fp8 ? f(t, d, KvFp8{}) : f(t, d, Kv16{}); });
}

}  // namespace
}  // namespace aule_hip
