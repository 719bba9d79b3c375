// mla_indexer_append_gfx950.hip -- the write side of the sparse MLA's indexer for MI355X: one launch transforms rows of 128 16-bit
// elements -- the index key of every new token, or the 64 index queries of every token -- and stores them densely (the query
// side) or into the paged [num_blocks, block_size, 128] index-key cache fa_mla_indexer_gfx950.hip reads (the key side), where a
// serving loop would otherwise spell a LayerNorm, a split / rotation / cat, a Hadamard matmul, an amax / divide / clamp / cast and
// two scatters.
//
// Per row x of 128 elements (row = (token t, head h); a cache destination has one head), loaded and carried in fp32 through every
// enabled stage:
//   1. norm (optional)      mu = mean(x); var = mean((x - mu)^2) (biased); x <- (x - mu) / sqrt(var + eps) * w + b, w and b [128] fp32
//                           (b absent: zero)
//   2. RoPE (optional)      the 64 elements [rope_offset, rope_offset + 64), rope_offset 0 or 64, by table row positions[t] of cos / sin
//                           [table_len, 32] fp32 (every head of a token: the same row); pairs (p, p + 32) ("half") or (2p, 2p + 1)
//                           ("interleaved") relative to rope_offset; the arithmetic is rope_pair (fa_device.h)
//   3. Hadamard (optional)  y[i] = 2^-3.5 * sum_j (-1)^popcount(i & j) * x[j]: the Sylvester H_128 in natural order, scaled by 128^-0.5,
//                           fp32 sums
//   4. round ONCE to the input's 16-bit type: the row r
//   5. store r   dense:         out[t, h, :] = r (out may be the input: every lane has read its row before any lane writes)
//                16-bit cache:  cache row slot_mapping[t] = the bits of r
//                FP8 cache:     amax = max |r|; s0 = amax > 0 ? amax / 448 : 1 (correctly rounded division); scale = s0 ("amax") or the
//                               power of two >= s0 ("ue8m0": bits(scale) = max((bits(s0) + 0x007FFFFF) & 0x7F800000, 0x00800000));
//                               code = cvt_e4m3fn(clamp(r / scale, -448, 448)) (quant8, kv_quant.h); k_scale[slot] = scale.  With "amax"
//                               this is quantize_indexer_cache_fp8's rule applied to r, bit for bit.
// A slot outside [0, num_blocks * block_size) -- -1 padding included -- skips the token, and so does, with RoPE, a position outside
// [0, table_len): NOTHING of that token's row and nothing of its scale is written.  Two tokens of one call with the same slot:
// which one the cache holds afterwards is unspecified.
//
// Shape: pure streaming, 256 bytes in and 256 or 128 + 4 bytes out per row, no LDS array.  8 lanes per row, two 16-byte chunks per
// lane: lane l = 4 g + j of its group holds chunks 8 g + j and 8 g + j + 4, i.e. elements 64 g + 8 j + [0, 8) and the same + 32.
// Element index bits: 0-2 the element of the chunk, 3-4 = j, 5 = which chunk, 6 = g.  So
//   * the "half" partner (p + 32) of every element is in the same lane, "interleaved" pairs are neighbours of a chunk, and only the
//     lanes with 64 g == rope_offset rotate;
//   * of the 7 butterfly stages of H_128 four are in registers (bits 0-2 and 5) and three cross lanes: xor 1 and xor 2 through DPP
//     quad_perm, xor 4 through ds_swizzle (the crossbar of the LDS unit; no LDS memory);
//   * mean, variance and amax are a 16-element reduction per lane and the same three exchanges.
// 8 rows per wave, 32 per workgroup of 256; a partial last group of rows or a skipped token switches whole 8-lane groups off, so
// every exchange stays among live lanes.  Stores are plain vector stores (16 bytes per chunk, 8 into an FP8 cache); lane 0 of the
// group stores the fp32 scale.  Byte offsets are 64-bit.  The element type, the destination and the three stages are template
// parameters; the pair layout, rope_offset, the bias and the scale format are run-time (uniform branches).
// Host requirements (checked by the C-ABI): 16-byte aligned tensors, tables and norm vectors, strides that are multiples of 8
// elements, table_pitch % 4 == 0, T * heads < 2^31.
#include "fa_kernels.h"
#include "kv_quant.h"

namespace aule_hip {
namespace {

constexpr int kRowW = 128;                                // elements of a row
constexpr int kRowLanes = 8;                              // lanes per row
constexpr int kRowsPerBlock = 256 / kRowLanes;
constexpr float kHadamardScale = 0.08838834764831845f;    // 2^-3.5

enum : int { kDstDense = 0, kDstCache16 = 1, kDstCacheFp8 = 2 };

struct IndexerRowsParams {
    const void* x;
    void* dst;                // out, or the cache
    float* k_scale;
    const long long* slots;
    const float* w;
    const float* b;           // may be null
    const float* cos;
    const float* sin;
    const long long* positions;
    long long x_ts, x_hs;     // token / head strides of x, in elements
    long long o_ts, o_hs;     // of out (dense)
    long long num_slots;      // num_blocks * block_size
    long long table_len;
    unsigned rows;            // T * heads
    unsigned heads;
    int tpitch;               // floats per table row
    int rope_g;               // rope_offset / 64: the half of the row that rotates
    int interleaved;
    int ue8m0;
    float eps;
};

// the value of lane ^ 1 / lane ^ 2 (DPP quad_perm [1,0,3,2] / [2,3,0,1]) and of lane ^ 4 (ds_swizzle, bit mode: and 0x1f, or 0, xor 4)
template <int M>
__device__ __forceinline__ float lane_xor(float x) {
    static_assert(M == 1 || M == 2 || M == 4, "exchanges inside a group of 8 lanes");
    const int v = __builtin_bit_cast(int, x);
    if constexpr (M == 4) return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(v, (4 << 10) | 0x1f));
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, v, M == 1 ? 0xB1 : 0x4E, 0xf, 0xf, false));
}
// sum / max over the 8 lanes of a row, the same bits in every lane of it
__device__ __forceinline__ float group_sum(float x) {
    x += lane_xor<1>(x);
    x += lane_xor<2>(x);
    return x + lane_xor<4>(x);
}
__device__ __forceinline__ float group_max(float x) {
    x = fmaxf(x, lane_xor<1>(x));
    x = fmaxf(x, lane_xor<2>(x));
    return fmaxf(x, lane_xor<4>(x));
}
// one butterfly stage across lanes: the lane whose bit M is clear takes mine + other, its partner other - mine
template <int M>
__device__ __forceinline__ void cross_stage(float (&v)[16], int l) {
    const unsigned flip = (l & M) ? 0x80000000u : 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = lane_xor<M>(v[i]) + __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v[i]) ^ flip);
}
// one stage inside the lane: element index bit S (0 .. 2: inside a chunk; 3: the lane's two chunks, element bit 5)
template <int S>
__device__ __forceinline__ void local_stage(float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i & (1 << S)) continue;
        const float a = v[i], b = v[i | (1 << S)];
        v[i] = a + b;
        v[i | (1 << S)] = a - b;
    }
}

__device__ __forceinline__ void load8(const float* p, float (&v)[16], int at) {
    const f32x4_t a = *reinterpret_cast<const f32x4_t*>(p), b = *reinterpret_cast<const f32x4_t*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[at + i] = a[i];
        v[at + 4 + i] = b[i];
    }
}

template <class E, int DST, bool NORM, bool ROPE, bool HAD>
__global__ void __launch_bounds__(256) mla_indexer_rows_kernel(const IndexerRowsParams p) {
    const unsigned row = blockIdx.x * (unsigned)kRowsPerBlock + (threadIdx.x >> 3);
    if (row >= p.rows) return;
    const int l = threadIdx.x & 7, g = l >> 2, j = l & 3;
    unsigned t = row, h = 0;
    if (DST == kDstDense && p.heads > 1) {
        t = row / p.heads;
        h = row - t * p.heads;
    }
    long long slot = 0;
    if constexpr (DST != kDstDense) {
        slot = p.slots[t];
        if ((unsigned long long)slot >= (unsigned long long)p.num_slots) return;   // negative (padding) or past the cache
    }
    long long pos = 0;
    if constexpr (ROPE) {
        pos = p.positions[t];
        if ((unsigned long long)pos >= (unsigned long long)p.table_len) return;    // the table row does not exist
    }
    const int ea = 64 * g + 8 * j, eb = ea + 32;   // the lane's two chunks
    const E* src = static_cast<const E*>(p.x) + (long long)t * p.x_ts + (long long)h * p.x_hs;
    const Chunk<E> xa = *reinterpret_cast<const Chunk<E>*>(src + ea);
    const Chunk<E> xb = *reinterpret_cast<const Chunk<E>*>(src + eb);
    float v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = (float)xa[i];
        v[8 + i] = (float)xb[i];
    }
    if constexpr (NORM) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
        const float mu = group_sum(s) * (1.0f / kRowW);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] -= mu;
            q = __builtin_fmaf(v[i], v[i], q);
        }
        const float rstd = 1.0f / __builtin_sqrtf(group_sum(q) * (1.0f / kRowW) + p.eps);
        float w[16], b[16];
        load8(p.w + ea, w, 0);
        load8(p.w + eb, w, 8);
        if (p.b != nullptr) {
            load8(p.b + ea, b, 0);
            load8(p.b + eb, b, 8);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) b[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = __builtin_fmaf(v[i] * rstd, w[i], b[i]);
    }
    if constexpr (ROPE) {
        if (g == p.rope_g) {
            const float* cr = p.cos + (size_t)pos * p.tpitch;
            const float* sr = p.sin + (size_t)pos * p.tpitch;
            if (!p.interleaved) {   // pair 8 j + i = (v[i], v[8 + i])
                float c[16], s[16];
                load8(cr + 8 * j, c, 0);
                load8(sr + 8 * j, s, 0);
#pragma unroll
                for (int i = 0; i < 8; ++i) rope_pair(v[i], v[8 + i], c[i], s[i], v[i], v[8 + i]);
            } else {                // pair 4 j + i = (v[2i], v[2i + 1]), pair 16 + 4 j + i = (v[8 + 2i], v[8 + 2i + 1])
                const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cr + 4 * j), c1 = *reinterpret_cast<const f32x4_t*>(cr + 16 + 4 * j);
                const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sr + 4 * j), s1 = *reinterpret_cast<const f32x4_t*>(sr + 16 + 4 * j);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    rope_pair(v[2 * i], v[2 * i + 1], c0[i], s0[i], v[2 * i], v[2 * i + 1]);
                    rope_pair(v[8 + 2 * i], v[8 + 2 * i + 1], c1[i], s1[i], v[8 + 2 * i], v[8 + 2 * i + 1]);
                }
            }
        }
    }
    if constexpr (HAD) {
        local_stage<0>(v);
        local_stage<1>(v);
        local_stage<2>(v);
        cross_stage<1>(v, l);   // element bit 3
        cross_stage<2>(v, l);   // element bit 4
        local_stage<3>(v);      // element bit 5
        cross_stage<4>(v, l);   // element bit 6
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] *= kHadamardScale;
    }
    Chunk<E> ra, rb;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        ra[i] = (E)v[i];
        rb[i] = (E)v[8 + i];
    }
    if constexpr (DST == kDstDense) {
        E* o = static_cast<E*>(p.dst) + (long long)t * p.o_ts + (long long)h * p.o_hs;
        *reinterpret_cast<Chunk<E>*>(o + ea) = ra;
        *reinterpret_cast<Chunk<E>*>(o + eb) = rb;
    } else {
        float scale = 1.0f;
        if constexpr (DST == kDstCacheFp8) {
            float amax = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fmaxf(__builtin_fabsf((float)ra[i]), __builtin_fabsf((float)rb[i])));
            amax = group_max(amax);
            scale = amax > 0.f ? amax / kFp8Max : 1.0f;
            if (p.ue8m0) {
                const unsigned up = (__builtin_bit_cast(unsigned, scale) + 0x007FFFFFu) & 0x7F800000u;
                scale = __builtin_bit_cast(float, up < 0x00800000u ? 0x00800000u : up);
            }
            if (l == 0) p.k_scale[slot] = scale;
        }
        const size_t base = (size_t)slot * kRowW;
        put<E, DST == kDstCacheFp8>(p.dst, base + ea, ra, scale);
        put<E, DST == kDstCacheFp8>(p.dst, base + eb, rb, scale);
    }
}

template <class E, int DST, bool NORM, bool ROPE, bool HAD>
int run(const IndexerRowsParams& p, hipStream_t stream) {
    const unsigned blocks = (p.rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL((mla_indexer_rows_kernel<E, DST, NORM, ROPE, HAD>), dim3(blocks), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

template <class E, int DST, bool NORM, bool ROPE>
int dispatch_had(const IndexerRowsParams& p, bool had, hipStream_t stream) {
    return had ? run<E, DST, NORM, ROPE, true>(p, stream) : run<E, DST, NORM, ROPE, false>(p, stream);
}

template <class E, int DST>
int dispatch_stages(const IndexerRowsParams& p, bool norm, bool rope, bool had, hipStream_t stream) {
    if (norm) return rope ? dispatch_had<E, DST, true, true>(p, had, stream) : dispatch_had<E, DST, true, false>(p, had, stream);
    return rope ? dispatch_had<E, DST, false, true>(p, had, stream) : dispatch_had<E, DST, false, false>(p, had, stream);
}

template <class E>
int dispatch(const IndexerRowsParams& p, int dst, bool norm, bool rope, bool had, hipStream_t stream) {
    if (dst == kDstDense) return dispatch_stages<E, kDstDense>(p, norm, rope, had, stream);
    if (dst == kDstCache16) return dispatch_stages<E, kDstCache16>(p, norm, rope, had, stream);
    return dispatch_stages<E, kDstCacheFp8>(p, norm, rope, had, stream);
}

}  // namespace

int launch_mla_indexer_rows(const MlaIndexerRowsArgs& a, hipStream_t stream) {
    if (a.T <= 0 || a.heads <= 0 || (long long)a.T * a.heads > 0x7fffffffLL) return -1;
    if (a.x == nullptr || (a.out != nullptr) == (a.k_cache != nullptr)) return -1;
    if (a.x_token_stride % 8 != 0 || a.x_head_stride % 8 != 0) return -1;
    int dst = kDstDense;
    if (a.k_cache != nullptr) {
        const bool fp8 = a.cache_kind == kCacheFp8E4M3;
        if (a.heads != 1 || a.slot_mapping == nullptr || a.num_blocks < 0 || a.block_size <= 0) return -1;
        if (fp8 ? a.k_scale == nullptr : a.cache_kind != kCache16) return -1;
        dst = fp8 ? kDstCacheFp8 : kDstCache16;
    } else if (a.out_token_stride % 8 != 0 || a.out_head_stride % 8 != 0) {
        return -1;
    }
    if (a.scale_format != 0 && a.scale_format != 1) return -1;
    if (a.rope_layout != 0 && a.rope_layout != 1) return -1;
    if (a.rope_offset != 0 && a.rope_offset != kRowW / 2) return -1;
    const bool rope = a.cos != nullptr;
    if (rope && (!a.sin || !a.positions || a.table_len <= 0)) return -1;
    IndexerRowsParams p;
    p.x = a.x; p.dst = dst == kDstDense ? a.out : a.k_cache; p.k_scale = a.k_scale;
    p.slots = a.slot_mapping; p.w = a.norm_weight; p.b = a.norm_bias;
    p.cos = a.cos; p.sin = a.sin; p.positions = a.positions;
    p.x_ts = a.x_token_stride; p.x_hs = a.x_head_stride; p.o_ts = a.out_token_stride; p.o_hs = a.out_head_stride;
    p.num_slots = a.num_blocks * (long long)a.block_size;
    p.table_len = a.table_len;
    p.rows = (unsigned)((long long)a.T * a.heads); p.heads = (unsigned)a.heads;
    p.tpitch = a.table_pitch > 0 ? a.table_pitch : kRowW / 4;
    if (rope && (p.tpitch < kRowW / 4 || p.tpitch % 4 != 0)) return -1;
    p.rope_g = a.rope_offset / (kRowW / 2); p.interleaved = a.rope_layout; p.ue8m0 = a.scale_format;
    p.eps = a.eps;
    const bool norm = a.norm_weight != nullptr;
    if (!norm && a.norm_bias != nullptr) return -1;
    if (a.dtype == kBF16) return dispatch<__bf16>(p, dst, norm, rope, a.hadamard, stream);
    if (a.dtype == kF16) return dispatch<_Float16>(p, dst, norm, rope, a.hadamard, stream);
    return -1;
}

}  // namespace aule_hip
