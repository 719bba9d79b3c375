// kv_append_gfx950.hip -- the write side of the paged KV cache for MI355X: one launch puts the K and V rows of T new
// tokens into the [num_blocks, block_size, heads_kv, head_dim] caches the paged decode reads, with the rotation of K
// and the FP8 quantisation a decode loop would otherwise spell as eight to ten small launches.
//
// Per token t and KV head hk:   slot = slot_mapping[t]   (block * block_size + offset; the caches are contiguous, so
// the slot IS the row index).  A slot outside [0, num_blocks * block_size) -- vLLM's -1 padding included -- is
// skipped: nothing of that token is read or written.  Two tokens of one call with the same slot: which one the cache
// holds afterwards is unspecified (the two rows are written by unrelated threads; per 8- or 16-byte piece it is one
// of the two).
//
//   K' = rope(K[t, hk], table row positions[t])     optional; half-split pairs (p, p + D/2), the fp32 expression of
//                                                   rope_gfx950.hip (fa_device.h: rope_pair), rounded ONCE to the
//                                                   input's 16-bit type -- and only then quantised, so the result
//                                                   is the rotation pass followed by the un-fused append, bit for bit
//   16-bit caches:  cache row = K' / V              a copy of the bits
//   FP8 caches:     code = cvt_e4m3fn(clamp(x / scale[hk], -448, 448))
//                                                   the fp32 division is the correctly rounded one (a reciprocal
//                                                   multiply differs at ties), the clamp keeps NaN (comparisons, not
//                                                   v_min / v_max), the cast is v_cvt_pk_fp8_f32: round to nearest
//                                                   even, subnormals included, -0 -> 0x80, NaN -> a NaN code.  That is
//                                                   quantize_kv_cache_fp8() with given scales.
// A rotated token whose position is outside [0, table_len) is skipped like a bad slot (the table row does not exist).
//
// Shape: pure HBM streaming, no LDS.  One thread owns one rotation pair of 16-byte chunks -- elements [8c, 8c + 8) of
// the first half of the row and the same of the second half -- of K AND of V: four independent 16-byte loads, each
// half read once, the rotation lane-local.  Stores are plain vector stores: 16 bytes per chunk into 16-bit caches,
// 8 bytes per chunk into FP8 caches.  The table rows ([table_len, D/2] fp32, shared by every head) and the scales stay
// in L2.  Algorithmic bytes: T * heads_kv * D * 2 * (2 + cache element size).  At decode sizes (a few KB) the launch
// itself is the cost; there is one.  Byte offsets into the caches are 64-bit.  Host requirements (checked by the
// C-ABI): 16-byte aligned tensors and tables, strides that are multiples of 8 elements, table_pitch % 4 == 0.
#include "fa_kernels.h"
#include "kv_quant.h"

namespace aule_hip {
namespace {

struct KvAppendParams {
    const void* key;
    const void* value;
    void* k_cache;
    void* v_cache;
    const long long* slots;
    const float* k_scale;
    const float* v_scale;
    const float* cos;
    const float* sin;
    const long long* positions;
    long long k_ts, k_hs, v_ts, v_hs;   // token / head strides of key and value, in elements
    long long num_slots;                // num_blocks * block_size
    long long nthreads;                 // T * heads_kv * (D / 16)
    long long table_len;
    int Hkv, D;
    int cshift;                         // log2(D / 16): chunk pairs per row
    int tpitch;                         // floats per table row
};

template <class E, bool FP8, bool ROPE>
__global__ void __launch_bounds__(256) kv_append_kernel(const KvAppendParams p) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= p.nthreads) return;
    const int c = (int)(gid & ((1 << p.cshift) - 1));
    const long long row = gid >> p.cshift;
    const int hk = (int)(row % p.Hkv);
    const long long t = row / p.Hkv;
    const long long slot = p.slots[t];
    if ((unsigned long long)slot >= (unsigned long long)p.num_slots) return;   // negative (padding) or past the cache
    long long pos = 0;
    if constexpr (ROPE) {
        pos = p.positions[t];
        if ((unsigned long long)pos >= (unsigned long long)p.table_len) return;
    }
    const int half = p.D >> 1, lo = 8 * c, hi = half + 8 * c;
    const E* krow = static_cast<const E*>(p.key) + t * p.k_ts + hk * p.k_hs;
    const E* vrow = static_cast<const E*>(p.value) + t * p.v_ts + hk * p.v_hs;
    Chunk<E> ka = *reinterpret_cast<const Chunk<E>*>(krow + lo);
    Chunk<E> kb = *reinterpret_cast<const Chunk<E>*>(krow + hi);
    const Chunk<E> va = *reinterpret_cast<const Chunk<E>*>(vrow + lo);
    const Chunk<E> vb = *reinterpret_cast<const Chunk<E>*>(vrow + hi);
    if constexpr (ROPE) {
        const float* cr = p.cos + (size_t)pos * p.tpitch + lo;
        const float* sr = p.sin + (size_t)pos * p.tpitch + lo;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4_t cs = *reinterpret_cast<const f32x4_t*>(cr + 4 * q);
            const f32x4_t sn = *reinterpret_cast<const f32x4_t*>(sr + 4 * q);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float y1, y2;
                rope_pair((float)ka[4 * q + i], (float)kb[4 * q + i], cs[i], sn[i], y1, y2);
                ka[4 * q + i] = (E)y1;
                kb[4 * q + i] = (E)y2;
            }
        }
    }
    float ks = 1.0f, vs = 1.0f;
    if constexpr (FP8) {
        ks = p.k_scale[hk];
        vs = p.v_scale[hk];
    }
    const size_t dst = ((size_t)slot * p.Hkv + hk) * (size_t)p.D;
    put<E, FP8>(p.k_cache, dst + lo, ka, ks);
    put<E, FP8>(p.k_cache, dst + hi, kb, ks);
    put<E, FP8>(p.v_cache, dst + lo, va, vs);
    put<E, FP8>(p.v_cache, dst + hi, vb, vs);
}

template <class E, bool FP8, bool ROPE>
int run(const KvAppendParams& p, hipStream_t stream) {
    const long long blocks = (p.nthreads + 255) / 256;
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL((kv_append_kernel<E, FP8, ROPE>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

template <class E>
int dispatch(const KvAppendParams& p, bool fp8, bool rope, hipStream_t stream) {
    if (fp8) return rope ? run<E, true, true>(p, stream) : run<E, true, false>(p, stream);
    return rope ? run<E, false, true>(p, stream) : run<E, false, false>(p, stream);
}

}  // namespace

int launch_kv_append(const KvAppendArgs& a, hipStream_t stream) {
    if (a.D != 32 && a.D != 64 && a.D != 128) return -1;
    if (a.T < 0 || a.Hkv <= 0 || a.num_blocks < 0 || a.block_size <= 0) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 && (!a.k_scale || !a.v_scale)) return -1;
    const bool rope = a.cos != nullptr;
    if (rope && (!a.sin || !a.positions || a.table_len <= 0)) return -1;
    KvAppendParams p;
    p.key = a.key; p.value = a.value; p.k_cache = a.k_cache; p.v_cache = a.v_cache;
    p.slots = a.slot_mapping; p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.cos = a.cos; p.sin = a.sin; p.positions = a.positions;
    p.k_ts = a.k_token_stride; p.k_hs = a.k_head_stride; p.v_ts = a.v_token_stride; p.v_hs = a.v_head_stride;
    p.num_slots = a.num_blocks * (long long)a.block_size;
    p.Hkv = a.Hkv; p.D = a.D;
    p.cshift = a.D == 32 ? 1 : a.D == 64 ? 2 : 3;
    p.nthreads = ((long long)a.T * a.Hkv) << p.cshift;
    p.table_len = a.table_len;
    p.tpitch = a.table_pitch > 0 ? a.table_pitch : a.D / 2;
    if (rope && p.tpitch < a.D / 2) return -1;
    if (a.dtype == kBF16) return dispatch<__bf16>(p, fp8, rope, stream);
    if (a.dtype == kF16) return dispatch<_Float16>(p, fp8, rope, stream);
    return -1;
}

}  // namespace aule_hip
