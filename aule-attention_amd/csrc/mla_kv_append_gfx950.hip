// mla_kv_append_gfx950.hip -- the write side of the paged MLA's latent cache for MI355X: one launch puts the latent rows of T new
// tokens into the [num_blocks, block_size, 576] cache fa_fwd_mla_paged*_gfx950.hip read, with the rotation of the 64 rotary
// dimensions and the FP8 quantisation a decode loop would otherwise spell as a rotation, a cat, a divide / clamp / cast and an
// index_copy_.
//
// Per token t:   slot = slot_mapping[t]   (block * block_size + offset; the cache is contiguous, so the slot IS the row index)
//   row[0 .. 511]   = c_kv[t]                                   the compressed dimensions, as they are
//   row[512 .. 575] = rope(k_pe[t], table row positions[t])     optional; pairs (p, p + 32) ("half") or (2p, 2p + 1)
//                                                               ("interleaved"), the fp32 expression of rope_gfx950.hip
//                                                               (fa_device.h: rope_pair), rounded ONCE to the input's 16-bit type
//                                                               -- and only then quantised, so the result is the rotation pass
//                                                               followed by the un-fused append, bit for bit
//   16-bit cache:  cache row = row                              a copy of the bits
//   FP8 cache:     code = cvt_e4m3fn(clamp(x / kv_scale[0], -448, 448))     kv_append_gfx950.hip's rules and code (kv_quant.h):
//                                                               correctly rounded division, a clamp that keeps NaN, v_cvt_pk_fp8_f32
// A slot outside [0, num_blocks * block_size) -- -1 padding included -- skips the token, and so does, with rotation, a position
// outside [0, table_len) (the table row does not exist): NOTHING of that token's row is written, the c_kv part included.  Two tokens
// of one call with the same slot: which one the cache holds afterwards is unspecified.
//
// Shape: pure HBM streaming, no LDS.  36 threads per token, two 16-byte chunks each, so that every thread of a wave does the same
// loads, the same quantisation and the same stores: thread c < 32 owns chunks c and c + 32 of c_kv; thread 32 + j, j < 4, owns one
// rotation's worth of k_pe -- chunks j and j + 4 (half: elements [8j, 8j + 8) and their partners 32 further) or chunks 2j and
// 2j + 1 (interleaved: pairs [8j, 8j + 8) side by side) -- so the rotation is lane-local and both layouts read table entries
// [8j, 8j + 8); only the rotation's arithmetic is divergent.  (One chunk per thread for c_kv made the waves that hold both kinds of
// thread run the quantiser three times.)  Stores are plain vector stores, 16 bytes per chunk into a 16-bit cache, 8 into an FP8 one.
// Algorithmic bytes: T * 576 * (2 + cache element size).  Byte offsets into the cache are 64-bit.  Host requirements (checked by
// the C-ABI): 16-byte aligned tensors and tables, token strides that are multiples of 8 elements, table_pitch % 4 == 0.
#include "fa_kernels.h"
#include "kv_quant.h"

namespace aule_hip {
namespace {

constexpr int kLatC = 512;                      // compressed dimensions
constexpr int kLatR = 64;                       // rotary dimensions
constexpr int kLatRow = kLatC + kLatR;          // elements of a latent row
constexpr int kLatCopy = kLatC / 16;            // threads of a token on c_kv, two chunks (c, c + 32) each
constexpr int kLatThreads = kLatRow / 16;       // threads per token: 32 on c_kv + 4 on k_pe

enum : int { kNoRope = 0, kRopeHalf = 1, kRopeInterleaved = 2 };

struct MlaKvAppendParams {
    const void* c_kv;
    const void* k_pe;
    void* cache;
    const long long* slots;
    const float* kv_scale;
    const float* cos;
    const float* sin;
    const long long* positions;
    long long c_ts, r_ts;     // token strides of c_kv / k_pe, in elements
    long long num_slots;      // num_blocks * block_size
    long long nthreads;       // T * 36
    long long table_len;
    int tpitch;               // floats per table row
};

template <class E, bool FP8, int ROPE>
__global__ void __launch_bounds__(256) mla_kv_append_kernel(const MlaKvAppendParams p) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= p.nthreads) return;
    const long long t = gid / kLatThreads;
    const int c = (int)(gid - t * kLatThreads);
    const long long slot = p.slots[t];
    if ((unsigned long long)slot >= (unsigned long long)p.num_slots) return;   // negative (padding) or past the cache
    long long pos = 0;
    if constexpr (ROPE != kNoRope) {
        pos = p.positions[t];
        if ((unsigned long long)pos >= (unsigned long long)p.table_len) return;   // the whole token: the copy threads leave too
    }
    float scale = 1.0f;
    if constexpr (FP8) scale = p.kv_scale[0];
    const size_t dst = (size_t)slot * kLatRow;
    // the thread's two chunks: where they come from and their element offsets in the latent row
    const bool rot = c >= kLatCopy;   // a thread of k_pe
    const int j = c - kLatCopy;
    const E* src = rot ? static_cast<const E*>(p.k_pe) + t * p.r_ts : static_cast<const E*>(p.c_kv) + t * p.c_ts;
    const int ea = !rot ? 8 * c : ROPE == kRopeInterleaved ? 16 * j : 8 * j;
    const int eb = !rot ? 8 * c + kLatC / 2 : ROPE == kRopeInterleaved ? 16 * j + 8 : 8 * j + kLatR / 2;
    Chunk<E> ka = *reinterpret_cast<const Chunk<E>*>(src + ea);
    Chunk<E> kb = *reinterpret_cast<const Chunk<E>*>(src + eb);
    if (ROPE != kNoRope && rot) {
        const float* cr = p.cos + (size_t)pos * p.tpitch + 8 * j;
        const float* sr = p.sin + (size_t)pos * p.tpitch + 8 * j;
        const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cr), c1 = *reinterpret_cast<const f32x4_t*>(cr + 4);
        const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sr), s1 = *reinterpret_cast<const f32x4_t*>(sr + 4);
        if constexpr (ROPE == kRopeHalf) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {   // pair 8j + i = (ka[i], kb[i])
                float y1, y2;
                rope_pair((float)ka[i], (float)kb[i], i < 4 ? c0[i & 3] : c1[i & 3], i < 4 ? s0[i & 3] : s1[i & 3], y1, y2);
                ka[i] = (E)y1;
                kb[i] = (E)y2;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // pair 8j + i = (ka[2i], ka[2i + 1]), pair 8j + 4 + i = (kb[2i], kb[2i + 1])
                float y1, y2;
                rope_pair((float)ka[2 * i], (float)ka[2 * i + 1], c0[i], s0[i], y1, y2);
                ka[2 * i] = (E)y1;
                ka[2 * i + 1] = (E)y2;
                rope_pair((float)kb[2 * i], (float)kb[2 * i + 1], c1[i], s1[i], y1, y2);
                kb[2 * i] = (E)y1;
                kb[2 * i + 1] = (E)y2;
            }
        }
    }
    const size_t base = dst + (rot ? kLatC : 0);
    put<E, FP8>(p.cache, base + ea, ka, scale);
    put<E, FP8>(p.cache, base + eb, kb, scale);
}

template <class E, bool FP8, int ROPE>
int run(const MlaKvAppendParams& p, hipStream_t stream) {
    const long long blocks = (p.nthreads + 255) / 256;
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL((mla_kv_append_kernel<E, FP8, ROPE>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

template <class E, bool FP8>
int dispatch_rope(const MlaKvAppendParams& p, int rope, hipStream_t stream) {
    if (rope == kRopeHalf) return run<E, FP8, kRopeHalf>(p, stream);
    if (rope == kRopeInterleaved) return run<E, FP8, kRopeInterleaved>(p, stream);
    return run<E, FP8, kNoRope>(p, stream);
}

template <class E>
int dispatch(const MlaKvAppendParams& p, bool fp8, int rope, hipStream_t stream) {
    return fp8 ? dispatch_rope<E, true>(p, rope, stream) : dispatch_rope<E, false>(p, rope, stream);
}

}  // namespace

int launch_mla_kv_append(const MlaKvAppendArgs& a, hipStream_t stream) {
    if (a.T < 0 || a.num_blocks < 0 || a.block_size <= 0) return -1;
    if (a.c_kv_token_stride < kLatC || a.k_pe_token_stride < kLatR || a.c_kv_token_stride % 8 != 0 || a.k_pe_token_stride % 8 != 0) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 ? a.kv_scale == nullptr : a.cache_kind != kCache16) return -1;
    if (a.rope_layout != 0 && a.rope_layout != 1) return -1;
    int rope = kNoRope;
    if (a.cos != nullptr) {
        if (!a.sin || !a.positions || a.table_len <= 0) return -1;
        rope = a.rope_layout == 1 ? kRopeInterleaved : kRopeHalf;
    }
    MlaKvAppendParams p;
    p.c_kv = a.c_kv; p.k_pe = a.k_pe; p.cache = a.kv_cache;
    p.slots = a.slot_mapping; p.kv_scale = a.kv_scale;
    p.cos = a.cos; p.sin = a.sin; p.positions = a.positions;
    p.c_ts = a.c_kv_token_stride; p.r_ts = a.k_pe_token_stride;
    p.num_slots = a.num_blocks * (long long)a.block_size;
    p.nthreads = (long long)a.T * kLatThreads;
    p.table_len = a.table_len;
    p.tpitch = a.table_pitch > 0 ? a.table_pitch : kLatR / 2;
    if (rope != kNoRope && (p.tpitch < kLatR / 2 || p.tpitch % 4 != 0)) return -1;
    if (a.dtype == kBF16) return dispatch<__bf16>(p, fp8, rope, stream);
    if (a.dtype == kF16) return dispatch<_Float16>(p, fp8, rope, stream);
    return -1;
}

}  // namespace aule_hip
