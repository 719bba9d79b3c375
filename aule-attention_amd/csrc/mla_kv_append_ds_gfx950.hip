// mla_kv_append_ds_gfx950.hip -- the write side of the per-128-scaled FP8 latent cache (fa_mla_ds.h): one launch
// quantises and writes the 656-byte rows of T new tokens, mla_kv_append_gfx950.hip's call with another row.
//
// Per token t:   slot = slot_mapping[t]   (block * block_size + offset; the cache is contiguous, so the slot IS the row index)
//   group g < 4 of c_kv[t] (columns 128 g .. 128 g + 127):
//     amax  = max |x| over the group, in fp32
//     scale = 2^max(ceil(log2(amax / 448)), -126), 1 for a group of zeros: a power of two, so code * scale is exact (the floor of
//             the exponent keeps the scale a normal fp32 number)
//     code  = e4m3fn_rne(clamp(x / scale, -448, 448))     (x / scale is exact too; the clamp keeps NaN)
//   row bytes 0 .. 511 = the codes, 512 .. 527 = the four scales, 528 .. 655 = rope(k_pe[t]) as bf16: mla_kv_append_gfx950.hip's
//   rotation (pairs (p, p + 32) or (2p, 2p + 1), rope_pair in fp32, rounded once to bf16), or the bits of k_pe without tables.
// A slot outside [0, num_blocks * block_size), or with rotation a position outside [0, table_len), skips the whole token.  The inputs
// are bf16 (the rotary part of a row is bf16 and is not converted twice), read in place with their own token strides.
//
// Shape: ONE WAVE PER TOKEN, four tokens per workgroup, no LDS.  Lane c owns the 8-element chunk c of c_kv, so group g is lanes
// 16 g .. 16 g + 15 -- one DPP row: the lane folds its eight magnitudes, then four v_max_f32 with row_ror:8/4/2/1 leave the group's
// amax in all 16 lanes (a rotation within a row never crosses into a neighbouring group, and every lane of the wave is live: a
// skipped token leaves as a whole wave).  Scale and its reciprocal are made from the exponent bits, the lane quantises its chunk and
// stores 8 bytes (the wave: 512 consecutive bytes); v_readlane gathers the four scales into one 16-byte store by lane 0.  Lanes
// 0 .. 3 also own one rotation's worth of k_pe each, two chunks, as in mla_kv_append_gfx950.hip; their loads are issued before the
// reduction.  Algorithmic bytes: T * (1152 + 656).  Host requirements (checked by the C-ABI): 16-byte aligned tensors and tables,
// token strides that are multiples of 8 elements, table_pitch % 4 == 0.
#include "fa_kernels.h"
#include "kv_quant.h"
#include "fa_mla_ds.h"

namespace aule_hip {
namespace {

enum : int { kNoRope = 0, kRopeHalf = 1, kRopeInterleaved = 2 };

struct MlaKvAppendDsParams {
    const __bf16* c_kv;
    const __bf16* k_pe;
    unsigned char* cache;
    const long long* slots;
    const float* cos;
    const float* sin;
    const long long* positions;
    long long c_ts, r_ts;     // token strides of c_kv / k_pe, in elements
    long long num_slots;      // num_blocks * block_size
    long long T;
    long long table_len;
    int tpitch;               // floats per table row
};

// max over the lane's DPP row (16 lanes), in every lane of it
template <int N>
__device__ __forceinline__ float ror_max(float x) {
    const int y = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + N, 0xf, 0xf, false);   // row_ror:N
    return fmaxf(x, __builtin_bit_cast(float, y));
}
__device__ __forceinline__ float row16_max(float x) { return ror_max<1>(ror_max<2>(ror_max<4>(ror_max<8>(x)))); }

template <int ROPE>
__global__ void __launch_bounds__(256) mla_kv_append_ds_kernel(const MlaKvAppendDsParams p) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= p.T) return;
    const long long slot = p.slots[t];
    if ((unsigned long long)slot >= (unsigned long long)p.num_slots) return;   // negative (padding) or past the cache
    long long pos = 0;
    if constexpr (ROPE != kNoRope) {
        pos = p.positions[t];
        if ((unsigned long long)pos >= (unsigned long long)p.table_len) return;
    }
    unsigned char* row = p.cache + (size_t)slot * kDsRow;
    const bf16x8_t x = *reinterpret_cast<const bf16x8_t*>(p.c_kv + t * p.c_ts + 8 * lane);
    // lanes 0 .. 3: rotation j's two chunks of k_pe
    const bool rot = lane < 4;
    const int ea = ROPE == kRopeInterleaved ? 16 * lane : 8 * lane;
    const int eb = ROPE == kRopeInterleaved ? 16 * lane + 8 : 8 * lane + 32;
    bf16x8_t ka = {}, kb = {};
    if (rot) {
        ka = *reinterpret_cast<const bf16x8_t*>(p.k_pe + t * p.r_ts + ea);
        kb = *reinterpret_cast<const bf16x8_t*>(p.k_pe + t * p.r_ts + eb);
    }
    float xf[8], amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        xf[i] = (float)x[i];
        amax = fmaxf(amax, __builtin_fabsf(xf[i]));
    }
    amax = row16_max(amax);
    // amax = m * 2^e, 1 <= m < 2, and 448 = 1.75 * 2^8: ceil(log2(amax / 448)) = e - 8, + 1 when m > 1.75
    const unsigned bits = __builtin_bit_cast(unsigned, amax);
    int k = (int)(bits >> 23) - 127 - 8 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    k = amax > 0.f ? max(k, -126) : 0;
    const float scale = __builtin_bit_cast(float, (unsigned)(k + 127) << 23);
    const float inv = __builtin_bit_cast(float, (unsigned)(127 - k) << 23);
    u32x2_t code;
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(xf[4 * w] * inv), sat448(xf[4 * w + 1] * inv), 0, false);
        word = __builtin_amdgcn_cvt_pk_fp8_f32(sat448(xf[4 * w + 2] * inv), sat448(xf[4 * w + 3] * inv), word, true);
        code[w] = (unsigned)word;
    }
    *reinterpret_cast<u32x2_t*>(row + 8 * lane) = code;
    const int sb = __builtin_bit_cast(int, scale);
    const u32x4_t s4 = {(unsigned)__builtin_amdgcn_readlane(sb, 0), (unsigned)__builtin_amdgcn_readlane(sb, 16),
                        (unsigned)__builtin_amdgcn_readlane(sb, 32), (unsigned)__builtin_amdgcn_readlane(sb, 48)};
    if (lane == 0) *reinterpret_cast<u32x4_t*>(row + kDsScaleAt) = s4;
    if (!rot) return;
    if constexpr (ROPE != kNoRope) {
        const float* cr = p.cos + (size_t)pos * p.tpitch + 8 * lane;
        const float* sr = p.sin + (size_t)pos * p.tpitch + 8 * lane;
        const f32x4_t c0 = *reinterpret_cast<const f32x4_t*>(cr), c1 = *reinterpret_cast<const f32x4_t*>(cr + 4);
        const f32x4_t s0 = *reinterpret_cast<const f32x4_t*>(sr), s1 = *reinterpret_cast<const f32x4_t*>(sr + 4);
        if constexpr (ROPE == kRopeHalf) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {   // pair 8j + i = (ka[i], kb[i])
                float y1, y2;
                rope_pair((float)ka[i], (float)kb[i], i < 4 ? c0[i & 3] : c1[i & 3], i < 4 ? s0[i & 3] : s1[i & 3], y1, y2);
                ka[i] = (__bf16)y1;
                kb[i] = (__bf16)y2;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {   // pair 8j + i = (ka[2i], ka[2i + 1]), pair 8j + 4 + i = (kb[2i], kb[2i + 1])
                float y1, y2;
                rope_pair((float)ka[2 * i], (float)ka[2 * i + 1], c0[i], s0[i], y1, y2);
                ka[2 * i] = (__bf16)y1;
                ka[2 * i + 1] = (__bf16)y2;
                rope_pair((float)kb[2 * i], (float)kb[2 * i + 1], c1[i], s1[i], y1, y2);
                kb[2 * i] = (__bf16)y1;
                kb[2 * i + 1] = (__bf16)y2;
            }
        }
    }
    *reinterpret_cast<bf16x8_t*>(row + kDsRopeAt + 2 * ea) = ka;
    *reinterpret_cast<bf16x8_t*>(row + kDsRopeAt + 2 * eb) = kb;
}

template <int ROPE>
int run(const MlaKvAppendDsParams& p, hipStream_t stream) {
    const long long blocks = (p.T + 3) / 4;
    if (blocks <= 0) return 0;
    if (blocks > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL((mla_kv_append_ds_kernel<ROPE>), dim3((unsigned)blocks), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// (`a`: launch_mla_kv_append's arguments with kv_cache the [num_blocks * block_size][656] rows; dtype kBF16, no kv_scale)
int launch_mla_kv_append_ds(const MlaKvAppendArgs& a, hipStream_t stream) {
    if (a.T < 0 || a.num_blocks < 0 || a.block_size <= 0) return -1;
    if (a.c_kv_token_stride < 512 || a.k_pe_token_stride < 64 || a.c_kv_token_stride % 8 != 0 || a.k_pe_token_stride % 8 != 0) return -1;
    if (a.dtype != kBF16 || a.kv_scale != nullptr) return -1;
    if (a.rope_layout != 0 && a.rope_layout != 1) return -1;
    int rope = kNoRope;
    if (a.cos != nullptr) {
        if (!a.sin || !a.positions || a.table_len <= 0) return -1;
        rope = a.rope_layout == 1 ? kRopeInterleaved : kRopeHalf;
    }
    MlaKvAppendDsParams p;
    p.c_kv = static_cast<const __bf16*>(a.c_kv); p.k_pe = static_cast<const __bf16*>(a.k_pe);
    p.cache = static_cast<unsigned char*>(a.kv_cache);
    p.slots = a.slot_mapping;
    p.cos = a.cos; p.sin = a.sin; p.positions = a.positions;
    p.c_ts = a.c_kv_token_stride; p.r_ts = a.k_pe_token_stride;
    p.num_slots = a.num_blocks * (long long)a.block_size;
    p.T = a.T;
    p.table_len = a.table_len;
    p.tpitch = a.table_pitch > 0 ? a.table_pitch : 32;
    if (rope != kNoRope && (p.tpitch < 32 || p.tpitch % 4 != 0)) return -1;
    if (rope == kRopeHalf) return run<kRopeHalf>(p, stream);
    if (rope == kRopeInterleaved) return run<kRopeInterleaved>(p, stream);
    return run<kNoRope>(p, stream);
}

}  // namespace aule_hip
