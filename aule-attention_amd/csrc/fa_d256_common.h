// fa_d256_common.h -- pieces shared by the head_dim = 256 kernels (fa_fwd_d256_gfx950.hip, fa_bwd_d256_gfx950.hip).
//
// At D = 256 one wave cannot hold a 64-row Q slab, a full O accumulator and the prefetch of the next K/V tile in the
// schedules of the D <= 128 kernels, so these kernels use one plain layout for every dtype ("D = 256"):
//   * one wave owns 32 rows (queries in the forward and the dQ kernel, keys in the dK/dV kernel) whose operand rows it keeps
//     in registers (16-bit) or re-reads through the buffer descriptor (fp32: the registers go to the accumulators);
//   * the shared operand streams through LDS in tiles of 64 (forward, dQ) or 32 (dK/dV) rows;
//   * every product that sums over the row index of an MFMA result takes that result as its B operand with no lane movement
//     (fa_device.h: element j of lane half h is row 16 s + 8 (j >> 2) + 4 h + (j & 3) of k-step s; fp32: register r of lane
//     half h is row crow(r, 0) + 4 h), and the other operand is read transposed from LDS (16-bit: ds_read_b64_tr_b16).
// Operand chunks: a lane's 16 bytes at byte column 32 g + 16 h of a row are one k-step of the 16-bit MFMA (8 elements) or
// four k-steps of v_mfma_f32_32x32x2_f32 (elements e = 0..3: k-step 4 g + e, lane half h supplies column 8 g + 4 h + e).
// Device code only.
#pragma once
#include "fa_fwd_tile.h"

namespace aule_hip {
namespace {

constexpr int kD256 = 256;

struct F32Traits {
    static constexpr int kDType = 0;
};

template <class T>
struct D256Cfg {
    static constexpr int ES = T::kDType == 0 ? 4 : 2;   // element bytes
    static constexpr int RB = kD256 * ES;                // row bytes in global memory
    static constexpr int G = RB / 32;                    // 16-byte chunk pairs per row (operand groups)
    // LDS row pitches: rows read as MFMA A operands with ds_read_b128 (16 rows of one column per lane group) shift by one 16-byte slot
    // per row; rows read transposed (ds_read_b64_tr_b16: four rows x 64 bytes per 32-lane half) by 64 bytes per row; rows read both
    // ways by 80 bytes (odd slot count: the b128 groups stay conflict-free, the transposed reads overlap in one slot pair)
    static constexpr int PA = RB + 16;
    static constexpr int PT = T::kDType == 0 ? RB : RB + 64;
    static constexpr int PAT = T::kDType == 0 ? RB + 16 : RB + 80;
};

template <class T>
__device__ __forceinline__ f32x16_t mfma16(u32x4_t a, u32x4_t b, f32x16_t c) {
    return T::mfma(as_v8<T>(a), as_v8<T>(b), c);
}

// fp32: the four k-steps of one operand chunk pair.  (The chunks are reinterpreted whole: a __builtin_bit_cast of a single vector
// element, bit_cast(float, a[1]), compiled to a read of element 0.)
__device__ __forceinline__ f32x16_t mfma_f32x4(u32x4_t a, u32x4_t b, f32x16_t c) {
    const f32x4_t fa = __builtin_bit_cast(f32x4_t, a), fb = __builtin_bit_cast(f32x4_t, b);
#pragma unroll
    for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], c, 0, 0, 0);
    return c;
}

template <class T>
__device__ __forceinline__ f32x16_t mfma_chunk(u32x4_t a, u32x4_t b, f32x16_t c) {
    if constexpr (T::kDType == 0) return mfma_f32x4(a, b, c);
    else return mfma16<T>(a, b, c);
}

__device__ __forceinline__ u32x4_t lds_b128(const char* p) { return *reinterpret_cast<const u32x4_t*>(p); }

// 16-bit A operand X^T[col][row] for the k-step over rows r0 .. r0 + 15 of a row-major LDS image X[row][col] (pitch bytes per row):
// lane (col c0 + (lane & 31), half h) gets rows r0 + 4 h + {0..3} (elements 0..3) and r0 + 8 + 4 h + {0..3} (4..7).
__device__ __forceinline__ u32x4_t lds_tr_step(const char* x, int pitch, int r0, int c0, int lane) {
    const int grp = lane >> 4, c = lane & 15;
    const int row = r0 + 4 * (grp >> 1) + (c >> 2);
    const int col = c0 + 16 * (grp & 1) + 4 * (c & 3);
    const char* p = x + row * pitch + col * 2;
    const s16x4_t a = lds_tr16(p);
    const s16x4_t b = lds_tr16(p + 8 * pitch);
    const s16x8_t t = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(u32x4_t, t);
}

// pack registers 8 s .. 8 s + 7 of an fp32 MFMA result into the 16-bit B operand of k-step s
template <class T>
__device__ __forceinline__ u32x4_t pack_step(const f32x16_t& x, int s) {
    return u32x4_t{T::pack2(x[8 * s + 0], x[8 * s + 1]), T::pack2(x[8 * s + 2], x[8 * s + 3]),
                   T::pack2(x[8 * s + 4], x[8 * s + 5]), T::pack2(x[8 * s + 6], x[8 * s + 7])};
}

// key j visible to the query at position pos (causal: j <= pos; window W > 0: pos - j < W; j < Sk)
__device__ __forceinline__ bool d256_visible(int pos, int j, int Sk, bool causal, int window) {
    return j < Sk && (!causal || j <= pos) && (window <= 0 || pos - j < window);
}

// A whole tile of `rows` rows x 256 columns from a buffer descriptor into registers: 16-byte chunk i of thread t is chunk t + 256 i
template <class T, int ROWS>
struct TileLoad {
    static constexpr int CPR = D256Cfg<T>::RB / 16;
    static constexpr int N = ROWS * CPR / 256;
    u32x4_t r[N];
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, int row0, int tid) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int idx = tid + 256 * i;
            r[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (row0 + idx / CPR) * D256Cfg<T>::RB + (idx % CPR) * 16, 0, 0);
        }
    }
    __device__ __forceinline__ void store(char* lds, int pitch, int tid) const {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int idx = tid + 256 * i;
            *reinterpret_cast<u32x4_t*>(lds + (idx / CPR) * pitch + (idx % CPR) * 16) = r[i];
        }
    }
};

}  // namespace
}  // namespace aule_hip
