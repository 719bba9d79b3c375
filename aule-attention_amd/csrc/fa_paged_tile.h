// fa_paged_tile.h -- what the tiled paged kernels share (fa_fwd_paged_prefill_gfx950.hip, fa_fwd_paged_shared_prefix_gfx950.hip):
// the two cache kinds, the tile sizes, the LDS pitches per head_dim and the K / V tile on its way from the block pool to LDS.
// The kernel's parameter struct P supplies k, v (const char*), Hkv, bs and bs_shift (>= 0: bs = 1 << bs_shift).
// Device code only.
#pragma once
#include <type_traits>

#include "fa_d256_common.h"
#include "kv_quant.h"

namespace aule_hip {
namespace {

struct Kv16 {};    // caches of q's dtype
struct KvFp8 {};   // caches of e4m3fn codes

constexpr int kPQ = 128;   // packed rows per workgroup
constexpr int kPK = 64;    // keys per tile

template <int D>
struct PrefillCfg {
    static constexpr int RB = D * 2;                       // bytes of a 16-bit row
    static constexpr int G = D / 16;                       // operand chunk pairs per row
    static constexpr int DT = D / 32;                      // O accumulators
    static constexpr int PA = RB + 16;                     // K image pitch (ds_read_b128 rows shift by one slot)
    static constexpr int PT = RB >= 256 ? RB + 64 : 192;   // V image pitch (transposed reads: four rows land in four 64-byte segments)
    static constexpr int CPR = D / 8;                      // 8-element chunks per row
    static constexpr int N = kPK * CPR / 256;              // chunks per thread and tile
};

// (cvt8, eight e4m3fn codes -> eight 16-bit elements: kv_quant.h, beside the quantiser)

// One K and one V tile of 64 keys on their way from the block pool to LDS: chunk i of thread t is 8-element chunk t + 256 i
// (row (t + 256 i) / CPR of the tile), 16 bytes of a 16-bit cache or 8 codes of an FP8 one.
template <class T, int D, bool FP8>
struct PagedTile {
    using C = PrefillCfg<D>;
    using Raw = typename std::conditional<FP8, u32x2_t, u32x4_t>::type;
    static constexpr int EB = FP8 ? 1 : 2;
    Raw k[C::N], v[C::N];
    long long slot[C::N];   // cache slot (block * bs + offset) of this thread's rows of the tile load() takes next
    // the table walk for keys k0 .. k0 + 63 of the sequence whose table row is `tab`, one tile ahead of the rows themselves: the
    // loads of K / V then do not wait for a table entry.  Keys >= kend are neither looked up nor read.
    template <class P>
    __device__ __forceinline__ void lookup(const P& p, const int* tab, int k0, int kend, int tid) {
#pragma unroll
        for (int i = 0; i < C::N; ++i) {
            const int kv = k0 + (tid + 256 * i) / C::CPR;
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
        for (int i = 0; i < C::N; ++i) {
            const int idx = tid + 256 * i;
            const int kv = k0 + idx / C::CPR;
            Raw kx = Raw{}, vx = Raw{};
            if (kv < kend) {
                const long long at = ((slot[i] * p.Hkv + hk) * D + (idx % C::CPR) * 8) * EB;
                kx = *reinterpret_cast<const Raw*>(p.k + at);
                vx = *reinterpret_cast<const Raw*>(p.v + at);
            }
            k[i] = kx;
            v[i] = vx;
        }
    }
    __device__ __forceinline__ void store(char* Ks, char* Vs, int tid) const {
#pragma unroll
        for (int i = 0; i < C::N; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx / C::CPR, cc = idx % C::CPR;
            u32x4_t kx, vx;
            if constexpr (FP8) {
                kx = cvt8<T>(k[i]);
                vx = cvt8<T>(v[i]);
            } else {
                kx = k[i];
                vx = v[i];
            }
            *reinterpret_cast<u32x4_t*>(Ks + row * C::PA + cc * 16) = kx;
            *reinterpret_cast<u32x4_t*>(Vs + row * C::PT + cc * 16) = vx;
        }
    }
};

}  // namespace
}  // namespace aule_hip
