// fa_fwd_splitkv_fp8_gfx950.hip -- paged decode whose K and V caches are stored as OCP FP8 e4m3fn (one byte per
// element, what gfx950 speaks; MI300X's e4m3fnuz is a different encoding), with the query and the output in fp16 or
// bf16 and one fp32 dequantisation scale per KV head for K and for V:
//     K[pos, hk, :] = k_scale[hk] * float(k_cache[block, off, hk, :])       V likewise with v_scale
// It is the wave-per-chunk split-KV kernel of fa_fwd_splitkv_gfx950.hip (same GQA row packing, same partials, same
// chunk rule, same block-table walk; read that file's header first) with three differences:
//   * every finite e4m3fn code is exactly representable in fp16 and in bf16, so a cache element is converted to the
//     query's 16-bit type WITHOUT its scale (v_cvt_pk_f32_fp8 + one pack: exact, NaN codes stay NaN) and the 16-bit
//     MFMAs are kept -- no FP8 MFMA, no quantisation of Q or P;
//   * the scales stay out of the loop: k_scale[hk] multiplies the logits, so it is folded into the softmax factor c
//     (a unit is one (batch, kv-head)); v_scale[hk] multiplies the un-normalised O, so it is applied once where the
//     partial is written.  Both are fp32 device values: no host synchronisation, capturable;
//   * a row is D bytes.  A lane's 16-byte load carries 16 elements = two MFMA k-slices, so K needs half as many loads:
//     lane (key, hi) loads chunk 2j + hi and feeds its low / high 8 elements to MFMA steps 2j / 2j + 1 -- the order of
//     d inside the k dimension is free as long as the Q fragments use the same permutation (qf[2j + e] holds
//     d = 32j + 16hi + 8e .. +7).  V is converted before the LDS write (16 bytes of fp8 -> 32 bytes = two adjacent
//     chunks of the sub-tiled image), so the image, the transpose reads and the operand maps are the 16-bit kernel's.
// The partials are merged by the 16-bit path's combine kernels (launch_splitkv_combine).
#include "fa_device.h"
#include "fa_kernels.h"

namespace aule_hip {
namespace {

struct PagedFp8Params {
    const void* q;
    const void* k;             // [num_blocks, block_size, Hkv, D] e4m3fn
    const void* v;
    const float* k_scale;      // [Hkv]
    const float* v_scale;      // [Hkv]
    float* part;               // [npart][rows_total][D + 2] fp32: O (un-normalised, v_scale applied), m (log2 units), l
    int Hq, Hkv;
    float c;                   // scale * log2(e) (k_scale[hk] is multiplied in by the kernel)
    int nrt;                   // 32-row tiles per (batch, kv-head) unit
    int chunk_tiles;           // 32-key tiles per wave
    int rows_total;            // B * Hkv * nrt * 32
    const int* block_tables;   // [B, max_blocks]
    const int* context_lens;   // [B]
    int block_size, max_blocks;
    int window;
};

// sixteen e4m3fn codes (four dwords) -> elements 0..7 and 8..15 in the 16-bit type, exact
template <class T>
__device__ __forceinline__ void cvt16(u32x4_t x, u32x4_t& e0, u32x4_t& e1) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], false);
        const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)x[w], true);
        const unsigned lo = T::pack2(a[0], a[1]), hi = T::pack2(b[0], b[1]);
        if (w < 2) {
            e0[2 * w] = lo;
            e0[2 * w + 1] = hi;
        } else {
            e1[2 * w - 4] = lo;
            e1[2 * w - 3] = hi;
        }
    }
}

template <class T, int D>
__global__ void __launch_bounds__(256) fa_fwd_paged_fp8_kernel(const PagedFp8Params p) {
    using v8 = typename T::v8;
    constexpr int RB = D;                 // bytes of a cache row
    constexpr int KS = D / 16, DB = D / 32;
    constexpr int NK = KS / 2;            // 16-byte K loads per lane and tile
    constexpr int NV = D / 32;            // 16-byte V loads per lane and tile (32 rows * D / 16 chunks over 64 lanes)
    constexpr int VT = 32 * D * 2;        // one wave's V tile in LDS (16-bit)
    __shared__ __attribute__((aligned(16))) char smem[4 * VT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* const Vw = smem + wave * VT;

    const int g = p.Hq / p.Hkv;
    const int unit = blockIdx.y / p.nrt, rt = blockIdx.y % p.nrt;
    const int b = unit / p.Hkv, hk = unit % p.Hkv;
    // keys of this sequence, read on the device and bounded by what the block table can address
    const int Sk = min(max(p.context_lens[b], 0), p.max_blocks * p.block_size);
    const int row = rt * 32 + l31;                 // packed row of this lane inside the unit (one query token: row = head of the group)
    const bool valid = row < g;
    const int head = hk * g + (valid ? row : 0);

    // byte address of key/value row `kv` of this unit inside the cache (64-bit: caches exceed 4 GiB)
    const int* const bt = p.block_tables + (size_t)b * p.max_blocks;
    auto paged_row = [&](int kv) -> size_t {
        const int lb = kv / p.block_size, off = kv - lb * p.block_size;
        const size_t phys = (size_t)bt[min(lb, p.max_blocks - 1)];   // (tiles are rounded up: rows past Sk are masked, never out of the table)
        return ((phys * p.block_size + off) * p.Hkv + hk) * (size_t)RB;
    };

    // Q fragments (B operand of S^T = K.Q^T) in the k order of the FP8 K loads: qf[2j + e] of lane (row, hi) holds
    // d = 32j + 16hi + 8e .. +7; rows beyond the unit are 0
    v8 qf[KS];
    {
        const char* qrow = reinterpret_cast<const char*>(p.q) + (size_t)(b * p.Hq + head) * (D * 2);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4_t x = {0u, 0u, 0u, 0u};
            if (valid) x = *reinterpret_cast<const u32x4_t*>(qrow + (32 * (ks >> 1) + 16 * hi + 8 * (ks & 1)) * 2);
            qf[ks] = as_v8<T>(x);
        }
    }

    // V staging map: 16-byte fp8 chunk u = lane + 64 i becomes chunks 2u, 2u + 1 of the sub-tiled 16-bit image
    // ([kv/4][d/16][4][16] 16-byte chunks, filled linearly: fa_fwd_pp_gfx950.hip), i.e. 32 bytes at u * 32
    int v_row[NV], v_col[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int bidx = (lane >> 2) + 16 * i;   // sub-tile index = kv4 * (D/16) + d16
        v_row[i] = (bidx / (D / 16)) * 4 + (lane & 3);
        v_col[i] = (bidx % (D / 16)) * 16;       // byte = element offset inside the row
    }
    const int tr_off = hi * (D / 16) * 128 + ((lane >> 4) & 1) * 128 + (lane & 15) * 8;
    // fast path (power-of-two block size >= 8): block index inside the tile and byte offset inside the block
    const bool pow2 = p.block_size >= 8 && (p.block_size & (p.block_size - 1)) == 0;
    const int bs_log2 = 31 - __builtin_clz(p.block_size | 1);
    const size_t blk_bytes = (size_t)p.block_size * p.Hkv * RB;
    int k_jb = 0, k_off = 0, v_jb[NV], v_off[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) { v_jb[i] = 0; v_off[i] = 0; }
    if (pow2) {
        k_jb = l31 >> bs_log2;
        k_off = ((l31 & (p.block_size - 1)) * p.Hkv + hk) * RB + hi * 16;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v_jb[i] = v_row[i] >> bs_log2;
            v_off[i] = ((v_row[i] & (p.block_size - 1)) * p.Hkv + hk) * RB + v_col[i];
        }
    }

    f32x16_t o[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    float m = -INFINITY, l = 0.f;
    const float c = p.c * p.k_scale[hk];   // logits = k_scale * (q . codes) * scale: one fp32 factor per unit

    const int ntiles = (Sk + 31) / 32;
    int t0 = (blockIdx.x * 4 + wave) * p.chunk_tiles;
    const int t1 = min(t0 + p.chunk_tiles, ntiles);
    if (p.window > 0) t0 = max(t0, max(0, Sk - p.window) / 32);   // tiles entirely before the window
    f32x16_t z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;

    for (int t = t0; t < t1; ++t) {
        const int kv0 = t * 32;
        u32x4_t kx[NK], vx[NV];
        const u32x4_t zero = {0u, 0u, 0u, 0u};
        if (pow2) {
            // the tile's <= 4 logical blocks are looked up once per tile with wave-uniform loads; each lane picks its
            // block with selects and adds a 32-bit in-block offset computed once per launch
            const int lb0 = kv0 >> bs_log2;
            const size_t tile_off = (size_t)(kv0 & (p.block_size - 1)) * p.Hkv * RB;   // blocks larger than a tile
            // (four named values, not an array: the compiler turns selects over an array into an indexed read from scratch)
            const size_t pb0 = (size_t)bt[min(lb0, p.max_blocks - 1)] * blk_bytes + tile_off;
            const size_t pb1 = (size_t)bt[min(lb0 + 1, p.max_blocks - 1)] * blk_bytes + tile_off;
            const size_t pb2 = (size_t)bt[min(lb0 + 2, p.max_blocks - 1)] * blk_bytes + tile_off;
            const size_t pb3 = (size_t)bt[min(lb0 + 3, p.max_blocks - 1)] * blk_bytes + tile_off;
            auto pick = [&](int jb) -> size_t { return jb == 0 ? pb0 : (jb == 1 ? pb1 : (jb == 2 ? pb2 : pb3)); };
            const bool kin = kv0 + l31 < Sk;
            const char* krow = reinterpret_cast<const char*>(p.k) + pick(k_jb) + k_off;
#pragma unroll
            for (int j = 0; j < NK; ++j) kx[j] = kin ? *reinterpret_cast<const u32x4_t*>(krow + j * 32) : zero;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const bool vin = kv0 + v_row[i] < Sk;
                vx[i] = vin ? *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(p.v) + pick(v_jb[i]) + v_off[i]) : zero;
            }
        } else {
            const bool kin = kv0 + l31 < Sk;
            const char* krow = reinterpret_cast<const char*>(p.k) + (kin ? paged_row(kv0 + l31) : 0) + hi * 16;
#pragma unroll
            for (int j = 0; j < NK; ++j) kx[j] = kin ? *reinterpret_cast<const u32x4_t*>(krow + j * 32) : zero;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const bool vin = kv0 + v_row[i] < Sk;
                vx[i] = vin ? *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const char*>(p.v) + paged_row(kv0 + v_row[i]) + v_col[i]) : zero;
            }
        }
        f32x16_t s;
#pragma unroll
        for (int j = 0; j < NK; ++j) {
            u32x4_t e0, e1;
            cvt16<T>(kx[j], e0, e1);
            s = T::mfma(as_v8<T>(e0), qf[2 * j], j == 0 ? z : s);
            s = T::mfma(as_v8<T>(e1), qf[2 * j + 1], s);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            u32x4_t e0, e1;
            cvt16<T>(vx[i], e0, e1);
            *reinterpret_cast<u32x4_t*>(Vw + lane * 32 + i * 2048) = e0;
            *reinterpret_cast<u32x4_t*>(Vw + lane * 32 + i * 2048 + 16) = e1;
        }

        // online softmax over this tile's 32 keys (16 per lane half), exp2 domain
        const bool ragged = kv0 + 32 > Sk || (p.window > 0 && Sk - 1 - kv0 >= p.window);
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float x = s[r] * c;
            if (ragged) {
                const int kv = kv0 + crow(r, hi);
                if (kv >= Sk || (p.window > 0 && Sk - 1 - kv >= p.window)) x = -INFINITY;
            }
            s[r] = x;
            mx = fmaxf(mx, x);
        }
        mx = fmaxf(mx, xhalf(mx));
        const float m_new = fmaxf(m, mx);   // finite: every tile has at least one key < Sk
        const float alpha = fast_exp2(m - m_new);
        m = m_new;
        float ls = 0.f;
        u32x4_t pu[2];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float p0 = fast_exp2(s[2 * i] - m_new), p1 = fast_exp2(s[2 * i + 1] - m_new);
            ls += p0 + p1;
            pu[i >> 2][i & 3] = T::pack2(p0, p1);
        }
        l = l * alpha + ls;
#pragma unroll
        for (int d = 0; d < DB; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        // O^T += V^T . P^T  (A by transpose read from the wave's LDS tile; k-slot order = S accumulator order)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int d = 0; d < DB; ++d) {
                const int off = ((4 * kk) * (D / 16) + 2 * d) * 128;
                const s16x4_t a0 = lds_tr16(Vw + tr_off + off);
                const s16x4_t a1 = lds_tr16(Vw + tr_off + off + 2 * (D / 16) * 128);
                o[d] = T::mfma(as_v8<T>(a0, a1), as_v8<T>(pu[kk]), o[d]);
            }
    }

    // partial of this wave: O (un-normalised, times v_scale[hk]), m, l of the lane's row
    const float vs = p.v_scale[hk];
    const float lt = l + xhalf(l);
    const int pi = blockIdx.x * 4 + wave;
    const size_t prow = (size_t)pi * p.rows_total + (size_t)blockIdx.y * 32 + l31;
    float* dst = p.part + prow * (D + 2);
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4_t x = {o[d][4 * g4] * vs, o[d][4 * g4 + 1] * vs, o[d][4 * g4 + 2] * vs, o[d][4 * g4 + 3] * vs};
            *reinterpret_cast<f32x4_t*>(dst + 32 * d + 8 * g4 + 4 * hi) = x;
        }
    if (hi == 0) {
        dst[D] = m;
        dst[D + 1] = lt;
    }
}

// Same plan as launch_paged (fa_fwd_splitkv_gfx950.hip): ~2048 waves whatever the shape and whatever the bytes per key,
// so the workspace is the 16-bit call's.
template <class T, int D>
int launch_paged_fp8_t(const PagedArgs& a, hipStream_t stream) {
    PagedFp8Params p;
    p.q = a.q; p.k = a.k_cache; p.v = a.v_cache; p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.Hq = a.Hq; p.Hkv = a.Hkv;
    p.c = a.scale * kLog2e;
    const int g = a.Hq / a.Hkv;
    p.nrt = (g + 31) / 32;
    const int units = a.B * a.Hkv * p.nrt;
    const int ntiles = (a.max_blocks * a.block_size + 31) / 32;
    const int want_waves = (2048 + units - 1) / units;
    p.chunk_tiles = (ntiles + want_waves - 1) / want_waves;
    if (p.chunk_tiles < 1) p.chunk_tiles = 1;
    const int nwaves = (ntiles + p.chunk_tiles - 1) / p.chunk_tiles;
    const int nsplit = (nwaves + 3) / 4;
    const int npart = nsplit * 4;
    p.rows_total = units * 32;
    p.block_tables = a.block_tables; p.context_lens = a.context_lens;
    p.block_size = a.block_size; p.max_blocks = a.max_blocks; p.window = a.window > 0 ? a.window : 0;
    const size_t bytes = (size_t)npart * p.rows_total * (D + 2) * sizeof(float);
    if (a.query_ws != nullptr) {
        *a.query_ws = bytes;
        return 0;
    }
    ScopedWorkspace ws(bytes, a.ws, a.ws_bytes, stream);
    if (ws.err != hipSuccess) return (int)ws.err;
    p.part = static_cast<float*>(ws.ptr);
    hipLaunchKernelGGL((fa_fwd_paged_fp8_kernel<T, D>), dim3((unsigned)nsplit, (unsigned)units), dim3(256), 0, stream, p);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    FwdArgs f;
    f.q = a.q; f.k = nullptr; f.v = nullptr; f.o = a.out; f.lse = nullptr;
    f.B = a.B; f.Hq = a.Hq; f.Hkv = a.Hkv; f.Sq = 1; f.Sk = a.max_blocks * a.block_size; f.D = D;
    f.scale = a.scale; f.causal = 0; f.dtype = a.dtype;
    return launch_splitkv_combine(f, p.part, npart, p.nrt, stream);
}

}  // namespace

int launch_paged_decode_fp8(const PagedArgs& a, hipStream_t stream) {
    if (a.cache_kind != kCacheFp8E4M3 || (a.query_ws == nullptr && (a.k_scale == nullptr || a.v_scale == nullptr))) return -1;
    if (a.dtype == kBF16) {
        if (a.D == 128) return launch_paged_fp8_t<Bf16Traits, 128>(a, stream);
        if (a.D == 64) return launch_paged_fp8_t<Bf16Traits, 64>(a, stream);
        if (a.D == 32) return launch_paged_fp8_t<Bf16Traits, 32>(a, stream);
    } else if (a.dtype == kF16) {
        if (a.D == 128) return launch_paged_fp8_t<F16Traits, 128>(a, stream);
        if (a.D == 64) return launch_paged_fp8_t<F16Traits, 64>(a, stream);
        if (a.D == 32) return launch_paged_fp8_t<F16Traits, 32>(a, stream);
    }
    return -1;
}

uint64_t paged_fp8_workspace_bytes(PagedArgs a) {
    uint64_t bytes = 0;
    a.query_ws = &bytes;
    (void)launch_paged_decode_fp8(a, nullptr);
    return bytes;
}

}  // namespace aule_hip
