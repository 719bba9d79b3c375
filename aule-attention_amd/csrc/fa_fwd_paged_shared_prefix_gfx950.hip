// fa_fwd_paged_shared_prefix_gfx950.hip -- the shared-prefix pass of the paged cascade.
//
// Sequences of a serving batch usually share a system prompt: their block tables start with the same blocks.  This pass reads that
// prefix ONCE for the whole batch: every one of the T tokens of q [T, Hq, D] sees the P = clamp(prefix_len[0], 0, capacity) keys
// behind prefix_block_table [max_prefix_blocks] -- no mask, no per-sequence data -- so the rows of all sequences pack into one dense
// problem per KV head: packed row r = token r / g, head hk g + r % g (the prefill's token-major packing without the sequence
// boundaries), R = T g rows.
// Work item = (KV head, block of 128 rows, key split k of nsplit), 4 waves x 32 rows; the layout is the prefill kernel's
// (fa_paged_tile.h, fa_d256_common.h): Q of the lane's row in registers, K / V tiles of 64 keys through LDS, the table walked one
// tile ahead of the loads and the loads one tile ahead of the MFMAs, FP8 codes converted on the way into LDS, k_scale[hk] in the
// log2-unit score factor.  Split k owns tiles [k tps, (k + 1) tps) of the prefix; tps comes from the host's plan, which knows only
// the table's capacity, P from the device: a split at or beyond P has no key.
// Each item writes the fp32 partial of its rows in the split-KV family's format, part [nsplit][T Hq][D + 2]: un-normalised O with
// v_scale[hk] applied, m in log2 units, l; a split without a key writes m = -inf, l = 0 and no O.  fa_merge_states_gfx950.hip merges
// them with the per-sequence state.
// A table entry at logical block >= ceil(P / bs) is never dereferenced, a key row at or beyond P never read (zeros in LDS, masked),
// lanes past R store nothing.
#include "fa_kernels.h"
#include "fa_tile_attention.h"

namespace aule_hip {
namespace {

struct SharedPrefixParams {
    const char* q;
    const char* k;
    const char* v;
    float* part;
    const int* table;
    const int* plen;
    const float* k_scale;
    const float* v_scale;
    long long q_stride;      // elements between tokens of q
    long long part_stride;   // floats between the partials of two splits: T * Hq * (D + 2)
    int Hq, Hkv, g, R;
    int bs, bs_shift;        // bs_shift >= 0: bs = 1 << bs_shift
    int max_blocks;
    int nrb, tps;            // row blocks; tiles per split
    float c;                 // scale * log2(e) (sign kept)
};

template <class T, int D, class KV>
__global__ void __launch_bounds__(256, 1) fa_fwd_paged_shared_prefix_kernel(const SharedPrefixParams p) {
    using C = PrefillCfg<D>;
    constexpr bool FP8 = std::is_same<KV, KvFp8>::value;
    __shared__ __attribute__((aligned(16))) char Ks[kPK * C::PA];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * C::PT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // work item: KV head fastest (with Hkv % 8 == 0 a KV head stays on one XCD), then the row blocks that share a key range
    const int bid = (int)blockIdx.x;
    const int hk = bid % p.Hkv, rest = bid / p.Hkv;
    const int rb = rest % p.nrb, ks = rest / p.nrb;

    // the prefix, clamped; this split's keys [kbeg, kend)
    const int P = min(max(p.plen[0], 0), p.max_blocks * p.bs);   // (capacity < 2^30: the host checks)
    const int kbeg = ks * p.tps * kPK;
    const int kend = min(P, kbeg + p.tps * kPK);
    const int ntiles = kend > kbeg ? (kend - kbeg + kPK - 1) / kPK : 0;

    // this lane's row (a lane past the end works on the block's last row and stores nothing)
    const int r0 = rb * kPQ;
    const int rows = min(kPQ, p.R - r0);   // >= 1
    const int rl = wave * 32 + l31;
    const bool live = rl < rows;
    const bool wave_live = wave * 32 < rows;
    const int r = r0 + min(rl, rows - 1);
    const int tok = r / p.g, head = hk * p.g + r % p.g;
    const long long orow = (long long)tok * p.Hq + head;
    float* pr = p.part + ks * p.part_stride + orow * (D + 2);

    if (ntiles == 0) {
        if (live && hi == 0) *reinterpret_cast<f32x2_t*>(pr + D) = f32x2_t{-__builtin_inff(), 0.f};
        return;
    }

    // Q operand chunks of this lane's row
    const char* qrow = p.q + ((long long)tok * p.q_stride + (long long)head * D) * 2;
    u32x4_t qf[C::G];
#pragma unroll
    for (int g = 0; g < C::G; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    float c = p.c;
    if constexpr (FP8) c *= p.k_scale[hk];

    f32x16_t o[C::DT];
#pragma unroll
    for (int i = 0; i < C::DT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    PagedTile<T, D, FP8> kt;
    kt.lookup(p, p.table, kbeg, kend, tid);
    kt.load(p, hk, kbeg, kend, tid);
    kt.lookup(p, p.table, kbeg + kPK, kend, tid);
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kPK;
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, Vs, tid);
        __syncthreads();
        if (t + 1 < ntiles) {
            kt.load(p, hk, k0 + kPK, kend, tid);
            kt.lookup(p, p.table, k0 + 2 * kPK, kend, tid);
        }
        if (!wave_live) continue;
        // S^T[key][row] = K.Q^T over the 64 keys of the tile
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
#pragma unroll
        for (int g = 0; g < C::G; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                sc[kk] = mfma16<T>(lds_b128(Ks + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), qf[g], sc[kk]);
        // scale to log2 units, running max over the lane pair (lanes l and l + 32 hold the same row); only the split's last tile can
        // hold keys at or beyond kend
        float mx = -__builtin_inff();
        if (k0 + kPK <= kend) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const float x = sc[kk][rr] * c;
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
                }
        } else {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int rr = 0; rr < 16; ++rr) {
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const float x = j < kend ? sc[kk][rr] * c : -__builtin_inff();
                    sc[kk][rr] = x;
                    mx = fmaxf(mx, x);
                }
        }
        mx = fmaxf(mx, xhalf(mx));
        const float mn = fmaxf(m, mx);
        const float mu = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(m - mu);   // m = -inf: 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < C::DT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - mu);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < C::DT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, C::PT, 16 * st, 32 * dt, lane), pb, o[dt]);
        }
    }
    l += xhalf(l);
    if (!live) return;
    float vs = 1.f;
    if constexpr (FP8) vs = p.v_scale[hk];
    // (a row of the partial is (D + 2) * 4 bytes: 8-byte aligned)
#pragma unroll
    for (int dt = 0; dt < C::DT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            *reinterpret_cast<f32x2_t*>(pr + d) = f32x2_t{o[dt][4 * g4] * vs, o[dt][4 * g4 + 1] * vs};
            *reinterpret_cast<f32x2_t*>(pr + d + 2) = f32x2_t{o[dt][4 * g4 + 2] * vs, o[dt][4 * g4 + 3] * vs};
        }
    if (hi == 0) *reinterpret_cast<f32x2_t*>(pr + D) = f32x2_t{m, l};
}

}  // namespace

// The plan.  Row blocks x KV heads are the items one key range gives; the keys are split until the items cover the device's CUs
// once, bounded by the tiles the table can address and by kSharedPrefixMaxSplit (every split costs one partial per row to write and
// to merge); then the tiles are dealt evenly and nsplit recounted, so that no split is empty by capacity.
SharedPrefixPlan shared_prefix_plan(const SharedPrefixArgs& a) {
    SharedPrefixPlan pl;
    if (a.T <= 0 || a.Hkv <= 0 || a.Hq <= 0 || a.Hq % a.Hkv != 0 || a.block_size <= 0 || a.max_prefix_blocks <= 0) return pl;
    const long long cap = (long long)a.block_size * a.max_prefix_blocks;
    const long long R = (long long)a.T * (a.Hq / a.Hkv);
    if (cap >= (1ll << 30) || R + kPQ > 0x7fffffffll) return pl;
    pl.row_blocks = (int)((R + kPQ - 1) / kPQ);
    pl.tiles = (int)((cap + kPK - 1) / kPK);
    const long long base = (long long)pl.row_blocks * a.Hkv;
    long long want = (device_cu_count(a.device) + base - 1) / base;
    if (want > kSharedPrefixMaxSplit) want = kSharedPrefixMaxSplit;
    if (want > pl.tiles) want = pl.tiles;
    if (want < 1) want = 1;
    pl.tiles_per_split = (int)((pl.tiles + want - 1) / want);
    pl.nsplit = (pl.tiles + pl.tiles_per_split - 1) / pl.tiles_per_split;
    pl.grid = base * pl.nsplit;
    const uint64_t rows = (uint64_t)a.T * a.Hq;
    pl.part_bytes = (uint64_t)pl.nsplit * rows * (a.D + 2) * 4;
    pl.lse_offset = (pl.part_bytes + 15) & ~15ull;
    pl.ws_bytes = (pl.lse_offset + rows * 4 + 15) & ~15ull;
    return pl;
}

int launch_shared_prefix(const SharedPrefixArgs& a, const SharedPrefixPlan& pl, hipStream_t stream) {
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (a.cache_kind != kCache16 && !fp8) return -1;
    if (fp8 && (a.k_scale == nullptr || a.v_scale == nullptr)) return -1;
    if (a.q_token_stride < (long long)a.Hq * a.D || a.q_token_stride % 8 != 0) return -1;
    if (pl.grid <= 0 || pl.grid > 0x7fffffffll || a.part == nullptr || a.prefix_block_table == nullptr || a.prefix_len == nullptr) return -1;
    SharedPrefixParams p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k_cache); p.v = static_cast<const char*>(a.v_cache);
    p.part = a.part;
    p.table = a.prefix_block_table; p.plen = a.prefix_len;
    p.k_scale = a.k_scale; p.v_scale = a.v_scale;
    p.q_stride = a.q_token_stride;
    p.part_stride = (long long)a.T * a.Hq * (a.D + 2);
    p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv; p.R = a.T * p.g;
    p.bs = a.block_size;
    p.bs_shift = shift_of(a.block_size);
    p.max_blocks = a.max_prefix_blocks;
    p.nrb = pl.row_blocks; p.tps = pl.tiles_per_split;
    p.c = a.scale * kLog2e;
    return dispatch_tile_instance(a.dtype, a.D, fp8, [&](auto t, auto d, auto kv) {
        hipLaunchKernelGGL((fa_fwd_paged_shared_prefix_kernel<decltype(t), decltype(d)::value, decltype(kv)>), dim3((unsigned)pl.grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
