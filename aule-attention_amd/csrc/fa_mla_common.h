// fa_mla_common.h -- what the translation units of the absorbed MLA share (fa_fwd_mla_paged_gfx950.hip: caches of q's dtype, the
// combine, the plan and the launch; fa_fwd_mla_paged_fp8_gfx950.hip: caches of e4m3fn codes; fa_fwd_mla_sparse_gfx950.hip: keys from a
// per-token list; fa_fwd_mla_verify_gfx950.hip: the dense call with a tree of new tokens): the sizes, the kernels' parameter struct, the
// clamps of the contract, the latent tile per cache kind, the list's key source, the tree's visibility words and the ONE body of the
// attention kernel.  The layout and the arithmetic are described at the top of
// fa_fwd_mla_paged_gfx950.hip.  Device code only.
#pragma once
#include "fa_kernels.h"
#include "fa_paged_tile.h"

namespace aule_hip {

struct MlaParams {
    const char* q;
    const char* kv;
    char* o;
    float* lse;
    float* part_o;    // nsplit > 1: [nsplit][T * Hq][512]
    float* part_ml;   //             [nsplit][T * Hq][2]
    const int* table;
    const int* ctx;
    const int* cu;    // null: sequence b owns row b
    long long q_stride;
    long long rows_total;   // T * Hq
    int T, B, Hq;
    int bs, bs_shift;
    int max_blocks, max_sq;
    int row_blocks, nsplit;
    float c;
    const float* kv_scale;   // FP8 cache: [1] fp32 on the device, key = kv_scale * float(code); else null
    // The sparse call (fa_fwd_mla_sparse_gfx950.hip): token b's keys are the cache rows that list[b * topk + i] names.  table, ctx and
    // cu are null there and B = T; the dense call leaves these three as they stand.
    const int* list = nullptr;   // [T][topk] slots; an entry outside [0, slots) is skipped
    int topk = 0;
    int slots = 0;               // rows of the cache read as a flat array
    // The dense call with tree masks (fa_fwd_mla_verify_gfx950.hip): one word per packed token, read by those instances alone.  The LAST
    // field: every other instance, the combine included, keeps its argument offsets.
    const long long* tree_mask = nullptr;   // [T] int64
};


// The FP8 attention kernel for `p` (fa_fwd_mla_paged_fp8_gfx950.hip; dtype: of q / out); partials and combine are the 16-bit call's.
int launch_mla_fp8_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream);
// ... and the sparse call's (`p` as launch_mla_sparse fills it, kv_scale set), beside it in that translation unit.
int launch_mla_sparse_fp8_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream);
// The dense call's attention kernel with tree masks, either cache kind (fa_fwd_mla_verify_gfx950.hip; `p` as launch_mla_paged fills it,
// tree_mask and cu set).
int launch_mla_verify_kernel(const MlaParams& p, long long grid, int dtype, hipStream_t stream);
// The combine of either call's partials (fa_fwd_mla_paged_gfx950.hip): row_blocks * p.B * 16 workgroups, after the attention kernel.
int launch_mla_combine(const MlaParams& p, int row_blocks, int dtype, hipStream_t stream);

// The split rule of both plans (fa_fwd_mla_paged_gfx950.hip): `row_blocks` blocks of rows per unit, `units` sequences or tokens, `tiles`
// 64-key tiles a split could own at most.  nsplit covers the device's compute units with row_blocks * units * nsplit workgroups, at most
// kMlaMaxSplit and at most one split per two tiles (a split is worth a launch slot only with some keys to read); nsplit > 0 (the sparse
// debug path's force_nsplit alone): that many instead.  The workspace is round16(nsplit * T * Hq * 514 * 4) bytes when nsplit > 1.
MlaPlan mla_split_plan(long long row_blocks, long long units, long long tiles, int T, int Hq, int device, long long nsplit = 0);

namespace {

constexpr int kMlaQK = 576;                     // key / query width
constexpr int kMlaV = 512;                      // value width
constexpr int kMlaKeys = 64;                    // keys per tile
constexpr int kMlaRB = kMlaQK * 2;              // bytes of a latent row in LDS (and in a 16-bit cache)
constexpr int kMlaPitch = kMlaRB + 80;          // LDS pitch of the image: read as A operand rows AND transposed
constexpr int kMlaG = kMlaQK / 16 / 2;          // operand chunk pairs of a wave's half of the reduction: 18
constexpr int kMlaDT = kMlaV / 32 / 2;          // O accumulators of a wave's half of the value columns: 8
constexpr int kMlaN = kMlaRB / 16 / 8;          // 16-byte chunks per thread and latent row: 9 (8 threads per row)
constexpr int kMlaLdsImage = kMlaKeys * kMlaPitch;   // bytes of the latent image
constexpr int kMlaLdsScores = 4 * 8 * 1024;           // partial scores: [wave][register quad][lane] 16 bytes

// Host: what launch_mla_paged and launch_mla_sparse (A: MlaArgs, MlaSparseArgs) refuse alike, and the fields of `p` they fill alike --
// the tensors, the workspace's two parts (`ws`: plan.ws_bytes bytes, 16-byte aligned, when plan.nsplit > 1), the row counts, the plan,
// the score scale and the FP8 scale.  The key source's fields (table, lengths and offsets, or the list) are the caller's.  -1: refused.
template <class A>
int mla_common_params(const A& a, const MlaPlan& plan, void* ws, MlaParams& p) {
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll) return -1;
    if (a.q_token_stride < (long long)a.Hq * kMlaQK || a.q_token_stride % 8 != 0) return -1;
    if (((long long)a.T + kMlaRows) * a.Hq > 0x7fffffffll) return -1;   // the kernels count packed rows in 32 bits
    if (plan.nsplit > 1 && ws == nullptr) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 ? a.kv_scale == nullptr : a.cache_kind != kCache16) return -1;
    p.q = static_cast<const char*>(a.q); p.kv = static_cast<const char*>(a.kv_cache);
    p.o = static_cast<char*>(a.out); p.lse = a.lse;
    p.rows_total = (long long)a.T * a.Hq;
    p.part_o = static_cast<float*>(ws);
    p.part_ml = p.part_o != nullptr ? p.part_o + (long long)plan.nsplit * p.rows_total * kMlaV : nullptr;
    p.q_stride = a.q_token_stride;
    p.T = a.T; p.Hq = a.Hq;
    p.row_blocks = plan.row_blocks; p.nsplit = plan.nsplit;
    p.c = a.scale * kLog2e;
    p.kv_scale = fp8 ? a.kv_scale : nullptr;
    return 0;
}

// what both kernels derive for workgroup (rank, sequence b): the clamps of the contract and the block of packed rows
struct MlaBlock {
    int L, s, n;
    int r0, rows;   // rows == 0: nothing to do
    __device__ __forceinline__ MlaBlock(const MlaParams& p, int b, int rank) {
        L = seq_len(p.ctx, b, p.max_blocks * p.bs);   // (the capacity < 2^30: the host checks)
        const SeqRange q = seq_range_or_row(p.cu, b, p.T, p.max_sq);   // (a null cu: b < T, the host checks)
        s = q.s;
        n = q.n;
        const int R = n * p.Hq;   // (T + 64) * Hq < 2^31: the host checks
        const int own = (R + kMlaRows - 1) / kMlaRows;
        r0 = 0;
        rows = 0;
        if (rank < own) {
            r0 = (own - 1 - rank) * kMlaRows;   // rank 0 is the sequence's last block, as in the paged prefill
            rows = min(kMlaRows, R - r0);
        }
    }
    // the sparse call: token b is a sequence of its own, its Hq heads cut into blocks in rank order; no length is read
    struct ListRows {};
    __device__ __forceinline__ MlaBlock(const MlaParams& p, int b, int rank, ListRows) {
        L = 0;
        s = b;   // (b < T: the grid)
        n = 1;
        r0 = rank * kMlaRows;
        rows = max(min(kMlaRows, p.Hq - r0), 0);
    }
};

// the block of workgroup (rank, b) for the body's key source
template <bool kList>
__device__ __forceinline__ MlaBlock mla_block(const MlaParams& p, int b, int rank) {
    if constexpr (kList) return MlaBlock(p, b, rank, MlaBlock::ListRows{});
    else return MlaBlock(p, b, rank);
}

// The sparse call's key source: key k of token b is entry k of its list, a slot of the flat cache; an entry outside [0, slots) names
// no row -- its image row is zeros and its score masked.  The mask of a tile is ONE wave-uniform word: lane i holds entry k0 + i (one
// coalesced 256-byte request, made a tile ahead) and the wave ballots its validity; each lane shifts the word once by its half's row
// offset (4 hi) into two 32-bit words, so that element rr of sc[kk] tests the COMPILE-TIME bit crow(rr, 0) of word kk.  (A
// per-element 64-bit shift by 32 kk + crow(rr, hi) spills 51 registers; this costs the entry and, while a tile is masked, two words.)
struct MlaListKeys {
    const int* list;
    int kbeg, kend;
    unsigned slots;
    int entry;       // lane i: entry k0 + i of the tile whose scores are masked next
    unsigned w[2];   // validity of the tile's keys 32 kk + 4 hi + (0 .. 31 - 4 hi)
    // this split's entries: whole tiles of the list
    __device__ __forceinline__ MlaListKeys(const MlaParams& p, int b, int split) {
        const int tiles = (p.topk + kMlaKeys - 1) / kMlaKeys;
        const int per = (tiles + p.nsplit - 1) / p.nsplit;
        kbeg = split * per * kMlaKeys;
        kend = min((split + 1) * per * kMlaKeys, p.topk);
        list = p.list + (long long)b * p.topk;
        slots = (unsigned)p.slots;
        entry = -1;
    }
    // the cache row of key kv, -1: none (past the range, or an entry outside the cache)
    __device__ __forceinline__ long long slot(int kv) const {
        long long at = -1;
        if (kv < kend) {
            const int e = list[kv];
            if ((unsigned)e < slots) at = e;
        }
        return at;
    }
    __device__ __forceinline__ void fetch_mask(int k0, int lane) {
        const int k = k0 + lane;
        entry = k < kend ? list[k] : -1;
    }
    __device__ __forceinline__ void tile_mask(int hi) {
        const unsigned long long vm = __builtin_amdgcn_ballot_w64((unsigned)entry < slots);
        w[0] = (unsigned)(vm >> (4 * hi));
        w[1] = (unsigned)(vm >> (32 + 4 * hi));
    }
    __device__ __forceinline__ bool visible(int kk, int rr) const { return ((w[kk] >> crow(rr, 0)) & 1u) != 0; }
};

// (what the dense instances hold in its place: nothing)
struct MlaNoList {
    static constexpr int kbeg = 0, kend = 0;
    __device__ __forceinline__ MlaNoList(const MlaParams&, int, int) {}
    __device__ __forceinline__ bool visible(int, int) const { return false; }
};

// The tree call's visibility (tree masks: DESIGN.md 3.18; the rule is aule_mla_paged_tree_desc's in include/aule.h).  A sequence with
// n <= 64 new tokens carries a tree: its token at position base + i, base = L - n, sees key j < L iff j < base or bit j - base of ITS
// word is set; a longer sequence keeps the causal rule and no word is read.  Either way the lane states what its row sees of a tile
// as ONE 64-bit word, built once per tile from the lane's word (kept as two 32-bit halves; 64-bit shifts happen here, a handful per
// tile, never per element), and shifted by the lane half's row offset into two 32-bit words exactly as MlaListKeys does -- so the
// per-element test is the list's: the COMPILE-TIME bit crow(rr, 0) of word kk, one test where the dense twin has two compares, in a
// tile of pure context as in a tile of new tokens.
struct MlaTreeKeys {
    unsigned lo, hi32;   // the lane's word; a causal row: unused
    int base;            // tree: L - n, the first new token's position; causal: the row's last visible key + 1
    bool tree;           // wave-uniform: the sequence carries a tree
    unsigned w[2];
    // (pos: the row's position, L - n + token; word: where the row's word lies)
    __device__ __forceinline__ MlaTreeKeys(const long long* word, int L, int n, int pos) {
        tree = n <= 64;
        lo = 0; hi32 = 0;
        base = pos + 1;
        if (tree) {
            const unsigned long long x = (unsigned long long)*word;
            // a row at a negative position sees nothing, whatever its word says
            lo = pos < 0 ? 0u : (unsigned)x;
            hi32 = pos < 0 ? 0u : (unsigned)(x >> 32);
            base = L - n;
        }
    }
    // the low `count` bits set, count clamped to 0 .. 64
    static __device__ __forceinline__ unsigned long long low_bits(int count) {
        return count >= 64 ? ~0ull : count <= 0 ? 0ull : (1ull << count) - 1ull;
    }
    // bit t of the tile's word: key k0 + t counts for this row (kend: the end of the workgroup's key range, at most L)
    __device__ __forceinline__ void tile_mask(int k0, int kend, int hi) {
        const int d = base - k0;   // keys of the tile below base: context keys (tree), or every visible key (causal)
        unsigned long long vm = low_bits(d);
        if (tree) {
            const unsigned long long x = ((unsigned long long)hi32 << 32) | lo;
            // bit b of the word is key base + b = bit d + b of the tile (b < n <= 64)
            vm |= d >= 64 || d <= -64 ? 0ull : d >= 0 ? x << d : x >> -d;
        }
        vm &= low_bits(kend - k0);
        w[0] = (unsigned)(vm >> (4 * hi));
        w[1] = (unsigned)(vm >> (32 + 4 * hi));
    }
    __device__ __forceinline__ bool visible(int kk, int rr) const { return ((w[kk] >> crow(rr, 0)) & 1u) != 0; }
};

// (what the other instances hold in its place: nothing)
struct MlaNoTree {
    static constexpr bool tree = false;
    __device__ __forceinline__ MlaNoTree(const long long*, int, int, int) {}
    __device__ __forceinline__ void tile_mask(int, int, int) {}
    __device__ __forceinline__ bool visible(int, int) const { return false; }
};

// One latent tile of 64 keys on its way from the block pool to LDS: thread t takes rows (t >> 3) and (t >> 3) + 32 of the tile,
// 8-element chunks (t & 7) + 8 i of each -- 16 bytes of a 16-bit cache (Kv16), 8 codes of an FP8 one (KvFp8), which store() converts
// exactly (cvt8) to the 16-bit type, so the image in LDS is the same for both kinds.
template <class T, class KV>
struct MlaTile {
    static constexpr bool kFp8 = std::is_same<KV, KvFp8>::value;
    using Raw = typename std::conditional<kFp8, u32x2_t, u32x4_t>::type;
    static constexpr int EB = kFp8 ? 1 : 2;   // bytes per cache element
    Raw d[2][kMlaN];
    long long slot[2];
    __device__ __forceinline__ void lookup(const MlaParams& p, const int* tab, int k0, int kend, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kv = k0 + (tid >> 3) + 32 * j;
            long long at = 0;
            if (kv < kend) {
                const int lb = block_of(kv, p.bs, p.bs_shift);
                at = (long long)tab[lb] * p.bs + (kv - lb * p.bs);
            }
            slot[j] = at;
        }
    }
    __device__ __forceinline__ void load(const MlaParams& p, int k0, int kend, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kv = k0 + (tid >> 3) + 32 * j;
            const char* row = p.kv + slot[j] * (kMlaQK * EB) + (tid & 7) * (8 * EB);
#pragma unroll
            for (int i = 0; i < kMlaN; ++i) d[j][i] = kv < kend ? *reinterpret_cast<const Raw*>(row + 64 * EB * i) : Raw{};
        }
    }
    // the same two steps for a list's tile: the slots are the entries themselves, and a row without one (slot -1) is zeros
    __device__ __forceinline__ void lookup(const MlaListKeys& keys, int k0, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) slot[j] = keys.slot(k0 + (tid >> 3) + 32 * j);
    }
    __device__ __forceinline__ void load(const MlaParams& p, int tid) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const char* row = p.kv + slot[j] * (kMlaQK * EB) + (tid & 7) * (8 * EB);
#pragma unroll
            for (int i = 0; i < kMlaN; ++i) d[j][i] = slot[j] >= 0 ? *reinterpret_cast<const Raw*>(row + 64 * EB * i) : Raw{};
        }
    }
    __device__ __forceinline__ void store(char* img, int tid) const {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < kMlaN; ++i) {
                u32x4_t x;
                if constexpr (kFp8) x = cvt8<T>(d[j][i]); else x = d[j][i];
                *reinterpret_cast<u32x4_t*>(img + ((tid >> 3) + 32 * j) * kMlaPitch + (tid & 7) * 16 + 128 * i) = x;
            }
    }
};

// The attention kernel's body, one for both cache kinds (KV: Kv16 / KvFp8 of fa_paged_tile.h) and both key sources (kList: the sparse
// call's list instead of a sequence's positions): the kinds differ in how a tile reaches the image (MlaTile) and in where the FP8
// scale enters, the sources in the block of rows, the key range, the cache row behind a key and the scores that count -- each a
// compile-time choice at its one place, so that the dense instances compile to what they were without the list.  kTree (the dense
// source only): the tree call -- the end of the key range and the scores that count are MlaTreeKeys', again one compile-time choice
// each.  Ls: the latent image (kMlaLdsImage bytes), Xs: the partial scores (kMlaLdsScores bytes), both 16-byte aligned LDS of the
// calling kernel.
template <class T, class KV, bool kList = false, bool kTree = false>
__device__ __forceinline__ void mla_paged_body(const MlaParams& p, char* Ls, char* Xs) {

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rh = wave & 1, ch = wave >> 1;
    // work item: (split, rank, sequence), the sequences side by side (the sparse call: a token is a sequence of its own)
    const int bid = (int)blockIdx.x;
    const int b = bid % p.B, rest = bid / p.B;
    const int rank = rest % p.row_blocks, split = rest / p.row_blocks;

    const MlaBlock blk = mla_block<kList>(p, b, rank);
    if (blk.rows == 0) return;
    const int L = blk.L, n = blk.n, r0 = blk.r0, rows = blk.rows;

    // this lane's row (a lane past the end works on the block's last row and stores nothing)
    const int rl = rh * 32 + l31;
    const bool live = rl < rows;
    const int r = r0 + min(rl, rows - 1);
    const int tok = r / p.Hq, head = r - tok * p.Hq;
    const int pos = L - n + tok;

    // this split's keys of this block: whole tiles of the sequence's own length, cut at the block's last visible key (or whole
    // tiles of the token's list: `keys`).  A sequence with a tree is NOT cut at the block's last position: a node may see a new token
    // behind its own.
    static_assert(!(kList && kTree), "a tree is a rule over a sequence's positions");
    typename std::conditional<kList, MlaListKeys, MlaNoList>::type keys(p, b, split);
    typename std::conditional<kTree, MlaTreeKeys, MlaNoTree>::type tree(kTree ? p.tree_mask + (blk.s + tok) : nullptr, L, n, pos);
    const int tiles = (L + kMlaKeys - 1) / kMlaKeys;
    const int per = (tiles + p.nsplit - 1) / p.nsplit;
    const int kbeg = kList ? keys.kbeg : split * per * kMlaKeys;
    const int kend = kList ? keys.kend : min(min((split + 1) * per * kMlaKeys, L), kTree && tree.tree ? L : L - n + (r0 + rows - 1) / p.Hq + 1);
    const int ntiles = kend > kbeg ? (kend - kbeg + kMlaKeys - 1) / kMlaKeys : 0;
    const int* tab = p.table + (long long)b * p.max_blocks;

    // Q operand chunks of this lane's row, the wave's half of the reduction
    const char* qrow = p.q + (((long long)blk.s + tok) * p.q_stride + (long long)head * kMlaQK) * 2 + ch * (kMlaRB / 2);
    u32x4_t qf[kMlaG];
#pragma unroll
    for (int g = 0; g < kMlaG; ++g) qf[g] = *reinterpret_cast<const u32x4_t*>(qrow + 32 * g + 16 * hi);

    // An FP8 cache's one scale is never applied per element: it multiplies the score scale here and the accumulators on their way out
    // (vs below); both are 1.0f for a 16-bit cache, where the products are exact and the bits the same as without them.
    float c = p.c, vs = 1.0f;
    if constexpr (std::is_same<KV, KvFp8>::value) {
        vs = *p.kv_scale;
        c *= vs;
    }

    f32x16_t o[kMlaDT];
#pragma unroll
    for (int i = 0; i < kMlaDT; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    MlaTile<T, KV> kt;
    if constexpr (kList) {
        if (ntiles > 0) {
            kt.lookup(keys, kbeg, tid);
            kt.load(p, tid);
            kt.lookup(keys, kbeg + kMlaKeys, tid);
            keys.fetch_mask(kbeg, lane);
        }
    } else if (ntiles > 0) {
        kt.lookup(p, tab, kbeg, kend, tid);
        kt.load(p, kbeg, kend, tid);
        kt.lookup(p, tab, kbeg + kMlaKeys, kend, tid);
    }
    char* xmine = Xs + wave * 8192 + lane * 16;
    const char* xother = Xs + (wave ^ 2) * 8192 + lane * 16;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kMlaKeys;
        __syncthreads();   // every wave is done with the previous tile and the previous partial scores
        kt.store(Ls, tid);
        __syncthreads();
        if constexpr (kList) {
            if (t + 1 < ntiles) {
                kt.load(p, tid);
                kt.lookup(keys, k0 + 2 * kMlaKeys, tid);
            }
        } else if (t + 1 < ntiles) {
            kt.load(p, k0 + kMlaKeys, kend, tid);
            kt.lookup(p, tab, k0 + 2 * kMlaKeys, kend, tid);
        }
        // partial S^T[key][row] over the wave's 288 elements
        f32x16_t sc[2] = {f32x16_t{}, f32x16_t{}};
        const char* kimg = Ls + l31 * kMlaPitch + ch * (kMlaRB / 2) + 16 * hi;
#pragma unroll
        for (int g = 0; g < kMlaG; ++g)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) sc[kk] = mfma16<T>(lds_b128(kimg + 32 * kk * kMlaPitch + 32 * g), qf[g], sc[kk]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                *reinterpret_cast<f32x4_t*>(xmine + (4 * kk + q4) * 1024) = f32x4_t{sc[kk][4 * q4], sc[kk][4 * q4 + 1], sc[kk][4 * q4 + 2], sc[kk][4 * q4 + 3]};
        __syncthreads();
        // own + other, scale to log2 units, mask, running max over the lane pair (lanes l and l + 32 hold the same row)
        if constexpr (kList) {
            keys.tile_mask(hi);                     // this tile's validity word, from the entries fetched a tile ago
            keys.fetch_mask(k0 + kMlaKeys, lane);   // ... and the next tile's entries
        }
        if constexpr (kTree) tree.tile_mask(k0, kend, hi);
        float mx = -__builtin_inff();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const f32x4_t y = *reinterpret_cast<const f32x4_t*>(xother + (4 * kk + q4) * 1024);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rr = 4 * q4 + i;
                    const int j = k0 + 32 * kk + crow(rr, hi);
                    const float x = (kList ? keys.visible(kk, rr) : kTree ? tree.visible(kk, rr) : j <= pos && j < kend) ? (sc[kk][rr] + y[i]) * c : -__builtin_inff();
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
        for (int i = 0; i < kMlaDT; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int rr = 0; rr < 16; ++rr) {
                const float ex = fast_exp2(sc[kk][rr] - mu);
                sc[kk][rr] = ex;
                l += ex;
            }
        // O^T[d][row] += V^T.P^T over the wave's 256 value columns, V = the image's first 512 columns
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const u32x4_t pb = pack_step<T>(sc[st >> 1], st & 1);
#pragma unroll
            for (int dt = 0; dt < kMlaDT; ++dt) o[dt] = mfma16<T>(lds_tr_step(Ls, kMlaPitch, 16 * st, 256 * ch + 32 * dt, lane), pb, o[dt]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    l += xhalf(l);
    if (!live) return;
    const long long orow = ((long long)blk.s + tok) * p.Hq + head;
    if (p.nsplit > 1) {
        const long long prow = (long long)split * p.rows_total + orow;
        float* po = p.part_o + prow * kMlaV + 256 * ch;
#pragma unroll
        for (int dt = 0; dt < kMlaDT; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<f32x4_t*>(po + 32 * dt + 8 * g4 + 4 * hi) =
                    f32x4_t{o[dt][4 * g4] * vs, o[dt][4 * g4 + 1] * vs, o[dt][4 * g4 + 2] * vs, o[dt][4 * g4 + 3] * vs};
        if (ch == 0 && hi == 0) *reinterpret_cast<f32x2_t*>(p.part_ml + prow * 2) = f32x2_t{m, l};
        return;
    }
    const float inv = (l > 0.f ? 1.f / l : 0.f) * vs;
    char* og = p.o + (orow * kMlaV + 256 * ch) * 2;
#pragma unroll
    for (int dt = 0; dt < kMlaDT; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && ch == 0 && hi == 0) {
        const float mu = m == -__builtin_inff() ? 0.f : m;
        p.lse[orow] = l > 0.f ? (mu + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

}  // namespace
}  // namespace aule_hip
