// fa_mla_indexer_gfx950.hip -- the indexer of the sparse MLA (DeepSeek-V3.2 "DSA"): the index logits of every query token over a paged
// cache of index keys, and the per-token top-k key lists that aule_attention_mla_sparse_ex consumes (the contracts are
// aule_mla_indexer_logits_desc and aule_mla_indexer_topk_desc in include/aule.h).
//
//   I[t, s] = sum_h w[t, h] * relu(q[t, h, :] . k[s, :])        q [T, H <= 64, 128] 16-bit, w [T, H] fp32, k one row per position
//
// LOGITS.  v_mfma_f32_32x32x16 with the HEADS as rows (A operand: q, 32 heads per accumulator, two accumulators for H > 32) and the
// KEYS as columns (B operand: 32 keys per tile).  A lane then holds, for ONE key (column lane & 31), the scores of 16 (or 32) heads in
// its accumulator registers: relu, the weight and the head sum are in-lane fused multiply-adds over those registers in a fixed order,
// and the two lane halves (heads crow(r, 0) and crow(r, 1)) meet in one cross-lane add.  Nothing per head goes through LDS or memory.
// A row past H is a row of zeros with weight 0.  An FP8 cache is converted exactly (cvt8) to q's type on its way to the operand; its
// per-row scale multiplies the finished sum (relu commutes with a positive factor), so with every scale 1 the bits are the 16-bit call's.
//
// Work item (sequence b, group of kIdxGroup = 4 tokens, chunk of chunk_keys keys): every logits column of every owned row belongs to
// exactly one item, which writes the logit where the key is visible (j <= p) and -inf elsewhere: no workspace, no combine, no atomics.
//   * a group with SEVERAL live tokens: wave w owns token w, its Q operand stays in registers; the K tile (64 keys) is staged ONCE in
//     LDS for the four waves, its rows fetched into registers a tile ahead.  Keys past the group's last visible one are not read.
//   * a group with ONE live token (decode, or the odd last token): the four waves share the token and take DIFFERENT 32-key tiles of
//     the chunk, each lane reading its key's row straight from the cache as the B operand (no LDS, no barrier).
// The grid is fixed on the host from (B, max_seqlen_q, W, CUs): mla_indexer_plan() below, which the launch and the debug hook read.
//
// TOP-K.  One workgroup of 1024 threads per token row.  Visible keys are positions 0 .. p (position arithmetic, not -inf marks).
// Order: logit descending by VALUE (-0 = +0, NaN = -inf), then position ascending; the first k = min(topk, p + 1) are emitted in
// ascending position order, the tail is -1.  p + 1 <= topk: every visible key, no logit is read.  Else a radix select over an
// order-preserving 32-bit key, 4 passes of 8 bits with a 256-bin LDS histogram, finds the k-th largest key and how many keys equal to
// it are taken (the first ones by position); one ordered pass then compacts.  In every pass a thread takes runs of 8 consecutive
// positions (two 16-byte loads) and the workgroup 8192 positions per step; the compaction counts a run, scans the counts over the wave,
// passes the waves' totals through LDS (one barrier per step) and places every selected position at (selected before it) -- ascending
// without a sort, no global atomics, the same bits on every run.
#include <type_traits>

#include "fa_kernels.h"
#include "kv_quant.h"

namespace aule_hip {
namespace {

constexpr int kIdxD = 128;                 // index head width
constexpr int kIdxRB = kIdxD * 2;          // bytes of a 16-bit row
constexpr int kIdxG = kIdxD / 16;          // k-steps of the 32x32x16 MFMA
constexpr int kIdxGroup = 4;               // tokens per work item: one per wave
constexpr int kIdxSub = 32;                // keys per MFMA tile
constexpr int kIdxTile = 64;               // keys per staged LDS tile
constexpr int kIdxPitch = kIdxRB + 16;     // LDS pitch: ds_read_b128 rows shift by one 16-byte slot
constexpr int kIdxUnit = 128;              // chunk_keys is a multiple of this: one 32-key tile per wave in the one-token path
constexpr int kTopkThreads = 1024;
constexpr int kTopkWaves = kTopkThreads / 64;
constexpr int kTopkRun = 8;                            // consecutive positions per thread and step
constexpr int kTopkStep = kTopkThreads * kTopkRun;     // positions per step of the workgroup

struct IdxParams {
    const char* q;
    const float* w;
    const char* k;
    const float* ks;     // FP8 cache: [num_blocks * block_size] fp32; else null
    const int* table;
    const int* ctx;
    const int* cu;       // null: sequence b owns row b
    float* out;
    long long q_stride, out_stride;
    int T, B, H;
    int nb, bs, bs_shift;
    int max_blocks, max_sq;
    int W;               // max_blocks * bs
    int groups, chunks, chunk_keys;
};

struct TopkParams {
    const float* logits;
    int* out;
    const int* table;
    const int* ctx;
    const int* cu;
    long long stride;
    int T, B, topk;
    int bs, bs_shift;
    int max_blocks, max_sq;
    int W;
    int positions;       // 1: raw positions, 0: slots through the table
};

// the cache row of position j of the sequence whose table row is `tab` (j < L_b: the entry is one of the used blocks); the entry is
// clamped into the cache, so a stale table cannot send a load outside it
__device__ __forceinline__ long long cache_row(const IdxParams& p, const int* tab, int j) {
    const int lb = block_of(j, p.bs, p.bs_shift);
    const unsigned blk = min((unsigned)tab[lb], (unsigned)(p.nb - 1));
    return (long long)blk * p.bs + (j - lb * p.bs);
}

// A token's operands: q chunks of head (lane & 31) + 32 hb at byte column 32 g + 16 hi, and the weights of the heads whose scores this
// lane's accumulator registers hold.  Heads at or past H: zeros, never read.
struct IdxToken {
    u32x4_t qf[2][kIdxG];
    float w[2][16];
    __device__ __forceinline__ void load(const IdxParams& p, long long row, int l31, int hi) {
        const char* qrow = p.q + row * p.q_stride * 2;
        const float* wrow = p.w + row * p.H;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int head = l31 + 32 * hb;
#pragma unroll
            for (int g = 0; g < kIdxG; ++g)
                qf[hb][g] = head < p.H ? *reinterpret_cast<const u32x4_t*>(qrow + head * kIdxRB + 32 * g + 16 * hi) : u32x4_t{};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int h = crow(r, hi) + 32 * hb;
                w[hb][r] = h < p.H ? wrow[h] : 0.f;
            }
        }
    }
};

// 32 keys (B operand chunks kf: key lane & 31, byte column 32 g + 16 hi) against the token: the weighted, rectified head sum of this
// lane's key, the same value in both lane halves.  One fixed order of operations for every cache kind.
template <class T>
__device__ __forceinline__ float head_sum(const IdxToken& t, const u32x4_t (&kf)[kIdxG], bool two) {
    f32x16_t a = {};
#pragma unroll
    for (int g = 0; g < kIdxG; ++g) a = T::mfma(as_v8<T>(t.qf[0][g]), as_v8<T>(kf[g]), a);
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = __builtin_fmaf(fmaxf(a[r], 0.f), t.w[0][r], s);
    if (two) {
        f32x16_t c = {};
#pragma unroll
        for (int g = 0; g < kIdxG; ++g) c = T::mfma(as_v8<T>(t.qf[1][g]), as_v8<T>(kf[g]), c);
#pragma unroll
        for (int r = 0; r < 16; ++r) s = __builtin_fmaf(fmaxf(c[r], 0.f), t.w[1][r], s);
    }
    return s + xhalf(s);
}

template <class T, bool FP8>
__global__ void __launch_bounds__(256) fa_mla_indexer_logits_kernel(const IdxParams p) {
    using Raw = typename std::conditional<FP8, u32x2_t, u32x4_t>::type;
    constexpr int EB = FP8 ? 1 : 2;
    __shared__ __attribute__((aligned(16))) char Ks[kIdxTile * kIdxPitch];
    __shared__ float Ss[kIdxTile];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = (int)blockIdx.x;
    const int chunk = bid % p.chunks, rest = bid / p.chunks;
    const int grp = rest % p.groups, b = rest / p.groups;

    // aule_mla_paged_desc's clamps (fa_device.h): L_b, s_b, n_b
    const int L = seq_len(p.ctx, b, p.W);
    const SeqRange own_rows = seq_range_or_row(p.cu, b, p.T, p.max_sq);   // (a null cu: b < T, the host checks)
    const int s = own_rows.s, n = own_rows.n;
    const int i0 = grp * kIdxGroup;
    const int live = min(kIdxGroup, n - i0);
    if (live <= 0) return;
    const int kbeg = chunk * p.chunk_keys;
    const int kstop = min(kbeg + p.chunk_keys, p.W);                 // columns this item writes
    const int kend = min(kstop, L - n + i0 + live);                  // keys this item reads: up to its last token's position
    const int* tab = p.table + (long long)b * p.max_blocks;
    const bool two = p.H > 32;
    const float ninf = -__builtin_inff();

    if (live == 1) {
        // one token, the waves on different tiles, the B operand straight from the cache
        const int pos = L - n + i0;
        float* orow = p.out + (long long)(s + i0) * p.out_stride;
        IdxToken tk;
        if (kbeg < kend) tk.load(p, s + i0, l31, hi);
        for (int j0 = kbeg + kIdxSub * wave; j0 < kstop; j0 += kIdxSub * 4) {
            const int j = j0 + l31;
            float v = ninf;
            if (j0 < kend) {
                const bool vis = j <= pos;
                const long long at = vis ? cache_row(p, tab, j) : 0;
                u32x4_t kf[kIdxG];
#pragma unroll
                for (int g = 0; g < kIdxG; ++g) {
                    const Raw x = vis ? *reinterpret_cast<const Raw*>(p.k + at * (kIdxD * EB) + (2 * g + hi) * (8 * EB)) : Raw{};
                    if constexpr (FP8) kf[g] = cvt8<T>(x); else kf[g] = x;
                }
                const float sum = head_sum<T>(tk, kf, two);
                if (vis) {
                    v = sum;
                    if constexpr (FP8) v *= p.ks[at];
                }
            }
            if (hi == 0 && j < kstop) orow[j] = v;
        }
        return;
    }

    // several tokens: wave w owns token i0 + w, the K tile staged once for all of them
    const bool alive = wave < live;
    const int pos = L - n + i0 + wave;
    float* orow = p.out + (long long)(s + i0 + min(wave, live - 1)) * p.out_stride;
    IdxToken tk;
    if (alive && kbeg <= pos) tk.load(p, s + i0 + wave, l31, hi);

    // thread t stages 16-byte chunks (t & 3) + 4 i of tile row t >> 2
    const int srow = tid >> 2, sc0 = tid & 3;
    Raw d[4];
    float dscale = 0.f;
    auto fetch = [&](int k0) {
        const int j = k0 + srow;
        const bool ok = j < kend;
        const long long at = ok ? cache_row(p, tab, j) : 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = ok ? *reinterpret_cast<const Raw*>(p.k + at * (kIdxD * EB) + (sc0 + 4 * i) * (8 * EB)) : Raw{};
        if constexpr (FP8) dscale = ok && sc0 == 0 ? p.ks[at] : 0.f;
    };
    if (kbeg < kend) fetch(kbeg);
    for (int k0 = kbeg; k0 < kstop; k0 += kIdxTile) {
        if (k0 < kend) {   // (uniform over the workgroup)
            __syncthreads();   // every wave is done with the previous tile
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u32x4_t x;
                if constexpr (FP8) x = cvt8<T>(d[i]); else x = d[i];
                *reinterpret_cast<u32x4_t*>(Ks + srow * kIdxPitch + (sc0 + 4 * i) * 16) = x;
            }
            if constexpr (FP8) {
                if (sc0 == 0) Ss[srow] = dscale;
            }
            __syncthreads();
            if (k0 + kIdxTile < kend) fetch(k0 + kIdxTile);
        }
        if (!alive) continue;
#pragma unroll
        for (int kk = 0; kk < kIdxTile / kIdxSub; ++kk) {
            const int j0 = k0 + kIdxSub * kk, j = j0 + l31;
            if (j0 >= kstop) break;
            float v = ninf;
            if (j0 <= pos) {   // (uniform over the wave; j0 <= pos < kend: the tile is staged)
                u32x4_t kf[kIdxG];
                const char* krow = Ks + (kIdxSub * kk + l31) * kIdxPitch + 16 * hi;
#pragma unroll
                for (int g = 0; g < kIdxG; ++g) kf[g] = *reinterpret_cast<const u32x4_t*>(krow + 32 * g);
                const float sum = head_sum<T>(tk, kf, two);
                if (j <= pos) {
                    v = sum;
                    if constexpr (FP8) v *= Ss[kIdxSub * kk + l31];
                }
            }
            if (hi == 0 && j < kstop) orow[j] = v;
        }
    }
}

// larger logit -> larger key; -0 = +0, NaN = -inf; every key is > 0
__device__ __forceinline__ unsigned order_key(float x) {
    unsigned u = __builtin_bit_cast(unsigned, x);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// positions j0 .. j0 + 7 of a row (j0 a multiple of 8) as order keys, 0 -- below every key -- at or past V; wide: the row is 16-byte
// aligned, so a whole run is two 16-byte loads
__device__ __forceinline__ void load_keys(const float* lg, int j0, int V, bool wide, unsigned (&key)[kTopkRun]) {
    if (wide && j0 + kTopkRun <= V) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(lg + j0), b = *reinterpret_cast<const f32x4_t*>(lg + j0 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            key[e] = order_key(a[e]);
            key[4 + e] = order_key(b[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < kTopkRun; ++e) key[e] = j0 + e < V ? order_key(lg[j0 + e]) : 0u;
    }
}

__global__ void __launch_bounds__(kTopkThreads) fa_mla_indexer_topk_kernel(const TopkParams p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[4];
    __shared__ unsigned pick[2];               // the chosen bin, and what is still to take inside it
    __shared__ unsigned cnt[2][kTopkWaves];    // per wave and step: keys above the threshold | keys equal to it << 16

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x / p.max_sq, i = (int)blockIdx.x % p.max_sq;
    // aule_mla_paged_desc's clamps (fa_device.h): L_b, s_b, n_b
    const int L = seq_len(p.ctx, b, p.W);
    const SeqRange own_rows = seq_range_or_row(p.cu, b, p.T, p.max_sq);   // (a null cu: b < T, the host checks)
    const int s = own_rows.s, n = own_rows.n;
    if (i >= n) return;
    int* out = p.out + (long long)(s + i) * p.topk;
    const int V = L - n + i + 1;   // visible keys: positions 0 .. V - 1
    const int k = max(min(p.topk, V), 0);
    for (int at = k + tid; at < p.topk; at += kTopkThreads) out[at] = -1;
    if (k == 0) return;
    const float* lg = p.logits + (long long)(s + i) * p.stride;
    const int* tab = p.table + (long long)b * p.max_blocks;
    const bool all = V <= p.topk;   // every visible key: no logit is read
    const bool wide = (reinterpret_cast<uintptr_t>(lg) & 15) == 0;
    // a thread takes runs of kTopkRun consecutive positions, the workgroup kTopkStep positions per step
    const int mine0 = tid * kTopkRun;

    unsigned thr = 0, need_eq = 0;
    if (!all) {
        unsigned prefix = 0, mask = 0, rem = (unsigned)k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int base = 0; base < V; base += kTopkStep) {
                unsigned key[kTopkRun];
                load_keys(lg, base + mine0, V, wide, key);
#pragma unroll
                for (int e = 0; e < kTopkRun; ++e) {
                    bool act = key[e] != 0u && (key[e] & mask) == prefix;
                    const unsigned digit = (key[e] >> shift) & 255u;
                    if (shift == 24) {
                        // sign and high exponent bits of real logits crowd into a few bins: the wave's two most common digits are
                        // counted by one lane each (the later digits spread, and few keys still match the prefix)
#pragma unroll
                        for (int it = 0; it < 2; ++it) {
                            const unsigned long long m = __builtin_amdgcn_ballot_w64(act);
                            if (m == 0) break;
                            const int leader = __builtin_ctzll(m);
                            const unsigned dl = (unsigned)__shfl((int)digit, leader, 64);
                            const unsigned long long same = __builtin_amdgcn_ballot_w64(act && digit == dl);
                            if (lane == leader) atomicAdd(&hist[dl], (unsigned)__builtin_popcountll(same));
                            act = act && digit != dl;
                        }
                    }
                    if (act) atomicAdd(&hist[digit], 1u);
                }
            }
            __syncthreads();
            // thread t < 256 holds bin 255 - t: an inclusive scan from the largest digit down finds the bin of the rem-th largest key
            unsigned c = 0, x = 0;
            if (tid < 256) {
                c = hist[255 - tid];
                x = c;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned y = (unsigned)__shfl_up((int)x, o, 64);
                    if (lane >= o) x += y;
                }
                if (lane == 63) wsum[wave] = x;
            }
            __syncthreads();
            if (tid < 256) {
                unsigned before = 0;
                for (int w = 0; w < wave; ++w) before += wsum[w];
                const unsigned incl = x + before, excl = incl - c;
                if (excl < rem && rem <= incl) {
                    pick[0] = 255u - (unsigned)tid;
                    pick[1] = rem - excl;
                }
            }
            __syncthreads();
            prefix |= pick[0] << shift;
            mask |= 255u << shift;
            rem = pick[1];
        }
        thr = prefix;   // (> 0: every key is)
        need_eq = rem;
    }

    // ordered compaction: position j lands at (keys above the threshold before it) + min(keys equal to it before it, need_eq).  Per
    // step: a thread counts its run, an inclusive scan over the wave, the waves' totals through LDS (the next step writes the other
    // half of cnt: one barrier per step), then the thread places its run in order.
    unsigned gt_run = 0, eq_run = 0;
    for (int base = 0, it = 0; base < V; base += kTopkStep, ++it) {
        const int j0 = base + mine0;
        unsigned key[kTopkRun];
        if (all) {
#pragma unroll
            for (int e = 0; e < kTopkRun; ++e) key[e] = j0 + e < V ? 0xffffffffu : 0u;   // (thr = 0: every position counts as above)
        } else {
            load_keys(lg, j0, V, wide, key);
        }
        // two bits per position of the run -- 1: above the threshold, 2: equal to it -- so that no compare mask outlives its use
        unsigned kinds = 0;
#pragma unroll
        for (int e = 0; e < kTopkRun; ++e) kinds |= (key[e] > thr ? 1u : (key[e] == thr && key[e] != 0u ? 2u : 0u)) << (2 * e);
        const unsigned own = (unsigned)__builtin_popcount(kinds & 0x5555u) | (unsigned)__builtin_popcount(kinds & 0xaaaau) << 16;
        unsigned x = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = (unsigned)__shfl_up((int)x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) cnt[it & 1][wave] = x;   // (at most kTopkStep of either kind per step: both halves fit 16 bits)
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kTopkWaves; ++w) {
            const unsigned c = cnt[it & 1][w];
            total += c;
            if (w < wave) before += c;
        }
        const unsigned excl = before + x - own;
        unsigned g = gt_run + (excl & 0xffffu), q = eq_run + (excl >> 16);
#pragma unroll
        for (int e = 0; e < kTopkRun; ++e) {
            const unsigned kind = (kinds >> (2 * e)) & 3u;
            const bool gt = kind == 1u, eq = kind == 2u;
            if (gt || (eq && q < need_eq)) {
                const unsigned at = g + min(q, need_eq);
                const int j = j0 + e;
                int v = j;
                if (!p.positions) {
                    const int lb = block_of(j, p.bs, p.bs_shift);
                    v = (int)((unsigned)tab[lb] * (unsigned)p.bs + (unsigned)(j - lb * p.bs));
                }
                if (at < (unsigned)k) out[at] = v;
            }
            g += kind & 1u;
            q += kind >> 1;
        }
        gt_run += total & 0xffffu;
        eq_run += total >> 16;
        if (gt_run + min(eq_run, need_eq) >= (unsigned)k) break;   // (uniform: the list is complete)
    }
}

}  // namespace

MlaIndexerPlan mla_indexer_plan(int B, int max_seqlen_q, long long W, int device) {
    MlaIndexerPlan plan;
    if (B <= 0 || max_seqlen_q <= 0 || W <= 0) return plan;
    const long long groups = ((long long)max_seqlen_q + kIdxGroup - 1) / kIdxGroup;
    const long long units = (W + kIdxUnit - 1) / kIdxUnit;
    const long long base = (long long)B * groups;
    const long long target = 4ll * device_cu_count(device);   // a few workgroups per compute unit
    long long chunks = (target + base - 1) / base;
    if (chunks > units) chunks = units;
    if (chunks < 1) chunks = 1;
    const long long per = (units + chunks - 1) / chunks;
    chunks = (units + per - 1) / per;
    plan.group_tokens = kIdxGroup;
    plan.token_groups = (int)groups;
    plan.chunk_keys = (int)(per * kIdxUnit);
    plan.key_chunks = (int)chunks;
    plan.grid = base * chunks;
    return plan;
}

int launch_mla_indexer_logits(const MlaIndexerArgs& a, const MlaIndexerPlan& plan, hipStream_t stream) {
    if (plan.grid <= 0 || plan.grid > 0x7fffffffll) return -1;
    if (a.H < 1 || a.H > kMlaIndexerMaxHeads || a.block_size < 1 || a.max_blocks < 1 || a.num_blocks < 1) return -1;
    const long long W = (long long)a.max_blocks * a.block_size;
    if (W >= (1ll << 30) || a.logits_stride < W) return -1;
    if (a.q_token_stride < (long long)a.H * kIdxD || a.q_token_stride % 8 != 0) return -1;
    if (a.cu_seqlens_q == nullptr && a.T < a.B) return -1;
    const bool fp8 = a.cache_kind == kCacheFp8E4M3;
    if (fp8 ? a.k_scale == nullptr : a.cache_kind != kCache16) return -1;
    IdxParams p;
    p.q = static_cast<const char*>(a.q); p.w = a.weights; p.k = static_cast<const char*>(a.k_cache);
    p.ks = fp8 ? a.k_scale : nullptr;
    p.table = a.block_tables; p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.out = a.logits;
    p.q_stride = a.q_token_stride; p.out_stride = a.logits_stride;
    p.T = a.T; p.B = a.B; p.H = a.H;
    p.nb = a.num_blocks; p.bs = a.block_size; p.bs_shift = shift_of(a.block_size);
    p.max_blocks = a.max_blocks; p.max_sq = a.max_seqlen_q;
    p.W = (int)W;
    p.groups = plan.token_groups; p.chunks = plan.key_chunks; p.chunk_keys = plan.chunk_keys;
    return dispatch_16bit(a.dtype, [&](auto t) {
        if (fp8) hipLaunchKernelGGL((fa_mla_indexer_logits_kernel<decltype(t), true>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((fa_mla_indexer_logits_kernel<decltype(t), false>), dim3((unsigned)plan.grid), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

int launch_mla_indexer_topk(const MlaIndexerTopkArgs& a, hipStream_t stream) {
    const long long grid = (long long)a.B * a.max_seqlen_q;
    if (grid <= 0 || grid > 0x7fffffffll) return -1;
    if (a.topk < 1 || a.topk > kMlaIndexerMaxTopk || a.block_size < 1 || a.max_blocks < 1) return -1;
    const long long W = (long long)a.max_blocks * a.block_size;
    if (W >= (1ll << 30) || a.logits_stride < W) return -1;
    if (a.cu_seqlens_q == nullptr && a.T < a.B) return -1;
    TopkParams p;
    p.logits = a.logits; p.out = a.indices;
    p.table = a.block_tables; p.ctx = a.context_lens; p.cu = a.cu_seqlens_q;
    p.stride = a.logits_stride;
    p.T = a.T; p.B = a.B; p.topk = a.topk;
    p.bs = a.block_size; p.bs_shift = shift_of(a.block_size);
    p.max_blocks = a.max_blocks; p.max_sq = a.max_seqlen_q;
    p.W = (int)W;
    p.positions = a.positions ? 1 : 0;
    hipLaunchKernelGGL(fa_mla_indexer_topk_kernel, dim3((unsigned)grid), dim3(kTopkThreads), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace aule_hip
