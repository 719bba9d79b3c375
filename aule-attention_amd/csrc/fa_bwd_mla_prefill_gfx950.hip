// fa_bwd_mla_prefill_gfx950.hip -- backward of the MLA 192 / 128 attention over a variable-length packed batch.
//
// The tensors, the clamps of cu_seqlens_q / cu_seqlens_k and the visibility rule are those of fa_fwd_mla_prefill_gfx950.hip:
//     q [Tq, H, 192]   k_nope, v [Tk, H, 128] with token AND head strides   k_pe [Tk, 64] with its token stride
//     out, dout [Tq, H, 128], lse [Tq, H], dq [Tq, H, 192], dk_pe [Tk, 64] contiguous   dk_nope, dv [Tk, H, 128] with token AND head strides
// The trio of fa_bwd_varlen_gfx950.hip in the shape of fa_mla_prefill_common.h -- a 192-wide key, a 128-wide value and one k_pe per
// token -- with the same dQ body and row store (fa_varlen_common.h, fa_tile_attention.h); three or four launches:
//   delta     delta = rowsum(dO * O) in fp32 over 128 columns, one wave per (token, head) row, all Tq rows (workspace: [Tq, H] fp32)
//   dQ        ragged_dq_body, the forward's decomposition: workgroup = (rank, sequence, head), 4 waves x 32 rows, Q (12 chunk pairs) and dO (8) of the
//             lane's row in registers; K tiles of 64 keys assembled in LDS from k_nope (columns 0 .. 127) and k_pe (128 .. 191) at pitch
//             464 (29 sixteen-byte slots: read as ds_read_b128 rows AND transposed), V tiles at pitch 272; S^T = K.Q^T over 192,
//             dP^T = V.dO^T over 128, dS^T = P^T (dP^T - delta) with P = exp2(S c - L log2 e) on visible keys only,
//             dQ^T[d][q] += K^T.dS^T over all 192 columns.  dq = scale * acc.
//   dK / dV   workgroup = (128 keys, sequence, head chunk), 4 waves x 32 keys.  The k_pe fragment of the lane's key (4 chunk pairs) and a
//             64-column fp32 dk_pe accumulator stay in registers across the heads of the chunk; per head the k_nope and v fragments
//             are reloaded and the sequence's tokens are walked TWICE (32-row tiles of Q and dO through LDS with lse log2 e and delta;
//             the range cut to the tokens that can see the block, a wave skipping tiles that see none of its keys; the next tile --
//             of the next pass or head at a walk's end -- prefetched into registers): pass 1 accumulates dk_nope (and dk_pe) from
//             dS = P (dP - delta) and writes dk_nope, pass 2 recomputes S and P and accumulates and writes dv.  One pass would hold
//             160 accumulators beside 80 operand registers and needed scratch (43 spilled VGPRs); the column passes are the remedy of
//             fa_bwd_d256_gfx950.hip, at the price of 12 more MFMAs per tile (52 against 40).  With one chunk dk_pe is written from
//             here; with more, chunk c writes its fp32 partial to plane c of [n_chunks, Tk, 64] and
//   reduce    workgroup = (128 keys, sequence) sums the planes in chunk order and writes the 16-bit dk_pe.  No atomics anywhere: two
//             runs of one call agree bit for bit.
// Every owned row of dq, dk_nope, dv and dk_pe is written (zeros where nothing is seen, n = 0 included); rows of no sequence never.
#include "fa_kernels.h"
#include "fa_mla_prefill_common.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

constexpr int kPQK = VarlenCfg<kDQK>::PAT;   // 464: 192-wide rows read both as b128 operands and transposed
constexpr int kPVT = VarlenCfg<kDV>::PAT;    // 336: 128-wide rows read both ways
constexpr int kPVA = PrefillCfg<kDV>::PA;    // 272: 128-wide rows read as b128 operands only
static_assert(kPQK == 464 && (kPQK / 16) % 2 == 1 && kPVT == 336 && kPVA == 272, "the LDS budget of DESIGN.md 3.11");

struct MlaBwdParams {
    const char* q;
    const char* k_nope;
    const char* k_pe;
    const char* v;
    const char* o;
    const char* dout;
    const float* lse;
    float* delta;
    char* dq;
    char* dkn;
    char* dkp;
    char* dv;
    float* part;                         // [nchunks, Tk, 64] fp32 (nchunks > 1)
    const int* cu_q;
    const int* cu_k;
    long long q_stride;                  // elements between tokens
    long long kn_stride, kn_hstride;     // elements between tokens / heads of k_nope
    long long v_stride, v_hstride;
    long long kp_stride;
    long long dkn_stride, dkn_hstride;   // ... of dk_nope
    long long dv_stride, dv_hstride;
    int Tq, Tk, B, H;
    int max_sq, max_sk;
    int hpc, nchunks;                    // heads per chunk, chunks (the plan)
    float c;        // scale * log2(e)
    float scale;
    int causal;     // 0, 1, 2
    // what query_block reads beside the above: MHA, no window
    static constexpr int g = 1;
    static constexpr int window = 0;
};

// one wave per (token, head) row of the contiguous out / dout (the arithmetic of the variable-length backward's delta kernel at D = 128)
template <class T>
__global__ void __launch_bounds__(256) fa_bwd_mla_delta_kernel(const MlaBwdParams p, long long rows) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float acc = 0.f;
    if (lane < kDV / 8) {
        const u32x4_t x = *reinterpret_cast<const u32x4_t*>(p.o + row * (kDV * 2) + 16 * lane);
        const u32x4_t y = *reinterpret_cast<const u32x4_t*>(p.dout + row * (kDV * 2) + 16 * lane);
#pragma unroll
        for (int w = 0; w < 4; ++w) acc += T::lo(x[w]) * T::lo(y[w]) + T::hi(x[w]) * T::hi(y[w]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) p.delta[row] = acc;
}

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_mla_dq_kernel(const MlaBwdParams p) {
    __shared__ __attribute__((aligned(16))) char Ks[kPK * kPQK];
    __shared__ __attribute__((aligned(16))) char Vs[kPK * kPVA];
    ragged_dq_body<T, MlaShape>(p, Ks, Vs);
}

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_mla_dkdv_kernel(const MlaBwdParams p) {
    constexpr int GN = kDN / 16, GR = kDR / 16, GV = kDV / 16;   // 8, 4, 8 operand chunk pairs
    constexpr int TN = kDN / 32, TR = kDR / 32, TV = kDV / 32;   // 4, 2, 4 accumulators
    __shared__ __attribute__((aligned(16))) char Qs[kVQT * kPQK];
    __shared__ __attribute__((aligned(16))) char Os[kVQT * kPVT];
    __shared__ float Ls[kVQT], Dl[kVQT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> (key block, sequence, head chunk): key block 0 first (under the top-left rule it sees the most queries)
    const int bid = (int)blockIdx.x;
    const int units = p.nchunks * p.B;
    const int kb = bid / units, unit = bid - kb * units;
    const int chunk = unit % p.nchunks, b = unit / p.nchunks;
    const int h0 = chunk * p.hpc, h1 = min(h0 + p.hpc, p.H);

    const SeqRange sk = seq_range(p.cu_k, b, p.Tk, p.max_sk);
    const int L = sk.n;
    const int k0 = kb * kVKB;
    if (k0 >= L) return;
    const SeqRange sq = seq_range(p.cu_q, b, p.Tq, p.max_sq);
    const int n = sq.n;
    const bool causal = p.causal != 0;
    const int coff = p.causal == 2 ? L - n : 0;

    // this lane's key (a lane past the end works on the sequence's last key and stores nothing)
    const int kj = k0 + wave * 32 + l31;
    const bool live = kj < L;
    const int kjc = min(kj, L - 1);
    const int wkey_lo = k0 + wave * 32;   // (wave-uniform)

    // tokens that see any key of the block
    const int tbeg = causal ? min(n, max(0, k0 - coff)) : 0;
    const int rbeg = tbeg / kVQT * kVQT;
    const int rend = n;
    const int ntiles = rend > rbeg ? (rend - rbeg + kVQT - 1) / kVQT : 0;

    // the shared k_pe fragment of this lane's key, and its gradient over the heads of the chunk
    const char* kprow = p.k_pe + ((long long)sk.s + kjc) * p.kp_stride * 2;
    u32x4_t kpf[GR];
#pragma unroll
    for (int g = 0; g < GR; ++g) kpf[g] = *reinterpret_cast<const u32x4_t*>(kprow + 32 * g + 16 * hi);
    f32x16_t dkp[TR];
#pragma unroll
    for (int i = 0; i < TR; ++i) dkp[i] = f32x16_t{};

    RowTile<kDQK, kVQT> qt;   // 3 chunks per thread
    RowTile<kDV, kVQT> ot;    // 2
    float pl = 0.f, pd = 0.f;   // threads 0 .. 31: lse log2 e and delta of row tid of the tile in flight
    const auto load_tile = [&](int h, int t0) {
        qt.load([&](int row) -> const char* {
            const int rr = t0 + row;
            if (rr >= rend) return nullptr;
            return p.q + (((long long)sq.s + rr) * p.q_stride + (long long)h * kDQK) * 2;
        }, tid);
        ot.load([&](int row) -> const char* {
            const int rr = t0 + row;
            if (rr >= rend) return nullptr;
            return p.dout + (((long long)sq.s + rr) * p.H + h) * (long long)(kDV * 2);
        }, tid);
        if (tid < kVQT) {
            const int rr = t0 + tid;
            pl = 0.f;
            pd = 0.f;
            if (rr < rend) {
                const long long at = ((long long)sq.s + rr) * p.H + h;
                pl = p.lse[at] * kLog2e;
                pd = p.delta[at];
            }
        }
    };
    // the tile in flight becomes the tile in LDS
    const auto stage = [&]() {
        __syncthreads();
        qt.store(Qs, kPQK, tid);
        ot.store(Os, kPVT, tid);
        if (tid < kVQT) {
            Ls[tid] = pl;
            Dl[tid] = pd;
        }
        __syncthreads();
    };
    // a wave skips the tiles whose rows see none of its keys: every position before its first key
    const auto skips = [&](int t0) { return wkey_lo >= L || (causal && coff + min(t0 + kVQT, rend) - 1 < wkey_lo); };
    // S[row][key] = Q.K^T over 192 from the tile in LDS
    const auto scores = [&](const u32x4_t (&knf)[GN]) {
        f32x16_t s = f32x16_t{};
#pragma unroll
        for (int g = 0; g < GN; ++g) s = mfma16<T>(lds_b128(Qs + l31 * kPQK + 32 * g + 16 * hi), knf[g], s);
#pragma unroll
        for (int g = 0; g < GR; ++g) s = mfma16<T>(lds_b128(Qs + l31 * kPQK + kDN * 2 + 32 * g + 16 * hi), kpf[g], s);
        return s;
    };
    // P[r] of row crow(r, hi) of the tile at t0: exp2(S c - L log2 e) on visible keys
    const auto prob = [&](float sc, int t0, int qr) {
        const int rr = t0 + qr;
        const bool vis = rr < rend && varlen_visible(coff + rr, kj, L, causal, 0);
        return vis ? fast_exp2(sc * p.c - Ls[qr]) : 0.f;
    };

    // Two passes over the sequence's tokens per head -- dk_nope and dk_pe, then dv -- so that 96 and 64 accumulators are live, not
    // 160 at once (one pass needs scratch: DESIGN.md 3.11); the second recomputes S and P.  The tiles form one prefetch chain.
    if (ntiles > 0) load_tile(h0, rbeg);
    for (int h = h0; h < h1; ++h) {
        const char* knrow = p.k_nope + (((long long)sk.s + kjc) * p.kn_stride + (long long)h * p.kn_hstride) * 2;
        u32x4_t knf[GN];
#pragma unroll
        for (int g = 0; g < GN; ++g) knf[g] = *reinterpret_cast<const u32x4_t*>(knrow + 32 * g + 16 * hi);
        {   // pass 1: dK^T[d][key] += Q^T.dS (128 nope columns of this head, 64 pe columns of the chunk)
            const char* vrow = p.v + (((long long)sk.s + kjc) * p.v_stride + (long long)h * p.v_hstride) * 2;
            u32x4_t vf[GV];
#pragma unroll
            for (int g = 0; g < GV; ++g) vf[g] = *reinterpret_cast<const u32x4_t*>(vrow + 32 * g + 16 * hi);
            f32x16_t dkn[TN];
#pragma unroll
            for (int i = 0; i < TN; ++i) dkn[i] = f32x16_t{};
            for (int t = 0; t < ntiles; ++t) {
                const int t0 = rbeg + t * kVQT;
                stage();
                load_tile(h, t + 1 < ntiles ? t0 + kVQT : rbeg);   // (the last tile is followed by the first one of pass 2)
                if (skips(t0)) continue;
                f32x16_t s = scores(knf), dp = f32x16_t{};
#pragma unroll
                for (int g = 0; g < GV; ++g) dp = mfma16<T>(lds_b128(Os + l31 * kPVT + 32 * g + 16 * hi), vf[g], dp);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qr = crow(r, hi);
                    s[r] = prob(s[r], t0, qr) * (dp[r] - Dl[qr]);   // dS
                }
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const u32x4_t db = pack_step<T>(s, st);
#pragma unroll
                    for (int dt = 0; dt < TN; ++dt) dkn[dt] = mfma16<T>(lds_tr_step(Qs, kPQK, 16 * st, 32 * dt, lane), db, dkn[dt]);
#pragma unroll
                    for (int dt = 0; dt < TR; ++dt) dkp[dt] = mfma16<T>(lds_tr_step(Qs, kPQK, 16 * st, kDN + 32 * dt, lane), db, dkp[dt]);
                }
            }
            if (live) store_row16<T, TN>(p.dkn + (((long long)sk.s + kj) * p.dkn_stride + (long long)h * p.dkn_hstride) * 2, dkn, p.scale, hi);
        }
        {   // pass 2: dV^T[d][key] += dO^T.P
            f32x16_t dv[TV];
#pragma unroll
            for (int i = 0; i < TV; ++i) dv[i] = f32x16_t{};
            for (int t = 0; t < ntiles; ++t) {
                const int t0 = rbeg + t * kVQT;
                stage();
                if (t + 1 < ntiles) load_tile(h, t0 + kVQT);
                else if (h + 1 < h1) load_tile(h + 1, rbeg);
                if (skips(t0)) continue;
                f32x16_t s = scores(knf);
#pragma unroll
                for (int r = 0; r < 16; ++r) s[r] = prob(s[r], t0, crow(r, hi));
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const u32x4_t pb = pack_step<T>(s, st);
#pragma unroll
                    for (int dt = 0; dt < TV; ++dt) dv[dt] = mfma16<T>(lds_tr_step(Os, kPVT, 16 * st, 32 * dt, lane), pb, dv[dt]);
                }
            }
            if (live) store_row16<T, TV>(p.dv + (((long long)sk.s + kj) * p.dv_stride + (long long)h * p.dv_hstride) * 2, dv, 1.f, hi);
        }
    }
    if (!live) return;
    // dk_pe of the chunk: the 16-bit result (one chunk) or this chunk's fp32 plane
    const long long krow_out = (long long)sk.s + kj;
#pragma unroll
    for (int dt = 0; dt < TR; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = dkp[dt][4 * g4] * p.scale, a1 = dkp[dt][4 * g4 + 1] * p.scale;
            const float a2 = dkp[dt][4 * g4 + 2] * p.scale, a3 = dkp[dt][4 * g4 + 3] * p.scale;
            if (p.nchunks == 1) *reinterpret_cast<u32x2_t*>(p.dkp + (krow_out * kDR + d) * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
            else *reinterpret_cast<f32x4_t*>(p.part + ((long long)chunk * p.Tk + krow_out) * kDR + d) = f32x4_t{a0, a1, a2, a3};
        }
}

// dk_pe = the chunks' planes summed in chunk order: workgroup = (128 keys, sequence), two threads per key, 32 columns each
template <class T>
__global__ void __launch_bounds__(256) fa_bwd_mla_dkpe_reduce_kernel(const MlaBwdParams p) {
    const int tid = threadIdx.x;
    const int bid = (int)blockIdx.x;
    const int kb = bid / p.B, b = bid - kb * p.B;
    const SeqRange sk = seq_range(p.cu_k, b, p.Tk, p.max_sk);
    const int kj = kb * kVKB + (tid >> 1);
    if (kj >= sk.n) return;
    const long long row = (long long)sk.s + kj;
    const int col = (tid & 1) * 32;
    f32x4_t acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x4_t{};
    for (int ch = 0; ch < p.nchunks; ++ch) {
        const f32x4_t* src = reinterpret_cast<const f32x4_t*>(p.part + ((long long)ch * p.Tk + row) * kDR + col);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += src[i];
    }
    char* dst = p.dkp + (row * kDR + col) * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<u32x4_t*>(dst + 16 * i) = u32x4_t{T::pack2(acc[2 * i][0], acc[2 * i][1]), T::pack2(acc[2 * i][2], acc[2 * i][3]),
                                                            T::pack2(acc[2 * i + 1][0], acc[2 * i + 1][1]), T::pack2(acc[2 * i + 1][2], acc[2 * i + 1][3])};
}

template <class T>
int launch_instance(const MlaBwdParams& p, const MlaPrefillBwdPlan& plan, hipStream_t stream) {
    if (plan.dq_grid > 0) {
        hipLaunchKernelGGL((fa_bwd_mla_delta_kernel<T>), dim3((unsigned)plan.delta_grid), dim3(256), 0, stream, p, (long long)p.Tq * p.H);
        hipLaunchKernelGGL((fa_bwd_mla_dq_kernel<T>), dim3((unsigned)plan.dq_grid), dim3(256), 0, stream, p);
    }
    if (plan.dkdv_grid > 0) hipLaunchKernelGGL((fa_bwd_mla_dkdv_kernel<T>), dim3((unsigned)plan.dkdv_grid), dim3(256), 0, stream, p);
    if (plan.reduce_grid > 0) hipLaunchKernelGGL((fa_bwd_mla_dkpe_reduce_kernel<T>), dim3((unsigned)plan.reduce_grid), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// The launch plan: one statement of the head chunks, the four grids and the workspace, read by the launch, the workspace query and the
// debug hook.  Key blocks x sequences is the dK/dV kernel's parallelism before the heads are cut: the heads are cut into as many chunks
// as it takes to offer every compute unit two workgroups and to keep the heaviest workgroup within a compute unit's share of the
// work, at most kMlaBwdMaxChunks (the bound of the dk_pe planes: 4 KiB per key row) and at most one per head; one chunk writes dk_pe
// itself and no reduce runs.  A grid beyond 31 bits: ok = false.
MlaPrefillBwdPlan mla_prefill_bwd_plan(int Tq, int Tk, int B, int H, int max_seqlen_q, int max_seqlen_k, int device) {
    MlaPrefillBwdPlan pl;
    pl.max_chunks = kMlaBwdMaxChunks;
    if (B <= 0 || H <= 0 || (Tq <= 0 && Tk <= 0)) return pl;
    const long long nq = seqlen_cut(max_seqlen_q, Tq), nk = seqlen_cut(max_seqlen_k, Tk);
    const long long qblocks = nq > 0 ? (nq + kPQ - 1) / kPQ : 0, kblocks = nk > 0 ? (nk + kVKB - 1) / kVKB : 0;
    pl.heads_per_chunk = H;
    pl.n_chunks = 1;
    if (kblocks > 0) {
        const long long cus = device_cu_count(device);
        const long long base = kblocks * B, want = (2 * cus + base - 1) / base;
        const long long chunks = want < 1 ? 1 : want > kMlaBwdMaxChunks ? kMlaBwdMaxChunks : want;
        long long hpc = (H + chunks - 1) / chunks;          // (chunks > H: 1)
        // ... and no workgroup outweighs a compute unit's share: the heaviest one (key block 0 of the longest sequence) walks up to
        // min(max_seqlen_q, Tq) rows per head, while the whole call has about H Tq Tk / B row-key pairs (equal lengths: a ragged batch has
        // more), half of them under a causal mask.  Without this a ragged batch with few long sequences ran at a fifth of the rate
        // (DESIGN.md 3.11): its grid is wide, but most of its workgroups return at once.
        const double fair = nq > 0 ? (double)H * Tq * Tk / (2.0 * B * cus * nq * kVKB) : 1.0;
        if (fair < (double)hpc) hpc = fair < 1.0 ? 1 : (long long)fair;
        const long long least = (H + kMlaBwdMaxChunks - 1) / kMlaBwdMaxChunks;
        pl.heads_per_chunk = (int)(hpc < least ? least : hpc);
        pl.n_chunks = (H + pl.heads_per_chunk - 1) / pl.heads_per_chunk;   // the last chunk may be short
    }
    pl.dq_grid = qblocks * H * B;
    pl.delta_grid = pl.dq_grid > 0 ? ((long long)Tq * H + 3) / 4 : 0;
    pl.dkdv_grid = kblocks * B * pl.n_chunks;
    pl.reduce = pl.dkdv_grid > 0 && pl.n_chunks > 1;
    pl.reduce_grid = pl.reduce ? kblocks * B : 0;
    pl.delta_bytes = pl.dq_grid > 0 ? ((uint64_t)Tq * H * sizeof(float) + 255) / 256 * 256 : 0;
    pl.ws_bytes = pl.delta_bytes + (pl.reduce ? (uint64_t)pl.n_chunks * Tk * kDR * sizeof(float) : 0);
    pl.ok = pl.dq_grid <= 0x7fffffffll && pl.delta_grid <= 0x7fffffffll && pl.dkdv_grid <= 0x7fffffffll && (long long)Tq + kPQ <= 0x7fffffffll;
    return pl;
}

int launch_mla_prefill_bwd(const MlaPrefillBwdArgs& a, const MlaPrefillBwdPlan& plan, void* ws, hipStream_t stream) {
    const MlaPrefillArgs& f = a.fwd;
    if (!plan.ok || f.causal < 0 || f.causal > 2) return -1;
    if (plan.dq_grid <= 0 && plan.dkdv_grid <= 0) return 0;
    if (plan.ws_bytes > 0 && ws == nullptr) return -1;
    MlaBwdParams p;
    mla_inputs(p, f);
    p.o = static_cast<const char*>(a.o); p.dout = static_cast<const char*>(a.dout);
    p.lse = a.lse;
    p.delta = static_cast<float*>(ws);
    p.part = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.delta_bytes);
    p.dq = static_cast<char*>(a.dq); p.dkn = static_cast<char*>(a.dk_nope); p.dkp = static_cast<char*>(a.dk_pe); p.dv = static_cast<char*>(a.dv);
    p.dkn_stride = a.dk_nope_token_stride; p.dkn_hstride = a.dk_nope_head_stride;
    p.dv_stride = a.dv_token_stride; p.dv_hstride = a.dv_head_stride;
    p.hpc = plan.heads_per_chunk; p.nchunks = plan.n_chunks;
    p.scale = f.scale;
    if (f.dtype == kBF16) return launch_instance<Bf16Traits>(p, plan, stream);
    if (f.dtype == kF16) return launch_instance<F16Traits>(p, plan, stream);
    return -1;
}

}  // namespace aule_hip
