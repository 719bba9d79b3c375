// fa_mla_prefill_common.h -- what the MLA 192 / 128 prefill forward and backward share (fa_fwd_mla_prefill_gfx950.hip,
// fa_bwd_mla_prefill_gfx950.hip): the widths, the host-side fill of the fields both parameter structs name alike, the K tile
// assembled from its two sources, and the shape the dQ body of fa_varlen_common.h runs with.  The two parameter structs stay apart:
// deriving both from one input struct moved the kernel arguments and cost the dQ kernel four SGPRs.
#pragma once
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

constexpr int kDQK = 192;    // q / key width: 128 (nope) + 64 (rope)
constexpr int kDN = 128;     // k_nope width
constexpr int kDR = 64;      // k_pe width
constexpr int kDV = 128;     // value / output width

// Host: the fields both parameter structs (forward, backward) name alike, from the C-level arguments; the max_seqlen cuts included
template <class P>
void mla_inputs(P& p, const MlaPrefillArgs& a) {
    p.q = static_cast<const char*>(a.q); p.k_nope = static_cast<const char*>(a.k_nope); p.k_pe = static_cast<const char*>(a.k_pe);
    p.v = static_cast<const char*>(a.v);
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k;
    p.q_stride = a.q_token_stride;
    p.kn_stride = a.k_nope_token_stride; p.kn_hstride = a.k_nope_head_stride;
    p.v_stride = a.v_token_stride; p.v_hstride = a.v_head_stride;
    p.kp_stride = a.k_pe_token_stride;
    p.Tq = a.Tq; p.Tk = a.Tk; p.B = a.B; p.H = a.H;
    p.max_sq = seqlen_cut(a.max_seqlen_q, a.Tq);
    p.max_sk = seqlen_cut(a.max_seqlen_k, a.Tk);
    p.c = a.scale * kLog2e;
    p.causal = a.causal;
}

// One K tile (from its two sources) and one V tile of 64 keys of sequence rows sk .. on their way to LDS; rows at or beyond kend
// (<= L: inside the tensors) are not read.
struct MlaKeyTiles {
    RowTile<kDN, kPK> kn;   // 4 chunks per thread
    RowTile<kDR, kPK> kp;   // 2
    RowTile<kDV, kPK> v;    // 4
    const char* knbase;
    const char* kpbase;
    const char* vbase;
    long long knpitch, kppitch, vpitch;
    int kend;
    template <class P>
    __device__ __forceinline__ MlaKeyTiles(const P& p, const QueryBlock& x, int head)
        : knbase(p.k_nope + ((long long)x.sk * p.kn_stride + (long long)head * p.kn_hstride) * 2), kpbase(p.k_pe + (long long)x.sk * p.kp_stride * 2),
          vbase(p.v + ((long long)x.sk * p.v_stride + (long long)head * p.v_hstride) * 2),
          knpitch(p.kn_stride * 2), kppitch(p.kp_stride * 2), vpitch(p.v_stride * 2), kend(x.kend) {}
    __device__ __forceinline__ void load(int k0, int tid) {
        kn.load([&](int row) { return k0 + row < kend ? knbase + (long long)(k0 + row) * knpitch : nullptr; }, tid);
        kp.load([&](int row) { return k0 + row < kend ? kpbase + (long long)(k0 + row) * kppitch : nullptr; }, tid);
        v.load([&](int row) { return k0 + row < kend ? vbase + (long long)(k0 + row) * vpitch : nullptr; }, tid);
    }
    // k_nope in columns 0 .. 127 of the K image, k_pe in 128 .. 191
    __device__ __forceinline__ void store(char* Ks, int kp_, char* Vs, int vp, int tid) const {
        kn.store(Ks, kp_, tid);
        kp.store(Ks + kDN * 2, kp_, tid);
        v.store(Vs, vp, tid);
    }
};

// The shape of the MLA prefill kernels: 192-wide q and key rows, 128-wide values, every head its own KV head
struct MlaShape {
    static constexpr int DQK = kDQK, DV = kDV;
    using Tiles = MlaKeyTiles;
    template <class P>
    static __device__ __forceinline__ int q_heads(const P& p) { return p.H; }
    template <class P>
    static __device__ __forceinline__ int kv_heads(const P& p) { return p.H; }
};

}  // namespace
}  // namespace aule_hip
