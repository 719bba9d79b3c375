// fa_varlen_d256.h -- what the head_dim 256 variable-length kernels share (fa_fwd_varlen_d256_gfx950.hip, fa_bwd_varlen_d256_gfx950.hip;
// DESIGN.md 3.21): the parameter block the kernels read and the one place that fills it from VarlenArgs.  The decomposition, the
// clamps, the tile source and the mask predicates are fa_varlen_common.h's; the pitches PrefillCfg<256> (PA 528, PT 576) and
// VarlenCfg<256>::PAT = D256Cfg::PAT (592).
#pragma once
#include "fa_kernels.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

constexpr int kVD = 256;
using CV256 = VarlenCfg<kVD>;
static_assert(CV256::PA == 528 && CV256::PT == 576 && CV256::PAT == D256Cfg<Bf16Traits>::PAT, "the pitches of the 256-wide kernels");

struct VarlenD256Params {
    const char* q;
    const char* k;
    const char* v;
    char* o;              // forward: written
    float* lse_out;       // forward: written (null: skipped)
    const char* dout;     // backward from here on
    const float* lse;
    const float* delta;
    char* dq;
    char* dk;
    char* dv;
    const int* cu_q;
    const int* cu_k;
    long long q_stride, k_stride, v_stride;   // elements between tokens
    int Tq, Tk, B, Hq, Hkv, g;
    int max_sq, max_sk;
    float c;       // scale * log2(e)
    float scale;
    int causal;    // 0, 1, 2
    int window;    // > 0: on
};

// (`a` passed varlen_args_ok)
inline VarlenD256Params varlen_d256_params(const VarlenArgs& a) {
    VarlenD256Params p;
    p.q = static_cast<const char*>(a.q); p.k = static_cast<const char*>(a.k); p.v = static_cast<const char*>(a.v);
    p.o = static_cast<char*>(a.out); p.lse_out = a.lse;
    p.dout = static_cast<const char*>(a.dout); p.lse = a.lse; p.delta = a.delta;
    p.dq = static_cast<char*>(a.dq); p.dk = static_cast<char*>(a.dk); p.dv = static_cast<char*>(a.dv);
    p.cu_q = a.cu_seqlens_q; p.cu_k = a.cu_seqlens_k;
    p.q_stride = a.q_token_stride; p.k_stride = a.k_token_stride; p.v_stride = a.v_token_stride;
    p.Tq = a.Tq; p.Tk = a.Tk; p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.g = a.Hq / a.Hkv;
    p.max_sq = varlen_max_sq(a);
    p.max_sk = varlen_max_sk(a);
    p.c = a.scale * kLog2e;
    p.scale = a.scale;
    p.causal = a.causal;
    p.window = varlen_window(a);
    return p;
}

}  // namespace
}  // namespace aule_hip
