// fa_bwd_d256_gfx950.hip -- backward for head_dim = 256, every dtype (route bit 128 of aule_hip_debug_last_backward_route).
//
// Three launches, the layout of fa_d256_common.h:
//   delta     delta = rowsum(dO * O) in fp32 (one wave per row)
//   dQ        4 waves x 32 query rows; K / V tiles of 64 keys stream through LDS; S^T = K.Q^T and dP^T = V.dO^T with Q and dO of
//             the wave's rows as B operands (16-bit: in registers); dS^T = P^T (dP^T - delta) is the B operand of
//             dQ^T[d][q] += K^T.dS^T, K read transposed from the same LDS tile.  dQ = scale * acc.
//   dK / dV   4 waves x 32 keys; each workgroup owns ONE 128-column half of dK and dV and recomputes S and dP over all 256
//             columns (the other half's workgroup does the same): S = Q.K^T and dP = dO.V^T with K and V of the wave's keys as
//             B operands, dV^T[d][key] += dO^T.P and dK^T[d][key] += Q^T.dS over 32-row Q / dO tiles in LDS.  The split costs
//             1.5x the MFMAs of an unsplit dK/dV kernel (per 32 x 32 tile and half: 16 + 16 for S and dP, 8 + 8 for dV and dK);
//             an unsplit wave would hold 256 accumulator registers for dK + dV next to K and V.
//             GQA / MQA: the workgroup walks every query head of its KV head's group itself (no partial planes, no reduction pass).
// Masks as the forward (causal with the position offset, sliding window, ragged tails); P is exp2(S c - L log2 e) with L the
// forward's LSE, and keys a query does not see contribute nothing (rows without any visible key: LSE = -inf, P = 0).
// The workspace is delta alone: B Hq Sq fp32 (bwd_plan at D = 256).
#include <cstdlib>

#include "fa_d256_common.h"
#include "fa_kernels.h"

namespace aule_hip {
namespace {

struct BwdD256Params {
    const void* q;
    const void* k;
    const void* v;
    const void* o;
    const void* dout;
    const float* lse;
    float* delta;
    void* dq;
    void* dk;
    void* dv;
    int B, Hq, Hkv, Sq, Sk;
    float c;       // scale * log2(e)
    float scale;
    int causal, window, coff;
    int nblk;      // dQ: 128-row query blocks per head; dK/dV: 128-key blocks per KV head
};

constexpr int kBQ = 128;   // dQ: query rows per workgroup
constexpr int kBK = 64;    // dQ: keys per tile
constexpr int kBKB = 128;  // dK/dV: keys per workgroup
constexpr int kBQT = 32;   // dK/dV: query rows per tile

template <class T>
__global__ void __launch_bounds__(256) fa_bwd_d256_delta_kernel(const BwdD256Params p, long long rows) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float acc = 0.f;
    if constexpr (T::kDType == 0) {
        const f32x4_t a = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(p.o) + row * kD256 + 4 * lane);
        const f32x4_t b = *reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(p.dout) + row * kD256 + 4 * lane);
        acc = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
    } else {
        const u32x2_t a = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const char*>(p.o) + (row * kD256 + 4 * lane) * 2);
        const u32x2_t b = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const char*>(p.dout) + (row * kD256 + 4 * lane) * 2);
        acc = T::lo(a[0]) * T::lo(b[0]) + T::hi(a[0]) * T::hi(b[0]) + T::lo(a[1]) * T::lo(b[1]) + T::hi(a[1]) * T::hi(b[1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) p.delta[row] = acc;
}

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_d256_dq_kernel(const BwdD256Params p) {
    using C = D256Cfg<T>;
    constexpr bool F32 = T::kDType == 0;
    constexpr int G = C::G;
    __shared__ __attribute__((aligned(16))) char Ks[kBK * C::PAT];
    __shared__ __attribute__((aligned(16))) char Vs[kBK * C::PA];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const WorkItem w = decode_work((int)blockIdx.x, p.B, p.Hq, p.Hkv, p.nblk, p.causal != 0);
    const int q0 = w.blk * kBQ;
    const long long qhead = (long long)w.b * p.Hq + w.h, kvhead = (long long)w.b * p.Hkv + w.hk;
    const unsigned qbytes = (unsigned)(p.Sq * C::RB), kbytes = (unsigned)(p.Sk * C::RB);
    const __amdgpu_buffer_rsrc_t qrs = make_srd(reinterpret_cast<const char*>(p.q) + qhead * qbytes, qbytes);
    const __amdgpu_buffer_rsrc_t ors = make_srd(reinterpret_cast<const char*>(p.dout) + qhead * qbytes, qbytes);
    const __amdgpu_buffer_rsrc_t krs = make_srd(reinterpret_cast<const char*>(p.k) + kvhead * kbytes, kbytes);
    const __amdgpu_buffer_rsrc_t vrs = make_srd(reinterpret_cast<const char*>(p.v) + kvhead * kbytes, kbytes);

    const int qi = q0 + wave * 32 + l31;
    const int pos = qi + p.coff;
    const bool causal = p.causal != 0;
    const bool valid = qi < p.Sq;
    const float l2 = valid ? p.lse[qhead * p.Sq + qi] * kLog2e : 0.f;
    const float dl = valid ? p.delta[qhead * p.Sq + qi] : 0.f;

    const int qlast = min(q0 + kBQ, p.Sq) - 1;
    int kend = p.Sk;
    if (causal) kend = min(kend, qlast + p.coff + 1);
    int kbeg = 0;
    if (p.window > 0) kbeg = max(0, q0 + p.coff - p.window + 1) / kBK * kBK;
    const int ntiles = kend > kbeg ? (kend - kbeg + kBK - 1) / kBK : 0;

    u32x4_t qf[F32 ? 1 : G], of[F32 ? 1 : G];
    if constexpr (!F32) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            qf[g] = __builtin_amdgcn_raw_buffer_load_b128(qrs, qi * C::RB + 32 * g + 16 * hi, 0, 0);
            of[g] = __builtin_amdgcn_raw_buffer_load_b128(ors, qi * C::RB + 32 * g + 16 * hi, 0, 0);
        }
    }
    f32x16_t acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = f32x16_t{};

    TileLoad<T, kBK> kt, vt;
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kBK;
        kt.load(krs, k0, tid);
        vt.load(vrs, k0, tid);
        __syncthreads();
        kt.store(Ks, C::PAT, tid);
        vt.store(Vs, C::PA, tid);
        __syncthreads();
        f32x16_t s[2] = {f32x16_t{}, f32x16_t{}}, dp[2] = {f32x16_t{}, f32x16_t{}};
        constexpr int kUnrollG = F32 ? 2 : G;
#pragma unroll kUnrollG
        for (int g = 0; g < G; ++g) {
            u32x4_t bq, bo;
            if constexpr (F32) {
                bq = __builtin_amdgcn_raw_buffer_load_b128(qrs, qi * C::RB + 32 * g + 16 * hi, 0, 0);
                bo = __builtin_amdgcn_raw_buffer_load_b128(ors, qi * C::RB + 32 * g + 16 * hi, 0, 0);
            } else {
                bq = qf[g];
                bo = of[g];
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                s[kk] = mfma_chunk<T>(lds_b128(Ks + (32 * kk + l31) * C::PAT + 32 * g + 16 * hi), bq, s[kk]);
                dp[kk] = mfma_chunk<T>(lds_b128(Vs + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), bo, dp[kk]);
            }
        }
        // dS^T = P^T (dP^T - delta), P^T = exp2(S^T c - L log2 e) on visible keys
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = k0 + 32 * kk + crow(r, hi);
                const float pr = d256_visible(pos, j, p.Sk, causal, p.window) ? fast_exp2(s[kk][r] * p.c - l2) : 0.f;
                s[kk][r] = pr * (dp[kk][r] - dl);
            }
        // dQ^T[d][q] += K^T.dS^T
        if constexpr (F32) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll 4
                for (int r = 0; r < 16; ++r) {
                    const char* krow = Ks + (32 * kk + crow(r, 0) + 4 * hi) * C::PAT + 4 * l31;
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt)
                        acc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(*reinterpret_cast<const float*>(krow + 128 * dt), s[kk][r], acc[dt], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const u32x4_t b = pack_step<T>(s[st >> 1], st & 1);
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) acc[dt] = mfma16<T>(lds_tr_step(Ks, C::PAT, 16 * st, 32 * dt, lane), b, acc[dt]);
            }
        }
    }
    if (!valid) return;
    char* g = reinterpret_cast<char*>(p.dq) + (qhead * p.Sq + qi) * (long long)C::RB;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = acc[dt][4 * g4] * p.scale, a1 = acc[dt][4 * g4 + 1] * p.scale;
            const float a2 = acc[dt][4 * g4 + 2] * p.scale, a3 = acc[dt][4 * g4 + 3] * p.scale;
            if constexpr (F32) *reinterpret_cast<f32x4_t*>(g + d * 4) = f32x4_t{a0, a1, a2, a3};
            else *reinterpret_cast<u32x2_t*>(g + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
}

template <class T>
__global__ void __launch_bounds__(256, 1) fa_bwd_d256_dkdv_kernel(const BwdD256Params p) {
    using C = D256Cfg<T>;
    constexpr bool F32 = T::kDType == 0;
    constexpr int G = C::G;
    __shared__ __attribute__((aligned(16))) char Qs[kBQT * C::PAT];
    __shared__ __attribute__((aligned(16))) char Os[kBQT * C::PAT];
    __shared__ float Ls[kBQT], Dl[kBQT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // blockIdx -> (batch, kv head, key block, column half): key block 0 first (under the causal rule it sees the most queries)
    const int hf = (int)(blockIdx.x & 1);
    const int rest = (int)(blockIdx.x >> 1);
    const int kb = rest % p.nblk;
    const int unit = rest / p.nblk;
    const int b = unit / p.Hkv, hk = unit % p.Hkv;
    const int grp = p.Hq / p.Hkv;
    const int k0 = kb * kBKB;
    const long long kvhead = (long long)b * p.Hkv + hk;
    const unsigned qbytes = (unsigned)(p.Sq * C::RB), kbytes = (unsigned)(p.Sk * C::RB);
    const __amdgpu_buffer_rsrc_t krs = make_srd(reinterpret_cast<const char*>(p.k) + kvhead * kbytes, kbytes);
    const __amdgpu_buffer_rsrc_t vrs = make_srd(reinterpret_cast<const char*>(p.v) + kvhead * kbytes, kbytes);
    const bool causal = p.causal != 0;

    const int kj = k0 + wave * 32 + l31;   // this lane's key
    const int c0 = 128 * hf;               // first output column of this workgroup

    // query range that sees any key of the block
    const int klast = min(k0 + kBKB, p.Sk) - 1;
    int qbeg = 0, qend = p.Sq;
    if (causal) qbeg = max(0, k0 - p.coff);
    if (p.window > 0) qend = min(qend, max(0, klast + p.window - p.coff));
    qbeg = qbeg / kBQT * kBQT;
    const int ntiles = qend > qbeg ? (qend - qbeg + kBQT - 1) / kBQT : 0;

    u32x4_t kf[F32 ? 1 : G], vf[F32 ? 1 : G];
    if constexpr (!F32) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            kf[g] = __builtin_amdgcn_raw_buffer_load_b128(krs, kj * C::RB + 32 * g + 16 * hi, 0, 0);
            vf[g] = __builtin_amdgcn_raw_buffer_load_b128(vrs, kj * C::RB + 32 * g + 16 * hi, 0, 0);
        }
    }
    f32x16_t dk[4], dv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dk[i] = dv[i] = f32x16_t{};

    TileLoad<T, kBQT> qt, ot;
    for (int hh = 0; hh < grp; ++hh) {
        const long long qhead = (long long)b * p.Hq + hk * grp + hh;
        const __amdgpu_buffer_rsrc_t qrs = make_srd(reinterpret_cast<const char*>(p.q) + qhead * qbytes, qbytes);
        const __amdgpu_buffer_rsrc_t ors = make_srd(reinterpret_cast<const char*>(p.dout) + qhead * qbytes, qbytes);
        for (int t = 0; t < ntiles; ++t) {
            const int qt0 = qbeg + t * kBQT;
            qt.load(qrs, qt0, tid);
            ot.load(ors, qt0, tid);
            __syncthreads();
            qt.store(Qs, C::PAT, tid);
            ot.store(Os, C::PAT, tid);
            if (tid < kBQT) {
                const int qi = qt0 + tid;
                Ls[tid] = qi < p.Sq ? p.lse[qhead * p.Sq + qi] * kLog2e : 0.f;
                Dl[tid] = qi < p.Sq ? p.delta[qhead * p.Sq + qi] : 0.f;
            }
            __syncthreads();
            // S[q][key] = Q.K^T, dP[q][key] = dO.V^T
            f32x16_t s = f32x16_t{}, dp = f32x16_t{};
            constexpr int kUnrollG = F32 ? 2 : G;
#pragma unroll kUnrollG
            for (int g = 0; g < G; ++g) {
                u32x4_t bk, bv;
                if constexpr (F32) {
                    bk = __builtin_amdgcn_raw_buffer_load_b128(krs, kj * C::RB + 32 * g + 16 * hi, 0, 0);
                    bv = __builtin_amdgcn_raw_buffer_load_b128(vrs, kj * C::RB + 32 * g + 16 * hi, 0, 0);
                } else {
                    bk = kf[g];
                    bv = vf[g];
                }
                s = mfma_chunk<T>(lds_b128(Qs + l31 * C::PAT + 32 * g + 16 * hi), bk, s);
                dp = mfma_chunk<T>(lds_b128(Os + l31 * C::PAT + 32 * g + 16 * hi), bv, dp);
            }
            // P and dS (rows q = crow(r, hi) of the tile)
            f32x16_t ds;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = crow(r, hi);
                const int qi = qt0 + qr;
                const bool vis = qi < p.Sq && d256_visible(qi + p.coff, kj, p.Sk, causal, p.window);
                const float pr = vis ? fast_exp2(s[r] * p.c - Ls[qr]) : 0.f;
                s[r] = pr;
                ds[r] = pr * (dp[r] - Dl[qr]);
            }
            // dV^T[d][key] += dO^T.P, dK^T[d][key] += Q^T.dS over this workgroup's 128 columns
            if constexpr (F32) {
#pragma unroll 4
                for (int r = 0; r < 16; ++r) {
                    const int qr = crow(r, 0) + 4 * hi;
                    const char* orow = Os + qr * C::PAT + 4 * (c0 + l31);
                    const char* qrow = Qs + qr * C::PAT + 4 * (c0 + l31);
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        dv[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(*reinterpret_cast<const float*>(orow + 128 * dt), s[r], dv[dt], 0, 0, 0);
                        dk[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(*reinterpret_cast<const float*>(qrow + 128 * dt), ds[r], dk[dt], 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int st = 0; st < 2; ++st) {
                    const u32x4_t pb = pack_step<T>(s, st), db = pack_step<T>(ds, st);
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) {
                        dv[dt] = mfma16<T>(lds_tr_step(Os, C::PAT, 16 * st, c0 + 32 * dt, lane), pb, dv[dt]);
                        dk[dt] = mfma16<T>(lds_tr_step(Qs, C::PAT, 16 * st, c0 + 32 * dt, lane), db, dk[dt]);
                    }
                }
            }
        }
    }
    if (kj >= p.Sk) return;
    char* gk = reinterpret_cast<char*>(p.dk) + (kvhead * p.Sk + kj) * (long long)C::RB;
    char* gv = reinterpret_cast<char*>(p.dv) + (kvhead * p.Sk + kj) * (long long)C::RB;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = c0 + 32 * dt + 8 * g4 + 4 * hi;
            const float k0v = dk[dt][4 * g4] * p.scale, k1v = dk[dt][4 * g4 + 1] * p.scale;
            const float k2v = dk[dt][4 * g4 + 2] * p.scale, k3v = dk[dt][4 * g4 + 3] * p.scale;
            const float v0 = dv[dt][4 * g4], v1 = dv[dt][4 * g4 + 1], v2 = dv[dt][4 * g4 + 2], v3 = dv[dt][4 * g4 + 3];
            if constexpr (F32) {
                *reinterpret_cast<f32x4_t*>(gk + d * 4) = f32x4_t{k0v, k1v, k2v, k3v};
                *reinterpret_cast<f32x4_t*>(gv + d * 4) = f32x4_t{v0, v1, v2, v3};
            } else {
                *reinterpret_cast<u32x2_t*>(gk + d * 2) = u32x2_t{T::pack2(k0v, k1v), T::pack2(k2v, k3v)};
                *reinterpret_cast<u32x2_t*>(gv + d * 2) = u32x2_t{T::pack2(v0, v1), T::pack2(v2, v3)};
            }
        }
}

template <class T>
int launch_d256(const BwdArgs& a, hipStream_t stream) {
    BwdD256Params p;
    p.q = a.q; p.k = a.k; p.v = a.v; p.o = a.o; p.dout = a.dout; p.lse = a.lse; p.delta = a.delta;
    p.dq = a.dq; p.dk = a.dk; p.dv = a.dv;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = a.Sq; p.Sk = a.Sk;
    p.c = a.scale * kLog2e;
    p.scale = a.scale;
    p.causal = a.causal;
    p.window = a.window > 0 ? a.window : 0;
    p.coff = a.causal ? a.coff : 0;
    const long long rows = (long long)a.B * a.Hq * a.Sq;
    const long long kvrows = (long long)a.B * a.Hkv * a.Sk;
    if (kvrows <= 0) return 0;
    if (rows <= 0) {   // no query: the gradients of K and V are zero
        const size_t bytes = (size_t)kvrows * kD256 * D256Cfg<T>::ES;
        hipError_t e = hipMemsetAsync(a.dk, 0, bytes, stream);
        if (e == hipSuccess) e = hipMemsetAsync(a.dv, 0, bytes, stream);
        return (int)e;
    }
    hipLaunchKernelGGL((fa_bwd_d256_delta_kernel<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, p, rows);
    p.nblk = (a.Sq + kBQ - 1) / kBQ;
    hipLaunchKernelGGL((fa_bwd_d256_dq_kernel<T>), dim3((unsigned)((long long)a.B * a.Hq * p.nblk)), dim3(256), 0, stream, p);
    p.nblk = (a.Sk + kBKB - 1) / kBKB;
    hipLaunchKernelGGL((fa_bwd_d256_dkdv_kernel<T>), dim3((unsigned)(2ll * a.B * a.Hkv * p.nblk)), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// launch_bwd's entry for D = 256 (every dtype)
int launch_bwd_d256(const BwdArgs& a, hipStream_t stream) {
    if (a.D != kD256) return -1;
    if (a.dtype == kBF16) return launch_d256<Bf16Traits>(a, stream);
    if (a.dtype == kF16) return launch_d256<F16Traits>(a, stream);
    if (a.dtype == kF32) return launch_d256<F32Traits>(a, stream);
    return -1;
}

// delta [B, Hq, Sq] fp32, on a 256-byte boundary
uint64_t bwd_d256_workspace_bytes(int B, int Hq, int Sq) {
    return ((uint64_t)B * Hq * Sq * sizeof(float) + 255) / 256 * 256;
}

}  // namespace aule_hip
