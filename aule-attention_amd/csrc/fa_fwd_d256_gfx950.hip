// fa_fwd_d256_gfx950.hip -- forward for head_dim = 256 (16-bit: route 9; fp32: the fp32 route 0 at this width).
//
// The D <= 128 kernels do not stretch to 256: the ping-pong kernel's LDS plan comes to 262 KB, the one-wave-per-SIMD streams
// are generated for 64 / 128 only, and the fp32 kernel spills 212 registers.  This one follows fa_d256_common.h:
//   workgroup = 4 waves x 32 query rows (one wave per SIMD), Q of the wave's rows in registers (16-bit: 64 VGPRs),
//   K / V tiles of 64 rows in LDS (16-bit: the next tile prefetched into registers while this one is computed),
//   S^T[key][q] = K.Q^T (2 accumulators), P^T as the B operand of O^T[d][q] += V^T.P^T (8 accumulators = 128 registers).
// Online softmax in log2 units with fp32 m, l, acc as the other forward kernels; P is cast to the
// V dtype before the PV product; a row without a visible key writes O = 0 and LSE = -inf.  Masks: causal with the position
// offset (bottom-right), sliding window, ragged tails (the buffer descriptors return 0 past the end; masked keys are -inf).
// Work order: decode_work (fa_device.h), heaviest causal blocks first, every block of one (batch, kv head) on one XCD.
// Short queries against long K/V run here too, one 128-row block per head (no key-range split at this width).
#include <cstdlib>

#include "fa_d256_common.h"
#include "fa_kernels.h"

namespace aule_hip {
namespace {

struct FwdD256Params {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    float* lse;
    int B, Hq, Hkv, Sq, Sk;
    float c;     // scale * log2(e) (sign kept)
    int causal, window, coff;
    int nqb;     // 128-row query blocks per head
};

constexpr int kFQ = 128;   // query rows per workgroup
constexpr int kFK = 64;    // keys per tile

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_d256_kernel(const FwdD256Params p) {
    using C = D256Cfg<T>;
    constexpr bool F32 = T::kDType == 0;
    constexpr int G = C::G;
    __shared__ __attribute__((aligned(16))) char Ks[kFK * C::PA];
    __shared__ __attribute__((aligned(16))) char Vs[kFK * C::PT];

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const WorkItem w = decode_work((int)blockIdx.x, p.B, p.Hq, p.Hkv, p.nqb, p.causal != 0);
    const int q0 = w.blk * kFQ;
    const long long qhead = (long long)w.b * p.Hq + w.h, kvhead = (long long)w.b * p.Hkv + w.hk;
    const char* qg = reinterpret_cast<const char*>(p.q) + qhead * p.Sq * C::RB;
    const __amdgpu_buffer_rsrc_t qrs = make_srd(qg, (unsigned)(p.Sq * C::RB));
    const __amdgpu_buffer_rsrc_t krs = make_srd(reinterpret_cast<const char*>(p.k) + kvhead * p.Sk * C::RB, (unsigned)(p.Sk * C::RB));
    const __amdgpu_buffer_rsrc_t vrs = make_srd(reinterpret_cast<const char*>(p.v) + kvhead * p.Sk * C::RB, (unsigned)(p.Sk * C::RB));

    const int qi = q0 + wave * 32 + l31;   // this lane's query
    const int pos = qi + p.coff;
    const bool causal = p.causal != 0;

    // key tiles this block needs
    const int qlast = min(q0 + kFQ, p.Sq) - 1;
    int kend = p.Sk;
    if (causal) kend = min(kend, qlast + p.coff + 1);
    int kbeg = 0;
    if (p.window > 0) kbeg = max(0, q0 + p.coff - p.window + 1) / kFK * kFK;
    const int ntiles = kend > kbeg ? (kend - kbeg + kFK - 1) / kFK : 0;

    // Q operand chunks of this lane's row (16-bit: held; fp32: re-read per tile through the descriptor)
    u32x4_t qf[F32 ? 1 : G];
    if constexpr (!F32) {
#pragma unroll
        for (int g = 0; g < G; ++g) qf[g] = __builtin_amdgcn_raw_buffer_load_b128(qrs, qi * C::RB + 32 * g + 16 * hi, 0, 0);
    }

    f32x16_t o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = f32x16_t{};
    float m = -__builtin_inff(), l = 0.f;

    TileLoad<T, kFK> kt, vt;
    if (ntiles > 0 && !F32) {
        kt.load(krs, kbeg, tid);
        vt.load(vrs, kbeg, tid);
    }
    for (int t = 0; t < ntiles; ++t) {
        const int k0 = kbeg + t * kFK;
        if constexpr (F32) {
            kt.load(krs, k0, tid);
            vt.load(vrs, k0, tid);
        }
        __syncthreads();   // every wave is done with the previous tile
        kt.store(Ks, C::PA, tid);
        vt.store(Vs, C::PT, tid);
        __syncthreads();
        if constexpr (!F32) {
            if (t + 1 < ntiles) {
                kt.load(krs, k0 + kFK, tid);
                vt.load(vrs, k0 + kFK, tid);
            }
        }
        // S^T[key][q] = K.Q^T over the 64 keys of the tile
        f32x16_t s[2] = {f32x16_t{}, f32x16_t{}};
        constexpr int kUnrollG = F32 ? 4 : G;   // (fp32: the fully unrolled re-reads of Q ran out of scalar registers)
#pragma unroll kUnrollG
        for (int g = 0; g < G; ++g) {
            u32x4_t b;
            if constexpr (F32) b = __builtin_amdgcn_raw_buffer_load_b128(qrs, qi * C::RB + 32 * g + 16 * hi, 0, 0);
            else b = qf[g];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                s[kk] = mfma_chunk<T>(lds_b128(Ks + (32 * kk + l31) * C::PA + 32 * g + 16 * hi), b, s[kk]);
        }
        // mask, scale to log2 units, running max over the lane pair (lanes l and l + 32 hold the same query)
        float mx = -__builtin_inff();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = k0 + 32 * kk + crow(r, hi);
                const float x = d256_visible(pos, j, p.Sk, causal, p.window) ? s[kk][r] * p.c : -__builtin_inff();
                s[kk][r] = x;
                mx = fmaxf(mx, x);
            }
        mx = fmaxf(mx, xhalf(mx));
        const float mn = fmaxf(m, mx);
        const float mu = mn == -__builtin_inff() ? 0.f : mn;
        const float alpha = fast_exp2(m - mu);   // m = -inf: 0
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] *= alpha;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = fast_exp2(s[kk][r] - mu);
                s[kk][r] = e;
                l += e;
            }
        // O^T[d][q] += V^T.P^T
        if constexpr (F32) {
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const char* vrow = Vs + (32 * kk + crow(r, 0) + 4 * hi) * C::PT + 4 * l31;
#pragma unroll
                    for (int dt = 0; dt < 8; ++dt)
                        o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(*reinterpret_cast<const float*>(vrow + 128 * dt), s[kk][r], o[dt], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const u32x4_t pb = pack_step<T>(s[st >> 1], st & 1);
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) o[dt] = mfma16<T>(lds_tr_step(Vs, C::PT, 16 * st, 32 * dt, lane), pb, o[dt]);
            }
        }
    }
    l += xhalf(l);
    if (qi >= p.Sq) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;
    char* og = reinterpret_cast<char*>(p.o) + (qhead * p.Sq + qi) * (long long)C::RB;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 32 * dt + 8 * g4 + 4 * hi;
            const float a0 = o[dt][4 * g4] * inv, a1 = o[dt][4 * g4 + 1] * inv, a2 = o[dt][4 * g4 + 2] * inv, a3 = o[dt][4 * g4 + 3] * inv;
            if constexpr (F32) *reinterpret_cast<f32x4_t*>(og + d * 4) = f32x4_t{a0, a1, a2, a3};
            else *reinterpret_cast<u32x2_t*>(og + d * 2) = u32x2_t{T::pack2(a0, a1), T::pack2(a2, a3)};
        }
    if (p.lse != nullptr && hi == 0) {
        const float mu = m == -__builtin_inff() ? 0.f : m;
        p.lse[qhead * p.Sq + qi] = l > 0.f ? (mu + fast_log2(l)) * kLn2 : -__builtin_inff();
    }
}

template <class T>
int launch_d256(const FwdArgs& a, hipStream_t stream) {
    FwdD256Params p;
    p.q = a.q; p.k = a.k; p.v = a.v; p.o = a.o; p.lse = a.lse;
    p.B = a.B; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Sq = a.Sq; p.Sk = a.Sk;
    p.c = a.scale * kLog2e;
    p.causal = a.causal;
    p.window = a.window > 0 ? a.window : 0;
    p.coff = a.causal ? a.coff : 0;
    p.nqb = (a.Sq + kFQ - 1) / kFQ;
    const long long nblocks = (long long)a.B * a.Hq * p.nqb;
    if (nblocks <= 0) return 0;
    hipLaunchKernelGGL((fa_fwd_d256_kernel<T>), dim3((unsigned)nblocks), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace

// launch_fwd's entry for D = 256 (every dtype; single launch, no workspace)
int launch_fwd_d256(const FwdArgs& a, hipStream_t stream) {
    if (a.D != kD256 || a.rope_cos != nullptr) return -1;
    if (a.dtype == kBF16) return launch_d256<Bf16Traits>(a, stream);
    if (a.dtype == kF16) return launch_d256<F16Traits>(a, stream);
    if (a.dtype == kF32) return launch_d256<F32Traits>(a, stream);
    return -1;
}

}  // namespace aule_hip
