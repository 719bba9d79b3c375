// fa_bwd_sinks_gfx950.hip -- the gradient of the per-head sink logits of a variable-length batch.
//
// With the sink-inclusive lse of fa_fwd_varlen_gfx950.hip's SINK instances the sink's softmax weight at a row is
// w = exp(sinks[h] - lse[row, h]); it carries no value, so dL/dsinks[h] = sum over rows of w (0 - delta) with delta = rowsum(dO * O),
// which fa_bwd_varlen_gfx950.hip's delta pass has left in the workspace:
//     dsinks[h] = - sum over the rows some sequence owns of exp(sinks[h] - lse[row, h]) delta[row, h]
// Only owned rows [s_q, s_q + n) are walked, with the clamps of fa_varlen_common.h: lse of a row no sequence owns is whatever the
// allocation held, and delta there is the product of two such rows.  A head with sinks[h] = -inf has no sink: dsinks[h] = 0 exactly.
// Two launches, no atomics, a fixed summation order (two runs agree bit for bit):
//   partial   workgroup = (sequence, chunk of kSinkRows tokens): for passes of min(Hq, 256) heads, thread (row slot, head) sums its
//             rows of the chunk in order, the slots of a head are added in order through LDS -> part[sequence][chunk][head]; a chunk
//             past the sequence's end writes zeros (the workspace arrives unset).
//   reduce    one wave per head: lane i adds part[i], part[i + 64], ... in order, then the xor butterfly; writes -sum, exactly Hq floats.
#include "fa_kernels.h"
#include "fa_varlen_common.h"

namespace aule_hip {
namespace {

constexpr int kSinkRows = 256;   // tokens per workgroup of the partial pass

struct SinkBwdParams {
    const float* lse;
    const float* delta;
    const float* sinks;
    const int* cu_q;
    float* part;     // [B][chunks][Hq]
    float* dsinks;   // [Hq]
    int Tq, B, Hq;
    int max_sq, chunks;
};

__global__ void __launch_bounds__(256) fa_bwd_sinks_partial_kernel(const SinkBwdParams p) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x / p.chunks, chunk = (int)blockIdx.x - b * p.chunks;
    const SeqRange sq = seq_range(p.cu_q, b, p.Tq, p.max_sq);
    const int r0 = min(chunk * kSinkRows, sq.n), r1 = min(r0 + kSinkRows, sq.n);   // tokens r0 .. r1 - 1 of the sequence (none: zeros)
    const int hpb = min(p.Hq, 256);   // heads per pass
    const int slots = 256 / hpb;      // row slots per head
    const int slot = tid / hpb, hl = tid - slot * hpb;
    float* dst = p.part + (long long)blockIdx.x * p.Hq;
    for (int h0 = 0; h0 < p.Hq; h0 += hpb) {
        const int h = h0 + hl;
        float acc = 0.f;
        if (slot < slots && h < p.Hq) {
            const float s = p.sinks[h];
            if (s != -__builtin_inff())
                for (int r = r0 + slot; r < r1; r += slots) {
                    const long long at = ((long long)sq.s + r) * p.Hq + h;
                    acc += fast_exp2((s - p.lse[at]) * kLog2e) * p.delta[at];
                }
        }
        red[tid] = acc;
        __syncthreads();
        if (tid < hpb && h0 + tid < p.Hq) {
            float t = red[tid];
            for (int j = 1; j < slots; ++j) t += red[tid + j * hpb];
            dst[h0 + tid] = t;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) fa_bwd_sinks_reduce_kernel(const SinkBwdParams p) {
    const int lane = threadIdx.x & 63;
    const int h = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= p.Hq) return;
    const long long n = (long long)p.B * p.chunks;
    float acc = 0.f;
    for (long long i = lane; i < n; i += 64) acc += p.part[i * p.Hq + h];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) p.dsinks[h] = p.sinks[h] == -__builtin_inff() ? 0.f : -acc;
}

int sink_chunks(const VarlenArgs& a) { return (varlen_max_sq(a) + kSinkRows - 1) / kSinkRows; }

}  // namespace

// part [B][ceil(min(max_seqlen_q, Tq) / 256)][Hq] fp32
uint64_t varlen_dsinks_partial_bytes(const VarlenArgs& a) {
    if (a.B <= 0 || a.Hq <= 0 || a.Tq <= 0 || a.max_seqlen_q <= 0) return 0;
    return ((uint64_t)a.B * sink_chunks(a) * a.Hq * sizeof(float) + 255) / 256 * 256;
}

int launch_varlen_dsinks(const VarlenArgs& a, float* dsinks, float* partials, hipStream_t stream) {
    if (a.Hq <= 0 || a.B < 0 || a.sinks == nullptr || dsinks == nullptr) return -1;
    SinkBwdParams p;
    p.lse = a.lse; p.delta = a.delta; p.sinks = a.sinks; p.cu_q = a.cu_seqlens_q;
    p.part = partials; p.dsinks = dsinks;
    p.Tq = a.Tq; p.B = a.B; p.Hq = a.Hq;
    p.max_sq = a.Tq > 0 && a.max_seqlen_q > 0 ? varlen_max_sq(a) : 0;
    p.chunks = p.max_sq > 0 ? sink_chunks(a) : 0;
    const long long nwg = (long long)p.chunks * p.B;
    if (nwg > 0x7fffffffll) return -1;
    if (nwg > 0) {
        if (partials == nullptr || a.lse == nullptr || a.delta == nullptr) return -1;
        hipLaunchKernelGGL(fa_bwd_sinks_partial_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, p);
    } else {
        p.B = 0;   // nothing owned: the reduce writes zeros
    }
    hipLaunchKernelGGL(fa_bwd_sinks_reduce_kernel, dim3((unsigned)((p.Hq + 3) / 4)), dim3(256), 0, stream, p);
    return (int)hipGetLastError();
}

}  // namespace aule_hip
