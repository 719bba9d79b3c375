// fa_fwd_varlen_d256_gfx950.hip -- forward over a variable-length packed batch at head_dim 256.
//
// The tensors, the clamps of cu_seqlens_q / cu_seqlens_k, the positions and the visibility rule are those of fa_fwd_varlen_gfx950.hip
// (VarlenArgs, fa_kernels.h); q [Tq, Hq, 256], k, v [Tk, Hkv, 256], 16-bit, each with its own token stride.
//
// Layout: workgroup = (rank, sequence, KV head), rank 0 the sequence's last block of 128 token-major PACKED rows (QueryBlock), 4 waves
// x 32 rows, one workgroup per compute unit.  A lane keeps the 16 operand chunks of its Q row (64 registers), 8 output accumulators
// (128 registers, accumulation registers) and the row's m / l; lanes l and l + 32 hold the two halves of one row's chunks.
// K and V tiles of 64 keys go through LDS at pitches 528 and 576 (33 792 + 36 864 = 70 656 bytes); the next tile sits in 64 registers
// per thread while this one is multiplied:
//   S^T[key][row] = K.Q^T   32 MFMAs of 32x32x16 (tile_scores, K read as ds_read_b128 rows)
//   online softmax in log2 units over the lane pair, P^T packed as the B operand with no lane movement
//   O^T[d][row] += V^T.P^T  32 MFMAs, V read transposed (ds_read_b64_tr_b16)
// 64 MFMAs per wave and tile, no product computed twice and no exchange between waves -- the 128-row block, not the split-head
// 64-row block of the paged kernel (3.20), which pays an LDS round trip per tile that long sequences do not amortise.
// A wave skips a tile none of its rows sees and runs unmasked where every row sees all of it (3.8).  A row without a visible key
// writes O = 0 and LSE = -inf.  One launch, no workspace: grid = ceil(min(max_seqlen_q, Tq) g / 128) x Hkv x B.
#include "fa_varlen_d256.h"

namespace aule_hip {
namespace {

template <class T>
__global__ void __launch_bounds__(256, 1) fa_fwd_varlen_d256_kernel(const VarlenD256Params p) {
    varlen_d256_fwd_body<T, false>(p, 0.f);   // (the body: fa_varlen_d256.h)
}

}  // namespace

int launch_varlen_d256_fwd(const VarlenArgs& a, hipStream_t stream) {
    if (a.D != kVD || a.sinks != nullptr || !varlen_args_ok(a)) return -1;
    const long long nwg = varlen_fwd_grid(a);   // (the grid rule does not depend on the head dimension)
    if (nwg <= 0) return 0;
    // the kernel counts packed rows in 32 bits
    if (nwg > 0x7fffffffll || ((long long)a.Tq + kPQ) * (a.Hq / a.Hkv) > 0x7fffffffll || a.Tk < 0) return -1;
    const VarlenD256Params p = varlen_d256_params(a);
    return dispatch_16bit(a.dtype, [&](auto t) {
        hipLaunchKernelGGL((fa_fwd_varlen_d256_kernel<decltype(t)>), dim3((unsigned)nwg), dim3(256), 0, stream, p);
        return (int)hipGetLastError();
    });
}

}  // namespace aule_hip
