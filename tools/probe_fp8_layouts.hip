// tools/probe_fp8_layouts.hip -- the layouts the FP8 paged prefill rests on: known byte patterns in, tables out.
//   1. v_mfma_scale_f32_32x32x64_f8f6f4, both operands e4m3, both E8M0 scales 127: which (row, column) of D = A.B each (lane, register)
//      holds (expected: column = lane & 31, row = crow(reg, lane >> 5), the rule of every other 32x32 MFMA), and that byte j of lane
//      half h of A multiplies byte j of lane half h of B (the k slots pair up, whatever k they are).
//   2. ds_read_b64_tr_b8: lane l reads the 8 bytes at 8 l of a 512-byte image whose bytes name their source (lane, byte); the table shows
//      which source bytes each lane receives, i.e. the exchange inside a 16-lane group, independent of row pitch (the pitch only enters
//      through the addresses the lanes supply).
//   3. v_perm_b32 4 x 4 byte transpose with the selectors of CodeTile::store, and v_exp_f32(8.0) == 256.
//   4. issue cost: shader cycles per scaled MFMA in a plain loop with the A operand in registers, from two ds_read_b128, from four
//      ds_read_b64_tr_b8; one and two waves per SIMD.
//   hipcc -O3 --offload-arch=gfx950 tools/probe_fp8_layouts.hip -o probe_fp8_layouts && ./probe_fp8_layouts
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ f32x16 mfma8(i32x8 a, i32x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
}
// e4m3 code of (8 + w) / 8 * 2^u for x = 8 u + w < 32: 32 distinct exactly representable values
__host__ __device__ inline unsigned code32(int x) { return (unsigned)(((7 + (x >> 3)) << 3) | (x & 7)); }
inline float value32(int x) { return (8 + (x & 7)) / 8.0f * (float)(1 << (x >> 3)); }

// mode 0: A[i][slot 0] = value32(i), B[slot 0][j] = 1 -> D[i][j] names i.  mode 1: the other way round -> D names j.
// mode 2 + s: A one-hot 1.0 in slot s = 32 h + j of every row, B slot t = code 0x20 + t in every column -> D names the B slot paired with s.
__global__ void k_layout(float* out, int mode) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    i32x8 a = {}, b = {};
    if (mode < 2) {
        const unsigned one = 0x38u;   // 1.0
        if (h == 0) {
            a[0] = (int)(mode == 0 ? code32(r) : one);
            b[0] = (int)(mode == 0 ? one : code32(r));
        }
    } else {
        const int s = mode - 2;
        if (h == (s >> 5)) a[(s & 31) >> 2] = (int)(0x38u << (8 * (s & 3)));
        for (int w = 0; w < 8; ++w) {
            unsigned x = 0;
            for (int e = 0; e < 4; ++e) x |= (0x20u + 32 * h + 4 * w + e) << (8 * e);
            b[w] = (int)x;
        }
    }
    f32x16 c = {};
    c = mfma8(a, b, c);
    for (int i = 0; i < 16; ++i) out[lane * 16 + i] = c[i];
}

__global__ void k_tr8(unsigned char* out, int which) {
    __shared__ __attribute__((aligned(16))) unsigned char img[512];
    const int lane = threadIdx.x;
    for (int e = 0; e < 8; ++e) img[8 * lane + e] = (unsigned char)(which == 0 ? lane : e);
    __syncthreads();
    const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((i32x2 __attribute__((address_space(3)))*)(img + 8 * lane));
    for (int e = 0; e < 8; ++e) out[8 * lane + e] = (unsigned char)(((unsigned)v[e >> 2] >> (8 * (e & 3))) & 255u);
}

__global__ void k_misc(unsigned* out) {
    const unsigned a0 = 0x03020100u, a1 = 0x13121110u, a2 = 0x23222120u, a3 = 0x33323130u;
    const unsigned x01l = __builtin_amdgcn_perm(a1, a0, 0x05010400u), x01h = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
    const unsigned x23l = __builtin_amdgcn_perm(a3, a2, 0x05010400u), x23h = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    out[0] = __builtin_amdgcn_perm(x23l, x01l, 0x05040100u);
    out[1] = __builtin_amdgcn_perm(x23l, x01l, 0x07060302u);
    out[2] = __builtin_amdgcn_perm(x23h, x01h, 0x05040100u);
    out[3] = __builtin_amdgcn_perm(x23h, x01h, 0x07060302u);
    float e = 8.0f + (float)threadIdx.x;   // not a compile-time constant
    out[4] = __builtin_bit_cast(unsigned, __builtin_amdgcn_exp2f(e));
    out[5] = __builtin_bit_cast(unsigned, __builtin_amdgcn_exp2f(e - 8.0f));
}

// KIND 0: operands in registers; 1: A from two ds_read_b128 (row pitch 144); 2: A from four ds_read_b64_tr_b8
template <int KIND, int NT>
__global__ void __launch_bounds__(NT) k_cost(float* out, unsigned long long* cyc, int iters) {
    __shared__ __attribute__((aligned(16))) char smem[32768];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 8192; i += blockDim.x) ((unsigned*)smem)[i] = 0x38383838u;
    __syncthreads();
    f32x16 acc[4] = {};
    i32x8 bq, a;
    for (int j = 0; j < 8; ++j) bq[j] = 0x38383838, a[j] = 0x30303030;
    asm volatile("" : "+v"(bq), "+v"(a));
    const char* kb = smem + (lane & 31) * 144 + (lane >> 5) * 32;
    const char* tb = smem + lane * 8;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if constexpr (KIND == 1) {
                const u32x4 x = *reinterpret_cast<const u32x4*>(kb + (i & 1) * 64 + (i >> 1) * 32 * 144);
                const u32x4 y = *reinterpret_cast<const u32x4*>(kb + (i & 1) * 64 + (i >> 1) * 32 * 144 + 16);
                a = i32x8{(int)x[0], (int)x[1], (int)x[2], (int)x[3], (int)y[0], (int)y[1], (int)y[2], (int)y[3]};
            } else if constexpr (KIND == 2) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const i32x2 v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((i32x2 __attribute__((address_space(3)))*)(tb + 512 * (4 * i + q)));
                    a[2 * q] = v[0];
                    a[2 * q + 1] = v[1];
                }
            }
            acc[i & 3] = mfma8(a, bq, acc[i & 3]);
        }
        if constexpr (KIND == 0) asm volatile("" : "+v"(a));
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    float s = 0.f;
    for (int d = 0; d < 4; ++d)
        for (int r = 0; r < 16; ++r) s += acc[d][r];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <int KIND, int NT>
static void cost(const char* name, float* out, unsigned long long* cyc) {
    const int iters = 2000;
    for (int rep = 0; rep < 2; ++rep) {
        hipLaunchKernelGGL((k_cost<KIND, NT>), dim3(256), dim3(NT), 0, 0, out, cyc, iters);
        if (hipDeviceSynchronize() != hipSuccess) { printf("cost %s: launch failed\n", name); return; }
    }
    unsigned long long c = 0;
    (void)hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost);
    printf("%-22s %d waves/SIMD: %6.1f s_memtime ticks per MFMA (wave 0, %d MFMAs)\n", name, NT / 256, (double)c / (8.0 * iters), 8 * iters);
}

static inline int crow(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

int main() {
    float* out;
    unsigned long long* cyc;
    (void)hipMalloc(&out, 256 * 512 * 4);
    (void)hipMalloc(&cyc, 64);
    static float h[2][1024];
    for (int mode = 0; mode < 2; ++mode) {
        hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, out, mode);
        if (hipDeviceSynchronize() != hipSuccess) { printf("layout launch failed\n"); return 1; }
        (void)hipMemcpy(h[mode], out, 4096, hipMemcpyDeviceToHost);
    }
    int bad = 0;
    printf("== 1. C/D layout of v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, scales 127): (row, col) held by lane, register\n");
    for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 16; ++r) {
            int row = -1, col = -1;
            for (int x = 0; x < 32; ++x) {
                if (h[0][lane * 16 + r] == value32(x)) row = x;
                if (h[1][lane * 16 + r] == value32(x)) col = x;
            }
            if (row != crow(r, lane >> 5) || col != (lane & 31)) ++bad;
            if (lane == 0 || lane == 1 || lane == 32 || lane == 63) printf("  lane %2d reg %2d: row %2d col %2d\n", lane, r, row, col);
        }
    printf("  entries that differ from row = crow(reg, lane >> 5), col = lane & 31: %d of 1024\n", bad);
    int badk = 0;
    for (int s = 0; s < 64; ++s) {
        hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, out, 2 + s);
        (void)hipDeviceSynchronize();
        float v;
        (void)hipMemcpy(&v, out, 4, hipMemcpyDeviceToHost);
        // value of e4m3 code 0x20 + s
        const int code = 0x20 + s, ex = code >> 3, ma = code & 7;
        const float want = ldexpf(1.0f + ma / 8.0f, ex - 7);
        if (v != want) { ++badk; printf("  A slot %2d (half %d byte %2d): D = %g, B's slot %2d holds %g\n", s, s >> 5, s & 31, v, s, want); }
    }
    printf("  A slots (half, byte) that do not pair with the same slot of B: %d of 64\n", badk);

    printf("== 2. ds_read_b64_tr_b8: lane l supplies address 8 l; received bytes as source lane.byte\n");
    unsigned char* ob;
    (void)hipMalloc(&ob, 512);
    static unsigned char t8[2][512];
    for (int w = 0; w < 2; ++w) {
        hipLaunchKernelGGL(k_tr8, dim3(1), dim3(64), 0, 0, ob, w);
        if (hipDeviceSynchronize() != hipSuccess) { printf("tr8 launch failed\n"); return 1; }
        (void)hipMemcpy(t8[w], ob, 512, hipMemcpyDeviceToHost);
    }
    int badg = 0;
    for (int lane = 0; lane < 64; ++lane) {
        if (lane < 16) printf("  lane %2d:", lane);
        for (int e = 0; e < 8; ++e) {
            if (lane < 16) printf(" %2d.%d", t8[0][8 * lane + e], t8[1][8 * lane + e]);
            if (t8[0][8 * lane + e] != t8[0][8 * (lane & 15) + e] + 16 * (lane >> 4) || t8[1][8 * lane + e] != t8[1][8 * (lane & 15) + e]) ++badg;
        }
        if (lane < 16) printf("\n");
    }
    printf("  bytes of lanes 16 .. 63 that do not repeat group 0's pattern inside their own 16-lane group: %d\n", badg);

    printf("== 3. v_perm_b32 transpose, v_exp_f32\n");
    unsigned* om;
    unsigned hm[6];
    (void)hipMalloc(&om, 64);
    hipLaunchKernelGGL(k_misc, dim3(1), dim3(1), 0, 0, om);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(hm, om, 24, hipMemcpyDeviceToHost);
    printf("  rows 03020100 13121110 23222120 33323130 -> %08x %08x %08x %08x (want 30201000 31211101 32221202 33231303)\n", hm[0], hm[1], hm[2], hm[3]);
    float e8, e0;
    memcpy(&e8, &hm[4], 4);
    memcpy(&e0, &hm[5], 4);
    printf("  v_exp_f32(8) = %.9g, v_exp_f32(0) = %.9g\n", e8, e0);

    printf("== 4. issue cost\n");
    cost<0, 256>("registers", out, cyc);
    cost<1, 256>("2 x ds_read_b128", out, cyc);
    cost<2, 256>("4 x ds_read_b64_tr_b8", out, cyc);
    cost<0, 512>("registers", out, cyc);
    cost<1, 512>("2 x ds_read_b128", out, cyc);
    cost<2, 512>("4 x ds_read_b64_tr_b8", out, cyc);
    return 0;
}
