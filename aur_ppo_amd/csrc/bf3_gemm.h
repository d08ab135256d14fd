// What the bf16x3 GEMM kernels of conv.hip (K11, K11p, K12) and linear.hip (k_linear*, k_linear_wgrad*) share: the k-step product, the
// tile constants, and the host side's choice of NB.  Device pieces are __forceinline__: each including file compiles them in place.
#pragma once
#include <type_traits>

#include "bf16x3.h"

namespace bf3 {

typedef float f32x16c __attribute__((ext_vector_type(16)));

// One k-step of a convolution's product: the six plane products of bf16x3.h summed from ZERO, smallest first, and the step's sum added
// to the running accumulator once.  mma32x3 chains all six through the running accumulator; after a few k-steps that sum is so much
// larger than a third-order product (2^-16 of a term) that the matrix pipe's addition drops it whole: on operands with known positive
// planes K11 and K12 lost 15 % of the third-order terms at a reduction of 288, 87 % at 2304 (tools/conv_plane_bias.py), and the robot
// policy's gradients through them sat at 6 x plain fp32 against an fp64 net.  Here each step's small products meet only
// that step's own a0 * b0, and the accumulator takes one rounded fp32 addition per k-step.
// NEG: the step is computed as -(sum of (-a) * b).  The matrix pipe cuts the bits below its adder's width off TOWARDS MINUS INFINITY,
// whatever the sign of the sum: 5e-9 of the sum of |terms| per output, always negative, which a sum over 10^5 pixels (a bias
// gradient) does not average away.  Every other k-step runs negated, so the cuts of neighbouring steps cancel.
__device__ __forceinline__ Frag3 neg3(const Frag3& a) {
    Frag3 r;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        u32x4 v = __builtin_bit_cast(u32x4, a.p[pl]);
        v = v ^ u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        r.p[pl] = __builtin_bit_cast(bf16x8, v);
    }
    return r;
}
// -DCONV_EXP_NO_ALTERNATE: every k-step with the same sign (a measuring build: tools/conv_plane_bias.py shows the one-sided cut alone)
__device__ __forceinline__ constexpr bool kStepNeg(int k) {
#ifdef CONV_EXP_NO_ALTERNATE
    return false;
#else
    return (k & 1) != 0;
#endif
}
template <bool NEG>
__device__ __forceinline__ f32x16c mma32x3_step(const Frag3& a, const Frag3& b, f32x16c c) {      // NEG: ``a`` comes negated (neg3)
    f32x16c t;
#pragma unroll
    for (int e = 0; e < 16; ++e) t[e] = 0.0f;
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[2], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[2], b.p[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[1], b.p[1], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[1], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[1], b.p[0], t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.p[0], b.p[0], t, 0, 0, 0);
    return NEG ? c - t : c + t;
}
constexpr int kConvThreads = 256;
constexpr int kNBW = 4;              // 32-channel blocks per wave
constexpr int kTileLd = 33;          // floats per row of the epilogue's LDS tile
constexpr int kMB = 2;               // 32-pixel blocks per wave
constexpr int kKC = 2;               // k-steps per staged chunk of the filter

__device__ __forceinline__ int acc_row_c(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }

// LDS-DMA: 16 bytes per lane from global memory straight into LDS at dst + lane * 16 (wave-uniform dst), no registers in between
__device__ __forceinline__ void dma16(const void* src, void* dst_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)dst_wave_uniform, 16, 0, 0);
}

// Host side.  A product of N output channels runs on n_mb (workgroups along M: 4 waves x kMB blocks of 32 rows) x n_ng (groups of NB
// 32-channel blocks) workgroups, NB the largest of 1, 2, 4 that N fills; bf3_with_nb hands that NB to `f` as a std::integral_constant, so the
// caller names its kernel build once:  bf3_with_nb(g.NB, [&](auto nb) { launch k<decltype(nb)::value, ...> }).
struct Bf3Grid {
    long long n_mb;                  // workgroups along M
    int NB, n_ng;
};
inline Bf3Grid bf3_grid(long long M, int N) {
    const int nblk = (N + 31) / 32, NB = nblk >= 4 ? 4 : (nblk >= 2 ? 2 : 1);
    return {(M + 32 * 4 * kMB - 1) / (32 * 4 * kMB), NB, (nblk + NB - 1) / NB};
}
// The small-M tile of the forward linear products (linear_body.h at MB = 1): 4 waves x ONE block of 32 rows, NB of 1 or 2 -- n_mb
// workgroups of 128 rows x n_ng groups of NB blocks, for each of the launch's `nets` same-shaped products (the paired form: 2).
// The NB rule, from measurement (DESIGN 4.12 has the table): 2 where the launch then still has two workgroups for each of the
// chip's 256 CUs, else 1 -- twice the workgroups, each splitting its A values for one column block only.  Below that NB 1 won
// every time (a pair at 4096 x 256: 512 workgroups 40 us per rollout step, 256 workgroups 46; at 1024 rows 31 against 40), from
// 512 NB-2 workgroups on NB 2 was level or ahead (a pair at 4096 x 512: 72 against 76; at 16384 x 256: 95 against 106).
// 4096 rows x 256 columns: one product 32 x 8 = 256 workgroups, a pair 512.  -DLINEAR_SMALL_NB=1|2: a measuring build that takes
// that NB wherever the product has two column blocks.
constexpr long long kSmallFillWgs = 2 * 256;
inline Bf3Grid bf3_small_grid(long long M, int N, int nets) {
    const int nblk = (N + 31) / 32;
    const long long n_mb = (M + 32 * 4 - 1) / (32 * 4);
#ifdef LINEAR_SMALL_NB
    const int NB = nblk >= 2 ? LINEAR_SMALL_NB : 1;
#else
    const int NB = nblk >= 2 && n_mb * ((nblk + 1) / 2) * nets >= kSmallFillWgs ? 2 : 1;
#endif
    return {n_mb, NB, (nblk + NB - 1) / NB};
}
template <class F>
void bf3_with_nb(int NB, F&& f) {
    if (NB == 4) f(std::integral_constant<int, 4>{});
    else if (NB == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}

}  // namespace bf3
