// What the bf16-plane step kernels (k_mlp_step3 in mlp3.hip, k_mlpw3_step in mlp_wide3.hip) share beyond bf16x3.h: the two epilogues
// that write a 32x32 accumulator block into an F image.  PL = bytes per plane of that image (64 features: bf3::kFPlane; K7w's 128).
// Both includers say `#pragma clang fp contract(fast)` in front of their includes, and this code is written for that mode.
#pragma once
#include "bf16x3.h"
#include "mlp_common.h"

namespace aurppo_mlp {

// Epilogues, four values (one 8-byte store per plane) at a time so that nothing but the accumulator is live across them.
// tanh(acc + bias) of a 32x32 block into an F image:
// om[e] = 1 - tanh^2 of the same element, kept in registers for the backward pass (dz_from_regs): re-read from the image's planes it
// cost three unpacks and two adds per value to join and twelve LDS reads per block (the register file has had room for the 2 x 16
// values since the fragment addresses stopped being re-derived, bf16x3.h)
template <int PL = bf3::kFPlane>
__device__ __forceinline__ void tanh_store(char* img, int f0, const f32x16& acc, float bias, int lane, float (&om)[16]) {
    const int f = f0 + (lane & 31), h = lane >> 5;
    const float bc = bias * kTanhC;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        unsigned a0, a1, a2, b0, b1, b2;
        const float t0 = tanh_fast_fma(acc[4 * gq + 0], bc), t1 = tanh_fast_fma(acc[4 * gq + 1], bc);
        const float t2 = tanh_fast_fma(acc[4 * gq + 2], bc), t3 = tanh_fast_fma(acc[4 * gq + 3], bc);
        om[4 * gq + 0] = 1.0f - t0 * t0; om[4 * gq + 1] = 1.0f - t1 * t1;
        om[4 * gq + 2] = 1.0f - t2 * t2; om[4 * gq + 3] = 1.0f - t3 * t3;
        bf3::split3(t0, t1, a0, a1, a2);
        bf3::split3(t2, t3, b0, b1, b2);
        const int o = bf3::foff(f, 4 * h) ^ (gq << 4);       // = foff(f, 8 gq + 4 h)
        *reinterpret_cast<bf3::u32x2*>(img + 0 * PL + o) = bf3::u32x2{a0, b0};
        *reinterpret_cast<bf3::u32x2*>(img + 1 * PL + o) = bf3::u32x2{a1, b1};
        *reinterpret_cast<bf3::u32x2*>(img + 2 * PL + o) = bf3::u32x2{a2, b2};
    }
}
// dZ = dH * (1 - h^2), (1 - h^2) from the forward pass's registers, written over the block of h in the image; returns the lane's column sum
template <int PL = bf3::kFPlane>
__device__ __forceinline__ float dz_from_regs(char* img, int f0, const f32x16& dh, const float (&om)[16], int lane) {
    const int f = f0 + (lane & 31), h = lane >> 5;
    float colsum = 0.0f;
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const float d0 = dh[4 * gq + 0] * om[4 * gq + 0], d1 = dh[4 * gq + 1] * om[4 * gq + 1];
        const float d2 = dh[4 * gq + 2] * om[4 * gq + 2], d3 = dh[4 * gq + 3] * om[4 * gq + 3];
        colsum += (d0 + d1) + (d2 + d3);
        unsigned a0, a1, a2, b0, b1, b2;
        bf3::split3(d0, d1, a0, a1, a2);
        bf3::split3(d2, d3, b0, b1, b2);
        const int o = bf3::foff(f, 4 * h) ^ (gq << 4);       // = foff(f, 8 gq + 4 h)
        *reinterpret_cast<bf3::u32x2*>(img + 0 * PL + o) = bf3::u32x2{a0, b0};
        *reinterpret_cast<bf3::u32x2*>(img + 1 * PL + o) = bf3::u32x2{a1, b1};
        *reinterpret_cast<bf3::u32x2*>(img + 2 * PL + o) = bf3::u32x2{a2, b2};
    }
    return colsum;
}

}  // namespace aurppo_mlp
