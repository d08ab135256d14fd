// The rollout forward of the 2 x 64 policy: the LDS plan of K8 (k_mlp_act, mlp.hip: one step) and K16 (k_cartpole_rollout,
// cartpole.hip: T steps of a device CartPole in one launch), and the staging of both nets' weights and the three-layer forward as K16
// runs them.  K8 forms its pointers from the plan's offsets and takes its byte count from it, but keeps a text of its own for the
// staging and the layers, for the measured reason given above it.  K16's contract is that it leaves, bit for bit, what T x (K8, K15)
// leave.
#pragma once
#include "mlp_common.h"

namespace aurppo_mlp {

// The plan of the dynamic LDS: ONE table of float counts, from which every pointer (K16: the members below; K8: lds + at(k...)) and
// both launches' byte counts are formed, so a member cannot be added to the plan without its bytes.  The log-std rows come last: a
// kernel with no Gaussian head (K16) asks for bytes(false) and never touches sLs / sSd; K8 asks for bytes(true).
struct ActLds {
    enum Member { kX, kH1, kH2, kW1, kW2, kW3, kOut, kB1, kB2, kB3, kLs, kSd, kMembers };
    // floats in front of member m (m == kMembers: the whole plan)
    static constexpr size_t at(int m) {
        constexpr int n[kMembers] = {
            R * LD,          // sX   [R][LD]
            2 * R * LD,      // sH1  [2][R][LD]
            2 * R * LD,      // sH2  [2][R][LD]
            2 * H * LD,      // sW1  [2][H][LD]
            2 * H * LD,      // sW2  [2][H][LD]
            2 * AP * LD,     // sW3  [2][AP][LD]
            2 * R * LDO,     // sOut [2][R][LDO]
            2 * H,           // sB1  [2][H]
            2 * H,           // sB2  [2][H]
            2 * AP,          // sB3  [2][AP]
            AP,              // sLs  [AP] log-std
            AP,              // sSd  [AP] exp(log-std)
        };
        size_t o = 0;
        for (int i = 0; i < m; ++i) o += n[i];
        return o;
    }
    static constexpr size_t bytes(bool with_logstd) { return sizeof(float) * at(with_logstd ? kMembers : kLs); }

    float *sX, *sH1, *sH2, *sW1, *sW2, *sW3, *sOut, *sB1, *sB2, *sB3, *sLs, *sSd;
    __device__ __forceinline__ explicit ActLds(float* base)
        : sX(base + at(kX)), sH1(base + at(kH1)), sH2(base + at(kH2)), sW1(base + at(kW1)), sW2(base + at(kW2)), sW3(base + at(kW3)),
          sOut(base + at(kOut)), sB1(base + at(kB1)), sB2(base + at(kB2)), sB3(base + at(kB3)), sLs(base + at(kLs)), sSd(base + at(kSd)) {}
};
static_assert(ActLds::bytes(true) == 122112 && ActLds::bytes(false) == 121984, "the LDS plan of K8 / K16 has changed size");

// Net n's (0 actor, 1 critic) W1 / W2 / W3 / b1 / b2 / b3 into LDS, zero beyond D columns and beyond the head's outputs (A, or the
// critic's one).  Every element's address comes from shifts of a flat index over rows padded to 64 columns (no division, no zero-fill
// pass), and all of a thread's loads are independent, so they go out together -- K8 is a latency chain (launch, staging, three layers,
// sampling) and this was its longest link; K16 pays it once per launch.
// The loop over the two nets is the caller's, `#pragma unroll for (n = 0; n < 2; ++n) act_stage_weights(..., n)`: with the loop in
// here K16's listing loaded its whole argument block at entry and sgpr_spill_count rose from 4 to 12 (profiles/
// refactor_act_forward.txt, section 2, with what is supposed to cause it).
__device__ __forceinline__ void act_stage_weights(const ActLds& s, const float* params, const MlpLayout& L, int D, int A, int n) {
    const int out_dim = n == 0 ? A : 1;
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < H * H / kThreads; ++u) {
        const int e = tid + u * kThreads, o = e >> 6, c = e & 63;
        // branch-free: a padding lane reads a clamped (valid) element and masks it -- a load under a divergent
        // condition makes the compiler wait for everything in flight
        const float w1v = params[L.w1[n] + o * D + (c < D ? c : D - 1)];
        const float w2v = params[L.w2[n] + e];
        s.sW1[(n * H + o) * LD + c] = c < D ? w1v : 0.0f;
        s.sW2[(n * H + o) * LD + c] = w2v;
    }
#pragma unroll
    for (int u = 0; u < AP * H / kThreads; ++u) {
        const int e = tid + u * kThreads, o = e >> 6, i = e & 63;
        s.sW3[(n * AP + o) * LD + i] = o < out_dim ? params[L.w3[n] + o * H + i] : 0.0f;
    }
    if (tid < H) {
        s.sB1[n * H + tid] = params[L.b1[n] + tid];
        s.sB2[n * H + tid] = params[L.b2[n] + tid];
    }
    if (tid < AP) s.sB3[n * AP + tid] = tid < out_dim ? params[L.b3[n] + tid] : 0.0f;
}

// The Gaussian head's log-std rows, as K8 fills them: sLs = log-std (0 beyond A, and for a Categorical head), sSd = exp(sLs).  For
// kernels that asked for bytes(true).
__device__ __forceinline__ void act_stage_logstd(const ActLds& s, const float* params, const MlpLayout& L, int A, bool continuous) {
    const int tid = threadIdx.x;
    if (tid < AP) {
        const float ls = (continuous && tid < A) ? params[L.logstd + tid] : 0.0f;
        s.sLs[tid] = ls;
        s.sSd[tid] = expf(ls);
    }
}

// The three layers of this wave's (net, column block) on the tile in sX, a barrier behind each: sH1 = tanh(sX W1' + b1), sH2 =
// tanh(sH1 W2' + b2), sOut = sH2 W3' + b3 (rows 0 .. R of sOut the actor's head, R .. 2R the critic's).  The barrier in FRONT of
// layer 1 -- behind whatever filled sX -- is the caller's.
__device__ __forceinline__ void act_forward(const ActLds& s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int net = wave >> 1, cb = wave & 1;
    {
        f32x16 acc = zero16();
        const float* W = s.sW1 + (net * H + cb * 32) * LD;
        const float* X = s.sX;
        mma32<H>(acc, [&](int i, int k) { return X[i * LD + k]; }, [&](int k, int j) { return W[j * LD + k]; });
        const int col = cb * 32 + (lane & 31);
        const float bias = s.sB1[net * H + col];
#pragma unroll
        for (int e = 0; e < 16; ++e) s.sH1[(net * R + acc_row(e, lane)) * LD + col] = tanh_fast(acc[e] + bias);
    }
    __syncthreads();
    {
        f32x16 acc = zero16();
        const float* W = s.sW2 + (net * H + cb * 32) * LD;
        const float* Hin = s.sH1 + net * R * LD;
        mma32<H>(acc, [&](int i, int k) { return Hin[i * LD + k]; }, [&](int k, int j) { return W[j * LD + k]; });
        const int col = cb * 32 + (lane & 31);
        const float bias = s.sB2[net * H + col];
#pragma unroll
        for (int e = 0; e < 16; ++e) s.sH2[(net * R + acc_row(e, lane)) * LD + col] = tanh_fast(acc[e] + bias);
    }
    __syncthreads();
    {
        const float* W = s.sW3 + net * AP * LD;
        const float* Hin = s.sH2 + (net * R + cb * 16) * LD;
        const f32x4 acc = mma16<H>([&](int i, int k) { return Hin[i * LD + k]; },
                                   [&](int k, int j) { return W[j * LD + k]; });
        const int col = lane & 15;
        const float bias = s.sB3[net * AP + col];
#pragma unroll
        for (int e = 0; e < 4; ++e) s.sOut[(net * R + cb * 16 + 4 * (lane >> 4) + e) * LDO + col] = acc[e] + bias;
    }
    __syncthreads();
}

}  // namespace aurppo_mlp
