// K13: the heads of the MLP actor-critic, the action distribution, the PPO loss and their backward pass in one kernel -- the
// part of a minibatch step (src/ppo.py:219-266) that sits between the last hidden layer of src/nets/nets.py:19-53 and the
// loss, for the policies the fused steps K7 / K7w do not cover (hidden_dim > 128 or more than 128 state floats), whose
// hidden layers run a layer at a time on k_linear / k_linear_wgrad (linear.hip).  It replaces, per minibatch: the two head
// GEMMs (A and 1 columns), the Normal / Categorical log-prob and entropy (a dozen element-wise kernels), K4 + K5, and
// autograd's backward of all of them down to the pre-activation of the last hidden layer.
//
// Memory bound (0.5 GB for 1.4 GFLOP at H = 256, M = 131 072), so: plain fp32 FMAs, no matrix pipe.
//   * a row's H activations lie along TPR = pow2(H / 4) threads, 4 columns (one 16-byte load) each; a workgroup of 256 threads
//     works on 256 / TPR rows at a time.  The (A + 1) x H head weights sit in LDS.  The A + 1 dot products of a row finish with
//     a butterfly over the row's lanes (and, for TPR > 64, a fixed-order sum over its waves through LDS), which leaves the same
//     bits in every lane: each lane then forms the row's loss terms itself (ppo_sample, ppo_math.h) -- no broadcast.
//   * log-prob as torch forms it: -(z * z) / (2 * std * std) - logstd - log sqrt(2 pi), one division per element; the
//     Categorical head through max-subtracted exponentials.
//   * backward: gz = (d head . W) * (1 - h * h) is stored (gz may alias h: a thread reads its four h before it writes them);
//     head weight / bias / logstd gradients and the column sums of gz (the last hidden layer's bias gradients) accumulate in
//     registers over the rows of a thread, are summed over the workgroup's row groups in group order, and leave as one slab
//     per workgroup.  k_head_fold sums the slabs in workgroup order (fp64 accumulator, rounded once) into the bucket's
//     gradient and folds the nine scalars.  The grid depends on (M, H) only: two launches on the same inputs give the same bits.
// K14 (k_head_act, below K13's host helpers) is the forward half alone for the rollout step: same layout, same head expressions in the
// same order, then sampling -- so the log-prob it stores is the one K13 forms from the stored action.  One dispatcher by threads per
// row launches either kernel (launch_k_head_ppo / launch_k_head_act), one function checks a layout's bounds, one fills K14's arguments.
// The layered rollout and update steps that run these kernels behind linear.hip's products are host code of their own: layered.hip.
#include "mlp_common.h"

namespace {

constexpr int kHT = 256;             // threads per workgroup
constexpr int kHeadMaxGrid = 512;
constexpr int kHeadStat = 64;        // statistics workgroups (at most)
// NA: the length of a head kernel's per-action register arrays, 16 for A <= 16 and 32 for A in 17 .. 32.  The critic's product sits in
// slot p[NA]; s_small and the slab tail are 3 NA floats: d b_actor [NA], d logstd [NA], d b_critic [1] + padding.
constexpr int kHeadMaxA = 32;
__host__ __device__ constexpr int head_na(int A) { return A > 16 ? 32 : 16; }
__host__ __device__ constexpr int head_small(int NA) { return 3 * NA; }
// The accumulator of a Gaussian head's log-prob, a sum of A fp32 terms of one sign: fp32, added in order, up to 16 actions.  At 17 .. 32
// that order's rounding is twice that of a tree sum at the same width and lifts the actor's gradients to 2.05 - 2.08 x the fp32 yardstick
// (tests/test_layered_actions_fp64_gpu.py: the per-sample ratio exp(logp - old_logp) carries it into every one of them), so NA = 32 adds
// the same fp32 terms in fp64 and rounds once.  K13 and K14 share the type: the log-prob K14 stores stays the one K13 forms.
template <int NA>
using HeadLogpAcc = std::conditional_t<(NA > 16), double, float>;

struct HeadArgs {
    const float* hA;                 // (M, H) last hidden activations, minibatch order
    const float* hC;
    float* gzA;                      // (M, H) d loss / d pre-activation of the last hidden layer (may be hA / hC)
    float* gzC;
    const float* actions;            // (B, aw) or nullptr (packed records)
    const float4* rec;               // (B, 4) {old_logp, adv, ret, old_v}; packed: (B, 16), the action row in floats 4..15
    int rec_stride;                  // float4s per record: 1 or 4
    int aw;                          // action floats per sample
    const int32_t* idx;              // (M,)
    const float* params;
    int off_wa, off_ba, off_wc, off_bc, off_ls, off_bla, off_blc;
    double (*stats)[2];              // (n_stat, 2)
    int n_stat;
    float* slabs;                    // (grid, slab_stride)
    double* loss_part;               // (grid, 8)
    int slab_stride;
    int M, H, A, continuous, n_iter;
    int Hr;                          // floats of a head row in the bucket: H, or fewer (the layered steps at a hidden width that is no
                                     // multiple of 32: H is the width rounded up, the activations' columns >= Hr are zeros)
    PpoHyper h;
};

__host__ __device__ constexpr int head_slab_floats(int H, int A) { return (A + 3) * H + head_small(head_na(A)); }

__global__ __launch_bounds__(kHT) void k_head_stats(const float4* __restrict__ rec, int rec_stride, const int32_t* __restrict__ idx, int M,
                                                    double (*__restrict__ stats)[2]) {
    __shared__ double sc[2][kHT / kWave];
    double s = 0.0, q = 0.0;
    aurppo_mlp::adv_partial_sums(rec, rec_stride, idx, M, blockIdx.x * kHT + threadIdx.x, gridDim.x * kHT, s, q);
    const double bs = block_sum<kHT / kWave>(s, sc[0]);
    const double bq = block_sum<kHT / kWave>(q, sc[1]);
    if (threadIdx.x == 0) {
        stats[blockIdx.x][0] = bs;
        stats[blockIdx.x][1] = bq;
    }
}

// mean / std of the minibatch's advantages from the partial sums: the same order, so the same bits, in every workgroup of both kernels
__device__ __forceinline__ void head_fold_stats(const double (*stats)[2], int n_stat, int M, double (*sc)[kHT / kWave], float* s_ms) {
    double s = 0.0, q = 0.0;
    for (int b = threadIdx.x; b < n_stat; b += kHT) {
        s += stats[b][0];
        q += stats[b][1];
    }
    const double ts = block_sum<kHT / kWave>(s, sc[0]);
    const double tq = block_sum<kHT / kWave>(q, sc[1]);
    if (threadIdx.x == 0) adv_mean_std(ts, tq, M, s_ms[0], s_ms[1]);
    __syncthreads();
}

__device__ __forceinline__ float dot4(const float4 a, const float4 b) {
    return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)));
}
__device__ __forceinline__ void fma4(float4& acc, float s, const float4 v) {
    acc.x = __builtin_fmaf(s, v.x, acc.x);
    acc.y = __builtin_fmaf(s, v.y, acc.y);
    acc.z = __builtin_fmaf(s, v.z, acc.z);
    acc.w = __builtin_fmaf(s, v.w, acc.w);
}

// The forward half (staging, thread geometry, dot4 products, butterfly, in-order sum over a row's waves, Categorical opening) stays
// written out in both k_head_ppo and k_head_act.  As shared __forceinline__ pieces called by both it kept every bit (build_bitdiff:
// identical) but was taken out again: k_head_ppo with a Categorical head ran 1528 -> 1547 us at H = 512 and 3061 -> 3081 us at
// H = 1024 (M = 131072), above the two-copy build in every one of four alternating rounds, and no single piece carried it
// (profiles/refactor_head_rollout.txt, section 5).  tests/test_layered_act_fp64_gpu.py and tools/build_bitdiff.py hold the two copies
// to the same bits.
//
// NA = 32 (A in 17 .. 32) is the same text with longer arrays, and two savings of registers that NA = 16 does not take (kLean): the
// logstd gradient of a row goes into dls[k] where it is formed (no dlr[]), and an action is read from its row where it is used, in both
// loops, instead of a copy of the row held across the reductions (no actv[]).  Both leave every sum's terms and order as they are.  The
// Gaussian log-prob alone is summed differently at NA = 32 (HeadLogpAcc).
template <int TPR, int NA>      // threads per row: the power of two >= H / 4, 8 ... 256; per-action array length: 16 | 32
__global__ __launch_bounds__(kHT) void k_head_ppo(const HeadArgs a) {
    constexpr int GPW = kHT / TPR;                     // rows a workgroup works on at a time
    constexpr int NWG = TPR > kWave ? TPR / kWave : 1;   // waves per row
    constexpr int LW = TPR > kWave ? kWave : TPR;      // lanes of a wave on one row
    constexpr int kSmall = head_small(NA);
    constexpr bool kLean = NA > 16;
    extern __shared__ __attribute__((aligned(16))) float sW[];       // (A + 1, H): actor head rows, then the critic's
    __shared__ __attribute__((aligned(16))) float s_red[kHT * 4];
    __shared__ float s_small[kSmall];                  // b_actor [NA], logstd [NA], std * std [NA]
    __shared__ float s_part[2][kHT / kWave][NA + 4];
    __shared__ float s_sm[32][kSmall];
    __shared__ double s_loss[32][6];
    __shared__ double s_dred[2][kHT / kWave];
    __shared__ float s_ms[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, A = a.A;
    head_fold_stats(a.stats, a.n_stat, a.h.M, s_dred, s_ms);
    if (a.Hr == H) {
        for (int e = tid; e < (A + 1) * H; e += kHT) sW[e] = e < A * H ? a.params[a.off_wa + e] : a.params[a.off_wc + (e - A * H)];
    } else {                                           // head rows of Hr floats: zero columns from Hr on, and no read behind a row's end
        for (int k = 0; k <= A; ++k) {
            const float* const src = k < A ? a.params + a.off_wa + (size_t)k * a.Hr : a.params + a.off_wc;
            for (int c = tid; c < H; c += kHT) sW[k * H + c] = c < a.Hr ? src[c] : 0.0f;
        }
    }
    if (tid < NA) {
        s_small[tid] = tid < A ? a.params[a.off_ba + tid] : 0.0f;
        const float ls = (a.continuous && tid < A) ? a.params[a.off_ls + tid] : 0.0f;
        const float sd = expf(ls);
        s_small[NA + tid] = ls;
        s_small[2 * NA + tid] = sd * sd;
    }
    __syncthreads();
    const float mean = s_ms[0], denom = s_ms[1] + 1e-8f;
    const float invM = 1.0f / (float)a.h.M;
    const float g_ent = -a.h.ent_coef * invM;
    const float bc = a.params[a.off_bc];

    const int g = tid / TPR, t = tid % TPR;
    const int c0 = 4 * t;
    const bool colok = c0 < H;
    const int cw = colok ? c0 : 0;
    const int G = (int)gridDim.x * GPW, gg = (int)blockIdx.x * GPW + g;
    const float4 wc = *reinterpret_cast<const float4*>(sW + A * H + cw);
    const float4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    float4 dWa[NA], dWc = zero4, dblA = zero4, dblC = zero4;
    float dba[NA], dls[NA], dbc = 0.0f;
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        dWa[k] = zero4;
        dba[k] = dls[k] = 0.0f;
    }
    double l_pg = 0.0, l_vl = 0.0, l_ent = 0.0, l_okl = 0.0, l_kl = 0.0, l_cf = 0.0;

    float4 na = zero4, nc = zero4;
    int nsrc = 0;
    auto fetch = [&](long long row) {
        na = nc = zero4;
        nsrc = 0;
        if (row < a.M) {
            nsrc = a.idx[row];
            if (colok) {
                na = *reinterpret_cast<const float4*>(a.hA + (size_t)row * H + c0);
                nc = *reinterpret_cast<const float4*>(a.hC + (size_t)row * H + c0);
            }
        }
    };
    fetch(gg);
    for (int it = 0; it < a.n_iter; ++it) {
        const long long row = (long long)it * G + gg;
        const bool valid = row < a.M;
        const float4 ha = na, hc = nc;
        const int src = nsrc;
        // this row's record and action row: asked for here, used behind the dot products
        float4 rc = zero4;
        float actv[NA];
        const float* ap = nullptr;
        if constexpr (!kLean) {
#pragma unroll
            for (int k = 0; k < NA; ++k) actv[k] = 0.0f;
        }
        if (valid) {
            rc = a.rec[(size_t)src * a.rec_stride];
            ap = a.actions ? a.actions + (size_t)src * a.aw : reinterpret_cast<const float*>(a.rec) + (size_t)src * 16 + 4;
            if constexpr (!kLean) {
#pragma unroll
                for (int k = 0; k < NA; ++k)
                    if (k < a.aw) actv[k] = ap[k];
            }
        }
        fetch(row + G);

        float p[NA + 1];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            p[k] = 0.0f;
            if (k < A) p[k] = dot4(ha, *reinterpret_cast<const float4*>(sW + k * H + cw));
        }
        p[NA] = dot4(hc, wc);
#pragma unroll
        for (int k = 0; k < NA + 1; ++k) {
            if (k < A || k == NA) {
#pragma unroll
                for (int off = LW / 2; off > 0; off >>= 1) p[k] += __shfl_xor(p[k], off, kWave);
            }
        }
        if (NWG > 1) {
            float* const mine = s_part[it & 1][wave];
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < NA + 1; ++k)
                    if (k < A || k == NA) mine[k] = p[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NA + 1; ++k) {
                if (k < A || k == NA) {
                    float s = 0.0f;
#pragma unroll
                    for (int w = 0; w < NWG; ++w) s += s_part[it & 1][g * NWG + w][k];
                    p[k] = s;
                }
            }
        }
        // ---- the row's loss terms (every lane of the row forms the same bits); p[k] becomes d loss / d head output k
        float dv = 0.0f;
        float dlr[NA];
        if constexpr (!kLean) {
#pragma unroll
            for (int k = 0; k < NA; ++k) dlr[k] = 0.0f;
        }
        if (valid) {
            const float v_new = p[NA] + bc;
            PpoSample ts;
            if (a.continuous) {
                HeadLogpAcc<NA> logp = 0.0f;
                float ent = 0.0f;
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    if (k < A) {
                        const float ls = s_small[NA + k], var = s_small[2 * NA + k];
                        const float z = (kLean ? ap[k] : actv[k]) - (p[k] + s_small[k]);
                        logp += gauss_logp_var(z, var, ls);
                        ent += gauss_ent(ls);
                    }
                }
                ts = ppo_sample((float)logp, rc.x, rc.y, v_new, rc.w, rc.z, mean, denom, invM, a.h);
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    if (k < A) {
                        const float var = s_small[2 * NA + k];
                        const float z = (kLean ? ap[k] : actv[k]) - (p[k] + s_small[k]);
                        p[k] = gauss_dmu_var(ts.g_logp, z, var);
                        if constexpr (kLean) dls[k] += gauss_dls_var(ts.g_logp, z, var, g_ent);
                        else dlr[k] = gauss_dls_var(ts.g_logp, z, var, g_ent);
                    }
                }
                l_ent += (double)ent;
            } else {
                float mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    if (k < A) {
                        p[k] += s_small[k];
                        mx = fmaxf(mx, p[k]);
                    }
                }
                float se = 0.0f;
#pragma unroll
                for (int k = 0; k < NA; ++k)
                    if (k < A) se += expf(p[k] - mx);
                const float lse = mx + logf(se);
                const int ai = (int)(kLean ? ap[0] : actv[0]);
                float logp = 0.0f, ent = 0.0f;
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    if (k < A) {
                        const float lpk = p[k] - lse;
                        ent -= expf(lpk) * lpk;
                        if (k == ai) logp = lpk;
                    }
                }
                ts = ppo_sample(logp, rc.x, rc.y, v_new, rc.w, rc.z, mean, denom, invM, a.h);
#pragma unroll
                for (int k = 0; k < NA; ++k) {
                    if (k < A) {
                        const float lpk = p[k] - lse;
                        const float pk = expf(lpk);
                        p[k] = cat_dlogit(ts.g_logp, k == ai, pk, lpk, ent, g_ent);
                    }
                }
                l_ent += (double)ent;
            }
            dv = ts.g_v;
            l_pg += (double)ts.pg;
            l_vl += (double)ts.vl;
            l_okl += (double)ts.okl;
            l_kl += (double)ts.kl;
            l_cf += (double)ts.cf;
        } else {
#pragma unroll
            for (int k = 0; k < NA; ++k) p[k] = 0.0f;
        }
        // ---- backward: gz of both nets for this thread's four columns, the register accumulators
        float4 ga = zero4;
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            if (k < A) {
                fma4(ga, p[k], *reinterpret_cast<const float4*>(sW + k * H + cw));
                fma4(dWa[k], p[k], ha);
                dba[k] += p[k];
                if constexpr (!kLean) dls[k] += dlr[k];
            }
        }
        const float4 gza = {ga.x * (1.0f - ha.x * ha.x), ga.y * (1.0f - ha.y * ha.y), ga.z * (1.0f - ha.z * ha.z), ga.w * (1.0f - ha.w * ha.w)};
        const float4 gzc = {(dv * wc.x) * (1.0f - hc.x * hc.x), (dv * wc.y) * (1.0f - hc.y * hc.y), (dv * wc.z) * (1.0f - hc.z * hc.z),
                            (dv * wc.w) * (1.0f - hc.w * hc.w)};
        if (valid && colok) {
            *reinterpret_cast<float4*>(a.gzA + (size_t)row * H + c0) = gza;
            *reinterpret_cast<float4*>(a.gzC + (size_t)row * H + c0) = gzc;
            fma4(dWc, dv, hc);
            dblA.x += gza.x; dblA.y += gza.y; dblA.z += gza.z; dblA.w += gza.w;
            dblC.x += gzc.x; dblC.y += gzc.y; dblC.z += gzc.z; dblC.w += gzc.w;
        }
        dbc += dv;
    }

    // ---- hand over: the workgroup's row groups summed in group order, one slab per workgroup
    float* const slab = a.slabs + (size_t)blockIdx.x * a.slab_stride;
    auto emit = [&](const float4 v, int slab_off) {
        __syncthreads();
        reinterpret_cast<float4*>(s_red)[tid] = v;
        __syncthreads();
        if (g == 0 && colok) {
            float4 s = reinterpret_cast<const float4*>(s_red)[t];
#pragma unroll
            for (int q = 1; q < GPW; ++q) {
                const float4 o = reinterpret_cast<const float4*>(s_red)[q * TPR + t];
                s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
            }
            *reinterpret_cast<float4*>(slab + slab_off + c0) = s;
        }
    };
#pragma unroll
    for (int k = 0; k < NA; ++k)
        if (k < A) emit(dWa[k], k * H);
    emit(dWc, A * H);
    emit(dblA, (A + 1) * H);
    emit(dblC, (A + 2) * H);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            s_sm[g][k] = dba[k];
            s_sm[g][NA + k] = dls[k];
            s_sm[g][2 * NA + k] = k == 0 ? dbc : 0.0f;
        }
        s_loss[g][0] = l_pg; s_loss[g][1] = l_vl; s_loss[g][2] = l_ent; s_loss[g][3] = l_okl; s_loss[g][4] = l_kl; s_loss[g][5] = l_cf;
    }
    __syncthreads();
    if (tid < kSmall) {
        float s = 0.0f;
        for (int q = 0; q < GPW; ++q) s += s_sm[q][tid];
        slab[(A + 3) * H + tid] = s;
    }
    if (tid >= 64 && tid < 70) {
        double s = 0.0;
        for (int q = 0; q < GPW; ++q) s += s_loss[q][tid - 64];
        a.loss_part[(size_t)blockIdx.x * 8 + (tid - 64)] = s;
    }
}

// grads[...] = the slabs summed in workgroup order (eight runs of consecutive slabs, each summed in order in fp64, then the eight
// in order; rounded once); the workgroup past the last folds the loss sums into the nine scalars (k_loss_final's arithmetic).
// NA: the slab tail's layout, the one the k_head_ppo build that wrote the slabs used.
__global__ __launch_bounds__(kHT) void k_head_fold(const HeadArgs a, int n_slabs, int NA, float* __restrict__ grads, float* __restrict__ out) {
    __shared__ double s_run[8][32];
    __shared__ double sc[6][kHT / kWave];
    __shared__ float s_ms[2];
    const int tid = threadIdx.x;
    const int H = a.H, A = a.A;
    const int n = head_slab_floats(H, A);
    if (blockIdx.x == gridDim.x - 1) {
        head_fold_stats(a.stats, a.n_stat, a.h.M, sc, s_ms);
        double acc[6] = {0, 0, 0, 0, 0, 0};
        for (int b = tid; b < n_slabs; b += kHT) {
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[k] += a.loss_part[(size_t)b * 8 + k];
        }
        double r[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = block_sum<kHT / kWave>(acc[k], sc[k]);
        if (tid == 0) {
            const double M = (double)a.h.M;
            const float pg = (float)(r[0] / M);
            const float vl = 0.5f * (float)(r[1] / M);
            const float ent = (float)(r[2] / M);
            out[AURPPO_S_PG] = pg;
            out[AURPPO_S_VL] = vl;
            out[AURPPO_S_ENT] = ent;
            out[AURPPO_S_OLD_KL] = (float)(r[3] / M);
            out[AURPPO_S_KL] = (float)(r[4] / M);
            out[AURPPO_S_CLIPFRAC] = (float)(r[5] / M);
            out[AURPPO_S_LOSS] = (pg - a.h.ent_coef * ent) + vl * a.h.vf_coef;
            out[AURPPO_S_ADV_MEAN] = s_ms[0];
            out[AURPPO_S_ADV_STD] = s_ms[1];
        }
        return;
    }
    const int el = tid & 31, run = tid >> 5;
    const int e = (int)blockIdx.x * 32 + el;
    const int per = (n_slabs + 7) / 8;
    const int lo = run * per, hi = lo + per < n_slabs ? lo + per : n_slabs;
    double tsum = 0.0;
    if (e < n) {
        int s = lo;
        for (; s + 4 <= hi; s += 4) {
            float x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = a.slabs[(size_t)(s + k) * a.slab_stride + e];
#pragma unroll
            for (int k = 0; k < 4; ++k) tsum += (double)x[k];
        }
        for (; s < hi; ++s) tsum += (double)a.slabs[(size_t)s * a.slab_stride + e];
    }
    s_run[run][el] = tsum;
    __syncthreads();
    if (run != 0 || e >= n) return;
    double total = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) total += s_run[q][el];
    int dst = -1;
    if (e < (A + 3) * H && a.Hr != H) {                // slab rows of H floats, bucket rows of Hr: the real columns at the bucket's stride
        const int k = e / H, c = e - k * H;
        if (c < a.Hr) dst = (k < A ? a.off_wa + k * a.Hr : k == A ? a.off_wc : k == A + 1 ? a.off_bla : a.off_blc) + c;
    } else if (e < A * H) dst = a.off_wa + e;
    else if (e < (A + 1) * H) dst = a.off_wc + (e - A * H);
    else if (e < (A + 2) * H) dst = a.off_bla + (e - (A + 1) * H);
    else if (e < (A + 3) * H) dst = a.off_blc + (e - (A + 2) * H);
    else {
        const int j = e - (A + 3) * H;
        if (j < NA) dst = j < A ? a.off_ba + j : -1;
        else if (j < 2 * NA) dst = (a.continuous && j - NA < A) ? a.off_ls + (j - NA) : -1;
        else if (j == 2 * NA) dst = a.off_bc;
    }
    if (dst >= 0) grads[dst] = (float)total;
}

int head_tpr(int H) {
    int tpr = 8;
    while (tpr * 4 < H) tpr *= 2;
    return tpr;
}
// workgroups: eight rows per row group where the minibatch has them, at most kHeadMaxGrid -- a function of (M, H) only
int head_grid(int M, int H) {
    const int gpw = kHT / head_tpr(H);
    long long g = ((long long)M + gpw * 8 - 1) / (gpw * 8);
    if (g < 1) g = 1;
    if (g > kHeadMaxGrid) g = kHeadMaxGrid;
    return (int)g;
}
int head_slab_stride(int H, int A) { return (head_slab_floats(H, A) + 63) & ~63; }

struct HeadWs {
    double (*stats)[2];
    double* loss_part;
    float* slabs;
    size_t bytes;
};
HeadWs head_carve(void* workspace, int M, int H, int A) {
    aurppo_mlp::WsCarver c(workspace);
    HeadWs w;
    const int grid = head_grid(M, H);
    w.stats = c.take<double[2]>(kHeadStat * 2 * sizeof(double));
    w.loss_part = c.take<double>((size_t)grid * 8 * sizeof(double));
    w.slabs = c.take<float>((size_t)grid * head_slab_stride(H, A) * sizeof(float), 64);
    w.bytes = c.bytes;
    return w;
}

// ---- K14: the forward-only sibling of k_head_ppo for the rollout step (src/ppo.py:103-108: policy.evaluate(next_obs) under no_grad,
// then the three buffer row stores) of the policies whose hidden layers run on k_linear.  K13's thread layout, LDS weights, butterfly
// and fixed-order sum over a row's waves; the head dot products, their reduction and the log-prob are K13's expressions in K13's
// order, so the log-prob stored here is bit for bit the one k_head_ppo forms from the stored action at the same parameters.  Lane 0
// of a row samples (a = mu + exp(logstd) * eps for the Gaussian head; the inverse CDF of softmax(logits) at u for the Categorical
// head, counted as k_mlp_act counts it) and stores action, log-prob and value with 4-byte stores: the outputs are rows of the rollout
// buffer.  One launch, no slabs: a row is finished by the workgroup that read it.  noise == nullptr: the value only (the bootstrap).
struct HeadActArgs {
    const float* hA;                 // (N, H) last hidden activations; nullptr allowed without noise
    const float* hC;
    const float* noise;              // (N, A) standard normal | (N,) uniform [0, 1) | nullptr
    const float* params;
    float* actions;                  // (N, A) | (N,)
    float* logp;                     // (N,)
    float* value;                    // (N,)
    int off_wa, off_ba, off_wc, off_bc, off_ls;
    int N, H, A, continuous, n_iter;
    int Hr;                          // floats of a head row in the bucket (HeadArgs::Hr)
};

template <int TPR, int NA>
__global__ __launch_bounds__(kHT) void k_head_act(const HeadActArgs a) {
    constexpr int GPW = kHT / TPR;
    constexpr int NWG = TPR > kWave ? TPR / kWave : 1;
    constexpr int LW = TPR > kWave ? kWave : TPR;
    extern __shared__ __attribute__((aligned(16))) float sW[];       // (A + 1, H): actor head rows, then the critic's
    __shared__ float s_small[head_small(NA)];          // b_actor [NA], logstd [NA], std [NA]
    __shared__ float s_part[2][kHT / kWave][NA + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, A = a.A;
    const int nA = a.noise ? A : 0;                    // actor outputs to form: none for the value alone
    if (a.Hr == H) {
        for (int e = tid; e < (A + 1) * H; e += kHT) {
            if (e >= A * H) sW[e] = a.params[a.off_wc + (e - A * H)];
            else if (nA) sW[e] = a.params[a.off_wa + e];
        }
    } else {                                           // head rows of Hr floats: zero columns from Hr on, and no read behind a row's end
        for (int k = nA ? 0 : A; k <= A; ++k) {
            const float* const src = k < A ? a.params + a.off_wa + (size_t)k * a.Hr : a.params + a.off_wc;
            for (int c = tid; c < H; c += kHT) sW[k * H + c] = c < a.Hr ? src[c] : 0.0f;
        }
    }
    if (tid < NA) {
        s_small[tid] = tid < nA ? a.params[a.off_ba + tid] : 0.0f;
        const float ls = (a.continuous && tid < nA) ? a.params[a.off_ls + tid] : 0.0f;
        s_small[NA + tid] = ls;
        s_small[2 * NA + tid] = expf(ls);
    }
    __syncthreads();
    const float bc = a.params[a.off_bc];

    const int g = tid / TPR, t = tid % TPR;
    const int c0 = 4 * t;
    const bool colok = c0 < H;
    const int cw = colok ? c0 : 0;
    const int G = (int)gridDim.x * GPW, gg = (int)blockIdx.x * GPW + g;
    const float4 wc = *reinterpret_cast<const float4*>(sW + A * H + cw);
    const float4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    float4 na = zero4, nc = zero4;
    auto fetch = [&](long long row) {
        na = nc = zero4;
        if (row < a.N && colok) {
            if (nA) na = *reinterpret_cast<const float4*>(a.hA + (size_t)row * H + c0);
            nc = *reinterpret_cast<const float4*>(a.hC + (size_t)row * H + c0);
        }
    };
    fetch(gg);
    for (int it = 0; it < a.n_iter; ++it) {
        const long long row = (long long)it * G + gg;
        const bool valid = row < a.N;
        const float4 ha = na, hc = nc;
        fetch(row + G);

        float p[NA + 1];
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            p[k] = 0.0f;
            if (k < nA) p[k] = dot4(ha, *reinterpret_cast<const float4*>(sW + k * H + cw));
        }
        p[NA] = dot4(hc, wc);
#pragma unroll
        for (int k = 0; k < NA + 1; ++k) {
            if (k < nA || k == NA) {
#pragma unroll
                for (int off = LW / 2; off > 0; off >>= 1) p[k] += __shfl_xor(p[k], off, kWave);
            }
        }
        if (NWG > 1) {
            float* const mine = s_part[it & 1][wave];
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < NA + 1; ++k)
                    if (k < nA || k == NA) mine[k] = p[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < NA + 1; ++k) {
                if (k < nA || k == NA) {
                    float s = 0.0f;
#pragma unroll
                    for (int w = 0; w < NWG; ++w) s += s_part[it & 1][g * NWG + w][k];
                    p[k] = s;
                }
            }
        }
        if (!valid || t != 0) continue;
        a.value[row] = p[NA] + bc;
        if (!nA) continue;
        if (a.continuous) {
            const float* const eps = a.noise + (size_t)row * A;
            float* const out = a.actions + (size_t)row * A;
            HeadLogpAcc<NA> logp = 0.0f;
#pragma unroll
            for (int k = 0; k < NA; ++k)
                if (k < A) logp += gauss_sample(p[k] + s_small[k], s_small[2 * NA + k], s_small[NA + k], eps[k], out[k]);
            a.logp[row] = (float)logp;
        } else {
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                if (k < A) {
                    p[k] += s_small[k];
                    mx = fmaxf(mx, p[k]);
                }
            }
            float se = 0.0f;
#pragma unroll
            for (int k = 0; k < NA; ++k)
                if (k < A) se += expf(p[k] - mx);
            const float lse = mx + logf(se);
            const float u = a.noise[row];
            float cdf = 0.0f;
            int pick = A - 1;
            bool open = true;
#pragma unroll
            for (int k = 0; k < NA; ++k) {
                if (k < A && open) {
                    cdf += expf(p[k] - lse);
                    if (u < cdf) {
                        pick = k;
                        open = false;
                    }
                }
            }
            float logp = 0.0f;
#pragma unroll
            for (int k = 0; k < NA; ++k)
                if (k == pick) logp = p[k] - lse;
            a.actions[row] = (float)pick;
            a.logp[row] = logp;
        }
    }
}

// workgroups of K14: two rows per row group where the step has them -- a rollout step is a few thousand rows, spread over the chip
int head_act_grid(int N, int H) {
    const int gpw = kHT / head_tpr(H);
    long long g = ((long long)N + gpw * 2 - 1) / (gpw * 2);
    if (g < 1) g = 1;
    if (g > 2 * kHeadMaxGrid) g = 2 * kHeadMaxGrid;
    return (int)g;
}

// The TPR build of a head kernel for a.H, on `grid` workgroups with its (A + 1) x H weights as dynamic LDS: launch_k_head_ppo,
// launch_k_head_act.  The limit is raised to the largest shape's, once per build and device.  NA follows from A alone (head_na): A <= 16
// runs the NA = 16 builds whichever entry asked.
#define AURPPO_HEAD_DISPATCH(K, ARGS)                                                                                  \
    template <int NA>                                                                                                  \
    int launch_na_##K(const ARGS& a, int grid, hipStream_t s) {                                                        \
        const size_t lds = (size_t)(a.A + 1) * a.H * sizeof(float), cap = (size_t)(NA + 1) * 1024 * sizeof(float);     \
        switch (head_tpr(a.H)) {                                                                                       \
            case 8: return launch_dyn_lds<K<8, NA>>(#K, grid, kHT, lds, cap, s, a);                                    \
            case 16: return launch_dyn_lds<K<16, NA>>(#K, grid, kHT, lds, cap, s, a);                                  \
            case 32: return launch_dyn_lds<K<32, NA>>(#K, grid, kHT, lds, cap, s, a);                                  \
            case 64: return launch_dyn_lds<K<64, NA>>(#K, grid, kHT, lds, cap, s, a);                                  \
            case 128: return launch_dyn_lds<K<128, NA>>(#K, grid, kHT, lds, cap, s, a);                                \
            default: return launch_dyn_lds<K<256, NA>>(#K, grid, kHT, lds, cap, s, a);                                 \
        }                                                                                                              \
    }                                                                                                                  \
    int launch_##K(const ARGS& a, int grid, hipStream_t s) {                                                           \
        return head_na(a.A) == 32 ? launch_na_##K<32>(a, grid, s) : launch_na_##K<16>(a, grid, s);                     \
    }
AURPPO_HEAD_DISPATCH(k_head_act, HeadActArgs)
AURPPO_HEAD_DISPATCH(k_head_ppo, HeadArgs)
#undef AURPPO_HEAD_DISPATCH

// The largest build's LDS: k_head_ppo<*, 32>'s static arrays (s_red, s_small, s_part, s_sm, s_loss, s_dred, s_ms, each rounded up to 16
// bytes) beside (32 + 1) x 1024 dynamic floats, within the CU's 160 KiB.
constexpr size_t head_ppo_static_lds(int NA) {
    auto up = [](size_t bytes) { return (bytes + 15) & ~(size_t)15; };
    return up((size_t)kHT * 16) + up((size_t)head_small(NA) * 4) + up((size_t)2 * (kHT / kWave) * (NA + 4) * 4) +
           up((size_t)32 * head_small(NA) * 4) + up((size_t)32 * 6 * 8) + up((size_t)2 * (kHT / kWave) * 8) + 16;
}
static_assert(head_ppo_static_lds(kHeadMaxA) + (size_t)(kHeadMaxA + 1) * 1024 * sizeof(float) <= (size_t)160 * 1024,
              "k_head_ppo<*, 32>: dynamic + static LDS above the CU's 160 KiB");

// rows each of the grid's row groups takes: ceil(rows / (grid * rows per workgroup))
int head_n_iter(int rows, int H, int grid) {
    const long long per = (long long)grid * (kHT / head_tpr(H));
    return (int)((rows + per - 1) / per);
}

// layout[i] .. layout[i] + need[i] lies in the bucket, for the first `count` offsets
int head_layout_check(const int* layout, const long long* need, int count, int n_params, const char* who) {
    for (int i = 0; i < count; ++i)
        AURPPO_REQUIRE(layout[i] >= 0 && (long long)layout[i] + need[i] <= (long long)n_params, AURPPO_EINVAL,
                       "%s: layout offset %d (%d) outside the bucket of %d", who, i, layout[i], n_params);
    return AURPPO_OK;
}

}  // namespace

// max_a: 16 for the entries that came first, 32 for the `wa` (wide action head) entries
bool head_shape_ok_upto(int H, int A, int continuous, int max_a) {
    return H % 32 == 0 && H >= 32 && H <= 1024 && A >= 1 && A <= max_a && (continuous || A >= 2);
}
bool head_shape_ok(int H, int A, int continuous) { return head_shape_ok_upto(H, A, continuous, 16); }

// K14 on checked operands; lay = {actor head w, b; critic head w, b; actor_logstd}  (this and head_shape_ok: also layered.hip's)
int head_act_launch(const float* hA, const float* hC, const float* noise, int N, int H, int Hr, int A, int continuous, const float* params,
                    const int* lay, float* actions, float* logp, float* value, hipStream_t s) {
    HeadActArgs a;
    a.hA = hA; a.hC = hC; a.noise = noise; a.params = params;
    a.actions = actions; a.logp = logp; a.value = value;
    a.off_wa = lay[0]; a.off_ba = lay[1]; a.off_wc = lay[2]; a.off_bc = lay[3]; a.off_ls = lay[4];
    a.N = N; a.H = H; a.Hr = Hr; a.A = A; a.continuous = continuous ? 1 : 0;
    const int grid = head_act_grid(N, H);
    a.n_iter = head_n_iter(N, H, grid);
    return launch_k_head_act(a, grid, s);
}

extern "C" size_t aurppo_head_ppo_workspace_bytes(int M, int H, int A) {
    if (M <= 0 || !head_shape_ok(H, A, 1)) return 0;
    return head_carve(nullptr, M, H, A).bytes;
}
// ... with A up to 32: the same figure at A <= 16
extern "C" size_t aurppo_head_ppo_wa_workspace_bytes(int M, int H, int A) {
    if (M <= 0 || !head_shape_ok_upto(H, A, 1, kHeadMaxA)) return 0;
    return head_carve(nullptr, M, H, A).bytes;
}

// K13's three launches under the entry's name `who`: (M, H) planes, head rows and last-layer biases of Hr <= H floats in the bucket,
// at most max_a (16 | 32) actions
int head_ppo_run(const char* who, const float* hA, const float* hC, float* gzA, float* gzC, const float* actions, const float* rec,
                 const int32_t* idx, int M, int H, int Hr, int A, int continuous, const float* params, const int* layout_h, int n_params,
                 float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace,
                 void* stream, int max_a) {
    AURPPO_REQUIRE(hA && hC && gzA && gzC && rec && idx && params && layout_h && grads && out_scalars && workspace, AURPPO_EINVAL,
                   "%s: null pointer", who);
    AURPPO_REQUIRE(M > 0, AURPPO_ESHAPE, "%s: M=%d", who, M);
    AURPPO_REQUIRE(head_shape_ok_upto(H, A, continuous, max_a) && Hr >= 1 && Hr <= H, AURPPO_ESHAPE,
                   "%s: H=%d (a multiple of 32, 32..1024), A=%d (1..%d, Categorical: 2..%d)", who, H, A, max_a, max_a);
    AURPPO_REQUIRE(vloss_mode >= 0 && vloss_mode <= 2, AURPPO_EINVAL, "%s: vloss_mode %d", who, vloss_mode);
    const int aw = continuous ? A : 1;
    AURPPO_REQUIRE(actions || aw <= 12, AURPPO_ESHAPE, "%s: packed records hold at most 12 action floats (A=%d)", who, A);
    AURPPO_REQUIRE(aligned_to(hA, 16) && aligned_to(hC, 16) && aligned_to(gzA, 16) && aligned_to(gzC, 16) && aligned_to(rec, 16) &&
                       aligned_to(workspace, 64),
                   AURPPO_EINVAL, "%s: operands not 16-byte / workspace not 64-byte aligned", who);
    HeadArgs a;
    a.off_wa = layout_h[0]; a.off_ba = layout_h[1]; a.off_wc = layout_h[2]; a.off_bc = layout_h[3]; a.off_ls = layout_h[4];
    a.off_bla = layout_h[5]; a.off_blc = layout_h[6];
    const long long need[7] = {(long long)A * Hr, A, Hr, 1, continuous ? A : 0, Hr, Hr};
    if (const int rc = head_layout_check(layout_h, need, 7, n_params, who)) return rc;
    const HeadWs w = head_carve(workspace, M, H, A);
    a.hA = hA; a.hC = hC; a.gzA = gzA; a.gzC = gzC;
    a.actions = actions; a.rec = reinterpret_cast<const float4*>(rec); a.rec_stride = actions ? 1 : 4; a.aw = aw;
    a.idx = idx; a.params = params;
    a.stats = w.stats; a.slabs = w.slabs; a.loss_part = w.loss_part;
    a.slab_stride = head_slab_stride(H, A);
    a.M = M; a.H = H; a.Hr = Hr; a.A = A; a.continuous = continuous ? 1 : 0;
    a.h = make_hyper(M, clip, ent_coef, vf_coef, norm_adv, vloss_mode);
    const int grid = head_grid(M, H);
    a.n_iter = head_n_iter(M, H, grid);
    int n_stat = (M + kHT * 4 - 1) / (kHT * 4);
    if (n_stat > kHeadStat) n_stat = kHeadStat;
    a.n_stat = n_stat;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_head_stats, dim3(n_stat), dim3(kHT), 0, s, a.rec, a.rec_stride, idx, M, w.stats);
    AURPPO_LAUNCH_CHECK("k_head_stats");
    if (const int rc = launch_k_head_ppo(a, grid, s)) return rc;
    const int n = head_slab_floats(H, A);
    hipLaunchKernelGGL(k_head_fold, dim3((n + 31) / 32 + 1), dim3(kHT), 0, s, a, grid, head_na(A), grads, out_scalars);
    AURPPO_LAUNCH_CHECK("k_head_fold");
    return AURPPO_OK;
}

#define AURPPO_HEAD_PPO_ENTRY(NAME, MAX_A)                                                                                                \
    extern "C" int NAME(const float* hA, const float* hC, float* gzA, float* gzC, const float* actions, const float* rec,                 \
                        const int32_t* idx, int M, int H, int A, int continuous, const float* params, const int* layout_h, int n_params,  \
                        float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode, float* out_scalars,      \
                        void* workspace, void* stream) {                                                                                  \
        return head_ppo_run(#NAME, hA, hC, gzA, gzC, actions, rec, idx, M, H, H, A, continuous, params, layout_h, n_params, grads, clip,  \
                            ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars, workspace, stream, MAX_A);                              \
    }
AURPPO_HEAD_PPO_ENTRY(aurppo_head_ppo_f32, 16)
AURPPO_HEAD_PPO_ENTRY(aurppo_head_ppo_wa_f32, kHeadMaxA)
#undef AURPPO_HEAD_PPO_ENTRY

namespace {

// K14 alone behind both entries: layout_h = {actor head w, b; critic head w, b; actor_logstd}.
int head_act_entry(const char* who, const float* hA, const float* hC, const float* noise, int N, int H, int A, int continuous,
                   const float* params, const int* layout_h, int n_params, float* actions, float* logp, float* value, void* stream, int max_a) {
    AURPPO_REQUIRE(hC && params && layout_h && value && (!noise || (hA && actions && logp)), AURPPO_EINVAL, "%s: null pointer", who);
    AURPPO_REQUIRE(N > 0, AURPPO_ESHAPE, "%s: N=%d", who, N);
    AURPPO_REQUIRE(head_shape_ok_upto(H, A, continuous, max_a), AURPPO_ESHAPE,
                   "%s: H=%d (a multiple of 32, 32..1024), A=%d (1..%d, Categorical: 2..%d)", who, H, A, max_a, max_a);
    AURPPO_REQUIRE((!noise || aligned_to(hA, 16)) && aligned_to(hC, 16), AURPPO_EINVAL, "%s: activations not 16-byte aligned", who);
    AURPPO_REQUIRE((!noise || (aligned_to(noise, 4) && aligned_to(actions, 4) && aligned_to(logp, 4))) && aligned_to(value, 4),
                   AURPPO_EINVAL, "%s: noise / outputs not 4-byte aligned", who);
    const long long need[5] = {(long long)A * H, A, H, 1, continuous ? A : 0};
    if (const int rc = head_layout_check(layout_h, need, 5, n_params, who)) return rc;
    return head_act_launch(hA, hC, noise, N, H, H, A, continuous, params, layout_h, actions, logp, value, (hipStream_t)stream);
}

}  // namespace

#define AURPPO_HEAD_ACT_ENTRY(NAME, MAX_A)                                                                                                \
    extern "C" int NAME(const float* hA, const float* hC, const float* noise, int N, int H, int A, int continuous, const float* params,   \
                        const int* layout_h, int n_params, float* actions, float* logp, float* value, void* stream) {                     \
        return head_act_entry(#NAME, hA, hC, noise, N, H, A, continuous, params, layout_h, n_params, actions, logp, value, stream, MAX_A); \
    }
AURPPO_HEAD_ACT_ENTRY(aurppo_head_act_f32, 16)
AURPPO_HEAD_ACT_ENTRY(aurppo_head_act_wa_f32, kHeadMaxA)
#undef AURPPO_HEAD_ACT_ENTRY
