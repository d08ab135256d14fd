// Per-sample PPO loss terms and their gradients (src/ppo.py:225-264), shared by the stand-alone loss
// kernel (loss.hip) and the fused MLP step (mlp.hip).  torch autograd conventions: max() ties split
// 0.5/0.5, clamp passes gradient on the closed interval.
//
// Non-finite inputs.  fmaxf / fminf return the operand that is not NaN, torch.max / torch.clamp return NaN, and torch's
// clamp backward SELECTS zero outside the interval where a product by 0 turns an infinite term into NaN.  ppo_sample<true>
// (the per-op loss kernel, whose inputs come from any caller) follows torch in all three; on finite inputs it gives the
// same bits as ppo_sample<false>.  The fused steps keep ppo_sample<false>: their log-prob and value are computed inside the
// kernel from the parameters, so a NaN there means NaN parameters, which turn every output NaN anyway.
#pragma once
#include "common.h"

struct PpoHyper {
    int M;
    float clip, lo, hi, ent_coef, vf_coef;
    int norm_adv, vloss_mode;
};

struct PpoSample {
    float g_logp;  // d loss / d newlogp
    float g_v;     // d loss / d newv
    float pg, vl, okl, kl, cf;  // this sample's contribution to the (un-normalised) sums
};

// torch.max / torch.clamp on a NaN operand, and torch's clamp backward (a select, not a product by 0) -- ppo_sample<true> only
__device__ __forceinline__ float ppo_nan_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }
__device__ __forceinline__ float ppo_nan_clamp(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float ppo_select(float t, float in) { return in != 0.0f ? t : copysignf(0.0f, t); }

template <bool NANPROP = false>
__device__ __forceinline__ PpoSample ppo_sample(float newlogp, float oldlogp, float a_raw, float v, float vo, float R,
                                                float mean, float denom, float invM, const PpoHyper& p) {
    PpoSample o;
    const float lr = newlogp - oldlogp;
    const float ratio = expf(lr);
    const float an = p.norm_adv ? (a_raw - mean) / denom : a_raw;
    o.okl = -lr;
    o.kl = (ratio - 1.0f) - lr;
    o.cf = (fabsf(ratio - 1.0f) > p.clip) ? 1.0f : 0.0f;
    const float rc = NANPROP ? ppo_nan_clamp(ratio, p.lo, p.hi) : fminf(fmaxf(ratio, p.lo), p.hi);
    const float l1 = -an * ratio;
    const float l2 = -an * rc;
    o.pg = NANPROP ? ppo_nan_max(l1, l2) : fmaxf(l1, l2);
    const float w1 = l1 > l2 ? 1.0f : (l1 == l2 ? 0.5f : 0.0f);
    const float inr = (ratio >= p.lo && ratio <= p.hi) ? 1.0f : 0.0f;
    const float dpg = NANPROP ? (w1 * (-an) + ppo_select((1.0f - w1) * (-an), inr)) * invM
                              : (w1 * (-an) + (1.0f - w1) * (-an) * inr) * invM;
    o.g_logp = dpg * ratio;
    float dvl;
    if (p.vloss_mode == AURPPO_VLOSS_CLIPPED) {
        const float du = v - R;
        const float vu = du * du;
        const float dv = v - vo;
        const float dcl = NANPROP ? ppo_nan_clamp(dv, -p.clip, p.clip) : fminf(fmaxf(dv, -p.clip), p.clip);
        const float dc = (vo + dcl) - R;
        const float vc = dc * dc;
        o.vl = NANPROP ? ppo_nan_max(vu, vc) : fmaxf(vu, vc);
        const float u1 = vu > vc ? 1.0f : (vu == vc ? 0.5f : 0.0f);
        const float inv = (dv >= -p.clip && dv <= p.clip) ? 1.0f : 0.0f;
        dvl = NANPROP ? (u1 * (2.0f * du) + ppo_select((1.0f - u1) * (2.0f * dc), inv)) * (0.5f * invM)
                      : (u1 * (2.0f * du) + (1.0f - u1) * (2.0f * dc) * inv) * (0.5f * invM);
    } else {
        const float du = v - (p.vloss_mode == AURPPO_VLOSS_RETURNS ? R : vo);
        o.vl = du * du;
        dvl = (2.0f * du) * (0.5f * invM);
    }
    o.g_v = dvl * p.vf_coef;
    return o;
}

// ---- Per-element terms of the action distributions (src/models/actor_critic.py:36-50), shared by every fused step (mlp2.hip, mlp3.hip,
// mlp_wide.hip, mlp_wide3.hip, head.hip) and rollout kernel (mlp.hip, mlp_wide.hip, head.hip).  The loss terms are scalars: the sums over a row's outputs
// stay in the loss lanes, whose layouts differ.  Sampling is here whole (below the terms): a Gaussian dimension is a scalar, and the
// Categorical rows of K8, K8w and k_mlpw_step<> share one layout -- one lane per row, its logits behind a pointer into LDS.  The kernels
// that hold a row elsewhere (k_head_ppo / k_head_act: registers; k_mlpw3_step: spread over lanes) keep their own Categorical sums.
// Each compiles in its includer's contract mode, like ppo_sample.
constexpr float kHalfLog2Pi = 0.9189385332046727f;   // log(2 pi) / 2

// Normal(mu, exp(ls)): one action dim's log-prob term, z = a - mu.  Two deliberate forms, not the same bits.  _ivar: the fused MLP steps
// (K7, K7w), which keep 1 / sd^2 in LDS and multiply.  _var: as torch forms it, a division by 2 var -- the rollout kernels (k_mlp_act,
// k_mlpw_act), whose log-prob becomes the stored old_logp that evaluate() is compared with, and K13 (k_head_ppo), which follows
// evaluate() through its gradients too (gauss_dmu_var / gauss_dls_var).
__device__ __forceinline__ float gauss_logp_ivar(float z, float ivar, float ls) { return (-(z * z) * (0.5f * ivar) - ls) - kHalfLog2Pi; }
__device__ __forceinline__ float gauss_logp_var(float z, float var, float ls) { return (-(z * z) / (2.0f * var) - ls) - kHalfLog2Pi; }
// ... its entropy term (state-independent), and d loss / d mu and d loss / d logstd from g_logp = d loss / d logp, g_ent = d loss / d entropy
__device__ __forceinline__ float gauss_ent(float ls) { return (0.5f + kHalfLog2Pi) + ls; }
__device__ __forceinline__ float gauss_dmu(float g_logp, float z, float ivar) { return g_logp * (z * ivar); }
__device__ __forceinline__ float gauss_dls(float g_logp, float z, float ivar, float g_ent) { return g_logp * (z * z * ivar - 1.0f) + g_ent; }
__device__ __forceinline__ float gauss_dmu_var(float g_logp, float z, float var) { return g_logp * (z / var); }
__device__ __forceinline__ float gauss_dls_var(float g_logp, float z, float var, float g_ent) { return g_logp * ((z * z) / var - 1.0f) + g_ent; }
// Categorical(logits): d loss / d logit k from p = softmax_k, lp = log p, ent = the row's entropy; hit: k is the action taken.
// d logp / d z_k = [k == a] - p_k ;  d H / d z_k = -p_k (log p_k + H)
__device__ __forceinline__ float cat_dlogit(float g_logp, bool hit, float p, float lp, float ent, float g_ent) {
    return g_logp * ((hit ? 1.0f : 0.0f) - p) + g_ent * (-p * (lp + ent));
}

// ---- Sampling (the rollout kernels K8 k_mlp_act, K8w k_mlpw_act, K14 k_head_act).
// Normal(mu, sd = exp(ls)) at the standard-normal draw eps: writes the action, returns the dimension's log-prob term with z formed from
// the action as evaluate() forms it, (a - mu) -- so the stored log-prob is the one the update computes from the stored action.
__device__ __forceinline__ float gauss_sample(float mu, float sd, float ls, float eps, float& action) {
    const float act = mu + sd * eps;
    action = act;
    return gauss_logp_var(act - mu, sd * sd, ls);
}
// Categorical(logits z[0 .. A)), one lane per row: log sum exp (max-subtracted) ...
__device__ __forceinline__ float cat_lse(const float* z, int A) {
    float mx = z[0];
    for (int k = 1; k < A; ++k) mx = fmaxf(mx, z[k]);
    float se = 0.0f;
    for (int k = 0; k < A; ++k) se += expf(z[k] - mx);
    return mx + logf(se);
}
// ... and the inverse CDF of softmax(z) at the uniform draw u (the last class where rounding leaves the sum below u), with its log-prob
__device__ __forceinline__ int cat_sample(const float* z, int A, float lse, float u, float& logp) {
    float cdf = 0.0f;
    int pick = A - 1;
    for (int k = 0; k < A; ++k) {
        cdf += expf(z[k] - lse);
        if (u < cdf) {
            pick = k;
            break;
        }
    }
    logp = z[pick] - lse;
    return pick;
}

// Mean and standard deviation (torch.std: over M - 1; M == 1 -> 0/0 = NaN, as there) of a minibatch's advantages from their sum and
// sum of squares, formed in double: every kernel that normalises advantages folds the same partial sums with this.
__device__ __forceinline__ void adv_mean_std(double ts, double tq, int M, float& mean, float& std) {
    const double m = ts / (double)M;
    double var = (tq - ts * m) / (double)(M - 1);
    if (var < 0.0) var = 0.0;
    mean = (float)m;
    std = (float)sqrt(var);
}

static inline PpoHyper make_hyper(int M, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode) {
    PpoHyper p;
    p.M = M;
    p.clip = (float)clip;
    p.lo = (float)(1.0 - clip);  // Python forms 1-eps / 1+eps in fp64; torch rounds them to fp32
    p.hi = (float)(1.0 + clip);
    p.ent_coef = (float)ent_coef;
    p.vf_coef = (float)vf_coef;
    p.norm_adv = norm_adv ? 1 : 0;
    p.vloss_mode = vloss_mode;
    return p;
}
