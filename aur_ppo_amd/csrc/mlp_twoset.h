// What the two builds of K7's two-tile-set step share -- k_mlp_step2 (mlp2.hip, fp32 MFMA) and k_mlp_step3 (mlp3.hip, bf16x3 MFMA):
// the software barriers of a tile set, the LDS accumulate and the loss lanes of the L phase (loss_lanes).  What differs stays in the
// kernels: the tile queue in front of the loss lanes and the stores behind them (fp32 in place in step2; bf16 planes and the next
// tile's row fetch in step3).  So does the hand-over at the end of the launch, written out in both: as one function here it gave
// the same bits and was slower -- k_mlp_step2 alone 157.7 -> 158.7 us (above the parent in each of four alternating rounds), the
// whole step as a hipGraph 1.952 -> 1.973 ms with k_mlp_step3's folded, the gap gone with it written out again
// (profiles/refactor_dist_terms.txt, section 5).
// Both includers say `#pragma clang fp contract(fast)` in front of their includes, and this code is written for that mode.
#pragma once
#include "mlp_common.h"

#ifndef AURPPO_BAR_SLEEP
#define AURPPO_BAR_SLEEP 1   // s_sleep argument of the software barriers' poll loops (A/B knob; 0 = poll back to back)
#endif

namespace aurppo_mlp {

constexpr int kTwoSetAccRegs = 72;           // gW1 (32) + gW2 (32) + gW3 (2 x 4) per lane: what set 1 parks at the hand-over

// LDS accumulate without reading the result back (ds_add_f64)
__device__ __forceinline__ void lds_add(double* p, double v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The two sets share no barrier inside the tile loop.  The NW waves that do meet at a counter in LDS (arrive = one ds_add by lane 0
// once the wave's LDS writes have completed, wait = poll until NW more arrivals than at the previous barrier; `gen` = the wave's own
// count), so neither set waits for the other's longer phase -- with workgroup-wide barriers 38 % of the loop was the tail of
// intervals where one set finished its epilogue alone -- and a set whose queue is dry simply leaves.  NW = 4: a set's waves (around
// S and L); NW = 2: the two waves of one net, the only ones that exchange data between that net's layers.
template <int NW>
__device__ __forceinline__ void wave_group_bar(int* arrivals, int& gen, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (lane == 0) (void)__hip_atomic_fetch_add(arrivals, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    gen += NW;
    while (__hip_atomic_load(arrivals, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) - gen < 0)
        __builtin_amdgcn_s_sleep(AURPPO_BAR_SLEEP);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- L phase: distribution + PPO terms of one tile, 8 lanes per row (lane lj of a row holds head outputs lj and lj + 8: m0, m1, and the
// stored action's dims act_cur).  Straight-line per lane: the 8-lane reductions are DPP moves (no LDS round trip), and a padding row
// (!real) only masks what is handed back.  d0 / d1 = d loss / d head output lj / lj + 8; the d-logstd terms accumulate into g_ls.
struct LossLanes {
    PpoSample t;
    float ent, d0, d1;
};
__device__ __forceinline__ LossLanes loss_lanes(int continuous, int A, int lj, bool real, float m0, float m1, const float (&act_cur)[2],
                                                const float* sIvar, const float* sLs, float ent_gauss, float g_ent, float4 rc,
                                                float v_new, float mean, float denom, float invM, const PpoHyper& h, float (&g_ls)[2]) {
    LossLanes o;
    const int k0 = lj, k1 = lj + 8;
    float logp = 0.0f;
    if (continuous) {
        // Normal(mu, exp(logstd)): log-prob summed over action dims (actor_critic.py:36-43)
        const float iv0 = k0 < A ? sIvar[k0] : 0.0f, iv1 = k1 < A ? sIvar[k1] : 0.0f;
        const float z0 = act_cur[0] - m0, z1 = act_cur[1] - m1;
        if (k0 < A) logp += gauss_logp_ivar(z0, iv0, sLs[k0]);
        if (k1 < A) logp += gauss_logp_ivar(z1, iv1, sLs[k1]);
        logp = sum8(logp);
        o.ent = ent_gauss;
        o.t = ppo_sample(logp, rc.x, rc.y, v_new, rc.w, rc.z, mean, denom, invM, h);
        o.d0 = (real && k0 < A) ? gauss_dmu(o.t.g_logp, z0, iv0) : 0.0f;
        o.d1 = (real && k1 < A) ? gauss_dmu(o.t.g_logp, z1, iv1) : 0.0f;
        if (real && k0 < A) g_ls[0] += gauss_dls(o.t.g_logp, z0, iv0, g_ent);
        if (real && k1 < A) g_ls[1] += gauss_dls(o.t.g_logp, z1, iv1, g_ent);
    } else {
        // Categorical(logits): log_softmax, log-prob of the stored action, entropy (actor_critic.py:45-50)
        const int ai = (int)sum8(act_cur[0]);   // only lane lj == 0 holds the action index, the others hold 0
        const float z0 = k0 < A ? m0 : -INFINITY, z1 = k1 < A ? m1 : -INFINITY;
        const float mx = max8(fmaxf(z0, z1));
        const float se = sum8((k0 < A ? expf(z0 - mx) : 0.0f) + (k1 < A ? expf(z1 - mx) : 0.0f));
        const float lse = mx + logf(se);
        const float lp0 = k0 < A ? z0 - lse : 0.0f, lp1 = k1 < A ? z1 - lse : 0.0f;
        const float p0 = k0 < A ? expf(lp0) : 0.0f, p1 = k1 < A ? expf(lp1) : 0.0f;
        o.ent = sum8(-(p0 * lp0) - p1 * lp1);
        logp = sum8((k0 == ai ? lp0 : 0.0f) + (k1 == ai ? lp1 : 0.0f));
        o.t = ppo_sample(logp, rc.x, rc.y, v_new, rc.w, rc.z, mean, denom, invM, h);
        o.d0 = (real && k0 < A) ? cat_dlogit(o.t.g_logp, k0 == ai, p0, lp0, o.ent, g_ent) : 0.0f;
        o.d1 = (real && k1 < A) ? cat_dlogit(o.t.g_logp, k1 == ai, p1, lp1, o.ent, g_ent) : 0.0f;
    }
    return o;
}

}  // namespace aurppo_mlp
