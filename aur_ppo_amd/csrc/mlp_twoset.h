// What the two builds of K7's two-tile-set step share -- k_mlp_step2 (mlp2.hip, fp32 MFMA) and k_mlp_step3 (mlp3.hip, bf16x3 MFMA):
// the software barriers of a tile set and the LDS accumulate.  (The loss lanes and the hand-over are still written out in both
// kernels: folded into functions here they compile to other instruction streams, which have not been timed against these.)
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

}  // namespace aurppo_mlp
