// The tail of a fused MLP minibatch step, as K7's host side (mlp.hip) and K7w's (mlp_wide.hip) call it: the fixed-order slab reduce
// and, for a whole minibatch, the optimizer launch behind it.  The kernels and the launchers are mlp_tail.hip.
#pragma once
#include "mlp_common.h"

namespace aurppo_mlp {

// Where an updated weight is also kept in MFMA-operand order for the next K7 launch (W1 in k_mlp_step2's fp32 B-operand order;
// W1 / W2 as bf16 planes for k_mlp_step3).  Offsets past the bucket switch a copy off.
struct OperandCopies {
    int w1_actor, w1_critic, D;
    float* w1op;
    int w2_actor, w2_critic;
    unsigned short* wop3;
    WideCopies wide;     // K7w's copies (wide.wop == nullptr: none)
};
// No copies at all (every offset past the bucket), K7's (L != nullptr: the two-layer nets at L; w1op / wop3 name the copies to refresh) or
// K7w's (wide != nullptr).
OperandCopies operand_copies(int n_params, const MlpLayout* L = nullptr, int D = 1, float* w1op = nullptr, unsigned short* wop3 = nullptr,
                             const WideCopies* wide = nullptr);

// The optimizer half of aurppo_mlp_ppo_minibatch_f32 / aurppo_mlp_wide_ppo_minibatch_f32 (and, with grad_only, the step advance of
// aurppo_mlp_ppo_grad_f32)
struct MlpTail {
    float* params_rw;
    float* exp_avg;
    float* exp_avg_sq;
    double max_norm;
    const float* lr_dev;
    float* step_dev;
    double beta1, beta2, eps;
    float* out_norm;
    const int32_t* next_idx;   // the slice stepped next: its statistics (and the refreshed operand copies) are left by this call
    int next_M;
    int chained;               // the previous call named this idx as its next_idx: no prepare pass
    int grad_only;             // stop after the reduce (the caller all-reduces the gradient, then calls the apply half)
};

// One launch of k_adam_chain: global-norm clip + Adam over the bucket, the operand copies refreshed, and -- where next_idx and stats
// are both given -- the next slice's advantage partial sums in stat_blocks_for(next_M) more workgroups.
struct AdamLaunch {
    float* params;              // the bucket: n_params elements each
    float* grads;
    float* exp_avg;
    float* exp_avg_sq;
    int n_params;
    const double* sq_part;      // the norm: n_part partial sums of squares (k_mlp_reduce's); nullptr: formed in the kernel from
    int n_part;                 //   grads * gscale
    float gscale;               // applied to the stored gradient first (1 / world after a SUM all-reduce)
    double max_norm;
    const float* lr_dev;
    const float* step_dev;
    double beta1, beta2, eps;
    float* out_norm;
    OperandCopies copies;
    const float4* rec;          // the next slice's statistics: records, float4s per record, indices, (kStatBlocks, 2) doubles
    int rec_stride;
    const int32_t* next_idx;
    int next_M;
    double* stats;
    const double* bc;           // {1 - beta1^t, 1 - beta2^t} formed by the reduce in front, or nullptr
};
int launch_adam_chain(const AdamLaunch& a, hipStream_t s);

// What a step path hands over after its main kernel: the slabs and loss partials that kernel wrote, where the gradient and the
// scalars go, and the workspace regions and operand copies of its family.
struct TailWork {
    const float* slabs;         // (n_slabs, slab_stride(n_params)) if slab_strided (K7: k_mlp_reduce_x4), else (n_slabs, n_params)
    bool slab_strided;          //   (K7w: k_mlp_reduce<1>, or <2> past kMaxGrid slabs)
    const double* loss_part;    // (n_slabs, 8)
    int n_slabs, n_params;
    PpoHyper h;
    float* grads;
    float* out_scalars;
    double* sq_part;            // workspace: the clip's partial sums, one per 64 parameters
    unsigned* counters;         // workspace: the 16-word counter block; the reduce clears words 0 and 1 when it advances the step, and
                                //   words 8..11 carry Adam's bias corrections from the reduce to the optimizer launch
    const float4* rec;          // for the next slice's statistics
    int rec_stride;
    double* stats;
    OperandCopies copies;       // what the optimizer launch refreshes
};
// The reduce; with a tail the Adam step count is advanced; with a tail that is not grad_only the reduce also leaves the clip's partial
// sums and the bias corrections, and the optimizer launch follows.
int launch_mlp_tail(const TailWork& w, const MlpTail* tail, hipStream_t s);

}  // namespace aurppo_mlp
