/*
 * aurppo.h -- C ABI of libaurppo_hip.so: the MI355X (gfx950) hot path of the aur_ppo trainer.
 *
 * The reference (biirving/aur_ppo) is pure Python/PyTorch and has no FFI of its own; the seam this
 * library replaces is the block of torch-op chains between "rollout buffer filled" and
 * "loss.backward()" in src/ppo.py / src/robot_ppo.py.  Each entry point cites the reference lines
 * whose arithmetic it performs.  Binding stub a maintainer would add: INTEGRATION.md (ctypes).
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer unless its name ends in _h.  Tensors are fp32, contiguous.
 *     Rollout tensors are time-major (T, N): element (t, n) at t*N + n -- the layout of
 *     torch_buffer (src/ppo.py:24-29) and of buffer.flatten() (src/ppo.py:32-39).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls enqueue and
 *     return; they never allocate, never synchronise (except the *_get_state/_set_state helpers).
 *     All entry points are safe to capture into a hipGraph EXCEPT the aurppo_mt19937_* / aurppo_shuffle_* family: a
 *     generator handle carries host-side sequence state and its own side streams, so those calls must run eagerly
 *     (aurppo_shuffle_*_i32 return AURPPO_EINVAL on a capturing stream); the trainer runs them on a side stream, one
 *     update ahead of the captured graph that reads their output.
 *   - Return 0 on success, <0 on error; aurppo_last_error() gives a thread-local message.
 *   - The caller owns all tensors.  The library owns only RNG handles.
 *   - No CPU fallbacks exist in this library: without a gfx950 device every compute call fails.
 */
#ifndef AURPPO_H
#define AURPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AURPPO_OK 0
#define AURPPO_EINVAL (-1) /* null pointer, bad enum, misaligned workspace            */
#define AURPPO_ESHAPE (-2) /* non-positive / inconsistent sizes, workspace too small  */
#define AURPPO_EHIP (-3)   /* a HIP runtime call failed (launch error, no device ...) */

#define AURPPO_VERSION 1

/* gae `mode` */
#define AURPPO_GAE 0           /* ppo.run_gae                       src/ppo.py:125-142        */
#define AURPPO_NORMAL_ADV 1    /* ppo.normal_advantage              src/ppo.py:145-157        */
#define AURPPO_GAE_SKIP_LAST 2 /* robot_ppo.run_gae as written      src/robot_ppo.py:224-244  */

/* loss `vloss_mode` (a bool clip_vloss maps to 1; the two un-clipped flavours differ upstream) */
#define AURPPO_VLOSS_RETURNS 0   /* 0.5*mean((v-R)^2)               src/robot_ppo.py:390      */
#define AURPPO_VLOSS_CLIPPED 1   /* clipped value loss              src/ppo.py:250-259        */
#define AURPPO_VLOSS_OLDVALUES 2 /* 0.5*mean((v-V_old)^2)           src/ppo.py:261            */

/* layout of out_scalars written by aurppo_loss_fwd_bwd_f32 */
#define AURPPO_S_LOSS 0     /* pg - ent_coef*ent + vl*vf_coef       src/ppo.py:264 */
#define AURPPO_S_PG 1       /* policy_loss                          src/ppo.py:245 */
#define AURPPO_S_VL 2       /* value_loss (un-weighted)             src/ppo.py:259,261 */
#define AURPPO_S_ENT 3      /* entropy_loss = mean(entropy)         src/ppo.py:263 */
#define AURPPO_S_OLD_KL 4   /* mean(-log_ratio)                     src/ppo.py:232 */
#define AURPPO_S_KL 5       /* mean((ratio-1)-log_ratio)            src/ppo.py:233 */
#define AURPPO_S_CLIPFRAC 6 /* mean(|ratio-1| > clip)               src/ppo.py:234 */
#define AURPPO_S_ADV_MEAN 7 /* minibatch advantage mean             src/ppo.py:239 */
#define AURPPO_S_ADV_STD 8  /* minibatch advantage std (ddof=1)     src/ppo.py:239 */
#define AURPPO_N_SCALARS 9

#define AURPPO_MAX_STREAMS 8

int aurppo_version(void);
const char* aurppo_last_error(void);
/* Number of gfx950 devices visible; <0 on HIP error.  Does not create a context on any of them. */
int aurppo_device_count(void);
/* Which build of the fused MLP step (K7) aurppo_mlp_ppo_*_f32 launches: 2 = k_mlp_step2 (v_mfma_f32_32x32x2_f32, fp32
 * operands), 3 = k_mlp_step3 (v_mfma_f32_32x32x16_bf16 over three-way bf16 splits of the fp32 operands, six products,
 * fp32 accumulate).  Same arguments, same results to the tolerances of tests/test_mlp_fused.py; environment variable
 * AURPPO_K7_VARIANT overrides the built-in default.  (No reference counterpart: the policy nets are torch modules
 * there, src/models/actor_critic.py:8-51.) */
int aurppo_k7_variant(void);
/* The library reads its AURPPO_* environment knobs once per process; this re-reads them now (diagnostics: bench.py switches
 * AURPPO_K7_VARIANT after its timed region to time the fp32-MFMA build beside the default).  Returns 0. */
int aurppo_reload_knobs(void);
/* Which kernel the aurppo_mlp_wide_* entry points launch for a net shape (K7w): 1 = both nets per workgroup on fp32 MFMA
 * (hidden_dim and state_dim <= 64), 2 = one net per workgroup on fp32 MFMA, 3 = one net per workgroup on bf16 MFMA over
 * three-way splits (default for the wider shapes; AURPPO_K7W_VARIANT=2 selects 2).  Same results to the tolerances of
 * tests/test_mlp_wide.py. */
int aurppo_k7w_kernel(int hidden, int state_dim);

/* ---- K1: advantage estimation -------------------------------------------------------------
 * Replaces ppo.run_gae / ppo.normal_advantage (src/ppo.py:125-157; duplicates in
 * src/utils/advantages.py:4-37) and robot_ppo.run_gae (src/robot_ppo.py:224-244, mode 2).
 *   for t = T-1..0:  nnt = 1 - done[t+1] (next_done at T-1);  nv = V[t+1] (next_value at T-1)
 *     delta = (r[t] + ((g*nv)*nnt)) - V[t];  A[t] = delta + (((g*lam)*nnt) * A[t+1]);  R = A + V
 * fp32 with exactly that association and no fused multiply-add (bit-identical to the reference's
 * CPU result); gamma is rounded to fp32, gamma*lam is formed in fp64 then rounded, as Python does.
 * Mode 1:  R[t] = r[t] + ((g*nnt)*R[t+1]) (R[T] = next_value);  A = R - V.
 * Mode 2:  the loop starts at T-2, so A[T-1] = 0 and R[T-1] = V[T-1] (upstream behaviour).       */
int aurppo_gae_f32(const float* rewards, const float* values, const float* terminals, /* (T,N) */
                   const float* next_value, const float* next_done,                    /* (N,)  */
                   float* advantages, float* returns,                                  /* (T,N) out */
                   int T, int N, double gamma, double lam, int mode, void* stream);

/* K1 + pack: as aurppo_gae_f32, and additionally writes the per-sample record
 *   rec[(t*N+n)*4 + {0,1,2,3}] = { log_probs[t,n], A[t,n], R[t,n], V[t,n] }   ((T*N, 4), 16-B aligned)
 * i.e. the four per-sample scalars buffer.flatten() hands to the update (src/ppo.py:32-39) laid out
 * so that the minibatch gather fetches them with ONE 16-byte request per sample.                   */
int aurppo_gae_pack_f32(const float* rewards, const float* values, const float* terminals,
                        const float* next_value, const float* next_done, const float* log_probs,
                        float* advantages, float* returns, float* rec, int T, int N, double gamma,
                        double lam, int mode, void* stream);

/* ---- K2: numpy-legacy MT19937 + Fisher-Yates shuffle --------------------------------------
 * Replaces np.random.seed(seed) (src/ppo.py:182) and np.random.shuffle(b_inds) (src/ppo.py:217,
 * src/robot_ppo.py:338).  Bit-exact with numpy's RandomState: init_genrand seeding, one 32-bit
 * draw per masked-rejection trial, descending Fisher-Yates.  The handle is a device-resident
 * generator state; successive shuffles continue the same stream, as the global numpy stream does. */
typedef struct aurppo_rng aurppo_rng;
int aurppo_mt19937_create(aurppo_rng** out, uint32_t seed, int max_n, void* stream);
int aurppo_mt19937_destroy(aurppo_rng* rng);
int aurppo_mt19937_seed(aurppo_rng* rng, uint32_t seed, void* stream);
/* Host copies of (key[624], pos) == np.random.get_state()[1:3].  These two synchronise `stream`. */
int aurppo_mt19937_get_state(aurppo_rng* rng, uint32_t* key_h, int32_t* pos_h, void* stream);
int aurppo_mt19937_set_state(aurppo_rng* rng, const uint32_t* key_h, int32_t pos_h, void* stream);
/* out[0] (device) = 1.0f if any shuffle since the last (re)seed ran out of pre-generated draws (the inventory rule
 * covers the expectation + 12 sigma of numpy's rejection sampling; beyond it the permutation is invalid and the flag
 * sticks), else 0.0f.  Enqueued on `stream`, never synchronises: the trainer folds it into the one host read it makes
 * per update (what np.random.shuffle, src/ppo.py:217, cannot fail at). */
int aurppo_mt19937_status_f32(aurppo_rng* rng, float* out, void* stream);
/* idx[i] = i  (np.arange, src/ppo.py:213) */
int aurppo_arange_i32(int32_t* idx, int n, void* stream);
/* In-place shuffle of idx[0..n), n <= max_n given at create. */
int aurppo_shuffle_i32(aurppo_rng* rng, int32_t* idx, int n, void* stream);
/* `epochs` successive shuffles of one carried array, epoch e written to out[e*n .. (e+1)*n):
 * out[0] = shuffle(arange(n)), out[e] = shuffle(out[e-1])  (src/ppo.py:213-217).               */
int aurppo_shuffle_epochs_i32(aurppo_rng* rng, int32_t* out, int n, int epochs, void* stream);

/* ---- K3: fused minibatch gather -----------------------------------------------------------
 * Replaces the advanced-indexing gathers b_obs[mb_inds], b_actions[mb_inds], b_logprobs[mb_inds],
 * b_advantages[mb_inds], b_returns[mb_inds], b_values[mb_inds] (src/ppo.py:219-220,225,236,251-257;
 * src/robot_ppo.py:341-345) with ONE launch over up to 8 streams:
 *   dst_h[s][m*row_elems_h[s] + e] = src_h[s][idx[m]*row_elems_h[s] + e],  0<=m<M.
 * src_h/dst_h/row_elems_h are HOST arrays (of device pointers / ints) of length n_streams.       */
int aurppo_gather_f32(const int32_t* idx, int M, const float* const* src_h, float* const* dst_h,
                      const int* row_elems_h, int n_streams, void* stream);

/* ---- K4+K5: advantage normalisation + clipped-surrogate loss, forward and backward ---------
 * Replaces src/ppo.py:225-264 (src/robot_ppo.py:345-398): log-ratio, ratio, KL diagnostics,
 * clip fraction, minibatch advantage normalisation (mean, unbiased std, +1e-8), policy loss,
 * value loss (vloss_mode), entropy bonus, total loss -- and their autograd:
 *   g_newlogp[m] = d loss / d newlogp[m],  g_newv[m] = d loss / d newv[m],
 *   g_entropy[m] = -ent_coef / M     (torch conventions for max ties and clamp edges).
 * clip / ent_coef / vf_coef are the Python floats of the params dict (fp64); the clip bounds are
 * formed as 1-clip, 1+clip in fp64 and rounded to fp32, as torch does.
 * out_scalars: AURPPO_N_SCALARS floats (device).  workspace: aurppo_loss_workspace_bytes(M)
 * bytes, 16-byte aligned, contents need not be initialised.                                      */
size_t aurppo_loss_workspace_bytes(int M);
int aurppo_loss_fwd_bwd_f32(const float* newlogp, const float* oldlogp, const float* adv,
                            const float* newv, const float* oldv, const float* ret,
                            const float* entropy, int M, double clip, double ent_coef, double vf_coef,
                            int norm_adv, int vloss_mode, float* out_scalars, float* g_newlogp,
                            float* g_newv, float* g_entropy, void* workspace, void* stream);

/* Same computation with the old-side inputs as a gathered (M,4) record {old_logp, adv, ret, old_v}
 * (rows of aurppo_gae_pack_f32's rec, picked by aurppo_gather_f32 with row_elems = 4).              */
int aurppo_loss_fwd_bwd_packed_f32(const float* newlogp, const float* newv, const float* entropy,
                                   const float* rec, int M, double clip, double ent_coef,
                                   double vf_coef, int norm_adv, int vloss_mode, float* out_scalars,
                                   float* g_newlogp, float* g_newv, float* g_entropy, void* workspace,
                                   void* stream);

/* ---- K7: fused minibatch step for the MLP actor-critic -----------------------------------------
 * One launch sequence replaces, for the reference's MLP policy (actor_critic over two Tanh hidden
 * layers of `hidden` units; Gaussian head with state-independent log-std when `continuous`, Categorical
 * head over A logits otherwise; src/models/actor_critic.py:8-51, src/nets/nets.py:19-53), everything
 * between "mb_inds chosen" and "gradients ready":
 *   gathers (src/ppo.py:219-220,225,236,251-257) + evaluate() (src/ppo.py:220) + the loss block
 *   (src/ppo.py:225-264) + loss.backward() (src/ppo.py:267).
 * obs (B,D), actions ((B,A) floats, or (B,) action indices stored as floats for the Categorical head)
 * and rec (B,4) = {old_logp, adv, ret, old_v} are the flattened rollout buffers, idx (M,) the minibatch slice of the epoch permutation.  `params` is the flat parameter
 * bucket, layout_h 13 float offsets into it {w1,b1,w2,b2,w3,b3} for the actor, the same for the
 * critic, then actor_logstd (ignored for the Categorical head; nn.Linear layout: weight[out][in]).  `grads` (n_params floats) is
 * OVERWRITTEN with d loss / d params in the same layout; out_scalars as aurppo_loss_fwd_bwd_f32.
 * Built for hidden = 64, two layers, D <= 64, A <= 16; other shapes return AURPPO_ESHAPE (callers then use
 * aurppo_mlp_wide_ppo_step_f32 below, or the per-op path beyond its limits).  workspace: aurppo_mlp_workspace_bytes(n_params) bytes, 16-byte aligned.      */
size_t aurppo_mlp_workspace_bytes(int n_params);
int aurppo_mlp_ppo_step_f32(const float* obs, const float* actions, const float* rec,
                            const int32_t* idx, int M, int D, int A, int continuous, int hidden,
                            const float* params, const int* layout_h, int n_params, float* grads,
                            double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                            float* out_scalars, void* workspace, void* stream);

/* Measurement variant: identical work, and the two caller-owned hipEvent_t handles (either may be NULL)
 * are recorded on `stream` immediately before and after the main kernel (k_mlp_step) -- bench.py times
 * the kernel with them (hipEventElapsedTime) without a profiler attached.                           */
int aurppo_mlp_ppo_step_ev_f32(const float* obs, const float* actions, const float* rec,
                               const int32_t* idx, int M, int D, int A, int continuous, int hidden,
                               const float* params, const int* layout_h, int n_params, float* grads, double clip,
                               double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                               float* out_scalars, void* workspace, void* stream, void* ev_begin,
                               void* ev_end);

/* ---- K7 + K6b chained: one whole minibatch of the update loop ---------------------------------------
 * Replaces src/ppo.py:219-269 for one minibatch -- everything aurppo_mlp_ppo_step_f32 does, then
 * nn.utils.clip_grad_norm_(parameters, max_norm) and optimizer.step() (Adam, as aurppo_clip_adam_f32) over
 * the same flat bucket of n_params floats (params / grads / exp_avg / exp_avg_sq), in three launches instead
 * of five.  Single-process only: there is no place for a gradient all-reduce between the halves.
 * next_idx / next_M: the index slice of the minibatch that will be stepped next (NULL: none); its advantage
 * statistics and the operand copy of the updated first layer are prepared by this call's last launch.
 * chained != 0 promises that the previous call on this workspace was this function with next_idx equal to this
 * call's idx (same M); then nothing is prepared again.  lr_dev / step_dev / out_norm as aurppo_clip_adam_f32. */
int aurppo_mlp_ppo_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M,
                                 int D, int A, int continuous, int hidden, float* params, const int* layout_h,
                                 int n_params, float* grads, double clip, double ent_coef, double vf_coef,
                                 int norm_adv, int vloss_mode, float* out_scalars, float* exp_avg,
                                 float* exp_avg_sq, double max_norm, const float* lr_dev, float* step_dev,
                                 double beta1, double beta2, double eps, float* out_norm, const int32_t* next_idx,
                                 int next_M, int chained, void* workspace, void* stream);

/* Packed records.  Every aurppo_mlp_ppo_* entry point accepts actions == NULL: rec is then (B, 16) floats per sample,
 * {old_logp, A, R, V, action row (at most 12 floats), 0 ...}, built by aurppo_pack_records_f32 from the (B, 4)
 * records of aurppo_gae_pack_f32 and the (B, action_floats) action buffer.  A sample's record and action row then
 * share one 64-B line instead of one 128-B line each: 3 lines per sample instead of 4 in K7's gather.            */
int aurppo_pack_records_f32(const float* rec4, const float* actions, int B, int action_floats, float* rec64,
                            void* stream);

/* The same minibatch in two halves, for one process per GPU (src/ppo.py:219-269 with a gradient all-reduce between
 * loss.backward() and clip_grad_norm_): aurppo_mlp_ppo_grad_f32 = aurppo_mlp_ppo_step_f32 that also advances the Adam
 * step count (step_dev) and, with chained != 0, skips the preparation the previous apply call already did;
 * aurppo_mlp_ppo_apply_f32 = clip_grad_norm_ + Adam over the bucket in ONE launch: the stored gradient is first
 * multiplied by grad_scale (1/world after a SUM all-reduce), its norm is formed inside the kernel (grads itself is
 * left as it was: other workgroups are still reading it), and -- as in
 * aurppo_mlp_ppo_minibatch_f32 -- the statistics of next_idx and the operand copy of the new first layer are
 * prepared for the next aurppo_mlp_ppo_grad_f32(chained = 1) on this workspace (rec_floats: 4, or 16 for packed
 * records, below).                                                                                           */
int aurppo_mlp_ppo_grad_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                            int A, int continuous, int hidden, const float* params, const int* layout_h, int n_params,
                            float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                            float* out_scalars, float* step_dev, int chained, void* workspace, void* stream);
int aurppo_mlp_ppo_apply_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* layout_h,
                             int n_params, int D, double grad_scale, double max_norm, const float* lr_dev,
                             const float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                             const float* rec, int rec_floats, const int32_t* next_idx, int next_M, void* workspace,
                             void* stream);

/* aurppo_mlp_ppo_apply_f32 for a gradient that is already the mean over ranks (aurppo_p2p_allreduce_mean_f32 below) and comes
 * with per-workgroup partial sums of squares: the clip's norm is their sum (n_part of them), nothing is rescaled. */
int aurppo_mlp_ppo_apply_parts_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, const int* layout_h,
                                   int n_params, int D, const double* sq_part, int n_part, double max_norm,
                                   const float* lr_dev, const float* step_dev, double beta1, double beta2, double eps,
                                   float* out_norm, const float* rec, int rec_floats, const int32_t* next_idx, int next_M,
                                   void* workspace, void* stream);

/* ---- K11: 3x3 convolution of the robot policy's hidden encoder blocks on the bf16 matrix pipe -----------------
 * nn.Conv2d(Ci, Co, 3, padding = pad) WITHOUT bias (src/nets/base_cnns.py:32-45; the bias / ReLU / max-pool tail is
 * aurppo_bias_relu_pool2_*), stride 1, NCHW fp32, as an implicit GEMM whose fp32 products are formed from three-way bf16
 * splits (fp32-equivalent).  mode 0: z = conv2d(x, w, padding = pad), x (B, Ci, H, W) -> z (B, Co, H + 2 pad - 2, W + 2 pad - 2).
 * mode 1: the gradient with respect to the input: x is the OUTPUT gradient (B, Co, H, W), z the input gradient
 * (B, Ci, H + 2 - 2 pad, W + 2 - 2 pad), w the same (Co, Ci, 3, 3) filter, pad the forward padding.  The product's input
 * channel count (Ci in mode 0, Co in mode 1) must be a multiple of 16.  wop_ws: aurppo_conv3x3_wop_bytes(input channels,
 * output channels of the product) bytes of scratch for the filter in operand order (an input channel count that is no multiple
 * of 16 -- a linear product's ragged inner dimension, below -- is rounded up to whole 16-column steps).  (The weight gradient:
 * aurppo_conv3x3_wgrad_f32.) */
size_t aurppo_conv3x3_wop_bytes(int cin_gemm, int cout_gemm);
int aurppo_conv3x3_f32(const float* x, const float* w, float* z, int B, int Ci_w, int Co_w, int H, int W, int pad, int mode,
                       void* wop_ws, void* stream);
/* K11p: a whole hidden block, nn.Conv2d(Ci, Co, 3, padding = pad) -> nn.ReLU -> nn.MaxPool2d(2), in one launch: K11's mode 0 with
 * the bias, the ReLU and the pool of aurppo_bias_relu_pool2_fwd_f32 in its epilogue, so the full-resolution pre-activation is
 * never stored.  y, mask (B, Co, (H + 2 pad - 2) / 2, (W + 2 pad - 2) / 2) (floor) hold bit for bit what that pair of calls leaves:
 * the first maximum in scan order, a NaN wins, mask = its window position 0..3 or 4 where the maximum is <= 0 (y = 0 there).
 * bias (Co) may be NULL.  wop_ws: aurppo_conv3x3_wop_bytes(Ci, Co) bytes.  Refuses what mode 0 refuses, and AURPPO_ESHAPE for a
 * map without one whole window.  The backward is aurppo_bias_relu_pool2_bwd_f32 on the mask, then K11's mode 1 and K12. */
int aurppo_conv3x3_pool_f32(const float* x, const float* w, const float* bias, float* y, uint8_t* mask, int B, int Ci, int Co,
                            int H, int W, int pad, void* wop_ws, void* stream);

/* ---- K11x: hidden activations kept as bf16 planes --------------------------------------------------------------
 * THE PLANES LAYOUT.  For an fp32 NCHW tensor x (B, C, H, W) with C a multiple of 8, its planes are
 *     uint16 xp[B][C / 8][3][H * W][8],      xp[b][g][pl][y * W + x][j] = plane pl of x[b][8 g + j][y][x]
 * where the three planes of a value a are the bf16x3 split every matrix kernel here forms in registers: a0 = bf16(a) (round to
 * nearest even), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1); a0 + a1 + a2 == a.  The 16 bytes at (b, g, pl, pixel) are the operand
 * fragment K11's lane builds for channels 8 g .. 8 g + 7 of that pixel; consecutive pixels are consecutive 16-byte pieces.  The
 * tensor is aurppo_planes_bytes(B, C, H, W) = 6 B C H W bytes (0 for a C that is no multiple of 8 or a dimension < 1) and its base
 * must be 16-byte aligned.  The split is a function of the value alone, so a kernel that READS planes multiplies the very bits the
 * fp32 kernel would have split: every result below equals its fp32 sibling's bit for bit.
 *
 * aurppo_split_planes_f32: xp = the planes of x (the layout's definition; for inputs no kernel here produced).
 * aurppo_conv3x3_planes_f32: aurppo_conv3x3_f32's mode 0 with x given as its planes.
 * aurppo_conv3x3_pool_planes_f32: aurppo_conv3x3_pool_f32 whose input is fp32 x (x_is_planes = 0) or its planes (1), and which,
 *   with yp_or_null set, also writes the planes of y -- (B, Co / 8, 3, Hp * Wp, 8), Co a multiple of 8, a dead window as the planes
 *   of 0.0f -- beside y and mask, which are written as before (the backward reads fp32).  Neither: aurppo_conv3x3_pool_f32 itself.
 * aurppo_first_block_planes_fwd_f32: aurppo_first_block_fwd_f32 (below) that also writes the planes of y.
 * All refuse before their first launch, with nothing written: AURPPO_EINVAL for a NULL or a planes pointer off its 16-byte
 * boundary, AURPPO_ESHAPE for what their fp32 siblings refuse and for planes of a channel count that is no multiple of 8. */
size_t aurppo_planes_bytes(int B, int C, int H, int W);
int aurppo_split_planes_f32(const float* x, uint16_t* xp, int B, int C, int H, int W, void* stream);
int aurppo_conv3x3_planes_f32(const uint16_t* xp, const float* w, float* z, int B, int Ci, int Co, int H, int W, int pad,
                              void* wop_ws, void* stream);
int aurppo_conv3x3_pool_planes_f32(const void* x_or_xp, int x_is_planes, const float* w, const float* bias, float* y, uint8_t* mask,
                                   uint16_t* yp_or_null, int B, int Ci, int Co, int H, int W, int pad, void* wop_ws, void* stream);

/* nn.Linear without its bias on the same arithmetic (the MLP policies wider than the fused steps cover, hidden_dim > 128:
 * src/nets/nets.py:21-27,33-39,45-51 per layer).  mode 0: y (M, N_w) = x (M, K_w) . w (N_w, K_w)^T, any K_w >= 1;
 * mode 1 (gradient with respect to the input; x is dY): y (M, K_w) = x (M, N_w) . w, N_w a multiple of 16.  Row-major fp32.
 * x must be 16-byte aligned at its base.  With K_w a multiple of 16 every row is, and a row's 16 columns of a step are two
 * 16-byte loads; any other K_w (a state of 3, 11, 17, 376 floats in a policy's first layer) takes the tail builds: rows need 4-byte
 * alignment only, every column is a load of its own that is issued only for columns < K_w, and nothing past a row's K_w
 * floats is read -- x may end at the end of a mapping.
 * wop_ws: aurppo_conv3x3_wop_bytes(inner dimension, columns) bytes. */
int aurppo_linear_f32(const float* x, const float* w, float* y, long long M, int K_w, int N_w, int mode, void* wop_ws,
                      void* stream);
/* The forward product with the layer's bias (may be NULL) and, act = 1, the nn.Tanh that follows every hidden layer
 * (src/nets/nets.py:21-27) in its epilogue: y = act(x . w^T + bias). */
int aurppo_linear_bias_act_f32(const float* x, const float* w, const float* bias, float* y, long long M, int K_w, int N_w,
                               int act, void* wop_ws, void* stream);
/* The same forward product on a tile for small M (k_linear_small): a workgroup takes 128 rows x 32 or 64 columns where
 * aurppo_linear_bias_act_f32's takes 256 x 128, so a few thousand rows reach every CU.  A row's k-steps, their order and their
 * arithmetic are unchanged: every result is bit for bit aurppo_linear_bias_act_f32's.  Forward only.
 *   aurppo_linear_small_bias_act_f32: argument list, limits, alignment and wop_ws of aurppo_linear_bias_act_f32; always the
 *     small tile, whatever M.
 *   aurppo_linear_pair_bias_act_f32: two products of one shape -- yA = act(xA . wA^T + biasA), yC = act(xC . wC^T + biasC), both
 *     weights (N_w, K_w), both inputs (M, K_w) -- in ONE launch behind the two operand copies (three launches in all): the actor's
 *     and the critic's layer of an MLP policy.  xA may be xC; each bias may be NULL; xA, xC 16-byte aligned at their bases.
 *     wop_ws: aurppo_linear_pair_wop_bytes(K_w, N_w) bytes (0 for a non-positive size), 16-byte aligned.
 * Both refuse before their first launch: AURPPO_EINVAL for a NULL pointer, an act outside {0, 1} or a misaligned x / wop_ws,
 * AURPPO_ESHAPE for M, K_w or N_w below 1. */
int aurppo_linear_small_bias_act_f32(const float* x, const float* w, const float* bias, float* y, long long M, int K_w, int N_w,
                                     int act, void* wop_ws, void* stream);
size_t aurppo_linear_pair_wop_bytes(int K_w, int N_w);
int aurppo_linear_pair_bias_act_f32(const float* xA, const float* xC, const float* wA, const float* wC, const float* biasA,
                                    const float* biasC, float* yA, float* yC, long long M, int K_w, int N_w, int act, void* wop_ws,
                                    void* stream);
/* nn.Linear's weight gradient on the same arithmetic: dw (N, K) = dy (M, N)^T . x (M, K) (what loss.backward() leaves in
 * <layer>.weight.grad, src/ppo.py:266).  Both operands are split once per workgroup through LDS; the minibatch's rows are cut
 * into slices whose partial products are summed in slice order (deterministic).  N a multiple of 4, any K >= 1; dy and x
 * 16-byte aligned at their bases.  With K a multiple of 4 the x rows are read in 16-byte pieces; any other K takes the tail
 * builds (rows 4-byte aligned, one guarded load per column, nothing read past a row's K floats).  ws:
 * aurppo_linear_wgrad_ws_bytes(M, N, K) bytes. */
size_t aurppo_linear_wgrad_ws_bytes(long long M, int N, int K);
int aurppo_linear_wgrad_f32(const float* dy, const float* x, float* dw, long long M, int N, int K, void* ws, void* stream);

/* The three products with what the layered PPO step (K13 below) needs riding in them.
 *   aurppo_linear_rows_bias_act_f32: aurppo_linear_bias_act_f32 with lane row m reading x row rows[m] -- `b_obs[mb_inds]`
 *     (src/ppo.py:219-220, the K3 gather) inside the first layer's product.  x (B, K_w), rows (M,) int32 with every entry in
 *     [0, B); y (M, N_w) stays in minibatch order.  rows == NULL: exactly aurppo_linear_bias_act_f32.
 *   aurppo_linear_wgrad_rows_f32: aurppo_linear_wgrad_f32 with the x operand read through the same index (dy is in minibatch
 *     order already); same slice rule, same aurppo_linear_wgrad_ws_bytes(M, N, K).  rows == NULL: the plain call.
 *   aurppo_linear_dx_tanh_f32: out (M, K_w) = (gz (M, N_w) . w (N_w, K_w)) * (1 - h * h), h (M, K_w) read at the address the
 *     store uses (out may be h): autograd's `grad @ W` followed by tanh_backward of the layer below, src/nets/nets.py:21-27, in one
 *     launch.  N_w a multiple of 16.
 * Alignment, limits and wop_ws as aurppo_linear_f32. */
int aurppo_linear_rows_bias_act_f32(const float* x, const int32_t* rows, const float* w, const float* bias, float* y, long long M,
                                    int K_w, int N_w, int act, void* wop_ws, void* stream);
int aurppo_linear_wgrad_rows_f32(const float* dy, const float* x, const int32_t* rows, float* dw, long long M, int N, int K, void* ws,
                                 void* stream);
int aurppo_linear_dx_tanh_f32(const float* gz, const float* w, const float* h, float* out, long long M, int K_w, int N_w,
                              void* wop_ws, void* stream);
/* aurppo_linear_wgrad_rows_f32 that also leaves the layer's bias gradient, db (N,) = the column sums of dy (what loss.backward()
 * leaves in <layer>.bias.grad, src/ppo.py:266), taken from the dy values the product's kernel holds anyway: no second pass over dy.
 * The sums are accumulated in fp64 -- per thread, across a workgroup's row groups, across the slices in slice order -- and rounded
 * to fp32 once; no floating-point atomics: two calls give the same bits.  dw is bit for bit aurppo_linear_wgrad_rows_f32's.
 * Limits and alignment as aurppo_linear_wgrad_rows_f32, except that K no multiple of 4 needs rows (AURPPO_ESHAPE with rows == NULL:
 * that build does not exist); db needs 4-byte alignment.  ws: aurppo_linear_wgrad_bias_ws_bytes(M, N, K) bytes (the partial products,
 * then the slices' partial column sums), 16-byte aligned. */
size_t aurppo_linear_wgrad_bias_ws_bytes(long long M, int N, int K);
int aurppo_linear_wgrad_bias_f32(const float* dy, const float* x, const int32_t* rows /* may be NULL */, float* dw, float* db,
                                 long long M, int N, int K, void* ws, void* stream);

/* ---- K13: heads + distribution + PPO loss + their backward for the MLP policies the fused steps do not cover -------------
 * For hidden_dim > 128 (or a state of more than 128 floats) the hidden layers of src/nets/nets.py:19-53 run a layer at a time
 * on the products above; this call is everything between the last hidden activations and the loss of one minibatch
 * (src/ppo.py:225-266): both heads' products, Normal(mean, exp(actor_logstd)) / Categorical(logits) log-prob and entropy
 * (src/models/actor_critic.py:34-51), advantage normalisation, the clipped-surrogate / value / entropy loss, and the backward
 * pass of all of it.  Three launches (advantage statistics, the kernel, a fixed-order fold); no floating-point atomics: two calls
 * on the same inputs give the same bits.
 *   hA, hC (M, H): the actor's / critic's last hidden activations (after tanh), minibatch order, 16-byte aligned.
 *   gzA, gzC (M, H): d loss / d (pre-activation of the last hidden layer), tanh' folded in.  Each may be its h (in place).
 *   actions / rec / idx: as aurppo_mlp_ppo_step_f32 -- (B, A) actions (Categorical: (B,) indices as floats) + (B, 4) records
 *     {old_logp, adv, ret, old_v}, or actions == NULL and (B, 16) packed records (aurppo_pack_records_f32); both read
 *     through idx (M,) int32.
 *   params / grads: the flat bucket and its gradient (n_params floats); layout_h: 7 float offsets {actor head weight (A, H),
 *     actor head bias, critic head weight (1, H), critic head bias, actor_logstd (ignored for the Categorical head), bias of the
 *     actor's last hidden layer, bias of the critic's}.  Written in grads: both heads' weight and bias gradients, the
 *     actor_logstd gradient, and the two last-hidden-layer bias gradients (the column sums of gz); nothing else.
 *   out_scalars: the 9 floats of AURPPO_S_*.   workspace: aurppo_head_ppo_workspace_bytes(M, H, A) bytes, 64-byte aligned.
 * Limits (AURPPO_ESHAPE otherwise): H a multiple of 32 in 32..1024, A in 1..16 (Categorical 2..16; packed records A <= 12; up to 32
 * actions: aurppo_head_ppo_wa_f32 below). */
size_t aurppo_head_ppo_workspace_bytes(int M, int H, int A);
int aurppo_head_ppo_f32(const float* hA, const float* hC, float* gzA, float* gzC, const float* actions, const float* rec,
                        const int32_t* idx, int M, int H, int A, int continuous, const float* params, const int* layout_h,
                        int n_params, float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                        float* out_scalars, void* workspace, void* stream);

/* ---- K14 and the layered rollout step: K8's contract for the MLP policies the fused kernels do not cover ------------------
 * Replaces `action, logprob, _, value = policy.evaluate(next_obs)` under no_grad and the three buffer row stores behind it
 * (src/ppo.py:104-108), and with noise == NULL the bootstrap `policy.value(next_obs)` (src/ppo.py:161), for hidden_dim > 128 or a
 * state of more than 128 floats.  The parameters stand still for the T steps of a rollout, so the operand-order copies of the
 * 2 L hidden-layer matrices are built once (aurppo_mlp_layered_prep_f32) and every step runs from them.
 *   offsets: the layered layout, as K7w's layout_h: for the actor, then the critic: {w_0, b_0, ..., w_L, b_L}, then actor_logstd --
 *     4 * (num_layers + 1) + 1 float offsets into the bucket of n_params floats; each is range-checked.
 *   wop: aurppo_mlp_layered_wop_bytes(D, hidden, num_layers) bytes (0: shape not supported), 16-byte aligned, caller-owned:
 *     aurppo_mlp_layered_prep_f32 fills it (2 L launches) and it stays valid until the parameters change.
 *   aurppo_mlp_layered_act_f32: per net L products with bias and tanh in the epilogue from the prepared copies, then K14: 2 L + 1
 *     launches; noise == NULL: the critic only, L + 1 launches, and actions / logp may be NULL.  obs (N, D) 16-byte aligned;
 *     noise (N, A) standard-normal draws (a = mu + exp(logstd) * eps) or (N,) uniform [0, 1) draws (inverse CDF of
 *     softmax(logits)); actions (N, A) | (N,), logp (N,), value (N,) go wherever the caller points them; noise and the outputs
 *     need 4-byte alignment only.  workspace: aurppo_mlp_layered_act_workspace_bytes(N, hidden) bytes, 64-byte aligned (the
 *     activations).  The log-prob is bit for bit the one aurppo_head_ppo_f32 forms from the stored action at the same parameters.
 *   aurppo_mlp_layered_act_paired_f32: the same step -- same arguments, same checks, same wop and workspace, same bits in
 *     actions, logp and value -- on the small-M products: per layer ONE launch for both nets (aurppo_linear_pair_bias_act_f32's
 *     kernel, from the prepared copies), then K14: L + 1 launches; noise == NULL: the critic alone on the single small-tile
 *     product, L + 1 launches.  For rollouts of a few thousand environments, where the step above leaves most CUs idle.
 *   aurppo_head_act_f32: K14 alone, from the last hidden activations hA, hC (N, H), 16-byte aligned (hA may be NULL without
 *     noise); layout_h: 5 float offsets {actor head weight (A, H), actor head bias, critic head weight (1, H), critic head bias,
 *     actor_logstd (ignored for the Categorical head)}.
 * Limits (AURPPO_ESHAPE otherwise): hidden / H a multiple of 32 in 32..1024, A in 1..16 (Categorical 2..16), any D >= 1 (no
 * multiple of 16: layer 0 on the tail builds of aurppo_linear_f32, its operand copy padded with zero planes to whole 16-column
 * steps; obs rows then need 4-byte alignment only, the base still 16), num_layers 1..16.  Up to 32 actions: the wa entries below. */
size_t aurppo_mlp_layered_wop_bytes(int D, int hidden, int num_layers);
int aurppo_mlp_layered_prep_f32(const float* params, const int* offsets, int n_params, int D, int hidden, int num_layers, void* wop,
                                void* stream);
size_t aurppo_mlp_layered_act_workspace_bytes(int N, int hidden);
int aurppo_mlp_layered_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                               int num_layers, const float* params, const int* offsets, int n_params, float* actions, float* logp,
                               float* value, const void* wop, void* workspace, void* stream);
int aurppo_mlp_layered_act_paired_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                      int num_layers, const float* params, const int* offsets, int n_params, float* actions,
                                      float* logp, float* value, const void* wop, void* workspace, void* stream);
int aurppo_head_act_f32(const float* hA, const float* hC, const float* noise, int N, int H, int A, int continuous,
                        const float* params, const int* layout_h, int n_params, float* actions, float* logp, float* value,
                        void* stream);

/* ---- the layered update step: aurppo_mlp_ppo_step_f32's contract for the MLP policies the fused steps do not cover ---------
 * One minibatch of src/ppo.py:219-266 (gather, policy.evaluate, the loss, loss.backward()) for hidden_dim > 128 or a state of more
 * than 128 floats, in one call that owns its launch sequence: per net layer 0 through idx and layers 1 .. L - 1
 * (aurppo_linear_rows_bias_act_f32 / aurppo_linear_bias_act_f32, tanh in the epilogue), K13 (aurppo_head_ppo_f32, in place of the
 * last activations), then per net from the last layer down the weight gradient and aurppo_linear_dx_tanh_f32.  The weight gradient
 * of every layer below the last is aurppo_linear_wgrad_bias_f32 (layer 0 through idx), which leaves that layer's bias gradient; K13
 * writes the last layers'.  12 L - 1 launches on the caller's stream; no allocation, no host synchronisation (capturable into a
 * hipGraph); no floating-point atomics: two calls give the same bits.
 *   obs / actions / rec / idx, the loss knobs and out_scalars: as aurppo_mlp_ppo_step_f32 (the three record forms: actions + (B, 4)
 *     records, Categorical indices + records, or actions == NULL and (B, 16) packed records).  obs and rec 16-byte aligned.
 *   offsets: the layered layout as aurppo_mlp_layered_act_f32 takes it, 4 * (num_layers + 1) + 1 entries, each range-checked.
 *   grads: [0, n_params) is overwritten -- every float of it that belongs to the policy -- and nothing past it.
 *   workspace: aurppo_mlp_layered_step_workspace_bytes(M, D, A, hidden, num_layers) bytes (0: shape not supported), 64-byte aligned,
 *     caller-owned: the 2 L activation arrays, the operand copy, the weight-gradient slices, K13's workspace and clip + Adam's.  A
 *     smaller buffer cannot be told from a bare pointer: the size function is the contract.
 *   aurppo_mlp_layered_minibatch_f32: the step, then aurppo_clip_adam_f32's two launches over [0, n_params) (clip_n = n_params) on
 *     the same stream -- src/ppo.py:219-269 -- with the same bits in params, moments, step count and norm as the two calls in turn.
 *     Single process only: nothing all-reduces the gradient in between.
 * Limits (AURPPO_ESHAPE before any launch otherwise): M >= 1, any D >= 1, hidden a multiple of 32 in 32..1024, A in 1..16
 * (Categorical 2..16; packed records A <= 12), num_layers 1..16.  Up to 32 actions: the wa entries below. */
size_t aurppo_mlp_layered_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers);
int aurppo_mlp_layered_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A,
                                int continuous, int hidden, int num_layers, const float* params, const int* offsets, int n_params,
                                float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                                float* out_scalars, void* workspace, void* stream);
int aurppo_mlp_layered_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                                     int A, int continuous, int hidden, int num_layers, float* params, const int* offsets,
                                     int n_params, float* grads, double clip, double ent_coef, double vf_coef, int norm_adv,
                                     int vloss_mode, float* out_scalars, float* exp_avg, float* exp_avg_sq, double max_norm,
                                     const float* lr_dev, float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                     void* workspace, void* stream);

/* ---- the layered steps at any hidden width ----------------------------------------------------------------------------------
 * The entries above refuse a hidden width that is no multiple of 32 (-d 200, 300, 400, 500; 100 over Humanoid's 376 state floats).
 * Each entry below takes the argument list of its sibling, unchanged, the same checks and the same limits, but any hidden width in
 * 1..1024: `hidden` is the bucket's width -- offsets and n_params are the unpadded policy's -- and the step runs as the policy of
 * width Hp = 32 * ceil(hidden / 32) whose extra weights and biases are zero.  That is exact (a pad unit's pre-activation is 0,
 * tanh(0) is exactly 0 as the kernels form it, its outgoing weights are zero planes), the pad entries exist in neither bucket, and
 * nothing is written for them: grads gets its [0, n_params) and nothing else.  Results are bit for bit those of the Hp-wide
 * zero-padded policy through the sibling entry, and at hidden % 32 == 0 each entry IS its sibling.
 *   wop: aurppo_mlp_layered_anyh_wop_bytes(D, hidden, num_layers) = the sibling's figure at Hp (the padded operand copies);
 *     workspaces likewise: the activation planes are (rows, Hp).  All three size functions return 0 outside 1..1024.
 *   Launch counts are the siblings': prep 2 L, act 2 L + 1 (paired: L + 1), step 12 L - 1, minibatch two more.
 *   A buffer prepared by aurppo_mlp_layered_anyh_prep_f32 goes to the anyh act entries only. */
size_t aurppo_mlp_layered_anyh_wop_bytes(int D, int hidden, int num_layers);
int aurppo_mlp_layered_anyh_prep_f32(const float* params, const int* offsets, int n_params, int D, int hidden, int num_layers, void* wop,
                                     void* stream);
size_t aurppo_mlp_layered_anyh_act_workspace_bytes(int N, int hidden);
int aurppo_mlp_layered_anyh_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                    int num_layers, const float* params, const int* offsets, int n_params, float* actions, float* logp,
                                    float* value, const void* wop, void* workspace, void* stream);
int aurppo_mlp_layered_anyh_act_paired_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                           int num_layers, const float* params, const int* offsets, int n_params, float* actions,
                                           float* logp, float* value, const void* wop, void* workspace, void* stream);
size_t aurppo_mlp_layered_anyh_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers);
int aurppo_mlp_layered_anyh_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A,
                                     int continuous, int hidden, int num_layers, const float* params, const int* offsets, int n_params,
                                     float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                                     float* out_scalars, void* workspace, void* stream);
int aurppo_mlp_layered_anyh_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                                          int A, int continuous, int hidden, int num_layers, float* params, const int* offsets,
                                          int n_params, float* grads, double clip, double ent_coef, double vf_coef, int norm_adv,
                                          int vloss_mode, float* out_scalars, float* exp_avg, float* exp_avg_sq, double max_norm,
                                          const float* lr_dev, float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                          void* workspace, void* stream);

/* ---- K13, K14 and the layered steps with up to 32 actions ---------------------------------------------------------------------
 * The entries above refuse more than 16 actions (Humanoid's 17, the dexterous hands' 20 - 30, a Categorical head of 17 - 32
 * choices).  Each `wa` (wide action head) entry below takes the argument list of the sibling named, unchanged, and the same checks,
 * with A in 1..32 (Categorical 2..32).  A in 17..32 runs K13 / K14's builds with 32-long per-action arrays (the head weights in
 * LDS: up to 33 x 1024 floats); A <= 16 runs the very kernels the sibling runs: same bits, same workspace bytes.
 *   aurppo_head_ppo_wa_workspace_bytes / aurppo_head_ppo_wa_f32 / aurppo_head_act_wa_f32: as aurppo_head_ppo_workspace_bytes /
 *     aurppo_head_ppo_f32 / aurppo_head_act_f32 (H a multiple of 32 in 32..1024).
 *   aurppo_mlp_layered_wa_*: as aurppo_mlp_layered_anyh_* -- any hidden width in 1..1024, so the two widenings compose.  The operand
 *     copies and the rollout workspace do not depend on A: use aurppo_mlp_layered_anyh_wop_bytes / _prep_f32 / _act_workspace_bytes.
 * Limits (AURPPO_ESHAPE before any launch otherwise, the message names A=<n>): A in 1..32 (Categorical 2..32); packed records hold
 * at most 12 action floats, so a Gaussian head with A > 12 needs `actions`; everything else as the sibling's. */
size_t aurppo_head_ppo_wa_workspace_bytes(int M, int H, int A);
int aurppo_head_ppo_wa_f32(const float* hA, const float* hC, float* gzA, float* gzC, const float* actions, const float* rec,
                           const int32_t* idx, int M, int H, int A, int continuous, const float* params, const int* layout_h,
                           int n_params, float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                           float* out_scalars, void* workspace, void* stream);
int aurppo_head_act_wa_f32(const float* hA, const float* hC, const float* noise, int N, int H, int A, int continuous,
                           const float* params, const int* layout_h, int n_params, float* actions, float* logp, float* value,
                           void* stream);
size_t aurppo_mlp_layered_wa_step_workspace_bytes(int M, int D, int A, int hidden, int num_layers);
int aurppo_mlp_layered_wa_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D, int A,
                                   int continuous, int hidden, int num_layers, const float* params, const int* offsets, int n_params,
                                   float* grads, double clip, double ent_coef, double vf_coef, int norm_adv, int vloss_mode,
                                   float* out_scalars, void* workspace, void* stream);
int aurppo_mlp_layered_wa_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M, int D,
                                        int A, int continuous, int hidden, int num_layers, float* params, const int* offsets,
                                        int n_params, float* grads, double clip, double ent_coef, double vf_coef, int norm_adv,
                                        int vloss_mode, float* out_scalars, float* exp_avg, float* exp_avg_sq, double max_norm,
                                        const float* lr_dev, float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                        void* workspace, void* stream);
int aurppo_mlp_layered_wa_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                  int num_layers, const float* params, const int* offsets, int n_params, float* actions, float* logp,
                                  float* value, const void* wop, void* workspace, void* stream);
int aurppo_mlp_layered_wa_act_paired_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                                         int num_layers, const float* params, const int* offsets, int n_params, float* actions,
                                         float* logp, float* value, const void* wop, void* workspace, void* stream);

/* K12 -- the weight gradient of the 3x3 convolution of aurppo_conv3x3_f32 (src/nets/base_cnns.py:32-45, src/nets/equiv.py:12-62;
 * what loss.backward() leaves in <conv>.weight.grad, src/robot_ppo.py:389): dw (Co, Ci, 3, 3) from x (B, Ci, H, W) and the
 * output gradient dy (B, Co, H + 2 pad - 2, W + 2 pad - 2), NCHW fp32, as a product over the batch's output pixels on bf16 MFMAs
 * over three-way splits (fp32-equivalent).  ws: aurppo_conv3x3_wgrad_ws_bytes(...) bytes (0 = shape not supported: pad outside
 * 0..2, an empty output, or one image of either tensor of 1 GB and more). */
size_t aurppo_conv3x3_wgrad_ws_bytes(int B, int Ci, int Co, int H, int W, int pad);
int aurppo_conv3x3_wgrad_f32(const float* dy, const float* x, float* dw, int B, int Ci, int Co, int H, int W, int pad, void* ws,
                             void* stream);

/* K11n / K12n -- the narrow builds of K11's mode 1 and of K12 for the first hidden block of the encoder, nn.Conv2d(16, 32, 3,
 * padding=1) (src/nets/base_cnns.py:32-33), whose gradients fill half of K11's 32-channel blocks and 28 % of K12's smallest tile:
 * the same arithmetic (three bf16 planes per fp32 operand, six products, fp32 accumulation) in 16 x 16 x 32 matrix blocks.  NCHW fp32;
 * H x W is the map of x / dx, pad the FORWARD padding (0..2), dy (B, Co, H + 2 pad - 2, W + 2 pad - 2), w (Co, Ci, 3, 3).
 * K11n: dx (B, Ci, H, W) = d conv2d(x, w, padding = pad) / d x applied to dy; Ci in 1..16, Co a positive multiple of 32.
 * wop_ws: aurppo_conv3x3_dgrad_narrow_wop_bytes(Ci, Co) bytes, 16-byte aligned (0 = channel counts outside the class).
 * K12n: dw (Co, Ci, 3, 3) from dy and x (B, Ci, H, W); Co in 1..32, Ci in 1..16; a deterministic split over the batch's pixels whose
 * partial filters live in ws: aurppo_conv3x3_wgrad_narrow_ws_bytes(...) bytes, 16-byte aligned (0 = shape not taken: outside the
 * class, an empty output, or one image of either tensor of 1 GB and more).  No atomics: a second call leaves the same bits.
 * Both refuse (AURPPO_EINVAL: null pointer, unaligned workspace; AURPPO_ESHAPE: the shape) before their first launch. */
size_t aurppo_conv3x3_dgrad_narrow_wop_bytes(int Ci, int Co);
int aurppo_conv3x3_dgrad_narrow_f32(const float* dy, const float* w, float* dx, int B, int Ci, int Co, int H, int W, int pad,
                                    void* wop_ws, void* stream);
size_t aurppo_conv3x3_wgrad_narrow_ws_bytes(int B, int Ci, int Co, int H, int W, int pad);
int aurppo_conv3x3_wgrad_narrow_f32(const float* dy, const float* x, float* dw, int B, int Ci, int Co, int H, int W, int pad,
                                    void* ws, void* stream);

/* ---- one-shot gradient all-reduce over peer memory (one process per GPU; SURVEY 8e plan B) ------------------
 * Where it sits in the reference: between loss.backward() and clip_grad_norm_ (src/ppo.py:266-268); upstream is
 * single-process, so there is no call to cite -- the semantics are "mean of the ranks' gradients, identical bits on
 * every rank".  An aurppo_p2p handle owns one exchange buffer (two slots of max_floats + flags) on the CURRENT device.
 * Set-up, once, host side:  create on every rank -> get_handle (aurppo_p2p_handle_bytes() bytes) -> exchange the handles
 * between the processes by any means (the trainer uses torch.distributed.all_gather_object) -> open_peers(handles of all
 * ranks, in rank order; the own entry is ignored).  HSA_ENABLE_IPC_MODE_LEGACY=0 must be in every rank's environment.
 * aurppo_p2p_allreduce_mean_f32: grads[0..n) <- mean over ranks, summed in rank order (bit-identical everywhere), in ONE
 * launch and one hop over xGMI; sq_part (optional, aurppo_p2p_parts(n) doubles) receives per-workgroup partial sums of
 * squares of the result.  step_dev: a device float holding the exchange's sequence number -- Adam's step count -- which
 * every rank must advance identically by exactly one between calls (aurppo_mlp_ppo_grad_f32 does).  Capturable into a
 * hipGraph.  A peer that does not arrive within timeout_s (<= 0: 10 s) raises a sticky status instead of hanging.      */
typedef struct aurppo_p2p aurppo_p2p;
int aurppo_p2p_handle_bytes(void);
int aurppo_p2p_parts(int n);
int aurppo_p2p_create(aurppo_p2p** out, int rank, int world, int max_floats, void* stream);
int aurppo_p2p_get_handle(aurppo_p2p* x, void* handle_h);
int aurppo_p2p_open_peers(aurppo_p2p* x, const void* handles_h);
int aurppo_p2p_allreduce_mean_f32(aurppo_p2p* x, float* grads, int n, const float* step_dev, double* sq_part,
                                  double timeout_s, void* stream);
int aurppo_p2p_status(aurppo_p2p* x, int* status_h, void* stream); /* 0 ok; 1 + r: rank r's flag timed out (sticky) */
int aurppo_p2p_destroy(aurppo_p2p* x);

/* ---- K8: rollout step for the MLP actor-critic -----------------------------------------------------
 * Replaces `action, logprob, _, value = policy.evaluate(next_obs)` under no_grad and the three buffer row
 * stores that follow it (src/ppo.py:104-108), and with noise == NULL the bootstrap `policy.value(next_obs)`
 * (src/ppo.py:161).  obs (N,D); noise: (N,A) standard-normal draws for the Gaussian head (a = mu +
 * exp(logstd)*eps) or (N,) uniform [0,1) draws for the Categorical head (inverse CDF of softmax(logits));
 * outputs go wherever the caller points them -- normally rows of the rollout buffer: actions (N,A) | (N,),
 * logp (N,), value (N,).  params / layout_h / n_params / shape limits as aurppo_mlp_ppo_step_f32.       */
int aurppo_mlp_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                       const float* params, const int* layout_h, int n_params, float* actions, float* logp,
                       float* value, void* stream);

/* ---- K15 / K16: CartPole-v1 on the device, and a whole rollout on it in one launch ------------------------------------
 * The env the reference CLI defaults to (src/run_ppo.py --gym_id CartPole-v1), stepped by gym's SyncVectorEnv on the host
 * every rollout step (src/ppo.py:66-68,110).  Env state, caller-owned device memory for N envs: state (N,4) fp64 (gym keeps
 * fp64 and hands out fp32 observations), steps (N,) and episode (N,) int32.  A reset draw is Philox4x32-10 on the counter
 * (env0 + n, episode, 0, 0) under the key (seed_lo, seed_hi); component j = -0.05 + 0.1 * ((word_j >> 8) * 2^-24).  The
 * dynamics' constants (gravity .. x_lim, max_steps) arrive as arguments: CartPoleVecEnv's class attributes (envs.py).
 *
 * aurppo_cartpole_reset replaces `envs.reset(seed=...)` (src/ppo.py:188): episode = 0, steps = 0, the state from the draw,
 *   obs (N,4) = (float)state.
 * aurppo_cartpole_step (K15) replaces `envs.step(action.cpu().numpy())` (src/ppo.py:110) with gym's auto-reset and
 *   RecordEpisodeStatistics (src/ppo.py:88): action (N,) fp32 0.0 / 1.0 as K8 writes it; the Euler step in fp64; steps += 1;
 *   done = |x| > x_lim or |theta| > theta_lim or steps >= max_steps.  Where done: ep_len[n] = steps (else 0; CartPole's
 *   return equals its length), episode += 1, the state from the next draw, steps = 0.  Writes obs (the reset observation
 *   where done), reward = 1, done as 0.0 / 1.0.
 * aurppo_cartpole_rollout_f32 (K16) replaces the T steps of src/ppo.py:201-205 for K8's shape alone (hidden == 64,
 *   num_layers == 2, D == 4, A == 2, continuous == 0; anything else: AURPPO_ESHAPE): per step t the rows states[t] /
 *   terminals[t] from the current observation / done flag, aurppo_mlp_act_f32 on noise[t] into actions[t] / logp[t] /
 *   values[t], K15 into rewards[t] / ep_len[t].  obs_io (N,4) / done_io (N,): in, the current observation and done flag (what
 *   the last reset / step left); out, those after step T - 1.  The env state is updated in place.  noise (T,N) uniform
 *   [0,1); states (T,N,4); every other row table (T,N).  Bit for bit what T x (aurppo_mlp_act_f32, aurppo_cartpole_step)
 *   leave.  params / layout_h / n_params as aurppo_mlp_act_f32 (the twelve weight / bias offsets).                        */
int aurppo_cartpole_reset(double* state, int32_t* steps, int32_t* episode, float* obs, int N, int env0, uint32_t seed_lo,
                          uint32_t seed_hi, void* stream);
int aurppo_cartpole_step(double* state, int32_t* steps, int32_t* episode, const float* action, float* obs, float* reward,
                         float* done, int32_t* ep_len, int N, int env0, uint32_t seed_lo, uint32_t seed_hi, double gravity,
                         double masscart, double masspole, double length, double force_mag, double tau, double theta_lim,
                         double x_lim, int max_steps, void* stream);
int aurppo_cartpole_rollout_f32(double* state, int32_t* steps, int32_t* episode, float* obs_io, float* done_io,
                                const float* noise, int N, int T, int D, int A, int continuous, int hidden, int num_layers,
                                const float* params, const int* layout_h, int n_params, float* states, float* terminals,
                                float* actions, float* logp, float* values, float* rewards, int32_t* ep_len, int env0,
                                uint32_t seed_lo, uint32_t seed_hi, double gravity, double masscart, double masspole,
                                double length, double force_mag, double tau, double theta_lim, double x_lim, int max_steps,
                                void* stream);

/* ---- K17 / K18: Pendulum-v1 on the device behind the continuous wrapper chain, and a whole rollout on it in one launch ----
 * The env of the reference CLI's Gaussian route (src/run_ppo.py --gym_id Pendulum-v1 -c true) behind src/ppo.py:85-99's
 * wrappers, per env as SyncVectorEnv over wrapped envs has them: RecordEpisodeStatistics, ClipAction, NormalizeObservation,
 * clip +-10, NormalizeReward (its own gamma 0.99), clip +-10 -- gym 0.26.2's arithmetic in fp64, PendulumVecEnv's formulas
 * (envs.py) operation for operation.  Env state, caller-owned device memory for N envs: steps (N,) and episode (N,) int32 and
 * state (N,16) fp64, a row being
 *   [0] th  [1] thdot  [2..4] observation mean  [5..7] observation var  [8] observation count
 *   [9] return mean  [10] return var  [11] return count  [12] the reward wrapper's discounted return
 *   [13] the running episode's raw return  [14..15] spare (a reset writes 0, nothing else touches them).
 * A reset draw is Philox4x32-10 on the counter (env0 + n, episode, 1, 0) under the key (seed_lo, seed_hi), u_j = (word_j >> 8)
 * * 2^-24: th = -pi + 2 pi u_0, thdot = -1 + 2 u_1.  The dynamics' constants (g, m, l, dt, max_speed, max_torque, max_steps)
 * arrive as arguments: PendulumVecEnv's class attributes.
 *
 * aurppo_pendulum_reset starts every env over: episode = 0, steps = 0, the state from the draw, both sets of statistics at
 *   (mean 0, var 1, count 1e-4), both returns 0; the statistics take the first raw observation and obs (N,3) is its normalised form.
 * aurppo_pendulum_step (K17): action (N,) fp32, the unclipped sample (clipped to +-max_torque inside); the core step; steps += 1;
 *   done = steps >= max_steps (a truncation; there is no termination).  The observation statistics take the raw fp32 observation
 *   [cos th, sin th, thdot]; where done: ep_len[n] = steps and ep_ret[n] = the raw return in fp32 (else both 0), episode += 1, the
 *   state from the next draw, steps = 0, and the statistics take the reset observation too.  Writes obs (N,3) = clip((x - mean) /
 *   sqrt(var + 1e-8), +-10) of the observation handed out, reward = clip(r / sqrt(return var + 1e-8), +-10), done as 0.0 / 1.0.
 * aurppo_pendulum_rollout_f32 (K18) is aurppo_cartpole_rollout_f32 for K8's Gaussian build (hidden == 64, num_layers == 2,
 *   D == 3, A == 1, continuous != 0; anything else: AURPPO_ESHAPE): noise (T,N,1) standard normal; states (T,N,3); actions
 *   (T,N,1); ep_ret (T,N) fp32 beside ep_len, meaningful where ep_len > 0; every other row table (T,N).  Bit for bit what T x
 *   (aurppo_mlp_act_f32, aurppo_pendulum_step) leave.  layout_h: the thirteen offsets (actor_logstd last).                    */
int aurppo_pendulum_reset(double* state, int32_t* steps, int32_t* episode, float* obs, int N, int env0, uint32_t seed_lo,
                          uint32_t seed_hi, void* stream);
int aurppo_pendulum_step(double* state, int32_t* steps, int32_t* episode, const float* action, float* obs, float* reward,
                         float* done, int32_t* ep_len, float* ep_ret, int N, int env0, uint32_t seed_lo, uint32_t seed_hi,
                         double g, double m, double l, double dt, double max_speed, double max_torque, int max_steps,
                         void* stream);
int aurppo_pendulum_rollout_f32(double* state, int32_t* steps, int32_t* episode, float* obs_io, float* done_io,
                                const float* noise, int N, int T, int D, int A, int continuous, int hidden, int num_layers,
                                const float* params, const int* layout_h, int n_params, float* states, float* terminals,
                                float* actions, float* logp, float* values, float* rewards, int32_t* ep_len, float* ep_ret,
                                int env0, uint32_t seed_lo, uint32_t seed_hi, double g, double m, double l, double dt,
                                double max_speed, double max_torque, int max_steps, void* stream);

/* ---- K7w / K8w:the same two operators for the other MLP shapes of the reference's CLI --------------------------------
 * src/run_ppo.py:33,37 expose -d/--hidden_dim and -nl/--num_layers and src/nets/nets.py:19-53 builds any of them:
 * `num_layers` (1..3) Tanh layers of `hidden` (1..128) units over a state of D (1..128) floats, A <= 16.  Same
 * arguments and results as aurppo_mlp_ppo_step_ev_f32 / aurppo_mlp_act_f32 except
 *   layout_h: for the actor, then the critic: {w_0, b_0, ..., w_L, b_L} (L = num_layers; layer L is the head), then
 *             actor_logstd -- 4 * (num_layers + 1) + 1 float offsets into the bucket;
 *   workspace: aurppo_mlp_wide_workspace_bytes(n_params, hidden, D) bytes, 64-byte aligned (slab region sized from the
 *             shape); the act entry point only keeps the operand-order copy of the weights there and is content with
 *             aurppo_mlp_wide_workspace_bytes(0, hidden, D).
 * ev_begin / ev_end (either may be NULL): hipEvent_t handles recorded around the main kernel.  The optimizer step that
 * follows is aurppo_clip_adam_f32 (K6b).                                                                              */
size_t aurppo_mlp_wide_workspace_bytes(int n_params, int hidden, int state_dim);
int aurppo_mlp_wide_ppo_step_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx, int M,
                                 int D, int A, int continuous, int hidden, int num_layers, const float* params,
                                 const int* layout_h, int n_params, float* grads, double clip, double ent_coef,
                                 double vf_coef, int norm_adv, int vloss_mode, float* out_scalars, void* workspace,
                                 void* stream, void* ev_begin, void* ev_end);
/* The step chained with clip_grad_norm_ + Adam.step over the same flat bucket (src/ppo.py:219-269 for one minibatch), as
 * aurppo_mlp_ppo_minibatch_f32 is for the default shape -- four launches (prepare, step, slab reduce that also leaves
 * the clip's partial sums and advances the step count, clip + Adam).  next_idx / next_M: the index slice the NEXT call
 * will step (NULL: none) -- the optimizer launch then also drops every updated weight into the operand-order copies and
 * forms that slice's advantage statistics; chained != 0: the previous call named this idx as its next_idx, so this call
 * has no prepare launch (three launches).  Single process only.                                                        */
int aurppo_mlp_wide_ppo_minibatch_f32(const float* obs, const float* actions, const float* rec, const int32_t* idx,
                                      int M, int D, int A, int continuous, int hidden, int num_layers, float* params,
                                      const int* layout_h, int n_params, float* grads, double clip, double ent_coef,
                                      double vf_coef, int norm_adv, int vloss_mode, float* out_scalars,
                                      float* exp_avg, float* exp_avg_sq, double max_norm, const float* lr_dev,
                                      float* step_dev, double beta1, double beta2, double eps, float* out_norm,
                                      const int32_t* next_idx, int next_M, int chained, void* workspace, void* stream);
int aurppo_mlp_wide_act_f32(const float* obs, const float* noise, int N, int D, int A, int continuous, int hidden,
                            int num_layers, const float* params, const int* layout_h, int n_params, float* actions,
                            float* logp, float* value, void* workspace, void* stream);

/* ---- K6: global-norm gradient clip over one flat bucket -------------------------------------
 * Replaces nn.utils.clip_grad_norm_(params, max_norm) (src/ppo.py:268; src/robot_ppo.py:401):
 * norm = ||g||_2, g *= min(1, max_norm / (norm + 1e-6)).  out_norm: 1 float (device), the
 * pre-clip norm.  workspace: aurppo_clip_workspace_bytes(n) bytes.                               */
size_t aurppo_clip_workspace_bytes(int64_t n);
int aurppo_grad_norm_clip_f32(float* flat_grads, int64_t n, double max_norm, float* out_norm,
                              void* workspace, void* stream);

/* K6b: clip + Adam fused over the flat bucket -- clip_grad_norm_ over the first clip_n elements
 * (src/ppo.py:268 clips everything, clip_n = n; src/robot_ppo.py:401 the actor's slice only) followed
 * by torch.optim.Adam's step (src/ppo.py:80,269; betas, eps as given) on all n elements.  lr_dev and
 * step_dev are 1-float DEVICE scalars: the learning rate (so an annealed rate works under hipGraph
 * replay) and the step counter, which this call increments.  exp_avg / exp_avg_sq are the moment
 * buffers (n floats each, zero-initialised by the caller).  workspace: aurppo_clip_workspace_bytes(n). */
int aurppo_clip_adam_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                         int64_t clip_n, double max_norm, const float* lr_dev, float* step_dev,
                         double beta1, double beta2, double eps, float* out_norm, void* workspace,
                         void* stream);

/* ---- K9: bias + gripper-state plane + ReLU + 2x2 max-pool, fused (robot policy encoder) -----------------------
 * Replaces, behind each convolution of the plain-CNN encoder (src/nets/base_cnns.py:28-45), the convolution's bias
 * add, `nn.ReLU` and `nn.MaxPool2d(2)`, and for the first block the tiled gripper-state input channel of
 * src/models/robot_actor_critic.py:58-59,106-107 (convolution is linear in its input channels: the tiled plane
 * contributes scale[b] * plane[c,h,w], plane = conv(ones, W[:, state channel])).
 *   forward:  y[b,c,ho,wo] = max(0, max over the 2x2 window of  x + bias[c] + scale[b]*plane[c,h,w])
 *             mask = window position of the FIRST maximum (0..3, row-major, torch's tie rule), 4 if it is <= 0
 *   backward: dx = dy routed to the masked position (zero elsewhere, zero on an odd trailing row / column),
 *             dbias_part[b*C + c] = sum of dy over that plane's live pooled elements (sum over b gives d bias)
 * x, dx: (B,C,H,W) contiguous; y, dy, mask: (B,C,H/2,W/2) (floor).  bias (C), scale (B) + plane (C,H,W) may be NULL
 * (scale and plane together).  aurppo_weighted_batch_sum_f32: out[k] = sum_b w[b] * x[b,k] -- the gradient of `plane`
 * from dx and scale. */
int aurppo_bias_relu_pool2_fwd_f32(const float* x, const float* bias, const float* scale, const float* plane, float* y,
                                   uint8_t* mask, int B, int C, int H, int W, void* stream);
int aurppo_bias_relu_pool2_bwd_f32(const float* dy, const uint8_t* mask, float* dx, float* dbias_part, int B, int C,
                                   int H, int W, void* stream);
int aurppo_weighted_batch_sum_f32(const float* x, const float* w, float* out, int B, int64_t K, void* stream);

/* ---- K10: the encoder's first block in one kernel ----------------------------------------------------------------
 * conv2d(cat[obs, tiled state], W, bias, padding 1) -> ReLU -> MaxPool2d(2) of src/nets/base_cnns.py:28-31 on the input
 * of src/models/robot_actor_critic.py:58-59,106-107, without the full-resolution tensors: forward reads obs (B,Ci,H,W),
 * Ci in 1..3, W (Co, Ci+1, 3, 3) whose LAST input channel is the state plane, bias (Co, may be NULL), state (B) and
 * writes y, mask (B,Co,H/2,W/2) with K9's conventions.  Backward leaves, per (sample, group of 16 output channels),
 * partial sums dw_part (B*Co/16, 16, (Ci+1)*9) and db_part (B*Co/16, 16): summed over the first dimension and laid out
 * per channel they are the gradients of W (Co, Ci+1, 3, 3) and bias.  The input takes no gradient (it is data).  Co must
 * be a multiple of 16, W at least 3. */
int aurppo_first_block_fwd_f32(const float* obs, const float* w, const float* bias, const float* state, float* y,
                               uint8_t* mask, int B, int Ci, int Co, int H, int W, void* stream);
/* ... and y's planes (K11x above: uint16 yp[B][Co / 8][3][(H / 2) * (W / 2)][8], 16-byte aligned) beside y and mask */
int aurppo_first_block_planes_fwd_f32(const float* obs, const float* w, const float* bias, const float* state, float* y,
                                      uint8_t* mask, uint16_t* yp, int B, int Ci, int Co, int H, int W, void* stream);
int aurppo_first_block_bwd_f32(const float* dy, const uint8_t* mask, const float* obs, const float* state,
                               float* dw_part, float* db_part, int B, int Ci, int Co, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* AURPPO_H */
