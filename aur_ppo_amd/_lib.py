"""ctypes binding of libaurppo_hip.so: ``_declare`` mirrors include/aurppo.h one to one (tests/test_abi_signatures.py checks it)."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaurppo_hip.so")

# every symbol include/aurppo.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = (
    "aurppo_version", "aurppo_last_error", "aurppo_device_count", "aurppo_k7_variant", "aurppo_reload_knobs", "aurppo_k7w_kernel", "aurppo_gae_f32", "aurppo_gae_pack_f32",
    "aurppo_mt19937_create", "aurppo_mt19937_destroy", "aurppo_mt19937_seed", "aurppo_mt19937_get_state",
    "aurppo_mt19937_set_state", "aurppo_mt19937_status_f32", "aurppo_arange_i32", "aurppo_shuffle_i32", "aurppo_shuffle_epochs_i32",
    "aurppo_gather_f32", "aurppo_loss_workspace_bytes", "aurppo_loss_fwd_bwd_f32", "aurppo_loss_fwd_bwd_packed_f32",
    "aurppo_clip_workspace_bytes", "aurppo_grad_norm_clip_f32", "aurppo_mlp_workspace_bytes", "aurppo_mlp_ppo_step_f32",
    "aurppo_mlp_ppo_step_ev_f32", "aurppo_mlp_ppo_minibatch_f32", "aurppo_mlp_ppo_grad_f32", "aurppo_mlp_ppo_apply_f32", "aurppo_mlp_ppo_apply_parts_f32", "aurppo_p2p_handle_bytes", "aurppo_p2p_parts", "aurppo_p2p_create",
    "aurppo_p2p_get_handle", "aurppo_p2p_open_peers", "aurppo_p2p_allreduce_mean_f32", "aurppo_p2p_status", "aurppo_p2p_destroy", "aurppo_pack_records_f32", "aurppo_mlp_act_f32", "aurppo_clip_adam_f32",
    "aurppo_bias_relu_pool2_fwd_f32", "aurppo_bias_relu_pool2_bwd_f32", "aurppo_weighted_batch_sum_f32",
    "aurppo_first_block_fwd_f32", "aurppo_first_block_bwd_f32", "aurppo_conv3x3_wop_bytes", "aurppo_conv3x3_f32", "aurppo_linear_f32", "aurppo_linear_bias_act_f32",
    "aurppo_linear_wgrad_ws_bytes", "aurppo_linear_wgrad_f32", "aurppo_conv3x3_wgrad_ws_bytes", "aurppo_conv3x3_wgrad_f32",
    "aurppo_mlp_wide_workspace_bytes", "aurppo_mlp_wide_ppo_step_f32", "aurppo_mlp_wide_ppo_minibatch_f32",
    "aurppo_mlp_wide_act_f32", "aurppo_linear_rows_bias_act_f32", "aurppo_linear_wgrad_rows_f32", "aurppo_linear_dx_tanh_f32",
    "aurppo_head_ppo_workspace_bytes", "aurppo_head_ppo_f32",
    "aurppo_mlp_layered_wop_bytes", "aurppo_mlp_layered_prep_f32", "aurppo_mlp_layered_act_workspace_bytes", "aurppo_mlp_layered_act_f32",
    "aurppo_head_act_f32",
    "aurppo_linear_wgrad_bias_ws_bytes", "aurppo_linear_wgrad_bias_f32", "aurppo_mlp_layered_step_workspace_bytes",
    "aurppo_mlp_layered_step_f32", "aurppo_mlp_layered_minibatch_f32",
    "aurppo_conv3x3_pool_f32",
    "aurppo_conv3x3_dgrad_narrow_wop_bytes", "aurppo_conv3x3_dgrad_narrow_f32", "aurppo_conv3x3_wgrad_narrow_ws_bytes",
    "aurppo_conv3x3_wgrad_narrow_f32",
    "aurppo_planes_bytes", "aurppo_split_planes_f32", "aurppo_conv3x3_planes_f32", "aurppo_conv3x3_pool_planes_f32",
    "aurppo_first_block_planes_fwd_f32",
    "aurppo_linear_small_bias_act_f32", "aurppo_linear_pair_wop_bytes", "aurppo_linear_pair_bias_act_f32",
    "aurppo_mlp_layered_act_paired_f32",
    "aurppo_mlp_layered_anyh_step_workspace_bytes", "aurppo_mlp_layered_anyh_step_f32", "aurppo_mlp_layered_anyh_minibatch_f32",
    "aurppo_mlp_layered_anyh_wop_bytes", "aurppo_mlp_layered_anyh_prep_f32", "aurppo_mlp_layered_anyh_act_workspace_bytes",
    "aurppo_mlp_layered_anyh_act_f32", "aurppo_mlp_layered_anyh_act_paired_f32",
    "aurppo_head_ppo_wa_workspace_bytes", "aurppo_head_ppo_wa_f32", "aurppo_head_act_wa_f32",
    "aurppo_mlp_layered_wa_step_workspace_bytes", "aurppo_mlp_layered_wa_step_f32", "aurppo_mlp_layered_wa_minibatch_f32",
    "aurppo_mlp_layered_wa_act_f32", "aurppo_mlp_layered_wa_act_paired_f32",
    "aurppo_cartpole_reset", "aurppo_cartpole_step", "aurppo_cartpole_rollout_f32",
    "aurppo_pendulum_reset", "aurppo_pendulum_step", "aurppo_pendulum_rollout_f32",
)

_lib = None


class AurppoLibraryMissing(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library or fail loudly -- there is no fallback implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AurppoLibraryMissing(
            f"{LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). aur_ppo_amd has no CPU or PyTorch fallback for its kernels.")
    # torch ships its own libamdhip64 (same SONAME as /opt/rocm's).  Import torch FIRST so this
    # library binds to the runtime torch uses: streams and device pointers are only meaningful
    # inside one HIP runtime instance.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    _declare(lib)
    _lib = lib
    return lib


def _declare(lib):
    """argtypes / restype of every symbol, in the header's order (tests/test_abi_signatures.py holds each one to its prototype in
    include/aurppo.h).  The fused-step family shares long runs of same-typed arguments: each run is spelled once here, and
    ``hip_ops`` builds the matching values with one helper per run (``_step_prefix``, ``_adam_tail``, ``_next_pair``, ``_rec_pair``)."""
    vp, i32, i64, u32, f64, pi32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_double, C.POINTER(C.c_int)
    ws_stream = [vp, vp]                                    # workspace, stream
    loss_knobs = [f64, f64, f64, i32, i32]                  # clip, ent_coef, vf_coef, norm_adv, vloss_mode
    adam_knobs = [f64, vp, vp, f64, f64, f64, vp]           # max_norm, lr_dev, step_dev, beta1, beta2, eps, out_norm
    adam_tail = [vp, vp] + adam_knobs                       # exp_avg, exp_avg_sq, ...
    next_pair = [vp, i32]                                   # next_idx, next_M
    rec_pair = [vp, i32]                                    # rec, rec_floats

    def step_prefix(shape_ints):
        """obs, actions, rec, idx; M, D, A, continuous + hidden (1) or hidden, num_layers (2); params, layout_h, n_params; grads;
        the loss knobs; out_scalars."""
        return [vp] * 4 + [i32] * (4 + shape_ints) + [vp, pi32, i32, vp] + loss_knobs + [vp]

    lib.aurppo_k7w_kernel.argtypes = [i32, i32]
    # K1
    lib.aurppo_gae_f32.argtypes = [vp] * 7 + [i32, i32, f64, f64, i32, vp]
    lib.aurppo_gae_pack_f32.argtypes = [vp] * 9 + [i32, i32, f64, f64, i32, vp]
    # K2
    lib.aurppo_mt19937_create.argtypes = [C.POINTER(vp), u32, i32, vp]
    lib.aurppo_mt19937_destroy.argtypes = [vp]
    lib.aurppo_mt19937_seed.argtypes = [vp, u32, vp]
    lib.aurppo_mt19937_get_state.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_int32), vp]
    lib.aurppo_mt19937_set_state.argtypes = [vp, C.POINTER(u32), C.c_int32, vp]
    lib.aurppo_mt19937_status_f32.argtypes = [vp, vp, vp]
    lib.aurppo_arange_i32.argtypes = [vp, i32, vp]
    lib.aurppo_shuffle_i32.argtypes = [vp, vp, i32, vp]
    lib.aurppo_shuffle_epochs_i32.argtypes = [vp, vp, i32, i32, vp]
    # K3
    lib.aurppo_gather_f32.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), pi32, i32, vp]
    # K4 + K5
    lib.aurppo_loss_workspace_bytes.argtypes = [i32]
    lib.aurppo_loss_fwd_bwd_f32.argtypes = [vp] * 7 + [i32] + loss_knobs + [vp] * 4 + ws_stream
    lib.aurppo_loss_fwd_bwd_packed_f32.argtypes = [vp] * 4 + [i32] + loss_knobs + [vp] * 4 + ws_stream
    # K7 and its chained / two-halves forms
    lib.aurppo_mlp_workspace_bytes.argtypes = [i32]
    lib.aurppo_mlp_ppo_step_f32.argtypes = step_prefix(1) + ws_stream
    lib.aurppo_mlp_ppo_step_ev_f32.argtypes = step_prefix(1) + ws_stream + [vp, vp]
    lib.aurppo_mlp_ppo_minibatch_f32.argtypes = step_prefix(1) + adam_tail + next_pair + [i32] + ws_stream
    lib.aurppo_pack_records_f32.argtypes = [vp, vp, i32, i32, vp, vp]
    lib.aurppo_mlp_ppo_grad_f32.argtypes = step_prefix(1) + [vp, i32] + ws_stream
    lib.aurppo_mlp_ppo_apply_f32.argtypes = [vp] * 4 + [pi32, i32, i32, f64] + adam_knobs + rec_pair + next_pair + ws_stream
    lib.aurppo_mlp_ppo_apply_parts_f32.argtypes = [vp] * 4 + [pi32, i32, i32, vp, i32] + adam_knobs + rec_pair + next_pair + ws_stream
    # K11, the linear products, K13, K12
    lib.aurppo_conv3x3_wop_bytes.argtypes = [i32, i32]
    lib.aurppo_conv3x3_f32.argtypes = [vp, vp, vp] + [i32] * 7 + ws_stream
    lib.aurppo_conv3x3_pool_f32.argtypes = [vp] * 5 + [i32] * 6 + ws_stream
    lib.aurppo_linear_f32.argtypes = [vp, vp, vp, C.c_longlong, i32, i32, i32] + ws_stream
    lib.aurppo_linear_bias_act_f32.argtypes = [vp, vp, vp, vp, C.c_longlong, i32, i32, i32] + ws_stream
    lib.aurppo_linear_small_bias_act_f32.argtypes = [vp, vp, vp, vp, C.c_longlong, i32, i32, i32] + ws_stream
    lib.aurppo_linear_pair_wop_bytes.argtypes = [i32, i32]
    lib.aurppo_linear_pair_bias_act_f32.argtypes = [vp] * 8 + [C.c_longlong, i32, i32, i32] + ws_stream
    lib.aurppo_linear_wgrad_ws_bytes.argtypes = [C.c_longlong, i32, i32]
    lib.aurppo_linear_wgrad_f32.argtypes = [vp, vp, vp, C.c_longlong, i32, i32] + ws_stream
    lib.aurppo_linear_rows_bias_act_f32.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, i32, i32, i32] + ws_stream
    lib.aurppo_linear_wgrad_rows_f32.argtypes = [vp, vp, vp, vp, C.c_longlong, i32, i32] + ws_stream
    lib.aurppo_linear_dx_tanh_f32.argtypes = [vp, vp, vp, vp, C.c_longlong, i32, i32] + ws_stream
    lib.aurppo_head_ppo_workspace_bytes.argtypes = [i32, i32, i32]
    lib.aurppo_head_ppo_f32.argtypes = [vp] * 7 + [i32] * 4 + [vp, pi32, i32, vp] + loss_knobs + [vp] + ws_stream
    # K14 and the layered rollout step
    lib.aurppo_mlp_layered_wop_bytes.argtypes = [i32, i32, i32]
    lib.aurppo_mlp_layered_prep_f32.argtypes = [vp, pi32, i32, i32, i32, i32, vp, vp]
    lib.aurppo_mlp_layered_act_workspace_bytes.argtypes = [i32, i32]
    lib.aurppo_mlp_layered_act_f32.argtypes = [vp, vp] + [i32] * 6 + [vp, pi32, i32, vp, vp, vp, vp] + ws_stream
    lib.aurppo_mlp_layered_act_paired_f32.argtypes = lib.aurppo_mlp_layered_act_f32.argtypes
    lib.aurppo_head_act_f32.argtypes = [vp, vp, vp] + [i32] * 4 + [vp, pi32, i32, vp, vp, vp, vp]
    # the layered update step
    lib.aurppo_linear_wgrad_bias_ws_bytes.argtypes = [C.c_longlong, i32, i32]
    lib.aurppo_linear_wgrad_bias_f32.argtypes = [vp, vp, vp, vp, vp, C.c_longlong, i32, i32] + ws_stream
    lib.aurppo_mlp_layered_step_workspace_bytes.argtypes = [i32] * 5
    lib.aurppo_mlp_layered_step_f32.argtypes = step_prefix(2) + ws_stream
    lib.aurppo_mlp_layered_minibatch_f32.argtypes = step_prefix(2) + adam_tail + ws_stream
    # the layered steps at any hidden width: each entry has its sibling's argument list
    for name in ("wop_bytes", "prep_f32", "act_workspace_bytes", "act_f32", "act_paired_f32", "step_workspace_bytes", "step_f32",
                 "minibatch_f32"):
        getattr(lib, "aurppo_mlp_layered_anyh_" + name).argtypes = getattr(lib, "aurppo_mlp_layered_" + name).argtypes
    # K13, K14 and the layered steps with up to 32 actions: each entry has its sibling's argument list
    lib.aurppo_head_ppo_wa_workspace_bytes.argtypes = lib.aurppo_head_ppo_workspace_bytes.argtypes
    lib.aurppo_head_ppo_wa_f32.argtypes = lib.aurppo_head_ppo_f32.argtypes
    lib.aurppo_head_act_wa_f32.argtypes = lib.aurppo_head_act_f32.argtypes
    for name in ("act_f32", "act_paired_f32", "step_workspace_bytes", "step_f32", "minibatch_f32"):
        getattr(lib, "aurppo_mlp_layered_wa_" + name).argtypes = getattr(lib, "aurppo_mlp_layered_anyh_" + name).argtypes
    lib.aurppo_conv3x3_wgrad_ws_bytes.argtypes = [i32] * 6
    lib.aurppo_conv3x3_wgrad_f32.argtypes = [vp, vp, vp] + [i32] * 6 + ws_stream
    # the narrow builds of the 16 -> 32 block's gradients
    lib.aurppo_conv3x3_dgrad_narrow_wop_bytes.argtypes = [i32] * 2
    lib.aurppo_conv3x3_dgrad_narrow_f32.argtypes = [vp, vp, vp] + [i32] * 6 + ws_stream
    lib.aurppo_conv3x3_wgrad_narrow_ws_bytes.argtypes = [i32] * 6
    lib.aurppo_conv3x3_wgrad_narrow_f32.argtypes = [vp, vp, vp] + [i32] * 6 + ws_stream
    # K11x: activations as bf16 planes
    lib.aurppo_planes_bytes.argtypes = [i32] * 4
    lib.aurppo_split_planes_f32.argtypes = [vp, vp] + [i32] * 4 + [vp]
    lib.aurppo_conv3x3_planes_f32.argtypes = [vp, vp, vp] + [i32] * 6 + ws_stream
    lib.aurppo_conv3x3_pool_planes_f32.argtypes = [vp, i32] + [vp] * 5 + [i32] * 6 + ws_stream
    lib.aurppo_first_block_planes_fwd_f32.argtypes = [vp] * 7 + [i32] * 5 + [vp]
    # the one-shot exchange
    lib.aurppo_p2p_parts.argtypes = [i32]
    lib.aurppo_p2p_create.argtypes = [C.POINTER(vp), i32, i32, i32, vp]
    lib.aurppo_p2p_get_handle.argtypes = [vp, vp]
    lib.aurppo_p2p_open_peers.argtypes = [vp, vp]
    lib.aurppo_p2p_allreduce_mean_f32.argtypes = [vp, vp, i32, vp, vp, f64, vp]
    lib.aurppo_p2p_status.argtypes = [vp, pi32, vp]
    lib.aurppo_p2p_destroy.argtypes = [vp]
    # K8, K7w / K8w
    lib.aurppo_mlp_act_f32.argtypes = [vp, vp] + [i32] * 5 + [vp, pi32, i32, vp, vp, vp, vp]
    lib.aurppo_mlp_wide_workspace_bytes.argtypes = [i32, i32, i32]
    lib.aurppo_mlp_wide_ppo_step_f32.argtypes = step_prefix(2) + ws_stream + [vp, vp]
    lib.aurppo_mlp_wide_ppo_minibatch_f32.argtypes = step_prefix(2) + adam_tail + next_pair + [i32] + ws_stream
    lib.aurppo_mlp_wide_act_f32.argtypes = [vp, vp] + [i32] * 6 + [vp, pi32, i32, vp, vp, vp] + ws_stream
    # K15, K16: the device CartPole and the one-launch rollout on it
    cart_env = [vp, vp, vp]                                 # state, steps, episode
    cart_seed = [i32, u32, u32]                             # env0, seed_lo, seed_hi
    cart_consts = [f64] * 8 + [i32]                         # gravity, masscart, masspole, length, force_mag, tau, theta_lim, x_lim, max_steps
    lib.aurppo_cartpole_reset.argtypes = cart_env + [vp, i32] + cart_seed + [vp]
    lib.aurppo_cartpole_step.argtypes = cart_env + [vp] * 5 + [i32] + cart_seed + cart_consts + [vp]
    lib.aurppo_cartpole_rollout_f32.argtypes = (cart_env + [vp] * 3 + [i32] * 7 + [vp, pi32, i32] + [vp] * 7 + cart_seed + cart_consts
                                                + [vp])
    # K17, K18: the device Pendulum and the one-launch rollout on it
    pend_consts = [f64] * 6 + [i32]                         # g, m, l, dt, max_speed, max_torque, max_steps
    lib.aurppo_pendulum_reset.argtypes = cart_env + [vp, i32] + cart_seed + [vp]
    lib.aurppo_pendulum_step.argtypes = cart_env + [vp] * 6 + [i32] + cart_seed + pend_consts + [vp]
    lib.aurppo_pendulum_rollout_f32.argtypes = (cart_env + [vp] * 3 + [i32] * 7 + [vp, pi32, i32] + [vp] * 8 + cart_seed + pend_consts
                                                + [vp])
    # K6, K6b
    lib.aurppo_clip_workspace_bytes.argtypes = [i64]
    lib.aurppo_grad_norm_clip_f32.argtypes = [vp, i64, f64, vp] + ws_stream
    lib.aurppo_clip_adam_f32.argtypes = [vp] * 4 + [i64, i64] + adam_knobs + ws_stream
    # K9, K10
    lib.aurppo_bias_relu_pool2_fwd_f32.argtypes = [vp] * 6 + [i32] * 4 + [vp]
    lib.aurppo_bias_relu_pool2_bwd_f32.argtypes = [vp] * 4 + [i32] * 4 + [vp]
    lib.aurppo_weighted_batch_sum_f32.argtypes = [vp, vp, vp, i32, i64, vp]
    lib.aurppo_first_block_fwd_f32.argtypes = [vp] * 6 + [i32] * 5 + [vp]
    lib.aurppo_first_block_bwd_f32.argtypes = [vp] * 6 + [i32] * 5 + [vp]
    # everything returns int except the error string and the size_t workspace plans
    sized = ("aurppo_loss_workspace_bytes", "aurppo_clip_workspace_bytes", "aurppo_mlp_workspace_bytes", "aurppo_conv3x3_wop_bytes",
             "aurppo_linear_wgrad_ws_bytes", "aurppo_conv3x3_wgrad_ws_bytes", "aurppo_mlp_wide_workspace_bytes",
             "aurppo_head_ppo_workspace_bytes", "aurppo_mlp_layered_wop_bytes", "aurppo_mlp_layered_act_workspace_bytes",
             "aurppo_linear_wgrad_bias_ws_bytes", "aurppo_mlp_layered_step_workspace_bytes",
             "aurppo_conv3x3_dgrad_narrow_wop_bytes", "aurppo_conv3x3_wgrad_narrow_ws_bytes", "aurppo_planes_bytes",
             "aurppo_linear_pair_wop_bytes", "aurppo_mlp_layered_anyh_wop_bytes", "aurppo_mlp_layered_anyh_act_workspace_bytes",
             "aurppo_mlp_layered_anyh_step_workspace_bytes", "aurppo_head_ppo_wa_workspace_bytes",
             "aurppo_mlp_layered_wa_step_workspace_bytes")
    for name in SYMBOLS:
        getattr(lib, name).restype = C.c_char_p if name == "aurppo_last_error" else C.c_size_t if name in sized else i32
