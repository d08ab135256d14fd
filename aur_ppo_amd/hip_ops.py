"""Torch-facing wrappers over the C ABI (include/aurppo.h).  Tensors must be CUDA(HIP), fp32 /
int32, contiguous; every call enqueues on torch's CURRENT stream and returns without syncing."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib

GAE, NORMAL_ADV, GAE_SKIP_LAST = 0, 1, 2
VLOSS_RETURNS, VLOSS_CLIPPED, VLOSS_OLDVALUES = 0, 1, 2
S_LOSS, S_PG, S_VL, S_ENT, S_OLD_KL, S_KL, S_CLIPFRAC, S_ADV_MEAN, S_ADV_STD = range(9)
N_SCALARS = 9


_runtime_checked = False


def _lib_or_raise():
    global _runtime_checked
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("aur_ppo_amd.hip_ops needs a gfx950 GPU: the HIP kernels have no CPU fallback")
    if not _runtime_checked:
        n = lib.aurppo_device_count()
        if n != torch.cuda.device_count():
            raise RuntimeError(f"libaurppo_hip.so sees {n} device(s) but torch sees {torch.cuda.device_count()}: the "
                               "library is bound to a different HIP runtime than torch (import torch before loading it)")
        _runtime_checked = True
    return lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {_lib.load().aurppo_last_error().decode()}")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"expected a contiguous CUDA {dtype} tensor, got {t.dtype} on {t.device}, "
                         f"contiguous={t.is_contiguous()}")
    return C.c_void_p(t.data_ptr())


_ws_cache = {}
_ws_retired = []      # outgrown workspaces stay allocated: a captured hipGraph may still point into them


def _workspace(kind, nbytes, device):
    key = (kind, device.index if device.index is not None else torch.cuda.current_device())
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _ws_retired.append(ws)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _ws_stream(ws):
    """workspace, stream: the two arguments most calls end with."""
    return (C.c_void_p(ws.data_ptr()), _stream())


def _loss_knobs(clip, ent_coef, vf_coef, norm_adv, vloss_mode):
    """clip, ent_coef, vf_coef, norm_adv, vloss_mode."""
    return (float(clip), float(ent_coef), float(vf_coef), int(bool(norm_adv)), int(vloss_mode))


# ------------------------------------------------------------------ K1
def gae(rewards, values, terminals, next_value, next_done, gamma, lam, mode=GAE, out=None, log_probs=None, rec=None):
    """``ppo.run_gae`` / ``normal_advantage`` (src/ppo.py:125-157).  Returns (returns, advantages).
    With ``log_probs`` (T,N) and ``rec`` (T*N,4) the kernel also writes the per-sample record
    {old_logp, A, R, V} the packed gather / loss path consumes."""
    lib = _lib_or_raise()
    T, N = rewards.shape
    if values.shape != (T, N) or terminals.shape != (T, N) or next_value.numel() != N or next_done.numel() != N:
        raise ValueError(f"shape mismatch: rewards {tuple(rewards.shape)}, values {tuple(values.shape)}, terminals "
                         f"{tuple(terminals.shape)}, next_value {tuple(next_value.shape)}, next_done {tuple(next_done.shape)}")
    if out is None:
        adv, ret = torch.empty_like(rewards), torch.empty_like(rewards)
    else:
        ret, adv = out
    if rec is not None:
        if log_probs is None or log_probs.shape != (T, N) or rec.numel() != 4 * T * N:
            raise ValueError("gae: rec needs log_probs (T,N) and rec (T*N,4)")
        _check(lib.aurppo_gae_pack_f32(_ptr(rewards), _ptr(values), _ptr(terminals), _ptr(next_value), _ptr(next_done),
                                       _ptr(log_probs), _ptr(adv), _ptr(ret), _ptr(rec), T, N, float(gamma),
                                       float(lam), int(mode), _stream()), "aurppo_gae_pack_f32")
        return ret, adv
    _check(lib.aurppo_gae_f32(_ptr(rewards), _ptr(values), _ptr(terminals), _ptr(next_value), _ptr(next_done),
                              _ptr(adv), _ptr(ret), T, N, float(gamma), float(lam), int(mode), _stream()),
           "aurppo_gae_f32")
    return ret, adv


# ------------------------------------------------------------------ K2
class MT19937:
    """Device-resident twin of numpy's global legacy stream: ``np.random.seed`` (src/ppo.py:182) and
    ``np.random.shuffle`` (src/ppo.py:217)."""

    def __init__(self, seed: int, max_n: int, device=None):
        lib = _lib_or_raise()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.max_n = int(max_n)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _check(lib.aurppo_mt19937_create(C.byref(h), int(seed) & 0xFFFFFFFF, self.max_n, _stream()),
                   "aurppo_mt19937_create")
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.load().aurppo_mt19937_destroy(h)
            except Exception:
                pass

    def seed(self, seed: int):
        _check(_lib.load().aurppo_mt19937_seed(self._h, int(seed) & 0xFFFFFFFF, _stream()), "aurppo_mt19937_seed")

    def get_state(self):
        key = np.empty(624, np.uint32)
        pos = C.c_int32()
        _check(_lib.load().aurppo_mt19937_get_state(self._h, key.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos),
                                                    _stream()), "aurppo_mt19937_get_state")
        return key, int(pos.value)

    def set_state(self, key, pos):
        key = np.ascontiguousarray(key, dtype=np.uint32)
        assert key.shape == (624,)
        _check(_lib.load().aurppo_mt19937_set_state(self._h, key.ctypes.data_as(C.POINTER(C.c_uint32)), int(pos),
                                                    _stream()), "aurppo_mt19937_set_state")

    def status_into(self, out):
        """``out[0]`` (1-element fp32 device tensor) = 1 if a shuffle ran out of pre-generated draws since the last
        (re)seed (its permutation is invalid), else 0.  No host sync: read it with the per-update scalars."""
        _check(_lib.load().aurppo_mt19937_status_f32(self._h, _ptr(out), _stream()), "aurppo_mt19937_status_f32")
        return out

    def shuffle_(self, idx):
        """In-place ``np.random.shuffle`` of an int32 device vector."""
        if idx.numel() == 0:
            return idx
        _check(_lib.load().aurppo_shuffle_i32(self._h, _ptr(idx, torch.int32), idx.numel(), _stream()),
               "aurppo_shuffle_i32")
        return idx

    def shuffle_epochs(self, n: int, epochs: int, out=None):
        """The ``epochs`` index arrays of one update (arange once, shuffled in place per epoch,
        src/ppo.py:213-217) as an (epochs, n) int32 tensor."""
        if out is None:
            out = torch.empty((epochs, n), dtype=torch.int32, device=self.device)
        _check(_lib.load().aurppo_shuffle_epochs_i32(self._h, _ptr(out, torch.int32), int(n), int(epochs), _stream()),
               "aurppo_shuffle_epochs_i32")
        return out


def arange_i32(n, device):
    out = torch.empty(n, dtype=torch.int32, device=device)
    _check(_lib_or_raise().aurppo_arange_i32(_ptr(out, torch.int32), n, _stream()), "aurppo_arange_i32")
    return out


# ------------------------------------------------------------------ K3
def gather(idx, srcs, outs=None, probe=None):
    """One fused launch for ``[s[idx] for s in srcs]`` (src/ppo.py:219-220,225,236,251-257).
    ``srcs``: flattened buffer tensors (B, ...) sharing dim 0; ``idx``: int32 (M,).
    ``probe``: optional object whose ``begin()``/``end()`` are called immediately around the C call
    (bench.py records HIP events there, so host-side argument marshalling is not timed)."""
    lib = _lib_or_raise()
    M = idx.numel()
    n = len(srcs)
    if outs is None:
        outs = [torch.empty((M,) + tuple(s.shape[1:]), dtype=torch.float32, device=s.device) for s in srcs]
    row = [int(np.prod(s.shape[1:])) if s.dim() > 1 else 1 for s in srcs]
    for s, o, r in zip(srcs, outs, row):
        if o.numel() != M * r:
            raise ValueError(f"gather: destination has {o.numel()} elements, expected {M}*{r}")
    VP = C.c_void_p * n
    src_a = VP(*[s.data_ptr() for s in srcs])
    dst_a = VP(*[o.data_ptr() for o in outs])
    for t in list(srcs) + list(outs):
        _ptr(t)
    row_a = (C.c_int * n)(*row)
    idx_p, st = _ptr(idx, torch.int32), _stream()
    if probe is not None:
        probe.begin()
    rc = lib.aurppo_gather_f32(idx_p, M, src_a, dst_a, row_a, n, st)
    if probe is not None:
        probe.end()
    _check(rc, "aurppo_gather_f32")
    return outs


# ------------------------------------------------------------------ K4 + K5
def _loss_call(lib, name, inputs, M, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars):
    """The part ``loss_fwd_bwd`` and ``loss_fwd_bwd_packed`` share: everything but ``inputs``, the kernel's leading pointers."""
    dev = inputs[0].device
    if out_scalars is None:
        out_scalars = torch.empty(N_SCALARS, dtype=torch.float32, device=dev)
    g_lp, g_v, g_e = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(3))
    ws = _workspace("loss", lib.aurppo_loss_workspace_bytes(M), dev)
    _check(getattr(lib, name)(*[_ptr(t) for t in inputs], M, *_loss_knobs(clip, ent_coef, vf_coef, norm_adv, vloss_mode),
                              _ptr(out_scalars), _ptr(g_lp), _ptr(g_v), _ptr(g_e), *_ws_stream(ws)), name)
    return out_scalars, g_lp, g_v, g_e


def loss_fwd_bwd(newlogp, oldlogp, adv, newv, oldv, ret, entropy, clip, ent_coef, vf_coef, norm_adv=True,
                 vloss_mode=VLOSS_CLIPPED, out_scalars=None):
    """src/ppo.py:225-264 forward and backward.  Returns (scalars[9], g_newlogp, g_newv, g_entropy)."""
    lib = _lib_or_raise()
    M = newlogp.numel()
    for t in (oldlogp, adv, newv, oldv, ret, entropy):
        if t.numel() != M:
            raise ValueError(f"loss_fwd_bwd: expected {M} elements, got {t.numel()}")
    return _loss_call(lib, "aurppo_loss_fwd_bwd_f32", (newlogp, oldlogp, adv, newv, oldv, ret, entropy), M, clip, ent_coef, vf_coef,
                      norm_adv, vloss_mode, out_scalars)


def loss_fwd_bwd_packed(newlogp, newv, entropy, rec, clip, ent_coef, vf_coef, norm_adv=True, vloss_mode=VLOSS_CLIPPED,
                        out_scalars=None):
    """As ``loss_fwd_bwd`` with the old-side inputs as a gathered (M,4) record {old_logp, adv, ret, old_v}."""
    lib = _lib_or_raise()
    M = newlogp.numel()
    if newv.numel() != M or entropy.numel() != M or rec.numel() != 4 * M:
        raise ValueError("loss_fwd_bwd_packed: size mismatch")
    return _loss_call(lib, "aurppo_loss_fwd_bwd_packed_f32", (newlogp, newv, entropy, rec), M, clip, ent_coef, vf_coef, norm_adv,
                      vloss_mode, out_scalars)


class _PPOLossBase(torch.autograd.Function):
    """``loss = ppo_loss(newlogp, newvalue, entropy, ...)`` with the reference's semantics; the
    HIP kernel produces the three input gradients in the forward pass, backward only scales them."""

    @staticmethod
    def _run(ctx, fwd_bwd, n_inputs, newlogp, newv, entropy):
        """``fwd_bwd(newlogp, newv, entropy)`` on detached flat inputs; keeps what backward needs.  ``n_inputs``: forward's."""
        sc, g_lp, g_v, g_e = fwd_bwd(newlogp.detach().contiguous(), newv.detach().reshape(-1).contiguous(),
                                     entropy.detach().contiguous())
        ctx.save_for_backward(g_lp, g_v, g_e)
        ctx.v_shape, ctx.n_no_grad = newv.shape, n_inputs - 3
        return sc[S_LOSS].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g_lp, g_v, g_e = ctx.saved_tensors
        return (g_lp * grad_out, (g_v * grad_out).view(ctx.v_shape), g_e * grad_out) + (None,) * ctx.n_no_grad


class PPOLossPackedFn(_PPOLossBase):
    @staticmethod
    def forward(ctx, newlogp, newv, entropy, rec, *knobs):
        return _PPOLossBase._run(ctx, lambda nl, nv, en: loss_fwd_bwd_packed(nl, nv, en, rec, *knobs), 4 + len(knobs),
                                 newlogp, newv, entropy)


def ppo_loss_packed(newlogp, newv, entropy, rec, clip, ent_coef, vf_coef, norm_adv=True, vloss_mode=VLOSS_CLIPPED,
                    out_scalars=None):
    return PPOLossPackedFn.apply(newlogp, newv, entropy, rec, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars)


class PPOLossFn(_PPOLossBase):
    @staticmethod
    def forward(ctx, newlogp, newv, entropy, oldlogp, adv, oldv, ret, *knobs):
        return _PPOLossBase._run(ctx, lambda nl, nv, en: loss_fwd_bwd(nl, oldlogp, adv, nv, oldv, ret, en, *knobs), 7 + len(knobs),
                                 newlogp, newv, entropy)


def ppo_loss(newlogp, newv, entropy, oldlogp, adv, oldv, ret, clip, ent_coef, vf_coef, norm_adv=True,
             vloss_mode=VLOSS_CLIPPED, out_scalars=None):
    return PPOLossFn.apply(newlogp, newv, entropy, oldlogp, adv, oldv, ret, clip, ent_coef, vf_coef, norm_adv,
                           vloss_mode, out_scalars)


# ------------------------------------------------------------------ K7
MLP_HIDDEN, MLP_MAX_D, MLP_MAX_A = 64, 64, 16
MLP_WIDE_MAX_HIDDEN, MLP_WIDE_MAX_D, MLP_WIDE_MAX_LAYERS = 128, 128, 3
MLP_LAYERED_MAX_HIDDEN = 1024
MLP_LAYERED_MAX_A = 32          # the layered routes' action cap with ``wide_actions``; without it, and for K7 / K7w, MLP_MAX_A


def _mlp_structure(policy, bucket, max_a=MLP_MAX_A):
    """(offsets, n_params, D, A, continuous, num_layers, hidden) of the reference's tanh actor-critic inside ``bucket``'s flat
    buffers -- for the actor, then the critic: {w_l, b_l} for l = 0..L (layer L is the head), then actor_logstd -- or None if
    ``policy`` is not that structure or has more than ``max_a`` actions."""
    NL, Hd = getattr(policy, "num_layers", None), getattr(policy, "hidden_dim", None)
    if not hasattr(policy, "continuous") or not isinstance(NL, int) or not isinstance(Hd, int) or NL < 1 or Hd < 1:
        return None
    cont = bool(policy.continuous)
    off, pos = {}, 0
    for p in bucket.params:
        off[id(p)] = pos
        pos += p.numel()
    try:
        seq = []
        for net in (policy.actor.net, policy.critic.net):
            if len(net) != 2 * NL + 1:
                return None
            for li in range(0, 2 * NL + 1, 2):
                seq += [off[id(net[li].weight)], off[id(net[li].bias)]]
        seq.append(off[id(policy.actor_logstd)] if cont else 0)
        D = policy.actor.net[0].weight.shape[1]
        A = policy.actor.net[2 * NL].weight.shape[0]
        for net, out in ((policy.actor.net, A), (policy.critic.net, 1)):
            dims = [D] + [Hd] * NL + [out]
            for l in range(NL + 1):
                if tuple(net[2 * l].weight.shape) != (dims[l + 1], dims[l]):
                    return None
    except (KeyError, AttributeError, IndexError, TypeError):
        return None
    if A > max_a or (not cont and A < 2):
        return None
    return seq, pos, D, A, cont, NL, Hd


def mlp_layout(policy, bucket, max_a=MLP_MAX_A):
    """Float offsets of ``policy`` (an ``actor_critic``: ``num_layers`` Tanh layers of ``hidden_dim``, src/nets/nets.py:19-53)
    inside ``bucket``'s flat buffers, or None if no fused kernel is built for its shape.

    The default shape (two layers of 64, D <= 64) gets K7/K8's layout {w1,b1,w2,b2,w3,b3} x {actor, critic} + actor_logstd;
    every other shape up to three layers of 128 over D <= 128 gets K7w/K8w's (``wide=True``: {w_l, b_l} for l = 0..L per
    net, then actor_logstd).  ``max_a``: the action count up to which the question is asked (the kernels take ``MLP_MAX_A``;
    ``mlp_layered_layout`` asks whether a shape would be a fused one but for its actions)."""
    st = _mlp_structure(policy, bucket, max_a)
    if st is None:
        return None
    seq, pos, D, A, cont, NL, Hd = st
    if not (1 <= NL <= MLP_WIDE_MAX_LAYERS and 1 <= Hd <= MLP_WIDE_MAX_HIDDEN):
        return None
    # AURPPO_MLP_FORCE_WIDE=1 (diagnostic): the default shape through K7w too, for a same-box A/B of the two kernels
    fast = NL == 2 and Hd == MLP_HIDDEN and D <= MLP_MAX_D and os.environ.get("AURPPO_MLP_FORCE_WIDE") != "1"
    if not fast and D > MLP_WIDE_MAX_D:
        return None
    return dict(offsets=seq, n_params=pos, D=D, A=A, continuous=cont, hidden=Hd, num_layers=NL, wide=not fast)


def mlp_layered_layout(policy, bucket, any_state=False, any_hidden=False, wide_actions=False):
    """The layout of ``policy`` for ``mlp_layered_step``, or None.  Eligible: the reference's tanh actor-critic that no fused
    kernel covers (``mlp_layout`` is None), one or more layers of ``hidden_dim`` a multiple of 32 up to 1024, at most 16 actions,
    and a state of a multiple of 16 floats -- or, with ``any_state=True``, of any width (Hopper's 11, HalfCheetah's 17, Humanoid's
    376: layer 0's three products then run on the tail builds of k_linear / k_linear_wgrad, csrc/linear.hip).  Offsets as K7w's:
    {w_l, b_l} for l = 0..L per net, then actor_logstd.  Needs no device.
    ``any_hidden=True``: any ``hidden_dim`` in 1..1024 (200, 300, 400, 500; 100 over Humanoid's state).  A width that is no multiple
    of 32 gives the same dict -- the unpadded policy's offsets and ``n_params`` -- plus ``ragged_hidden=True``: the native calls
    (``mlp_layered_step_native``, ``mlp_layered_minibatch``, ``mlp_layered_prepare``, ``mlp_layered_act``) then run the policy at the
    width rounded up to 32 through the library's ``anyh`` entries (csrc/layered.hip); the per-product route refuses it.
    ``wide_actions=True``: up to 32 actions (Humanoid's 17, the dexterous hands' 20 - 30, a Categorical head of 17 - 32 choices).  A
    policy with 17 .. 32 actions gives the same dict plus ``wide_actions=True``: the native calls, ``head_ppo`` and ``head_act`` then go
    through the library's ``wa`` entries (K13 / K14 with 32-long per-action arrays, csrc/head.hip); the per-product route refuses it.  A
    policy with at most 16 actions gets the dict it gets without the keyword.  The state and hidden rules follow their own keywords."""
    if mlp_layout(policy, bucket) is not None:
        return None
    st = _mlp_structure(policy, bucket, MLP_LAYERED_MAX_A if wide_actions else MLP_MAX_A)
    if st is None or mlp_layout(policy, bucket, MLP_LAYERED_MAX_A) is not None:      # a fused shape stays the fused kernels', at any A
        return None
    seq, pos, D, A, cont, NL, Hd = st
    if (Hd % 32 != 0 and not any_hidden) or Hd > MLP_LAYERED_MAX_HIDDEN or (D % 16 != 0 and not any_state):
        return None
    lay = dict(offsets=seq, n_params=pos, D=D, A=A, continuous=cont, hidden=Hd, num_layers=NL, layered=True)
    if Hd % 32 != 0:
        lay["ragged_hidden"] = True
    if A > MLP_MAX_A:
        lay["wide_actions"] = True
    return lay


# what does not depend on the action count has no ``wa`` entry: a wide-action layout takes the ``anyh`` one (any hidden width)
_LAYERED_NO_WA = ("wop_bytes", "prep_f32", "act_workspace_bytes")


def _layered_entry(lib, layout, name):
    """(function, its name) of the layered entry ``aurppo_mlp_layered_<name>`` for ``layout``: the ``anyh`` sibling where the hidden
    width is no multiple of 32, the ``wa`` sibling (any hidden width too) where the policy has more than 16 actions, with the same
    arguments in the same order."""
    if layout.get("wide_actions"):
        family = "anyh_" if name in _LAYERED_NO_WA else "wa_"
    else:
        family = "anyh_" if layout.get("ragged_hidden") else ""
    entry = "aurppo_mlp_layered_" + family + name
    return getattr(lib, entry), entry


def _head_entry(lib, layout, name):
    """(function, its name) of K13 / K14's entry ``aurppo_head_<kernel>_<rest>`` (``name``: ``ppo_f32``, ``ppo_workspace_bytes``,
    ``act_f32``): the ``wa`` sibling ``aurppo_head_<kernel>_wa_<rest>`` for a wide-action layout."""
    kernel, rest = name.split("_", 1)
    entry = f"aurppo_head_{kernel}_{'wa_' if layout.get('wide_actions') else ''}{rest}"
    return getattr(lib, entry), entry


def _layered_ws_kind(kind, layout):
    """The workspace's cache key: a ragged hidden width keeps a buffer of its own per width (200 and 224 share none), and so does a
    wide-action layout, whose entries are another family's."""
    key = f"{kind}_h{layout['hidden']}" if layout.get("ragged_hidden") else kind
    return f"{key}_wa" if layout.get("wide_actions") else key


def _refuse_ragged_hidden(who, layout):
    if layout.get("ragged_hidden"):
        raise ValueError(f"{who}: a hidden width of {layout['hidden']} (no multiple of 32) runs through mlp_layered_step_native / "
                         f"mlp_layered_minibatch / mlp_layered_act only")


def _refuse_wide_actions(who, layout):
    if layout.get("wide_actions"):
        raise ValueError(f"{who}: a policy with {layout['A']} actions (more than {MLP_MAX_A}) runs through mlp_layered_step_native / "
                         f"mlp_layered_minibatch / mlp_layered_act only")


def k7_variant():
    """Which build of the fused MLP step the library launches for the default 64-64 policy (include/aurppo.h)."""
    return int(_lib_or_raise().aurppo_k7_variant())


def mlp_step_flops(layout, M):
    """Algorithmic FLOPs of one K7 / K7w launch (un-padded): forward of both nets, weight gradients of every
    layer, input gradients of every layer but the first (which needs none)."""
    D, A, Hd, NL = layout["D"], layout["A"], layout["hidden"], layout["num_layers"]
    total = 0
    for out in (A, 1):
        dims = [D] + [Hd] * NL + [out]
        mats = [dims[l] * dims[l + 1] for l in range(NL + 1)]
        total += 2 * sum(mats) + sum(mats[1:])      # forward + dW of every layer, dX of layers 2..
    return 2 * total * M


def k7w_kernel(hidden, state_dim):
    """Which K7w kernel runs for a net shape: 1 both nets per workgroup (fp32 MFMA), 2 one net (fp32 MFMA), 3 one net (bf16x3 MFMA)."""
    return int(_lib_or_raise().aurppo_k7w_kernel(int(hidden), int(state_dim)))


def k7w_kernel_name(hidden, state_dim, num_layers):
    k = k7w_kernel(hidden, state_dim)
    return {1: f"k_mlpw_step<{num_layers}, true>", 2: f"k_mlpw_step<{num_layers}, false>", 3: f"k_mlpw3_step<{num_layers}>"}[k]


def reload_knobs():
    """Make the library re-read its AURPPO_* environment knobs now (it reads them once per process otherwise)."""
    _check(_lib_or_raise().aurppo_reload_knobs(), "aurppo_reload_knobs")


def mlp_step_issued_bf16_flops(layout, M):
    """bf16 MFMA FLOPs k_mlp_step3 ISSUES per launch (csrc/mlp3.hip): every fp32 product is six bf16 products (bf16x3.h), the
    heads are padded to 16 outputs, the state to a multiple of 16 columns.  Per 32-row tile and wave (net, column half cb):
    v_mfma_f32_32x32x16_bf16 (32 768 FLOP): F1 6 x ceil(D / 16), F2 24, dH2 6, dW2 + dH1 48, dW1 24 (if cb * 32 < D);
    v_mfma_f32_16x16x32_bf16 (16 384 FLOP): head 12, dW3 12.  None for K7w / the fp32-MFMA build (they issue fp32 MFMAs)."""
    if layout.get("wide"):
        return None
    D = layout["D"]
    nks1 = (D + 15) // 16
    n32 = sum(6 * nks1 + 24 + 6 + 48 + (24 if cb * 32 < D else 0) for _net in range(2) for cb in range(2))
    n16 = 4 * 24
    tiles = (M + 31) // 32
    return tiles * (n32 * 32768 + n16 * 16384)


def _wide_only_step(layout, who):
    if layout.get("wide"):
        raise ValueError(f"{who}: only the default 64-64 MLP has the chained minibatch kernels; this policy "
                         f"({layout['num_layers']} x {layout['hidden']}) steps through mlp_ppo_step + clip_adam_")


def pack_records(rec, actions, out=None):
    """(B, 16) packed records {old_logp, A, R, V, action row, 0 ...} for the fused MLP step (pass them as ``rec`` with
    ``actions=None``): a sample's record and action row then share one 64-B line."""
    lib = _lib_or_raise()
    B = rec.shape[0]
    aw = actions.numel() // B
    if rec.numel() != 4 * B or aw * B != actions.numel() or not 1 <= aw <= 12:
        raise ValueError("pack_records: need (B, 4) records and at most 12 action floats per sample")
    if out is None:
        out = torch.empty((B, 16), dtype=torch.float32, device=rec.device)
    _check(lib.aurppo_pack_records_f32(_ptr(rec), _ptr(actions), B, aw, _ptr(out), _stream()), "aurppo_pack_records_f32")
    return out


def _mlp_buffers_ok(obs, actions, rec, layout):
    """The one place that knows the record / action shape rule of the fused-step family: (B, 4) records beside (B, A) actions
    ((B,) indices for the Categorical head), or ``actions=None`` and (B, 16) packed records (``pack_records``: at most 12 action
    floats).  ``obs`` (B, D) gives B; K13 has no observations (``obs=None``) and counts the records' rows."""
    aw = layout["A"] if layout["continuous"] else 1
    if obs is None:
        B = rec.shape[0]
    elif obs.shape[-1] != layout["D"]:
        return False
    else:
        B = obs.shape[0]
    if actions is None:
        return aw <= 12 and rec.numel() == B * 16
    return actions.numel() == B * aw and rec.numel() == B * 4


def _bucket_fits(n, *tensors, who):
    if min(t.numel() for t in tensors) < n:
        raise ValueError(f"{who}: the flat bucket is smaller than the policy")


def _optr(t, dtype=torch.float32):
    return _ptr(t, dtype) if t is not None else None


def _obias(b):
    """A linear wrapper's optional bias: its contiguous form's pointer, or None."""
    return _optr(b.contiguous() if b is not None else None)


# The argument order of the fused-step family (include/aurppo.h) lives in the builders below and nowhere else in this layer; each
# returns one run of a call's arguments, and _lib._declare spells the matching run of argtypes.  A transposition inside a run of
# same-typed pointers raises nothing on the host and faults on the GPU: tests/test_hip_ops_calls.py pins what every call passes.
def _layout_shape(layout, rows):
    """The offsets as a ``c_int`` array and the shape run: rows (M or N), D, A, continuous, hidden and, for every layout but the
    default 64-64 one, num_layers."""
    lay = (C.c_int * len(layout["offsets"]))(*layout["offsets"])
    shape = (rows, layout["D"], layout["A"], int(layout["continuous"]), layout["hidden"])
    return lay, shape + ((layout["num_layers"],) if layout.get("wide") or layout.get("layered") else ())


def _mlp_family(lib, layout, rows, device, n_ws):
    """What differs between the default 64-64 layout (K7 / K8) and the wide ones (K7w / K8w): the entry points' infix (also the
    workspace kind), the workspace for ``n_ws`` parameters (K8 has none: ``n_ws=None``), the offsets as a ``c_int`` array, and the
    shape arguments: rows (M or N), D, A, continuous, hidden and, for the wide layouts, num_layers."""
    lay, shape = _layout_shape(layout, rows)
    if layout.get("wide"):
        ws = _workspace("mlp_wide", lib.aurppo_mlp_wide_workspace_bytes(n_ws, layout["hidden"], layout["D"]), device)
        return "mlp_wide", ws, lay, shape
    ws = _workspace("mlp", lib.aurppo_mlp_workspace_bytes(n_ws), device) if n_ws is not None else None
    return "mlp", ws, lay, shape


def _step_prefix(inputs, actions, rec, idx, shape, flat_param, lay, n, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                 out_scalars):
    """``inputs`` ((obs,), or K13's four activation / gradient matrices), actions, rec, idx; ``shape`` (``_mlp_family``'s; K13: M, H,
    A, continuous); params, layout_h, n_params; grads; clip, ent_coef, vf_coef, norm_adv, vloss_mode; out_scalars."""
    return (*[_ptr(t) for t in inputs], _optr(actions), _ptr(rec), _ptr(idx, torch.int32), *shape, _ptr(flat_param), lay, n,
            _ptr(flat_grad), *_loss_knobs(clip, ent_coef, vf_coef, norm_adv, vloss_mode), _ptr(out_scalars))


def _adam_knobs(max_norm, lr_dev, step_dev, betas, eps, out_norm):
    """max_norm, lr_dev, step_dev, beta1, beta2, eps, out_norm."""
    return (float(max_norm), _ptr(lr_dev), _ptr(step_dev), float(betas[0]), float(betas[1]), float(eps), _ptr(out_norm))


def _adam_tail(exp_avg, exp_avg_sq, *knobs):
    """exp_avg, exp_avg_sq, then ``_adam_knobs``."""
    return (_ptr(exp_avg), _ptr(exp_avg_sq)) + _adam_knobs(*knobs)


def _next_pair(next_idx):
    """next_idx, next_M."""
    return (None, 0) if next_idx is None else (_ptr(next_idx, torch.int32), int(next_idx.numel()))


def _rec_pair(rec):
    """rec, rec_floats (4, or 16 for packed records)."""
    return (None, 4) if rec is None else (_ptr(rec), rec.numel() // rec.shape[0])


def mlp_ppo_step(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                 vloss_mode=VLOSS_CLIPPED, out_scalars=None, events=None):
    """K7: gather + evaluate + loss + backward for one minibatch of the MLP actor-critic; overwrites
    ``flat_grad[:n_params]`` and returns the 9 loss scalars.  ``events``: optional pair of
    ``torch.cuda.Event(enable_timing=True)`` recorded right around the main kernel (bench.py)."""
    lib = _lib_or_raise()
    n = layout["n_params"]
    if not _mlp_buffers_ok(obs, actions, rec, layout):
        raise ValueError("mlp_ppo_step: buffer shapes do not match the policy")
    if out_scalars is None:
        out_scalars = torch.empty(N_SCALARS, dtype=torch.float32, device=obs.device)
    family, ws, lay, shape = _mlp_family(lib, layout, idx.numel(), obs.device, n)
    handles = (C.c_void_p(0), C.c_void_p(0))
    if events is not None:
        for ev in events:          # materialise the hipEvent handles (torch creates them lazily on record())
            ev.record()
        handles = tuple(C.c_void_p(ev.cuda_event) for ev in events)
    args = _step_prefix((obs,), actions, rec, idx, shape, flat_param, lay, n, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                        out_scalars) + _ws_stream(ws)
    if family == "mlp_wide":       # K7w's one entry point always takes the handles; K7 has a measurement variant beside the plain one
        name, args = "aurppo_mlp_wide_ppo_step_f32", args + handles
    elif events is not None:
        name, args = "aurppo_mlp_ppo_step_ev_f32", args + handles
    else:
        name = "aurppo_mlp_ppo_step_f32"
    _check(getattr(lib, name)(*args), name)
    return out_scalars


def mlp_ppo_minibatch(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                      out_scalars, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps, out_norm, next_idx=None,
                      chained=False):
    """K7 (K7w) + K6b chained: one whole minibatch (src/ppo.py:219-269) -- fused step, clip_grad_norm_ and Adam over the
    same flat bucket -- in three launches.  ``next_idx``: the slice stepped next (its statistics are prepared by
    this call); ``chained=True`` when the previous call named this ``idx`` as its ``next_idx``.

    K7w: prepare + step + slab reduce + clip/Adam; with ``next_idx`` the optimizer launch leaves the operand copies and the
    next slice's statistics, and a chained call then skips its prepare launch."""
    lib = _lib_or_raise()
    n = layout["n_params"]
    if not _mlp_buffers_ok(obs, actions, rec, layout):
        raise ValueError("mlp_ppo_minibatch: buffer shapes do not match the policy")
    # alignment padding past n_params is left alone: its gradient is never written, so clip and Adam are no-ops there
    _bucket_fits(n, flat_param, flat_grad, exp_avg, exp_avg_sq, who="mlp_ppo_minibatch")
    family, ws, lay, shape = _mlp_family(lib, layout, idx.numel(), obs.device, n)
    name = f"aurppo_{family}_ppo_minibatch_f32"
    _check(getattr(lib, name)(
        *_step_prefix((obs,), actions, rec, idx, shape, flat_param, lay, n, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                      out_scalars),
        *_adam_tail(exp_avg, exp_avg_sq, max_norm, lr_dev, step_dev, betas, eps, out_norm), *_next_pair(next_idx), int(bool(chained)),
        *_ws_stream(ws)), name)
    return out_scalars


def mlp_ppo_grad(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                 out_scalars, step_dev, chained=False):
    """First half of a minibatch for one process per GPU: K7 + slab reduce into ``flat_grad[:n_params]`` (as
    ``mlp_ppo_step``), the Adam step count advanced.  The caller all-reduces ``flat_grad`` and calls ``mlp_ppo_apply``."""
    lib = _lib_or_raise()
    n = layout["n_params"]
    if not _mlp_buffers_ok(obs, actions, rec, layout):
        raise ValueError("mlp_ppo_grad: buffer shapes do not match the policy")
    _wide_only_step(layout, "mlp_ppo_grad")
    _family, ws, lay, shape = _mlp_family(lib, layout, idx.numel(), obs.device, n)
    _check(lib.aurppo_mlp_ppo_grad_f32(
        *_step_prefix((obs,), actions, rec, idx, shape, flat_param, lay, n, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                      out_scalars),
        _ptr(step_dev), int(bool(chained)), *_ws_stream(ws)), "aurppo_mlp_ppo_grad_f32")
    return out_scalars


def mlp_ppo_apply(flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm,
                  grad_scale=1.0, rec=None, next_idx=None):
    """Second half: ``flat_grad *= grad_scale`` (1/world after a SUM all-reduce), ``clip_grad_norm_`` and ``Adam.step`` in
    one launch, which also prepares ``next_idx`` for the next ``mlp_ppo_grad(..., chained=True)``."""
    lib = _lib_or_raise()
    n = layout["n_params"]
    _bucket_fits(n, flat_param, flat_grad, exp_avg, exp_avg_sq, who="mlp_ppo_apply")
    _wide_only_step(layout, "mlp_ppo_apply")
    _family, ws, lay, _shape = _mlp_family(lib, layout, None, flat_param.device, n)
    _check(lib.aurppo_mlp_ppo_apply_f32(
        _ptr(flat_param), _ptr(flat_grad), _ptr(exp_avg), _ptr(exp_avg_sq), lay, n, layout["D"], float(grad_scale),
        *_adam_knobs(max_norm, lr_dev, step_dev, betas, eps, out_norm), *_rec_pair(rec), *_next_pair(next_idx), *_ws_stream(ws)),
        "aurppo_mlp_ppo_apply_f32")
    return out_norm


def mlp_ppo_apply_parts(flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm,
                        sq_part, rec=None, next_idx=None):
    """``mlp_ppo_apply`` for a gradient that already is the mean over ranks and comes with partial sums of squares
    (``P2PExchange.allreduce_mean_``): the clip's norm is their sum, nothing is rescaled."""
    lib = _lib_or_raise()
    n = layout["n_params"]
    _bucket_fits(n, flat_param, flat_grad, exp_avg, exp_avg_sq, who="mlp_ppo_apply_parts")
    _wide_only_step(layout, "mlp_ppo_apply_parts")
    _family, ws, lay, _shape = _mlp_family(lib, layout, None, flat_param.device, n)
    _check(lib.aurppo_mlp_ppo_apply_parts_f32(
        _ptr(flat_param), _ptr(flat_grad), _ptr(exp_avg), _ptr(exp_avg_sq), lay, n, layout["D"], _ptr(sq_part, torch.float64),
        int(sq_part.numel()), *_adam_knobs(max_norm, lr_dev, step_dev, betas, eps, out_norm), *_rec_pair(rec), *_next_pair(next_idx),
        *_ws_stream(ws)), "aurppo_mlp_ppo_apply_parts_f32")
    return out_norm


class P2PExchange:
    """One-shot all-reduce of a small flat gradient over peer memory (include/aurppo.h, csrc/p2p.hip): every rank publishes its
    vector in a buffer the peers have mapped through HIP IPC and reads theirs directly -- one launch, one hop over xGMI, sums
    formed in rank order (bit-identical on every rank).  ``exchange_handles`` is the one collective it needs, at set-up:
    ``fn(bytes) -> [bytes of rank 0, bytes of rank 1, ...]`` (the trainer passes torch.distributed.all_gather_object)."""

    def __init__(self, rank, world, max_floats, device, exchange_handles):
        lib = _lib_or_raise()
        if os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") != "0":
            raise RuntimeError("P2PExchange: HSA_ENABLE_IPC_MODE_LEGACY=0 must be set before the process touches the GPU "
                               "(this driver only supports dmabuf IPC)")
        self.rank, self.world, self.n_cap, self.device = int(rank), int(world), int(max_floats), device
        self._h = C.c_void_p()
        with torch.cuda.device(device):
            nb = lib.aurppo_p2p_handle_bytes()
            mine, err = b"", None
            try:        # a rank that cannot create its buffer still takes part in the handle exchange (with an empty handle):
                _check(lib.aurppo_p2p_create(C.byref(self._h), self.rank, self.world, self.n_cap, _stream()), "aurppo_p2p_create")
                buf = C.create_string_buffer(nb)
                _check(lib.aurppo_p2p_get_handle(self._h, buf), "aurppo_p2p_get_handle")
                mine = bytes(buf.raw)
            except RuntimeError as e:
                err = str(e)
            every = exchange_handles(mine)          # ... so that every rank sees the failure and raises, none waits for ever
            if len(every) != self.world or any(len(h) != nb for h in every):
                raise RuntimeError("P2PExchange: not every rank could publish an exchange buffer"
                                   + (f" (this rank: {err})" if err else ""))
            if self.world > 1:
                _check(lib.aurppo_p2p_open_peers(self._h, C.create_string_buffer(b"".join(every), nb * self.world)),
                       "aurppo_p2p_open_peers")
        self.sq_part = torch.zeros(lib.aurppo_p2p_parts(self.n_cap), dtype=torch.float64, device=device)

    def allreduce_mean_(self, flat, n, step_dev, timeout_s=10.0):
        """``flat[:n]`` <- mean over ranks; leaves the partial sums of squares of the result in ``self.parts(n)``."""
        lib = _lib_or_raise()
        _check(lib.aurppo_p2p_allreduce_mean_f32(self._h, _ptr(flat), int(n), _ptr(step_dev), _ptr(self.sq_part, torch.float64),
                                                 float(timeout_s), _stream()), "aurppo_p2p_allreduce_mean_f32")
        return flat

    def parts(self, n):
        return self.sq_part[:_lib_or_raise().aurppo_p2p_parts(int(n))]

    def status(self):
        """0 = every exchange met its peers; 1 + r = rank r's flag timed out at least once (sticky).  Synchronises the stream."""
        v = C.c_int(0)
        _check(_lib_or_raise().aurppo_p2p_status(self._h, C.byref(v), _stream()), "aurppo_p2p_status")
        return int(v.value)

    def close(self):
        if self._h:
            _lib_or_raise().aurppo_p2p_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def mlp_act(obs, noise, flat_param, layout, actions=None, logp=None, value=None):
    """K8: the rollout step of the MLP actor-critic in one launch.  ``noise``: (N,A) standard-normal draws
    (Gaussian head) or (N,) uniform draws (Categorical head); None -> value only.  Outputs may be rows of
    the rollout buffer.  Returns (actions, logp, value)."""
    lib = _lib_or_raise()
    N, dev = obs.shape[0], obs.device
    if obs.shape[-1] != layout["D"]:
        raise ValueError("mlp_act: obs shape does not match the policy")
    actions, logp, value = _act_outputs("mlp_act", N, layout, noise, actions, logp, value, dev)
    # K8w keeps the operand-order copy of the weights in a workspace sized for no parameters; K8 has none
    family, ws, lay, shape = _mlp_family(lib, layout, N, dev, 0 if layout.get("wide") else None)
    name = f"aurppo_{family}_act_f32"
    null = C.c_void_p(0)
    _check(getattr(lib, name)(_ptr(obs), _ptr(noise) if noise is not None else null, *shape, _ptr(flat_param), lay, layout["n_params"],
                              _ptr(actions) if noise is not None else null, _ptr(logp) if noise is not None else null, _ptr(value),
                              *(_ws_stream(ws) if ws is not None else (_stream(),))), name)
    return actions, logp, value


# ------------------------------------------------------------------ K6
def grad_norm_clip_(flat_grads, max_norm, out_norm=None):
    """In-place ``clip_grad_norm_`` over one flat gradient bucket (src/ppo.py:268).  Returns the
    pre-clip norm as a 1-element device tensor."""
    lib = _lib_or_raise()
    n = flat_grads.numel()
    if out_norm is None:
        out_norm = torch.empty(1, dtype=torch.float32, device=flat_grads.device)
    ws = _workspace("clip", lib.aurppo_clip_workspace_bytes(n), flat_grads.device)
    _check(lib.aurppo_grad_norm_clip_f32(_ptr(flat_grads), n, float(max_norm), _ptr(out_norm),
                                         *_ws_stream(ws)), "aurppo_grad_norm_clip_f32")
    return out_norm


def clip_adam_(flat_param, flat_grad, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, clip_n=None, betas=(0.9, 0.999),
               eps=1e-5, out_norm=None):
    """K6b: ``clip_grad_norm_`` over the first ``clip_n`` elements + ``Adam.step`` over the whole flat
    bucket, two launches.  ``lr_dev`` / ``step_dev`` are 1-element device tensors (step is incremented)."""
    lib = _lib_or_raise()
    n = flat_param.numel()
    if clip_n is None:
        clip_n = n
    if out_norm is None:
        out_norm = torch.empty(1, dtype=torch.float32, device=flat_param.device)
    ws = _workspace("clip", lib.aurppo_clip_workspace_bytes(n), flat_param.device)
    _check(lib.aurppo_clip_adam_f32(_ptr(flat_param), _ptr(flat_grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, int(clip_n),
                                    *_adam_knobs(max_norm, lr_dev, step_dev, betas, eps, out_norm), *_ws_stream(ws)),
           "aurppo_clip_adam_f32")
    return out_norm


# ------------------------------------------------------------------ K9
def _pool2_bwd(dy, mask, shape, has_bias):
    """K9's backward from the pooled gradient and the mask alone: (dx of ``shape`` (B, C, H, W), the bias gradient or None)."""
    lib = _lib_or_raise()
    B, Cc, Hh, Ww = shape
    dy = dy.contiguous()
    dx = torch.empty((B, Cc, Hh, Ww), dtype=torch.float32, device=dy.device)
    part = torch.empty((B, Cc), dtype=torch.float32, device=dy.device) if has_bias else None
    _check(lib.aurppo_bias_relu_pool2_bwd_f32(_ptr(dy), C.c_void_p(mask.data_ptr()), _ptr(dx), _optr(part), B, Cc, Hh, Ww,
                                              _stream()), "aurppo_bias_relu_pool2_bwd_f32")
    return dx, (part.sum(0) if part is not None else None)


class _BiasReluPool2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, scale, plane):
        lib = _lib_or_raise()
        x = x.contiguous()
        B, Cc, Hh, Ww = x.shape
        y = torch.empty((B, Cc, Hh // 2, Ww // 2), dtype=torch.float32, device=x.device)
        mask = torch.empty((B, Cc, Hh // 2, Ww // 2), dtype=torch.uint8, device=x.device)
        if plane is not None:
            plane = plane.detach().reshape(Cc, Hh, Ww).contiguous()
            scale = scale.detach().reshape(B).contiguous()
        _check(lib.aurppo_bias_relu_pool2_fwd_f32(_ptr(x.detach()), _optr(bias.detach().contiguous() if bias is not None else None),
                                                  _optr(scale), _optr(plane), _ptr(y), C.c_void_p(mask.data_ptr()), B, Cc, Hh, Ww,
                                                  _stream()), "aurppo_bias_relu_pool2_fwd_f32")
        ctx.save_for_backward(mask, scale if plane is not None else None)
        ctx.shape = (B, Cc, Hh, Ww)
        ctx.has = (bias is not None, plane is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib_or_raise()
        mask, scale = ctx.saved_tensors
        B, Cc, Hh, Ww = ctx.shape
        dx, dbias = _pool2_bwd(dy, mask, ctx.shape, ctx.has[0])
        dplane = None
        if ctx.has[1]:
            dplane = torch.empty((1, Cc, Hh, Ww), dtype=torch.float32, device=dy.device)
            _check(lib.aurppo_weighted_batch_sum_f32(_ptr(dx), _ptr(scale), _ptr(dplane), B, Cc * Hh * Ww, _stream()),
                   "aurppo_weighted_batch_sum_f32")
        return dx, dbias, None, dplane


def bias_relu_pool2(x, bias=None, scale=None, plane=None):
    """K9: ``max_pool2d(relu(x + bias[c] + scale[b] * plane[c]), 2)`` in one pass (and one for the backward): the tail of a
    convolution block of src/nets/base_cnns.py:28-45; ``scale`` / ``plane`` carry the tiled gripper-state channel of
    src/models/robot_actor_critic.py:58-59 (no gradient flows to ``scale``, the state is an input)."""
    return _BiasReluPool2.apply(x, bias, scale, plane)


# ------------------------------------------------------------------ K10
def _planes_like(y):
    """An uninitialised planes tensor for the fp32 NCHW ``y`` (include/aurppo.h, K11x): int16 (B, C / 8, 3, H * W, 8)."""
    B, Cc, Hh, Ww = y.shape
    if Cc % 8 != 0:
        raise ValueError(f"planes hold whole groups of eight channels, got {Cc}")
    return torch.empty((B, Cc // 8, 3, Hh * Ww, 8), dtype=torch.int16, device=y.device)


class _FirstBlock(torch.autograd.Function):
    """K10: y, or with ``want_planes`` y and its planes (not differentiable); what is saved and the backward are the same."""
    @staticmethod
    def forward(ctx, obs, state, weight, bias, want_planes):
        lib = _lib_or_raise()
        obs = obs.detach().contiguous()
        state = state.detach().reshape(-1).to(torch.float32).contiguous()
        B, Ci, Hh, Ww = obs.shape
        Co = weight.shape[0]
        w = weight.detach().contiguous()
        y = torch.empty((B, Co, Hh // 2, Ww // 2), dtype=torch.float32, device=obs.device)
        mask = torch.empty((B, Co, Hh // 2, Ww // 2), dtype=torch.uint8, device=obs.device)
        head = (_ptr(obs), _ptr(w), _optr(bias.detach().contiguous() if bias is not None else None), _ptr(state), _ptr(y),
                C.c_void_p(mask.data_ptr()))
        yp = _planes_like(y) if want_planes else None
        if yp is None:
            _check(lib.aurppo_first_block_fwd_f32(*head, B, Ci, Co, Hh, Ww, _stream()), "aurppo_first_block_fwd_f32")
        else:
            _check(lib.aurppo_first_block_planes_fwd_f32(*head, _ptr(yp, torch.int16), B, Ci, Co, Hh, Ww, _stream()),
                   "aurppo_first_block_planes_fwd_f32")
        ctx.save_for_backward(obs, state, mask)
        ctx.dims = (B, Ci, Co, Hh, Ww, bias is not None)
        if yp is None:
            return y
        ctx.mark_non_differentiable(yp)
        return y, yp

    @staticmethod
    def backward(ctx, dy, _dyp=None):
        lib = _lib_or_raise()
        obs, state, mask = ctx.saved_tensors
        B, Ci, Co, Hh, Ww, has_bias = ctx.dims
        G = B * (Co // 16)
        dw_part = torch.empty((G, 16, (Ci + 1) * 9), dtype=torch.float32, device=dy.device)
        db_part = torch.empty((G, 16), dtype=torch.float32, device=dy.device)
        _check(lib.aurppo_first_block_bwd_f32(_ptr(dy.contiguous()), C.c_void_p(mask.data_ptr()), _ptr(obs), _ptr(state),
                                              _ptr(dw_part), _ptr(db_part), B, Ci, Co, Hh, Ww, _stream()),
               "aurppo_first_block_bwd_f32")
        # (B, Co/16, 16, taps) -> sum over the samples -> (Co, Ci+1, 3, 3)
        dw = dw_part.view(B, Co // 16, 16, (Ci + 1) * 9).sum(0).reshape(Co, Ci + 1, 3, 3)
        db = db_part.view(B, Co // 16, 16).sum(0).reshape(Co) if has_bias else None
        return None, None, dw, db, None


CONV3X3_MIN_PIXELS = 131072
CONV3X3_MIN_WGS = 512
K12_MIN_COUT, K12_MIN_CIN, K12_MIN_PIXELS = 64, 32, 16384
NARROW_MIN_PIXELS = 262144      # output pixels of the batch from which K11n / K12n are taken (512 one-wave slices of K12n, 2048 tiles of K11n)


class _Conv3x3(torch.autograd.Function):
    """The hidden 3x3 convolution behind ``conv3x3``, ``conv3x3_pool``, ``conv3x3_planes`` and ``conv3x3_pool_planes``.  ``pool``: the
    whole block (K11p: ``bias``, ReLU and the 2x2 max-pool in the epilogue; the mask is saved); ``xp``: the planes of ``x`` to read
    instead of it (K11x; fp32 ``x`` is saved for the backward all the same); ``want_planes``: ``(y, yp)``, the pooled output and its
    planes (not differentiable).  These options alone decide which C entry runs.  The backward is K9's (when pooled), then K11's mode 1
    and K12 (``_conv3x3_grads``), whatever the forward read or wrote."""
    @staticmethod
    def forward(ctx, x, w, bias, xp, pad, pool, want_planes):
        lib = _lib_or_raise()
        x, w = x.contiguous(), w.contiguous()
        B, Ci, Hh, Ww = x.shape
        Co = w.shape[0]
        Ho, Wo = Hh + 2 * pad - 2, Ww + 2 * pad - 2
        y = torch.empty((B, Co, Ho // 2, Wo // 2) if pool else (B, Co, Ho, Wo), dtype=torch.float32, device=x.device)
        mask = torch.empty(y.shape, dtype=torch.uint8, device=x.device) if pool else None
        yp = _planes_like(y) if want_planes else None
        ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Ci, Co), x.device)
        src = _planes_of(x, xp) if xp is not None else _ptr(x.detach())
        dims = (B, Ci, Co, Hh, Ww, int(pad))
        if not pool:
            assert bias is None and yp is None, "the bias and the planes are written by the pooled epilogue"
            name, args = ("aurppo_conv3x3_f32", (*dims, 0)) if xp is None else ("aurppo_conv3x3_planes_f32", dims)
            args = (src, _ptr(w.detach()), _ptr(y), *args)
        else:
            args = (_ptr(w.detach()), _optr(bias.detach().contiguous() if bias is not None else None), _ptr(y), C.c_void_p(mask.data_ptr()))
            if xp is None and yp is None:
                name, args = "aurppo_conv3x3_pool_f32", (src, *args, *dims)
            else:
                name, args = "aurppo_conv3x3_pool_planes_f32", (src, int(xp is not None), *args, _optr(yp, torch.int16), *dims)
        _check(getattr(lib, name)(*args, *_ws_stream(ws)), name)
        ctx.pad, ctx.has_bias = int(pad), bias is not None
        if not pool:
            ctx.save_for_backward(x, w)
            return y
        ctx.save_for_backward(x, w, mask)
        if yp is None:
            return y
        ctx.mark_non_differentiable(yp)
        return y, yp

    @staticmethod
    def backward(ctx, g, _gyp=None):
        x, w, *mask = ctx.saved_tensors
        dbias = None
        if mask:      # K9's backward rebuilds dz from the pooled gradient and the mask alone; from there on it is the unpooled backward
            g, dbias = _pool2_bwd(g, mask[0], mask[0].shape[:2] + (x.shape[2] + 2 * ctx.pad - 2, x.shape[3] + 2 * ctx.pad - 2), ctx.has_bias)
        dx, dw = _conv3x3_grads(g.contiguous(), x, w, ctx.pad, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dx, dw, dbias, None, None, None, None


def _conv3x3_grads(g, x, w, pad, need_dx, need_dw):
    """(dx, dw) of ``conv2d(x, w, padding=pad)`` under the output gradient ``g`` (contiguous): K11's mode 1 and K12 where their
    shape rules hold, the library's kernels elsewhere.  The backward of ``_Conv3x3``, pooled or not."""
    lib = _lib_or_raise()
    B, Ci, Hh, Ww = x.shape
    Co = w.shape[0]
    dx = dw = None
    if os.environ.get("AURPPO_NARROW_GRADS") == "1":      # opt-in: the narrow builds first, where their rules hold
        if need_dx and conv3x3_dgrad_narrow_ok(g, w, pad):
            dx, need_dx = conv3x3_dgrad_narrow(g, w, pad), False      # K11n
        if need_dw and conv3x3_wgrad_narrow_ok(g, x, Co, pad):
            dw, need_dw = conv3x3_wgrad_narrow(g, x, Co, pad), False      # K12n
    if need_dx and Ci % 32 != 0 and os.environ.get("AURPPO_K11_DGRAD16") != "1":
        # an input gradient with 16 output channels would leave half of every 32-wide matrix block empty: the library's kernel
        dx = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1,
                                                 [True, False, False])[0]
    elif need_dx:
        dx = torch.empty_like(x)
        ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Co, Ci), x.device)
        _check(lib.aurppo_conv3x3_f32(_ptr(g), _ptr(w.detach()), _ptr(dx), B, Ci, Co, g.shape[2], g.shape[3], pad, 1,
                                      *_ws_stream(ws)), "aurppo_conv3x3_f32")
    if need_dw:
        if conv3x3_wgrad_ok(x, Ci, Co, pad):
            dw = conv3x3_wgrad(g, x, Co, pad)       # K12
        else:
            # small channel counts would leave most of K12's 128 x 128 tile empty: the library's implicit-GEMM kernels
            dw = torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1,
                                                     [False, True, False])[1]
    return dx, dw


def _conv_tensor_ok(t, pad=0):
    """The tensor rule every shape predicate of this family starts from: a CUDA fp32 4-d tensor (and a padding of 0..2)."""
    return t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and pad in (0, 1, 2)


def _conv_grad(name, query, qargs, kind, g, other, out_shape, dims):
    """One gradient of the K12 / K11n / K12n family, ``name(g, other, out, *dims, workspace, stream)``: the byte query (0: the entry
    does not take the shape), the workspace of ``kind``, the output, the checked call."""
    lib = _lib_or_raise()
    nb = getattr(lib, query)(*qargs)
    if nb == 0:
        raise RuntimeError(f"aur_ppo_amd: {name} does not take this shape")
    ws = _workspace(kind, nb, g.device)
    out = torch.empty(out_shape, dtype=torch.float32, device=g.device)
    _check(getattr(lib, name)(_ptr(g), _ptr(other.detach()), _ptr(out), *dims, *_ws_stream(ws)), name)
    return out


def conv3x3_wgrad_ok(x, cin, cout, pad):
    """K12's shape rule: the product's tile is 128 (64 for cout <= 64) output channels x 128 (192) filter columns (cin * 9), and
    the layers below 64 output channels / 32 input channels leave most of it empty (the library's small-tile kernels win there).
    ``AURPPO_NO_K12=1`` switches it off, ``AURPPO_K12_ALL=1`` takes every shape the kernel accepts (tests)."""
    env = os.environ
    if env.get("AURPPO_NO_K12") == "1" or not _conv_tensor_ok(x, pad):
        return False
    if _lib_or_raise().aurppo_conv3x3_wgrad_ws_bytes(x.shape[0], cin, cout, x.shape[2], x.shape[3], pad) == 0:
        return False
    if env.get("AURPPO_K12_ALL") == "1":
        return True
    pixels = x.shape[0] * (x.shape[2] + 2 * pad - 2) * (x.shape[3] + 2 * pad - 2)
    return cout >= K12_MIN_COUT and cin >= K12_MIN_CIN and pixels >= K12_MIN_PIXELS


def conv3x3_wgrad(g, x, cout, pad):
    """K12: the gradient of ``conv2d(x, w (cout, cin, 3, 3), padding=pad)`` with respect to ``w`` given the output gradient ``g``
    (csrc/conv.hip::k_conv3x3_wgrad: a product over the batch's output pixels, both operands split once per workgroup)."""
    g, x = g.contiguous(), x.contiguous()
    B, Ci, Hh, Ww = x.shape
    assert g.shape == (B, cout, Hh + 2 * pad - 2, Ww + 2 * pad - 2), (g.shape, x.shape, cout, pad)
    dims = (B, Ci, cout, Hh, Ww, int(pad))
    return _conv_grad("aurppo_conv3x3_wgrad_f32", "aurppo_conv3x3_wgrad_ws_bytes", dims, "wgrad", g, x, (cout, Ci, 3, 3), dims)


def _narrow_tensor_ok(t):
    return _conv_tensor_ok(t) and t.is_contiguous()


def conv3x3_dgrad_narrow_ok(g, w, pad):
    """K11n's rule for the input gradient of ``conv2d(x, w (Co, Ci, 3, 3), padding=pad)`` under ``g`` (B, Co, Ho, Wo): contiguous CUDA
    fp32 4-d tensors, Ci in 1..16, Co a multiple of 32, pad 0..2 (the library's byte query says so), and at least
    ``NARROW_MIN_PIXELS`` pixels in ``g``."""
    if not (_narrow_tensor_ok(g) and _narrow_tensor_ok(w) and pad in (0, 1, 2) and tuple(w.shape[2:]) == (3, 3) and g.shape[1] == w.shape[0]):
        return False
    if g.shape[2] + 2 - 2 * pad <= 0 or g.shape[3] + 2 - 2 * pad <= 0:
        return False
    if _lib_or_raise().aurppo_conv3x3_dgrad_narrow_wop_bytes(w.shape[1], w.shape[0]) == 0:
        return False
    return g.shape[0] * g.shape[2] * g.shape[3] >= NARROW_MIN_PIXELS


def conv3x3_dgrad_narrow(g, w, pad):
    """K11n: the gradient of ``conv2d(x, w (Co, Ci <= 16, 3, 3), padding=pad)`` with respect to ``x`` given the output gradient ``g``
    (csrc/conv_narrow.hip::k_conv3x3_narrow_dgrad: 16-wide matrix blocks, the dy tile split once for all nine taps)."""
    B, Co, Ho, Wo = g.shape
    Ci = w.shape[1]
    Hh, Ww = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
    return _conv_grad("aurppo_conv3x3_dgrad_narrow_f32", "aurppo_conv3x3_dgrad_narrow_wop_bytes", (Ci, Co), "dgrad_narrow", g, w,
                      (B, Ci, Hh, Ww), (B, Ci, Co, Hh, Ww, int(pad)))


def conv3x3_wgrad_narrow_ok(g, x, cout, pad):
    """K12n's rule for the weight gradient of ``conv2d(x, w (cout, Ci, 3, 3), padding=pad)``: contiguous CUDA fp32 4-d tensors, Ci in
    1..16, cout in 1..32, pad 0..2 and an addressable shape (the library's byte query), and at least ``NARROW_MIN_PIXELS`` pixels
    in ``g``."""
    if not (_narrow_tensor_ok(g) and _narrow_tensor_ok(x) and pad in (0, 1, 2)):
        return False
    B, Ci, Hh, Ww = x.shape
    if tuple(g.shape) != (B, cout, Hh + 2 * pad - 2, Ww + 2 * pad - 2):
        return False
    if _lib_or_raise().aurppo_conv3x3_wgrad_narrow_ws_bytes(B, Ci, cout, Hh, Ww, pad) == 0:
        return False
    return g.shape[0] * g.shape[2] * g.shape[3] >= NARROW_MIN_PIXELS


def conv3x3_wgrad_narrow(g, x, cout, pad):
    """K12n: the gradient of ``conv2d(x, w (cout <= 32, Ci <= 16, 3, 3), padding=pad)`` with respect to ``w`` given ``g``
    (csrc/conv_narrow.hip::k_conv3x3_narrow_wgrad: a wave owns the whole 32 x 144 filter and a slice of the pixels; slices folded in order)."""
    B, Ci, Hh, Ww = x.shape
    assert g.shape == (B, cout, Hh + 2 * pad - 2, Ww + 2 * pad - 2), (g.shape, x.shape, cout, pad)
    dims = (B, Ci, cout, Hh, Ww, int(pad))
    return _conv_grad("aurppo_conv3x3_wgrad_narrow_f32", "aurppo_conv3x3_wgrad_narrow_ws_bytes", dims, "wgrad_narrow", g, x,
                      (cout, Ci, 3, 3), dims)


def _conv3x3_shape_ok(x, cin, cout, pixels):
    """What K11 and K11p ask of the channels of ``x`` (``_conv_tensor_ok``) and of a product of ``pixels`` rows (``conv3x3_ok`` says why)."""
    # a workgroup takes 256 output pixels x 128 output channels: the launch needs a few hundred of them to fill 256 CUs
    return (x.shape[1] == cin and cin % 16 == 0 and cout % 32 == 0
            and (pixels >= CONV3X3_MIN_PIXELS or ((pixels + 255) // 256) * ((cout + 127) // 128) >= CONV3X3_MIN_WGS))


def _conv3x3_module_ok(conv):
    """An ``nn.Conv2d`` K11 / K11p can stand in for: 3x3 kernel, stride 1, square zero padding 0..2, no dilation / groups."""
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and conv.padding in ((0, 0), (1, 1), (2, 2)) and conv.padding_mode == "zeros")


def conv3x3_ok(x, cin, cout, pad):
    """K11's shape rule for ``conv2d(x, w (cout, cin, 3, 3), padding=pad)``, stride 1: a CUDA fp32 NCHW tensor, cin a multiple
    of 16 (one k-step = 16 channels of a tap), cout a multiple of 32 (whole matrix blocks), and enough output pixels -- a workgroup
    takes 256 of them, and below ~512 workgroups (the encoder's last 3x3 -> 1x1 layers) the launch is a handful of long serial K
    loops that the library's kernels beat."""
    return _conv_tensor_ok(x, pad) and _conv3x3_shape_ok(x, cin, cout, x.shape[0] * (x.shape[2] + 2 * pad - 2) * (x.shape[3] + 2 * pad - 2))


def conv3x3_supported(x, conv):
    """``conv3x3_ok`` for an ``nn.Conv2d`` (``_conv3x3_module_ok``)."""
    return _conv3x3_module_ok(conv) and conv3x3_ok(x, conv.in_channels, conv.out_channels, conv.padding[0])


def conv3x3(x, weight, padding):
    """K11: ``conv2d(x, weight, None, stride=1, padding=padding)`` for a 3x3 filter on the bf16 matrix pipe (fp32 products from
    three-way bf16 splits), forward and input gradient (src/nets/base_cnns.py:32-45's hidden convolutions)."""
    return _Conv3x3.apply(x, weight, None, None, int(padding), False, False)


def conv3x3_pool_ok(x, cin, cout, pad):
    """K11p's shape rule: ``conv3x3_ok``'s with the pixel count taken as the four positions of every whole pooling window
    (4 * B * Hp * Wp: an odd trailing row / column is never computed), and at least one window."""
    if not _conv_tensor_ok(x, pad):
        return False
    hp, wp = (x.shape[2] + 2 * pad - 2) // 2, (x.shape[3] + 2 * pad - 2) // 2
    return hp >= 1 and wp >= 1 and _conv3x3_shape_ok(x, cin, cout, 4 * x.shape[0] * hp * wp)


def conv3x3_pool_supported(x, conv):
    """``conv3x3_pool_ok`` for an ``nn.Conv2d`` that a ReLU and a ``MaxPool2d(2)`` follow (``conv3x3_supported``'s module rule)."""
    return _conv3x3_module_ok(conv) and conv3x3_pool_ok(x, conv.in_channels, conv.out_channels, conv.padding[0])


def conv3x3_pool(x, weight, bias, padding):
    """K11p: ``max_pool2d(relu(conv2d(x, weight, bias, padding=padding)), 2)`` in one launch -- K11 with K9's bias / ReLU / pool in
    its epilogue, bit for bit ``bias_relu_pool2(conv3x3(x, weight, padding), bias)`` without the full-resolution tensor in
    between.  The backward is K9's (the mask is saved) followed by ``conv3x3``'s."""
    return _Conv3x3.apply(x, weight, bias, None, int(padding), True, False)


# ------------------------------------------------------------------ K11x: activations kept as bf16 planes
def split_planes(x):
    """The planes of an fp32 NCHW ``x`` with whole groups of eight channels (include/aurppo.h, K11x): int16
    (B, C / 8, 3, H * W, 8), the three bf16 parts of every value in the order K11's lanes read them."""
    lib = _lib_or_raise()
    x = x.detach().contiguous()
    xp = _planes_like(x)
    B, Cc, Hh, Ww = x.shape
    _check(lib.aurppo_split_planes_f32(_ptr(x), _ptr(xp, torch.int16), B, Cc, Hh, Ww, _stream()), "aurppo_split_planes_f32")
    return xp


def _planes_of(x, xp):
    B, Cc, Hh, Ww = x.shape
    if xp.dtype != torch.int16 or tuple(xp.shape) != (B, Cc // 8, 3, Hh * Ww, 8) or Cc % 8 != 0:
        raise ValueError(f"planes of shape {tuple(xp.shape)} ({xp.dtype}) do not belong to an input of shape {tuple(x.shape)}")
    return _ptr(xp, torch.int16)


def conv3x3_planes(x, xp, weight, padding):
    """K11 on planes: ``conv3x3(x, weight, padding)``, bit for bit, computed from ``xp`` -- the planes of ``x`` that its producer
    wrote (``first_block`` / ``conv3x3_pool_planes`` with ``want_planes``, or ``split_planes``).  ``x`` takes the gradient."""
    if xp is None:
        raise ValueError("conv3x3_planes: no planes given (conv3x3 reads x itself)")
    return _Conv3x3.apply(x, weight, None, xp, int(padding), False, False)


def conv3x3_pool_planes(x, xp, weight, bias, padding, want_planes=False):
    """K11p on planes: ``conv3x3_pool(x, weight, bias, padding)``, bit for bit, reading ``xp`` (the planes of ``x``; None: ``x`` itself)
    and, with ``want_planes``, returning ``(y, yp)`` -- ``yp == split_planes(y)``, written by the same launch for the next block."""
    return _Conv3x3.apply(x, weight, bias, xp, int(padding), True, bool(want_planes))


def like_gpu(shape):
    """What the shape rules above ask of a tensor, for an fp32 CUDA tensor of ``shape`` that does not exist yet (a block's output)."""
    import types
    shape = tuple(int(v) for v in shape)
    return types.SimpleNamespace(shape=shape, dtype=torch.float32, is_cuda=True, dim=lambda: len(shape))


LINEAR_MIN_ROWS = 32768


def linear_ok(x, in_features, out_features):
    """K11's row-major sibling takes ``x (M, in) @ w (out, in).T`` on a CUDA fp32 contiguous matrix when the inner dimension is a
    multiple of 16, the output width a multiple of 32, and there are enough rows to fill the chip (a workgroup takes 256)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == in_features and in_features % 16 == 0
            and out_features % 32 == 0 and x.shape[0] >= LINEAR_MIN_ROWS)


def linear_nobias(x, w, mode=0):
    """mode 0: ``x @ w.T``; mode 1: ``x @ w`` (the gradient of mode 0 with respect to its input, x being dY) -- fp32 products formed
    from three-way bf16 splits on the MFMA pipe (csrc/linear.hip::k_linear).  The inner dimension: mode 0 any width (no multiple of 16:
    k_linear_tail, which reads nothing past a row's floats), mode 1 a multiple of 16."""
    lib = _lib_or_raise()
    x, w = x.contiguous(), w.contiguous()
    M = x.shape[0]
    Nw, Kw = w.shape
    y = torch.empty((M, Nw if mode == 0 else Kw), dtype=torch.float32, device=x.device)
    ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Kw if mode == 0 else Nw, Nw if mode == 0 else Kw), x.device)
    _check(lib.aurppo_linear_f32(_ptr(x), _ptr(w), _ptr(y), M, Kw, Nw, int(mode), *_ws_stream(ws)),
           "aurppo_linear_f32")
    return y


def _linear_wgrad(gy, x, rows):
    lib = _lib_or_raise()
    gy, x = gy.contiguous(), x.contiguous()
    M, N = gy.shape
    K = x.shape[1]
    if rows is not None and rows.numel() != M:
        raise ValueError("linear_wgrad_rows: one index per row of gy")
    ws = _workspace("wgrad", lib.aurppo_linear_wgrad_ws_bytes(M, N, K), x.device)
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device)
    if rows is None:
        _check(lib.aurppo_linear_wgrad_f32(_ptr(gy), _ptr(x.detach()), _ptr(dw), M, N, K, *_ws_stream(ws)), "aurppo_linear_wgrad_f32")
    else:
        _check(lib.aurppo_linear_wgrad_rows_f32(_ptr(gy), _ptr(x), _ptr(rows, torch.int32), _ptr(dw), M, N, K, *_ws_stream(ws)),
               "aurppo_linear_wgrad_rows_f32")
    return dw


def linear_wgrad(gy, x):
    """``gy.T @ x`` -- nn.Linear's weight gradient -- on the bf16 matrix pipe (csrc/linear.hip::k_linear_wgrad: both operands split
    once per workgroup through LDS, the rows cut into slices that are summed in slice order).  ``gy``'s width a multiple of 4; ``x`` of
    any width (no multiple of 4: k_linear_wgrad_tail)."""
    return _linear_wgrad(gy, x, None)


def linear_wgrad_ok(gy, x):
    return (gy.is_cuda and gy.dtype == torch.float32 and gy.dim() == 2 and x.dim() == 2 and gy.shape[1] % 4 == 0 and x.shape[1] % 4 == 0
            and gy.shape[0] >= LINEAR_MIN_ROWS and gy.shape[1] >= 64 and x.shape[1] >= 64)


def _linear_bias_act(x, rows, w, bias, act):
    lib = _lib_or_raise()
    x, w = x.contiguous(), w.contiguous()
    M = x.shape[0] if rows is None else rows.numel()
    Nw, Kw = w.shape
    y = torch.empty((M, Nw), dtype=torch.float32, device=x.device)
    ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Kw, Nw), x.device)
    tail = (_ptr(w), _obias(bias), _ptr(y), M, Kw, Nw, int(act), *_ws_stream(ws))
    if rows is None:
        _check(lib.aurppo_linear_bias_act_f32(_ptr(x), *tail), "aurppo_linear_bias_act_f32")
    else:
        _check(lib.aurppo_linear_rows_bias_act_f32(_ptr(x), _ptr(rows, torch.int32), *tail), "aurppo_linear_rows_bias_act_f32")
    return y


def linear_bias_act(x, w, bias, act=0):
    """``act(x @ w.T + bias)`` in one kernel (act: 0 none, 1 tanh): csrc/linear.hip::k_linear with the layer's tail in its epilogue.
    ``x`` of any width (``linear_nobias``, mode 0)."""
    return _linear_bias_act(x, None, w, bias, act)


def linear_small_bias_act(x, w, bias, act=0):
    """``linear_bias_act`` on the tile for small M (csrc/linear.hip::k_linear_small: a workgroup takes 128 rows x 32 or 64 columns,
    so a few thousand rows reach every CU): the same bits, forward only."""
    lib = _lib_or_raise()
    x, w = x.contiguous(), w.contiguous()
    M = x.shape[0]
    Nw, Kw = w.shape
    if x.dim() != 2 or x.shape[1] != Kw or (bias is not None and bias.numel() != Nw):
        raise ValueError("linear_small_bias_act: shape mismatch")
    y = torch.empty((M, Nw), dtype=torch.float32, device=x.device)
    ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Kw, Nw), x.device)
    _check(lib.aurppo_linear_small_bias_act_f32(_ptr(x), _ptr(w), _obias(bias), _ptr(y), M, Kw, Nw, int(act), *_ws_stream(ws)),
           "aurppo_linear_small_bias_act_f32")
    return y


def linear_pair_bias_act(xA, xC, wA, wC, bA, bC, act=0):
    """``(act(xA @ wA.T + bA), act(xC @ wC.T + bC))`` -- two products of one shape, an actor's and a critic's layer -- from ONE
    launch of the small-M product behind the two operand copies (csrc/linear.hip::k_linear_pair).  Each result is ``linear_bias_act``'s
    bit for bit.  ``xA`` may be ``xC``; each bias may be None."""
    lib = _lib_or_raise()
    xA, xC, wA, wC = xA.contiguous(), xC.contiguous(), wA.contiguous(), wC.contiguous()
    Nw, Kw = wA.shape
    if (xA.dim() != 2 or xA.shape != xC.shape or xA.shape[1] != Kw or wC.shape != wA.shape
            or any(b is not None and b.numel() != Nw for b in (bA, bC))):
        raise ValueError("linear_pair_bias_act: the two products do not have one shape")
    M = xA.shape[0]
    yA = torch.empty((M, Nw), dtype=torch.float32, device=xA.device)
    yC = torch.empty((M, Nw), dtype=torch.float32, device=xA.device)
    ws = _workspace("conv_pair", lib.aurppo_linear_pair_wop_bytes(Kw, Nw), xA.device)
    _check(lib.aurppo_linear_pair_bias_act_f32(_ptr(xA), _ptr(xC), _ptr(wA), _ptr(wC), _obias(bA), _obias(bC), _ptr(yA), _ptr(yC), M, Kw, Nw,
                                               int(act), *_ws_stream(ws)), "aurppo_linear_pair_bias_act_f32")
    return yA, yC


def first_block(obs, state, weight, bias, want_planes=False):
    """K10: ``max_pool2d(relu(conv2d(cat[obs, state tiled to a plane], weight, bias, padding=1)), 2)`` -- the first block of
    src/nets/base_cnns.py:28-31 on the input of src/models/robot_actor_critic.py:58-59 -- forward and backward without the
    full-resolution tensors.  ``weight``: (Co, Ci + 1, 3, 3), state plane last; Ci in 1..3, Co a multiple of 16.
    ``want_planes``: returns ``(y, yp)``, ``yp`` the planes of ``y`` (``split_planes``) written by the same launch."""
    return _FirstBlock.apply(obs, state, weight, bias, bool(want_planes))


def linear_rows_bias_act(x, rows, w, bias, act=0):
    """``act(x[rows] @ w.T + bias)`` without materialising ``x[rows]``: k_linear reads its rows through the int32 index."""
    return _linear_bias_act(x, rows, w, bias, act)


def linear_wgrad_rows(gy, x, rows):
    """``gy.T @ x[rows]`` (k_linear_wgrad with its x operand read through the index)."""
    return _linear_wgrad(gy, x, rows)


def linear_wgrad_bias(gy, x, rows=None):
    """``(gy.T @ x, gy.sum(0))`` (``x[rows]`` with an index) -- a layer's weight and bias gradient -- from one pass over ``gy``:
    k_linear_wgrad's BIAS builds sum the ``gy`` pieces they stage, in fp64, rounded once.  ``dw`` is ``linear_wgrad``'s bit for bit.
    Without ``rows`` the width of ``x`` must be a multiple of 4."""
    lib = _lib_or_raise()
    gy, x = gy.contiguous(), x.contiguous()
    M, N = gy.shape
    K = x.shape[1]
    if rows is not None and rows.numel() != M:
        raise ValueError("linear_wgrad_bias: one index per row of gy")
    ws = _workspace("wgrad", lib.aurppo_linear_wgrad_bias_ws_bytes(M, N, K), x.device)
    dw = torch.empty((N, K), dtype=torch.float32, device=x.device)
    db = torch.empty(N, dtype=torch.float32, device=x.device)
    _check(lib.aurppo_linear_wgrad_bias_f32(_ptr(gy), _ptr(x), _optr(rows, torch.int32), _ptr(dw), _ptr(db), M, N, K, *_ws_stream(ws)),
           "aurppo_linear_wgrad_bias_f32")
    return dw, db


def linear_dx_tanh(gz, w, h, out=None):
    """``(gz @ w) * (1 - h * h)``: a hidden layer's input gradient with tanh' of the layer below in the product's epilogue.
    ``out`` may be ``h``."""
    lib = _lib_or_raise()
    gz, w = gz.contiguous(), w.contiguous()
    M = gz.shape[0]
    Nw, Kw = w.shape
    if out is None:
        out = torch.empty((M, Kw), dtype=torch.float32, device=gz.device)
    if h.shape != (M, Kw) or out.shape != (M, Kw) or gz.shape[1] != Nw:
        raise ValueError("linear_dx_tanh: shape mismatch")
    ws = _workspace("conv", lib.aurppo_conv3x3_wop_bytes(Nw, Kw), gz.device)
    _check(lib.aurppo_linear_dx_tanh_f32(_ptr(gz), _ptr(w), _ptr(h), _ptr(out), M, Kw, Nw, *_ws_stream(ws)),
           "aurppo_linear_dx_tanh_f32")
    return out


# ------------------------------------------------------------------ K13 + the layered step
def head_layout(layout):
    """K13's seven offsets out of a layered (or K7w) layout: actor head w, b; critic head w, b; actor_logstd; the biases of the two last hidden layers."""
    o, L = layout["offsets"], layout["num_layers"]
    per = 2 * (L + 1)
    return [o[2 * L], o[2 * L + 1], o[per + 2 * L], o[per + 2 * L + 1], o[2 * per], o[2 * L - 1], o[per + 2 * L - 1]]


def head_ppo(hA, hC, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
             vloss_mode=VLOSS_CLIPPED, out_scalars=None, gzA=None, gzC=None):
    """K13: both heads, the action distribution, the PPO loss and their backward from the last hidden activations ``hA`` /
    ``hC`` (M, H).  Writes ``gzA`` / ``gzC`` (default: in place of the activations), the heads', actor_logstd's and the last
    hidden layers' bias gradients at their bucket offsets in ``flat_grad``, and returns the 9 scalars."""
    lib = _lib_or_raise()
    _refuse_ragged_hidden("head_ppo", layout)
    M, Hd = hA.shape
    A, n = layout["A"], layout["n_params"]
    gzA, gzC = hA if gzA is None else gzA, hC if gzC is None else gzC
    if hC.shape != (M, Hd) or gzA.shape != (M, Hd) or gzC.shape != (M, Hd) or idx.numel() != M or Hd != layout["hidden"]:
        raise ValueError("head_ppo: shape mismatch")
    if not _mlp_buffers_ok(None, actions, rec, layout):
        raise ValueError("head_ppo: buffer shapes do not match the policy")
    _bucket_fits(n, flat_param, flat_grad, who="head_ppo")
    if out_scalars is None:
        out_scalars = torch.empty(N_SCALARS, dtype=torch.float32, device=hA.device)
    fn, entry = _head_entry(lib, layout, "ppo_f32")
    nb = _head_entry(lib, layout, "ppo_workspace_bytes")[0](M, Hd, A)
    if nb == 0:
        raise RuntimeError(f"aur_ppo_amd: {entry} does not take this shape")
    ws = _workspace("head", nb, hA.device)
    lay = (C.c_int * 7)(*head_layout(layout))
    _check(fn(
        *_step_prefix((hA, hC, gzA, gzC), actions, rec, idx, (M, Hd, A, int(layout["continuous"])), flat_param, lay, n, flat_grad, clip,
                      ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars), *_ws_stream(ws)), entry)
    return out_scalars


_layered_cache = {}


def _layered_buffers(M, layout, device):
    """Activations of one minibatch, (M, hidden) per hidden layer and net, kept per (M, shape): a captured update replays into them."""
    key = (M, layout["hidden"], layout["num_layers"], device.index if device.index is not None else torch.cuda.current_device())
    buf = _layered_cache.get(key)
    if buf is None:
        buf = [[torch.empty((M, layout["hidden"]), dtype=torch.float32, device=device) for _ in range(layout["num_layers"])]
               for _net in range(2)]
        _layered_cache[key] = buf
    return buf


def mlp_layered_step(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                     vloss_mode=VLOSS_CLIPPED, out_scalars=None):
    """``mlp_ppo_step``'s contract for the MLP policies wider than the fused kernels (``mlp_layered_layout``): gather + evaluate +
    loss + backward of one minibatch, overwriting ``flat_grad[:n_params]`` and returning the 9 scalars -- no autograd, no host
    synchronisation.  Per net: layer 0 through the index (k_linear, bias + tanh in the epilogue), layers 1 .. L - 1, then K13
    (heads, distribution, loss, their backward; its statistics and fold launches), then from the last layer down the weight
    gradient (k_linear_wgrad, layer 0's x through the index), the input gradient with tanh' (k_linear) and the bias
    gradient (a column sum)."""
    lib = _lib_or_raise()
    _refuse_ragged_hidden("mlp_layered_step", layout)
    _refuse_wide_actions("mlp_layered_step", layout)
    M, D, Hd, L, n = idx.numel(), layout["D"], layout["hidden"], layout["num_layers"], layout["n_params"]
    if not layout.get("layered") or not _mlp_buffers_ok(obs, actions, rec, layout):
        raise ValueError("mlp_layered_step: buffer shapes do not match the policy")
    _bucket_fits(n, flat_param, flat_grad, who="mlp_layered_step")
    dev = obs.device
    if out_scalars is None:
        out_scalars = torch.empty(N_SCALARS, dtype=torch.float32, device=dev)
    acts = _layered_buffers(M, layout, dev)
    wop = C.c_void_p(_workspace("conv", lib.aurppo_conv3x3_wop_bytes(max(D, Hd), Hd), dev).data_ptr())
    wgw = C.c_void_p(_workspace("wgrad", max(lib.aurppo_linear_wgrad_ws_bytes(M, Hd, D), lib.aurppo_linear_wgrad_ws_bytes(M, Hd, Hd)),
                                dev).data_ptr())
    st, off, per = _stream(), layout["offsets"], 2 * (L + 1)
    p0, g0 = _ptr(flat_param).value, _ptr(flat_grad).value
    obs_p, idx_p = _ptr(obs), _ptr(idx, torch.int32)

    def at(base, o):
        return C.c_void_p(base + 4 * o)
    for net in range(2):
        o, h = off[net * per:(net + 1) * per], acts[net]
        _check(lib.aurppo_linear_rows_bias_act_f32(obs_p, idx_p, at(p0, o[0]), at(p0, o[1]), _ptr(h[0]), M, D, Hd, 1, wop, st),
               "aurppo_linear_rows_bias_act_f32")
        for l in range(1, L):
            _check(lib.aurppo_linear_bias_act_f32(_ptr(h[l - 1]), at(p0, o[2 * l]), at(p0, o[2 * l + 1]), _ptr(h[l]), M, Hd, Hd, 1, wop, st),
                   "aurppo_linear_bias_act_f32")
    head_ppo(acts[0][L - 1], acts[1][L - 1], actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv,
             vloss_mode, out_scalars)
    for net in range(2):
        o, h = off[net * per:(net + 1) * per], acts[net]        # h[l] now holds gz_l for l = L - 1; lower layers follow in place
        for l in range(L - 1, 0, -1):
            _check(lib.aurppo_linear_wgrad_f32(_ptr(h[l]), _ptr(h[l - 1]), at(g0, o[2 * l]), M, Hd, Hd, wgw, st), "aurppo_linear_wgrad_f32")
            _check(lib.aurppo_linear_dx_tanh_f32(_ptr(h[l]), at(p0, o[2 * l]), _ptr(h[l - 1]), _ptr(h[l - 1]), M, Hd, Hd, wop, st),
                   "aurppo_linear_dx_tanh_f32")
            torch.sum(h[l - 1], 0, out=flat_grad[o[2 * l - 1]:o[2 * l - 1] + Hd])
        _check(lib.aurppo_linear_wgrad_rows_f32(_ptr(h[0]), obs_p, idx_p, at(g0, o[0]), M, Hd, D, wgw, st), "aurppo_linear_wgrad_rows_f32")
    return out_scalars


def _layered_native(lib, who, obs, actions, rec, idx, flat_param, layout, *buckets):
    """The checks and the three argument runs the two native layered calls share: layout array, shape, workspace."""
    if not layout.get("layered") or not _mlp_buffers_ok(obs, actions, rec, layout):
        raise ValueError(f"{who}: buffer shapes do not match the policy")
    _bucket_fits(layout["n_params"], flat_param, *buckets, who=who)
    lay, shape = _layout_shape(layout, idx.numel())
    nb = _layered_entry(lib, layout, "step_workspace_bytes")[0](shape[0], layout["D"], layout["A"], layout["hidden"], layout["num_layers"])
    if nb == 0:
        raise RuntimeError(f"aur_ppo_amd: {who} does not take this shape")
    return lay, shape, _workspace(_layered_ws_kind("layered_step", layout), nb, obs.device)


def mlp_layered_step_native(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                            vloss_mode=VLOSS_CLIPPED, out_scalars=None):
    """``mlp_layered_step`` as one native call (aurppo_mlp_layered_step_f32): the same products and K13 in the same order from one
    workspace, and the lower layers' bias gradients out of the weight-gradient kernel (fp64 sums, rounded once) instead of a column
    sum per layer.  Everything but those bias gradients is ``mlp_layered_step``'s bit for bit."""
    lib = _lib_or_raise()
    lay, shape, ws = _layered_native(lib, "mlp_layered_step_native", obs, actions, rec, idx, flat_param, layout, flat_grad)
    if out_scalars is None:
        out_scalars = torch.empty(N_SCALARS, dtype=torch.float32, device=obs.device)
    fn, entry = _layered_entry(lib, layout, "step_f32")
    _check(fn(*_step_prefix((obs,), actions, rec, idx, shape, flat_param, lay, layout["n_params"], flat_grad, clip, ent_coef, vf_coef, norm_adv,
                            vloss_mode, out_scalars), *_ws_stream(ws)), entry)
    return out_scalars


def mlp_layered_minibatch(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                          out_scalars, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps, out_norm):
    """``mlp_layered_step_native`` + ``clip_grad_norm_`` + ``Adam.step`` over ``[0, n_params)`` in one native call
    (aurppo_mlp_layered_minibatch_f32): one whole minibatch (src/ppo.py:219-269) of a layered policy.  Single process only."""
    lib = _lib_or_raise()
    lay, shape, ws = _layered_native(lib, "mlp_layered_minibatch", obs, actions, rec, idx, flat_param, layout, flat_grad, exp_avg,
                                     exp_avg_sq)
    fn, entry = _layered_entry(lib, layout, "minibatch_f32")
    _check(fn(*_step_prefix((obs,), actions, rec, idx, shape, flat_param, lay, layout["n_params"], flat_grad, clip, ent_coef, vf_coef, norm_adv,
                            vloss_mode, out_scalars),
              *_adam_tail(exp_avg, exp_avg_sq, max_norm, lr_dev, step_dev, betas, eps, out_norm), *_ws_stream(ws)), entry)
    return out_scalars


# ------------------------------------------------------------------ K14 + the layered rollout step
def head_act_layout(layout):
    """K14's five offsets out of a layered (or K7w) layout: actor head w, b; critic head w, b; actor_logstd."""
    return head_layout(layout)[:5]


def _act_outputs(who, N, layout, noise, actions, logp, value, device):
    """``mlp_act``'s output rule: the value always; with noise, the actions ((N, A), or (N,) indices for the Categorical head) and
    the log-prob.  Allocates what the caller did not pass; raises ValueError on a mismatch."""
    A, cont = layout["A"], layout["continuous"]
    if value is None:
        value = torch.empty(N, dtype=torch.float32, device=device)
    if noise is not None:
        if actions is None:
            actions = torch.empty((N, A) if cont else (N,), dtype=torch.float32, device=device)
        if logp is None:
            logp = torch.empty(N, dtype=torch.float32, device=device)
        if noise.numel() != (N * A if cont else N) or actions.numel() != noise.numel() or logp.numel() != N:
            raise ValueError(f"{who}: noise / output shapes do not match the policy")
    if value.numel() != N:
        raise ValueError(f"{who}: value shape does not match the policy")
    return actions, logp, value


def _act_outputs_ptrs(noise, actions, logp, value):
    """actions, logp, value (the first two NULL without noise)."""
    return (_optr(actions if noise is not None else None), _optr(logp if noise is not None else None), _ptr(value))


def head_act(hA, hC, noise, flat_param, layout, actions=None, logp=None, value=None):
    """K14: both heads, the sampled action, its log-prob and the value from the last hidden activations ``hA`` / ``hC`` (N, H).
    ``noise`` as ``mlp_act``'s; None -> the value only (``hA`` may then be None).  Returns (actions, logp, value)."""
    lib = _lib_or_raise()
    _refuse_ragged_hidden("head_act", layout)
    N, Hd = hC.shape
    if Hd != layout["hidden"] or (noise is not None and (hA is None or hA.shape != (N, Hd))):
        raise ValueError("head_act: activation shapes do not match the policy")
    actions, logp, value = _act_outputs("head_act", N, layout, noise, actions, logp, value, hC.device)
    _bucket_fits(layout["n_params"], flat_param, who="head_act")
    lay = (C.c_int * 5)(*head_act_layout(layout))
    fn, entry = _head_entry(lib, layout, "act_f32")
    _check(fn(_optr(hA if noise is not None else None), _ptr(hC), _optr(noise), N, Hd, layout["A"], int(layout["continuous"]),
              _ptr(flat_param), lay, layout["n_params"], *_act_outputs_ptrs(noise, actions, logp, value), _stream()), entry)
    return actions, logp, value


_layered_wop_cache = {}


def _layered_wop(lib, layout, device):
    """The prepared-weights buffer of a layered shape: a tensor of its own per (shape, device) -- not ``_workspace("conv")``, which
    every other linear call overwrites."""
    D, Hd, L = layout["D"], layout["hidden"], layout["num_layers"]
    key = (D, Hd, L, device.index if device.index is not None else torch.cuda.current_device())
    wop = _layered_wop_cache.get(key)
    if wop is None:
        nb = _layered_entry(lib, layout, "wop_bytes")[0](D, Hd, L)
        if nb == 0:
            raise RuntimeError("aur_ppo_amd: aurppo_mlp_layered_prep_f32 does not take this shape")
        wop = _layered_wop_cache[key] = torch.empty(nb, dtype=torch.uint8, device=device)
    return wop


def mlp_layered_prepare(flat_param, layout):
    """The operand-order copies of the 2 L hidden-layer matrices of a layered policy, built from ``flat_param`` as it stands now
    (k_conv_prep, 2 L launches) into the shape's prepared buffer, which is returned: pass it as ``wop`` to ``mlp_layered_act``
    for as long as the parameters stand still (a rollout).  No host synchronisation; capturable."""
    lib = _lib_or_raise()
    if not layout.get("layered"):
        raise ValueError("mlp_layered_prepare: not a layered layout")
    _bucket_fits(layout["n_params"], flat_param, who="mlp_layered_prepare")
    wop = _layered_wop(lib, layout, flat_param.device)
    lay, _ = _layout_shape(layout, 0)
    fn, entry = _layered_entry(lib, layout, "prep_f32")
    _check(fn(_ptr(flat_param), lay, layout["n_params"], layout["D"], layout["hidden"], layout["num_layers"], C.c_void_p(wop.data_ptr()),
              _stream()), entry)
    return wop


def mlp_layered_act(obs, noise, flat_param, layout, actions=None, logp=None, value=None, wop=None, paired=False):
    """``mlp_act``'s contract and return value for the MLP policies wider than the fused kernels (``mlp_layered_layout``): per net the
    hidden layers on k_linear (bias + tanh in the epilogue) from the prepared operand copies ``wop`` (``mlp_layered_prepare``;
    None: prepared here, from ``flat_param`` as it stands), then K14.  No host synchronisation; capturable.
    ``paired``: the same step, bit for bit, on the small-M products -- per layer one launch for both nets (k_linear_pair), L + 1
    launches where the default has 2 L + 1; same prepared buffer, same workspace."""
    lib = _lib_or_raise()
    N = obs.shape[0]
    if not layout.get("layered") or obs.dim() != 2 or obs.shape[1] != layout["D"]:
        raise ValueError("mlp_layered_act: obs shape does not match the policy")
    dev = obs.device
    actions, logp, value = _act_outputs("mlp_layered_act", N, layout, noise, actions, logp, value, dev)
    _bucket_fits(layout["n_params"], flat_param, who="mlp_layered_act")
    if wop is None:
        wop = mlp_layered_prepare(flat_param, layout)
    elif wop.numel() * wop.element_size() < _layered_entry(lib, layout, "wop_bytes")[0](layout["D"], layout["hidden"], layout["num_layers"]):
        raise ValueError("mlp_layered_act: the prepared buffer is smaller than the policy's operand copies")
    lay, shape = _layout_shape(layout, N)
    ws = _workspace(_layered_ws_kind("layered_act", layout), _layered_entry(lib, layout, "act_workspace_bytes")[0](N, layout["hidden"]), dev)
    fn, entry = _layered_entry(lib, layout, "act_paired_f32" if paired else "act_f32")
    _check(fn(_ptr(obs), _optr(noise), *shape, _ptr(flat_param), lay, layout["n_params"], *_act_outputs_ptrs(noise, actions, logp, value),
              C.c_void_p(wop.data_ptr()), *_ws_stream(ws)), entry)
    return actions, logp, value


# ------------------------------------------------------------------ K15 / K16: the device CartPole and the one-launch rollout on it
# ``env_state``: what ``envs.CartPoleDeviceVecEnv.native_state()`` returns -- ``state`` (N, 4) float64, ``steps`` / ``episode`` (N,) int32,
# ``seed``, ``env0`` (the global index of env 0) and ``consts`` (gravity, masscart, masspole, length, force_mag, tau, theta_lim, x_lim,
# max_steps).  Shapes and dtypes are checked (ValueError) before the library is reached.
def _cart_tensor(who, name, t, shape, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}")


def _cart_env(who, env_state, doubles=4, n_consts=9, consts_of="nine CartPole"):
    """N after the env-state checks (the device Pendulum's calls pass their own block width and constant count)."""
    steps = env_state["steps"]
    N = steps.numel() if isinstance(steps, torch.Tensor) else 0
    if N < 1:
        raise ValueError(f"{who}: no envs")
    _cart_tensor(who, "state", env_state["state"], (N, doubles), torch.float64)
    _cart_tensor(who, "steps", steps, (N,), torch.int32)
    _cart_tensor(who, "episode", env_state["episode"], (N,), torch.int32)
    if len(env_state["consts"]) != n_consts or int(env_state["env0"]) < 0:
        raise ValueError(f"{who}: consts must be the {consts_of} constants and env0 >= 0")
    return N


def _cart_env_ptrs(env_state):
    """state, steps, episode."""
    return (_ptr(env_state["state"], torch.float64), _ptr(env_state["steps"], torch.int32), _ptr(env_state["episode"], torch.int32))


def _cart_seed(env_state):
    """env0, seed_lo, seed_hi."""
    seed = int(env_state["seed"]) & 0xFFFFFFFFFFFFFFFF
    return (int(env_state["env0"]), seed & 0xFFFFFFFF, seed >> 32)


def _cart_consts(env_state):
    """gravity, masscart, masspole, length, force_mag, tau, theta_lim, x_lim, max_steps."""
    c = env_state["consts"]
    return (*[float(v) for v in c[:8]], int(c[8]))


def cartpole_reset(env_state, obs):
    """Episode 0 of every env: ``episode = steps = 0``, the state from the reset draw, ``obs`` (N, 4) = the state in fp32."""
    N = _cart_env("cartpole_reset", env_state)
    _cart_tensor("cartpole_reset", "obs", obs, (N, 4))
    lib = _lib_or_raise()
    _check(lib.aurppo_cartpole_reset(*_cart_env_ptrs(env_state), _ptr(obs), N, *_cart_seed(env_state), _stream()), "aurppo_cartpole_reset")
    return obs


def cartpole_step(env_state, action, obs, reward, done, ep_len):
    """K15: one step of every env.  ``action`` (N,) fp32 0.0 / 1.0 (as K8 writes it); writes ``obs`` (N, 4) (the reset observation where
    the episode ended), ``reward`` = 1, ``done`` 0.0 / 1.0 and ``ep_len`` (N,) int32: the finished episode's length, or 0."""
    who = "cartpole_step"
    N = _cart_env(who, env_state)
    _cart_tensor(who, "action", action, (N,))
    _cart_tensor(who, "obs", obs, (N, 4))
    _cart_tensor(who, "reward", reward, (N,))
    _cart_tensor(who, "done", done, (N,))
    _cart_tensor(who, "ep_len", ep_len, (N,), torch.int32)
    lib = _lib_or_raise()
    _check(lib.aurppo_cartpole_step(*_cart_env_ptrs(env_state), _ptr(action), _ptr(obs), _ptr(reward), _ptr(done), _ptr(ep_len, torch.int32),
                                    N, *_cart_seed(env_state), *_cart_consts(env_state), _stream()), "aurppo_cartpole_step")
    return obs, reward, done, ep_len


def cartpole_rollout_ok(layout):
    """K16's shape rule: K8's default layout (two layers of 64) with a Categorical head of 2 over CartPole's 4 floats."""
    return bool(layout is not None and not layout.get("wide") and not layout.get("layered") and not layout["continuous"]
                and layout["D"] == 4 and layout["A"] == 2 and layout["hidden"] == MLP_HIDDEN and layout["num_layers"] == 2)


def cartpole_rollout(env_state, flat_param, layout, noise, states, terminals, actions, log_probs, values, rewards, ep_len, next_obs,
                     next_done):
    """K16: T rollout steps in one launch -- per step t what ``mlp_act`` on ``noise[t]`` and ``cartpole_step`` leave, bit for bit, in
    the buffer rows ``states[t]`` (N, 4), ``terminals[t]``, ``actions[t]``, ``log_probs[t]``, ``values[t]``, ``rewards[t]`` and
    ``ep_len[t]`` (int32).  ``next_obs`` (N, 4) / ``next_done`` (N,) are read and written: on entry the current observation and done
    flag, on exit those behind the last step.  The env state is updated in place.  A policy shape other than ``cartpole_rollout_ok``'s
    is refused by the library (RuntimeError)."""
    who = "cartpole_rollout"
    N = _cart_env(who, env_state)
    if not isinstance(noise, torch.Tensor) or noise.dim() != 2 or noise.shape[0] < 1:
        raise ValueError(f"{who}: noise must be (T, N) uniform draws")
    T = noise.shape[0]
    _cart_tensor(who, "noise", noise, (T, N))
    _cart_tensor(who, "states", states, (T, N, 4))
    for name, t in (("terminals", terminals), ("actions", actions), ("log_probs", log_probs), ("values", values), ("rewards", rewards)):
        _cart_tensor(who, name, t, (T, N))
    _cart_tensor(who, "ep_len", ep_len, (T, N), torch.int32)
    _cart_tensor(who, "next_obs", next_obs, (N, 4))
    _cart_tensor(who, "next_done", next_done, (N,))
    _bucket_fits(layout["n_params"], flat_param, who=who)
    lib = _lib_or_raise()
    lay = (C.c_int * len(layout["offsets"]))(*layout["offsets"])
    _check(lib.aurppo_cartpole_rollout_f32(*_cart_env_ptrs(env_state), _ptr(next_obs), _ptr(next_done), _ptr(noise), N, T, layout["D"],
                                           layout["A"], int(layout["continuous"]), layout["hidden"], layout["num_layers"], _ptr(flat_param),
                                           lay, layout["n_params"], _ptr(states), _ptr(terminals), _ptr(actions), _ptr(log_probs),
                                           _ptr(values), _ptr(rewards), _ptr(ep_len, torch.int32), *_cart_seed(env_state),
                                           *_cart_consts(env_state), _stream()), "aurppo_cartpole_rollout_f32")
    return next_obs, next_done


# ------------------------------------------------------------------ K17 / K18: the device Pendulum and the one-launch rollout on it
# ``env_state``: what ``envs.PendulumDeviceVecEnv.native_state()`` returns -- ``state`` (N, 16) float64 (the row layout: include/aurppo.h),
# ``steps`` / ``episode`` (N,) int32, ``seed``, ``env0`` and ``consts`` (g, m, l, dt, max_speed, max_torque, max_steps).  Shapes and
# dtypes are checked (ValueError) before the library is reached, by the CartPole calls' helpers.
PENDULUM_STATE_DOUBLES = 16


def _pend_env(who, env_state):
    """N after the env-state checks."""
    return _cart_env(who, env_state, PENDULUM_STATE_DOUBLES, 7, "seven Pendulum")


def _pend_consts(env_state):
    """g, m, l, dt, max_speed, max_torque, max_steps."""
    c = env_state["consts"]
    return (*[float(v) for v in c[:6]], int(c[6]))


def pendulum_reset(env_state, obs):
    """Every env starts over: ``episode = steps = 0``, the state from the reset draw, fresh statistics that have taken the first raw
    observation; ``obs`` (N, 3) = its normalised form."""
    N = _pend_env("pendulum_reset", env_state)
    _cart_tensor("pendulum_reset", "obs", obs, (N, 3))
    lib = _lib_or_raise()
    _check(lib.aurppo_pendulum_reset(*_cart_env_ptrs(env_state), _ptr(obs), N, *_cart_seed(env_state), _stream()), "aurppo_pendulum_reset")
    return obs


def pendulum_step(env_state, action, obs, reward, done, ep_len, ep_ret):
    """K17: one step of every env.  ``action`` (N,) or (N, 1) fp32, the unclipped sample as K8 writes it; writes the normalised ``obs``
    (N, 3) (the reset observation where the episode ended) and ``reward``, ``done`` 0.0 / 1.0, and the finished episode's length
    ``ep_len`` (N,) int32 and raw return ``ep_ret`` (N,) fp32, or 0."""
    who = "pendulum_step"
    N = _pend_env(who, env_state)
    _cart_tensor(who, "action", action, (N, 1) if isinstance(action, torch.Tensor) and action.dim() == 2 else (N,))
    _cart_tensor(who, "obs", obs, (N, 3))
    _cart_tensor(who, "reward", reward, (N,))
    _cart_tensor(who, "done", done, (N,))
    _cart_tensor(who, "ep_len", ep_len, (N,), torch.int32)
    _cart_tensor(who, "ep_ret", ep_ret, (N,))
    lib = _lib_or_raise()
    _check(lib.aurppo_pendulum_step(*_cart_env_ptrs(env_state), _ptr(action), _ptr(obs), _ptr(reward), _ptr(done), _ptr(ep_len, torch.int32),
                                    _ptr(ep_ret), N, *_cart_seed(env_state), *_pend_consts(env_state), _stream()), "aurppo_pendulum_step")
    return obs, reward, done, ep_len, ep_ret


def pendulum_rollout_ok(layout):
    """K18's shape rule: K8's default layout (two layers of 64) with a Gaussian head of 1 over Pendulum's 3 floats."""
    return bool(layout is not None and not layout.get("wide") and not layout.get("layered") and layout["continuous"]
                and layout["D"] == 3 and layout["A"] == 1 and layout["hidden"] == MLP_HIDDEN and layout["num_layers"] == 2)


def pendulum_rollout(env_state, flat_param, layout, noise, states, terminals, actions, log_probs, values, rewards, ep_len, ep_ret, next_obs,
                     next_done):
    """K18: T rollout steps in one launch -- per step t what ``mlp_act`` on ``noise[t]`` and ``pendulum_step`` leave, bit for bit, in
    the buffer rows ``states[t]`` (N, 3), ``terminals[t]``, ``actions[t]`` (N, 1), ``log_probs[t]``, ``values[t]``, ``rewards[t]``,
    ``ep_len[t]`` (int32) and ``ep_ret[t]``.  ``noise``: (T, N, 1) standard-normal draws.  ``next_obs`` (N, 3) / ``next_done`` (N,) are
    read and written: on entry the current observation and done flag, on exit those behind the last step.  The env state is updated in
    place.  A policy shape other than ``pendulum_rollout_ok``'s is refused by the library (RuntimeError)."""
    who = "pendulum_rollout"
    N = _pend_env(who, env_state)
    if not isinstance(noise, torch.Tensor) or noise.dim() != 3 or noise.shape[0] < 1:
        raise ValueError(f"{who}: noise must be (T, N, 1) standard-normal draws")
    T = noise.shape[0]
    _cart_tensor(who, "noise", noise, (T, N, 1))
    _cart_tensor(who, "states", states, (T, N, 3))
    _cart_tensor(who, "actions", actions, (T, N, 1))
    for name, t in (("terminals", terminals), ("log_probs", log_probs), ("values", values), ("rewards", rewards), ("ep_ret", ep_ret)):
        _cart_tensor(who, name, t, (T, N))
    _cart_tensor(who, "ep_len", ep_len, (T, N), torch.int32)
    _cart_tensor(who, "next_obs", next_obs, (N, 3))
    _cart_tensor(who, "next_done", next_done, (N,))
    _bucket_fits(layout["n_params"], flat_param, who=who)
    lib = _lib_or_raise()
    lay = (C.c_int * len(layout["offsets"]))(*layout["offsets"])
    _check(lib.aurppo_pendulum_rollout_f32(*_cart_env_ptrs(env_state), _ptr(next_obs), _ptr(next_done), _ptr(noise), N, T, layout["D"],
                                           layout["A"], int(layout["continuous"]), layout["hidden"], layout["num_layers"], _ptr(flat_param),
                                           lay, layout["n_params"], _ptr(states), _ptr(terminals), _ptr(actions), _ptr(log_probs),
                                           _ptr(values), _ptr(rewards), _ptr(ep_len, torch.int32), _ptr(ep_ret), *_cart_seed(env_state),
                                           *_pend_consts(env_state), _stream()), "aurppo_pendulum_rollout_f32")
    return next_obs, next_done
