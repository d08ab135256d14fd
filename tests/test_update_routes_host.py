"""CPU: which kernels ``ppo._update_body`` calls on each of its six routes, in which order and with which slices -- with
recording stand-ins for the fused-step family on top of the oracle's ops.  T = 4, N = 4, two minibatches, two epochs: four steps,
so both ``next_idx`` rules (the next slice of the epoch; the first slice of the next epoch) and the final ``None`` are reached.

The step stand-ins write a known gradient (6 everywhere), the collectives change it (SUM: x world; mean / p2p: a constant), the
optimizer stand-ins zero it: the value ``first_grad_probe`` holds then says where its copy was taken and what it was divided by."""
import pytest
import torch

from aur_ppo_amd import dist as D
from aur_ppo_amd import hip_ops as H
from aur_ppo_amd.ppo import ppo
from tests import oracle_ops

T, N, E, MB = 4, 4, 2, 2
B, M = T * N, T * N // MB
STEPS = [(ep, start) for ep in range(E) for start in range(0, B, M)]
NEXT = STEPS[1:] + [None]
WORLD = 2


def _params():
    return dict(gym_id="Synthetic-v0", seed=1.0, num_steps=T, gae=True, total_timesteps=4 * B, anneal_lr=True, gae_lambda=0.95,
                num_update_epochs=E, num_envs=N, num_minibatches=MB, entropy_coeff=0.01, value_coeff=0.5, clip_coeff=0.2,
                clip_vloss=True, max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=64,
                continuous=True, obs_dim=5, act_dim=3, learning_rate=2.5e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99,
                track=False, log=False, save=False, device="cpu")


class Recorder:
    """The oracle's ops (imported, not copied) + recording stand-ins for the fused-step family; ``log`` is the ordered call list."""

    def __init__(self, agent_ref):
        self.log, self._agent = [], agent_ref
        for k in dir(oracle_ops):
            if not k.startswith("_") and not hasattr(self, k):
                setattr(self, k, getattr(oracle_ops, k))

    # ---- what an argument IS, by identity / storage offset
    def _slice(self, idx):
        if idx is None:
            return None
        a = self._agent[0]
        assert idx.dtype == torch.int32 and idx.untyped_storage().data_ptr() == a._test_perms.untyped_storage().data_ptr()
        off = idx.storage_offset()
        return (off // B, off % B, idx.numel())

    def _row(self, t, of, width):
        assert t.untyped_storage().data_ptr() == of.untyped_storage().data_ptr() and t.numel() == width
        return t.storage_offset() // width

    def _pair(self, actions, rec):
        a = self._agent[0]
        if actions is None:
            assert rec is a._rec64
            return "packed"
        assert actions.data_ptr() == a.buffer.actions.data_ptr() and rec is a._rec
        return "separate"

    def _bucket(self, flat_param, flat_grad):
        a = self._agent[0]
        assert flat_param is a.bucket.flat_param and flat_grad is a.bucket.flat_grad

    def _adam(self, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps):
        a = self._agent[0]
        assert exp_avg is a._adam_m and exp_avg_sq is a._adam_v and lr_dev is a._lr_tensor and step_dev is a._adam_t
        assert (max_norm, tuple(betas), eps) == (0.5, (0.9, 0.999), 1e-5)

    def _step_common(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars):
        a = self._agent[0]
        scratch = flat_grad is not a.bucket.flat_grad          # probe_mlp_step: gradients and scalars go to buffers of its own
        assert flat_param is a.bucket.flat_param and flat_grad.shape == a.bucket.flat_grad.shape
        assert obs.data_ptr() == a.buffer.states.data_ptr() and obs.shape == (B, 5)
        assert (clip, ent_coef, vf_coef, norm_adv, vloss_mode) == (0.2, 0.01, 0.5, True, self.VLOSS_CLIPPED)
        flat_grad.fill_(6.0)
        out_scalars.zero_()
        return dict(idx=self._slice(idx), pair=self._pair(actions, rec), scalars=None if scratch else self._row(out_scalars, a._scalars, self.N_SCALARS),
                    layout="layered" if layout is a._mlp_layered else "fused" if layout is a._mlp else "?")

    # ---- the stand-ins
    def mlp_ppo_step(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                     vloss_mode=1, out_scalars=None, events=None):
        self.log.append(("mlp_ppo_step", self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef,
                                                           norm_adv, vloss_mode, out_scalars)))
        return out_scalars

    def mlp_layered_step(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv=True,
                         vloss_mode=1, out_scalars=None):
        self.log.append(("mlp_layered_step", self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef,
                                                               norm_adv, vloss_mode, out_scalars)))
        return out_scalars

    def mlp_ppo_minibatch(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                          out_scalars, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps, out_norm, next_idx=None, chained=False):
        e = self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars)
        self._adam(exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps)
        e.update(next=self._slice(next_idx), chained=chained, norm=self._row(out_norm, self._agent[0]._norms, 1))
        flat_grad.zero_()
        out_norm.zero_()
        self.log.append(("mlp_ppo_minibatch", e))
        return out_scalars

    def mlp_ppo_grad(self, obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode,
                     out_scalars, step_dev, chained=False):
        e = self._step_common(obs, actions, rec, idx, flat_param, layout, flat_grad, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars)
        assert step_dev is self._agent[0]._adam_t
        e.update(chained=chained)
        self.log.append(("mlp_ppo_grad", e))
        return out_scalars

    def _apply(self, name, flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm, rec, next_idx, **more):
        a = self._agent[0]
        self._bucket(flat_param, flat_grad)
        self._adam(exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps)
        assert layout is a._mlp
        self.log.append((name, dict(norm=self._row(out_norm, a._norms, 1), rec="packed" if rec is a._rec64 else "separate" if rec is a._rec else "?",
                                    next=self._slice(next_idx), **more)))
        flat_grad.zero_()
        out_norm.zero_()
        return out_norm

    def mlp_ppo_apply(self, flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm,
                      grad_scale=1.0, rec=None, next_idx=None):
        return self._apply("mlp_ppo_apply", flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm,
                           rec, next_idx, grad_scale=grad_scale)

    def mlp_ppo_apply_parts(self, flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps, out_norm,
                            sq_part, rec=None, next_idx=None):
        return self._apply("mlp_ppo_apply_parts", flat_param, flat_grad, exp_avg, exp_avg_sq, layout, lr_dev, step_dev, max_norm, betas, eps,
                           out_norm, rec, next_idx, parts=sq_part is self._agent[0]._p2p.sq_part)

    def clip_adam_(self, flat_param, flat_grad, exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, clip_n=None, betas=(0.9, 0.999), eps=1e-5,
                   out_norm=None):
        self._bucket(flat_param, flat_grad)
        self._adam(exp_avg, exp_avg_sq, lr_dev, step_dev, max_norm, betas, eps)
        self.log.append(("clip_adam_", dict(norm=self._row(out_norm, self._agent[0]._norms, 1), clip_n=clip_n)))
        flat_grad.zero_()
        out_norm.zero_()
        return out_norm

    # ---- the per-op route: the oracle's functions, recorded
    def gather(self, idx, srcs, outs=None):
        a = self._agent[0]
        assert len(srcs) == 3 and srcs[2] is a._rec and srcs[0].data_ptr() == a.buffer.states.data_ptr()
        self.log.append(("gather", dict(idx=self._slice(idx))))
        return oracle_ops.gather(idx, srcs, outs)

    def ppo_loss_packed(self, newlogp, newv, entropy, rec, clip, ent_coef, vf_coef, norm_adv=True, vloss_mode=1, out_scalars=None):
        assert (clip, ent_coef, vf_coef, norm_adv, vloss_mode) == (0.2, 0.01, 0.5, True, self.VLOSS_CLIPPED)
        self.log.append(("ppo_loss_packed", dict(scalars=self._row(out_scalars, self._agent[0]._scalars, self.N_SCALARS))))
        return oracle_ops.ppo_loss_packed(newlogp, newv, entropy, rec, clip, ent_coef, vf_coef, norm_adv, vloss_mode, out_scalars)

    def grad_norm_clip_(self, flat_grads, max_norm, out_norm=None):
        assert flat_grads is self._agent[0].bucket.flat_grad and max_norm == 0.5
        self.log.append(("grad_norm_clip_", dict(norm=self._row(out_norm, self._agent[0]._norms, 1))))
        return oracle_ops.grad_norm_clip_(flat_grads, max_norm, out_norm)


class _P2P:
    def __init__(self, rec, n):
        self.rec, self.n, self.sq_part = rec, n, torch.zeros(4, dtype=torch.float64)

    def allreduce_mean_(self, flat, n, step_dev, timeout_s=10.0):
        a = self.rec._agent[0]
        assert flat is a.bucket.flat_grad and n == self.n and step_dev is a._adam_t and timeout_s == a._p2p_timeout
        self.rec.log.append(("p2p.allreduce_mean_", {}))
        flat.fill_(3.0)
        return flat

    def parts(self, n):
        assert n == self.n
        return self.sq_part


def _agent(monkeypatch, route, rec64):
    ref = []
    ops = Recorder(ref)
    a = ppo(_params(), ops=ops)
    ref.append(a)
    assert (a.batch_size, a.minibatch_size, a._mlp, a._mlp_layered, a._fused_adam, a._dp) == (B, M, None, None, False, False)
    torch.manual_seed(3)
    a._test_perms = torch.stack([torch.randperm(B) for _ in range(E)]).to(torch.int32)
    a._rec = torch.randn(B, 4)
    a._rec[:, 0] = a.buffer.log_probs.reshape(-1)
    a._rec64 = torch.zeros(B, 16) if rec64 else None
    lay = H.mlp_layout(a.policy, a.bucket)
    assert lay is not None and not lay["wide"] and lay["n_params"] == a.bucket.numel
    if route != "autograd":
        a._fused_adam = True
        a._adam_m, a._adam_v = torch.zeros_like(a.bucket.flat_param), torch.zeros_like(a.bucket.flat_param)
        a._adam_t, a._lr_tensor = torch.zeros(1), torch.tensor(2.5e-4)
    if route in ("chained", "halves_allreduce", "halves_p2p", "fused"):
        a._mlp, a._bucket_is_policy = lay, True
    if route == "fused":
        a._bucket_is_policy = False          # e.g. a wide policy or a shared bucket: no chained tail, K7 + K6b
    if route == "layered":
        a._mlp_layered = dict(lay, layered=True)
    if route in ("halves_allreduce", "halves_p2p"):
        a._dp, a.world = True, WORLD
    if route == "halves_p2p":
        a._p2p = _P2P(ops, lay["n_params"])

    def sum_(flat, world=None, force=False):
        assert flat is a.bucket.flat_grad
        ops.log.append(("dist.allreduce_sum_", dict(world=world, force=force)))
        return flat.mul_(world)

    def mean_(flat, world=None, force=False):
        assert flat is a.bucket.flat_grad
        ops.log.append(("dist.allreduce_mean_", dict(world=world, force=force)))
        return flat if route == "autograd" else flat.fill_(5.0)
    monkeypatch.setattr(D, "allreduce_sum_", sum_)
    monkeypatch.setattr(D, "allreduce_mean_", mean_)
    a.first_grad_probe = []
    return a, ops


def _run(a):
    ret, adv = torch.randn(T, N), torch.randn(T, N)
    assert a._update_body(ret, adv, a._test_perms, True) == len(STEPS)


def _sl(s):
    return None if s is None else (s[0], s[1], M)


@pytest.mark.parametrize("rec64", [True, False])
def test_chained_route(monkeypatch, rec64):
    a, ops = _agent(monkeypatch, "chained", rec64)
    _run(a)
    pair = "packed" if rec64 else "separate"
    assert ops.log == [("mlp_ppo_minibatch", dict(idx=_sl(s), pair=pair, scalars=k, layout="fused", next=_sl(NEXT[k]), chained=k > 0, norm=k))
                       for k, s in enumerate(STEPS)]
    assert a.first_grad_probe == []          # the chained call leaves no gradient between its launches to copy


def test_two_halves_around_the_allreduce(monkeypatch):
    a, ops = _agent(monkeypatch, "halves_allreduce", True)
    _run(a)
    want = []
    for k, s in enumerate(STEPS):
        want += [("mlp_ppo_grad", dict(idx=_sl(s), pair="packed", scalars=k, layout="fused", chained=k > 0)),
                 ("dist.allreduce_sum_", dict(world=WORLD, force=True)),
                 ("mlp_ppo_apply", dict(norm=k, rec="packed", next=_sl(NEXT[k]), grad_scale=1.0 / WORLD))]
    assert ops.log == want
    # copied behind the SUM all-reduce (6 x world), before the apply (which zeroes), divided by the world
    assert len(a.first_grad_probe) == 1 and bool((a.first_grad_probe[0] == 6.0).all())
    assert a.first_grad_probe[0].data_ptr() != a.bucket.flat_grad.data_ptr()


def test_two_halves_around_the_p2p_exchange(monkeypatch):
    a, ops = _agent(monkeypatch, "halves_p2p", False)
    _run(a)
    want = []
    for k, s in enumerate(STEPS):
        want += [("mlp_ppo_grad", dict(idx=_sl(s), pair="separate", scalars=k, layout="fused", chained=k > 0)),
                 ("p2p.allreduce_mean_", {}),
                 ("mlp_ppo_apply_parts", dict(norm=k, rec="separate", next=_sl(NEXT[k]), parts=True))]
    assert ops.log == want
    assert len(a.first_grad_probe) == 1 and bool((a.first_grad_probe[0] == 3.0).all())       # the exchange's mean, undivided


@pytest.mark.parametrize("route,fn", [("fused", "mlp_ppo_step"), ("layered", "mlp_layered_step")])
@pytest.mark.parametrize("rec64", [True, False])
def test_step_then_clip_and_adam(monkeypatch, route, fn, rec64):
    a, ops = _agent(monkeypatch, route, rec64)
    _run(a)
    want = []
    for k, s in enumerate(STEPS):
        want += [(fn, dict(idx=_sl(s), pair="packed" if rec64 else "separate", scalars=k, layout=route)),
                 ("dist.allreduce_mean_", dict(world=1, force=False)),
                 ("clip_adam_", dict(norm=k, clip_n=None))]
    assert ops.log == want
    assert len(a.first_grad_probe) == 1 and bool((a.first_grad_probe[0] == 5.0).all())       # behind the mean, undivided


def test_autograd_route(monkeypatch):
    a, ops = _agent(monkeypatch, "autograd", True)
    before = a.bucket.flat_param.clone()
    _run(a)
    want = []
    for k, s in enumerate(STEPS):
        want += [("gather", dict(idx=_sl(s))), ("ppo_loss_packed", dict(scalars=k)), ("dist.allreduce_mean_", dict(world=1, force=False)),
                 ("grad_norm_clip_", dict(norm=k))]
    assert ops.log == want
    assert a.first_grad_probe == [] and not torch.equal(before, a.bucket.flat_param)


def test_probe_mlp_step_uses_the_bodys_pair_and_value_mode(monkeypatch):
    for rec64 in (True, False):
        a, ops = _agent(monkeypatch, "fused", rec64)
        a._last_perms = a._test_perms
        a.probe_mlp_step(events=None)
        (name, e), = ops.log
        assert name == "mlp_ppo_step" and e["idx"] == (0, 0, M) and e["pair"] == ("packed" if rec64 else "separate") and e["scalars"] is None
