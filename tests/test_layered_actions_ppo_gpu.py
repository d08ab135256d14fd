"""GPU: the trainer with an MLP policy of 17 actions (Humanoid's shape: two layers of 256 over 376 state floats), which ``ppo.__init__``
hands to the layered routes once ``AURPPO_LAYERED_WIDE_ACTIONS=1`` stands beside ``AURPPO_LAYERED_STEP`` / ``AURPPO_LAYERED_ACT``
(``mlp_layered_layout(..., any_state=True, wide_actions=True)``).  Modelled on tests/test_layered_hidden_ppo_gpu.py; the hyper-parameters
and tolerances are those of tests/test_layered_ragged_ppo_gpu.py, imported.

T1  a two-update ``train()`` on the synthetic env with the three switches on: every update takes ``layered_minibatch`` (17 actions have no
    per-product route, whatever ``AURPPO_LAYERED_NATIVE`` says), the rollout takes the layered act from copies prepared once per rollout
    with the torch modules not running, and the first minibatch of an update's first epoch has old_kl == 0 exactly: K14's log-prob is K13's.
T2  one whole ``ppo.update`` against ``oracle.reference_update`` on the same tensors: permutations bit-exact, advantages 1e-5, scalars
    rtol 1e-4 + 1e-5, clip fraction within 1.5 / M, final weights rtol 1e-4 + 2e-5.
T3  with ``AURPPO_LAYERED_WIDE_ACTIONS`` unset the same agent has no layered layout and takes the ``autograd`` route."""
import types

import numpy as np
import pytest
import torch

from tests import test_layered_hidden_ppo_gpu as LHP

pytestmark = pytest.mark.gpu

LRP = LHP.LRP
T, N = LRP.T, LRP.N
HIDDEN, LAYERS, DM, A = 256, 2, 376, 17


def _switches(monkeypatch, wide_actions=True):
    LHP._switches(monkeypatch, any_hidden=False)
    if wide_actions:
        monkeypatch.setenv("AURPPO_LAYERED_WIDE_ACTIONS", "1")
    else:
        monkeypatch.delenv("AURPPO_LAYERED_WIDE_ACTIONS", raising=False)


def test_two_updates_through_the_trainer_at_17_actions(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    _switches(monkeypatch)
    torch.manual_seed(3)
    a = LRP._agent(LRP._hp_rollout(hidden_dim=HIDDEN, num_layers=LAYERS, obs_dim=DM, act_dim=A, total_timesteps=8 * 64 * 2, hip_graph=False))
    assert a._mlp is None and a._layered_native is False
    for lay in (a._mlp_layered, a._mlp_layered_act):
        assert lay is not None and lay["wide_actions"] is True and (lay["hidden"], lay["D"], lay["A"]) == (HIDDEN, DM, A)
    assert a._update_route(True) == "layered_minibatch"
    ops = a.ops
    calls = {"act": 0, "prepare": 0, "minibatch": 0}

    def count(name, fn):
        def wrapped(*args, **kw):
            calls[name] += 1
            return fn(*args, **kw)
        return wrapped
    a.ops = types.SimpleNamespace(**{k: getattr(ops, k) for k in dir(ops) if not k.startswith("__")})
    a.ops.mlp_layered_act = count("act", ops.mlp_layered_act)
    a.ops.mlp_layered_prepare = count("prepare", ops.mlp_layered_prepare)
    a.ops.mlp_layered_minibatch = count("minibatch", ops.mlp_layered_minibatch)
    a.ops.mlp_layered_step = lambda *args, **kw: pytest.fail("the per-product route ran")
    monkeypatch.setattr(a.policy, "evaluate", lambda *args, **kw: pytest.fail("the torch modules ran"))
    p0 = a.bucket.flat_param.clone()
    a.train()
    torch.cuda.synchronize()
    steps = a.num_update_epochs * ((a.batch_size + a.minibatch_size - 1) // a.minibatch_size)
    assert steps == 4 and calls["minibatch"] == 2 * steps                          # two updates, every minibatch in one native call
    assert calls["prepare"] == 2 and calls["act"] >= 2 * (a.num_steps + 1)         # per rollout: one prepare, T steps and the bootstrap
    assert a._rec64 is None                                                        # 17 action floats do not fit a packed record
    assert bool(torch.isfinite(a.bucket.flat_param).all()) and not torch.equal(a.bucket.flat_param, p0)
    sc = a._scalars[:steps].cpu()
    assert bool(torch.isfinite(sc).all())
    print(f"\nupdate 2, epoch 1, minibatch 1: old_kl {float(sc[0, H.S_OLD_KL])!r}, kl {float(sc[0, H.S_KL])!r}; minibatch 2: old_kl {float(sc[1, H.S_OLD_KL])!r}")
    assert float(sc[0, H.S_OLD_KL]) == 0.0 and float(sc[0, H.S_KL]) == 0.0 and float(sc[0, H.S_CLIPFRAC]) == 0.0
    assert float(sc[1, H.S_OLD_KL]) != 0.0          # (the parameters have moved by the second minibatch)


def _update(monkeypatch):
    """tests/test_layered_hidden_ppo_gpu.py::_update at Humanoid's shape with the three switches; returns error / tolerance per class."""
    import bench
    from aur_ppo_amd.ppo import ppo
    from oracle import ppo_oracle as O
    _switches(monkeypatch)
    hp = LRP._hp(DM, hidden_dim=HIDDEN, num_layers=LAYERS, act_dim=A, hip_graph=False)
    torch.manual_seed(1)
    agent = ppo(hp)
    assert agent._mlp is None and agent._mlp_layered is not None and agent._mlp_layered["wide_actions"] is True
    assert agent._update_route(True) == "layered_minibatch"
    data = bench.synth_buffers(T, N, DM, A, 1234)
    init_sd = {k: v.detach().cpu().clone() for k, v in agent.policy.state_dict().items()}
    for k in ("states", "actions", "values", "rewards", "terminals"):
        getattr(agent.buffer, k).copy_(data[k])
    with torch.no_grad():
        _, lp, _, _ = agent.policy.evaluate(agent.buffer.states.view(-1, DM), agent.buffer.actions.view(-1, A))
        agent.buffer.log_probs.copy_(lp.view(T, N))
    data["log_probs"] = agent.buffer.log_probs.cpu()
    agent.seed_all(1)
    ret, adv = agent.advantages(data["next_obs"].cuda(), data["next_done"].cuda())
    n = agent.update(ret, adv)
    torch.cuda.synchronize()
    assert n == 16
    net = O.make_actor_critic(DM, (A,), HIDDEN, LAYERS, True)
    net.load_state_dict(init_sd)
    opt = torch.optim.Adam(net.parameters(), lr=hp["learning_rate"], eps=1e-5)
    buf = {k: data[k] for k in ("states", "actions", "log_probs", "rewards", "terminals", "values")}
    res = O.reference_update(net, opt, buf, data["next_obs"], data["next_done"], hp, np.random.RandomState(1))
    sd_ref = net.state_dict()
    perms = agent._last_perms.cpu().numpy()
    for e in range(4):
        assert np.array_equal(perms[e], res["perms"][e]), f"epoch {e} permutation"
    np.testing.assert_allclose(adv.cpu().numpy(), res["advantages"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(ret.cpu().numpy(), res["returns"].numpy(), rtol=0, atol=1e-5)
    got = agent._scalars[:n].cpu().numpy()
    cols = [0, 1, 2, 3, 4, 5, 7, 8]
    r_sc = float((np.abs(got[:, cols] - res["scalars"][:, cols]) / (1e-5 + 1e-4 * np.abs(res["scalars"][:, cols]))).max())
    r_cf = float(np.abs(got[:, 6] - res["scalars"][:, 6]).max() / (1.5 / agent.minibatch_size))
    r_w = max(float(((v.cpu() - sd_ref[k]).abs() / (2e-5 + 1e-4 * sd_ref[k].abs())).max()) for k, v in agent.policy.state_dict().items())
    return dict(scalars=r_sc, clipfrac=r_cf, weights=r_w)


def test_full_update_at_17_actions_matches_oracle(monkeypatch):
    """Permutations bit-exact, advantages 1e-5, every step's scalars rtol 1e-4 + 1e-5, clip fraction within 1.5 / M, final weights
    rtol 1e-4 + 2e-5: the tolerances tests/test_layered_hidden_ppo_gpu.py uses for the layered route."""
    got = _update(monkeypatch)
    print(f"\n{LAYERS} x {HIDDEN} / D {DM} / A {A}: error / tolerance -- layered minibatch {got}")
    for k, v in got.items():
        assert v <= 1.0, (k, v)


def test_without_the_switch_17_actions_keep_the_autograd_route(monkeypatch):
    _switches(monkeypatch, wide_actions=False)
    a = LRP._agent(LRP._hp_rollout(hidden_dim=HIDDEN, num_layers=LAYERS, obs_dim=DM, act_dim=A))
    assert a._mlp is None and a._mlp_layered is None and a._mlp_layered_act is None and a._act_layout() is None
    assert a._update_route(True) == "autograd"
    # 16 actions are what they were, switch or no switch
    b = LRP._agent(LRP._hp_rollout(hidden_dim=HIDDEN, num_layers=LAYERS, obs_dim=DM, act_dim=16))
    assert b._mlp_layered is not None and "wide_actions" not in b._mlp_layered and b._update_route(True) == "layered_step"
