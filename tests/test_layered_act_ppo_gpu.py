"""GPU: the layered rollout step inside the trainer (``AURPPO_LAYERED_ACT=1``): the switch, one ``_rollout_steps`` against
``policy.evaluate`` on what it left in the buffer, the captured rollout against the eager one (the construction and tolerances of
tests/test_ppo_gpu.py::test_captured_rollout_matches_eager_rollout at hidden 256, both layered switches on), and a short ``train()``
with a Categorical head."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _hp(**kw):
    hp = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=8, gae=True, total_timesteps=8 * 64 * 5, anneal_lr=True,
              gae_lambda=0.95, num_update_epochs=2, num_envs=64, num_minibatches=2, entropy_coeff=0.0, value_coeff=0.5,
              clip_coeff=0.2, clip_vloss=True, max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False,
              hidden_dim=256, continuous=True, learning_rate=3e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99,
              track=False, log=False, save=False, obs_dim=16, act_dim=3)
    hp.update(kw)
    return hp


def _agent(hp):
    from aur_ppo_amd.ppo import ppo
    assert torch.cuda.is_available()
    return ppo(hp)


def test_layered_act_env_switch(monkeypatch):
    """``AURPPO_LAYERED_ACT=1`` gives the agent an act layout, ``=0`` and an unset variable do not, and ``rewards_to_go`` then calls
    ``policy.evaluate``; the fused kernels' shapes never get it; ``AURPPO_LAYERED_STEP`` neither gives nor takes it."""
    from aur_ppo_amd import ppo as P
    assert P.LAYERED_ACT_DEFAULT == "0"
    monkeypatch.delenv("AURPPO_LAYERED_STEP", raising=False)
    for setting in ("0", None):
        if setting is None:
            monkeypatch.delenv("AURPPO_LAYERED_ACT", raising=False)
        else:
            monkeypatch.setenv("AURPPO_LAYERED_ACT", setting)
        a = _agent(_hp())
        assert a._mlp is None and a._mlp_layered_act is None and a._mlp_layered is None
        calls = []
        evaluate = a.policy.evaluate
        monkeypatch.setattr(a.policy, "evaluate", lambda *args, **kw: calls.append(1) or evaluate(*args, **kw))
        obs = torch.as_tensor(a.envs.reset(seed=list(range(a.num_envs)))[0], dtype=torch.float32).to(a.device)
        a.rewards_to_go(0, obs, 0, None)
        assert calls == [1]
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    a = _agent(_hp())
    assert a._mlp_layered is not None and a._mlp_layered_act is None
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    a = _agent(_hp())
    assert a._mlp is None and a._mlp_layered is not None and a._mlp_layered_act is not None and a._mlp_layered_act["hidden"] == 256
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "0")
    a = _agent(_hp())
    assert a._mlp is None and a._mlp_layered is None and a._mlp_layered_act is not None
    b = _agent(_hp(hidden_dim=128))
    assert b._mlp is not None and b._mlp_layered_act is None
    assert _agent(_hp(fused_mlp=False))._mlp_layered_act is None


def test_one_rollout_matches_evaluate_and_prepares_once(monkeypatch):
    """T 8, N 64, 2 x 256, D 16, A 3: what the T steps left in the buffer against ``policy.evaluate`` of the stored states and
    actions (tolerances of test_wide_act_kernel_matches_torch_formulas); T calls of ``mlp_layered_act``, one of
    ``mlp_layered_prepare``, none of ``policy.evaluate``."""
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    monkeypatch.delenv("AURPPO_LAYERED_STEP", raising=False)
    torch.manual_seed(3)
    a = _agent(_hp())
    ops = a.ops
    calls = {"act": 0, "prepare": 0, "wops": []}

    def act(*args, **kw):
        calls["act"] += 1
        calls["wops"].append(kw.get("wop"))
        return ops.mlp_layered_act(*args, **kw)

    def prepare(*args, **kw):
        calls["prepare"] += 1
        return ops.mlp_layered_prepare(*args, **kw)
    a.ops = types.SimpleNamespace(**{k: getattr(ops, k) for k in dir(ops) if not k.startswith("__")})
    a.ops.mlp_layered_act, a.ops.mlp_layered_prepare = act, prepare
    monkeypatch.setattr(a.policy, "evaluate", lambda *args, **kw: pytest.fail("the torch modules ran"))
    a.seed_all(1)
    obs = torch.as_tensor(a.envs.reset(seed=list(range(a.num_envs)))[0], dtype=torch.float32).to(a.device)
    a.buffer.values.fill_(float("nan"))
    a.buffer.log_probs.fill_(float("nan"))
    a.buffer.actions.fill_(float("nan"))
    a._rollout_steps(obs, torch.zeros(a.num_envs, device=a.device), 0, None)
    torch.cuda.synchronize()
    T = a.num_steps
    assert calls["act"] == T and calls["prepare"] == 1
    assert all(w is not None and w.data_ptr() == calls["wops"][0].data_ptr() for w in calls["wops"])
    assert a._act_wop is None and a._rollout_noise is None
    monkeypatch.undo()
    b = a.buffer
    with torch.no_grad():
        _, lp_ref, _, v_ref = a.policy.evaluate(b.states.view(T * 64, 16), b.actions.view(T * 64, 3))
    assert bool(torch.isfinite(b.actions).all()) and float(b.actions.std()) > 0.1
    np.testing.assert_allclose(b.values.view(-1).cpu().numpy(), v_ref.view(-1).cpu().numpy(), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(b.log_probs.view(-1).cpu().numpy(), lp_ref.view(-1).cpu().numpy(), rtol=2e-5, atol=2e-5)
    # the bootstrap: value-only mode, prepared for itself
    ret, adv = a.advantages(obs, torch.zeros(a.num_envs, device=a.device))
    assert calls["act"] == T + 1 and calls["wops"][-1] is None and bool(torch.isfinite(ret).all()) and bool(torch.isfinite(adv).all())


def test_captured_layered_rollout_matches_eager_rollout(monkeypatch):
    """train() on the device-resident synthetic env with a 2 x 256 policy and both layered switches on: rollouts replayed from a
    hipGraph (the prepare launch inside it, so a replay reads the updated parameters) leave the same policy as rollouts run step by
    step."""
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")

    def run(graph):
        torch.manual_seed(7)
        agent = _agent(_hp(hip_graph=graph))
        assert agent._mlp is None and agent._mlp_layered is not None and agent._mlp_layered_act is not None
        agent.train()
        torch.cuda.synchronize()
        return agent, agent.bucket.flat_param.clone(), agent.buffer.states.clone(), agent.buffer.actions.clone()

    a_g, p_g, s_g, act_g = run(True)
    a_e, p_e, s_e, act_e = run(False)
    assert a_g._ro_state == 2 and a_g._ro_graph is not None and a_e._ro_graph is None
    assert torch.equal(s_g, s_e)                       # the env's generator advanced identically
    torch.testing.assert_close(act_g, act_e, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(p_g, p_e, rtol=1e-4, atol=1e-6)


def test_train_with_a_categorical_layered_policy_stays_finite(monkeypatch):
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    torch.manual_seed(11)
    agent = _agent(_hp(hidden_dim=160, num_layers=3, continuous=False, act_dim=5, total_timesteps=8 * 64 * 3, hip_graph=False))
    assert agent._mlp_layered_act is not None and agent._mlp_layered_act["continuous"] is False
    agent.train()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(agent.bucket.flat_param).all()) and bool(torch.isfinite(agent._scalars).all())
    assert float(agent._scalars[:, 3].abs().max()) > 0          # the updates ran: an entropy was written
    assert bool(torch.isfinite(agent.buffer.log_probs).all()) and bool((agent.buffer.actions >= 0).all()) and bool((agent.buffer.actions < 5).all())
