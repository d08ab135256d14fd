"""GPU: the trainer with an MLP policy wider than the fused kernels over a state that is no multiple of 16 floats (HalfCheetah's 17,
Hopper's 11), which ``ppo.__init__`` now hands to the layered routes (``mlp_layered_layout(..., any_state=True)``).

T1  one whole ``ppo.update`` through the layered step (``AURPPO_LAYERED_STEP=1``) against ``oracle.reference_update``: the construction
    and the tolerances of tests/test_layered_ppo_gpu.py, restated (T 32, N 256, A 6, 4 epochs x 4 minibatches), eager and as a hipGraph.
T2  one ``_rollout_steps`` with both switches on against ``policy.evaluate`` on what it left in the buffer, the torch modules not
    running (tests/test_layered_act_ppo_gpu.py::test_one_rollout_matches_evaluate_and_prepares_once, restated at D 17, A 6).
T3  a short captured ``train()`` against the eager one (test_captured_layered_rollout_matches_eager_rollout, restated)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, N, A = 32, 256, 6
_ORACLE = {}


def _hp(Dm, **kw):
    hp = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=T, gae=True, total_timesteps=T * N, anneal_lr=False,
              gae_lambda=0.95, num_update_epochs=4, num_envs=N, num_minibatches=4, entropy_coeff=0.01,
              value_coeff=0.5, clip_coeff=0.2, clip_vloss=True, max_grad_norm=0.5, target_kl=None, norm_adv=True,
              capture_video=False, hidden_dim=64, continuous=True, learning_rate=3e-4, exp_name="t", num_layers=2,
              dropout=0.0, gamma=0.99, track=False, log=False, save=False, obs_dim=Dm, act_dim=A)
    hp.update(kw)
    return hp


def _update(hidden, layers, Dm, launch, monkeypatch):
    """One update of a freshly seeded agent through the layered step; returns the agent's results next to the oracle's as the worst
    ratio of error to tolerance per class (<= 1: within the tolerance)."""
    import bench
    from aur_ppo_amd.ppo import ppo
    from oracle import ppo_oracle as O
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    hp = _hp(Dm, hidden_dim=hidden, num_layers=layers, hip_graph=(launch == "hipGraph"))
    torch.manual_seed(1)
    agent = ppo(hp)
    assert agent._mlp is None and agent._mlp_layered is not None and agent._mlp_layered["D"] == Dm
    data = bench.synth_buffers(T, N, Dm, A, 1234)
    init_sd = {k: v.detach().cpu().clone() for k, v in agent.policy.state_dict().items()}
    for k in ("states", "actions", "values", "rewards", "terminals"):
        getattr(agent.buffer, k).copy_(data[k])
    with torch.no_grad():
        _, lp, _, _ = agent.policy.evaluate(agent.buffer.states.view(-1, Dm), agent.buffer.actions.view(-1, A))
        agent.buffer.log_probs.copy_(lp.view(T, N))
    data["log_probs"] = agent.buffer.log_probs.cpu()
    agent.seed_all(1)
    if launch == "hipGraph":
        agent._graph_state = 1
    ret, adv = agent.advantages(data["next_obs"].cuda(), data["next_done"].cuda())
    n = agent.update(ret, adv)
    torch.cuda.synchronize()
    assert (agent._graph is not None) == (launch == "hipGraph") and n == 16
    key = (hidden, layers, Dm)
    if key not in _ORACLE:          # the oracle's update of this shape, once (both launches start from the same seeded weights)
        net = O.make_actor_critic(Dm, (A,), hidden, layers, True)
        net.load_state_dict(init_sd)
        opt = torch.optim.Adam(net.parameters(), lr=hp["learning_rate"], eps=1e-5)
        buf = {k: data[k] for k in ("states", "actions", "log_probs", "rewards", "terminals", "values")}
        res = O.reference_update(net, opt, buf, data["next_obs"], data["next_done"], hp, np.random.RandomState(1))
        _ORACLE[key] = (init_sd, res, {k: v.clone() for k, v in net.state_dict().items()})
    sd0, res, sd_ref = _ORACLE[key]
    for k in init_sd:
        assert torch.equal(init_sd[k], sd0[k]), "both launches start from the same weights"
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


@pytest.mark.parametrize("launch", ["eager", "hipGraph"])
@pytest.mark.parametrize("hidden,layers,Dm", [(256, 2, 17), (160, 3, 11)])
def test_full_update_with_a_layered_policy_over_a_ragged_state_matches_oracle(hidden, layers, Dm, launch, monkeypatch):
    """Permutations bit-exact, advantages 1e-5, every step's scalars rtol 1e-4 + 1e-5, clip fraction within 1.5 / M, final weights
    rtol 1e-4 + 2e-5."""
    layered = _update(hidden, layers, Dm, launch, monkeypatch)
    print(f"\n{layers} x {hidden} / D {Dm}, {launch}: error / tolerance -- layered step {layered}")
    for k, v in layered.items():
        assert v <= 1.0, (k, v)


# ---------------------------------------------------------------------------------- the rollout
def _hp_rollout(**kw):
    hp = dict(gym_id="Synthetic-v0", seed=1.0, num_steps=8, gae=True, total_timesteps=8 * 64 * 5, anneal_lr=True,
              gae_lambda=0.95, num_update_epochs=2, num_envs=64, num_minibatches=2, entropy_coeff=0.0, value_coeff=0.5,
              clip_coeff=0.2, clip_vloss=True, max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False,
              hidden_dim=256, continuous=True, learning_rate=3e-4, exp_name="t", num_layers=2, dropout=0.0, gamma=0.99,
              track=False, log=False, save=False, obs_dim=17, act_dim=6)
    hp.update(kw)
    return hp


def _agent(hp):
    from aur_ppo_amd.ppo import ppo
    assert torch.cuda.is_available()
    return ppo(hp)


def test_one_rollout_over_a_ragged_state_matches_evaluate(monkeypatch):
    """T 8, N 64, 2 x 256, D 17, A 6, both switches on: what the T steps left in the buffer against ``policy.evaluate`` of the stored
    states and actions; T calls of ``mlp_layered_act``, one of ``mlp_layered_prepare``, none of ``policy.evaluate``."""
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    torch.manual_seed(3)
    a = _agent(_hp_rollout())
    assert a._mlp is None and a._mlp_layered is not None and a._mlp_layered_act is not None and a._mlp_layered_act["D"] == 17
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
    Ts = a.num_steps
    assert calls["act"] == Ts and calls["prepare"] == 1
    assert all(w is not None and w.data_ptr() == calls["wops"][0].data_ptr() for w in calls["wops"])
    assert a._act_wop is None and a._rollout_noise is None
    monkeypatch.undo()
    b = a.buffer
    with torch.no_grad():
        _, lp_ref, _, v_ref = a.policy.evaluate(b.states.view(Ts * 64, 17), b.actions.view(Ts * 64, 6))
    assert bool(torch.isfinite(b.actions).all()) and float(b.actions.std()) > 0.1
    np.testing.assert_allclose(b.values.view(-1).cpu().numpy(), v_ref.view(-1).cpu().numpy(), rtol=2e-5, atol=1e-5)
    np.testing.assert_allclose(b.log_probs.view(-1).cpu().numpy(), lp_ref.view(-1).cpu().numpy(), rtol=2e-5, atol=2e-5)


def test_captured_layered_rollout_over_a_ragged_state_matches_eager_rollout(monkeypatch):
    """train() on the device-resident synthetic env with a 2 x 256 policy over 17 state floats and both layered switches on: rollouts
    replayed from a hipGraph leave the same policy as rollouts run step by step."""
    monkeypatch.setenv("AURPPO_LAYERED_ACT", "1")
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")

    def run(graph):
        torch.manual_seed(7)
        agent = _agent(_hp_rollout(hip_graph=graph))
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
