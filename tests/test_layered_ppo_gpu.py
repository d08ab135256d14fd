"""GPU: one whole ``ppo.update`` with an MLP policy wider than the fused kernels, through the layered step
(hip_ops.mlp_layered_step, ``AURPPO_LAYERED_STEP=1``) and through the per-op route it replaces (``AURPPO_LAYERED_STEP=0``: K3
gather, torch evaluate, K4 + K5, autograd), both against ``oracle.reference_update`` -- the construction and the tolerances of
tests/test_mlp_wide.py::test_full_update_with_a_wide_policy_matches_oracle (T 32, N 256, A 6, 4 epochs x 4 minibatches)."""
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


def _update(hidden, layers, Dm, launch, layered, monkeypatch):
    """One update of a freshly seeded agent; returns the agent's results next to the oracle's as the worst ratio of error to tolerance
    per class (<= 1: within the tolerance)."""
    import bench
    from aur_ppo_amd.ppo import ppo
    from oracle import ppo_oracle as O
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1" if layered else "0")
    hp = _hp(Dm, hidden_dim=hidden, num_layers=layers, hip_graph=(launch == "hipGraph"))
    torch.manual_seed(1)
    agent = ppo(hp)
    assert agent._mlp is None and (agent._mlp_layered is not None) == layered
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
    if key not in _ORACLE:          # the oracle's update of this shape, once (both arms start from the same seeded weights)
        net = O.make_actor_critic(Dm, (A,), hidden, layers, True)
        net.load_state_dict(init_sd)
        opt = torch.optim.Adam(net.parameters(), lr=hp["learning_rate"], eps=1e-5)
        buf = {k: data[k] for k in ("states", "actions", "log_probs", "rewards", "terminals", "values")}
        res = O.reference_update(net, opt, buf, data["next_obs"], data["next_done"], hp, np.random.RandomState(1))
        _ORACLE[key] = (init_sd, res, {k: v.clone() for k, v in net.state_dict().items()})
    sd0, res, sd_ref = _ORACLE[key]
    for k in init_sd:
        assert torch.equal(init_sd[k], sd0[k]), "both arms start from the same weights"
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
@pytest.mark.parametrize("hidden,layers,Dm", [(256, 2, 64), (160, 3, 144)])
def test_full_update_with_a_layered_policy_matches_oracle(hidden, layers, Dm, launch, monkeypatch):
    """Permutations bit-exact, advantages 1e-5, every step's scalars rtol 1e-4 + 1e-5, clip fraction within 1.5 / M, final weights
    rtol 1e-4 + 2e-5 -- for the layered step, with the per-op route measured against the same oracle beside it."""
    per_op = _update(hidden, layers, Dm, launch, False, monkeypatch)
    layered = _update(hidden, layers, Dm, launch, True, monkeypatch)
    print(f"\n{layers} x {hidden} / D {Dm}, {launch}: error / tolerance -- per-op route {per_op}, layered step {layered}")
    for k, v in layered.items():
        assert v <= 1.0, (k, v, per_op[k])


def test_layered_step_env_switch(monkeypatch):
    """``AURPPO_LAYERED_STEP=1`` takes the layered step, ``=0`` and (the step being opt-in) an unset variable keep the per-op route;
    the fused kernels' shapes never take it."""
    from aur_ppo_amd.ppo import ppo
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "0")
    assert ppo(_hp(64, hidden_dim=256))._mlp_layered is None
    monkeypatch.delenv("AURPPO_LAYERED_STEP")
    assert ppo(_hp(64, hidden_dim=256))._mlp_layered is None
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    a = ppo(_hp(64, hidden_dim=256))
    assert a._mlp is None and a._mlp_layered is not None and a._mlp_layered["hidden"] == 256
    b = ppo(_hp(64, hidden_dim=128))
    assert b._mlp is not None and b._mlp_layered is None
    assert ppo(_hp(64, hidden_dim=256, fused_mlp=False))._mlp_layered is None
