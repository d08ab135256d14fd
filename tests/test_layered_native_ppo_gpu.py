"""GPU: one whole ``ppo.update`` through the native layered routes (``AURPPO_LAYERED_STEP=1 AURPPO_LAYERED_NATIVE=1``:
hip_ops.mlp_layered_minibatch, or hip_ops.mlp_layered_step_native + clip_adam_) against ``oracle.reference_update`` -- the construction
and the tolerances of tests/test_layered_ppo_gpu.py (T 32, N 256, A 6, 4 epochs x 4 minibatches), whose helpers and oracle cache are
imported.  At one layer the native step has no bias gradient of its own, so the final weights and all 16 x 9 scalars equal the same
update with ``AURPPO_LAYERED_NATIVE=0`` bit for bit, on either native route."""
import numpy as np
import pytest
import torch

from tests import test_layered_ppo_gpu as LP

pytestmark = pytest.mark.gpu

T, N, A = LP.T, LP.N, LP.A


def _update(hidden, layers, Dm, launch, native, monkeypatch):
    """tests/test_layered_ppo_gpu.py::_update with the native switch; returns (error / tolerance per class, the agent, its route)."""
    import bench
    from aur_ppo_amd.ppo import ppo
    from oracle import ppo_oracle as O
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    monkeypatch.setenv("AURPPO_LAYERED_NATIVE", "1" if native else "0")
    hp = LP._hp(Dm, hidden_dim=hidden, num_layers=layers, hip_graph=(launch == "hipGraph"))
    torch.manual_seed(1)
    agent = ppo(hp)
    assert agent._mlp is None and agent._mlp_layered is not None and agent._layered_native == native
    route = agent._update_route(True)
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
    if key not in LP._ORACLE:
        net = O.make_actor_critic(Dm, (A,), hidden, layers, True)
        net.load_state_dict(init_sd)
        opt = torch.optim.Adam(net.parameters(), lr=hp["learning_rate"], eps=1e-5)
        buf = {k: data[k] for k in ("states", "actions", "log_probs", "rewards", "terminals", "values")}
        res = O.reference_update(net, opt, buf, data["next_obs"], data["next_done"], hp, np.random.RandomState(1))
        LP._ORACLE[key] = (init_sd, res, {k: v.clone() for k, v in net.state_dict().items()})
    sd0, res, sd_ref = LP._ORACLE[key]
    for k in init_sd:
        assert torch.equal(init_sd[k], sd0[k]), "both arms start from the same weights"
    perms = agent._last_perms.cpu().numpy()
    for e in range(4):
        assert np.array_equal(perms[e], res["perms"][e]), f"epoch {e} permutation"
    got = agent._scalars[:n].cpu().numpy()
    cols = [0, 1, 2, 3, 4, 5, 7, 8]
    r_sc = float((np.abs(got[:, cols] - res["scalars"][:, cols]) / (1e-5 + 1e-4 * np.abs(res["scalars"][:, cols]))).max())
    r_cf = float(np.abs(got[:, 6] - res["scalars"][:, 6]).max() / (1.5 / agent.minibatch_size))
    r_w = max(float(((v.cpu() - sd_ref[k]).abs() / (2e-5 + 1e-4 * sd_ref[k].abs())).max()) for k, v in agent.policy.state_dict().items())
    return dict(scalars=r_sc, clipfrac=r_cf, weights=r_w), agent, route


@pytest.mark.parametrize("launch", ["eager", "hipGraph"])
@pytest.mark.parametrize("hidden,layers,Dm", [(256, 2, 64), (160, 3, 144)])
def test_full_update_on_the_native_layered_route_matches_oracle(hidden, layers, Dm, launch, monkeypatch):
    """Permutations bit-exact, every step's scalars rtol 1e-4 + 1e-5, clip fraction within 1.5 / M, final weights rtol 1e-4 + 2e-5."""
    got, agent, route = _update(hidden, layers, Dm, launch, True, monkeypatch)
    print(f"\n{layers} x {hidden} / D {Dm}, {launch}, route {route}: error / tolerance {got}")
    assert route == "layered_minibatch"         # single process, fused Adam, the bucket holds exactly the policy
    for k, v in got.items():
        assert v <= 1.0, (k, v)


@pytest.mark.parametrize("with_minibatch", [True, False], ids=["layered_minibatch", "layered_native_step"])
def test_one_layer_native_update_equals_the_python_route_bit_for_bit(with_minibatch, monkeypatch):
    from aur_ppo_amd import hip_ops as H
    _r0, python, route0 = _update(256, 1, 64, "eager", False, monkeypatch)
    assert route0 == "layered_step"
    if not with_minibatch:
        monkeypatch.delattr(H, "mlp_layered_minibatch")          # the trainer then steps natively and keeps its own clip + Adam
    _r1, native, route1 = _update(256, 1, 64, "eager", True, monkeypatch)
    assert route1 == ("layered_minibatch" if with_minibatch else "layered_native_step")
    assert torch.equal(native._scalars[:16], python._scalars[:16]) and native._scalars[:16].shape == (16, 9)
    assert torch.equal(native._norms[:16], python._norms[:16])
    for (k, v), w in zip(native.policy.state_dict().items(), python.policy.state_dict().values()):
        assert torch.equal(v, w), k


def test_the_native_switch_is_read_only_where_the_layered_update_is_on(monkeypatch):
    from aur_ppo_amd.ppo import LAYERED_NATIVE_DEFAULT, ppo
    assert LAYERED_NATIVE_DEFAULT == "0"
    monkeypatch.setenv("AURPPO_LAYERED_NATIVE", "1")
    monkeypatch.delenv("AURPPO_LAYERED_STEP", raising=False)
    a = ppo(LP._hp(64, hidden_dim=256))
    assert a._mlp_layered is None and a._layered_native is False and a._update_route(True) == "autograd"
    monkeypatch.setenv("AURPPO_LAYERED_STEP", "1")
    monkeypatch.delenv("AURPPO_LAYERED_NATIVE")
    b = ppo(LP._hp(64, hidden_dim=256))
    assert b._mlp_layered is not None and b._layered_native is False and b._update_route(True) == "layered_step"
