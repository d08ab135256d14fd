"""GPU: the device Pendulum (K17) against the host class and the Philox restatement, and the one-launch rollout (K18) against the T
launches of K8 + K17 it replaces -- bit for bit, through ``hip_ops`` and through ``ppo._rollout`` on both routes.

The host class draws its resets from numpy's ``RandomState``, the device from Philox; ``_host_env`` below is the host class with its
draw replaced by the restatement's (tests/pendulum_ref.py), so that every quantity behind an auto-reset can be compared too.

Measured on an MI355X: the worst |device - numpy| over every fp64 quantity is 8.9e-16 in the one-step test (N = 257) and over the
40-step trajectory (N = 33), against the bound of 1e-12."""
import numpy as np
import pytest
import torch

from tests import pendulum_ref as R

pytestmark = pytest.mark.gpu

HP = dict(gym_id="Pendulum-v1", seed=1.0, num_steps=128, gae=True, total_timesteps=512 * 60, anneal_lr=True, gae_lambda=0.95,
          num_update_epochs=4, num_envs=4, num_minibatches=4, entropy_coeff=0.0, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True,
          max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=64, continuous=True, learning_rate=3e-4,
          exp_name="t", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False, save=False)
F64 = ("th", "thdot", "obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "ret", "ep_ret")
# Every fp64 quantity within 1e-12 absolute of numpy's: a handful of fp64 roundings on terms up to ~20 with a 2-ulp sin / cos gives
# about 1e-14, and the bound is 100 times that (the argument of tests/test_cartpole_gpu.py).
BOUND = 1e-12


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device_env(n, seed=0):
    from aur_ppo_amd.envs import PendulumDeviceVecEnv
    return PendulumDeviceVecEnv(n, "cuda", seed=seed)


def _host_env(n, seed=0, env0=0):
    from aur_ppo_amd.envs import PendulumVecEnv

    class PhiloxHost(PendulumVecEnv):
        """The host class's arithmetic on the device's reset draws: episode e of env i starts from the restatement's (seed, env0 + i, e)."""
        def __init__(self, n):
            self.episode, self._resetting = np.zeros(n, np.int64), False
            super().__init__(n)

        def _reset_one(self, i):
            if not self._resetting:
                self.episode[i] += 1
            self.th[i], self.thdot[i] = R.reset_state(seed, env0 + int(i), int(self.episode[i]))
            self.steps[i] = 0
            self.ep_ret[i] = 0.0

        def reset(self, seed=None):
            self.episode[:] = 0
            self._resetting = True
            out = super().reset()
            self._resetting = False
            return out
    return PhiloxHost(n)


def _sync(dev, host):
    """The device env at the host's state, statistics and episode numbers included."""
    return dev.set_state(**host.get_state(), episode=host.episode)


def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b)))).all())


def _host_finals(info, n):
    lens, rets = np.zeros(n, np.int64), np.zeros(n, np.float64)
    for i, item in enumerate(info.get("final_info", [None] * n)):
        if item is not None:
            lens[i], rets[i] = item["episode"]["l"], item["episode"]["r"]
    return lens, rets


def _step_both(host, dev, actions):
    """One step of both from where they stand, and every comparison of the one-step contract; returns the worst fp64 difference."""
    n = host.num_envs
    obs_h, rew_h, done_h, _, info = host.step(actions.reshape(n, 1))
    dev.begin_rollout(1)
    obs_d, rew_d, done_d, _, _ = dev.step(torch.from_numpy(actions.reshape(n, 1)).cuda())
    hs, ds = host.get_state(), dev.get_state()
    lens, rets = _host_finals(info, n)
    assert np.array_equal(done_d.cpu().numpy() != 0, done_h)
    assert np.array_equal(ds["steps"], hs["steps"]) and np.array_equal(ds["episode"], host.episode)
    assert np.array_equal(dev.ep_len[0].cpu().numpy(), lens)
    got = dev.ep_ret[0].cpu().numpy()
    assert _within_one_ulp(got[done_h], rets[done_h].astype(np.float32)) and not got[~done_h].any()
    worst = max(float(np.abs(ds[k] - hs[k]).max()) for k in F64)
    assert worst <= BOUND, {k: float(np.abs(ds[k] - hs[k]).max()) for k in F64}
    assert _within_one_ulp(obs_d.cpu().numpy(), obs_h) and _within_one_ulp(rew_d.cpu().numpy(), rew_h)
    return worst, done_h


# ---------------------------------------------------------------------------------------------- reset
@pytest.mark.parametrize("seed", [3, (5 << 32) + 17])
@pytest.mark.parametrize("env0", [0, 5])
def test_reset_is_the_restatement_bit_for_bit(seed, env0):
    N = 70
    env = _device_env(N, seed=seed)
    obs, _ = env.reset(seed=list(range(env0, env0 + N)))
    s = env.get_state()
    ref = R.reset_states(seed, env0, N)
    assert np.array_equal(_bits(s["th"]), _bits(ref[:, 0])) and np.array_equal(_bits(s["thdot"]), _bits(ref[:, 1]))
    assert not s["steps"].any() and not s["episode"].any()
    assert np.array_equal(s["obs_count"], np.full(N, 1.0001)) and np.array_equal(s["ret_count"], np.full(N, 1e-4))
    assert not s["ret"].any() and not s["ep_ret"].any() and not s["ret_mean"].any() and (s["ret_var"] == 1).all()
    assert not env.state[:, 14:].any()
    # the first observation and the statistics that took it, against the restatement's scalar arithmetic
    first = [R.first_obs(*ref[i]) for i in range(N)]
    assert _within_one_ulp(obs.cpu().numpy(), np.stack([o for o, _ in first]))
    mean = np.array([[m for m, _, _ in st] for _, st in first])
    var = np.array([[v for _, v, _ in st] for _, st in first])
    assert np.abs(s["obs_mean"] - mean).max() <= BOUND and np.abs(s["obs_var"] - var).max() <= BOUND


# ---------------------------------------------------------------------------------------------- K17 against the host class
def _one_step_inputs():
    """N = 257: th in +-10 (past +-pi: the modulo's fix-up branch runs), thdot in +-8 with four exactly at +-8 and four that clip,
    actions in +-3 with four exactly +-2, steps cycling through 0, 198, 199 (the last truncates), statistics from a host env run
    for 0, 1 and 50 steps."""
    N = 257
    rs = np.random.RandomState(20)
    th, thdot = rs.uniform(-10, 10, N), rs.uniform(-8, 8, N)
    actions = rs.uniform(-3, 3, N).astype(np.float32)
    thdot[0:4] = [8.0, -8.0, 8.0, -8.0]
    clip = [6, 7, 9, 10]                      # (envs that do not truncate in this step: their next state is the stepped one)
    th[clip], thdot[clip], actions[clip] = [np.pi / 2, -np.pi / 2, np.pi / 2 + 2 * np.pi, -np.pi / 2 - 2 * np.pi], [7.9, -7.9, 7.9, -7.9], [3, -3, 2.5, -2.5]
    actions[12:16] = [2.0, -2.0, 2.0, -2.0]
    steps = np.array([0, 198, 199], np.int64)[np.arange(N) % 3]
    src = _host_env(N, seed=11)
    snaps = [src.get_state()]
    for t in range(50):
        src.step(rs.uniform(-2, 2, (N, 1)).astype(np.float32))
        if t in (0, 49):
            snaps.append(src.get_state())
    pick = (np.arange(N) // 3) % 3
    state = {k: np.where((pick == 0).reshape((N,) + (1,) * (snaps[0][k].ndim - 1)), snaps[0][k],
                         np.where((pick == 1).reshape((N,) + (1,) * (snaps[0][k].ndim - 1)), snaps[1][k], snaps[2][k]))
             for k in F64 if k not in ("th", "thdot")}
    state.update(th=th, thdot=thdot, steps=steps)
    return state, actions


def test_one_step_against_the_host_class():
    """Measured worst |device - numpy| over every fp64 quantity of the 257 envs: 8.9e-16."""
    state, actions = _one_step_inputs()
    N = len(actions)
    assert (np.abs(state["th"]) > np.pi).any() and (state["th"] + np.pi < 0).any()           # the fix-up branch of the modulo
    host, dev = _host_env(N, seed=11), _device_env(N, seed=11)
    host.set_state(**state)
    _sync(dev, host)
    worst, done = _step_both(host, dev, actions)
    print(f"worst |device - numpy| over every fp64 quantity of {N} envs: {worst:.3e}")
    assert np.array_equal(done, state["steps"] == 199) and done.any() and not done.all()
    hs = host.get_state()
    keep = ~done
    assert (np.abs(hs["thdot"][keep]) == 8.0).sum() >= 4                                       # some did clip
    # where the episode ended: the restatement's draw for episode 1, bit for bit
    ds, ref = dev.get_state(), R.reset_states(11, 0, N, episodes=np.ones(N))
    assert np.array_equal(_bits(ds["th"][done]), _bits(ref[done, 0])) and np.array_equal(_bits(ds["thdot"][done]), _bits(ref[done, 1]))
    assert np.array_equal(ds["obs_count"], state["obs_count"] + 1 + done)                      # two observations where it ended


def test_a_trajectory_step_by_step():
    """40 steps, N = 33: at every step the device is put at the host's state and stepped once, so errors cannot compound and the
    one-step bound stays the derived one."""
    N, T = 33, 40
    rs = np.random.RandomState(3)
    host, dev = _host_env(N, seed=4), _device_env(N, seed=4)
    host.set_state(steps=160 + np.arange(N, dtype=np.int64))               # truncations spread over the last 34 of the 40 steps
    worst, ended = 0.0, 0
    for t in range(T):
        _sync(dev, host)
        w, done = _step_both(host, dev, rs.uniform(-3, 3, N).astype(np.float32))
        worst, ended = max(worst, w), ended + int(done.sum())
    print(f"worst one-step |device - numpy| over {T} steps of {N} envs: {worst:.3e}")
    assert ended == N


def test_free_running_episodes_end_where_the_host_class_ends_them():
    N, T = 33, 8
    rs = np.random.RandomState(5)
    host, dev = _host_env(N, seed=9), _device_env(N, seed=9)
    host.set_state(steps=np.full(N, 195, np.int64))
    _sync(dev, host)
    dev.begin_rollout(T)
    for t in range(T):
        a = rs.uniform(-3, 3, (N, 1)).astype(np.float32)
        _, _, done_h, _, info = host.step(a)
        _, _, done_d, _, _ = dev.step(torch.from_numpy(a).cuda())
        assert np.array_equal(done_d.cpu().numpy() != 0, done_h) and done_h.all() == (t == 4) and done_h.any() == (t == 4)
        if t == 4:
            lens, rets = _host_finals(info, N)
            assert (lens == 200).all() and np.array_equal(dev.ep_len[t].cpu().numpy(), lens)
            assert _within_one_ulp(dev.ep_ret[t].cpu().numpy(), rets.astype(np.float32))
            ds, ref = dev.get_state(), R.reset_states(9, 0, N, episodes=np.ones(N))
            assert np.array_equal(_bits(ds["th"]), _bits(ref[:, 0])) and np.array_equal(_bits(ds["thdot"]), _bits(ref[:, 1]))
            assert (ds["episode"] == 1).all() and not ds["steps"].any()
    assert not dev.ep_len[:4].any() and not dev.ep_len[5:].any() and not dev.ep_ret[:4].any()
    assert np.array_equal(dev.get_state()["steps"], np.full(N, 3))


# ---------------------------------------------------------------------------------------------- K18 against T x (K8, K17)
def _policy(seed=0, D=3, A=(1,), hidden=64, continuous=True):
    from aur_ppo_amd import hip_ops as Hops
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(D, A, hidden, 2, 0.0, continuous).cuda()
    bucket = FlatBucket(pol.parameters())
    return pol, bucket, Hops.mlp_layout(pol, bucket)


def _start(env, T):
    """From the env's own reset: every third env 5 steps short of the truncation (1 step where T < 5), every third entering as done."""
    N = env.num_envs
    steps = np.zeros(N, np.int64)
    steps[1::3] = 195 if T >= 5 else 199
    obs = env.set_state(steps=steps)
    return obs.contiguous(), torch.from_numpy((np.arange(N) % 3 == 0).astype(np.float32)).cuda()


def _buffers(T, N):
    z = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device="cuda")       # poisoned: every element must be written
    return dict(states=z(T, N, 3), terminals=z(T, N), actions=z(T, N, 1), log_probs=z(T, N), values=z(T, N), rewards=z(T, N),
                ep_len=z(T, N, dt=torch.int32), ep_ret=z(T, N))


def _same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if x.dtype.is_floating_point:       # raw bits: -0.0 is not 0.0 here, and a NaN equals itself
            x, y = x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32), y.contiguous().view(
                torch.int64 if y.dtype == torch.float64 else torch.int32)
        assert torch.equal(x, y), f"{what}: {k} differs at {int((x != y).sum())} places"


@pytest.mark.parametrize("N,T", [(1, 1), (33, 5), (70, 40)])
def test_one_launch_equals_T_steps_bit_for_bit(N, T):
    from aur_ppo_amd import hip_ops as Hops
    _, bucket, lay = _policy()
    assert Hops.pendulum_rollout_ok(lay)
    noise = torch.randn((T, N, 1), device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    # route 1: K18
    e1 = _device_env(N, seed=21)
    obs1, done1 = _start(e1, T)
    b1 = _buffers(T, N)
    Hops.pendulum_rollout(e1.native_state(), bucket.flat_param, lay, noise, b1["states"], b1["terminals"], b1["actions"], b1["log_probs"],
                          b1["values"], b1["rewards"], b1["ep_len"], b1["ep_ret"], obs1, done1)
    # route 2: T x (K8, K17)
    e2 = _device_env(N, seed=21)
    obs2, done2 = _start(e2, T)
    b2 = _buffers(T, N)
    e2.begin_rollout(T)
    for t in range(T):
        b2["states"][t] = obs2
        b2["terminals"][t] = done2
        Hops.mlp_act(obs2, noise[t], bucket.flat_param, lay, b2["actions"][t], b2["log_probs"][t], b2["values"][t])
        obs2, rew, done2, _, _ = e2.step(b2["actions"][t])
        b2["rewards"][t] = rew
    b2["ep_len"], b2["ep_ret"] = e2.ep_len, e2.ep_ret
    _same(b1, b2, f"N={N} T={T}")
    _same(dict(next_obs=obs1, next_done=done1, state=e1.state, steps=e1.steps, episode=e1.episode),
          dict(next_obs=obs2, next_done=done2, state=e2.state, steps=e2.steps, episode=e2.episode), f"N={N} T={T} behind the rollout")
    if N > 1:      # the comparison covered what it is meant to: truncations with their auto-resets, torques on both sides of the clip
        lens = b1["ep_len"].cpu().numpy()
        assert (lens == 200).sum() == len(range(1, N, 3)) and e1.episode.sum().item() == len(range(1, N, 3))
        assert (b1["ep_ret"][b1["ep_len"] > 0] < 0).all() and not b1["ep_ret"][b1["ep_len"] == 0].any()
        acts = b1["actions"].abs()
        assert (acts > 2).any() and (acts < 2).any()


def _agent(N, T, **more):
    from aur_ppo_amd.ppo import ppo
    torch.manual_seed(0)
    return ppo(dict(HP, num_envs=N, num_steps=T, total_timesteps=N * T * 4, device_env=True, **more))


def _agent_rollouts(agent, N, T, n_rollouts):
    """``n_rollouts`` rollouts of ``ppo._rollout`` from _start's states; a copy of everything each one left."""
    from aur_ppo_amd.envs import PendulumDeviceVecEnv
    assert isinstance(agent.envs, PendulumDeviceVecEnv)
    agent.envs.reset(seed=list(range(N)))
    next_obs, next_done = _start(agent.envs, T)
    out, gs = [], 0
    for k in range(n_rollouts):
        torch.manual_seed(100 + k)          # the rollout's noise: the same draw on every route
        next_obs, next_done, gs = agent._rollout(next_obs, next_done, gs, None)
        b = agent.buffer
        snap = dict(states=b.states, terminals=b.terminals, actions=b.actions, log_probs=b.log_probs, values=b.values, rewards=b.rewards,
                    ep_len=agent.envs.ep_len, ep_ret=agent.envs.ep_ret, next_obs=next_obs, next_done=next_done, env_state=agent.envs.state,
                    env_steps=agent.envs.steps, env_episode=agent.envs.episode, generator=torch.cuda.get_rng_state())
        out.append({k2: v.clone() for k2, v in snap.items()})
    assert gs == n_rollouts * N * T
    return out


@pytest.mark.parametrize("N,T", [(33, 5), (70, 40)])
def test_ppo_rollout_routes_agree(N, T, monkeypatch):
    """ppo._rollout on the one-launch route, and with AURPPO_ROLLOUT_KERNEL=0 on the per-step route eagerly, at capture and at
    replay: the same tensors, the same episode statistics, the generator left in the same state."""
    monkeypatch.delenv("AURPPO_ROLLOUT_KERNEL", raising=False)
    a = _agent(N, T)
    assert a._one_launch_rollout()
    ra = _agent_rollouts(a, N, T, 3)
    monkeypatch.setenv("AURPPO_ROLLOUT_KERNEL", "0")
    b = _agent(N, T)
    assert not b._one_launch_rollout()
    rb = _agent_rollouts(b, N, T, 3)
    assert b._ro_state == 2 and b._ro_graph is not None       # eager, capture, replay
    for k, (x, y) in enumerate(zip(ra, rb)):
        _same({n: v for n, v in x.items() if n != "generator" or k == 0}, {n: v for n, v in y.items() if n != "generator" or k == 0},
              f"rollout {k}")          # (a captured rollout advances the generator through the graph's own registered state)
    assert len(a.total_returns) > 0 and all(r < 0 for r in a.total_returns) and set(a.total_episode_lengths) == {200}
    assert (a.total_returns, a.total_episode_lengths, a.x_indices) == (b.total_returns, b.total_episode_lengths, b.x_indices)
    c = _agent(N, T, hip_graph=False)                          # ... and with no graph at all
    rc = _agent_rollouts(c, N, T, 2)
    assert c._ro_graph is None
    for k, (x, y) in enumerate(zip(ra, rc)):
        _same(x, y, f"eager rollout {k}")


# ---------------------------------------------------------------------------------------------- refusals
SHAPES = {"categorical": dict(A=2, continuous=False), "two_actions": dict(A=(2,)), "four_floats": dict(D=4), "wide": dict(hidden=128)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_other_policy_shapes_are_refused(shape, monkeypatch):
    from aur_ppo_amd import hip_ops as Hops
    _, bucket, lay = _policy(**SHAPES[shape])
    assert lay is not None and not Hops.pendulum_rollout_ok(lay)
    N, T = 5, 3
    env = _device_env(N)
    before = [t.clone() for t in (env.state, env.steps, env.episode)]
    b = _buffers(T, N)
    with pytest.raises(RuntimeError, match=r"aurppo_pendulum_rollout_f32 failed \(rc=-2\)"):
        Hops.pendulum_rollout(env.native_state(), bucket.flat_param, lay, torch.randn((T, N, 1), device="cuda"), b["states"], b["terminals"],
                              b["actions"], b["log_probs"], b["values"], b["rewards"], b["ep_len"], b["ep_ret"],
                              torch.zeros((N, 3), device="cuda"), torch.zeros(N, device="cuda"))
    assert all(torch.equal(x, y) for x, y in zip(before, (env.state, env.steps, env.episode))) and (b["states"] == -7).all()
    # ... and ppo keeps such a policy on the per-step route
    monkeypatch.delenv("AURPPO_ROLLOUT_KERNEL", raising=False)
    agent = _agent(N, T)
    assert agent._one_launch_rollout()
    agent._mlp = lay
    assert not agent._one_launch_rollout()


def test_ppo_steps_the_device_env_for_a_wide_policy(monkeypatch):
    """A policy K18 is not built for (2 x 128: K8w) steps the device env through the captured rollout: eagerly, at capture, at replay."""
    monkeypatch.delenv("AURPPO_ROLLOUT_KERNEL", raising=False)
    N, T = 33, 5
    agent = _agent(N, T, hidden_dim=128)
    assert agent._mlp is not None and agent._mlp["wide"] and not agent._one_launch_rollout()
    obs = agent.envs.reset(seed=list(range(N)))[0]
    first = obs.clone()
    next_obs, next_done, gs = obs, torch.zeros(N, device="cuda"), 0
    for k in range(3):
        next_obs, next_done, gs = agent._rollout(next_obs, next_done, gs, None)
        if k == 0:
            assert torch.equal(agent.buffer.states[0], first)
    assert gs == 3 * N * T and agent._ro_state == 2
    s = agent.envs.get_state()
    assert (s["steps"] == 3 * T).all() and not s["episode"].any() and np.abs(s["obs_count"] - (1e-4 + 1 + 3 * T)).max() < 1e-9
    assert np.abs(s["ret_count"] - (1e-4 + 3 * T)).max() < 1e-9
    r = agent.buffer.rewards
    assert torch.isfinite(r).all() and (r <= 0).all() and (r >= -10).all() and (r < 0).any()
    assert torch.isfinite(agent.buffer.actions).all() and not agent.total_returns
