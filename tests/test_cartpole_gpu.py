"""GPU: the device CartPole (K15) against the host class and the Philox restatement, and the one-launch rollout (K16) against the T
launches of K8 + K15 it replaces -- bit for bit, through ``hip_ops`` and through ``ppo._rollout`` on both routes."""
import numpy as np
import pytest
import torch

from tests import cartpole_ref as R

pytestmark = pytest.mark.gpu

HP = dict(gym_id="CartPole-v1", seed=1.0, num_steps=128, gae=True, total_timesteps=512 * 60, anneal_lr=True, gae_lambda=0.95,
          num_update_epochs=4, num_envs=4, num_minibatches=4, entropy_coeff=0.01, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True,
          max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False, hidden_dim=64, continuous=False, learning_rate=2.5e-4,
          exp_name="t", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False, save=False)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device_env(n, seed=0):
    from aur_ppo_amd.envs import CartPoleDeviceVecEnv
    return CartPoleDeviceVecEnv(n, "cuda", seed=seed)


def _host_env(state, steps):
    from aur_ppo_amd.envs import CartPoleVecEnv
    h = CartPoleVecEnv(len(steps))
    h.state, h.steps, h.ret = state.copy(), steps.astype(np.int64).copy(), steps.astype(np.float64).copy()
    return h


def _host_lengths(info, n):
    out = np.zeros(n, np.int64)
    for i, item in enumerate(info.get("final_info", [None] * n)):
        if item is not None:
            out[i] = item["episode"]["l"]
    return out


@pytest.mark.parametrize("seed", [3, (5 << 32) + 17])
@pytest.mark.parametrize("env0", [0, 5])
def test_reset_is_the_restatement_bit_for_bit(seed, env0):
    N = 70
    env = _device_env(N, seed=seed)
    obs, _ = env.reset(seed=list(range(env0, env0 + N)))
    state, steps, episode = env.get_state()
    ref = R.reset_states(seed, env0, N)
    assert np.array_equal(_bits(state), _bits(ref))
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), ref.astype(np.float32).view(np.uint32))
    assert not steps.any() and not episode.any()


def _one_step_states():
    """N = 257 states: x in +-2.5, theta in +-0.22, velocities in +-3; the first 16 are placed so that the NEXT x (theta) lands 5e-7
    inside or outside each limit; steps cycle through 0, 498, 499 (the last truncates)."""
    from aur_ppo_amd.envs import CartPoleVecEnv as H
    N = 257
    rs = np.random.RandomState(20)
    st = np.stack([rs.uniform(-2.5, 2.5, N), rs.uniform(-3, 3, N), rs.uniform(-0.22, 0.22, N), rs.uniform(-3, 3, N)], 1)
    k = 0
    for lim, pos, vel in ((H.x_lim, 0, 1), (H.theta_lim, 2, 3)):
        for sign in (1.0, -1.0):
            for side in (5e-7, -5e-7):
                for v in (0.7, -1.3):
                    st[k] = [0.1, 0.2, 0.01, -0.3]
                    st[k, vel] = v
                    st[k, pos] = sign * (lim + side) - H.tau * v
                    k += 1
    steps = np.array([0, 498, 499], np.int64)[np.arange(N) % 3]
    actions = rs.randint(0, 2, N).astype(np.float32)
    return st, steps, actions


def test_one_step_against_the_host_class():
    from aur_ppo_amd.envs import CartPoleVecEnv as H
    st, steps, actions = _one_step_states()
    N = len(steps)
    # every draw is at least 1e-9 away from both limits: a last-bit difference cannot decide a done flag
    for col, lim in ((0, H.x_lim), (2, H.theta_lim)):
        assert (np.abs(np.abs(st[:, col]) - lim) >= 1e-9).all()
    host = _host_env(st, steps)
    _, _, done_h, _, info = host.step(actions)
    # ... and so is every NEXT position and angle (host.state holds the reset draw where done, so they are formed here, by the
    # host class's own expressions); the 16 placed ones sit within 1e-6 of a limit, 8 inside and 8 outside
    nxt_x, nxt_th = st[:, 0] + H.tau * st[:, 1], st[:, 2] + H.tau * st[:, 3]
    assert (np.abs(np.abs(nxt_x) - H.x_lim) >= 1e-9).all() and (np.abs(np.abs(nxt_th) - H.theta_lim) >= 1e-9).all()
    near = (np.abs(np.abs(nxt_x) - H.x_lim) < 1e-6) | (np.abs(np.abs(nxt_th) - H.theta_lim) < 1e-6)
    assert near[:16].all() and _outside(nxt_x, nxt_th)[:16].sum() == 8
    assert np.array_equal(done_h, _outside(nxt_x, nxt_th) | (steps == 499))
    assert done_h.any() and not done_h.all()
    env = _device_env(N, seed=11)
    env.set_state(st, steps)
    env.begin_rollout(1)
    obs, reward, done, _, _ = env.step(torch.from_numpy(actions).cuda())
    state_d, steps_d, episode_d = env.get_state()
    done_d = done.cpu().numpy() != 0
    assert np.array_equal(done_d, done_h)
    assert np.array_equal(env.ep_len[0].cpu().numpy(), _host_lengths(info, N))
    assert np.array_equal(steps_d, host.steps)
    assert np.array_equal(episode_d, done_h.astype(np.int32))
    assert (reward.cpu().numpy() == 1.0).all()
    err = np.abs(state_d[~done_h] - host.state[~done_h]).max()
    print(f"worst |device - numpy| over {int((~done_h).sum())} next states: {err:.3e}")
    assert err <= 1e-12
    # where the episode ended: the restatement's draw for episode 1, and the observation is its fp32 rounding
    ref = R.reset_states(11, 0, N, episodes=np.ones(N))
    assert np.array_equal(_bits(state_d[done_h]), _bits(ref[done_h]))
    assert np.array_equal(obs.cpu().numpy().view(np.uint32), state_d.astype(np.float32).view(np.uint32))


def _outside(x, th):
    from aur_ppo_amd.envs import CartPoleVecEnv as H
    return (np.abs(x) > H.x_lim) | (np.abs(th) > H.theta_lim)


def test_first_episodes_end_where_the_host_class_ends_them():
    from aur_ppo_amd.envs import CartPoleVecEnv as H
    N, T = 33, 40
    i = np.arange(N)
    st = np.stack([2.35 - 0.03 * i, np.full(N, 1.0), 0.002 * (i % 7), np.zeros(N)], 1)
    st[1::2, 0] *= -1.0          # every other env runs at the left limit
    st[1::2, 1] *= -1.0
    steps = np.zeros(N, np.int64)
    actions = (st[:, 1] > 0).astype(np.float32)           # push on, the same action every step
    host, env = _host_env(st, steps), _device_env(N, seed=4)
    env.set_state(st, steps)
    env.begin_rollout(T)
    first_h, first_d = np.full(N, -1), np.full(N, -1)
    len_h, len_d = np.zeros(N, np.int64), np.zeros(N, np.int64)
    act_t = torch.from_numpy(actions).cuda()
    for t in range(T):
        going, pre = first_h < 0, host.state
        for pos, vel, lim in ((0, 1, H.x_lim), (2, 3, H.theta_lim)):        # no first episode is decided by a last bit
            assert (np.abs(np.abs(pre[going, pos] + H.tau * pre[going, vel]) - lim) >= 1e-9).all()
        _, _, done_h, _, info = host.step(actions)
        _, _, done, _, _ = env.step(act_t)
        done_d = done.cpu().numpy() != 0
        row = env.ep_len[t].cpu().numpy()
        assert np.array_equal(row > 0, done_d)
        state_d, steps_d, episode_d = env.get_state()
        new_d = done_d & (first_d < 0)
        if new_d.any():            # behind its first done an env holds the restatement's draw for episode 1
            assert (episode_d[new_d] == 1).all() and not steps_d[new_d].any()
            ref = R.reset_states(4, 0, N, episodes=np.ones(N))
            assert np.array_equal(_bits(state_d[new_d]), _bits(ref[new_d]))
        hl = _host_lengths(info, N)
        new_h = done_h & (first_h < 0)
        first_h[new_h], len_h[new_h] = t, hl[new_h]
        first_d[new_d], len_d[new_d] = t, row[new_d]
    assert (first_h >= 0).all(), "the start states are meant to end every first episode inside the 40 steps"
    assert np.array_equal(first_d, first_h) and np.array_equal(len_d, len_h)
    assert np.array_equal(len_h, first_h + 1) and len(set(first_h.tolist())) > 3


# ---------------------------------------------------------------------------------------------- K16 against T x (K8, K15)
def _policy(seed=0, scale=40.0):
    from aur_ppo_amd import hip_ops as Hops
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(seed)
    pol = actor_critic(4, 2, 64, 2, 0.0, False).cuda()
    with torch.no_grad():
        pol.actor.net[4].weight.mul_(scale)          # W3 of the actor: logits that move with the state, so both actions occur
    bucket = FlatBucket(pol.parameters())
    lay = Hops.mlp_layout(pol, bucket)
    assert Hops.cartpole_rollout_ok(lay)
    return pol, bucket, lay


def _start(N, T, seed=5):
    """Start states from which some envs terminate inside T (they sit at a limit, moving out) and some truncate (steps = 495)."""
    rs = np.random.RandomState(seed)
    st = rs.uniform(-0.05, 0.05, (N, 4))
    steps = np.zeros(N, np.int64)
    st[0::4, 0], st[0::4, 1] = 2.39, 1.5            # out at x within a step or two
    st[2::8, 2], st[2::8, 3] = -0.2, -1.0           # out at theta
    steps[1::3] = 495 if T >= 5 else 499
    done0 = (np.arange(N) % 3 == 0).astype(np.float32)
    return st, steps, done0


def _buffers(T, N):
    z = lambda *s, dt=torch.float32: torch.full(s, -7, dtype=dt, device="cuda")       # poisoned: every element must be written
    return dict(states=z(T, N, 4), terminals=z(T, N), actions=z(T, N), log_probs=z(T, N), values=z(T, N), rewards=z(T, N),
                ep_len=z(T, N, dt=torch.int32))


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs at {int((a[k] != b[k]).sum())} places"


@pytest.mark.parametrize("N,T", [(1, 1), (33, 5), (70, 40)])
def test_one_launch_equals_T_steps_bit_for_bit(N, T):
    from aur_ppo_amd import hip_ops as Hops
    _, bucket, lay = _policy()
    st, steps, done0 = _start(N, T)
    noise = torch.rand((T, N), device="cuda", generator=torch.Generator("cuda").manual_seed(8))
    # route 1: K16
    e1 = _device_env(N, seed=21)
    obs1 = e1.set_state(st, steps).contiguous()
    done1 = torch.from_numpy(done0).cuda()
    b1 = _buffers(T, N)
    Hops.cartpole_rollout(e1.native_state(), bucket.flat_param, lay, noise, b1["states"], b1["terminals"], b1["actions"], b1["log_probs"],
                          b1["values"], b1["rewards"], b1["ep_len"], obs1, done1)
    # route 2: T x (K8, K15)
    e2 = _device_env(N, seed=21)
    obs2 = e2.set_state(st, steps).contiguous()
    done2 = torch.from_numpy(done0).cuda()
    b2 = _buffers(T, N)
    e2.begin_rollout(T)
    for t in range(T):
        b2["states"][t] = obs2
        b2["terminals"][t] = done2
        Hops.mlp_act(obs2, noise[t], bucket.flat_param, lay, b2["actions"][t], b2["log_probs"][t], b2["values"][t])
        obs2, rew, done2, _, _ = e2.step(b2["actions"][t])
        b2["rewards"][t] = rew
    b2["ep_len"] = e2.ep_len
    _same(b1, b2, f"N={N} T={T}")
    assert torch.equal(obs1, obs2) and torch.equal(done1, done2)
    s1, s2 = e1.get_state(), e2.get_state()
    assert np.array_equal(_bits(s1[0]), _bits(s2[0])) and np.array_equal(s1[1], s2[1]) and np.array_equal(s1[2], s2[2])
    if N > 1:      # the comparison covered what it is meant to: both actions, terminations and truncations
        lens = b1["ep_len"].cpu().numpy()
        assert set(b1["actions"].unique().tolist()) == {0.0, 1.0}
        assert (lens == 500).any() and ((lens > 0) & (lens < 500)).any()


def _agent(N, T, **more):
    from aur_ppo_amd.ppo import ppo
    torch.manual_seed(0)
    a = ppo(dict(HP, num_envs=N, num_steps=T, total_timesteps=N * T * 4, device_env=True, **more))
    with torch.no_grad():
        a.policy.actor.net[4].weight.mul_(40.0)
    return a


def _agent_rollouts(agent, N, T, n_rollouts):
    """``n_rollouts`` rollouts of ``ppo._rollout`` from _start's states; a copy of everything each one left."""
    from aur_ppo_amd.envs import CartPoleDeviceVecEnv
    assert isinstance(agent.envs, CartPoleDeviceVecEnv)
    agent.envs.reset(seed=list(range(N)))
    st, steps, done0 = _start(N, T)
    next_obs, next_done = agent.envs.set_state(st, steps).contiguous(), torch.from_numpy(done0).cuda()
    out, gs = [], 0
    for k in range(n_rollouts):
        torch.manual_seed(100 + k)          # the rollout's noise: the same draw on every route
        next_obs, next_done, gs = agent._rollout(next_obs, next_done, gs, None)
        b = agent.buffer
        snap = dict(states=b.states, terminals=b.terminals, actions=b.actions, log_probs=b.log_probs, values=b.values, rewards=b.rewards,
                    ep_len=agent.envs.ep_len, next_obs=next_obs, next_done=next_done, env_state=agent.envs.state,
                    env_steps=agent.envs.steps, env_episode=agent.envs.episode)
        out.append({k2: v.clone() for k2, v in snap.items()})
    assert gs == n_rollouts * N * T
    return out


@pytest.mark.parametrize("N,T", [(33, 5), (70, 40)])
def test_ppo_rollout_routes_agree(N, T, monkeypatch):
    """ppo._rollout on the one-launch route, and with AURPPO_ROLLOUT_KERNEL=0 on the per-step route eagerly, at capture and at
    replay: the same tensors, and the same episode statistics."""
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
        _same(x, y, f"rollout {k}")
    assert len(a.total_returns) > 0
    assert (a.total_returns, a.total_episode_lengths, a.x_indices) == (b.total_returns, b.total_episode_lengths, b.x_indices)
    c = _agent(N, T, hip_graph=False)                          # ... and with no graph at all
    rc = _agent_rollouts(c, N, T, 2)
    assert c._ro_graph is None
    for k, (x, y) in enumerate(zip(ra, rc)):
        _same(x, y, f"eager rollout {k}")


def test_device_env_learns():
    """The plumbing config of test_gpu_train_end_to_end_synthetic_and_cartpole (its hp2) on the device env, held to that test's own
    criterion."""
    from aur_ppo_amd.envs import CartPoleDeviceVecEnv
    from aur_ppo_amd.ppo import ppo
    agent = ppo(dict(HP, device_env=True))
    assert isinstance(agent.envs, CartPoleDeviceVecEnv) and agent._one_launch_rollout()
    r, l, x = agent.train()
    assert len(r) == len(l) == len(x)
    assert len(r) > 20
    assert np.mean(r[-10:]) > 2.0 * np.mean(r[:10]), (np.mean(r[:10]), np.mean(r[-10:]))


@pytest.mark.parametrize("shape", ["wide", "three_actions", "gaussian"])
def test_other_policy_shapes_are_refused(shape):
    from aur_ppo_amd import hip_ops as Hops
    from aur_ppo_amd.actor_critic import actor_critic
    from aur_ppo_amd.flat import FlatBucket
    torch.manual_seed(0)
    pol = {"wide": lambda: actor_critic(4, 2, 128, 2, 0.0, False), "three_actions": lambda: actor_critic(4, 3, 64, 2, 0.0, False),
           "gaussian": lambda: actor_critic(4, (2,), 64, 2, 0.0, True)}[shape]().cuda()
    bucket = FlatBucket(pol.parameters())
    lay = Hops.mlp_layout(pol, bucket)
    assert lay is not None and not Hops.cartpole_rollout_ok(lay)
    N, T = 5, 3
    env = _device_env(N)
    before = [t.clone() for t in (env.state, env.steps, env.episode)]
    b = _buffers(T, N)
    with pytest.raises(RuntimeError, match=r"aurppo_cartpole_rollout_f32 failed \(rc=-2\)"):
        Hops.cartpole_rollout(env.native_state(), bucket.flat_param, lay, torch.rand((T, N), device="cuda"), b["states"], b["terminals"],
                              b["actions"], b["log_probs"], b["values"], b["rewards"], b["ep_len"], torch.zeros((N, 4), device="cuda"),
                              torch.zeros(N, device="cuda"))
    assert all(torch.equal(x, y) for x, y in zip(before, (env.state, env.steps, env.episode))) and (b["states"] == -7).all()


def test_ppo_steps_the_device_env_for_a_wide_policy():
    """A policy K16 is not built for (2 x 128: K8w) keeps the device env on the per-step route."""
    from aur_ppo_amd.ppo import ppo
    N, T = 33, 5
    torch.manual_seed(0)
    agent = ppo(dict(HP, num_envs=N, num_steps=T, total_timesteps=N * T * 4, device_env=True, hidden_dim=128))
    assert agent._mlp is not None and agent._mlp["wide"] and not agent._one_launch_rollout()
    obs = agent.envs.reset(seed=list(range(N)))[0]
    ref = R.reset_states(0, 0, N).astype(np.float32)
    next_obs, next_done, gs = agent._rollout(obs, torch.zeros(N, device="cuda"), 0, None)
    assert gs == N * T and np.array_equal(agent.buffer.states[0].cpu().numpy(), ref)
    assert (agent.buffer.rewards == 1.0).all() and agent.envs.steps.max().item() <= T
    assert set(agent.buffer.actions.unique().tolist()) <= {0.0, 1.0}
