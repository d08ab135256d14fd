"""CPU: the built-in Pendulum-v1 -- the host class's core step and wrapper arithmetic (known answers), the Philox restatement the GPU
tests compare with, the episode-table reader with returns, ``make_vec_env``'s switch, and every refusal that happens before a kernel
is reached."""
import ctypes as C
import math
import sys

import numpy as np
import pytest
import torch

from tests import pendulum_ref as R


def _host(n=1, **state):
    from aur_ppo_amd.envs import PendulumVecEnv
    env = PendulumVecEnv(n)
    if state:
        env.set_state(**{k: np.full(n, v) if np.ndim(v) == 0 else np.asarray(v) for k, v in state.items()})
    return env


def _raw_reward(env, action):
    """The raw reward of one step, read through the episode statistics (ep_ret is the fp64 sum of the raw rewards)."""
    before = env.get_state()["ep_ret"]
    env.step(np.asarray(action, np.float32).reshape(env.num_envs, 1))
    return env.get_state()["ep_ret"] - before


# ---------------------------------------------------------------------------------------------- make_vec_env
def test_make_vec_env_returns_the_host_class_without_gym(monkeypatch):
    from aur_ppo_amd import envs
    monkeypatch.setitem(sys.modules, "gym", None)           # `import gym` raises ImportError: the built-in classes are what is left
    monkeypatch.delenv("AURPPO_DEVICE_ENV", raising=False)
    e = envs.make_vec_env("Pendulum-v1", 3, True, "cpu", {})
    assert type(e) is envs.PendulumVecEnv and not e.device_native
    assert e.single_observation_space.shape == (3,) and e.single_action_space.shape == (1,)
    obs, info = e.reset()
    assert obs.shape == (3, 3) and obs.dtype == np.float32 and info == {}
    with pytest.raises(RuntimeError, match=r"built-ins: 'CartPole-v1', 'Pendulum-v1', 'Synthetic-v0'"):
        envs.make_vec_env("Acrobot-v1", 3, False, "cpu", {})


class _Stub:
    def __init__(self, num_envs, device, seed=0):
        self.args = (num_envs, str(device), seed)


def test_make_vec_env_switch(monkeypatch):
    from aur_ppo_amd import envs
    monkeypatch.setitem(sys.modules, "gym", None)
    monkeypatch.setattr(envs, "PendulumDeviceVecEnv", _Stub)
    monkeypatch.delenv("AURPPO_DEVICE_ENV", raising=False)
    assert type(envs.make_vec_env("Pendulum-v1", 3, True, "cuda", {})) is envs.PendulumVecEnv           # unset: the host class
    assert type(envs.make_vec_env("Pendulum-v1", 3, True, "cuda", {"device_env": False})) is envs.PendulumVecEnv
    e = envs.make_vec_env("Pendulum-v1", 3, True, "cuda", {"device_env": True, "env_seed": 9})
    assert type(e) is _Stub and e.args == (3, "cuda", 9)
    assert type(envs.make_vec_env("Pendulum-v1", 3, True, "cpu", {"device_env": True})) is envs.PendulumVecEnv     # a CUDA device only
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cpu", {"device_env": True})) is envs.CartPoleVecEnv
    monkeypatch.setenv("AURPPO_DEVICE_ENV", "1")
    assert type(envs.make_vec_env("Pendulum-v1", 3, True, "cuda", {})) is _Stub
    monkeypatch.setenv("AURPPO_DEVICE_ENV", "0")
    assert type(envs.make_vec_env("Pendulum-v1", 3, True, "cuda", {})) is envs.PendulumVecEnv


def test_cpu_device_is_refused():
    from aur_ppo_amd.envs import PendulumDeviceVecEnv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PendulumDeviceVecEnv(4, "cpu")
    assert PendulumDeviceVecEnv.device_native and PendulumDeviceVecEnv.capturable
    assert PendulumDeviceVecEnv.rollout_op == "pendulum_rollout"


def test_reset_refuses_a_seed_list_that_is_not_consecutive():
    from aur_ppo_amd.envs import PendulumDeviceVecEnv
    env = PendulumDeviceVecEnv.__new__(PendulumDeviceVecEnv)        # no device here: reset() must refuse before it needs one
    env.num_envs = 4
    for seeds in ([0, 1, 3, 4], [3, 2, 1, 0], [0, 1, 2], [-1, 0, 1, 2]):
        with pytest.raises(ValueError, match="consecutive"):
            env.reset(seed=seeds)


def test_the_trainer_takes_the_host_class_as_continuous_with_one_action(monkeypatch):
    """What ``run_ppo.py -id Pendulum-v1 -c true`` builds with no gym installed: the host class, A = 1, and train() runs on it."""
    from aur_ppo_amd import envs
    from aur_ppo_amd.ppo import ppo
    from aur_ppo_amd.run_ppo import build_parser, params_from_args
    from tests import oracle_ops
    monkeypatch.setitem(sys.modules, "gym", None)
    monkeypatch.delenv("AURPPO_DEVICE_ENV", raising=False)
    p = params_from_args(build_parser().parse_args(["-id", "Pendulum-v1", "-c", "true"]))
    assert p["gym_id"] == "Pendulum-v1" and p["continuous"] is True
    p.update(num_envs=2, num_steps=100, total_timesteps=2 * 100 * 3, num_minibatches=4, num_update_epochs=1, log=False, save=False, device="cpu")
    a = ppo(p, ops=oracle_ops)
    assert type(a.envs) is envs.PendulumVecEnv and a.action_dim == (1,) and a.state_dim == (3,)
    r, l, x = a.train()
    # 300 steps of 2 envs: both truncate at step 200 (global step 400), and the trainer logs a step's first finished env
    assert l == [200] and x == [400] and -3500.0 < r[0] < 0.0        # a step's cost is below 16.3


# ---------------------------------------------------------------------------------------------- the core step
def test_core_known_answers():
    env = _host(1, th=0.0, thdot=0.0)
    assert _raw_reward(env, [0.0])[0] == 0.0
    s = env.get_state()
    assert s["th"][0] == 0.0 and s["thdot"][0] == 0.0 and s["steps"][0] == 1
    env = _host(1, th=math.pi / 2, thdot=0.0)
    r = _raw_reward(env, [0.0])[0]
    s = env.get_state()
    assert s["thdot"][0] == 0.75 and s["th"][0] == math.pi / 2 + 0.0375 and r == -(math.pi / 2) ** 2
    # (15 * sin(pi / 2) + 3 * 0) * 0.05: sin(pi / 2) is exactly 1 in fp64


def test_torque_is_clipped_and_the_speed_too():
    a, b = _host(1, th=0.3, thdot=-0.2), _host(1, th=0.3, thdot=-0.2)
    ra, rb = _raw_reward(a, [5.0])[0], _raw_reward(b, [2.0])[0]
    assert ra == rb and a.get_state()["thdot"][0] == b.get_state()["thdot"][0] and a.get_state()["th"][0] == b.get_state()["th"][0]
    assert _raw_reward(_host(1, th=0.3, thdot=-0.2), [-7.0])[0] == _raw_reward(_host(1, th=0.3, thdot=-0.2), [-2.0])[0]
    assert ra != _raw_reward(_host(1, th=0.3, thdot=-0.2), [1.0])[0]
    up = _host(1, th=math.pi / 2, thdot=7.9)
    up.step(np.array([[2.0]], np.float32))                  # 7.9 + (15 + 6) * 0.05 = 8.95
    assert up.get_state()["thdot"][0] == 8.0 and up.get_state()["th"][0] == math.pi / 2 + 8.0 * 0.05
    dn = _host(1, th=-math.pi / 2, thdot=-7.9)
    dn.step(np.array([[-2.0]], np.float32))
    assert dn.get_state()["thdot"][0] == -8.0


def test_angle_normalize_is_numpys_floored_modulo():
    from aur_ppo_amd.envs import PendulumVecEnv as P
    xs = np.array([-math.pi, math.pi, 3 * math.pi + 0.1, -7.0])
    got = P.angle_normalize(xs)
    assert np.array_equal(got, ((xs + np.pi) % (2 * np.pi)) - np.pi)
    assert got[0] == -math.pi and got[1] == -math.pi                    # both ends fold to -pi: the range is [-pi, pi)
    assert abs(got[2] - (-math.pi + 0.1)) < 1e-14 and abs(got[3] - (2 * math.pi - 7.0)) < 1e-14
    assert ((got >= -math.pi) & (got < math.pi)).all()
    # ... and the cost is formed from it: th = -7 costs what th = 2 pi - 7 costs
    assert abs(_raw_reward(_host(1, th=-7.0, thdot=0.0), [0.0])[0] + (2 * math.pi - 7.0) ** 2) < 1e-13


# ---------------------------------------------------------------------------------------------- the wrappers
def test_first_observation_statistics():
    env = _host(2)
    obs, _ = env.reset()
    s = env.get_state()
    raw = np.stack([np.cos(s["th"]), np.sin(s["th"]), s["thdot"]], 1).astype(np.float32).astype(np.float64)
    assert np.array_equal(s["obs_count"], [1.0001, 1.0001])
    assert np.array_equal(s["obs_mean"], raw / 1.0001)
    var = (1.0 * 1e-4 + raw ** 2 * 1e-4 / 1.0001) / 1.0001
    assert np.array_equal(s["obs_var"], var)
    assert np.array_equal(obs, np.clip((raw - raw / 1.0001) / np.sqrt(var + 1e-8), -10, 10).astype(np.float32))
    for i in range(2):                                       # ... and as the restatement forms them, scalar by scalar
        ref_obs, stats = R.first_obs(s["th"][i], s["thdot"][i])
        assert np.array_equal(obs[i], ref_obs)
        assert [m for m, _, _ in stats] == s["obs_mean"][i].tolist() and [v for _, v, _ in stats] == s["obs_var"][i].tolist()
    assert (s["ret"] == 0).all() and (s["ret_count"] == 1e-4).all() and (s["ep_ret"] == 0).all()


def test_rms_update_restatement():
    m, v, c = R.rms_update(0.0, 1.0, 1e-4, 3.0)
    assert (m, c) == (3.0 / 1.0001, 1.0001) and v == (1e-4 + 9.0 * 1e-4 / 1.0001) / 1.0001
    m2, v2, c2 = R.rms_update(m, v, c, -1.0)
    d = -1.0 - m
    assert (m2, c2) == (m + d / (c + 1), c + 1) and v2 == (v * c + d ** 2 * c / (c + 1)) / (c + 1)


def test_observation_and_reward_clip_at_ten():
    env = _host(1, th=0.0, thdot=0.0, obs_mean=np.array([[-5.0, 5.0, 0.0]]), obs_var=np.full((1, 3), 1e-6), obs_count=1e9,
                ret_var=1e-8, ret_count=1e9, ret_mean=0.0)
    obs, rew, _, _, _ = env.step(np.array([[2.0]], np.float32))      # cos ~ 1 is 6000 deviations above -5, sin ~ 0 as far below 5
    assert obs[0, 0] == 10.0 and obs[0, 1] == -10.0
    assert rew[0] == -10.0                                           # a raw reward of -0.004 over sqrt(~2e-8)
    assert obs.dtype == np.float32 and rew.dtype == np.float32


def test_reward_wrapper_arithmetic_and_ret_survives_a_truncation():
    env = _host(1, th=1.0, thdot=0.5, steps=198, ret=-3.0)
    s0 = env.get_state()
    r1 = _raw_reward(env, [0.3])[0]
    s1 = env.get_state()
    assert s1["ret"][0] == -3.0 * 0.99 + r1
    m, v, c = R.rms_update(s0["ret_mean"][0], s0["ret_var"][0], s0["ret_count"][0], s1["ret"][0])
    assert (s1["ret_mean"][0], s1["ret_var"][0], s1["ret_count"][0]) == (m, v, c)
    before = env.get_state()["ep_ret"][0]
    _, rew, done, trunc, info = env.step(np.array([[0.3]], np.float32))          # step 200: the truncation
    s2 = env.get_state()
    r2 = info["final_info"][0]["episode"]["r"] - before
    assert done[0] and trunc[0] and s2["steps"][0] == 0
    assert s2["ret"][0] == s1["ret"][0] * 0.99 + r2 and s2["ret"][0] != 0.0      # gym 0.26.2 clears it on `terminated` only
    assert rew[0] == np.float32(np.clip(r2 / np.sqrt(s2["ret_var"][0] + 1e-8), -10, 10))
    assert s2["ep_ret"][0] == 0.0


def test_the_200th_step_reports_the_episode_and_takes_two_observations():
    env = _host(3)
    env.reset(seed=5)
    total = np.zeros(3)
    for t in range(199):
        total += _raw_reward(env, np.full(3, 0.5))
    s = env.get_state()
    assert (s["steps"] == 199).all() and np.abs(s["obs_count"] - (1e-4 + 200)).max() < 1e-9        # the reset one and 199 steps
    last = s["ep_ret"].copy()
    obs, _, done, trunc, info = env.step(np.full((3, 1), 0.5, np.float32))
    s2 = env.get_state()
    assert done.all() and trunc.all()
    assert [f["episode"]["l"] for f in info["final_info"]] == [200] * 3
    finals = np.array([f["episode"]["r"] for f in info["final_info"]])
    from aur_ppo_amd.envs import PendulumVecEnv as P
    cost = P.angle_normalize(s["th"]) ** 2 + 0.1 * s["thdot"] ** 2 + 0.001 * 0.5 ** 2
    assert np.allclose(last, total, rtol=0, atol=1e-9) and np.array_equal(finals, last + -cost)      # the raw return, the 200th reward in it
    assert np.array_equal(s2["obs_count"], s["obs_count"] + 2)                  # the final observation, then the reset one
    assert (s2["steps"] == 0).all() and (s2["ep_ret"] == 0).all()
    raw = np.stack([np.cos(s2["th"]), np.sin(s2["th"]), s2["thdot"]], 1).astype(np.float32).astype(np.float64)
    assert np.array_equal(obs, np.clip((raw - s2["obs_mean"]) / np.sqrt(s2["obs_var"] + 1e-8), -10, 10).astype(np.float32))
    assert (np.abs(s2["th"]) <= math.pi).all() and (np.abs(s2["thdot"]) <= 1).all()       # the returned one is the reset observation
    # the step before: no final_info, one observation
    assert "final_info" not in _host(1, steps=10).step(np.zeros((1, 1), np.float32))[4]


def test_set_state_round_trip_and_refusals():
    env = _host(2)
    s = env.get_state()
    assert set(s) == {"th", "thdot", "steps", "obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "ret", "ep_ret"}
    other = _host(2)
    other.set_state(**s)
    a = env.step(np.array([[0.1], [-0.4]], np.float32))
    b = other.step(np.array([[0.1], [-0.4]], np.float32))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError, match="obs_mean"):
        env.set_state(obs_mean=np.zeros(2))
    with pytest.raises(ValueError, match="speed"):
        env.set_state(speed=np.zeros(2))


# ---------------------------------------------------------------------------------------------- the reset draw's restatement
def test_philox_known_answers_for_pendulums_counter():
    h = lambda words: " ".join("%08x" % w for w in words)
    assert h(R.reset_words(0, 0, 0)) == "844515e1 f08d6eaa 0f19c053 83f875f0"
    assert h(R.reset_words((5 << 32) + 17, 7, 3)) == "0d9c1d26 451e4813 abff7506 ba77db13"
    from tests.cartpole_ref import philox4x32_10
    assert R.reset_words(0, 0, 0) != philox4x32_10((0, 0, 0, 0), (0, 0))           # the third word keeps the stream apart from CartPole's
    th, thdot = R.reset_state(1, 5, 3)
    assert (float(th).hex(), float(thdot).hex()) == ("-0x1.7c5925f446280p-3", "0x1.60b5100000000p-2")


def test_reset_ranges():
    s = R.reset_states(7, 11, 256)
    assert s.shape == (256, 2) and s.dtype == np.float64
    assert (s[:, 0] >= -math.pi).all() and (s[:, 0] < math.pi).all() and (s[:, 1] >= -1).all() and (s[:, 1] < 1).all()
    assert s[:, 0].min() < -2.5 and s[:, 0].max() > 2.5 and s[:, 1].min() < -0.8 and s[:, 1].max() > 0.8
    assert len({tuple(r) for r in s}) == 256
    assert R.reset_state(7, 11, 0) != R.reset_state(7, 11, 1) and R.reset_state(7, 11, 0) != R.reset_state(7 + (1 << 32), 11, 0)
    from aur_ppo_amd.envs import PendulumVecEnv
    h = PendulumVecEnv(64).get_state()                       # the host class's own draws (numpy's RandomState) keep the same ranges
    assert (np.abs(h["th"]) <= math.pi).all() and (np.abs(h["thdot"]) <= 1).all()


# ---------------------------------------------------------------------------------------------- the episode tables
def test_episode_triples_with_and_without_returns():
    from aur_ppo_amd.envs import episode_triples
    lens = torch.tensor([[0, 0, 0, 0],
                         [0, 200, 0, 200],      # two envs finish: the lower index is logged
                         [0, 0, 0, 0],
                         [200, 0, 0, 0],
                         [0, 0, 0, 200]], dtype=torch.int32)
    rets = torch.tensor([[9.0, 9.0, 9.0, 9.0],     # (garbage where ep_len == 0 is never read)
                         [9.0, -812.5, 9.0, -1.0],
                         [9.0, 9.0, 9.0, 9.0],
                         [-1500.25, 9.0, 9.0, 9.0],
                         [9.0, 9.0, 9.0, -0.5]])
    assert episode_triples(lens, 1000, 8, ep_ret=rets) == [(-812.5, 200, 1016), (-1500.25, 200, 1032), (-0.5, 200, 1040)]
    assert episode_triples(lens, 1000, 8) == [(200.0, 200, 1016), (200.0, 200, 1032), (200.0, 200, 1040)]       # as before
    assert episode_triples(lens, 1000, 8, None) == episode_triples(lens, 1000, 8)
    assert episode_triples(torch.zeros((3, 2), dtype=torch.int32), 0, 2, ep_ret=torch.zeros((3, 2))) == []
    assert episode_triples(torch.tensor([[5]], dtype=torch.int32), 0, 1, ep_ret=torch.tensor([[-2.0]])) == [(-2.0, 5, 1)]


# ---------------------------------------------------------------------------------------------- refusals in front of a kernel
def _env_state(n, **over):
    st = dict(state=torch.zeros((n, 16), dtype=torch.float64), steps=torch.zeros(n, dtype=torch.int32),
              episode=torch.zeros(n, dtype=torch.int32), seed=0, env0=0, consts=(10.0, 1.0, 1.0, 0.05, 8.0, 2.0, 200))
    st.update(over)
    return st


def _rollout_args(T, N):
    f = lambda *s: torch.zeros(s)
    return dict(noise=f(T, N, 1), states=f(T, N, 3), terminals=f(T, N), actions=f(T, N, 1), log_probs=f(T, N), values=f(T, N),
                rewards=f(T, N), ep_len=torch.zeros((T, N), dtype=torch.int32), ep_ret=f(T, N), next_obs=f(N, 3), next_done=f(N))


LAYOUT = dict(offsets=list(range(13)), n_params=100, D=3, A=1, continuous=True, hidden=64, num_layers=2, wide=False)


def test_value_errors_come_before_the_library():
    from aur_ppo_amd import hip_ops as H
    with pytest.raises(ValueError, match="state"):
        H.pendulum_reset(_env_state(3, state=torch.zeros((3, 4), dtype=torch.float64)), torch.zeros((3, 3)))     # CartPole's block
    with pytest.raises(ValueError, match="state"):
        H.pendulum_reset(_env_state(3, state=torch.zeros((3, 16))), torch.zeros((3, 3)))                         # fp32
    with pytest.raises(ValueError, match="steps"):
        H.pendulum_reset(_env_state(3, steps=torch.zeros(3, dtype=torch.int64)), torch.zeros((3, 3)))
    with pytest.raises(ValueError, match="obs"):
        H.pendulum_reset(_env_state(3), torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="consts"):
        H.pendulum_reset(_env_state(3, consts=(9.8, 1.0, 0.1, 0.5, 10.0, 0.02, 0.2, 2.4, 500)), torch.zeros((3, 3)))
    with pytest.raises(ValueError, match="env0"):
        H.pendulum_reset(_env_state(3, env0=-1), torch.zeros((3, 3)))
    ok = dict(action=torch.zeros((3, 1)), obs=torch.zeros((3, 3)), reward=torch.zeros(3), done=torch.zeros(3),
              ep_len=torch.zeros(3, dtype=torch.int32), ep_ret=torch.zeros(3))
    for name, bad in (("action", torch.zeros((3, 2))), ("action", torch.zeros(3, dtype=torch.float64)), ("obs", torch.zeros((3, 4))),
                      ("reward", torch.zeros(2)), ("done", torch.zeros((3, 1))), ("ep_len", torch.zeros(3)),
                      ("ep_ret", torch.zeros(3, dtype=torch.int32))):
        with pytest.raises(ValueError, match=name):
            H.pendulum_step(_env_state(3), **dict(ok, **{name: bad}))
    flat = torch.zeros(128)
    for name, bad in (("noise", torch.zeros((5, 3))), ("noise", torch.zeros((5, 3, 2))), ("states", torch.zeros((5, 3, 4))),
                      ("actions", torch.zeros((5, 3))), ("ep_len", torch.zeros((5, 3))), ("ep_ret", torch.zeros((5, 3), dtype=torch.int32)),
                      ("next_obs", torch.zeros((3, 3), dtype=torch.float64)), ("next_done", torch.zeros(4)),
                      ("values", torch.zeros((5, 6))[:, ::2])):
        with pytest.raises(ValueError, match=name):
            H.pendulum_rollout(_env_state(3), flat, LAYOUT, **dict(_rollout_args(5, 3), **{name: bad}))
    with pytest.raises(ValueError, match="smaller than the policy"):
        H.pendulum_rollout(_env_state(3), torch.zeros(50), LAYOUT, **_rollout_args(5, 3))


def test_rollout_shape_rule():
    from aur_ppo_amd import hip_ops as H
    assert H.pendulum_rollout_ok(LAYOUT)
    assert not H.pendulum_rollout_ok(None)
    for change in (dict(wide=True), dict(A=2), dict(continuous=False), dict(D=4), dict(hidden=128), dict(num_layers=3), dict(layered=True)):
        assert not H.pendulum_rollout_ok(dict(LAYOUT, **change)), change
    assert not H.cartpole_rollout_ok(LAYOUT)                 # ... and each env's rule refuses the other's policy
    assert not H.pendulum_rollout_ok(dict(LAYOUT, D=4, A=2, continuous=False))


def test_library_refuses_before_any_launch():
    """The C entries' argument checks need no device: null pointers are EINVAL (-1), sizes and policy shapes ESHAPE (-2)."""
    import __graft_entry__ as g
    g.build()
    from aur_ppo_amd import _lib
    lib = _lib.load()
    consts = (10.0, 1.0, 1.0, 0.05, 8.0, 2.0, 200)
    assert lib.aurppo_pendulum_reset(None, None, None, None, 4, 0, 0, 0, None) == -1 and b"null pointer" in lib.aurppo_last_error()
    assert lib.aurppo_pendulum_step(*[None] * 9, 4, 0, 0, 0, *consts, None) == -1 and b"null pointer" in lib.aurppo_last_error()
    buf = (C.c_double * 64)()            # a host buffer: every check below returns before a pointer is followed on the device
    p = C.cast(buf, C.c_void_p)
    lay = (C.c_int * 13)(*range(13))

    def rollout(N=4, T=2, D=3, A=1, cont=1, hidden=64, layers=2, n_params=100, lay=lay, first=p, consts=consts):
        return lib.aurppo_pendulum_rollout_f32(first, p, p, p, p, p, N, T, D, A, cont, hidden, layers, p, lay, n_params, p, p, p, p, p, p, p, p,
                                               0, 0, 0, *consts, None)
    assert rollout(first=None) == -1 and b"null pointer" in lib.aurppo_last_error()
    assert rollout(N=0) == -2 and rollout(T=0) == -2
    assert rollout(hidden=128) == -2 and b"hidden_dim=128" in lib.aurppo_last_error()
    assert rollout(layers=3) == -2
    assert rollout(D=4) == -2 and rollout(A=2) == -2 and rollout(cont=0) == -2
    assert b"Gaussian" in lib.aurppo_last_error()
    assert rollout(lay=(C.c_int * 13)(*([0] * 12 + [100]))) == -2 and b"layout[12]=100" in lib.aurppo_last_error()     # the log-std's offset
    assert rollout(consts=(10.0, 1.0, 1.0, 0.05, 8.0, 2.0, 0)) == -1 and b"max_steps=0" in lib.aurppo_last_error()
    assert lib.aurppo_pendulum_reset(p, p, p, p, 0, 0, 0, 0, None) == -2
    assert lib.aurppo_pendulum_reset(p, p, p, p, 4, -1, 0, 0, None) == -2
    assert lib.aurppo_pendulum_step(*[p] * 9, 4, 0, 0, 0, 10.0, 0.0, 1.0, 0.05, 8.0, 2.0, 200, None) == -1          # m = 0


# ---------------------------------------------------------------------------------------------- the argument order at the C boundary
def test_pointer_order_at_the_c_boundary(monkeypatch):
    """Rows of same-typed pointers: a transposition raises nothing on the host and faults on the GPU.  Every pointer hip_ops hands to
    the three entries is the tensor include/aurppo.h names at that position."""
    from aur_ppo_amd import hip_ops as H
    calls = []

    class Lib:
        def __getattr__(self, fn):
            return lambda *args: calls.append((fn, [a.value if isinstance(a, C.c_void_p) else a for a in args])) or 0

    def ptr(t, dtype=torch.float32):
        assert t.dtype == dtype and t.is_contiguous()
        return C.c_void_p(t.data_ptr())
    monkeypatch.setattr(H, "_lib_or_raise", lambda: Lib())
    monkeypatch.setattr(H, "_ptr", ptr)
    monkeypatch.setattr(H, "_stream", lambda: C.c_void_p(0x57))
    T, N = 5, 3
    es = _env_state(N, seed=(5 << 32) + 17, env0=6)
    env3 = [es["state"].data_ptr(), es["steps"].data_ptr(), es["episode"].data_ptr()]
    seed3, consts = [6, 17, 5], [10.0, 1.0, 1.0, 0.05, 8.0, 2.0, 200]
    obs = torch.zeros((N, 3))
    H.pendulum_reset(es, obs)
    assert calls.pop() == ("aurppo_pendulum_reset", env3 + [obs.data_ptr(), N] + seed3 + [0x57])
    k = dict(action=torch.zeros((N, 1)), obs=obs, reward=torch.zeros(N), done=torch.zeros(N), ep_len=torch.zeros(N, dtype=torch.int32),
             ep_ret=torch.zeros(N))
    H.pendulum_step(es, **k)
    assert calls.pop() == ("aurppo_pendulum_step", env3 + [k[n].data_ptr() for n in ("action", "obs", "reward", "done", "ep_len", "ep_ret")]
                           + [N] + seed3 + consts + [0x57])
    r, flat = _rollout_args(T, N), torch.zeros(128)
    H.pendulum_rollout(es, flat, LAYOUT, **r)
    fn, args = calls.pop()
    lay = args[14]
    assert fn == "aurppo_pendulum_rollout_f32" and list(lay) == list(range(13))
    assert args[:14] == env3 + [r["next_obs"].data_ptr(), r["next_done"].data_ptr(), r["noise"].data_ptr(), N, T, 3, 1, 1, 64, 2, flat.data_ptr()]
    assert args[15:] == ([100] + [r[n].data_ptr() for n in ("states", "terminals", "actions", "log_probs", "values", "rewards", "ep_len",
                                                               "ep_ret")] + seed3 + consts + [0x57])
