"""CPU: the host side of the device CartPole -- the Philox restatement the GPU tests compare with (known answers), the episode-table
reader, ``make_vec_env``'s switch, and every refusal that happens before a kernel is reached."""
import ctypes as C
import sys

import numpy as np
import pytest
import torch

from tests import cartpole_ref as R


def test_philox_known_answers():
    h = lambda words: " ".join("%08x" % w for w in words)
    assert h(R.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert h(R.philox4x32_10((R.MASK,) * 4, (R.MASK,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert h(R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_reset_state_example_and_range():
    assert float(R.reset_state(1, 5, 3)[0]).hex() == "0x1.679239999999ap-5"
    s = R.reset_states(7, 11, 64)
    assert s.shape == (64, 4) and s.dtype == np.float64 and (s >= -0.05).all() and (s < 0.05).all()
    assert len({tuple(r) for r in s}) == 64                               # every env draws its own
    assert not np.array_equal(R.reset_state(7, 11, 0), R.reset_state(7, 11, 1))          # ... and every episode
    assert not np.array_equal(R.reset_state(7, 11, 0), R.reset_state(7 + (1 << 32), 11, 0))   # the seed's high word is in the key


def test_episode_rows_take_the_lowest_env_of_a_step():
    from aur_ppo_amd.envs import episode_rows, episode_triples
    tab = torch.tensor([[0, 0, 0, 0],
                        [0, 17, 0, 9],       # two envs finish: the lower index is logged
                        [0, 0, 0, 0],
                        [500, 0, 0, 0],
                        [0, 0, 0, 3]], dtype=torch.int32)
    assert episode_rows(tab).tolist() == [0, 17, 0, 500, 3]
    assert episode_triples(tab, 1000, 8) == [(17.0, 17, 1016), (500.0, 500, 1032), (3.0, 3, 1040)]
    assert episode_triples(torch.zeros((3, 2), dtype=torch.int32), 0, 2) == []
    one = torch.tensor([[5]], dtype=torch.int32)
    assert episode_triples(one, 0, 1) == [(5.0, 5, 1)]


class _Stub:
    def __init__(self, num_envs, device, seed=0):
        self.args = (num_envs, str(device), seed)


def test_make_vec_env_switch(monkeypatch):
    from aur_ppo_amd import envs
    monkeypatch.setitem(sys.modules, "gym", None)           # `import gym` raises ImportError: the built-in classes are what is left
    monkeypatch.setattr(envs, "CartPoleDeviceVecEnv", _Stub)
    monkeypatch.delenv("AURPPO_DEVICE_ENV", raising=False)
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cuda", {})) is envs.CartPoleVecEnv           # unset: nothing changes
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cuda", {"device_env": False})) is envs.CartPoleVecEnv
    e = envs.make_vec_env("CartPole-v1", 3, False, "cuda", {"device_env": True, "env_seed": 9})
    assert type(e) is _Stub and e.args == (3, "cuda", 9)
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cpu", {"device_env": True})) is envs.CartPoleVecEnv     # a CUDA device only
    assert type(envs.make_vec_env("Synthetic-v0", 3, False, "cpu", {"device_env": True})) is envs.SyntheticVecEnv
    monkeypatch.setenv("AURPPO_DEVICE_ENV", "1")
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cuda", {})) is _Stub
    monkeypatch.setenv("AURPPO_DEVICE_ENV", "0")
    assert type(envs.make_vec_env("CartPole-v1", 3, False, "cuda", {})) is envs.CartPoleVecEnv


def test_cpu_device_is_refused():
    from aur_ppo_amd.envs import CartPoleDeviceVecEnv
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CartPoleDeviceVecEnv(4, "cpu")
    assert CartPoleDeviceVecEnv.device_native and CartPoleDeviceVecEnv.capturable


def test_reset_refuses_a_seed_list_that_is_not_consecutive():
    from aur_ppo_amd.envs import CartPoleDeviceVecEnv
    env = CartPoleDeviceVecEnv.__new__(CartPoleDeviceVecEnv)        # no device here: reset() must refuse before it needs one
    env.num_envs = 4
    for seeds in ([0, 1, 3, 4], [3, 2, 1, 0], [0, 1, 2], [-1, 0, 1, 2]):
        with pytest.raises(ValueError, match="consecutive"):
            env.reset(seed=seeds)


def _env_state(n, **over):
    st = dict(state=torch.zeros((n, 4), dtype=torch.float64), steps=torch.zeros(n, dtype=torch.int32),
              episode=torch.zeros(n, dtype=torch.int32), seed=0, env0=0, consts=(9.8, 1.0, 0.1, 0.5, 10.0, 0.02, 0.2, 2.4, 500))
    st.update(over)
    return st


def _rollout_args(T, N):
    f = lambda *s: torch.zeros(s)
    return dict(noise=f(T, N), states=f(T, N, 4), terminals=f(T, N), actions=f(T, N), log_probs=f(T, N), values=f(T, N),
                rewards=f(T, N), ep_len=torch.zeros((T, N), dtype=torch.int32), next_obs=f(N, 4), next_done=f(N))


LAYOUT = dict(offsets=list(range(13)), n_params=100, D=4, A=2, continuous=False, hidden=64, num_layers=2, wide=False)


def test_value_errors_come_before_the_library():
    """Wrong shapes and dtypes raise ValueError on a box without a GPU too: the checks run before the library is asked for."""
    from aur_ppo_amd import hip_ops as H
    with pytest.raises(ValueError, match="state"):
        H.cartpole_reset(_env_state(3, state=torch.zeros((3, 4))), torch.zeros((3, 4)))              # fp32 state
    with pytest.raises(ValueError, match="episode"):
        H.cartpole_reset(_env_state(3, episode=torch.zeros(3, dtype=torch.int64)), torch.zeros((3, 4)))
    with pytest.raises(ValueError, match="obs"):
        H.cartpole_reset(_env_state(3), torch.zeros((3, 3)))
    with pytest.raises(ValueError, match="consts"):
        H.cartpole_reset(_env_state(3, consts=(1.0,)), torch.zeros((3, 4)))
    ok = dict(action=torch.zeros(3), obs=torch.zeros((3, 4)), reward=torch.zeros(3), done=torch.zeros(3),
              ep_len=torch.zeros(3, dtype=torch.int32))
    for name, bad in (("action", torch.zeros(3, dtype=torch.int64)), ("obs", torch.zeros((4, 4))), ("reward", torch.zeros(2)),
                      ("done", torch.zeros((3, 1))), ("ep_len", torch.zeros(3))):
        with pytest.raises(ValueError, match=name):
            H.cartpole_step(_env_state(3), **dict(ok, **{name: bad}))
    flat = torch.zeros(128)
    for name, bad in (("noise", torch.zeros((5, 4))), ("states", torch.zeros((5, 3, 3))), ("actions", torch.zeros((5, 3, 1))),
                      ("ep_len", torch.zeros((5, 3))), ("next_obs", torch.zeros((3, 4), dtype=torch.float64)),
                      ("next_done", torch.zeros(4)), ("values", torch.zeros((5, 6))[:, ::2])):
        with pytest.raises(ValueError, match=name):
            H.cartpole_rollout(_env_state(3), flat, LAYOUT, **dict(_rollout_args(5, 3), **{name: bad}))
    with pytest.raises(ValueError, match="smaller than the policy"):
        H.cartpole_rollout(_env_state(3), torch.zeros(50), LAYOUT, **_rollout_args(5, 3))


def test_rollout_shape_rule():
    from aur_ppo_amd import hip_ops as H
    assert H.cartpole_rollout_ok(LAYOUT)
    assert not H.cartpole_rollout_ok(None)
    for change in (dict(wide=True), dict(A=3), dict(continuous=True), dict(D=5), dict(hidden=128), dict(num_layers=3), dict(layered=True)):
        assert not H.cartpole_rollout_ok(dict(LAYOUT, **change)), change


def test_library_refuses_before_any_launch():
    """The C entries' argument checks need no device: null pointers are EINVAL (-1), sizes and policy shapes ESHAPE (-2)."""
    import __graft_entry__ as g
    g.build()
    from aur_ppo_amd import _lib
    lib = _lib.load()
    consts = (9.8, 1.0, 0.1, 0.5, 10.0, 0.02, 0.2, 2.4, 500)
    assert lib.aurppo_cartpole_reset(None, None, None, None, 4, 0, 0, 0, None) == -1 and b"null pointer" in lib.aurppo_last_error()
    assert lib.aurppo_cartpole_step(*[None] * 8, 4, 0, 0, 0, *consts, None) == -1 and b"null pointer" in lib.aurppo_last_error()
    buf = (C.c_double * 64)()            # a host buffer: every check below returns before a pointer is followed on the device
    p = C.cast(buf, C.c_void_p)
    lay = (C.c_int * 13)(*range(13))

    def rollout(N=4, T=2, D=4, A=2, cont=0, hidden=64, layers=2, n_params=100, lay=lay, first=p):
        return lib.aurppo_cartpole_rollout_f32(first, p, p, p, p, p, N, T, D, A, cont, hidden, layers, p, lay, n_params, p, p, p, p, p, p, p,
                                               0, 0, 0, *consts, None)
    assert rollout(first=None) == -1 and b"null pointer" in lib.aurppo_last_error()
    assert rollout(N=0) == -2 and rollout(T=0) == -2
    assert rollout(hidden=128) == -2 and b"hidden_dim=128" in lib.aurppo_last_error()
    assert rollout(layers=3) == -2
    assert rollout(D=5) == -2 and rollout(A=3) == -2 and rollout(cont=1) == -2
    assert b"Categorical" in lib.aurppo_last_error()
    assert rollout(lay=(C.c_int * 13)(*([0] * 11 + [100, 0]))) == -2 and b"layout[11]=100" in lib.aurppo_last_error()
    assert lib.aurppo_cartpole_reset(p, p, p, p, 0, 0, 0, 0, None) == -2
    assert lib.aurppo_cartpole_reset(p, p, p, p, 4, -1, 0, 0, None) == -2
