"""Vector environments for the trainer.  The reference steps ``gym.vector.SyncVectorEnv`` on the
host every rollout step (src/ppo.py:66-68,110); gym is not part of this image, and the BASELINE
metric is defined on synthetic rollout tensors, so these built-ins are provided behind the same
``reset(seed=) -> (obs, info)`` / ``step(a) -> (obs, rew, done, trunc, info)`` interface:

* ``SyntheticVecEnv`` -- device-resident N(0,1) observations / rewards, Bernoulli terminals
  (SURVEY section 8d); ``device_native = True`` tells the trainer to skip the host round trip.
* ``CartPoleVecEnv``  -- CartPole-v1 dynamics (Barto-Sutton-Anderson cart-pole as in gym's
  classic_control: Euler, tau 0.02, 12 deg / 2.4 m limits, 500-step truncation) with auto-reset
  and ``final_info`` episode statistics, for the plumbing config.
* ``CartPoleDeviceVecEnv`` -- the same env as a HIP kernel on state kept on the device (csrc/cartpole.hip), opt-in
  (``params["device_env"]`` / AURPPO_DEVICE_ENV=1): ``device_native`` and ``capturable``, and with the default
  2 x 64 policy the trainer runs a whole rollout on it as one launch (``hip_ops.cartpole_rollout``).
* ``PendulumVecEnv`` -- Pendulum-v1 (gym 0.26.2's classic_control pendulum) behind the reference's continuous wrapper chain
  (ClipAction, NormalizeObservation, clip +-10, NormalizeReward, clip +-10; src/ppo.py:85-99), per env, in fp64.
* ``PendulumDeviceVecEnv`` -- the same env as HIP kernels (csrc/pendulum.hip) behind the device CartPole's switches; with the default
  2 x 64 Gaussian policy the trainer runs a whole rollout on it as one launch (``hip_ops.pendulum_rollout``).
"""
from __future__ import annotations

import math
import os
import types

import numpy as np
import torch


class _Space:
    def __init__(self, shape, n=None):
        self.shape = tuple(shape)
        self.n = n


class SyntheticVecEnv:
    device_native = True
    capturable = True          # step() is a fixed sequence of device ops: a whole rollout can be captured as one hipGraph

    def __init__(self, num_envs, obs_dim, act_dim, continuous, device, seed=1234, p_done=0.02):
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.p_done = p_done
        self.obs_shape = tuple(obs_dim) if isinstance(obs_dim, (tuple, list)) else (int(obs_dim),)
        self.single_observation_space = _Space(self.obs_shape)
        self.single_action_space = _Space((int(act_dim),)) if continuous else _Space((), int(act_dim))
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def _obs(self):
        return torch.randn((self.num_envs,) + self.obs_shape, device=self.device, generator=self.gen)

    def reset(self, seed=None):
        return self._obs(), {}

    def step(self, action):
        rew = torch.randn(self.num_envs, device=self.device, generator=self.gen)
        done = (torch.rand(self.num_envs, device=self.device, generator=self.gen) < self.p_done).float()
        return self._obs(), rew, done, None, {}

    def generators(self):
        """Generators step() draws from (a graph capture has to know them)."""
        return [self.gen]

    def close(self):
        pass


class CartPoleVecEnv:
    device_native = False
    gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
    theta_lim, x_lim, max_steps = 12 * 2 * math.pi / 360, 2.4, 500

    def __init__(self, num_envs, seed=0):
        self.num_envs = num_envs
        self.single_observation_space = _Space((4,))
        self.single_action_space = _Space((), 2)
        self.rs = [np.random.RandomState(seed + i) for i in range(num_envs)]
        self.state = np.zeros((num_envs, 4), np.float64)
        self.steps = np.zeros(num_envs, np.int64)
        self.ret = np.zeros(num_envs, np.float64)

    def _reset_one(self, i):
        self.state[i] = self.rs[i].uniform(-0.05, 0.05, size=4)
        self.steps[i] = 0
        self.ret[i] = 0.0

    def reset(self, seed=None):
        if seed is not None:
            seeds = seed if isinstance(seed, (list, tuple)) else [seed + i for i in range(self.num_envs)]
            self.rs = [np.random.RandomState(int(s)) for s in seeds]
        for i in range(self.num_envs):
            self._reset_one(i)
        return self.state.astype(np.float32), {}

    def step(self, action):
        a = np.asarray(action).reshape(-1)
        x, xd, th, thd = self.state.T
        force = np.where(a == 1, self.force_mag, -self.force_mag)
        ct, st = np.cos(th), np.sin(th)
        total_mass = self.masscart + self.masspole
        pml = self.masspole * self.length
        temp = (force + pml * thd * thd * st) / total_mass
        thacc = (self.gravity * st - ct * temp) / (self.length * (4.0 / 3.0 - self.masspole * ct * ct / total_mass))
        xacc = temp - pml * thacc * ct / total_mass
        self.state = np.stack([x + self.tau * xd, xd + self.tau * xacc, th + self.tau * thd, thd + self.tau * thacc], 1)
        self.steps += 1
        self.ret += 1.0
        term = (np.abs(self.state[:, 0]) > self.x_lim) | (np.abs(self.state[:, 2]) > self.theta_lim)
        trunc = self.steps >= self.max_steps
        done = term | trunc
        info = {}
        if done.any():
            finals = [None] * self.num_envs
            for i in np.nonzero(done)[0]:
                finals[i] = {"episode": {"r": float(self.ret[i]), "l": int(self.steps[i])}}
                self._reset_one(i)
            info["final_info"] = finals
        return self.state.astype(np.float32), np.ones(self.num_envs, np.float32), term | trunc, trunc, info

    def close(self):
        pass


def _rms_update(mean, var, count, x):
    """One ``RunningMeanStd.update`` of gym 0.26.2 with a batch of one (``batch_var = 0``, ``batch_count = 1``), per env: ``count`` is
    (N,), ``mean`` / ``var`` / ``x`` are (N,) or (N, k).  Returns the new (mean, var, count)."""
    cnt = count if mean.ndim == 1 else count[:, None]
    delta = x - mean
    tot = cnt + 1
    new_mean = mean + delta / tot
    M2 = var * cnt + delta ** 2 * cnt / tot
    return new_mean, M2 / tot, count + 1


class PendulumVecEnv:
    """Pendulum-v1 (gym 0.26.2 ``classic_control/pendulum.py``) behind the reference's continuous wrapper chain (src/ppo.py:85-99), each
    wrapper per env as ``SyncVectorEnv`` over wrapped envs has it: RecordEpisodeStatistics on the raw rewards, ClipAction (which
    coincides with the env's own clip to +-max_torque), NormalizeObservation, clip +-10, NormalizeReward (its own gamma 0.99; the
    discounted return is cleared on a termination only, and Pendulum has none), clip +-10, with gym's auto-reset: on the step that
    ends an episode the observation statistics take the final observation, then the reset one, which is returned.  Everything is
    fp64; observations and rewards are handed out rounded to fp32.  ``reset()`` starts every env over, statistics included.
    This class is the definition ``PendulumDeviceVecEnv`` is held to.  It makes no claim on gym's float32 torque arithmetic (gym forms
    ``u`` and the cost in the action's float32 where numpy's promotion rules keep it there) or on gym's ``RandomState`` draws."""
    device_native = False
    g, m, l, dt, max_speed, max_torque, max_steps = 10.0, 1.0, 1.0, 0.05, 8.0, 2.0, 200
    norm_gamma, norm_eps, norm_clip, count0 = 0.99, 1e-8, 10.0, 1e-4      # the wrappers' constants (gym 0.26.2's defaults, src/ppo.py's clips)

    def __init__(self, num_envs, seed=0):
        self.num_envs = num_envs
        self.single_observation_space = _Space((3,))
        self.single_action_space = _Space((1,))
        self.rs = [np.random.RandomState(seed + i) for i in range(num_envs)]
        self.th = np.zeros(num_envs, np.float64)
        self.thdot = np.zeros(num_envs, np.float64)
        self.steps = np.zeros(num_envs, np.int64)
        self.reset()

    @staticmethod
    def angle_normalize(x):
        return ((x + np.pi) % (2 * np.pi)) - np.pi

    def _raw_obs(self):
        """[cos th, sin th, thdot] rounded to fp32, (N, 3)."""
        return np.stack([np.cos(self.th), np.sin(self.th), self.thdot], 1).astype(np.float32)

    def _take_obs(self, raw, rows=None):
        """The observation statistics of ``rows`` (default: every env) take the raw fp32 observation, promoted to fp64."""
        r = slice(None) if rows is None else rows
        self.obs_mean[r], self.obs_var[r], self.obs_count[r] = _rms_update(self.obs_mean[r], self.obs_var[r], self.obs_count[r],
                                                                          raw[r].astype(np.float64))

    def _norm_obs(self, raw):
        z = (raw.astype(np.float64) - self.obs_mean) / np.sqrt(self.obs_var + self.norm_eps)
        return np.clip(z, -self.norm_clip, self.norm_clip).astype(np.float32)

    def _reset_one(self, i):
        self.th[i] = self.rs[i].uniform(-np.pi, np.pi)
        self.thdot[i] = self.rs[i].uniform(-1.0, 1.0)
        self.steps[i] = 0
        self.ep_ret[i] = 0.0

    def reset(self, seed=None):
        if seed is not None:
            seeds = seed if isinstance(seed, (list, tuple)) else [seed + i for i in range(self.num_envs)]
            self.rs = [np.random.RandomState(int(s)) for s in seeds]
        n = self.num_envs
        self.obs_mean, self.obs_var = np.zeros((n, 3), np.float64), np.ones((n, 3), np.float64)
        self.obs_count = np.full(n, self.count0, np.float64)
        self.ret_mean, self.ret_var, self.ret_count = np.zeros(n, np.float64), np.ones(n, np.float64), np.full(n, self.count0, np.float64)
        self.ret = np.zeros(n, np.float64)           # NormalizeReward's discounted return
        self.ep_ret = np.zeros(n, np.float64)        # RecordEpisodeStatistics' raw return
        for i in range(n):
            self._reset_one(i)
        raw = self._raw_obs()
        self._take_obs(raw)
        return self._norm_obs(raw), {}

    def step(self, action):
        a = np.asarray(action).reshape(self.num_envs, -1)
        th, thdot = self.th, self.thdot
        u = np.clip(a[:, 0].astype(np.float64), -self.max_torque, self.max_torque)     # the buffer keeps the unclipped sample
        cost = self.angle_normalize(th) ** 2 + 0.1 * thdot ** 2 + 0.001 * u ** 2
        thdot = np.clip(thdot + (3 * self.g / (2 * self.l) * np.sin(th) + 3.0 / (self.m * self.l ** 2) * u) * self.dt,
                        -self.max_speed, self.max_speed)
        self.th = th + thdot * self.dt
        self.thdot = thdot
        r = -cost
        self.steps += 1
        self.ep_ret += r
        trunc = self.steps >= self.max_steps
        raw = self._raw_obs()
        self._take_obs(raw)                          # the final observation where an episode ends
        info = {}
        if trunc.any():
            finals = [None] * self.num_envs
            rows = np.nonzero(trunc)[0]
            for i in rows:
                finals[i] = {"episode": {"r": float(self.ep_ret[i]), "l": int(self.steps[i])}}
                self._reset_one(i)
            info["final_info"] = finals
            raw = self._raw_obs()
            self._take_obs(raw, rows)                # ... and the reset one behind it: gym's auto-reset
        obs = self._norm_obs(raw)
        self.ret = self.ret * self.norm_gamma + r    # not cleared at a truncation (0.26.2 clears on `terminated` only)
        self.ret_mean, self.ret_var, self.ret_count = _rms_update(self.ret_mean, self.ret_var, self.ret_count, self.ret)
        reward = np.clip(r / np.sqrt(self.ret_var + self.norm_eps), -self.norm_clip, self.norm_clip).astype(np.float32)
        return obs, reward, trunc.copy(), trunc, info

    STATE_KEYS = ("th", "thdot", "steps", "obs_mean", "obs_var", "obs_count", "ret_mean", "ret_var", "ret_count", "ret", "ep_ret")

    def get_state(self):
        """A dict of copies: th, thdot, steps, both sets of statistics, the reward wrapper's return ``ret`` and the raw ``ep_ret``."""
        return {k: np.array(getattr(self, k)) for k in self.STATE_KEYS}

    def set_state(self, **state):
        """Overwrite any of ``get_state()``'s entries (each (N,), the observation mean / var (N, 3)); returns the observation the
        statistics as they stand make of the state (the statistics do not take it)."""
        for k, v in state.items():
            if k not in self.STATE_KEYS:
                raise ValueError(f"PendulumVecEnv.set_state: no entry named {k!r}")
            cur = getattr(self, k)
            new = np.array(v, dtype=cur.dtype)
            if new.shape != cur.shape:
                raise ValueError(f"PendulumVecEnv.set_state: {k} must have shape {cur.shape}")
            setattr(self, k, new)
        return self._norm_obs(self._raw_obs())

    def close(self):
        pass


def _take_seed(env, seed):
    """A device env's ``reset(seed=)``: an int becomes the key of every draw from here on; the trainer's list of consecutive per-env
    seeds gives the global index of env 0 (its first entry); None changes nothing."""
    if isinstance(seed, (list, tuple)):
        seeds = [int(s) for s in seed]
        if len(seeds) != env.num_envs or any(b - a != 1 for a, b in zip(seeds, seeds[1:])) or seeds[0] < 0:
            raise ValueError(f"{type(env).__name__}.reset: a seed list must hold num_envs consecutive non-negative integers")
        env.env0 = seeds[0]
    elif seed is not None:
        env.seed = int(seed)


class CartPoleDeviceVecEnv:
    """``CartPoleVecEnv`` on the device (csrc/cartpole.hip): the same dynamics, limits, 500-step truncation and auto-reset in fp64,
    one thread per env, behind the same ``reset`` / ``step`` interface.  What differs: resets draw from Philox4x32-10 on (seed, global
    env index, episode number) instead of numpy's ``RandomState`` (so a reset does not depend on how a rollout is cut into launches),
    and finished episodes are not reported through ``info`` but as rows of an int32 table -- ``begin_rollout(T)`` opens a (T, N)
    table, every ``step()`` fills its next row with the lengths of the episodes that ended in it (0 elsewhere; CartPole's return is
    its length), ``episode_triples`` reads it once per rollout.  There is no CPU fallback."""
    device_native = True
    capturable = True          # step() is one kernel launch into rows fixed at capture time
    takes_float_actions = True  # step() reads K8's fp32 0.0 / 1.0 action row as it is
    rollout_op = "cartpole_rollout"     # the ``ops`` call that runs a whole rollout on this env in one launch; its shape rule: + "_ok"

    def __init__(self, num_envs, device, seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("CartPoleDeviceVecEnv needs a gfx950 GPU: the env's HIP kernels have no CPU fallback")
        self.num_envs = int(num_envs)
        self.single_observation_space = _Space((4,))
        self.single_action_space = _Space((), 2)
        self.seed, self.env0 = int(seed), 0
        self.state = torch.zeros((self.num_envs, 4), dtype=torch.float64, device=self.device)
        self.steps = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.ep_len = None         # (T, N) int32, see begin_rollout
        self._row = 0
        self._spare_row = None     # where a step() outside a rollout's table leaves its lengths
        self.reset()

    def native_state(self):
        """What the ``hip_ops.cartpole_*`` calls take as ``env_state``."""
        C = CartPoleVecEnv
        return dict(state=self.state, steps=self.steps, episode=self.episode, seed=self.seed, env0=self.env0,
                    consts=(C.gravity, C.masscart, C.masspole, C.length, C.force_mag, C.tau, C.theta_lim, C.x_lim, C.max_steps))

    def generators(self):
        return []

    def reset(self, seed=None):
        """``seed``: an int (the key of every draw from here on), or the trainer's list of consecutive per-env seeds, whose first
        becomes the global index of env 0 (a rank's shard then draws what the same envs draw in a single process)."""
        _take_seed(self, seed)
        from . import hip_ops
        obs = torch.empty((self.num_envs, 4), dtype=torch.float32, device=self.device)
        hip_ops.cartpole_reset(self.native_state(), obs)
        return obs, {}

    def begin_rollout(self, num_steps, clear=True):
        """Open the (num_steps, N) episode-length table (allocated once per size) and point the next ``step()`` at its row 0."""
        if self.ep_len is None or tuple(self.ep_len.shape) != (int(num_steps), self.num_envs):
            self.ep_len = torch.zeros((int(num_steps), self.num_envs), dtype=torch.int32, device=self.device)
        elif clear:
            self.ep_len.zero_()
        self._row = 0
        return self.ep_len

    def episode_tables(self):
        """(ep_len, ep_ret) of the open rollout; ep_ret None: an episode's return is its length."""
        return self.ep_len, None

    def step(self, action):
        from . import hip_ops
        a = action.to(self.device).reshape(-1)
        if a.dtype != torch.float32:
            a = a.float()
        if self.ep_len is not None and self._row < self.ep_len.shape[0]:
            row = self.ep_len[self._row]
            self._row += 1
        else:
            if self._spare_row is None:
                self._spare_row = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            row = self._spare_row
        obs = torch.empty((self.num_envs, 4), dtype=torch.float32, device=self.device)
        reward = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        done = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        hip_ops.cartpole_step(self.native_state(), a.contiguous(), obs, reward, done, row)
        return obs, reward, done, None, {}

    def set_state(self, state64, steps):
        """Overwrite every env's state (N, 4) and step count (N,), for tests and checkpoints; returns the observation."""
        st = torch.as_tensor(np.asarray(state64.cpu() if isinstance(state64, torch.Tensor) else state64), dtype=torch.float64)
        sp = torch.as_tensor(np.asarray(steps.cpu() if isinstance(steps, torch.Tensor) else steps)).to(torch.int32)
        if tuple(st.shape) != (self.num_envs, 4) or tuple(sp.shape) != (self.num_envs,):
            raise ValueError("CartPoleDeviceVecEnv.set_state: state must be (num_envs, 4) and steps (num_envs,)")
        self.state.copy_(st)
        self.steps.copy_(sp)
        return self.state.float()

    def get_state(self):
        """(state (N, 4) float64, steps (N,), episode (N,)) as numpy arrays."""
        return self.state.cpu().numpy(), self.steps.cpu().numpy(), self.episode.cpu().numpy()

    def close(self):
        pass


class PendulumDeviceVecEnv:
    """``PendulumVecEnv`` on the device (csrc/pendulum.hip): the same core step, wrapper arithmetic, 200-step truncation and auto-reset
    in fp64, one thread per env, behind the same ``reset`` / ``step`` interface.  What differs is what differs between the CartPole
    classes: resets draw from Philox4x32-10 on (seed, global env index, episode number) -- counter (env0 + n, episode, 1, 0) --
    instead of numpy's ``RandomState``, and finished episodes are rows of two tables, ``ep_len`` (T, N) int32 and ``ep_ret`` (T, N)
    fp32 (the raw return, meaningful where ``ep_len > 0``), opened by ``begin_rollout(T)`` and read once per rollout by
    ``episode_triples``.  The state is one (N, 16) float64 block (its row layout: include/aurppo.h, ``ROW`` below) plus int32 ``steps``
    / ``episode``.  There is no CPU fallback."""
    device_native = True
    capturable = True          # step() is one kernel launch into rows fixed at capture time
    rollout_op = "pendulum_rollout"
    # the state block's row: name -> (first column, width)
    ROW = dict(th=(0, 1), thdot=(1, 1), obs_mean=(2, 3), obs_var=(5, 3), obs_count=(8, 1), ret_mean=(9, 1), ret_var=(10, 1),
               ret_count=(11, 1), ret=(12, 1), ep_ret=(13, 1))

    def __init__(self, num_envs, device, seed=0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("PendulumDeviceVecEnv needs a gfx950 GPU: the env's HIP kernels have no CPU fallback")
        self.num_envs = int(num_envs)
        self.single_observation_space = _Space((3,))
        self.single_action_space = _Space((1,))
        self.seed, self.env0 = int(seed), 0
        self.state = torch.zeros((self.num_envs, 16), dtype=torch.float64, device=self.device)
        self.steps = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.episode = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        self.ep_len = None         # (T, N) int32, see begin_rollout
        self.ep_ret = None         # (T, N) float32
        self._row = 0
        self._spare_rows = None    # where a step() outside a rollout's tables leaves its length and return
        self.reset()

    def native_state(self):
        """What the ``hip_ops.pendulum_*`` calls take as ``env_state``."""
        P = PendulumVecEnv
        return dict(state=self.state, steps=self.steps, episode=self.episode, seed=self.seed, env0=self.env0,
                    consts=(P.g, P.m, P.l, P.dt, P.max_speed, P.max_torque, P.max_steps))

    def generators(self):
        return []

    def reset(self, seed=None):
        """``seed``: as ``CartPoleDeviceVecEnv.reset`` takes it -- an int (the key of every draw from here on), or the trainer's list of
        consecutive per-env seeds, whose first becomes the global index of env 0.  Every env starts over, statistics included."""
        _take_seed(self, seed)
        from . import hip_ops
        obs = torch.empty((self.num_envs, 3), dtype=torch.float32, device=self.device)
        hip_ops.pendulum_reset(self.native_state(), obs)
        return obs, {}

    def begin_rollout(self, num_steps, clear=True):
        """Open the (num_steps, N) episode tables (allocated once per size) and point the next ``step()`` at their row 0; returns
        ``(ep_len, ep_ret)``."""
        if self.ep_len is None or tuple(self.ep_len.shape) != (int(num_steps), self.num_envs):
            self.ep_len = torch.zeros((int(num_steps), self.num_envs), dtype=torch.int32, device=self.device)
            self.ep_ret = torch.zeros((int(num_steps), self.num_envs), dtype=torch.float32, device=self.device)
        elif clear:
            self.ep_len.zero_()
            self.ep_ret.zero_()
        self._row = 0
        return self.ep_len, self.ep_ret

    def episode_tables(self):
        """(ep_len, ep_ret) of the open rollout."""
        return self.ep_len, self.ep_ret

    def step(self, action):
        from . import hip_ops
        a = action.to(self.device).reshape(-1)
        if a.dtype != torch.float32:
            a = a.float()
        if self.ep_len is not None and self._row < self.ep_len.shape[0]:
            rows = self.ep_len[self._row], self.ep_ret[self._row]
            self._row += 1
        else:
            if self._spare_rows is None:
                self._spare_rows = (torch.zeros(self.num_envs, dtype=torch.int32, device=self.device),
                                    torch.zeros(self.num_envs, dtype=torch.float32, device=self.device))
            rows = self._spare_rows
        obs = torch.empty((self.num_envs, 3), dtype=torch.float32, device=self.device)
        reward = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        done = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        hip_ops.pendulum_step(self.native_state(), a.contiguous(), obs, reward, done, *rows)
        return obs, reward, done, None, {}

    def set_state(self, **state):
        """Overwrite any of ``PendulumVecEnv.get_state()``'s entries (and ``episode``), for tests and checkpoints; returns the
        observation the statistics as they stand make of the state, computed by the host class's expressions (fp32, on the device)."""
        block = self.state.cpu().numpy()
        for k, v in state.items():
            v = np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
            if k in ("steps", "episode"):
                if v.shape != (self.num_envs,):
                    raise ValueError(f"PendulumDeviceVecEnv.set_state: {k} must be (num_envs,)")
                getattr(self, k).copy_(torch.as_tensor(v.astype(np.int32)))
            elif k in self.ROW:
                c0, w = self.ROW[k]
                if v.shape != ((self.num_envs,) if w == 1 else (self.num_envs, w)):
                    raise ValueError(f"PendulumDeviceVecEnv.set_state: {k} must be (num_envs{'' if w == 1 else ', %d' % w})")
                block[:, c0:c0 + w] = v.reshape(self.num_envs, w)
            else:
                raise ValueError(f"PendulumDeviceVecEnv.set_state: no entry named {k!r}")
        self.state.copy_(torch.as_tensor(block))
        th, thdot = block[:, 0], block[:, 1]
        raw = np.stack([np.cos(th), np.sin(th), thdot], 1).astype(np.float32).astype(np.float64)
        z = (raw - block[:, 2:5]) / np.sqrt(block[:, 5:8] + PendulumVecEnv.norm_eps)
        return torch.as_tensor(np.clip(z, -PendulumVecEnv.norm_clip, PendulumVecEnv.norm_clip).astype(np.float32)).to(self.device)

    def get_state(self):
        """``PendulumVecEnv.get_state()``'s dict (numpy; ``steps`` int32) plus ``episode``."""
        block = self.state.cpu().numpy()
        out = {k: (block[:, c0].copy() if w == 1 else block[:, c0:c0 + w].copy()) for k, (c0, w) in self.ROW.items()}
        out["steps"], out["episode"] = self.steps.cpu().numpy(), self.episode.cpu().numpy()
        return out

    def close(self):
        pass


def episode_rows(ep_len):
    """Per row t of an episode-length table (T, N): the length recorded by the LOWEST env index with ``ep_len > 0``, or 0 -- the
    reference logs the first finished env of a step and breaks (src/ppo.py:114-123).  Pure torch, any device; returns (T,) int64."""
    T, N = ep_len.shape
    cols = torch.arange(N, device=ep_len.device).expand(T, N)
    first = torch.where(ep_len > 0, cols, torch.full_like(cols, N)).min(dim=1).values
    picked = ep_len.gather(1, first.clamp(max=N - 1).view(T, 1)).view(T).to(torch.int64)
    return torch.where(first < N, picked, torch.zeros_like(picked))


def episode_triples(ep_len, global_step, step_stride, ep_ret=None):
    """The ``(return, length, global_step)`` triples a rollout's table stands for, in step order: row t was filled at global step
    ``global_step + (t + 1) * step_stride``.  The return is the length (CartPole), or with ``ep_ret`` (T, N) the entry of the row's
    lowest finished env.  One host read."""
    if ep_ret is None:
        rows = episode_rows(ep_len).cpu().tolist()
        return [(float(l), int(l), int(global_step + (t + 1) * step_stride)) for t, l in enumerate(rows) if l > 0]
    T, N = ep_len.shape
    cols = torch.arange(N, device=ep_len.device).expand(T, N)
    first = torch.where(ep_len > 0, cols, torch.full_like(cols, N)).min(dim=1).values.clamp(max=N - 1).view(T, 1)
    both = torch.stack([ep_len.gather(1, first).view(T).to(torch.float64), ep_ret.gather(1, first).view(T).to(torch.float64)]).cpu().tolist()
    return [(float(r), int(l), int(global_step + (t + 1) * step_stride)) for t, (l, r) in enumerate(zip(*both)) if l > 0]


def device_env_wanted(params):
    """The opt-in switch of the device envs (CartPole, Pendulum): ``params["device_env"]`` or AURPPO_DEVICE_ENV=1."""
    return bool(params.get("device_env", False)) or os.environ.get("AURPPO_DEVICE_ENV", "0") not in ("", "0")


def make_vec_env(gym_id, num_envs, continuous, device, params):
    """Synthetic-* ids -> SyntheticVecEnv (obs_dim/act_dim from params, defaults 64/6 continuous,
    4/2 discrete); otherwise gym's SyncVectorEnv when gym is importable (same wrappers as
    src/ppo.py:85-99), else the built-in CartPole for 'CartPole-v1'.  With the device-env switch on
    (``device_env_wanted``) and a CUDA device, 'CartPole-v1' is ``CartPoleDeviceVecEnv``.  'Pendulum-v1' likewise: the built-in
    ``PendulumVecEnv`` (the continuous wrapper chain inside it) without gym, ``PendulumDeviceVecEnv`` with the switch."""
    if str(gym_id).lower().startswith("synthetic"):
        obs_dim = params.get("obs_dim", 64 if continuous else 4)
        act_dim = params.get("act_dim", 6 if continuous else 2)
        return SyntheticVecEnv(num_envs, obs_dim, act_dim, continuous, device,
                               seed=int(params.get("env_seed", 1234)) + int(params.get("rank", 0)))
    if gym_id == "CartPole-v1" and device_env_wanted(params) and torch.device(device).type == "cuda":
        return CartPoleDeviceVecEnv(num_envs, device, seed=int(params.get("env_seed", 0)))
    if gym_id == "Pendulum-v1" and device_env_wanted(params) and torch.device(device).type == "cuda":
        return PendulumDeviceVecEnv(num_envs, device, seed=int(params.get("env_seed", 0)))
    try:
        import gym  # noqa: F401
    except ImportError:
        gym = None
    if gym is not None:
        def thunk():
            env = gym.make(gym_id)
            env = gym.wrappers.RecordEpisodeStatistics(env)
            if continuous:
                env = gym.wrappers.ClipAction(env)
                env = gym.wrappers.NormalizeObservation(env)
                env = gym.wrappers.TransformObservation(env, lambda obs: np.clip(obs, -10, 10))
                env = gym.wrappers.NormalizeReward(env)
                env = gym.wrappers.TransformReward(env, lambda reward: np.clip(reward, -10, 10))
            return env
        return gym.vector.SyncVectorEnv([thunk for _ in range(num_envs)])
    if gym_id == "CartPole-v1":
        return CartPoleVecEnv(num_envs)
    if gym_id == "Pendulum-v1":
        return PendulumVecEnv(num_envs)
    raise RuntimeError(f"gym is not installed and no built-in environment is named {gym_id!r} "
                       "(built-ins: 'CartPole-v1', 'Pendulum-v1', 'Synthetic-v0')")


class SyntheticArmEnv:
    """Device-resident stand-in for BulletArm's ``EnvWrapper`` (src/utils/env_wrapper.py:7-59) with its
    interface: ``reset() -> (states, obs)``, ``step(actions, auto_reset=False) -> (states, obs, rewards,
    dones)``, ``getNextAction() -> plan (N, 5)``.  Observations are (N, C, H, W) heightmap-like images (C = 1 upstream),
    ``states`` the gripper open/closed flag.  Used when bulletarm is not installed (it is not part of
    this image) and for the synthetic image-observation configs of BASELINE.json."""
    device_native = True

    def __init__(self, num_envs, device, obs_size=128, seed=4321, p_done=0.02, p_reward=0.05, channels=1):
        self.num_envs, self.device, self.obs_size, self.channels = num_envs, torch.device(device), obs_size, channels
        self.p_done, self.p_reward = p_done, p_reward
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def _draw(self):
        n, dev, g = self.num_envs, self.device, self.gen
        states = (torch.rand(n, device=dev, generator=g) < 0.5).float()
        obs = torch.rand((n, self.channels, self.obs_size, self.obs_size), device=dev, generator=g)
        return states, obs

    def reset(self):
        return self._draw()

    def getNextAction(self):
        n, dev, g = self.num_envs, self.device, self.gen
        plan = torch.randn((n, 5), device=dev, generator=g) * torch.tensor([0.5, 0.02, 0.02, 0.02, 0.4], device=dev)
        plan[:, 0] = (plan[:, 0] > 0).float()
        return plan

    def step(self, actions, auto_reset=False):
        n, dev, g = self.num_envs, self.device, self.gen
        rewards = (torch.rand(n, device=dev, generator=g) < self.p_reward).float()
        dones = (torch.rand(n, device=dev, generator=g) < self.p_done).float()
        states, obs = self._draw()
        return states, obs, rewards, dones

    def close(self):
        pass


def make_arm_envs(gym_id, num_envs, device, params, seed_offset=0):
    """bulletarm's env_factory when importable (same config as src/robot_ppo.py:113-135), else the
    synthetic stand-in."""
    if not str(gym_id).lower().startswith("synthetic"):
        try:
            from bulletarm import env_factory
        except ImportError:
            env_factory = None
        if env_factory is not None:
            env_config = {"workspace": np.array([[0.25, 0.65], [-0.2, 0.2], [0.01, 0.25]]), "max_steps": 100,
                          "obs_size": 128, "fast_mode": True, "action_sequence": "pxyzr",
                          "render": params.get("render", False), "num_objects": 2, "random_orientation": True,
                          "robot": "kuka", "workspace_check": "point", "object_scale_range": (1, 1),
                          "hard_reset_freq": 100, "physics_mode": "fast", "view_type": "camera_center_xyz",
                          "obs_type": "pixel", "view_scale": 1.5, "transparent_bin": True}
            planner_config = {"random_orientation": True, "dpos": 0.02, "drot": 0.19634954084936207}
            return _BulletArmWrapper(env_factory.createEnvs(num_envs, gym_id, env_config, planner_config))
    return SyntheticArmEnv(num_envs, device, obs_size=int(params.get("obs_size", 128)),
                           seed=int(params.get("env_seed", 4321)) + seed_offset, channels=int(params.get("obs_channels", 1)))


class _BulletArmWrapper:
    """``EnvWrapper`` over a real bulletarm runner: numpy in, float tensors out."""
    device_native = False

    def __init__(self, envs):
        self.envs = envs

    def reset(self):
        states, _in_hands, obs = self.envs.reset()
        return torch.tensor(states).float(), torch.tensor(obs).float()

    def getNextAction(self):
        return torch.tensor(self.envs.getNextAction()).float()

    def step(self, actions, auto_reset=False):
        (states, _in_hands, obs), rewards, dones = self.envs.step(actions.cpu().numpy(), auto_reset)
        return (torch.tensor(states).float(), torch.tensor(obs).float(), torch.tensor(rewards).float(),
                torch.tensor(dones).float())

    def close(self):
        self.envs.close()
