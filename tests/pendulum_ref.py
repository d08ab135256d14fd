"""A plain-Python restatement of what the device Pendulum (csrc/pendulum.hip) draws at a reset and of one ``RunningMeanStd`` update,
shared by the host and GPU tests: Philox4x32-10 (tests/cartpole_ref.py's) on the counter (global env index, episode, 1, 0) under the
key (seed low word, seed high word).  Python floats are IEEE doubles, so ``reset_state`` is the device's value bit for bit."""
import math

import numpy as np

from tests.cartpole_ref import MASK, philox4x32_10


def reset_words(seed, genv, episode):
    return philox4x32_10((genv & MASK, episode & MASK, 1, 0), (seed & MASK, (seed >> 32) & MASK))


def reset_state(seed, genv, episode):
    """(th, thdot) of global env ``genv`` at the start of its episode ``episode``: th in [-pi, pi), thdot in [-1, 1)."""
    w = reset_words(seed, genv, episode)
    u0, u1 = (w[0] >> 8) * 2.0 ** -24, (w[1] >> 8) * 2.0 ** -24
    return -math.pi + 2 * math.pi * u0, -1.0 + 2 * u1


def reset_states(seed, env0, n, episodes=None):
    """(n, 2) float64: env ``env0 + i`` at episode ``episodes[i]`` (default 0)."""
    return np.array([reset_state(seed, env0 + i, 0 if episodes is None else int(episodes[i])) for i in range(n)], np.float64)


def rms_update(mean, var, count, x):
    """One RunningMeanStd.update of gym 0.26.2 with a batch of one (batch_var = 0, batch_count = 1): the new (mean, var, count)."""
    delta = x - mean
    tot = count + 1
    return mean + delta / tot, (var * count + delta ** 2 * count / tot) / tot, tot


def first_obs(th, thdot):
    """The normalised fp32 observation a reset hands out: fresh statistics (0, 1, 1e-4) take the raw fp32 observation once."""
    raw = np.array([math.cos(th), math.sin(th), thdot], np.float64).astype(np.float32).astype(np.float64)
    out, stats = [], []
    for x in raw:
        m, v, c = rms_update(0.0, 1.0, 1e-4, float(x))
        out.append(min(max((float(x) - m) / math.sqrt(v + 1e-8), -10.0), 10.0))
        stats.append((m, v, c))
    return np.array(out, np.float64).astype(np.float32), stats
