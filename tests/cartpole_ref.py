"""A plain-Python restatement of what the device CartPole (csrc/cartpole.hip) draws at a reset, shared by the host and GPU tests:
Philox4x32-10 on the counter (global env index, episode, 0, 0) under the key (seed low word, seed high word), and the state it
makes.  Python floats are IEEE doubles, so ``reset_state`` is the device's value bit for bit."""
import numpy as np

MASK = 0xFFFFFFFF
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def reset_state(seed, genv, episode):
    """The (4,) float64 state of global env ``genv`` at the start of its episode ``episode``."""
    words = philox4x32_10((genv & MASK, episode & MASK, 0, 0), (seed & MASK, (seed >> 32) & MASK))
    return np.array([-0.05 + 0.1 * ((w >> 8) * 2.0 ** -24) for w in words], np.float64)


def reset_states(seed, env0, n, episodes=None):
    """(n, 4): env ``env0 + i`` at episode ``episodes[i]`` (default 0)."""
    return np.stack([reset_state(seed, env0 + i, 0 if episodes is None else int(episodes[i])) for i in range(n)])
