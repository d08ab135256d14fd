"""End-to-end train() time per update on CartPole-v1 (rollout + GAE + update), tools/bench_train.py's method: the host env, the device
env stepped per step under the captured rollout, and the one-launch rollout (K16) -- alternated, ROUNDS rounds in one process --
with the synthetic env's figure beside them and K16's duration alone (HIP events).  Prints one JSON line per run and a summary.

    python tools/bench_train_cartpole.py [N=4096] [UPDATES=40] [ROUNDS=3]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aur_ppo_amd.ppo import ppo

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
U = int(sys.argv[2]) if len(sys.argv) > 2 else 40
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
T = 128
HP = dict(seed=1.0, num_steps=T, gae=True, anneal_lr=True, gae_lambda=0.95, num_update_epochs=4, num_envs=N, num_minibatches=4,
          value_coeff=0.5, clip_coeff=0.2, clip_vloss=True, max_grad_norm=0.5, target_kl=None, norm_adv=True, capture_video=False,
          hidden_dim=64, learning_rate=2.5e-4, exp_name="bench", num_layers=2, dropout=0.0, gamma=0.99, track=False, log=False,
          save=False)
MODES = {
    "host": dict(gym_id="CartPole-v1", continuous=False, entropy_coeff=0.01),                                    # (a)
    "device_steps": dict(gym_id="CartPole-v1", continuous=False, entropy_coeff=0.01, device_env=True),           # (b)
    "one_launch": dict(gym_id="CartPole-v1", continuous=False, entropy_coeff=0.01, device_env=True),             # (c)
    "synthetic": dict(gym_id="Synthetic-v0", continuous=True, entropy_coeff=0.0, obs_dim=64, act_dim=6),         # bench_train.py's
}


def run(mode, updates):
    """ms per update over the steady state: the first updates (eager warm-up, the graph captures) are outside the window."""
    os.environ["AURPPO_ROLLOUT_KERNEL"] = "0" if mode == "device_steps" else "1"
    agent = ppo(dict(HP, total_timesteps=T * N * updates, **MODES[mode]))
    if mode in ("device_steps", "one_launch"):
        assert agent._one_launch_rollout() == (mode == "one_launch")
    marks, orig = [], agent._log_update

    def mark(*args, **kw):
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return orig(*args, **kw)
    agent._log_update = mark
    agent.train()
    torch.cuda.synchronize()
    skip = min(10, updates - 2)
    n = len(marks) - skip
    ms = (marks[-1] - marks[skip - 1]) / n * 1e3
    out = dict(mode=mode, N=N, T=T, steady_updates=n, ms_per_update=round(ms, 3), episodes=len(agent.total_returns))
    print(json.dumps(out), flush=True)
    return agent, ms


def time_k16(agent, reps=20):
    """K16 alone: HIP events around ``reps`` launches on the trained agent's own env and buffer."""
    env, b = agent.envs, agent.buffer
    noise = torch.rand((T, N), device=agent.device)
    obs, done = env.reset()[0], torch.zeros(N, device=agent.device)
    table = env.begin_rollout(T)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k in range(-3, reps):
        if k >= 0:
            ev[k][0].record()
        agent.ops.cartpole_rollout(env.native_state(), agent.bucket.flat_param, agent._mlp, noise, b.states, b.terminals, b.actions,
                                   b.log_probs, b.values, b.rewards, table, obs, done)
        if k >= 0:
            ev[k][1].record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(z) * 1e3 for a, z in ev)
    return dict(k16_us_median=round(us[len(us) // 2], 1), k16_us_min=round(us[0], 1), k16_us_max=round(us[-1], 1), reps=reps)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ms = {m: [] for m in MODES}
    k16 = None
    for r in range(ROUNDS):
        for mode in ("host", "device_steps", "one_launch", "synthetic"):
            agent, t = run(mode, max(U // 2, 12) if mode == "host" else U)
            ms[mode].append(t)
            if mode == "one_launch" and k16 is None:
                k16 = time_k16(agent)
                print(json.dumps(k16), flush=True)
            del agent
    print(json.dumps(dict(summary={m: dict(ms_per_update=[round(x, 3) for x in v], median=round(sorted(v)[len(v) // 2], 3))
                                   for m, v in ms.items()}, k16=k16, N=N, T=T)), flush=True)
