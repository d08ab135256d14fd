"""End-to-end train() time per update on Pendulum-v1 (rollout + GAE + update), tools/bench_train_cartpole.py's method: the host env,
the device env stepped per step under the captured rollout, and the one-launch rollout (K18) -- alternated, ROUNDS rounds in one
process -- and K18's duration alone (HIP events).  Prints one JSON line per run and a summary; with OUT, appends them to that file.

    python tools/bench_train_pendulum.py [N=4096] [UPDATES=40] [ROUNDS=3] [OUT.jsonl]
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
OUT = sys.argv[4] if len(sys.argv) > 4 else None
T = 128
HP = dict(gym_id="Pendulum-v1", continuous=True, entropy_coeff=0.0, seed=1.0, num_steps=T, gae=True, anneal_lr=True, gae_lambda=0.95,
          num_update_epochs=4, num_envs=N, num_minibatches=4, value_coeff=0.5, clip_coeff=0.2, clip_vloss=True, max_grad_norm=0.5,
          target_kl=None, norm_adv=True, capture_video=False, hidden_dim=64, learning_rate=3e-4, exp_name="bench", num_layers=2,
          dropout=0.0, gamma=0.99, track=False, log=False, save=False)
MODES = {"host": dict(), "device_steps": dict(device_env=True), "one_launch": dict(device_env=True)}


def emit(record):
    line = json.dumps(record)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def run(mode, updates):
    """ms per update over the steady state: the first updates (eager warm-up, the graph captures) are outside the window."""
    os.environ["AURPPO_ROLLOUT_KERNEL"] = "0" if mode == "device_steps" else "1"
    agent = ppo(dict(HP, total_timesteps=T * N * updates, **MODES[mode]))
    if mode != "host":
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
    r = agent.total_returns
    emit(dict(mode=mode, N=N, T=T, steady_updates=n, ms_per_update=round(ms, 3), episodes=len(r),
              first_returns=round(sum(r[:10]) / max(len(r[:10]), 1), 1), last_returns=round(sum(r[-10:]) / max(len(r[-10:]), 1), 1)))
    return agent, ms


def time_k18(agent, reps=20):
    """K18 alone: HIP events around ``reps`` launches on the trained agent's own env and buffer."""
    env, b = agent.envs, agent.buffer
    noise = torch.randn((T, N, 1), device=agent.device)
    obs, done = env.reset()[0], torch.zeros(N, device=agent.device)
    tables = env.begin_rollout(T)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k in range(-3, reps):
        if k >= 0:
            ev[k][0].record()
        agent.ops.pendulum_rollout(env.native_state(), agent.bucket.flat_param, agent._mlp, noise, b.states, b.terminals, b.actions,
                                   b.log_probs, b.values, b.rewards, *tables, obs, done)
        if k >= 0:
            ev[k][1].record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(z) * 1e3 for a, z in ev)
    return dict(k18_us_median=round(us[len(us) // 2], 1), k18_us_min=round(us[0], 1), k18_us_max=round(us[-1], 1), reps=reps)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    ms = {m: [] for m in MODES}
    k18 = None
    for r in range(ROUNDS):
        for mode in MODES:
            agent, t = run(mode, max(U // 2, 12) if mode == "host" else U)
            ms[mode].append(t)
            if mode == "one_launch" and k18 is None:
                k18 = time_k18(agent)
                emit(k18)
            del agent
    emit(dict(summary={m: dict(ms_per_update=[round(x, 3) for x in v], median=round(sorted(v)[len(v) // 2], 3)) for m, v in ms.items()},
              k18=k18, N=N, T=T))
