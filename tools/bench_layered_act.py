"""One rollout step of an MLP policy wider than the fused kernels at N = 4096 (D 64, A 6, Gaussian head; 2 x 256 and 3 x 256): the
torch-modules route (``policy.evaluate`` under no_grad + the three buffer row stores, what ``ppo.rewards_to_go`` does with
AURPPO_LAYERED_ACT=0) against ``hip_ops.mlp_layered_act`` with weights prepared once (a rollout) and prepared in every call, and against
its paired route (``paired=True``: the small-M products, both nets' layer in one launch; weights prepared once), all eager.
The arms run in the same process, alternating: ROUNDS rounds of one batch of STEPS steps per arm between device events, after a
warm-up; every batch's time is printed so the spread shows.  Prints one JSON object (``profiles/layered_act_bench.json`` and
``profiles/layered_act_paired_bench.json`` hold one each); run on the GPU box:
    python tools/bench_layered_act.py > layered_act_bench.json
Arm names as arguments keep those arms only (a kernel trace of two routes:
    rocprofv3 --kernel-trace --stats -- python tools/bench_layered_act.py layered_act_prepared layered_act_paired)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aur_ppo_amd import hip_ops as H                       # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic         # noqa: E402
from aur_ppo_amd.flat import FlatBucket                   # noqa: E402

N, D, A, STEPS, ROUNDS, WARMUP = 4096, 64, 6, 400, 7, 100


def batch(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def main(only=()):
    rows = []
    for hidden, layers in [(256, 2), (256, 3)]:
        torch.manual_seed(0)
        pol = actor_critic(D, (A,), hidden, layers, 0.0, True).cuda()
        bucket = FlatBucket(pol.parameters())
        lay = H.mlp_layered_layout(pol, bucket)
        g = torch.Generator(device="cuda").manual_seed(1)
        obs = torch.randn(N, D, device="cuda", generator=g)
        noise = torch.randn(N, A, device="cuda", generator=g)
        actions, logp, value = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
        wop = H.mlp_layered_prepare(bucket.flat_param, lay)

        def torch_route():
            # rewards_to_go's torch branch; evaluate() draws its own noise
            with torch.no_grad():
                a, lp, _, v = pol.evaluate(obs)
                value.copy_(v.flatten())
            actions.copy_(a)
            logp.copy_(lp)

        arms = {"torch_modules": torch_route,
                "layered_act_prepared": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop),
                "layered_act_unprepared": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value),
                "layered_act_paired": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop,
                                                                paired=True)}
        if only:
            arms = {k: fn for k, fn in arms.items() if k in only}
        for fn in arms.values():
            for _ in range(WARMUP):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(ROUNDS):
            for k, fn in arms.items():
                times[k].append(round(batch(fn), 2))
        row = dict(hidden=hidden, layers=layers, launches_prepared=2 * layers + 1, launches_unprepared=4 * layers + 1,
                   launches_paired=layers + 1)
        for k, ts in times.items():
            s = sorted(ts)
            row[k] = dict(us_per_step=ts, median=s[len(s) // 2], min=s[0], max=s[-1])
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
    print(json.dumps(dict(N=N, D=D, A=A, steps_per_batch=STEPS, rounds=ROUNDS, warmup_steps=WARMUP, rows=rows,
                          note="us per rollout step, eager, host included; one batch per arm and round, arms alternating"), indent=1))


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
