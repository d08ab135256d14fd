"""One rollout step of a layered MLP policy at hidden widths that are no multiple of 32 -- 2 x 200 and 2 x 400 through the ``anyh``
entries (``mlp_layered_layout(..., any_hidden=True)``) -- next to their aligned neighbours 2 x 224 and 2 x 416 through the entries that
were there before: the price of the padding.  N = 4096, D 64, A 6, Gaussian head.  Per width three arms: the torch-modules route
(``policy.evaluate`` under no_grad + the three row stores), ``hip_ops.mlp_layered_act`` from copies prepared once, and its paired route.
tools/bench_layered_act.py's alternation: all arms of all widths in one process, ROUNDS rounds of one batch of STEPS steps per arm between
device events, after a warm-up; every batch's time is kept so the spread shows.  All eager, host included.  Prints one JSON object
(``profiles/layered_hidden_bench.json`` holds one, beside the update's figures from bench.py); run on the GPU box:
    python tools/bench_layered_hidden.py > layered_hidden_act.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aur_ppo_amd import hip_ops as H                       # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic         # noqa: E402
from aur_ppo_amd.flat import FlatBucket                   # noqa: E402

N, D, A, LAYERS, STEPS, ROUNDS, WARMUP = 4096, 64, 6, 2, 400, 7, 100
WIDTHS = (200, 224, 400, 416)


def batch(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS * 1e3


def arms_of(hidden):
    torch.manual_seed(0)
    pol = actor_critic(D, (A,), hidden, LAYERS, 0.0, True).cuda()
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layered_layout(pol, bucket, any_hidden=True)
    assert lay is not None and bool(lay.get("ragged_hidden")) == (hidden % 32 != 0)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(N, D, device="cuda", generator=g)
    noise = torch.randn(N, A, device="cuda", generator=g)
    actions, logp, value = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    wop = H.mlp_layered_prepare(bucket.flat_param, lay)

    def torch_route():
        with torch.no_grad():
            a, lp, _, v = pol.evaluate(obs)
            value.copy_(v.flatten())
        actions.copy_(a)
        logp.copy_(lp)

    return {f"{hidden}/torch_modules": torch_route,
            f"{hidden}/layered_act_prepared": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop),
            f"{hidden}/layered_act_paired": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop,
                                                                     paired=True)}


def main():
    arms = {}
    for hidden in WIDTHS:
        arms.update(arms_of(hidden))
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            times[k].append(round(batch(fn), 2))
    rows = {}
    for k, ts in times.items():
        s = sorted(ts)
        rows[k] = dict(us_per_step=ts, median=s[len(s) // 2], min=s[0], max=s[-1])
        print(k, rows[k], file=sys.stderr, flush=True)
    print(json.dumps(dict(N=N, D=D, A=A, layers=LAYERS, steps_per_batch=STEPS, rounds=ROUNDS, warmup_steps=WARMUP, rows=rows,
                          note="us per rollout step, eager, host included; one batch per arm and round, arms alternating; 200 and 400 "
                               "through the anyh entries, 224 and 416 through the entries of the aligned widths"), indent=1))


if __name__ == "__main__":
    main()
