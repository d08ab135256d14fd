"""The layered routes at action heads of 17 .. 32 outputs (``mlp_layered_layout(..., wide_actions=True)``, the library's ``wa`` entries:
K13 / K14's builds with 32-long per-action arrays) next to the 16-action head through the entries that were there before.
(1) K13 alone (``hip_ops.head_ppo``: statistics, the kernel, its fold) at H = 256, M = 131 072, gz written beside the activations, for
    A = 16 through the old entry, A = 16 through the ``wa`` entry (the same NA = 16 kernel), A = 17 and A = 32, Gaussian and Categorical
    head; each row carries the bytes the launch moves (the four (M, H) planes, the action rows, the records and the index), so a time can
    be held against the A = 16 time scaled by the byte ratio.
(2) One rollout step at N = 4096, 2 x 256 over D = 376 with A = 17 (Humanoid): the torch-modules route (``policy.evaluate`` under no_grad
    + the three row stores), ``hip_ops.mlp_layered_act`` from copies prepared once, and its paired route.
tools/bench_layered_hidden.py's alternation: all arms in one process, ROUNDS rounds of one batch of STEPS calls per arm between device
events, after a warm-up; every batch's time is kept so the spread shows.  All eager, host included.  Prints one JSON object
(``profiles/layered_actions_bench.json`` holds one, beside the update's figures from bench.py); run on the GPU box:
    python tools/bench_layered_actions.py > layered_actions.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aur_ppo_amd import hip_ops as H                       # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic         # noqa: E402
from aur_ppo_amd.flat import FlatBucket                   # noqa: E402

HEAD_M, HEAD_H, HEAD_STEPS = 131072, 256, 40
N, D, A, HIDDEN, LAYERS, ACT_STEPS = 4096, 376, 17, 256, 2, 400
ROUNDS, WARMUP = 7, 20


def batch(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def head_arms():
    """K13 on one pair of activation planes shared by every arm (read only: gz goes to a second pair)."""
    g = torch.Generator(device="cuda").manual_seed(1)
    M, Hd = HEAD_M, HEAD_H
    hA, hC = torch.tanh(torch.randn(M, Hd, device="cuda", generator=g)), torch.tanh(torch.randn(M, Hd, device="cuda", generator=g))
    gzA, gzC = torch.empty_like(hA), torch.empty_like(hC)
    rec = torch.stack([-20 + 0.2 * torch.randn(M, device="cuda", generator=g), torch.randn(M, device="cuda", generator=g),
                       torch.randn(M, device="cuda", generator=g), torch.randn(M, device="cuda", generator=g)], 1).contiguous()
    idx = torch.randperm(M, device="cuda", generator=g).to(torch.int32).contiguous()
    arms, info = {}, {}
    for cont in (True, False):
        for A_, wa in ((16, False), (16, True), (17, True), (32, True)):
            torch.manual_seed(0)
            pol = actor_critic(16, (A_,) if cont else A_, Hd, 1, 0.0, cont).cuda()
            bucket = FlatBucket(pol.parameters())
            seq, n, _D, _A, _cont, NL, _Hd = H._mlp_structure(pol, bucket, H.MLP_LAYERED_MAX_A)
            lay = dict(offsets=seq, n_params=n, D=16, A=A_, continuous=cont, hidden=Hd, num_layers=NL, layered=True)
            if wa:
                lay["wide_actions"] = True
            act = torch.randn(M, A_, device="cuda", generator=g) if cont else torch.randint(0, A_, (M,), device="cuda", generator=g).float()
            sc = torch.empty(H.N_SCALARS, device="cuda")
            name = f"k13/{'gauss' if cont else 'cat'}/A{A_}/{'wa' if wa else 'old'}_entry"
            arms[name] = (lambda act=act, lay=lay, bucket=bucket, sc=sc: H.head_ppo(
                hA, hC, act, rec, idx, bucket.flat_param, lay, bucket.flat_grad, 0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED, sc, gzA=gzA, gzC=gzC))
            info[name] = dict(bytes_moved=4 * M * Hd * 4 + act.numel() * 4 + rec.numel() * 4 + idx.numel() * 4)
    return arms, info


def act_arms():
    torch.manual_seed(0)
    pol = actor_critic(D, (A,), HIDDEN, LAYERS, 0.0, True).cuda()
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layered_layout(pol, bucket, any_state=True, wide_actions=True)
    assert lay is not None and lay["wide_actions"] is True
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

    return {"act/torch_modules": torch_route,
            "act/layered_act_prepared": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop),
            "act/layered_act_paired": lambda: H.mlp_layered_act(obs, noise, bucket.flat_param, lay, actions, logp, value, wop=wop, paired=True)}


def main():
    arms, info = head_arms()
    steps = {k: HEAD_STEPS for k in arms}
    acts = act_arms()
    arms.update(acts)
    steps.update({k: ACT_STEPS for k in acts})
    for fn in arms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            times[k].append(round(batch(fn, steps[k]), 2))
    rows = {}
    for k, ts in times.items():
        s = sorted(ts)
        rows[k] = dict(us_per_call=ts, median=s[len(s) // 2], min=s[0], max=s[-1], **info.get(k, {}))
        print(k, rows[k], file=sys.stderr, flush=True)
    print(json.dumps(dict(k13=dict(M=HEAD_M, H=HEAD_H, calls_per_batch=HEAD_STEPS), act=dict(N=N, D=D, A=A, hidden=HIDDEN, layers=LAYERS,
                                                                                               calls_per_batch=ACT_STEPS),
                          rounds=ROUNDS, warmup_calls=WARMUP, rows=rows,
                          note="us per call, eager, host included; one batch per arm and round, arms alternating; k13: head_ppo's three "
                               "launches with gz beside the activations; old_entry: aurppo_head_ppo_f32, wa_entry: aurppo_head_ppo_wa_f32"),
                     indent=1))


if __name__ == "__main__":
    main()
