"""The layered routes over a state that is no multiple of 16 floats, timed at 2 x 256, A 6, Gaussian head: one rollout step at
N = 4096 and one minibatch step at M = 131 072 (out of B = 4 M rows), each three ways --
  * ``layered_D17``: ``hip_ops.mlp_layered_act`` (weights prepared once) / ``hip_ops.mlp_layered_step`` at D 17: layer 0 on the tail builds
    k_linear_tail / k_linear_wgrad_tail;
  * ``layered_D32_padded``: the same policy with layer 0's weights and the observations zero-padded to D 32: the aligned kernels;
  * ``per_op_D17``: what the trainer does without the layered switches at D 17 -- ``policy.evaluate`` under no_grad + the three row
    stores for the rollout step; K3 gather, ``policy.evaluate``, K4 + K5, ``zero_grad`` and autograd's backward for the minibatch step.
tools/bench_layered_act.py's alternation: the arms run in the same process, ROUNDS rounds of one batch of steps per arm between device
events, after a warm-up; every batch's time is kept so the spread shows.  All eager, host included.  Prints one JSON object
(``profiles/layered_ragged_bench.json`` holds one); run on the GPU box:
    python tools/bench_layered_ragged.py > layered_ragged_bench.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aur_ppo_amd import hip_ops as H                       # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic         # noqa: E402
from aur_ppo_amd.flat import FlatBucket                   # noqa: E402

HIDDEN, LAYERS, D, DP, A = 256, 2, 17, 32, 6
N, M, B = 4096, 131072, 4 * 131072
ROUNDS = 7
ACT_STEPS, ACT_WARMUP, UPD_STEPS, UPD_WARMUP = 400, 100, 20, 5


def batch(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def alternate(arms, steps, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            times[k].append(round(batch(fn, steps), 2))
    out = {}
    for k, ts in times.items():
        s = sorted(ts)
        out[k] = dict(us_per_step=ts, median=s[len(s) // 2], min=s[0], max=s[-1])
    print(out, file=sys.stderr, flush=True)
    return out


def policies():
    """The D 17 policy and the same policy over a state padded to 32 floats (layer 0's extra columns zero), each with bucket and layout."""
    torch.manual_seed(0)
    pol = actor_critic(D, (A,), HIDDEN, LAYERS, 0.0, True).cuda()
    polp = actor_critic(DP, (A,), HIDDEN, LAYERS, 0.0, True).cuda()
    sd = pol.state_dict()
    with torch.no_grad():
        for k, v in polp.state_dict().items():
            if v.shape == sd[k].shape:
                v.copy_(sd[k])
            else:
                v.zero_()
                v[:, :D].copy_(sd[k])
    bk, bkp = FlatBucket(pol.parameters()), FlatBucket(polp.parameters())
    lay, layp = H.mlp_layered_layout(pol, bk, any_state=True), H.mlp_layered_layout(polp, bkp)
    assert lay is not None and lay["D"] == D and layp is not None and layp["D"] == DP
    return (pol, bk, lay), (polp, bkp, layp)


def main():
    (pol, bk, lay), (_polp, bkp, layp) = policies()
    g = torch.Generator(device="cuda").manual_seed(1)
    pad = lambda t: torch.nn.functional.pad(t, (0, DP - D)).contiguous()

    # ---- one rollout step
    obs = torch.randn(N, D, device="cuda", generator=g)
    obsp = pad(obs)
    noise = torch.randn(N, A, device="cuda", generator=g)
    actions, logp, value = torch.empty(N, A, device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    wop, wopp = H.mlp_layered_prepare(bk.flat_param, lay), H.mlp_layered_prepare(bkp.flat_param, layp)
    a17 = [t.clone() for t in H.mlp_layered_act(obs, noise, bk.flat_param, lay, wop=wop)]
    a32 = H.mlp_layered_act(obsp, noise, bkp.flat_param, layp, wop=wopp)
    same_act = all(bool(torch.equal(x, y)) for x, y in zip(a17, a32))

    def torch_route():
        with torch.no_grad():
            a, lp, _, v = pol.evaluate(obs)
            value.copy_(v.flatten())
        actions.copy_(a)
        logp.copy_(lp)

    act = alternate({"layered_D17": lambda: H.mlp_layered_act(obs, noise, bk.flat_param, lay, actions, logp, value, wop=wop),
                     "layered_D32_padded": lambda: H.mlp_layered_act(obsp, noise, bkp.flat_param, layp, actions, logp, value, wop=wopp),
                     "per_op_D17": torch_route}, ACT_STEPS, ACT_WARMUP)

    # ---- one minibatch step
    obs = torch.randn(B, D, device="cuda", generator=g)
    obsp = pad(obs)
    acts = torch.randn(B, A, device="cuda", generator=g)
    with torch.no_grad():
        _, lp0, _, v0 = pol.evaluate(obs, acts)
    rec = torch.stack([lp0 + 0.05 * torch.randn(B, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g),
                       v0.flatten() + torch.randn(B, device="cuda", generator=g),
                       v0.flatten() + 0.05 * torch.randn(B, device="cuda", generator=g)], 1).contiguous()
    idx = torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    sc = torch.empty(H.N_SCALARS, device="cuda")
    knobs = (0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED)
    s17 = H.mlp_layered_step(obs, acts, rec, idx, bk.flat_param, lay, bk.flat_grad, *knobs).clone()
    s32 = H.mlp_layered_step(obsp, acts, rec, idx, bkp.flat_param, layp, bkp.flat_grad, *knobs)
    same_step = bool(torch.equal(s17, s32))

    def per_op():
        mb = H.gather(idx, [obs, acts, rec])
        _, nlp, ent, nv = pol.evaluate(mb[0], mb[1])
        loss = H.ppo_loss_packed(nlp, nv, ent, mb[2], *knobs, sc)
        bk.zero_grad()
        loss.backward()

    upd = alternate({"layered_D17": lambda: H.mlp_layered_step(obs, acts, rec, idx, bk.flat_param, lay, bk.flat_grad, *knobs, sc),
                     "layered_D32_padded": lambda: H.mlp_layered_step(obsp, acts, rec, idx, bkp.flat_param, layp, bkp.flat_grad, *knobs, sc),
                     "per_op_D17": per_op}, UPD_STEPS, UPD_WARMUP)
    print(json.dumps(dict(hidden=HIDDEN, layers=LAYERS, D=D, D_padded=DP, A=A, rounds=ROUNDS,
                          rollout_step=dict(N=N, steps_per_batch=ACT_STEPS, warmup_steps=ACT_WARMUP, padded_outputs_bit_equal=same_act, **act),
                          minibatch_step=dict(M=M, B=B, steps_per_batch=UPD_STEPS, warmup_steps=UPD_WARMUP, padded_scalars_bit_equal=same_step,
                                              **upd),
                          note="us per step, eager, host included; one batch per arm and round, arms alternating"), indent=1))


if __name__ == "__main__":
    main()
