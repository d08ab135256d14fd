"""One minibatch step of the layered update route, timed at M = 131 072 out of B = 524 288 rows for 2 x 256 and 3 x 256 (A 6, Gaussian
head) over D 64 and D 17, four ways --
  * ``layered_step``: ``hip_ops.mlp_layered_step``, the Python loop over the C entry points with a ``torch.sum`` per lower layer;
  * ``layered_step_native``: ``hip_ops.mlp_layered_step_native``, one native call, the lower layers' bias gradients out of k_linear_wgrad;
  * ``layered_minibatch``: ``hip_ops.mlp_layered_minibatch``, the native step with clip + Adam behind it (the only arm that also steps
    the optimizer: two more launches over n_params floats);
  * ``per_op``: what the trainer does without the layered switches -- K3 gather, ``policy.evaluate``, K4 + K5, ``zero_grad`` and
    autograd's backward.
tools/bench_layered_ragged.py's alternation: the arms run in the same process, ROUNDS rounds of one batch of steps per arm between
device events, after a warm-up; median, minimum and maximum of the rounds.  All eager, host included.  Prints one JSON object
(``profiles/layered_native_bench.json`` holds one); run on the GPU box:
    python tools/bench_layered_step.py > layered_native_bench.json"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aur_ppo_amd import _lib                              # noqa: E402
if os.environ.get("AURPPO_LIB"):                          # another build of the library (tools/build_variant.sh), as tools/bench_wgrad.py
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H                       # noqa: E402
from aur_ppo_amd.actor_critic import actor_critic         # noqa: E402
from aur_ppo_amd.flat import FlatBucket                   # noqa: E402
from tools.bench_layered_ragged import alternate          # noqa: E402

HIDDEN, A = 256, 6
M, B = 131072, 4 * 131072
STEPS, WARMUP = 10, 3
SHAPES = [(2, 64), (3, 64), (2, 17), (3, 17)]           # (layers, D)


def one_shape(layers, D):
    torch.manual_seed(0)
    pol = actor_critic(D, (A,), HIDDEN, layers, 0.0, True).cuda()
    bk = FlatBucket(pol.parameters())
    lay = H.mlp_layered_layout(pol, bk, any_state=True)
    assert lay is not None and lay["D"] == D and lay["num_layers"] == layers and bk.numel == lay["n_params"]
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(B, D, device="cuda", generator=g)
    acts = torch.randn(B, A, device="cuda", generator=g)
    with torch.no_grad():
        _, lp0, _, v0 = pol.evaluate(obs, acts)
    rec = torch.stack([lp0 + 0.05 * torch.randn(B, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g),
                       v0.flatten() + torch.randn(B, device="cuda", generator=g),
                       v0.flatten() + 0.05 * torch.randn(B, device="cuda", generator=g)], 1).contiguous()
    idx = torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    sc = torch.empty(H.N_SCALARS, device="cuda")
    knobs = (0.2, 0.01, 0.5, True, H.VLOSS_CLIPPED)
    head = (obs, acts, rec, idx, bk.flat_param, lay)
    # the minibatch arm steps a copy of the parameters at a learning rate of 0: the weights every arm reads stand still
    p_mb, g_mb = bk.flat_param.clone(), torch.empty_like(bk.flat_grad)
    m, v = torch.zeros_like(p_mb), torch.zeros_like(p_mb)
    lr, t, norm = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.empty(1, device="cuda")

    s_py = H.mlp_layered_step(*head, bk.flat_grad, *knobs).clone()
    g_py = bk.flat_grad.clone()
    s_nat = H.mlp_layered_step_native(*head, bk.flat_grad, *knobs)
    lower = torch.zeros_like(g_py, dtype=torch.bool)
    for net in range(2):
        for l in range(layers - 1):
            o = lay["offsets"][net * 2 * (layers + 1) + 2 * l + 1]
            lower[o:o + HIDDEN] = True
    same = bool(torch.equal(s_py, s_nat)) and bool(torch.equal(g_py[~lower], bk.flat_grad[~lower]))

    def per_op():
        mb = H.gather(idx, [obs, acts, rec])
        _, nlp, ent, nv = pol.evaluate(mb[0], mb[1])
        loss = H.ppo_loss_packed(nlp, nv, ent, mb[2], *knobs, sc)
        bk.zero_grad()
        loss.backward()

    arms = {"layered_step": lambda: H.mlp_layered_step(*head, bk.flat_grad, *knobs, sc),
            "layered_step_native": lambda: H.mlp_layered_step_native(*head, bk.flat_grad, *knobs, sc),
            "layered_minibatch": lambda: H.mlp_layered_minibatch(obs, acts, rec, idx, p_mb, lay, g_mb, *knobs, sc, m, v, lr, t, 0.5,
                                                                 (0.9, 0.999), 1e-5, norm),
            "per_op": per_op}
    return dict(layers=layers, D=D, native_equals_python_outside_lower_biases=same, launches_python=14 * layers - 3,
                launches_native=12 * layers - 1, **alternate(arms, STEPS, WARMUP))


def main():
    out = [one_shape(layers, D) for layers, D in SHAPES]
    print(json.dumps(dict(library=os.environ.get("AURPPO_LIB", "default build"), hidden=HIDDEN, A=A, M=M, B=B, rounds=7, steps_per_batch=STEPS, warmup_steps=WARMUP, shapes=out,
                          note="us per step, eager, host included; one batch per arm and round, arms alternating; layered_minibatch "
                               "alone includes clip + Adam"), indent=1))


if __name__ == "__main__":
    main()
