"""Run the case list of tests/test_layered_act_fp64_gpu.py (tests/layered_act_cases.py) once and print, per case and quantity, the
rollout step's metric against fp64, the yardstick Y (the same formulas in fp32 torch on the GPU, same metric, floored at one ulp) and
their ratio; for the Categorical head also how many sampled indices differ from the reference's (the test demands none).
profiles/layered_act_fp64_table.txt holds its output.

    python tools/layered_act_fp64_table.py          Exit status 1 if a ratio exceeds ref64.MARGIN or an index differs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from aur_ppo_amd import hip_ops as H
from aur_ppo_amd.actor_critic import actor_critic
from aur_ppo_amd.flat import FlatBucket
from tests import layered_act_cases as LA
from tests import ref64 as R

over, worst = 0, {}
print(f"layered rollout step (k_linear from prepared copies + K14 k_head_act); margin {R.MARGIN:g}")
print(f"{'quantity':8s} {'metric':>10s} {'Y':>10s} {'ratio':>6s} {'index != ref':>12s} {'moved':>5s}  case")
for c in LA.CASES:
    data = LA.build(c)
    Y, _y = LA.yardstick(c, data, "cuda")
    pol = actor_critic(c.D, (c.A,) if c.cont else c.A, c.hidden, c.layers, 0.0, c.cont)
    pol.load_state_dict(data["sd"])
    pol = pol.cuda()
    bucket = FlatBucket(pol.parameters())
    lay = H.mlp_layered_layout(pol, bucket)
    a, lp, v = H.mlp_layered_act(data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous(), bucket.flat_param, lay)
    torch.cuda.synchronize()
    wrong = "" if c.cont else str(int((a.long().cpu() != data["ref"]["action"]).sum()))
    over += bool(wrong and wrong != "0")
    for n, x in LA.metrics(c, data["ref"], v, a, lp).items():
        print(f"{n:8s} {x:10.3e} {Y:10.3e} {x / Y:6.2f} {wrong:>12s} {data['moved']:5d}  {R.case_id(c)}", flush=True)
        worst[n] = max(worst.get(n, 0.0), x / Y)
        over += x / Y > R.MARGIN
print("== worst ratio per quantity")
for n in sorted(worst):
    print(f"{n:8s} {worst[n]:6.2f}")
print(f"{over} ratios above the margin {R.MARGIN:g} or cases with a differing index")
sys.exit(1 if over else 0)
