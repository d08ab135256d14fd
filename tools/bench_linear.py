"""A workload for per-launch kernel times of the linear kernels at one size: k_linear (the forward product; the input gradient is the
same build at a square layer) and k_linear_wgrad on M rows of a WIDTH-wide hidden layer, REPS launches each after a warm-up.  The
launches are shorter than the host's call at small M, so the times come from the kernel trace, not from events around the loop:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_linear.py --rows 4096
    python tools/kstats.py <dir> 8
    AURPPO_LIB=<another build of the library> rocprofv3 ... -- python tools/bench_linear.py --rows 4096        (alternate the two builds)"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=4096)
ap.add_argument("--width", type=int, default=256)
ap.add_argument("--reps", type=int, default=200)
args = ap.parse_args()
g = torch.Generator(device="cuda").manual_seed(0)
x = torch.tanh(torch.randn(args.rows, args.width, device="cuda", generator=g))
gy = torch.randn(args.rows, args.width, device="cuda", generator=g) * 1e-4
w = torch.randn(args.width, args.width, device="cuda", generator=g) * (1.0 / args.width) ** 0.5
for reps in (10, args.reps):
    for _ in range(reps):
        H.linear_nobias(x, w, 0)
    for _ in range(reps):
        H.linear_wgrad(gy, x)
    torch.cuda.synchronize()
print(f"library {os.environ.get('AURPPO_LIB', 'default build')}: rows {args.rows}, width {args.width}, {args.reps} + 10 launches per kernel")
