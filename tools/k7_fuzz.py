"""Stress: K7 (both builds) on random shapes -- tiny and ragged minibatches, every head width, odd observation widths, the three
data regimes, packed records, indices with repeats -- against the fp64 reference of tests/ref64.py, at the bars of
tests/test_mlp_fp64_gpu.py.  The inputs come from ref64's margin-safe builder (no sample within 1e-4 of a branch of the loss), so no
case is skipped.  Looks for hangs too (run it under `timeout`).    FUZZ_CASES=120 FUZZ_SEED=1 [FUZZ_ONLY=case] python tools/k7_fuzz.py"""
import os, sys, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")
import torch
from tests import ref64 as R
random.seed(int(os.environ.get("FUZZ_SEED", "1")))
n_cases = int(os.environ.get("FUZZ_CASES", "120"))
only = int(os.environ.get("FUZZ_ONLY", "-1"))   # re-run one case of a seed (the draws of the others are still consumed)
worst_g = worst_s = 0.0
for case in range(n_cases):
    cont = random.random() < 0.6
    D = random.choice([1, 2, 3, 4, 5, 6, 8, 10, 11, 16, 17, 30, 32, 33, 48, 62, 63, 64])
    A = random.randint(1, 16) if cont else random.randint(2, 16)
    M = random.choice([1, 2, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 1000, 2048, 4096, 8192])
    norm_adv = random.random() < 0.7 and M > 1
    vmode = random.choice([0, 1, 2])
    packed = (A if cont else 1) <= 12 and random.random() < 0.5
    regime, index = random.choice(["normal", "scaled", "bf16half"]), random.choice(["perm", "repeat"])
    static = random.choice([0, 1])
    if only >= 0 and case != only:
        continue
    c = R._mk("k7", 64, 2, D, A, cont, M, norm_adv, vmode, regime, index, packed)._replace(seed=case)
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    data["gpu"] = R.gpu_inputs(c, data)
    for k in R.kernels_for(c):
        label = R.select_kernel(c, k, static, os.environ.__setitem__)
        sc, g = R.kernel_step(c, data, R.gpu_policy(c, data["sd"]))
        torch.cuda.synchronize()
        _, _, rg, rs = R.check_step(c, sc, g, data["ref"], Y, Ys, f"case {case} {label}")
        if M >= R.TINY_M:
            worst_g = max(worst_g, rg)
        worst_s = max(worst_s, rs)
print(f"k7_fuzz: {n_cases} cases ok, nothing skipped; worst gradient tensor {worst_g:.2f} x Y at M >= {R.TINY_M} (margin {R.MARGIN:g}), "
      f"worst scalar {worst_s:.2f} x Y (margin {R.MARGIN_SCALARS:g})")
