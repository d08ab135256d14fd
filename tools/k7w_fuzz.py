"""Stress: K7w (every build of k_mlpw_step / k_mlpw3_step) on random net shapes -- hidden 8..128, 1..3 layers, state widths that do
and do not fill float4 rows or k-steps, tiny and ragged minibatches, both heads, the three data regimes -- against the fp64 reference
of tests/ref64.py, at the bars of tests/test_mlp_fp64_gpu.py.  The inputs come from ref64's margin-safe builder (no sample within
1e-4 of a branch of the loss), so no case is skipped.  Run it under `timeout` (it also looks for hangs).
    FUZZ_CASES=100 FUZZ_SEED=1 python tools/k7w_fuzz.py"""
import os, sys, random
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")
import torch
from tests import ref64 as R
random.seed(int(os.environ.get("FUZZ_SEED", "1")))
n_cases = int(os.environ.get("FUZZ_CASES", "100"))
worst_g = worst_s = 0.0
kernels = set()
for case in range(n_cases):
    cont = random.random() < 0.6
    hidden = random.choice([8, 24, 32, 48, 64, 65, 80, 96, 100, 112, 128, 128, 128])
    layers = random.choice([1, 2, 3])
    D = random.choice([1, 3, 4, 5, 8, 11, 16, 17, 32, 33, 48, 63, 64, 65, 96, 100, 127, 128])
    A = random.randint(1, 16) if cont else random.randint(2, 16)
    M = random.choice([1, 2, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 1000, 2048, 4096, 8192])
    norm_adv = random.random() < 0.7 and M > 1
    vmode = random.choice([0, 1, 2])
    packed = (A if cont else 1) <= 12 and random.random() < 0.5
    regime, index = random.choice(["normal", "scaled", "bf16half"]), random.choice(["perm", "repeat"])
    if layers == 2 and hidden == 64 and D <= 64:
        continue                       # (2 x 64 over <= 64 state floats is K7's: tools/k7_fuzz.py)
    c = R._mk("k7w", hidden, layers, D, A, cont, M, norm_adv, vmode, regime, index, packed)._replace(seed=case)
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    data["gpu"] = R.gpu_inputs(c, data)
    for k in R.kernels_for(c):
        label = R.select_kernel(c, k, random.choice([0, 1]), os.environ.__setitem__)
        sc, g = R.kernel_step(c, data, R.gpu_policy(c, data["sd"]))
        torch.cuda.synchronize()
        _, _, rg, rs = R.check_step(c, sc, g, data["ref"], Y, Ys, f"case {case} {label}")
        if M >= R.TINY_M:
            worst_g = max(worst_g, rg)
        worst_s = max(worst_s, rs)
        kernels.add((k.name, layers))
print(f"k7w_fuzz: {n_cases} cases ok over {len(kernels)} kernel builds, nothing skipped; worst gradient tensor {worst_g:.2f} x Y at M >= {R.TINY_M} "
      f"(margin {R.MARGIN:g}), worst scalar {worst_s:.2f} x Y (margin {R.MARGIN_SCALARS:g})")
