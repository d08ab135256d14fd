"""Run the finite-input cases of tests/test_loss_fp64_gpu.py once (the M sweep, and every regime x hyperparameter set) and print, per case,
entry point and output class, the metric against the fp64 loss of tests/ref64_loss.py, the yardstick Y (fp32 torch autograd on the CPU,
same metric, floored at one fp32 ulp) and their ratio.  DESIGN 2.3 quotes this table (profiles/loss_fp64_table.txt).

    python tools/loss_fp64_table.py          AURPPO_LIB=<other build of the library> to judge that build instead
Exit status 1 if any ratio exceeds its margin (tests/ref64_loss.py), or if a packed result differs from the unpacked one in bits."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from aur_ppo_amd import _lib  # noqa: E402
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from tests import ref64_loss as R  # noqa: E402
from tests import test_loss_fp64_gpu as T  # noqa: E402

CLASSES = R.ARRAYS + ("scalars",)
worst, over = {}, 0


def rows(M, regime, hi):
    global over
    case = T._case(M, regime, hi)
    for na, vm in R.COMBOS:
        ref, Y = T._ref(case, hi, na, vm)
        got = {p: R.kernel_run(case["gpu"], R.HYPERS[hi], na, vm, p) for p in (False, True)}
        same = T._bits_equal(got[False], got[True])
        over += not same
        for p, g in got.items():
            am, sm, r = R.ratios(g, ref, Y)
            cells = []
            for q in CLASSES:
                m, y = (max(sm.values()), Y[1]) if q == "scalars" else (am[q], Y[0][q])
                cells.append(f"{q} {m:9.3e} {y:9.3e} {r[q]:5.2f}")
                key = (q, "M >= TINY_M" if M >= R.TINY_M else "M <  TINY_M")
                worst[key] = max(worst.get(key, 0.0), r[q])
                over += r[q] > (R.scalar_margin(M) if q == "scalars" else R.margin(q, M))
            print(f"{'packed  ' if p else 'unpacked'} " + " | ".join(cells) + f" : M{M}-{regime}-h{hi}-{'norm' if na else 'raw'}-v{vm}"
                  + ("" if same else "  PACKED != UNPACKED"), flush=True)


print(f"library: {os.path.basename(_lib.LIB_PATH) if os.environ.get('AURPPO_LIB') else 'default build'}; margins "
      + ", ".join(f"{q} {R.MARGINS[q]:g} ({R.MARGINS_TINY_M[q]:g} below M = {R.TINY_M})" for q in R.ARRAYS)
      + f", scalars {R.MARGIN_SCALARS:g} ({R.MARGIN_SCALARS_TINY_M:g})")
print("per class: metric, Y, ratio")
print("== the M sweep: normal inputs, hyperparameter set 0")
for M in T.SWEEP_M:
    rows(M, "normal", 0)
print("== every regime x hyperparameter set")
for M in T.REGIME_M:
    for regime in R.REGIMES:
        for hi in range(len(R.HYPERS)):
            rows(M, regime, hi)
print("== worst ratio per class")
for (q, cls) in sorted(worst):
    m = (R.MARGIN_SCALARS if cls.startswith("M >=") else R.MARGIN_SCALARS_TINY_M) if q == "scalars" else R.margin(q, R.TINY_M if cls.startswith("M >=") else 1)
    print(f"{q:10s} {cls} {worst[(q, cls)]:8.2f}  (margin {m:g})")
print(f"{over} ratios above their margin or packed / unpacked mismatches")
sys.exit(1 if over else 0)
