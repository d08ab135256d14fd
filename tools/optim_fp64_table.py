"""Run the case lists of tests/test_optim_fp64_gpu.py once and print, per entry point, case and quantity, the metric against the fp64
clip + Adam of tests/ref64_optim.py, the yardstick Y (torch's clip_grad_norm_ + single-tensor Adam in fp32 on the GPU, same metric) and
their ratio.  DESIGN 2.2 quotes this table (profiles/optim_fp64_table.txt).  The kernels judged: clip.hip (K6, K6b) and mlp_tail.hip (the
reduce kernels and k_adam_chain behind mlp_ppo_minibatch / mlp_ppo_apply).

    python tools/optim_fp64_table.py          AURPPO_LIB=<other build of the library> to judge that build instead
Exit status 1 if any ratio exceeds its margin (tests/ref64_optim.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")      # the library re-reads its knobs on every call
import torch  # noqa: E402,F401
from aur_ppo_amd import _lib  # noqa: E402
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from tests import ref64_optim as R  # noqa: E402
from tests import test_optim_fp64_gpu as T  # noqa: E402

worst, over = {}, 0


def setenv(k, v):
    os.environ[k] = v


def row(entry, case, got, quantities=R.QUANTITIES):
    global over
    ref = R.reference_of(case)
    Y, _ = R.yardstick(case, ref, "cuda")
    cells = []
    for q, x in R.metrics(got, ref, None, quantities).items():
        r = x / Y[q]
        cells.append(f"{q} {x:9.3e} {Y[q]:9.3e} {r:5.2f}")
        key = (entry, q)
        worst[key] = max(worst.get(key, 0.0), r)
        over += r > R.MARGINS[q]
    print(f"{entry:44s} " + " | ".join(cells) + f" : {case['id']}", flush=True)


print(f"library: {os.path.basename(_lib.LIB_PATH) if os.environ.get('AURPPO_LIB') else 'default build'}; margins "
      + ", ".join(f"{q} {m:g}" for q, m in R.MARGINS.items()))
print("per quantity: metric, Y, ratio")
print("== K6: grad_norm_clip_ (k_sqnorm, k_clip_scale)")
for kw in R.K6_CASES:
    case = R.build(**kw)
    row("K6", case, R.run_k6(case), ("norm", "gc"))
print("== K6b: clip_adam_ (k_sqnorm_step, k_clip_adam)")
for kw in R.K6B_CASES:
    case = R.build(**kw)
    got, step = R.run_k6b(case)
    assert step == case["t"]
    row("K6b", case, got)
print("== mlp_ppo_apply (k_adam_chain, in-kernel norm)")
for pol in R.APPLY_POLICIES:
    lay = T._policy(pol)
    cases = [R.build(n=lay["n_params"], **kw) for kw in R.apply_cases(pol)]
    for case, mis in [(c, False) for c in cases] + [(cases[-1], True)]:
        got, _, _ = R.run_apply(case, lay, misalign=mis)
        row("apply (g misaligned)" if mis else "apply", case, got, ("norm", "m", "v", "p"))
print("== mlp_ppo_apply_parts (k_adam_chain, the caller's partial sums)")
for pol in R.APPLY_POLICIES:
    lay = T._policy(pol)
    n = lay["n_params"]
    p2p = int(_lib.load().aurppo_p2p_parts(n))
    for kw, parts in R.parts_cases(pol):
        case = R.build(n=n, **kw)
        n_part = p2p if isinstance(parts, str) else parts
        got, _, _ = R.run_apply(case, lay, parts=R.host_sq_parts(case["g"], n_part, sparse=parts == "p2p-sparse"))
        row(f"apply_parts[{parts}]", case, got)
print("== mlp_ppo_minibatch: the chained tail (mlp_tail.hip: k_mlp_reduce_x4 / k_mlp_reduce<1,2> -> k_adam_chain), static tiles")
for c, k in T._TAIL:
    for t0, lr in T._TAIL_T:
        for label, case, got in T.tail_runs(c, k, t0, lr, setenv):
            row("tail " + k.name, case, got)

print("== worst ratio per entry point and quantity")
for (entry, q) in sorted(worst):
    print(f"{entry:44s} {q:5s} {worst[(entry, q)]:8.2f}  (margin {R.MARGINS[q]:g})")
print(f"{over} ratios above their margin")
sys.exit(1 if over else 0)
