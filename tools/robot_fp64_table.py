"""The robot policy's step-1 gradients against the routing-pinned fp64 reference (tests/ref64_robot.py), per path, observation
shape and tensor: metric (max |g - g64| over the tensor's largest sum of |terms|), Y (the same pinned step in plain fp32 torch on the
GPU), their ratio, the per-element figures of both, and the earlier gate's figure max|g - g_torch32| / max|g| beside them; per layer
the near-tie share of its decisions and the routing disagreements inside the near-tie set.

    python tools/robot_fp64_table.py > profiles/robot_fp64_table.txt          exit status 1 if a ratio exceeds its margin
    python tools/robot_fp64_table.py --margins [N]      CPU only: the second correct fp32 formulation (split first convolution) against
                                                        Y over N seeds (default 60), both shapes: where the class margins come from"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")
import torch
from oracle import ppo_oracle as O
from tests import ref64_robot as R


def margins(n_seeds):
    worst = {}
    for seed in range(2, 2 + n_seeds):
        for C, S in R.SHAPES:
            sd, case = R.make_case(C, S, seed)
            ref = R.step(sd, case, None, O.VLOSS_CLIPPED, scales=True)
            shares = R.check_routing(ref["routing"], ref["decisions"])
            Y = R.yardstick(sd, case, ref, O.VLOSS_CLIPPED)
            got = R.step(sd, case, ref["routing"], O.VLOSS_CLIPPED, torch.float32, split_first=True)
            r, _, _, _ = R.ratios(got, ref, Y)
            pe = R.grad_metrics(got["grads"], ref, per_element=True)
            r.update(per_element=max(pe[n] / Y["per_element"][n] for n in pe), Y_per_element=max(Y["per_element"].values()),
                     near_tie_share=max(s for s, _ in shares))
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
            print(f"seed {seed:2d} {C}x{S}x{S}: " + "  ".join(f"{k} {v:.3g}" for k, v in r.items()) + f"  records moved {case['moved']}", flush=True)
            R._CASES.clear()
    print("worst: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def table():
    over = 0
    worst_by_path = {}
    for path in R.PATHS:
        for C, S in R.SHAPES:
            sd, case = R.make_case(C, S)
            pol = R.gpu_policy(sd, C, S)
            saved_env = os.environ.get("AURPPO_K12_ALL")
            undo = []

            def setattr_(obj, name, value):
                undo.append((obj, name, getattr(obj, name), name in vars(obj)))
                setattr(obj, name, value)
            calls = R.select_path(path, pol, setattr_, os.environ.__setitem__)
            lp, ent, v, routing, counts = R.path_evaluate(pol, case)
            for vmode, vname in ((O.VLOSS_CLIPPED, "clip_vloss"), (O.VLOSS_RETURNS, "returns")):
                ref = R.reference((C, S, 2), sd, case, routing, vmode)
                Y = R.gpu_yardstick((C, S, 2), sd, case, ref, vmode)
                got = R.path_step(pol, case, lp, ent, v, vmode, True)
                r, gm, fm, sm = R.ratios(got, ref, Y)
                pe = R.grad_metrics(got["grads"], ref, per_element=True)
                print(f"== {path}  {C}x{S}x{S}  {vname}: worst ratios " + "  ".join(f"{k} {x:.2f}" for k, x in r.items())
                      + f"   K9 {counts['K9']} (with plane {counts['K9_plane']})  K10 {counts['K10']}  K11 {calls['K11']}  K12 {calls['K12']}")
                if vmode == O.VLOSS_CLIPPED:
                    sh = R.check_routing(routing, ref["decisions"], label=path)
                    print("   near-tie share per layer (%): " + " ".join(f"{100 * s:.3f}" for s, _ in sh))
                    print("   routing disagreements inside the near-tie set: " + " ".join(str(n) for _, n in sh) + "   (outside: 0, asserted)")
                print(f"   {'tensor':28s} {'metric':>10s} {'Y':>10s} {'ratio':>6s} {'per-elem':>10s} {'Y per-el':>10s} {'old gate: max|d|/max|g|':>24s}")
                for n, m in gm.items():
                    g32 = Y["got"]["grads"][n]
                    old = float((got["grads"][n] - g32).abs().max() / g32.abs().max().clamp_min(1e-30))
                    print(f"   {n:28s} {m:10.3e} {Y['grads'][n]:10.3e} {m / Y['grads'][n]:6.2f} {pe[n]:10.3e} {Y['per_element'][n]:10.3e} {old:24.3e}")
                    over += m > R.MARGIN_GRADS * Y["grads"][n]
                for n, m in fm.items():
                    print(f"   {n:28s} {m:10.3e} {Y['fwd'][n]:10.3e} {m / Y['fwd'][n]:6.2f}")
                    over += m > R.MARGIN_FWD * Y["fwd"][n]
                ws = max(sm, key=sm.get)
                print(f"   scalars, worst: {ws:12s} {sm[ws]:10.3e} {Y['scalars']:10.3e} {sm[ws] / Y['scalars']:6.2f}", flush=True)
                over += sm[ws] > R.MARGIN_SCALARS_ROBOT * Y["scalars"]
                for k, x in r.items():
                    worst_by_path[(path, k)] = max(worst_by_path.get((path, k), 0.0), x)
            R.assert_path_ran(path, counts, calls, sd, 2)
            for obj, name, old, own in reversed(undo):
                setattr(obj, name, old) if own else delattr(obj, name)
            if saved_env is None:
                os.environ.pop("AURPPO_K12_ALL", None)
    print("== worst ratio per path and class")
    for (path, k), x in worst_by_path.items():
        print(f"{path:28s} {k:8s} {x:6.2f}")
    print(f"{over} figures above their margin (gradients {R.MARGIN_GRADS:g}, forward {R.MARGIN_FWD:g}, scalars {R.MARGIN_SCALARS_ROBOT:g})")
    return over


if __name__ == "__main__":
    if "--margins" in sys.argv:
        i = sys.argv.index("--margins")
        margins(int(sys.argv[i + 1]) if i + 1 < len(sys.argv) else 60)
        sys.exit(0)
    sys.exit(1 if table() else 0)
