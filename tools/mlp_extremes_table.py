"""Run the case lists of tests/test_mlp_extremes_fp64_gpu.py once and print, per case and kernel, the worst gradient tensor's metric against
fp64, the three members of the band (Y: plain PyTorch fp32 autograd on the GPU; F, P: the CPU renditions of tests/ref64_extremes.py) and
the metric over each; the same for the scalars and for the rollout step.  DESIGN 2.6 quotes this table (profiles/mlp_extremes_table.txt).

    python tools/mlp_extremes_table.py          Exit status 1 if any ratio over the band exceeds its margin (tests/ref64.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")      # the library re-reads its knobs on every call
import torch
from aur_ppo_amd import hip_ops as H
from tests import ref64 as R
from tests import ref64_extremes as X
from tests import test_mlp_extremes_fp64_gpu as T

worst, over = {}, 0


def note(key, ratio, margin):
    global over
    worst[key] = max(worst.get(key, 0.0), ratio)
    over += ratio > margin


def setenv(k, v):
    os.environ[k] = v


def row(kname, c, sc, g, data):
    band = data["band"]
    gm, sm = R.grad_metrics(g, data["ref"]), R.scalar_metrics(sc, data["ref"])
    w, ws = max(gm, key=gm.get), max(sm, key=sm.get)
    p, Bs = band["parts"], max(band["Bs"].values())
    print(f"{kname:34s} {gm[w]:10.3e} {p['Y']:10.3e} {p['F']:10.3e} {p['P']:10.3e} {gm[w] / p['Y']:8.2f} {gm[w] / p['F']:6.2f} {gm[w] / p['P']:6.2f} "
          f"{gm[w] / band['B']:6.2f} {sm[ws] / Bs:7.2f}  {w} / {ws} : {R.case_id(c)}", flush=True)
    note(f"{kname} gradients, {c.regime}", gm[w] / band["B"], R.MARGIN)
    note(f"{kname} scalars, {c.regime}", sm[ws] / Bs, R.MARGIN_SCALARS)
    note(f"{kname} gradients over Y alone, {c.regime}", gm[w] / p["Y"], float("inf"))


print(f"margins: gradients and rollout {R.MARGIN:g} x B (rollout in deep: {X.MARGIN_ACT_DEEP:g}), scalars {R.MARGIN_SCALARS:g} x max Bs; B = max(Y, F, P)")
print("== one launch at M 1000: worst gradient tensor")
print(f"{'kernel':34s} {'metric':>10s} {'Y':>10s} {'F':>10s} {'P':>10s} {'/Y':>8s} {'/F':>6s} {'/P':>6s} {'/B':>6s} {'scalars':>7s}  worst tensor / scalar : case")
for c in X.STEP_CASES:
    data = T._case(c)
    if c.kind == "layered":
        _H, bucket, lay, _fn, _label = T._act_policy(c, data["sd"])
        obs, act, rec, idx = data["gpu"]
        for route in ("mlp_layered_step", "mlp_layered_step_native"):
            g = torch.full_like(bucket.flat_grad, float("nan"))
            sc = getattr(H, route)(obs, act, rec, idx, bucket.flat_param, lay, g, R.HYPER["clip"], R.HYPER["ent_coef"], R.HYPER["vf_coef"], c.norm_adv, c.vmode)
            torch.cuda.synchronize()
            row(route, c, sc, g[:lay["n_params"]], data)
        continue
    for k in R.kernels_for(c):
        R.select_kernel(c, k, 0, setenv)
        sc, g = R.kernel_step(c, data, R.gpu_policy(c, data["sd"]))
        torch.cuda.synchronize()
        row(k.name, c, sc, g, data)

print("== the rollout step at N 257: worst of value / action / log-prob")
print(f"{'kernel':10s} {'metric':>10s} {'Y':>10s} {'F':>10s} {'P':>10s} {'/Y':>8s} {'/F':>6s} {'/P':>6s} {'/B':>6s}  case")
for c in X.ACT_CASES:
    data = X.build_act(c)
    band = X.band_act(c, data, "cuda")
    _H, bucket, lay, act_fn, label = T._act_policy(c, data["sd"])
    a, lp, v = act_fn(data["obs"].cuda().contiguous(), data["noise"].cuda().contiguous(), bucket.flat_param, lay)
    torch.cuda.synchronize()
    m = max(X.act_metrics(c, data["ref"], v, a, lp).values())
    p = {k: max(x, R.ULP32) for k, x in band["parts"].items()}
    same = "" if c.cont else f"  index equal: {bool(torch.equal(a.long().cpu(), data['ref']['action']))}"
    print(f"{label.split()[0]:10s} {m:10.3e} {p['Y']:10.3e} {p['F']:10.3e} {p['P']:10.3e} {m / p['Y']:8.2f} {m / p['F']:6.2f} {m / p['P']:6.2f} {m / band['B']:6.2f}  "
          f"{R.case_id(c)}{same}", flush=True)
    note(f"{label.split()[0]} rollout, {c.regime}", m / band["B"], X.act_margin(c))
    note(f"{label.split()[0]} rollout over Y alone, {c.regime}", m / p["Y"], float("inf"))

print("== worst ratio per kernel and regime")
for key in sorted(worst):
    print(f"{key:72s} {worst[key]:9.2f}")
print(f"{over} ratios above their margin")
sys.exit(1 if over else 0)
