"""Run the case list of tests/test_mlp_fp64_gpu.py once and print, per case and kernel, the worst gradient tensor's metric against
fp64, the yardstick Y (plain PyTorch fp32 autograd on the GPU, same metric) and their ratio; the same for the scalars and for the
per-sample forward values.  DESIGN's parity section derives the tests' margin from this table (profiles/mlp_fp64_table.txt).

    python tools/mlp_fp64_table.py [--small]          AURPPO_LIB=<other build of the library> to judge that build instead
    --small: leave out the cases with M > 40000.  Exit status 1 if any ratio exceeds its margin (tests/ref64.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("AURPPO_TEST_KNOBS", "1")      # the library re-reads its knobs on every call
import torch
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H
from tests import ref64 as R

small = "--small" in sys.argv
worst_by_kernel, over = {}, 0


def note(kname, ratio, margin=R.MARGIN):
    global over
    worst_by_kernel[kname] = max(worst_by_kernel.get(kname, 0.0), ratio)
    over += ratio > margin


def setenv(k, v):
    os.environ[k] = v


print(f"library: {os.path.basename(_lib.LIB_PATH) if os.environ.get('AURPPO_LIB') else 'default build'}; margin {R.MARGIN:g}")
print("== one launch: worst gradient tensor (metric, Y, ratio) and worst scalar over the worst of the nine scalars' Y")
print(f"{'kernel':34s} {'tiles':7s} {'metric':>10s} {'Y':>10s} {'ratio':>6s} {'scalars':>7s}  worst tensor / scalar : case")
for c in R.K7_CASES + R.K7W_CASES:
    if small and c.M > 40000:
        continue
    data = R.build_case(c)
    data["ref"] = R.reference_step(c, data)
    Y, Ys, _ = R.yardstick_step(c, data, "cuda")
    data["gpu"] = R.gpu_inputs(c, data)
    for k in R.kernels_for(c):
        for static in (0, 1):
            R.select_kernel(c, k, static, setenv)
            sc, g = R.kernel_step(c, data, R.gpu_policy(c, data["sd"]))
            torch.cuda.synchronize()
            gm, sm = R.grad_metrics(g, data["ref"]), R.scalar_metrics(sc, data["ref"])
            w = max(gm, key=gm.get)
            ws, Ysc = max(sm, key=sm.get), max(Ys.values())
            print(f"{k.name:34s} {'static' if static else 'counter':7s} {gm[w]:10.3e} {Y:10.3e} {gm[w] / Y:6.2f} {sm[ws] / Ysc:7.2f}  "
                  f"{w} / {ws} : {R.case_id(c)}", flush=True)
            note(k.name + (" gradients, M >= 31" if c.M >= R.TINY_M else " gradients, M < 31"), gm[w] / Y, R.grad_margin(c.M))
            note(k.name + " scalars", sm[ws] / Ysc, R.MARGIN_SCALARS)

print("== per-sample forward (64 minibatches of one sample): log-prob, entropy, value over Y (worst of the three in fp32 torch)")
for c in R.FWD_CASES:
    data = R.build_case(c)
    li = data["idx"].long()
    obs, act = data["obs"][li], data["act"][li]
    rec = torch.zeros(c.M, 4)
    rec[:, 1] = 1.0
    ref = R.run_step(data["net64"], obs.double(), act.double(), rec.double(), 0.2, 0.01, 1.0, False, 0, scales=True)
    net32 = R.make_net(data["sd"], torch.float32, "cuda")
    with torch.no_grad():
        _, lp_t, ent_t, v_t = net32.evaluate(obs.cuda(), act.cuda() if c.cont else act.cuda().long())
    Y = max(R.forward_metrics(lp_t, ent_t, v_t, ref).values())
    obs_g, act_g, rec_g = obs.cuda().contiguous(), act.cuda().contiguous(), rec.cuda().contiguous()
    for k in R.kernels_for(c):
        R.select_kernel(c, k, 0, setenv)
        _pol, bucket, lay = R.gpu_policy(c, data["sd"])
        g = torch.empty_like(bucket.flat_grad)
        lp, ent, val = [], [], []
        for i in range(c.M):
            sc = H.mlp_ppo_step(obs_g, act_g, rec_g, torch.tensor([i], device="cuda", dtype=torch.int32), bucket.flat_param, lay, g,
                                0.2, 0.01, 1.0, False, H.VLOSS_RETURNS).cpu()
            lp.append(-float(sc[H.S_OLD_KL])), ent.append(float(sc[H.S_ENT])), val.append(float(g[lay["offsets"][-2]]))
        m = R.forward_metrics(torch.tensor(lp), torch.tensor(ent), torch.tensor(val), ref)
        print(f"{k.name:34s} Y {Y:10.3e}  " + "  ".join(f"{n} {v / Y:5.2f}" for n, v in m.items()) + f" : {R.case_id(c)}", flush=True)
        note(k.name + " forward", max(m.values()) / Y)

print("== worst ratio per kernel")
for kname in sorted(worst_by_kernel):
    print(f"{kname:44s} {worst_by_kernel[kname]:8.2f}")
print(f"{over} ratios above their margin (gradients {R.MARGIN:g}, at M < {R.TINY_M} {R.MARGIN_TINY_M:g}; scalars {R.MARGIN_SCALARS:g}; forward {R.MARGIN:g})")
sys.exit(1 if over else 0)
