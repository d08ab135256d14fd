"""K11x (hidden activations kept as bf16 planes) per hidden layer of the robot encoder, config 3 (128 x 128) and config 5 (84 x 84) at
batch 2 048 like tools/bench_conv.py: the K11 / K11p forward with fp32 input against the same launch reading planes, the producer's
extra stores counted on the producer's side (K11p and K10 with and without the output's planes), and k_split_planes alone on every
layer's input.  Forward only.  The routes of a layer alternate in batches of ``--reps`` launches, ``--rounds`` times; reported is the
median of the rounds' means [min - max] in milliseconds.  Every planes result is checked bit for bit against its fp32 sibling first.
    python tools/bench_conv_planes.py [--rounds 7] [--reps 5] [--batch 2048] [--out profiles/conv_planes_bench.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--out", default=None)
args = ap.parse_args()
B = args.batch
# (config, Ci, Co, size, pad, a pool follows)
LAYERS = [("config3", 16, 32, 64, 1, True), ("config3", 32, 64, 32, 1, True), ("config3", 64, 128, 16, 1, True), ("config3", 128, 256, 8, 1, False),
          ("config5", 16, 32, 42, 1, True), ("config5", 32, 64, 21, 1, True), ("config5", 64, 128, 10, 1, True), ("config5", 128, 256, 5, 0, False)]
FIRST = [("config3", 1, 16, 128), ("config5", 3, 16, 84)]      # K10: (config, image channels, Co, size)
def batch(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
def timed(routes):
    for fn in routes.values(): fn()                  # warm: workspaces, code objects
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            t[k].append(batch(fn, args.reps))
    return {k + "_ms": stats(v) for k, v in t.items()}, {k: statistics.median(v) for k, v in t.items()}
def bits(t):
    return t.view(torch.int32)
rows = []
with torch.no_grad():
    for cfg, ci, co, S in FIRST:
        obs, state = torch.rand(B, ci, S, S, device="cuda"), (torch.rand(B, device="cuda") < 0.5).float()
        w, b = torch.randn(co, ci + 1, 3, 3, device="cuda") * 0.3, torch.randn(co, device="cuda") * 0.1
        y, yp = H.first_block(obs, state, w, b, want_planes=True)
        assert torch.equal(bits(y), bits(H.first_block(obs, state, w, b))) and torch.equal(yp, H.split_planes(y))
        ms, med = timed(dict(k10=lambda: H.first_block(obs, state, w, b), k10_planes_out=lambda: H.first_block(obs, state, w, b, want_planes=True),
                             split_of_output=lambda: H.split_planes(y)))
        rows.append(dict(kernel="K10", config=cfg, batch=B, Ci=ci, Co=co, size=S, **ms,
                         planes_out_over_plain=round(med["k10_planes_out"] / med["k10"], 3)))
        print(rows[-1], file=sys.stderr, flush=True)
        del obs, y, yp
        torch.cuda.empty_cache()
    for cfg, ci, co, S, pad, pooled in LAYERS:
        x = torch.relu(torch.randn(B, ci, S, S, device="cuda"))      # what a block hands on: half of it zeros
        w, b = torch.randn(co, ci, 3, 3, device="cuda") * (2.0 / (9 * ci)) ** 0.5, torch.randn(co, device="cuda") * 0.1
        xp = H.split_planes(x)
        if pooled:
            ref = H.conv3x3_pool(x, w, b, pad)
            for pin, want in ((True, False), (False, True), (True, True)):
                got = H.conv3x3_pool_planes(x, xp if pin else None, w, b, pad, want)
                y = got[0] if want else got
                assert torch.equal(bits(y), bits(ref)) and (not want or torch.equal(got[1], H.split_planes(ref)))
            routes = dict(f32_in=lambda: H.conv3x3_pool(x, w, b, pad), planes_in=lambda: H.conv3x3_pool_planes(x, xp, w, b, pad, False),
                          f32_in_planes_out=lambda: H.conv3x3_pool_planes(x, None, w, b, pad, True),
                          planes_in_planes_out=lambda: H.conv3x3_pool_planes(x, xp, w, b, pad, True), split_of_input=lambda: H.split_planes(x))
        else:
            assert torch.equal(bits(H.conv3x3_planes(x, xp, w, pad)), bits(H.conv3x3(x, w, pad)))
            routes = dict(f32_in=lambda: H.conv3x3(x, w, pad), planes_in=lambda: H.conv3x3_planes(x, xp, w, pad), split_of_input=lambda: H.split_planes(x))
        ms, med = timed(routes)
        row = dict(kernel="K11p" if pooled else "K11", config=cfg, batch=B, Ci=ci, Co=co, size=S, pad=pad, **ms,
                   planes_in_over_f32=round(med["planes_in"] / med["f32_in"], 3))
        if pooled:
            row.update(planes_out_over_f32=round(med["f32_in_planes_out"] / med["f32_in"], 3),
                       both_over_f32=round(med["planes_in_planes_out"] / med["f32_in"], 3))
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
        del x, xp
        torch.cuda.empty_cache()
out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
