"""K11p (aurppo_conv3x3_pool_f32: convolution + bias + ReLU + 2 x 2 max-pool in one launch) against the two launches K11 + K9 it
replaces, per (Conv2d, ReLU, MaxPool2d) block of the robot encoder: config 3 (128 x 128, minibatch 8192) and config 5's shard
(84 x 84, 4096).  Forward only (the backward is the same calls either way).  The two routes alternate in batches of ``--reps``
launches, ``--rounds`` times; reported is the median of the rounds' means [min - max], and the bytes of z that the fused route
neither writes nor reads.
    python tools/bench_conv_pool.py [--rounds 7] [--reps 5] [--out profiles/conv_pool_bench.json]"""
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
ap.add_argument("--out", default=None)
args = ap.parse_args()
# (config, batch, Ci, Co, size, pad): every block a pool follows and K11 takes
LAYERS = [("config3", 8192, 16, 32, 64, 1), ("config3", 8192, 32, 64, 32, 1), ("config3", 8192, 64, 128, 16, 1), ("config3", 8192, 256, 256, 8, 0),
          ("config5", 4096, 16, 32, 42, 1), ("config5", 4096, 32, 64, 21, 1), ("config5", 4096, 64, 128, 10, 1)]
def batch(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
rows = []
with torch.no_grad():
    for cfg, B, Ci, Co, S, pad in LAYERS:
        x = torch.rand(B, Ci, S, S, device="cuda")
        w = torch.randn(Co, Ci, 3, 3, device="cuda") * (2.0 / (9 * Ci)) ** 0.5
        b = torch.randn(Co, device="cuda") * 0.1
        assert H.conv3x3_pool_ok(x, Ci, Co, pad) and H.conv3x3_ok(x, Ci, Co, pad)
        fused = lambda: H.conv3x3_pool(x, w, b, pad)
        pair = lambda: H.bias_relu_pool2(H.conv3x3(x, w, pad), b)
        k11 = lambda: H.conv3x3(x, w, pad)
        assert torch.equal(fused().view(torch.int32), pair().view(torch.int32))
        torch.cuda.synchronize()
        t = dict(fused=[], pair=[], k11=[])
        for _ in range(args.rounds):
            for name, fn in (("pair", pair), ("fused", fused), ("k11", k11)):
                t[name].append(batch(fn, args.reps))
        So = S + 2 * pad - 2
        rows.append(dict(config=cfg, batch=B, Ci=Ci, Co=Co, size=S, pad=pad, z_gb=round(B * Co * So * So * 4 / 1e9, 2),
                         fused_ms=stats(t["fused"]), k11_k9_ms=stats(t["pair"]), k11_alone_ms=stats(t["k11"]),
                         fused_over_pair=round(statistics.median(t["fused"]) / statistics.median(t["pair"]), 3)))
        print(rows[-1], file=sys.stderr, flush=True)
        del x
        torch.cuda.empty_cache()
out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
