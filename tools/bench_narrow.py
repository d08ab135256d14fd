"""K11n / K12n (csrc/conv_narrow.hip) against the two routes the 16 -> 32 encoder block's gradients have today, per layer shape, in one
process: (a) the library (aten.convolution_backward, one gradient per call as ``hip_ops._conv3x3_grads`` makes them, the weight
gradient's layout transposes included: the whole call is timed), (b) the wide builds K11 mode 1 / K12 (what AURPPO_K11_DGRAD16=1 /
AURPPO_K12_ALL=1 select), (c) the narrow builds.  The arms alternate in batches of ``--reps`` launches, ``--rounds`` times, after a
warm-up per shape and arm; reported is the median of the rounds' means [min - max] in ms, and per arm the worst error against fp64
(of the sum of |products|) on the same inputs, taken on the first ``--check-images`` images.
Shapes: 16 -> 32 at 64 x 64 with B = 2048 and 8192 (config 3's minibatch), 16 -> 32 at 42 x 42 with B = 4096 (config 5's).
    python tools/bench_narrow.py [--rounds 7] [--reps 5] [--out profiles/narrow_bench.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H
ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--check-images", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
LAYERS = [("config3/4", 2048, 16, 32, 64, 1), ("config3", 8192, 16, 32, 64, 1), ("config5", 4096, 16, 32, 42, 1)]
def batch(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps
def stats(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
def aten(g, x, w, pad, mask):
    return torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)
rows = []
with torch.no_grad():
    lib = H._lib_or_raise()
    for cfg, B, Ci, Co, S, pad in LAYERS:
        x = torch.randn(B, Ci, S, S, device="cuda")
        w = torch.randn(Co, Ci, 3, 3, device="cuda") * (2.0 / (9 * Ci)) ** 0.5
        g = torch.randn(B, Co, S + 2 * pad - 2, S + 2 * pad - 2, device="cuda")
        def k11_wide():
            dx = torch.empty_like(x)
            ws = H._workspace("conv", lib.aurppo_conv3x3_wop_bytes(Co, Ci), x.device)
            H._check(lib.aurppo_conv3x3_f32(H._ptr(g), H._ptr(w), H._ptr(dx), B, Ci, Co, g.shape[2], g.shape[3], pad, 1, *H._ws_stream(ws)), "aurppo_conv3x3_f32")
            return dx
        arms = dict(dx=dict(library=lambda: aten(g, x, w, pad, [True, False, False])[0], wide=k11_wide, narrow=lambda: H.conv3x3_dgrad_narrow(g, w, pad)),
                    dw=dict(library=lambda: aten(g, x, w, pad, [False, True, False])[1], wide=lambda: H.conv3x3_wgrad(g, x, Co, pad),
                            narrow=lambda: H.conv3x3_wgrad_narrow(g, x, Co, pad)))
        # worst error per arm against fp64 on the same inputs: dx on the first images, dw on a batch cut to them
        n = min(B, args.check_images)
        xs, gs = x[:n].contiguous(), g[:n].contiguous()
        ref_dx = F.conv_transpose2d(gs.double(), w.double(), None, padding=pad)
        mag_dx = F.conv_transpose2d(gs.abs().double(), w.abs().double(), None, padding=pad).clamp_min(1e-30)
        def w64(xx, gg):
            with torch.enable_grad():
                wd = torch.zeros(Co, Ci, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
                F.conv2d(xx.double(), wd, None, padding=pad).backward(gg.double())
            return wd.grad
        ref_dw, mag_dw = w64(xs, gs), w64(xs.abs(), gs.abs()).clamp_min(1e-30)
        err = dict(dx={}, dw={})
        for name, fn in arms["dx"].items():
            err["dx"][name] = float(((fn()[:n].double() - ref_dx).abs() / mag_dx).max())
        small = dict(library=lambda: aten(gs, xs, w, pad, [False, True, False])[1], wide=lambda: H.conv3x3_wgrad(gs, xs, Co, pad),
                     narrow=lambda: H.conv3x3_wgrad_narrow(gs, xs, Co, pad))
        for name, fn in small.items():
            err["dw"][name] = float(((fn().double() - ref_dw).abs() / mag_dw).max())
        row = dict(config=cfg, batch=B, Ci=Ci, Co=Co, size=S, pad=pad, gflop=round(2 * B * Co * Ci * 9 * (S + 2 * pad - 2) ** 2 / 1e9, 1))
        for what in ("dx", "dw"):
            for fn in arms[what].values():          # warm-up per shape and arm (the library's first call searches its kernels)
                fn(); fn()
            torch.cuda.synchronize()
            t = {name: [] for name in arms[what]}
            for _ in range(args.rounds):
                for name, fn in arms[what].items():
                    t[name].append(batch(fn, args.reps))
            row[what] = {name: dict(ms=stats(v), err_of_sum_ab=float(f"{err[what][name]:.3e}")) for name, v in t.items()}
            row[what]["narrow_over_library"] = round(statistics.median(t["narrow"]) / statistics.median(t["library"]), 3)
        rows.append(row)
        print(row, file=sys.stderr, flush=True)
        del x, g
        torch.cuda.empty_cache()
out = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, rows=rows)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
