"""Time the head kernels and the fused rollout kernels alone at the headline sizes, one line per kernel and shape:
K13 (hip_ops.head_ppo: statistics + k_head_ppo + fold, M = 131072) and K14 (hip_ops.head_act, N = 4096) for H = 256, 512 and 1024
(one, two and four waves per row); K8 (2 x 64) and K8w (1 x 64, 3 x 128; its prepare launch included) through hip_ops.mlp_act at
N = 4096; each with a Gaussian head of 6 and a Categorical head of 6.  No other tool resolves these: bench_wide.py's widest shape
is 3 x 128 (no K13), bench_layered_act.py times the whole layered step with its host time, rollout_step.sh gives one sample of K8
per run.  The calls are captured into a hipGraph (no host time between launches) and its replays timed between device events:
    [AURPPO_LIB=<other build>] python tools/head_time.py"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H
from aur_ppo_amd.actor_critic import actor_critic
from aur_ppo_amd.flat import FlatBucket
from build_bitdiff import head_layout      # (tools/ is this script's directory)
M, N, A, BATCHES = 131072, 4096, 6, 7
g = torch.Generator(device="cuda").manual_seed(1)


def graph_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    graph.replay()
    ts = []
    for _ in range(BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps * 1e3)
    return f"{np.median(ts):.2f} us (min {min(ts):.2f}, max {max(ts):.2f})"


def policy(D, hidden, layers, cont):
    torch.manual_seed(0)
    pol = actor_critic(D, (A,) if cont else A, hidden, layers, 0.0, cont).cuda()
    noise = torch.randn(N, A, device="cuda", generator=g) if cont else torch.rand(N, device="cuda", generator=g)
    out = [torch.empty((N, A) if cont else (N,), device="cuda"), torch.empty(N, device="cuda"), torch.empty(N, device="cuda")]
    return pol, FlatBucket(pol.parameters()), noise, out


for Hd in (256, 512, 1024):
    for cont in (True, False):
        pol, bucket, noise, out = policy(16, Hd, 1, cont)
        lay = head_layout(H, pol, bucket, Hd, A, cont)
        hA, hC = (torch.tanh(torch.randn(M, Hd, device="cuda", generator=g)) for _ in range(2))
        gzA, gzC = torch.empty_like(hA), torch.empty_like(hC)
        act = torch.randn(M, A, device="cuda", generator=g) if cont else torch.randint(0, A, (M,), device="cuda", generator=g).float()
        rec = torch.stack([-4 + 0.2 * torch.randn(M, device="cuda", generator=g), 2 * torch.randn(M, device="cuda", generator=g),
                           torch.randn(M, device="cuda", generator=g), torch.randn(M, device="cuda", generator=g)], 1).contiguous()
        idx, sc = torch.randperm(M, device="cuda").int(), torch.empty(9, device="cuda")
        tag = f"H={Hd} {'gauss' if cont else 'cat'}"
        print(f"K13 {tag} M={M}: " + graph_us(lambda: H.head_ppo(hA, hC, act, rec, idx, bucket.flat_param, lay, bucket.flat_grad, 0.2, 0.01, 0.5,
                                                                 True, 1, sc, gzA=gzA, gzC=gzC), 20), flush=True)
        print(f"K14 {tag} N={N}: " + graph_us(lambda: H.head_act(hA[:N], hC[:N], noise, bucket.flat_param, lay, *out), 200), flush=True)
for hidden, layers in ((64, 2), (64, 1), (128, 3)):
    for cont in (True, False):
        pol, bucket, noise, out = policy(64, hidden, layers, cont)
        lay = H.mlp_layout(pol, bucket)
        obs = torch.randn(N, 64, device="cuda", generator=g)
        print(f"{'K8w' if lay['wide'] else 'K8'} {layers}x{hidden} {'gauss' if cont else 'cat'} N={N}: "
              + graph_us(lambda: H.mlp_act(obs, noise, bucket.flat_param, lay, *out), 200), flush=True)
