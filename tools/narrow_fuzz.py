"""Random-shape stress of the narrow gradient builds K11n / K12n (csrc/conv_narrow.hip) against fp64: any Ci in 1..16, Co a multiple of 32
(K11n) or in 1..32 (K12n), maps of one pixel to several tiles, batches from one image to several slices, every padding; every case is
run twice and must leave the same bits.
    python tools/narrow_fuzz.py [n_cases]"""
import os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from aur_ppo_amd import hip_ops as H
n = int(sys.argv[1]) if len(sys.argv) > 1 else 80
random.seed(34)
worst_d = worst_w = 0.0
done = 0
for case in range(n):
    B = random.choice([1, 2, 3, 7, 16, 33, 128, 300])
    Ci = random.randint(1, 16)
    Hh, Ww = random.choice([1, 2, 3, 5, 8, 9, 16, 17, 21, 42]), random.choice([1, 2, 4, 7, 15, 16, 17, 31, 33, 42, 64])
    pad = random.choice([0, 1, 1, 2])
    Ho, Wo = Hh + 2 * pad - 2, Ww + 2 * pad - 2
    if Ho <= 0 or Wo <= 0 or B * 96 * Ho * Wo > 30_000_000:
        continue
    g = torch.Generator(device="cuda").manual_seed(case)
    Co = 32 * random.randint(1, 3)
    dy = torch.randn(B, Co, Ho, Wo, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * (2.0 / (9 * Co)) ** 0.5
    dx = H.conv3x3_dgrad_narrow(dy, w, pad)
    ref = F.conv_transpose2d(dy.double(), w.double(), None, padding=pad)
    mag = F.conv_transpose2d(dy.abs().double(), w.abs().double(), None, padding=pad).clamp_min(1e-30)
    e = ((dx.double() - ref).abs() / mag).max().item()
    assert dx.shape == ref.shape and e <= 1e-6, ("K11n", case, B, Ci, Co, Hh, Ww, pad, e)
    assert torch.equal(H.conv3x3_dgrad_narrow(dy, w, pad), dx), ("K11n not deterministic", case)
    worst_d = max(worst_d, e)
    Co = random.randint(1, 32)
    x = torch.randn(B, Ci, Hh, Ww, device="cuda", generator=g)
    dy = torch.randn(B, Co, Ho, Wo, device="cuda", generator=g)
    dw = H.conv3x3_wgrad_narrow(dy, x, Co, pad)
    def w64(xx, gg):
        wd = torch.zeros(Co, Ci, 3, 3, device="cuda", dtype=torch.float64, requires_grad=True)
        F.conv2d(xx.double(), wd, None, padding=pad).backward(gg.double())
        return wd.grad
    ref, mag = w64(x, dy), w64(x.abs(), dy.abs()).clamp_min(1e-30)
    e = ((dw.double() - ref).abs() / mag).max().item()
    assert e <= 1e-6, ("K12n", case, B, Ci, Co, Hh, Ww, pad, e)
    assert torch.equal(H.conv3x3_wgrad_narrow(dy, x, Co, pad), dw), ("K12n not deterministic", case)
    worst_w = max(worst_w, e)
    done += 1
torch.cuda.synchronize()
print(f"narrow_fuzz: {done} shapes ok; worst error of sum|ab|: K11n {worst_d:.3e}, K12n {worst_w:.3e}")
