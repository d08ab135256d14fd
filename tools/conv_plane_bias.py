"""How K11 forward, K11 input gradient and K12 sum their bf16x3 plane products (tests/test_conv_gpu.py asserts the first part).

  1. Operands with KNOWN positive planes p0 * (1 + 2^-10 + 2^-20): every third-order product is exactly 2^-20 of every output, so a product
     that does not arrive is a mean signed error of -1 (in units of 2^-20), while rounding is unbiased.  Printed: mean (max |.|) per role.
  2. Realistic operands (relu'd inputs, xavier filters, dense and 80 % sparse output gradients) against fp64: worst element over the
     largest sum of |terms|, and the mean error over the mean sum of |terms| (a one-sided cut shows there), beside torch's convolution.

    python tools/conv_plane_bias.py >> profiles/conv_plane_bias.txt
    AURPPO_LIB=<another build of the library> python tools/conv_plane_bias.py      the parent's build, or tools/build_variant.sh
                                                                                    x.so -DCONV_EXP_NO_ALTERNATE (step sums, one sign)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from aur_ppo_amd import _lib
if os.environ.get("AURPPO_LIB"):
    _lib.LIB_PATH = os.environ["AURPPO_LIB"]
from aur_ppo_amd import hip_ops as H

UNIT = 2.0 ** -20
SHAPES = ((8, 32, 64, 32, 1), (8, 64, 128, 16, 1), (8, 256, 256, 8, 0))          # (B, Ci, Co, H = W, pad): reductions 288, 576, 2304
VARIANTS = (("a * b0          [a1*b0, a2*b0]", (0, 1, 2), (0,)), ("a0 * b          [a0*b1, a0*b2]", (0,), (0, 1, 2)),
            ("(a0+a1)*(b0+b1) [a1*b1]", (0, 1), (0, 1)), ("a * b, all planes", (0, 1, 2), (0, 1, 2)))


def planes(shape, gen, which):
    """fp32 values p0 * sum(2^-10k for k in which), p0 = (1 + j / 8) * 2^e: split3 gives exactly these planes (asserted)."""
    p0 = (1 + torch.randint(0, 8, shape, generator=gen).double() / 8) * 2.0 ** torch.randint(-2, 3, shape, generator=gen).double()
    v = p0 * sum(2.0 ** (-10 * k) for k in which)
    x = v.float()
    assert torch.equal(x.double(), v)
    b0 = x.bfloat16().float()
    b1 = (x - b0).bfloat16().float()
    b2 = (x - b0 - b1).bfloat16().float()
    for k, b in enumerate((b0, b1, b2)):
        assert torch.equal(b.double(), p0 * 2.0 ** (-10 * k) if k in which else torch.zeros_like(p0))
    return x


def wgrad_all_shapes():
    """K12 takes every shape its kernel accepts while this is set (conv3x3_wgrad_ok); restores the variable afterwards."""
    class _Ctx:
        def __enter__(self):
            self.old = os.environ.get("AURPPO_K12_ALL")
            os.environ["AURPPO_K12_ALL"] = "1"

        def __exit__(self, *a):
            if self.old is None:
                os.environ.pop("AURPPO_K12_ALL", None)
            else:
                os.environ["AURPPO_K12_ALL"] = self.old
    return _Ctx()


def roles(x, w, g, pad, conv):
    """(z, dx, dw) of ``conv`` (H.conv3x3 or torch's) on the GPU."""
    xi, wi = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    with wgrad_all_shapes():
        z = conv(xi, wi, pad)
        z.backward(g.cuda())
    torch.cuda.synchronize()
    return z.detach(), xi.grad, wi.grad


def refs(x, w, g, pad):
    """fp64 (z, dx, dw) and the sums of |terms| behind them."""
    xd, wd, gd = x.double(), w.double(), g.double()
    f = lambda a, b, c: (F.conv2d(a, b, None, padding=pad), torch.nn.grad.conv2d_input(x.shape, b, c, padding=pad),      # noqa: E731
                         torch.nn.grad.conv2d_weight(a, w.shape, c, padding=pad))
    return f(xd, wd, gd), f(xd.abs(), wd.abs(), gd.abs())


def plane_bias(B, Ci, Co, Hh, pad, wa, wb, gen):
    """Mean signed relative error and max |.| of K11 forward / K11 input gradient / K12 in units of 2^-20; operand a (x, dz, dz)
    holds the planes ``wa``, operand b (w, w, x) the planes ``wb``."""
    Ho = Hh + 2 * pad - 2
    out = []
    for x, w, g in ((planes((B, Ci, Hh, Hh), gen, wa), planes((Co, Ci, 3, 3), gen, wb), None),
                    (None, planes((Co, Ci, 3, 3), gen, wb), planes((B, Co, Ho, Ho), gen, wa)),
                    (planes((B, Ci, Hh, Hh), gen, wb), None, planes((B, Co, Ho, Ho), gen, wa))):
        role = 0 if g is None else (1 if x is None else 2)
        x = torch.ones(B, Ci, Hh, Hh) if x is None else x
        w = torch.ones(Co, Ci, 3, 3) if w is None else w
        g = torch.ones(B, Co, Ho, Ho) if g is None else g
        got, ref = roles(x, w, g, pad, H.conv3x3)[role], refs(x, w, g, pad)[0][role]
        rel = (got.double().cpu() - ref) / ref
        out.append((float(rel.mean()) / UNIT, float(rel.abs().max()) / UNIT))
    return out


def realistic(B, Ci, Co, Hh, pad, sparse, gen):
    x = torch.relu(torch.randn(B, Ci, Hh, Hh, generator=gen))
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * (2.0 / (9 * Ci + 9 * Co)) ** 0.5
    Ho = Hh + 2 * pad - 2
    g = torch.randn(B, Co, Ho, Ho, generator=gen) * 1e-4 * torch.exp(torch.randn(B, Co, 1, 1, generator=gen))
    if sparse:
        g = g * (torch.rand(B, Co, Ho, Ho, generator=gen) < 0.2)
    ref, S = refs(x, w, g, pad)
    res = {}
    for name, conv in (("K11/K12", H.conv3x3), ("torch", lambda a, b, p: F.conv2d(a, b, None, padding=p))):
        got = roles(x, w, g, pad, conv)
        res[name] = [(float((a.double().cpu() - r).abs().max() / s.max()), float((a.double().cpu() - r).mean() / s.mean())) for a, r, s in zip(got, ref, S)]
    return res


if __name__ == "__main__":
    print(f"library: {os.environ.get('AURPPO_LIB', 'default build')}")
    gen = torch.Generator().manual_seed(0)
    print("== known positive planes: mean signed error (max |.|) in units of 2^-20; a missing third-order product reads -1")
    for B, Ci, Co, Hh, pad in SHAPES:
        for name, wa, wb in VARIANTS:
            r = plane_bias(B, Ci, Co, Hh, pad, wa, wb, gen)
            print(f"{Ci:3d}->{Co:3d} {Hh:2d}x{Hh:<2d} pad {pad}  {name:32s} " + "  ".join(f"{n} {m:+.3f} ({x:.2f})" for n, (m, x) in zip(("fwd", "dx", "dw"), r)), flush=True)
    print("== realistic operands against fp64: worst element / largest sum|terms| (mean error / mean sum|terms|)")
    for B, Ci, Co, Hh, pad in ((32, 32, 64, 32, 1), (32, 64, 128, 16, 1), (32, 128, 256, 8, 1), (32, 256, 256, 8, 0)):
        for sparse in (False, True):
            res = realistic(B, Ci, Co, Hh, pad, sparse, gen)
            print(f"{Ci:3d}->{Co:3d} {Hh:2d}x{Hh:<2d} pad {pad} {'sparse' if sparse else 'dense ':6s} " + "   ".join(
                f"{k}: " + "  ".join(f"{n} {a:.2e} ({b:+.1e})" for n, (a, b) in zip(("fwd", "dx", "dw"), v)) for k, v in res.items()), flush=True)
