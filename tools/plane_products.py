"""How the linear kernels (csrc/linear.hip: k_linear*, k_linear_wgrad*) and the narrow convolutions (csrc/conv_narrow.hip: K11n, K12n) sum
their bf16x3 plane products: tools/conv_plane_bias.py's two probes on every build of those kernels (DESIGN 2.5;
tests/test_plane_products_gpu.py asserts both, tests/test_plane_products_host.py pins the probe's own arithmetic).

  1. Operands with KNOWN positive planes p0 * sum(2^-10k) (conv_plane_bias.planes): every third-order product of csrc/bf16x3.h is
     exactly 2^-20 of every output, so one that does not arrive reads as a mean signed error of -1 in that unit.
  2. Realistic operands (tanh'd activations, xavier weights, relu'd images, output gradients 1e-4 * exp(randn) per column or channel,
     dense and 80 % sparse) against fp64: the worst element over its own sum of |terms|, and the mean error over the mean sum of
     |terms|, where a one-sided cut shows.

A ROLE TABLE maps the name of a kernel build to (got, fp64 reference, fp64 sum of |terms|), all on the CPU; ``*_roles`` build them from
operands of either construction.  ``emulate`` is the same product on the CPU with every 16-wide plane product exact and every addition
rounded to fp32 (nearest even): the chained sum of bf16x3.h::mma32x3 and the per-step sum of bf3_gemm.h::mma32x3_step.

    python tools/plane_products.py >> profiles/linear_plane_bias.txt
    AURPPO_LIB=<another build of the library> python tools/plane_products.py          the parent's build, or tools/build_variant.sh"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import torch.nn.functional as F
import conv_plane_bias as C              # planes(), VARIANTS, UNIT; honours AURPPO_LIB
from conv_plane_bias import UNIT, VARIANTS, planes

H = C.H

# linear forward / input gradient (M, K, N): NB 4; the longest reduction the layered step claims; k_linear_tail, NB 2, a zero-padded
# k-step; NB 1, three k-steps, a ragged row block
LINEAR_SHAPES = ((512, 256, 256), (384, 1024, 128), (512, 250, 96), (300, 48, 32))
# weight gradient (M, N, K): several slices on four tiles; a ragged K tile; the tail build, one short slice
WGRAD_SHAPES = ((2048, 256, 256), (4096, 64, 144), (300, 64, 250))
# K11n (B, Ci, Co, H, W, pad): reduction 288; 576, staged twice; ragged tiles
DGRAD_NARROW_SHAPES = ((4, 16, 32, 32, 32, 1), (4, 16, 64, 16, 16, 1), (6, 3, 32, 19, 21, 2))
WGRAD_NARROW_SHAPES = ((16, 16, 32, 32, 32, 1), (5, 3, 32, 19, 21, 0))
POOL = 7e4                               # outputs behind a mean: fewer, and independent draws are pooled (tests/test_conv_gpu.py's bound)


def split3(x):
    """The three bf16 planes of fp32 ``x`` as fp32 tensors (csrc/bf16x3.h::split3)."""
    b0 = x.bfloat16().float()
    b1 = (x - b0).bfloat16().float()
    b2 = (x - b0 - b1).bfloat16().float()
    return b0, b1, b2


def _perm(x, gen):
    """(xp, rows) with xp[rows] == x: the ROWS builds read their rows through an index."""
    rows = torch.randperm(x.shape[0], generator=gen)
    xp = torch.empty_like(x)
    xp[rows] = x
    return xp, rows.to(torch.int32)


def _mm(a, b):
    """fp64 (a @ b, |a| @ |b|) of fp32 operands."""
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def _cpu(t):
    torch.cuda.synchronize()
    return t.detach().double().cpu()


# ---------------------------------------------------------------------------------------------------------------------- role tables
def forward_roles(x, w, gen, rows_build=True):
    """x (M, K) @ w (N, K).T: k_linear / k_linear_tail, and their ROWS builds through a permutation with a zero bias."""
    ref, S = _mm(x, w.t())
    xg, wg = x.cuda(), w.cuda()
    out = {"forward": (_cpu(H.linear_nobias(xg, wg, 0)), ref, S)}
    if rows_build:
        xp, rows = _perm(x, gen)
        out["forward rows"] = (_cpu(H.linear_rows_bias_act(xp.cuda(), rows.cuda(), wg, torch.zeros(w.shape[0], device="cuda"), 0)), ref, S)
    return out


def dgrad_roles(gy, w, gate_build=True):
    """gy (M, K) @ w (K, N): k_linear mode 1, and the GATE build with h = 0 (its epilogue multiplies by exactly 1)."""
    ref, S = _mm(gy, w)
    gg, wg = gy.cuda(), w.cuda()
    out = {"mode 1": (_cpu(H.linear_nobias(gg, wg, 1)), ref, S)}
    if gate_build:
        out["dx_tanh h=0"] = (_cpu(H.linear_dx_tanh(gg, wg, torch.zeros(gy.shape[0], w.shape[1], device="cuda"))), ref, S)
    return out


def wgrad_roles(gy, x, gen):
    """gy (M, N).T @ x (M, K): k_linear_wgrad / _tail plain and ROWS, and the BIAS builds (no plain one at a K that is no multiple of 4).
    The BIAS builds' entries are (dw, db): ``"db"`` holds (got, fp64 column sum, column sum of |gy|)."""
    ref, S = _mm(gy.t(), x)
    xp, rows = _perm(x, gen)
    gg, xg, xpg, rg = gy.cuda(), x.cuda(), xp.cuda(), rows.cuda()
    out = {"wgrad": (_cpu(H.linear_wgrad(gg, xg)), ref, S), "wgrad rows": (_cpu(H.linear_wgrad_rows(gg, xpg, rg)), ref, S)}
    dbref = (gy.double().sum(0), gy.double().abs().sum(0))
    if x.shape[1] % 4 == 0:
        dw, db = H.linear_wgrad_bias(gg, xg)
        out["wgrad bias"] = (_cpu(dw), ref, S)
        out["db"] = (_cpu(db),) + dbref
    dw, db = H.linear_wgrad_bias(gg, xpg, rg)
    out["wgrad bias rows"] = (_cpu(dw), ref, S)
    out["db rows"] = (_cpu(db),) + dbref
    return out


def dgrad_narrow_roles(g, w, pad):
    """K11n: the input gradient of conv2d(x, w (Co, Ci, 3, 3), padding=pad) under g (B, Co, Ho, Wo)."""
    B, Co, Ho, Wo = g.shape
    shape = (B, w.shape[1], Ho + 2 - 2 * pad, Wo + 2 - 2 * pad)
    ref = torch.nn.grad.conv2d_input(shape, w.double(), g.double(), padding=pad)
    S = torch.nn.grad.conv2d_input(shape, w.double().abs(), g.double().abs(), padding=pad)
    return {"K11n": (_cpu(H.conv3x3_dgrad_narrow(g.cuda(), w.cuda(), pad)), ref, S)}


def wgrad_narrow_ref(g, x, pad):
    """fp64 (dw, sum of |terms|): dw[o][c, tap] = sum over images and output pixels of g[b, o, px] * patch[b, (c, tap), px], one matrix
    product over the unfolded patches (torch.nn.grad.conv2d_weight in fp64 gives the same sums, the host test holds them together, at
    0.1 s a call where a pooled case makes 32)."""
    shape = (g.shape[1], x.shape[1], 3, 3)
    cols, gd = F.unfold(x.double(), 3, padding=pad), g.double().flatten(2)
    return (torch.einsum("bol,bkl->ok", gd, cols).reshape(shape), torch.einsum("bol,bkl->ok", gd.abs(), cols.abs()).reshape(shape))


def wgrad_narrow_roles(g, x, pad):
    """K12n: the weight gradient of conv2d(x (B, Ci, H, W), w (Co, Ci, 3, 3), padding=pad) under g."""
    return {"K12n": (_cpu(H.conv3x3_wgrad_narrow(g.cuda(), x.cuda(), g.shape[1], pad)),) + wgrad_narrow_ref(g, x, pad)}


# ------------------------------------------------------------------------------------------------------- known positive planes
def known(kind, shape, wa, wb, gen):
    """The role table of ``kind`` at ``shape`` on known positive planes: the data operand (x, gy, dy) holds the planes ``wa``, the other
    one (w; x for a weight gradient) the planes ``wb``."""
    if kind == "forward":
        M, K, N = shape
        return forward_roles(planes((M, K), gen, wa), planes((N, K), gen, wb), gen)
    if kind == "dgrad":
        M, K, N = shape
        return dgrad_roles(planes((M, K), gen, wa), planes((K, N), gen, wb))
    if kind == "wgrad":
        M, N, K = shape
        return wgrad_roles(planes((M, N), gen, wa), planes((M, K), gen, wb), gen)
    B, Ci, Co, Hh, Ww, pad = shape
    g = planes((B, Co, Hh + 2 * pad - 2, Ww + 2 * pad - 2), gen, wa)
    if kind == "K11n":
        return dgrad_narrow_roles(g, planes((Co, Ci, 3, 3), gen, wb), pad)
    assert kind == "K12n", kind
    return wgrad_narrow_roles(g, planes((B, Ci, Hh, Ww), gen, wb), pad)


def plane_bias(got, ref):
    """(mean signed relative error, max |.|) in units of 2^-20."""
    rel = (got - ref) / ref
    return float(rel.mean()) / UNIT, float(rel.abs().max()) / UNIT


# ----------------------------------------------------------------------------------------------------------- realistic operands
def _xavier(n_out, n_in, gen):
    return torch.randn(n_out, n_in, generator=gen) * (2.0 / (n_in + n_out)) ** 0.5


def _out_grad(shape, sparse, gen):
    """1e-4 * exp(randn) per column (2-d) or per image and channel (4-d) times randn, 80 % of it zero when ``sparse``."""
    scale = torch.randn((1, shape[1]) if len(shape) == 2 else shape[:2] + (1, 1), generator=gen)
    g = torch.randn(shape, generator=gen) * 1e-4 * torch.exp(scale)
    return g * (torch.rand(shape, generator=gen) < 0.2) if sparse else g


def realistic(kind, shape, sparse, gen):
    """The role table of ``kind`` at ``shape`` on realistic operands (``sparse``: the output gradient; the forward product has none)."""
    if kind == "forward":
        M, K, N = shape
        return forward_roles(torch.tanh(torch.randn(M, K, generator=gen)), _xavier(N, K, gen), gen)
    if kind == "dgrad":
        M, K, N = shape
        return dgrad_roles(_out_grad((M, K), sparse, gen), _xavier(K, N, gen))
    if kind == "wgrad":
        M, N, K = shape
        return wgrad_roles(_out_grad((M, N), sparse, gen), torch.tanh(torch.randn(M, K, generator=gen)), gen)
    B, Ci, Co, Hh, Ww, pad = shape
    g = _out_grad((B, Co, Hh + 2 * pad - 2, Ww + 2 * pad - 2), sparse, gen)
    if kind == "K11n":
        return dgrad_narrow_roles(g, torch.randn(Co, Ci, 3, 3, generator=gen) * (2.0 / (9 * Ci + 9 * Co)) ** 0.5, pad)
    assert kind == "K12n", kind
    return wgrad_narrow_roles(g, torch.relu(torch.randn(B, Ci, Hh, Ww, generator=gen)), pad)


def draws_for(n_outputs):
    """Independent draws whose outputs together number at least POOL."""
    return max(1, math.ceil(POOL / n_outputs))


def sidedness(tables):
    """Per role over the pooled draws ``tables`` (a list of role tables): (worst |error| of an element over its own sum of |terms|,
    mean error over the mean sum of |terms|).  An element whose sum of |terms| is 0 must be exactly 0: it counts as 0 or as inf."""
    out = {}
    for role in tables[0]:
        if role.startswith("db"):
            continue
        err = torch.cat([(t[role][0] - t[role][1]).reshape(-1) for t in tables])
        S = torch.cat([t[role][2].reshape(-1) for t in tables])
        rel = torch.where(S > 0, err.abs() / S.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())
        out[role] = (float(rel.max()), float(err.mean() / S.mean()))
    return out


# ------------------------------------------------------------------------------------------------------------- CPU emulation
def slices_for(tiles, most):
    """csrc/conv.hip::slices_for."""
    most = min(max(most, 1), 4096)
    best, best_util = 1, 0.0
    S = 1
    while S <= most and tiles * S <= 4 * 512:
        rounds = (tiles * S + 511) // 512
        util = tiles * S / (rounds * 512)
        if util > best_util + 0.02:
            best_util, best = util, S
        S += 1
    return best


def wgrad_rows_per_slice(M, N, K):
    """csrc/linear.hip::linear_wgrad_impl's slice: whole 32-row chunks."""
    S0 = slices_for(((N + 127) // 128) * ((K + 127) // 128), (M + 255) // 256)
    return ((M + S0 - 1) // S0 + 31) // 32 * 32


def six_products(pa, pb, drop=()):
    """fp64 sum of the six plane products bf16x3.h keeps, of planes ``pa`` (M, K) and ``pb`` (K, N), without those in ``drop``."""
    keep = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
    return sum(pa[i].double() @ pb[j].double() for i, j in keep if (i, j) not in drop)


def emulate(a, b, per_step, rows_per_slice=None):
    """a (M, K) @ b (K, N) as the kernels sum it, on the CPU: every 16-wide plane product exact (fp64 holds it), every addition rounded
    to fp32, nearest even.  ``per_step``: the step's six products from zero, then one addition to the accumulator (mma32x3_step; under
    nearest-even rounding its alternating sign changes nothing); otherwise all six chained through the accumulator (mma32x3).
    ``rows_per_slice``: the reduction is cut into slices that start from zero and are added in order, in fp32 (the weight gradient)."""
    pa, pb = split3(a), split3(b)
    K = a.shape[1]
    order = [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]
    rnd = lambda t: t.float().double()      # noqa: E731
    total = None
    for lo in range(0, K, rows_per_slice or K):
        acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float64)
        for k in range(lo, min(K, lo + (rows_per_slice or K)), 16):
            t = torch.zeros_like(acc) if per_step else acc
            for i, j in order:
                t = rnd(t + pa[i][:, k:k + 16].double() @ pb[j][k:k + 16].double())
            acc = rnd(acc + t) if per_step else t
        total = acc if total is None else rnd(total + acc)
    return total


# ------------------------------------------------------------------------------------------------------------------- printout
KINDS = (("forward", LINEAR_SHAPES), ("dgrad", LINEAR_SHAPES[:2]), ("wgrad", WGRAD_SHAPES), ("K11n", DGRAD_NARROW_SHAPES),
         ("K12n", WGRAD_NARROW_SHAPES))

if __name__ == "__main__":
    print(f"library: {os.environ.get('AURPPO_LIB', 'default build')}")
    gen = torch.Generator().manual_seed(0)
    print("== known positive planes: mean signed error (max |.|) in units of 2^-20; a missing third-order product reads -1")
    for kind, shapes in KINDS:
        for shape in shapes:
            for name, wa, wb in VARIANTS:
                t = known(kind, shape, wa, wb, gen)
                print(f"{kind:8s}{str(shape):26s} {name:32s} " + "  ".join(
                    "{} {:+.3f} ({:.2f})".format(r, *plane_bias(v[0], v[1])) for r, v in t.items() if not r.startswith("db")), flush=True)
    print("== realistic operands against fp64: worst element / its sum|terms| (mean error / mean sum|terms|), draws pooled to 7e4 outputs")
    for kind, shapes in KINDS:
        for shape in shapes:
            for sparse in ((False,) if kind == "forward" else (False, True)):
                first = realistic(kind, shape, sparse, gen)
                n = next(iter(first.values()))[0].numel()
                tables = [first] + [realistic(kind, shape, sparse, gen) for _ in range(draws_for(n) - 1)]
                print(f"{kind:8s}{str(shape):26s} {'sparse' if sparse else 'dense ':6s} x{len(tables):<3d}" + "  ".join(
                    f"{r} {a:.2e} ({b:+.1e})" for r, (a, b) in sidedness(tables).items()), flush=True)
