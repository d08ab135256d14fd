"""GPU: every bf16x3 plane product of the linear kernels (csrc/linear.hip: k_linear, k_linear_tail, k_linear_wgrad, k_linear_wgrad_tail and
their ROWS / GATE / BIAS builds) and of the narrow convolutions (csrc/conv_narrow.hip: K11n, K12n) arrives in the sum, and the sums are
not one-sided: tests/test_conv_gpu.py's two probes of K11 / K12 on the kernels outside them (tools/plane_products.py builds the operands
and the role tables; tests/test_plane_products_host.py pins the probe's arithmetic on the CPU).

The fp64 bars of the layered steps are a multiple of torch's fp32 error on whole-network gradients, and 1e-6 of the sum of |terms| is met
by a kernel that loses most of its third-order products (K11 did, at 1.6 - 5.0e-7): neither sees a product that is 2^-16 of a term go
missing, nor a cut that is one-sided.  Both probes here do."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

LINEAR_SHAPES = ((512, 256, 256), (384, 1024, 128), (512, 250, 96), (300, 48, 32))           # (M, K, N)
WGRAD_SHAPES = ((2048, 256, 256), (4096, 64, 144), (300, 64, 250))                            # (M, N, K)
DGRAD_NARROW_SHAPES = ((4, 16, 32, 32, 32, 1), (4, 16, 64, 16, 16, 1), (6, 3, 32, 19, 21, 2))      # (B, Ci, Co, H, W, pad)
WGRAD_NARROW_SHAPES = ((16, 16, 32, 32, 32, 1), (5, 3, 32, 19, 21, 0))
CASES = ([("forward", s) for s in LINEAR_SHAPES] + [("dgrad", s) for s in LINEAR_SHAPES[:2]] + [("wgrad", s) for s in WGRAD_SHAPES]
         + [("K11n", s) for s in DGRAD_NARROW_SHAPES] + [("K12n", s) for s in WGRAD_NARROW_SHAPES])
# what each kind's role table must hold: no build drops out of a case unseen
ROLES = {"forward": {"forward", "forward rows"}, "dgrad": {"mode 1", "dx_tanh h=0"}, "K11n": {"K11n"}, "K12n": {"K12n"},
         "wgrad": {"wgrad", "wgrad rows", "wgrad bias", "db", "wgrad bias rows", "db rows"}}


def _probe():
    import plane_products as P
    assert (P.LINEAR_SHAPES, P.WGRAD_SHAPES, P.DGRAD_NARROW_SHAPES, P.WGRAD_NARROW_SHAPES) == (
        LINEAR_SHAPES, WGRAD_SHAPES, DGRAD_NARROW_SHAPES, WGRAD_NARROW_SHAPES)
    return P


def _check_roles(kind, shape, table):
    want = set(ROLES[kind])
    if kind == "wgrad" and shape[2] % 4 != 0:
        want -= {"wgrad bias", "db"}             # the library has no BIAS tail build without rows (aurppo_linear_wgrad_bias_f32 refuses it)
    assert set(table) == want, (kind, shape, sorted(table))


def _check_bias_builds(table):
    """The BIAS builds' dw is the plain builds' bit for bit, and db the fp64 column sum rounded once: half an ulp, 2^-24 of it (the
    kernel's own fp64 sum takes another order: 1e-13 of the column's sum of |terms| covers that)."""
    for dw, plain, db in (("wgrad bias", "wgrad", "db"), ("wgrad bias rows", "wgrad rows", "db rows")):
        if dw in table:
            assert torch.equal(table[dw][0], table[plain][0]), f"{dw} differs from {plain}"
            got, ref, S = table[db]
            assert bool(((got - ref).abs() <= 2.0 ** -24 * ref.abs() + 1e-13 * S).all()), f"{db}: {float((got - ref).abs().max()):.3e}"


@pytest.mark.parametrize("kind,shape", CASES)
def test_every_plane_product_arrives(kind, shape):
    """Operands with KNOWN positive bf16 planes p0 * sum(2^-10k): every third-order product is exactly 2^-20 of every output, so one that
    does not arrive is a mean signed error of -1 x 2^-20 per product.  Bound: |mean| <= 0.05 x 2^-20 per role and variant, the bar
    K11 / K12 are held to (they read -0.003 ... -0.005; the six products summed exactly read 0, or -0.002 with all planes).  The products
    chained through the running accumulator read -0.48 per third-order product at a reduction of 1024 under round-to-nearest alone
    (the host test), and the linear kernels did so chain before they took bf3_gemm.h::mma32x3_step: on the MI355X that build read
    -0.11 / -0.70 per product at K = 256 / 1024 and -0.23 in the weight gradient (-2.1 at K = 1024 with all planes), this one reads
    |mean| <= 0.003 everywhere, K11n and K12n <= 0.004 (profiles/linear_plane_bias.txt)."""
    P = _probe()
    gen = torch.Generator().manual_seed(sum(shape))
    for name, wa, wb in P.VARIANTS:
        table = P.known(kind, shape, wa, wb, gen)
        _check_roles(kind, shape, table)
        res = {r: P.plane_bias(v[0], v[1]) for r, v in table.items() if not r.startswith("db")}
        print(f"\n{kind} {shape} {name}: " + "  ".join(f"{r} {m:+.4f} (max {x:.2f})" for r, (m, x) in res.items()))
        for role, (mean, _) in res.items():
            assert abs(mean) <= 0.05, f"{kind} {shape} {role}, {name}: mean error {mean:+.3f} x 2^-20"
        _check_bias_builds(table)


@pytest.mark.parametrize("kind,shape,sparse", [(k, s, sp) for k, s in CASES for sp in ((False,) if k == "forward" else (False, True))])
def test_sums_are_not_one_sided(kind, shape, sparse):
    """Realistic operands (tanh'd activations, xavier weights, relu'd images, output gradients 1e-4 * exp(randn) per column or channel,
    dense and 80 % sparse) against fp64.  Every element within 1e-6 of its own sum of |terms|, and |mean error| <= 1e-9 of the mean sum of
    |terms|: tests/test_conv_gpu.py::test_k11_and_k12_sums_are_not_one_sided derives that bound for >= 7e4 outputs (an unbiased fp32
    sum stays below 6e-8 / sqrt(7e4) = 2.3e-10; a one-sided cut reads 5e-9), so a role with fewer outputs pools independent draws
    until it has 7e4 (K12n's 4608: 16 draws).  No element is left out.  Measured on the MI355X: the chained linear kernels read -1.2e-9
    ... -5.2e-9 in every role; with every other k-step negated the forward and weight-gradient roles read <= 1e-10 (4e-10 in the one
    short slice, 8e-10 at three k-steps, where two steps stand against one), and the input gradient read 9e-10 ... 1.0e-9 at K = 256 --
    its columns differ in scale, the cut follows a step's largest term, so neighbouring steps do not cancel -- until the two row
    blocks of a wave took opposite signs (csrc/linear_body.h): <= 1e-10.  K11n reads -2e-10 ... -9e-10 (five taps against four)."""
    P = _probe()
    gen = torch.Generator().manual_seed(sum(shape) + 7 * sparse)
    tables = [P.realistic(kind, shape, sparse, gen)]
    n = next(iter(tables[0].values()))[0].numel()
    tables += [P.realistic(kind, shape, sparse, gen) for _ in range(P.draws_for(n) - 1)]
    assert n * len(tables) >= P.POOL
    res = P.sidedness(tables)
    print(f"\n{kind} {shape} {'sparse' if sparse else 'dense'} x{len(tables)}: " + "  ".join(f"{r} {a:.2e} ({b:+.1e})" for r, (a, b) in res.items()))
    for t in tables:
        _check_roles(kind, shape, t)
        _check_bias_builds(t)
    for role, (worst, mean) in res.items():
        assert worst <= 1e-6 and abs(mean) <= 1e-9, f"{kind} {shape} {role}: worst {worst:.2e}, mean {mean:+.2e}"
