"""CPU: the plane-product probe itself (tools/plane_products.py).  tests/test_plane_products_gpu.py holds the linear and narrow-convolution
kernels to |mean signed error| <= 0.05 x 2^-20 on operands with known positive planes; this file pins what that figure means, with a
right arithmetic and a wrong one both on record: the planes split as claimed, the six products of csrc/bf16x3.h summed exactly read 0
(-0.002 with all planes: the three products the header drops by design), one third-order product less reads -1, a per-k-step sum rounded
to fp32 (bf3_gemm.h::mma32x3_step) stays inside the bound at every linear shape of the GPU file, and the sum chained through the running
accumulator (bf16x3.h::mma32x3) does not at a reduction of 1024 -- with round-to-nearest, before the matrix pipe's truncation adds to it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plane_products as P  # noqa: E402

THIRD = {0: [(2, 0)], 1: [(0, 2)], 2: [(1, 1)], 3: [(0, 2), (2, 0), (1, 1)]}        # the third-order products each variant holds
DROPPED = -(2 * 2.0 ** -30 + 2.0 ** -40) / (1 + 2.0 ** -10 + 2.0 ** -20) ** 2 / P.UNIT      # a1*b2 + a2*b1 + a2*b2 of all planes: -0.00195


def _operands(v, M=96, K=256, N=80, seed=0):
    gen = torch.Generator().manual_seed(seed + v)
    _, wa, wb = P.VARIANTS[v]
    return P.planes((M, K), gen, wa), P.planes((K, N), gen, wb)


@pytest.mark.parametrize("which", [(0,), (0, 1), (0, 1, 2)])
def test_planes_split_exactly_as_claimed(which):
    x = P.planes((64, 48), torch.Generator().manual_seed(len(which)), which)
    b = P.split3(x)
    p0 = b[0].double()
    m, _ = torch.frexp(p0)                                              # p0 = (1 + j / 8) * 2^e > 0: three mantissa bits under the leading one
    assert torch.equal(m * 16, (m * 16).round()) and bool((p0 > 0).all())
    for k in range(3):
        assert torch.equal(b[k].double(), p0 * 2.0 ** (-10 * k) if k in which else torch.zeros_like(p0))
    assert torch.equal((b[0].double() + b[1].double() + b[2].double()), x.double())


@pytest.mark.parametrize("v", range(4))
def test_the_six_products_summed_exactly_read_zero(v):
    a, b = _operands(v)
    ref = a.double() @ b.double()
    mean, worst = P.plane_bias(P.six_products(P.split3(a), P.split3(b)), ref)
    print(f"\n{P.VARIANTS[v][0]}: six products in fp64 {mean:+.5f} (max {worst:.5f})")
    assert abs(mean - (DROPPED if v == 3 else 0.0)) <= 1e-6 and worst <= 0.002


@pytest.mark.parametrize("v", range(4))
def test_one_third_order_product_less_reads_minus_one(v):
    a, b = _operands(v)
    ref = a.double() @ b.double()
    for drop in THIRD[v]:
        mean, _ = P.plane_bias(P.six_products(P.split3(a), P.split3(b), drop=(drop,)), ref)
        print(f"\n{P.VARIANTS[v][0]} without a{drop[0]}*b{drop[1]}: {mean:+.5f}")
        assert abs(mean + 1.0) <= 0.002


def _emulated(kind, shape, v, per_step):
    gen = torch.Generator().manual_seed(sum(shape) + v)
    _, wa, wb = P.VARIANTS[v]
    if kind == "forward":
        M, K, N = shape
        a, b, rps = P.planes((M, K), gen, wa), P.planes((N, K), gen, wb).t(), None
    else:
        M, N, K = shape
        a, b, rps = P.planes((M, N), gen, wa).t(), P.planes((M, K), gen, wb), P.wgrad_rows_per_slice(M, N, K)
    return P.plane_bias(P.emulate(a, b, per_step, rps), a.double() @ b.double())


@pytest.mark.parametrize("kind,shape", [("forward", s) for s in P.LINEAR_SHAPES] + [("wgrad", s) for s in P.WGRAD_SHAPES])
def test_the_emulated_per_step_sum_stays_inside_the_bound(kind, shape):
    for v in range(4):
        mean, worst = _emulated(kind, shape, v, True)
        print(f"\n{kind} {shape} {P.VARIANTS[v][0]}: per-step sum, nearest even {mean:+.4f} (max {worst:.2f})")
        assert abs(mean) <= 0.05


def test_the_emulated_chain_leaves_the_bound_at_a_reduction_of_1024():
    for v in range(4):
        mean, worst = _emulated("forward", P.LINEAR_SHAPES[1], v, False)
        print(f"\nforward {P.LINEAR_SHAPES[1]} {P.VARIANTS[v][0]}: chained sum, nearest even {mean:+.4f} (max {worst:.2f})")
        assert mean < -0.05


@pytest.mark.parametrize("B,Ci,Co,H,W,pad", [(2, 3, 32, 9, 11, 0), (2, 16, 32, 8, 8, 1), (1, 5, 7, 6, 5, 2)])
def test_the_unfolded_weight_gradient_is_the_convolutions(B, Ci, Co, H, W, pad):
    gen = torch.Generator().manual_seed(B + Ci + H)
    x, g = torch.randn(B, Ci, H, W, generator=gen), torch.randn(B, Co, H + 2 * pad - 2, W + 2 * pad - 2, generator=gen)
    ref, S = P.wgrad_narrow_ref(g, x, pad)
    want = torch.nn.grad.conv2d_weight(x.double(), (Co, Ci, 3, 3), g.double(), padding=pad)
    wantS = torch.nn.grad.conv2d_weight(x.double().abs(), (Co, Ci, 3, 3), g.double().abs(), padding=pad)
    assert bool(((ref - want).abs() <= 1e-14 * wantS).all()) and bool(((S - wantS).abs() <= 1e-14 * wantS).all())


def test_the_slice_rule_is_the_librarys():
    """wgrad_rows_per_slice mirrors csrc/linear.hip: whole 32-row chunks, at least 8 of them a slice unless M is shorter."""
    assert P.LINEAR_SHAPES[1][1] == 1024
    for M, N, K in P.WGRAD_SHAPES:
        rps = P.wgrad_rows_per_slice(M, N, K)
        assert rps % 32 == 0 and (rps >= 256 or rps >= M)
