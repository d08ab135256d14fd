"""GPU: the small-M forward products of csrc/linear.hip -- k_linear_small (``hip_ops.linear_small_bias_act``) and the paired form
k_linear_pair (``hip_ops.linear_pair_bias_act``: two nets' same-shaped products in one launch) -- against k_linear
(``hip_ops.linear_bias_act``).  A forward result for a row depends on the row's values, the operand copy and the order of the k-steps,
and the small tile (128 rows x 32 or 64 columns) keeps all three: every comparison here is ``torch.equal``, no tolerance anywhere.

T1  the small tile equals ``linear_bias_act``: M of one row, a ragged last wave (33), a ragged last workgroup of the 128-row tile (127,
    129) and one row past k_linear's own 256-row tile (257); inner dimensions of one k-step to 16, a chunk boundary, N of one column
    block to 32; the tail builds at K of 1, 11, 17, 33, 376; with and without tanh, with and without a bias.
T2  the pair equals two single calls, once with one input for both nets (layer 0) and once with two.
T3  the same under guards: x a view inside a NaN-filled buffer whose last row ends the view, the outputs views into NaN-filled
    buffers at a 4-byte (not 16-byte) offset; no guard float is written, the results do not change.
T4  a NaN row and an Inf row stay in their rows: every other row's bits are ``linear_bias_act``'s."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64          # floats of NaN either side of x and of every output
SHIFT = 3           # the outputs start 3 floats past a 16-byte boundary: 4-byte aligned, not 16

MS = [1, 33, 127, 129, 257]
ALIGNED = [(16, 32), (48, 96), (64, 64), (160, 160), (256, 256), (32, 1024)]
TAILS = [(1, 32), (11, 96), (17, 256), (33, 64), (376, 64)]


def _operands(M, K, N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    return g, x, w, b


# ---------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("K,N", ALIGNED + TAILS)
def test_small_tile_equals_linear_bias_act(K, N, M):
    from aur_ppo_amd import hip_ops as H
    _, x, w, b = _operands(M, K, N, 1000 * M + K + N)
    for act in (0, 1):
        for bias in (b, None):
            ref = H.linear_bias_act(x, w, bias, act)
            y = H.linear_small_bias_act(x, w, bias, act)
            assert y.shape == (M, N) and bool(torch.isfinite(y).all())
            assert torch.equal(y, ref), (act, bias is not None, int((y != ref).sum()))


# ---------------------------------------------------------------------------------- T2
PAIR = [(16, 32), (64, 64), (256, 256), (32, 1024), (17, 256), (376, 64)]


@pytest.mark.parametrize("shared", [True, False], ids=["one-input", "two-inputs"])
@pytest.mark.parametrize("M", [1, 129, 257])
@pytest.mark.parametrize("K,N", PAIR)
def test_pair_equals_two_single_calls(K, N, M, shared):
    from aur_ppo_amd import hip_ops as H
    g, xA, wA, bA = _operands(M, K, N, 2000 * M + K + N)
    xC = xA if shared else torch.randn(M, K, device="cuda", generator=g)
    wC = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    bC = torch.randn(N, device="cuda", generator=g)
    for act in (0, 1):
        refA, refC = H.linear_bias_act(xA, wA, bA, act), H.linear_bias_act(xC, wC, bC, act)
        yA, yC = H.linear_pair_bias_act(xA, xC, wA, wC, bA, bC, act)
        assert yA.shape == (M, N) and yC.shape == (M, N)
        assert torch.equal(yA, refA) and torch.equal(yC, refC), (act, int((yA != refA).sum()), int((yC != refC).sum()))
    yA, yC = H.linear_pair_bias_act(xA, xC, wA, wC, None, bC, 1)          # a bias on one net only
    assert torch.equal(yA, H.linear_bias_act(xA, wA, None, 1)) and torch.equal(yC, H.linear_bias_act(xC, wC, bC, 1))
    assert not torch.equal(yA, yC)


# ---------------------------------------------------------------------------------- the two-column-block builds
# A launch takes two column blocks per workgroup (NB = 2) from 512 such workgroups on (bf3_gemm.h::bf3_small_grid), which none of the
# shapes above reaches.  N = 1024 is 16 groups of two blocks: one product needs 32 row tiles (M > 3968), a pair 16 (M > 1920).  Both
# sides of each threshold, with a ragged last tile on the NB = 2 side; the aligned and the tail build.
@pytest.mark.parametrize("K", [32, 17])
def test_the_two_column_block_builds_equal_linear_bias_act(K):
    from aur_ppo_amd import hip_ops as H
    N = 1024
    for M in (3968, 4097):                       # 31 x 16 = 496 workgroups: NB 1; 33 x 16 = 528: NB 2
        _, x, w, b = _operands(M, K, N, 5000 + M + K)
        assert torch.equal(H.linear_small_bias_act(x, w, b, 1), H.linear_bias_act(x, w, b, 1)), M
    for M in (1920, 2049):                       # 2 x 15 x 16 = 480: NB 1; 2 x 17 x 16 = 544: NB 2
        g, xA, wA, bA = _operands(M, K, N, 6000 + M + K)
        xC = torch.randn(M, K, device="cuda", generator=g)
        wC = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
        yA, yC = H.linear_pair_bias_act(xA, xC, wA, wC, bA, None, 1)
        assert torch.equal(yA, H.linear_bias_act(xA, wA, bA, 1)) and torch.equal(yC, H.linear_bias_act(xC, wC, None, 1)), M
    # an odd number of column blocks: the last group's second block is past N (operand slack, nothing stored)
    M, N = 4097, 1056
    g, xA, wA, bA = _operands(M, K, N, 7000 + K)
    assert torch.equal(H.linear_small_bias_act(xA, wA, bA, 0), H.linear_bias_act(xA, wA, bA, 0))
    wC = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    yA, yC = H.linear_pair_bias_act(xA, xA, wA, wC, bA, bA, 0)
    assert torch.equal(yA, H.linear_bias_act(xA, wA, bA, 0)) and torch.equal(yC, H.linear_bias_act(xA, wC, bA, 0))


# ---------------------------------------------------------------------------------- T3
class _Guarded:
    """An (n, w) output as a view into a NaN-filled buffer: GUARD floats, SHIFT more, the view, GUARD floats."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.buf = torch.full((GUARD + SHIFT + n + GUARD + 4,), float("nan"), device="cuda")
        base = (-self.buf.data_ptr() % 16) // 4         # floats to the next 16-byte boundary
        self.lo = base + GUARD + SHIFT
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.view.data_ptr() % 16 != 0 and self.view.data_ptr() % 4 == 0 and self.view.is_contiguous()
        self.n = n

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.lo]).all()) and bool(torch.isnan(self.buf[self.lo + self.n:]).all())


def _guarded_x(M, K, g):
    """x: exactly M rows of exactly K floats at a 16-byte-aligned offset inside a NaN-filled buffer, GUARD floats of NaN either side:
    the last row of x ends the view, and what follows it is NaN."""
    buf = torch.full((GUARD + 4 + M * K + GUARD,), float("nan"), device="cuda")
    lo = (-buf.data_ptr() % 16) // 4 + GUARD
    x = buf[lo:lo + M * K].view(M, K)
    assert x.data_ptr() % 16 == 0 and x.is_contiguous()
    x.copy_(torch.randn(M, K, device="cuda", generator=g))
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + M * K:]).all()) and bool(torch.isfinite(x).all())
    return buf, x


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("K", [17, 64])
@pytest.mark.parametrize("M", [1, 129])
def test_small_and_pair_under_guards(M, K):
    from aur_ppo_amd import _lib, hip_ops as H
    lib = _lib.load()
    N = 96
    g = torch.Generator(device="cuda").manual_seed(3000 * M + K)
    _bufA, xA = _guarded_x(M, K, g)
    _bufC, xC = _guarded_x(M, K, g)
    wA = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    wC = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    bA, bC = torch.randn(N, device="cuda", generator=g), torch.randn(N, device="cuda", generator=g)
    refA, refC = H.linear_bias_act(xA.clone(), wA, bA, 1), H.linear_bias_act(xC.clone(), wC, bC, 1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.aurppo_conv3x3_wop_bytes(K, N), dtype=torch.uint8, device="cuda")
    y = _Guarded(M, N)
    rc = lib.aurppo_linear_small_bias_act_f32(_p(xA), _p(wA), _p(bA), _p(y.view), M, K, N, 1, _p(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and y.guards_intact()
    assert bool(torch.isfinite(y.view).all()) and torch.equal(y.view, refA)
    ws2 = torch.empty(lib.aurppo_linear_pair_wop_bytes(K, N), dtype=torch.uint8, device="cuda")
    yA, yC = _Guarded(M, N), _Guarded(M, N)
    rc = lib.aurppo_linear_pair_bias_act_f32(_p(xA), _p(xC), _p(wA), _p(wC), _p(bA), _p(bC), _p(yA.view), _p(yC.view), M, K, N, 1, _p(ws2), st)
    torch.cuda.synchronize()
    assert rc == 0 and yA.guards_intact() and yC.guards_intact()
    assert torch.equal(yA.view, refA) and torch.equal(yC.view, refC)
    # one input for both nets, as layer 0 of a policy has it
    rc = lib.aurppo_linear_pair_bias_act_f32(_p(xA), _p(xA), _p(wA), _p(wC), _p(bA), _p(bC), _p(yA.view), _p(yC.view), M, K, N, 1, _p(ws2), st)
    torch.cuda.synchronize()
    assert rc == 0 and yA.guards_intact() and yC.guards_intact()
    assert torch.equal(yA.view, refA) and torch.equal(yC.view, H.linear_bias_act(xA.clone(), wC, bC, 1))


# ---------------------------------------------------------------------------------- T4
@pytest.mark.parametrize("M,K,N", [(129, 64, 64), (257, 17, 256), (33, 256, 256)])
def test_non_finite_rows_stay_in_their_rows(M, K, N):
    from aur_ppo_amd import hip_ops as H
    g, x, w, b = _operands(M, K, N, 4000 * M + K + N)
    r_nan, r_inf = M // 3, M - 1
    x[r_nan, K // 2] = float("nan")
    x[r_inf, 0] = float("inf")
    keep = torch.ones(M, dtype=torch.bool, device="cuda")
    keep[r_nan] = keep[r_inf] = False
    wC = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    for act in (0, 1):
        ref = H.linear_bias_act(x, w, b, act)
        refC = H.linear_bias_act(x, wC, None, act)
        y = H.linear_small_bias_act(x, w, b, act)
        yA, yC = H.linear_pair_bias_act(x, x, w, wC, b, None, act)
        for got, want in ((y, ref), (yA, ref), (yC, refC)):
            assert torch.equal(got[keep], want[keep]) and bool(torch.isfinite(got[keep]).all())
            for r in (r_nan, r_inf):
                assert not bool(torch.isfinite(want[r]).all()) and not bool(torch.isfinite(got[r]).all())
