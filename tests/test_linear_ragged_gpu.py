"""GPU: csrc/linear.hip's nn.Linear products at an inner dimension that is no multiple of 16 (forward: k_linear_tail, plain and through
the minibatch index, from k_linear_prep_tail's zero-padded operand copy) or of 4 (weight gradient: k_linear_wgrad_tail, its x operand).

T1  bit equality with the aligned kernels on zero-padded operands: the k-steps and their order are the same and the padded columns are
    zero planes in both operands, so the accumulators see the same sequence.
T2  the same under guards: x is a (B, K) view inside a NaN-filled buffer whose every row the index does not name is NaN too, its last
    row named; outputs are views into NaN-filled buffers.  A tail that loads past a row and relies on the zero weights gives NaN.
T3  one ragged shape of each product, and linear_dx_tanh behind them, against the fp64 product on
    tests/test_linear_rows_gpu.py::test_the_three_against_the_fp64_product's metric and bound (1e-6 of sum |a b|)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64          # floats of NaN either side of x and of every output
SHIFT = 3           # the outputs start 3 floats past a 16-byte boundary: 4-byte aligned, not 16

# K = 1: one live lane half; 11: the Hopper row, a tail inside the second lane half; 17: a full k-step plus one column, rows off
# 16-byte alignment; 20: a multiple of 4 but not of 16; 33: a staged chunk of two k-steps plus one column; 376: a tail of exactly one
# lane half
FWD = [(1, 1, 32), (255, 11, 96), (257, 17, 256), (33, 20, 160), (257, 33, 64), (1000, 376, 64)]
WGRAD = [(1, 64, 1), (33, 160, 11), (257, 64, 17), (1000, 256, 27), (300, 64, 129), (257, 64, 376)]


def _index(M, B, kind, g):
    if kind == "perm":
        return torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    return torch.randint(0, max(1, B // 3), (M,), device="cuda", generator=g).to(torch.int32)


def _pad(t):
    """The inner dimension zero-filled to the next multiple of 16."""
    K = t.shape[1]
    return torch.nn.functional.pad(t, (0, -K % 16)).contiguous()


# ---------------------------------------------------------------------------------- T1
@pytest.mark.parametrize("kind", ["perm", "repeat"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,K,N", FWD)
def test_ragged_forward_equals_the_aligned_kernel_on_padded_operands(M, K, N, act, kind):
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    B = M + 37
    x = torch.randn(B, K, device="cuda", generator=g)           # exactly B rows of exactly K floats
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    rows = _index(M, B, kind, g)
    xg = x[rows.long()].contiguous()
    ref = H.linear_bias_act(_pad(xg), _pad(w), b, act)
    y_rows = H.linear_rows_bias_act(x, rows, w, b, act)
    y_plain = H.linear_bias_act(xg, w, b, act)
    assert y_rows.shape == (M, N) and torch.equal(y_rows, ref)
    assert y_plain.shape == (M, N) and torch.equal(y_plain, ref)


@pytest.mark.parametrize("kind", ["perm", "repeat"])
@pytest.mark.parametrize("M,N,K", WGRAD)
def test_ragged_weight_gradient_equals_the_aligned_kernel_on_padded_x(M, N, K, kind):
    """ceil(K / 128) is unchanged by the padding, so the tiles and the slice count are too."""
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M + K + N + 1)
    B = M + 37
    x = torch.randn(B, K, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    rows = _index(M, B, kind, g)
    xg = x[rows.long()].contiguous()
    ref = H.linear_wgrad(dy, _pad(xg))[:, :K]
    dw_rows = H.linear_wgrad_rows(dy, x, rows)
    dw_plain = H.linear_wgrad(dy, xg)
    assert dw_rows.shape == (N, K) and torch.equal(dw_rows, ref)
    assert dw_plain.shape == (N, K) and torch.equal(dw_plain, ref)


# ---------------------------------------------------------------------------------- T2
class _Guarded:
    """An (n,) or (n, w) output as a view into a NaN-filled buffer: GUARD floats, SHIFT more, the view, GUARD floats."""

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


def _guarded_x(B, K, rows, g):
    """(buffer, x): x a (B, K) view at a 16-byte-aligned offset inside a NaN-filled buffer, GUARD floats of NaN either side; the rows the
    index names hold numbers, every other row NaN."""
    buf = torch.full((GUARD + 4 + B * K + GUARD,), float("nan"), device="cuda")
    lo = (-buf.data_ptr() % 16) // 4 + GUARD
    x = buf[lo:lo + B * K].view(B, K)
    assert x.data_ptr() % 16 == 0 and x.is_contiguous()
    named = torch.unique(rows.long())
    x[named] = torch.randn(named.numel(), K, device="cuda", generator=g)
    assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + B * K:]).all())
    assert int(torch.isnan(x).any(1).sum()) == B - named.numel()
    return buf, x


def _index_naming_the_last_row(M, B, g):
    rows = _index(M, B, "perm", g)
    rows[M // 2] = B - 1
    return rows


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("M,K,N", FWD)
def test_ragged_forward_under_guards(M, K, N):
    from aur_ppo_amd import _lib, hip_ops as H
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M + K + N + 3)
    B = M + 37
    rows = _index_naming_the_last_row(M, B, g)
    _buf, x = _guarded_x(B, K, rows, g)
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    xg = x[rows.long()].contiguous()
    assert bool(torch.isfinite(xg).all())
    ref = H.linear_bias_act(_pad(xg), _pad(w), b, 1)
    ws = torch.empty(lib.aurppo_conv3x3_wop_bytes(K, N), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = _Guarded(M, N)
    rc = lib.aurppo_linear_rows_bias_act_f32(_p(x), _p(rows), _p(w), _p(b), _p(y.view), M, K, N, 1, _p(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and y.guards_intact()
    assert bool(torch.isfinite(y.view).all()) and torch.equal(y.view, ref)
    # plain addressing: the last M rows of a buffer of its own kind, so the last row of x is the last row of the product
    rows_all = torch.arange(B, device="cuda", dtype=torch.int32)
    _buf2, x2 = _guarded_x(B, K, rows_all, g)
    ref2 = H.linear_bias_act(_pad(x2), _pad(w), b, 1)
    y2 = _Guarded(B, N)
    rc = lib.aurppo_linear_bias_act_f32(_p(x2), _p(w), _p(b), _p(y2.view), B, K, N, 1, _p(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and y2.guards_intact()
    assert bool(torch.isfinite(y2.view).all()) and torch.equal(y2.view, ref2)


@pytest.mark.parametrize("M,N,K", WGRAD)
def test_ragged_weight_gradient_under_guards(M, N, K):
    from aur_ppo_amd import _lib, hip_ops as H
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(M + K + N + 4)
    B = M + 37
    rows = _index_naming_the_last_row(M, B, g)
    _buf, x = _guarded_x(B, K, rows, g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    xg = x[rows.long()].contiguous()
    ref = H.linear_wgrad(dy, _pad(xg))[:, :K]
    ws = torch.empty(lib.aurppo_linear_wgrad_ws_bytes(M, N, K), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dw = _Guarded(N, K)
    rc = lib.aurppo_linear_wgrad_rows_f32(_p(dy), _p(x), _p(rows), _p(dw.view), M, N, K, _p(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and dw.guards_intact()
    assert bool(torch.isfinite(dw.view).all()) and torch.equal(dw.view, ref)
    # plain addressing over a guarded x of exactly M rows
    rows_all = torch.arange(M, device="cuda", dtype=torch.int32)
    _buf2, x2 = _guarded_x(M, K, rows_all, g)
    ref2 = H.linear_wgrad(dy, _pad(x2))[:, :K]
    dw2 = _Guarded(N, K)
    rc = lib.aurppo_linear_wgrad_f32(_p(dy), _p(x2), _p(dw2.view), M, N, K, _p(ws), st)
    torch.cuda.synchronize()
    assert rc == 0 and dw2.guards_intact()
    assert bool(torch.isfinite(dw2.view).all()) and torch.equal(dw2.view, ref2)


# ---------------------------------------------------------------------------------- T3
def test_the_three_against_the_fp64_product_at_a_ragged_width():
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(7)
    M, K, N, B = 1000, 27, 160, 1037
    x = torch.randn(B, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    rows = _index(M, B, "perm", g)
    xg = x[rows.long()].double()
    y = H.linear_rows_bias_act(x, rows, w, None, 0)
    err = ((y.double() - xg @ w.double().t()).abs() / (xg.abs() @ w.abs().double().t())).max().item()
    print(f"\nragged indexed forward: {err:.3e} of sum|ab|")
    assert err <= 1e-6
    dy = torch.randn(M, N, device="cuda", generator=g)
    dw = H.linear_wgrad_rows(dy, x, rows)
    err = ((dw.double() - dy.double().t() @ xg).abs() / (dy.abs().double().t() @ xg.abs())).max().item()
    print(f"ragged indexed weight gradient: {err:.3e} of sum|ab|")
    assert err <= 1e-6
    h = torch.tanh(torch.randn(M, K, device="cuda", generator=g))
    gx = H.linear_dx_tanh(dy, w, h)
    dt = 1.0 - h.double() * h.double()
    err = ((gx.double() - (dy.double() @ w.double()) * dt).abs() / ((dy.abs().double() @ w.abs().double()) * dt)).max().item()
    print(f"input gradient with tanh' behind a ragged layer: {err:.3e} of sum|ab| (1 - h^2)")
    assert err <= 1e-6
