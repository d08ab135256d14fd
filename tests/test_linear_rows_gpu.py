"""GPU: the three additions to csrc/linear.hip's nn.Linear products that the layered PPO step rides on -- rows through the minibatch
index in k_linear and in k_linear_wgrad's x operand, and tanh' of the layer below in k_linear's epilogue.  Each is the plain kernel
with one operand addressed differently (or one more multiply), so each is held to the plain call's BITS on the gathered / un-gated
operands; one shape of each also goes against the fp64 product on tests/test_conv_gpu.py's metric and bound (1e-6 of sum |a b|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _index(M, B, kind, g):
    if kind == "perm":
        return torch.randperm(B, device="cuda", generator=g)[:M].to(torch.int32).contiguous()
    return torch.randint(0, max(1, B // 3), (M,), device="cuda", generator=g).to(torch.int32)


# one row; one short of and one past a workgroup's 256 rows; one k-step; a chunk tail (K = 144: 9 k-steps); NB = 1 / 2 / 4 with a ragged
# last column group (N = 96: 3 blocks, N = 160: 5 blocks)
@pytest.mark.parametrize("kind", ["perm", "repeat"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,K,N", [(1, 16, 32), (255, 16, 96), (257, 64, 256), (1000, 144, 160)])
def test_indexed_forward_equals_the_product_on_gathered_rows(M, K, N, act, kind):
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    B = M + 37
    x = torch.randn(B, K, device="cuda", generator=g)           # exactly B rows: an index past them would read outside the tensor
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    rows = _index(M, B, kind, g)
    y = H.linear_rows_bias_act(x, rows, w, b, act)
    ref = H.linear_bias_act(x[rows.long()].contiguous(), w, b, act)
    assert y.shape == (M, N) and torch.equal(y, ref)


@pytest.mark.parametrize("kind", ["perm", "repeat"])
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (33, 160, 16), (257, 64, 144), (1000, 256, 64)])
def test_indexed_weight_gradient_equals_the_product_on_gathered_rows(M, N, K, kind):
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M + K + N + 1)
    B = M + 37
    x = torch.randn(B, K, device="cuda", generator=g)
    dy = torch.randn(M, N, device="cuda", generator=g)
    rows = _index(M, B, kind, g)
    dw = H.linear_wgrad_rows(dy, x, rows)
    assert dw.shape == (N, K) and torch.equal(dw, H.linear_wgrad(dy, x[rows.long()].contiguous()))


@pytest.mark.parametrize("M,K,N", [(1, 32, 32), (255, 96, 32), (257, 256, 256), (1000, 160, 160)])
def test_tanh_backward_epilogue_equals_product_then_tanh_backward(M, K, N):
    """(gz @ w) * (1 - h * h) in one launch == the mode-1 product followed by aten's tanh_backward, bit for bit (linear.hip is
    compiled without contraction: the epilogue is a multiply, a subtract and a multiply); in place of ``h`` too."""
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(M + K + N + 2)
    gz = torch.randn(M, N, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / N) ** 0.5
    h = torch.tanh(torch.randn(M, K, device="cuda", generator=g))
    out = H.linear_dx_tanh(gz, w, h)
    ref = torch.ops.aten.tanh_backward(H.linear_nobias(gz, w, 1), h)
    assert torch.equal(out, ref)
    h2 = h.clone()
    assert H.linear_dx_tanh(gz, w, h2, out=h2) is h2 and torch.equal(h2, ref)


def test_the_three_against_the_fp64_product():
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator(device="cuda").manual_seed(7)
    M, K, N, B = 1000, 144, 160, 1037
    x = torch.randn(B, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * (1.0 / K) ** 0.5
    rows = _index(M, B, "perm", g)
    xg = x[rows.long()].double()
    y = H.linear_rows_bias_act(x, rows, w, None, 0)
    err = ((y.double() - xg @ w.double().t()).abs() / (xg.abs() @ w.abs().double().t())).max().item()
    print(f"\nindexed forward: {err:.3e} of sum|ab|")
    assert err <= 1e-6
    dy = torch.randn(M, N, device="cuda", generator=g)
    dw = H.linear_wgrad_rows(dy, x, rows)
    err = ((dw.double() - dy.double().t() @ xg).abs() / (dy.abs().double().t() @ xg.abs())).max().item()
    print(f"indexed weight gradient: {err:.3e} of sum|ab|")
    assert err <= 1e-6
    h = torch.tanh(torch.randn(M, K, device="cuda", generator=g))
    gx = H.linear_dx_tanh(dy, w, h)
    dt = 1.0 - h.double() * h.double()
    err = ((gx.double() - (dy.double() @ w.double()) * dt).abs() / ((dy.abs().double() @ w.abs().double()) * dt)).max().item()
    print(f"input gradient with tanh': {err:.3e} of sum|ab| (1 - h^2)")
    assert err <= 1e-6
