"""GPU: the encoder kernels (K9, K10: csrc/pool.hip; K11, K12, k_fold_slices: csrc/conv.hip) at the smallest shapes at which each of
their branches can go wrong, called through the C ABI so that every tensor is a view the test owns:

* every input is a view of exactly its size inside a NaN-filled buffer, every output a NaN-filled view between guards, 3 floats past a
  16-byte boundary wherever the entry point does not ask for alignment (tests/encoder_cases.py::Guarded);
* every workspace is exactly aurppo_conv3x3_wop_bytes / aurppo_conv3x3_wgrad_ws_bytes long and poisoned: K11 reads a slack group of the
  operand copy that k_conv_prep never wrote, K12 stages rows past the tensor from wherever offset 0 lands -- neither may reach an output;
* afterwards the guards are intact, every output element has been written, and the values meet the bounds the project already has
  (K11 / K12: 1e-6 of the sum of |products| against fp64, tests/test_conv_gpu.py; K9: bit equality with torch's fp32 op chain; K10: the
  tolerances of tests/test_hip_parity.py against the same MIOpen-free torch reference).

The second half places one NaN / +Inf / -Inf: K9 and K10 must propagate it as torch's relu and max_pool2d do (forward and routing),
K11 and K12 must have non-finite outputs exactly where the fp64 reference has them -- element 0 of either operand included, which is
what K12's rows past the tensor read."""
import pytest
import torch
import torch.nn.functional as F

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

BOUND = 1e-6        # of the sum of |products| behind an element (tests/test_conv_gpu.py)


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


def _gen(*shape_key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * int(v) for i, v in enumerate(shape_key)) + 17)


# =================================================================================================================== K11
def _k11_operands(shape, mode, g):
    """x, w as the entry point takes them, plus its integer arguments and the fp64 reference / scale of the output."""
    B, cin, cout, H, W, p = shape
    x = torch.randn(B, cin, H, W, device="cuda", generator=g)
    if mode == 0:
        w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
        args = (B, cin, cout, H, W, p, 0)
    else:                      # the filter of the forward layer whose input gradient this product is: (Co_w = cin, Ci_w = cout)
        w = torch.randn(cin, cout, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
        args = (B, cout, cin, H, W, 2 - p, 1)
    return x, w, args


def _k11_reference(x, w, shape, mode):
    p = shape[5]
    if mode == 0:
        return E.conv64(x, w, p), E.conv64(x.abs(), w.abs(), p)
    return E.dgrad64(x, w, 2 - p), E.dgrad64(x.abs(), w.abs(), 2 - p)


def _k11_call(lib, x, w, shape, args):
    B, cin, cout, H, W, p = shape
    gx, gw = E.Guarded(*x.shape, like=x), E.Guarded(*w.shape, like=w)
    z = E.Guarded(B, cout, H + 2 * p - 2, W + 2 * p - 2)
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(cin, cout))
    rc = lib.aurppo_conv3x3_f32(E.ptr(gx.view), E.ptr(gw.view), E.ptr(z.view), *args, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert z.guards_intact() and ws.guards_intact() and gx.guards_intact() and gw.guards_intact()
    return z


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", E.K11_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k11_under_guards_meets_the_fp64_convolution(lib, shape, mode):
    g = _gen(*shape, mode)
    x, w, args = _k11_operands(shape, mode, g)
    z = _k11_call(lib, x, w, shape, args)
    ref, mag = _k11_reference(x, w, shape, mode)
    assert z.view.shape == ref.shape and z.written()
    err = E.rel_err(z.view, ref, mag)
    print(f"\nK11 mode {mode} {shape}: {err:.3e} of sum|ab|")
    assert err <= BOUND


def _place(t, where, value):
    """One ``value`` at element 0, the last element or an interior element of the flattened tensor."""
    n = t.numel()
    at = {"first": 0, "last": n - 1, "interior": n // 2 + n // 7}[where]
    t.view(-1)[at] = value
    return t


def _same_non_finite_set_and_bound(got, ref, mag, what):
    bad_ref = ~torch.isfinite(ref)
    bad_got = ~torch.isfinite(got)
    assert bool(bad_ref.any()), f"{what}: the reference has no non-finite output: the case checks nothing"
    assert torch.equal(bad_got, bad_ref), (f"{what}: {int(bad_got.sum())} non-finite outputs, the fp64 reference has {int(bad_ref.sum())}; "
                                           f"{int((bad_got & ~bad_ref).sum())} extra, {int((~bad_got & bad_ref).sum())} missing")
    ok = ~bad_ref
    if bool(ok.any()):
        err = float(((got.double() - ref).abs()[ok] / mag[ok].clamp_min(1e-30)).max())
        print(f"\n{what}: finite outputs {err:.3e} of sum|ab|, {int(bad_ref.sum())} non-finite")
        assert err <= BOUND, what


NONFINITE_K11 = [(3, 48, 80, 6, 5, 1), (2, 16, 160, 7, 6, 0)]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first", "last", "interior"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", NONFINITE_K11, ids=lambda s: "x".join(map(str, s)))
def test_k11_non_finite_outputs_are_the_fp64_references(lib, shape, mode, where, value):
    g = _gen(*shape, mode, 5)
    x, w, args = _k11_operands(shape, mode, g)
    _place(x, where, value)
    z = _k11_call(lib, x, w, shape, args)
    ref, mag = _k11_reference(x, w, shape, mode)
    _same_non_finite_set_and_bound(z.view, ref, mag, f"K11 mode {mode} {shape} {value} at {where}")


# =================================================================================================================== K12
def _k12_call(lib, x, dy, shape):
    B, Ci, Co, H, W, pad = shape
    plan = E.k12_plan(*shape)
    gx = E.Guarded(*x.shape, like=x)
    gdy = E.Guarded(*dy.shape, like=dy, aligned=plan["quad"])      # (an unaligned dy would turn a QUAD shape into the other build)
    dw = E.Guarded(Co, Ci, 3, 3)
    nbytes = lib.aurppo_conv3x3_wgrad_ws_bytes(*shape)
    assert E.k12_slices_from_ws(nbytes, Ci, Co) == plan["S"]
    ws = E.Workspace(nbytes)
    rc = lib.aurppo_conv3x3_wgrad_f32(E.ptr(gdy.view), E.ptr(gx.view), E.ptr(dw.view), *shape, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert dw.guards_intact() and ws.guards_intact() and gx.guards_intact() and gdy.guards_intact()
    return dw


def _k12_operands(shape, g):
    B, Ci, Co, H, W, pad = shape
    x = torch.randn(B, Ci, H, W, device="cuda", generator=g)
    dy = torch.randn(B, Co, H + 2 * pad - 2, W + 2 * pad - 2, device="cuda", generator=g)
    return x, dy


@pytest.mark.parametrize("shape", E.K12_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k12_under_guards_meets_the_fp64_weight_gradient(lib, shape):
    g = _gen(*shape)
    x, dy = _k12_operands(shape, g)
    dw = _k12_call(lib, x, dy, shape)
    Co, pad = shape[2], shape[5]
    ref, mag = E.wgrad64(x, dy, Co, pad), E.wgrad64(x.abs(), dy.abs(), Co, pad)
    assert dw.written()
    err = E.rel_err(dw.view, ref, mag)
    print(f"\nK12 {shape}: {err:.3e} of sum|ab|")
    assert err <= BOUND


NONFINITE_K12 = [(5, 16, 65, 4, 4, 1), (2, 16, 160, 5, 5, 1), (37, 16, 64, 12, 12, 1)]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first", "last", "interior"])
@pytest.mark.parametrize("operand", ["x", "dy"])
@pytest.mark.parametrize("shape", NONFINITE_K12, ids=lambda s: "x".join(map(str, s)))
def test_k12_non_finite_outputs_are_the_fp64_references(lib, shape, operand, where, value):
    g = _gen(*shape, 9)
    x, dy = _k12_operands(shape, g)
    _place(x if operand == "x" else dy, where, value)
    dw = _k12_call(lib, x, dy, shape)
    Co, pad = shape[2], shape[5]
    ref, mag = E.wgrad64(x, dy, Co, pad), E.wgrad64(x.abs(), dy.abs(), Co, pad)
    _same_non_finite_set_and_bound(dw.view, ref, mag, f"K12 {shape} {value} in {operand} at {where}")


# =================================================================================================================== K9
def _k9_reference(x, bias, scale, plane, w):
    """torch's fp32 op chain in base_encoder.forward_split's association, (conv + state * plane) + bias, and its gradients under the
    output gradient w: y, dx, dbias, dplane."""
    leaves = [t.clone().requires_grad_(True) for t in (x, bias)] + ([plane.clone().requires_grad_(True)] if plane is not None else [])
    pre = ((leaves[0] + scale.view(-1, 1, 1, 1) * leaves[2]) if plane is not None else leaves[0]) + leaves[1].view(1, -1, 1, 1)
    y = F.max_pool2d(F.relu(pre), 2)
    y.backward(w)
    return y.detach(), leaves[0].grad, leaves[1].grad, (leaves[2].grad if plane is not None else None)


def _k9_call(lib, x, bias, scale, plane, w, aligned, plane_aligned=None):
    """Forward and backward through the C ABI; ``aligned`` puts x and dx at 16-byte boundaries (the float4 paths for a W that is a
    multiple of 4), otherwise 3 floats past one (the scalar paths); ``plane_aligned`` the plane (default: as x) -- the forward's ``vec``
    test needs both."""
    plane_aligned = aligned if plane_aligned is None else plane_aligned
    B, C_, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    gx = E.Guarded(B, C_, H, W, like=x, aligned=aligned)
    gb = E.Guarded(C_, like=bias)
    gs = E.Guarded(B, like=scale) if plane is not None else None
    gp = E.Guarded(C_, H, W, like=plane.reshape(C_, H, W), aligned=plane_aligned) if plane is not None else None
    y, mask = E.Guarded(B, C_, Ho, Wo), E.Guarded(B, C_, Ho, Wo, dtype=torch.uint8)
    rc = lib.aurppo_bias_relu_pool2_fwd_f32(E.ptr(gx.view), E.ptr(gb.view), E.ptr(gs.view) if gs else None, E.ptr(gp.view) if gp else None,
                                            E.ptr(y.view), E.ptr(mask.view), B, C_, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    for t in (gx, gb, y, mask) + ((gs, gp) if gp else ()):
        assert t.guards_intact()
    assert mask.written() and int(mask.view.max()) <= 4
    gw = E.Guarded(B, C_, Ho, Wo, like=w)
    dx, part = E.Guarded(B, C_, H, W, aligned=aligned), E.Guarded(B, C_)
    rc = lib.aurppo_bias_relu_pool2_bwd_f32(E.ptr(gw.view), E.ptr(mask.view), E.ptr(dx.view), E.ptr(part.view), B, C_, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    for t in (gw, mask, dx, part):
        assert t.guards_intact()
    dplane = None
    if plane is not None:
        dplane = E.Guarded(C_, H, W)
        rc = lib.aurppo_weighted_batch_sum_f32(E.ptr(dx.view), E.ptr(gs.view), E.ptr(dplane.view), B, C_ * H * W, E.stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.aurppo_last_error()
        assert dplane.guards_intact() and dx.guards_intact() and gs.guards_intact()
    return y, dx, part, dplane


def _k9_operands(shape, g):
    B, C_, H, W, with_plane = shape
    x = torch.randn(B, C_, H, W, device="cuda", generator=g)
    x[0, 0].fill_(0.25)                       # a plane of ties: the first window element must win
    x[-1, -1].fill_(-1.0)                     # a dead plane
    bias = torch.randn(C_, device="cuda", generator=g)
    if B * C_ == 1:
        x.normal_(generator=g)
    scale = (torch.arange(B, device="cuda") % 2 == 0).float() if with_plane else None      # (B = 1: the plane is on)
    plane = torch.randn(1, C_, H, W, device="cuda", generator=g) if with_plane else None
    w = torch.randn(B, C_, H // 2, W // 2, device="cuda", generator=g)
    return x, bias, scale, plane, w


@pytest.mark.parametrize("shape", E.K9_SHAPES, ids=lambda s: "x".join(map(str, map(int, s))))
def test_k9_under_guards_equals_the_fp32_op_chain_at_either_alignment(lib, shape):
    B, C_, H, W, with_plane = shape
    g = _gen(*shape)
    x, bias, scale, plane, w = _k9_operands(shape, g)
    ry, rdx, rdb, rdp = _k9_reference(x, bias, scale, plane, w)
    outs = {}
    # x and the plane aligned (float4 bodies); x aligned and the plane alone 3 floats past a boundary (the third term of the forward's
    # ``vec`` test: the scalar body, with the float4 backward); neither aligned
    for aligned in ((True, True), (True, False), (False, False)) if with_plane else ((True, True), (False, False)):
        y, dx, part, dplane = _k9_call(lib, x, bias, scale, plane, w, *aligned)
        assert y.written() and dx.written() and part.written() and (dplane is None or dplane.written())
        assert torch.equal(y.view, ry)                               # same additions in the same order: bit-exact
        assert torch.equal(dx.view, rdx)                             # routing only
        n_terms = B * (H // 2) * (W // 2)
        torch.testing.assert_close(part.view.sum(0), rdb, rtol=1e-5, atol=2e-7 * n_terms ** 0.5 * float(w.abs().max()) + 1e-6)
        if with_plane:
            torch.testing.assert_close(dplane.view.view_as(rdp), rdp, rtol=1e-5, atol=1e-6)
        outs[aligned] = (y.view.clone(), dx.view.clone(), part.view.clone(), None if dplane is None else dplane.view.clone())
    # the scalar fallback of the ``vec`` test against the float4 path: y, dx and the plane gradient bit for bit (the per-plane bias sums
    # add the same terms in another order -- the float4 body pairs two gradients in fp32 first -- and keep their tolerance above)
    for key in outs:
        for i in (0, 1, 3):
            a, b = outs[(True, True)][i], outs[key][i]
            assert (a is None and b is None) or torch.equal(a, b), (key, i)
    if with_plane:          # the backward of the plane-only case is the aligned backward: there the bias sums are the same bits too
        assert torch.equal(outs[(True, True)][2], outs[(True, False)][2])


@pytest.mark.parametrize("K", [1, 300])
@pytest.mark.parametrize("B", [1, 3, 4, 5])
def test_weighted_batch_sum_with_distinct_weights(lib, B, K):
    """k_weighted_batch_sum alone with random fp32 weights (the state flags of the calls above are 0 / 1, which cannot tell w[b] from
    w[b + 2]): out[k] = sum_b w[b] x[b, k] against the fp64 sum at the plane gradient's tolerance; B of 1, 3, 4 (one unrolled group of
    four) and 5 (a group and one), K of one thread and of a second, partial workgroup."""
    g = _gen(B, K, 3)
    x, w = torch.randn(B, K, device="cuda", generator=g), torch.randn(B, device="cuda", generator=g)
    gx, gw, out = E.Guarded(B, K, like=x), E.Guarded(B, like=w), E.Guarded(K)
    rc = lib.aurppo_weighted_batch_sum_f32(E.ptr(gx.view), E.ptr(gw.view), E.ptr(out.view), B, K, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert out.guards_intact() and gx.guards_intact() and gw.guards_intact() and out.written()
    ref = (w.double().view(B, 1) * x.double()).sum(0)
    torch.testing.assert_close(out.view.double(), ref, rtol=1e-5, atol=1e-6)


def _nan_equal(got, ref):
    """NaN exactly where the reference has it, equal elsewhere (infinities compare as values)."""
    return torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(torch.nan_to_num(got, nan=0.0, posinf=float("inf"), neginf=float("-inf")),
                                                                           torch.nan_to_num(ref, nan=0.0, posinf=float("inf"), neginf=float("-inf")))


SPECIALS = [("nan", float("nan"), pos) for pos in range(4)] + [("+inf", float("inf"), 1), ("-inf", float("-inf"), 2)]


@pytest.mark.parametrize("name,value,pos", SPECIALS, ids=[f"{n}@{p}" for n, _, p in SPECIALS])
@pytest.mark.parametrize("shape", [(2, 3, 8, 12, True), (2, 2, 7, 9, False), (1, 2, 36, 32, False)], ids=lambda s: "x".join(map(str, map(int, s))))
def test_k9_propagates_non_finite_values_as_torch_does(lib, shape, name, value, pos):
    """One NaN at window position ``pos`` (0..3, row-major) of a pooling window, one +Inf, one -Inf in x: y is NaN exactly where
    max_pool2d(relu(.)) is and equal elsewhere, and with a finite dy the routing (dx), the bias sums and the plane gradient are those of
    torch's autograd on the same pattern -- at both alignments (the float4 and the scalar forward bodies)."""
    B, C_, H, W, with_plane = shape
    g = _gen(*shape, pos)
    x, bias, scale, plane, w = _k9_operands(shape, g)
    x = x.abs() + 0.5 if name == "-inf" else x          # (-inf in a window that is alive without it)
    b, c, ho, wo = B - 1, 0, (H // 2) - 1, 1
    x[b, c, 2 * ho + (pos >> 1), 2 * wo + (pos & 1)] = value
    ry, rdx, rdb, rdp = _k9_reference(x, bias, scale, plane, w)
    if name != "-inf":
        assert not bool(torch.isfinite(ry[b, c, ho, wo]))
    for aligned in (True, False):
        y, dx, part, dplane = _k9_call(lib, x, bias, scale, plane, w, aligned)
        assert _nan_equal(y.view, ry), f"y: {y.view[b, c, ho, wo].item()} where torch has {ry[b, c, ho, wo].item()}"
        assert _nan_equal(dx.view, rdx)
        n_terms = B * (H // 2) * (W // 2)
        torch.testing.assert_close(part.view.sum(0), rdb, rtol=1e-5, atol=2e-7 * n_terms ** 0.5 * float(w.abs().max()) + 1e-6, equal_nan=True)
        if with_plane:
            torch.testing.assert_close(dplane.view.view_as(rdp), rdp, rtol=1e-5, atol=1e-6, equal_nan=True)


# =================================================================================================================== K10
def _k10_operands(shape, g):
    B, Ci, Co, H, W = shape
    obs = torch.rand(B, Ci, H, W, device="cuda", generator=g)
    state = (torch.arange(B, device="cuda") % 2 == 0).float()
    w = 0.3 * torch.randn(Co, Ci + 1, 3, 3, device="cuda", generator=g)
    b = 0.1 * torch.randn(Co, device="cuda", generator=g)
    gy = torch.randn(B, Co, H // 2, W // 2, device="cuda", generator=g)
    return obs, state, w, b, gy


def _k10_reference(obs, state, w, b, gy):
    """conv2d(cat[obs, tiled state]) + bias -> ReLU -> MaxPool2d(2) on torch's own direct fp32 convolution (no library solver)."""
    B, _, H, W = obs.shape
    w1, b1 = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    x = torch.cat([obs, state.view(-1, 1, 1, 1).expand(B, 1, H, W)], 1)
    with torch.backends.cudnn.flags(enabled=False):
        ref = F.max_pool2d(F.relu(F.conv2d(x, w1, b1, padding=1)), 2)
        ref.backward(gy)
    return ref.detach(), w1.grad, b1.grad


def _k10_call(lib, obs, state, w, b, gy):
    B, Ci, H, W = obs.shape
    Co, Ho, Wo, NT = w.shape[0], H // 2, W // 2, (Ci + 1) * 9
    gobs, gst, gw, gb = E.Guarded(*obs.shape, like=obs), E.Guarded(B, like=state), E.Guarded(*w.shape, like=w), E.Guarded(Co, like=b)
    y, mask = E.Guarded(B, Co, Ho, Wo), E.Guarded(B, Co, Ho, Wo, dtype=torch.uint8)
    rc = lib.aurppo_first_block_fwd_f32(E.ptr(gobs.view), E.ptr(gw.view), E.ptr(gb.view), E.ptr(gst.view), E.ptr(y.view), E.ptr(mask.view),
                                        B, Ci, Co, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    for t in (gobs, gst, gw, gb, y, mask):
        assert t.guards_intact()
    assert mask.written() and int(mask.view.max()) <= 4
    ggy = E.Guarded(B, Co, Ho, Wo, like=gy)
    dwp, dbp = E.Guarded(B * (Co // 16), 16, NT), E.Guarded(B * (Co // 16), 16)
    rc = lib.aurppo_first_block_bwd_f32(E.ptr(ggy.view), E.ptr(mask.view), E.ptr(gobs.view), E.ptr(gst.view), E.ptr(dwp.view), E.ptr(dbp.view),
                                        B, Ci, Co, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    for t in (ggy, mask, gobs, gst, dwp, dbp):
        assert t.guards_intact()
    dw = dwp.view.view(B, Co // 16, 16, NT).sum(0).reshape(Co, Ci + 1, 3, 3)          # as hip_ops._FirstBlock.backward folds them
    db = dbp.view.view(B, Co // 16, 16).sum(0).reshape(Co)
    return y, dwp, dbp, dw, db


@pytest.mark.parametrize("shape", E.K10_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_k10_under_guards_matches_conv_relu_pool(lib, shape):
    g = _gen(*shape)
    obs, state, w, b, gy = _k10_operands(shape, g)
    ref, rdw, rdb = _k10_reference(obs, state, w, b, gy)
    y, dwp, dbp, dw, db = _k10_call(lib, obs, state, w, b, gy)
    assert y.written() and dwp.written() and dbp.written()
    torch.testing.assert_close(y.view, ref, rtol=1e-5, atol=2e-6)
    sw, sb = float(rdw.abs().max()), float(rdb.abs().max())
    assert float((dw - rdw).abs().max()) <= 2e-5 * sw + 1e-6, (float((dw - rdw).abs().max()), sw)
    assert float((db - rdb).abs().max()) <= 2e-5 * sb + 1e-6


K10_SPECIALS = [(n, v, p, t) for t in ("obs", "weight", "bias") for (n, v, p) in SPECIALS]
# A non-finite observation value where k_first_block_bwd's walk clamps a row or a column (its weight-0 products must agree with the
# 0 * x terms torch's dense gradient forms) and where no pooled window reaches (the odd trailing row / column, read apart):
# (shape, (row, column), what)
K10_BORDER_SHAPES = [(2, 2, 16, 8, 8), (2, 1, 48, 7, 9)]
K10_BORDERS = [((2, 2, 16, 8, 8), (0, 0), "corner"), ((2, 2, 16, 8, 8), (7, 3), "last-row"), ((2, 2, 16, 8, 8), (4, 7), "last-column"),
               ((2, 2, 16, 8, 8), (7, 7), "last-corner"), ((2, 1, 48, 7, 9), (0, 0), "corner"), ((2, 1, 48, 7, 9), (6, 4), "trailing-row"),
               ((2, 1, 48, 7, 9), (3, 8), "trailing-column"), ((2, 1, 48, 7, 9), (6, 8), "trailing-corner"),
               ((2, 1, 48, 7, 9), (5, 7), "last-pooled-corner"), ((2, 1, 48, 7, 9), (0, 5), "first-row")]
K10_BORDER_CASES = [(s, at, what, n, v) for (s, at, what) in K10_BORDERS for (n, v) in (("nan", float("nan")), ("+inf", float("inf")), ("-inf", float("-inf")))]


def _k10_close(got, want, rtol, atol, what):
    """NaN and each infinity exactly where torch has them, the tolerance elsewhere."""
    bad_w = ~torch.isfinite(want)
    zero = torch.zeros_like(want)
    same = torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.where(torch.isinf(got), got, zero),
                                                                            torch.where(torch.isinf(want), want, zero))
    assert same, (f"{what}: NaN at {int(torch.isnan(got).sum())} elements, torch at {int(torch.isnan(want).sum())}; "
                  f"Inf at {int(torch.isinf(got).sum())}, torch at {int(torch.isinf(want).sum())}")
    ok = ~bad_w
    if bool(ok.any()):
        d = (got[ok] - want[ok]).abs()
        assert bool((d <= atol + rtol * want[ok].abs()).all()), f"{what}: {float(d.max()):.3e}"


def _k10_check_against_torch(lib, obs, state, w, b, gy):
    ref, rdw, rdb = _k10_reference(obs, state, w, b, gy)
    y, dwp, dbp, dw, db = _k10_call(lib, obs, state, w, b, gy)
    _k10_close(y.view, ref, 1e-5, 2e-6, "y")
    fin_w, fin_b = rdw[torch.isfinite(rdw)], rdb[torch.isfinite(rdb)]
    sw = float(fin_w.abs().max()) if fin_w.numel() else 0.0
    sb = float(fin_b.abs().max()) if fin_b.numel() else 0.0
    _k10_close(dw, rdw, 0.0, 2e-5 * sw + 1e-6, "weight gradient")
    _k10_close(db, rdb, 0.0, 2e-5 * sb + 1e-6, "bias gradient")
    return rdw


@pytest.mark.parametrize("shape,at,what,name,value", K10_BORDER_CASES, ids=[f"{'x'.join(map(str, s))}-{w}-{n}" for s, _, w, n, _ in K10_BORDER_CASES])
def test_k10_non_finite_observation_at_the_borders_matches_torch(lib, shape, at, what, name, value):
    """The same comparison with the value on row 0 / column 0, on the last row / column of an even image, on the odd trailing row /
    column of the 7 x 9 image and on the last pooled position beside them.  With +-Inf torch's weight gradient holds +-Inf where the one
    position that reads the value is a visited, alive maximum and NaN where an unvisited position reads it: both must come out."""
    B, Ci, Co, H, W = shape
    g = _gen(*shape, *at)
    obs, state, w, b, gy = _k10_operands(shape, g)
    obs[B - 1, Ci - 1, at[0], at[1]] = value
    rdw = _k10_check_against_torch(lib, obs, state, w, b, gy)
    assert bool(torch.isnan(rdw).any())          # the case is not empty: torch's dense gradient has 0 * x terms


@pytest.mark.parametrize("name,value,pos,target", K10_SPECIALS, ids=[f"{t}:{n}@{p}" for n, _, p, t in K10_SPECIALS])
@pytest.mark.parametrize("shape", [(2, 2, 16, 8, 8), (2, 1, 48, 7, 9)], ids=lambda s: "x".join(map(str, s)))
def test_k10_propagates_non_finite_values_as_torch_does(lib, shape, name, value, pos, target):
    """One NaN / +Inf / -Inf in the observation (at window position ``pos`` of a pooling window), in one weight (tap ``pos``) or in one
    bias element: y has NaN exactly where torch's chain has it and meets the tolerance elsewhere; with a finite dy the folded weight and
    bias sums have NaN where torch's autograd has it and meet the tolerance elsewhere."""
    B, Ci, Co, H, W = shape
    g = _gen(*shape, pos)
    obs, state, w, b, gy = _k10_operands(shape, g)
    if target == "obs":
        obs[B - 1, Ci - 1, 2 + (pos >> 1), 2 + (pos & 1)] = value
    elif target == "weight":
        w[Co - 3, 0, pos >> 1, pos & 1] = value
    else:
        b[5] = value
    _k10_check_against_torch(lib, obs, state, w, b, gy)
