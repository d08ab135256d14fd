"""GPU: the narrow gradient builds K11n / K12n (csrc/conv_narrow.hip) -- the input and the weight gradient of the encoder's
16 -> 32 block in 16 x 16 x 32 matrix blocks -- against the fp64 references of tests/encoder_cases.py at K11 / K12's own bound, 1e-6 of the
sum of |products| behind an element (tests/test_conv_gpu.py), nothing excluded: under guards at every boundary of their tilings
(tests/narrow_cases.py), with non-finite operands, through ``hip_ops``' routing (AURPPO_NARROW_GRADS=1), through the encoder and the whole
policy step against the routing-pinned fp64 net, and at config 3's own tensors (dy of 2^32 bytes).  Run with -s for the figures."""
import collections
import gc

import pytest
import torch

from tests import encoder_cases as E
from tests import narrow_cases as NC

pytestmark = pytest.mark.gpu

BOUND = 1e-6        # of the sum of |products| behind an element (tests/test_conv_gpu.py)
P = 7               # base images of the large cases (tests/test_encoder_large_gpu.py)


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * int(v) for i, v in enumerate(key)) + 29)


def _ids(s):
    return "x".join(map(str, s))


def _operands(shape, g):
    B, Ci, Co, H, W, pad = shape
    x = torch.randn(B, Ci, H, W, device="cuda", generator=g)
    dy = torch.randn(B, Co, H + 2 * pad - 2, W + 2 * pad - 2, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * (2.0 / (9 * Co)) ** 0.5
    return x, dy, w


# =================================================================================================================== K11n
def _dgrad_call(lib, dy, w, shape, aligned):
    """dx under guards, called twice: the second call must leave the same bits."""
    B, Ci, Co, H, W, pad = shape
    gdy, gw = E.Guarded(*dy.shape, like=dy, aligned=aligned), E.Guarded(*w.shape, like=w, aligned=aligned)
    dx = E.Guarded(B, Ci, H, W, aligned=aligned)
    nbytes = lib.aurppo_conv3x3_dgrad_narrow_wop_bytes(Ci, Co)
    assert nbytes == NC.dgrad_plan(*shape)["wop_bytes"]
    ws = E.Workspace(nbytes)
    first = None
    for _ in range(2):
        rc = lib.aurppo_conv3x3_dgrad_narrow_f32(E.ptr(gdy.view), E.ptr(gw.view), E.ptr(dx.view), *shape, E.ptr(ws.view), E.stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.aurppo_last_error()
        assert dx.guards_intact() and ws.guards_intact() and gdy.guards_intact() and gw.guards_intact()
        if first is None:
            first = dx.view.clone()
    assert torch.equal(first.view(torch.int32), dx.view.view(torch.int32)), "a second call left other bits"
    return dx


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "shifted"])
@pytest.mark.parametrize("shape", NC.DGRAD_SHAPES, ids=_ids)
def test_k11n_under_guards_meets_the_fp64_input_gradient(lib, shape, aligned):
    x, dy, w = _operands(shape, _gen(*shape))
    dx = _dgrad_call(lib, dy, w, shape, aligned)
    pad = shape[5]
    ref, mag = E.dgrad64(dy, w, pad), E.dgrad64(dy.abs(), w.abs(), pad)
    assert dx.view.shape == ref.shape and dx.written()
    err = E.rel_err(dx.view, ref, mag)
    print(f"\nK11n {shape} {'aligned' if aligned else 'shifted'}: {err:.3e} of sum|ab|")
    assert err <= BOUND


# =================================================================================================================== K12n
def _wgrad_call(lib, x, dy, shape, aligned):
    B, Ci, Co, H, W, pad = shape
    plan = NC.wgrad_plan(*shape)
    gx, gdy = E.Guarded(*x.shape, like=x, aligned=aligned), E.Guarded(*dy.shape, like=dy, aligned=aligned)
    dw = E.Guarded(Co, Ci, 3, 3, aligned=aligned)
    nbytes = lib.aurppo_conv3x3_wgrad_narrow_ws_bytes(*shape)
    assert NC.wgrad_slices_from_ws(nbytes, Ci, Co) == plan["S"]
    ws = E.Workspace(nbytes)
    first = None
    for _ in range(2):
        rc = lib.aurppo_conv3x3_wgrad_narrow_f32(E.ptr(gdy.view), E.ptr(gx.view), E.ptr(dw.view), *shape, E.ptr(ws.view), E.stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.aurppo_last_error()
        assert dw.guards_intact() and ws.guards_intact() and gx.guards_intact() and gdy.guards_intact()
        if first is None:
            first = dw.view.clone()
    assert torch.equal(first.view(torch.int32), dw.view.view(torch.int32)), "a second call left other bits"
    return dw


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "shifted"])
@pytest.mark.parametrize("shape", NC.WGRAD_SHAPES, ids=_ids)
def test_k12n_under_guards_meets_the_fp64_weight_gradient(lib, shape, aligned):
    x, dy, _ = _operands(shape, _gen(*shape))
    dw = _wgrad_call(lib, x, dy, shape, aligned)
    Co, pad = shape[2], shape[5]
    ref, mag = E.wgrad64(x, dy, Co, pad), E.wgrad64(x.abs(), dy.abs(), Co, pad)
    assert dw.written()
    err = E.rel_err(dw.view, ref, mag)
    print(f"\nK12n {shape} {'aligned' if aligned else 'shifted'}: {err:.3e} of sum|ab|")
    assert err <= BOUND


# =================================================================================================================== non-finite values
def _place(t, where, value):
    """One ``value`` at element 0, the last element or an interior element of the flattened tensor."""
    n = t.numel()
    at = {"first": 0, "last": n - 1, "interior": n // 2 + n // 7}[where]
    t.view(-1)[at] = value
    return t


def _same_non_finite_set_and_bound(got, ref, mag, what):
    bad_ref, bad_got = ~torch.isfinite(ref), ~torch.isfinite(got)
    assert bool(bad_ref.any()), f"{what}: the reference has no non-finite output: the case checks nothing"
    assert torch.equal(bad_got, bad_ref), (f"{what}: {int(bad_got.sum())} non-finite outputs, the fp64 reference has {int(bad_ref.sum())}; "
                                           f"{int((bad_got & ~bad_ref).sum())} extra, {int((~bad_got & bad_ref).sum())} missing")
    ok = ~bad_ref
    if bool(ok.any()):
        err = float(((got.double() - ref).abs()[ok] / mag[ok].clamp_min(1e-30)).max())
        print(f"\n{what}: finite outputs {err:.3e} of sum|ab|, {int(bad_ref.sum())} non-finite")
        assert err <= BOUND, what


NONFINITE_DGRAD = [(3, 16, 64, 10, 10, 1), (2, 16, 96, 7, 6, 0)]          # one padded, one unpadded
NONFINITE_WGRAD = [(37, 16, 32, 12, 12, 1), (23, 16, 32, 17, 17, 0)]


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first", "last", "interior"])
@pytest.mark.parametrize("shape", NONFINITE_DGRAD, ids=_ids)
def test_k11n_non_finite_outputs_are_the_fp64_references(lib, shape, where, value):
    x, dy, w = _operands(shape, _gen(*shape, 5))
    _place(dy, where, value)
    dx = _dgrad_call(lib, dy, w, shape, True)
    pad = shape[5]
    _same_non_finite_set_and_bound(dx.view, E.dgrad64(dy, w, pad), E.dgrad64(dy.abs(), w.abs(), pad), f"K11n {shape} {value} in dy at {where}")


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("where", ["first", "last", "interior"])
@pytest.mark.parametrize("operand", ["x", "dy"])
@pytest.mark.parametrize("shape", NONFINITE_WGRAD, ids=_ids)
def test_k12n_non_finite_outputs_are_the_fp64_references(lib, shape, operand, where, value):
    x, dy, _ = _operands(shape, _gen(*shape, 9))
    _place(x if operand == "x" else dy, where, value)
    dw = _wgrad_call(lib, x, dy, shape, True)
    Co, pad = shape[2], shape[5]
    _same_non_finite_set_and_bound(dw.view, E.wgrad64(x, dy, Co, pad), E.wgrad64(x.abs(), dy.abs(), Co, pad),
                                   f"K12n {shape} {value} in {operand} at {where}")


# =================================================================================================================== routing
def _counted(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    calls = collections.Counter()
    real_d, real_w = H.conv3x3_dgrad_narrow, H.conv3x3_wgrad_narrow
    monkeypatch.setattr(H, "conv3x3_dgrad_narrow", lambda g, w, pad: (calls.update(K11n=1), real_d(g, w, pad))[1])
    monkeypatch.setattr(H, "conv3x3_wgrad_narrow", lambda g, x, cout, pad: (calls.update(K12n=1), real_w(g, x, cout, pad))[1])
    return calls, real_d, real_w


def _library_grads(g, x, w, pad):
    """Today's route for the 16 -> 32 block: ``_conv3x3_grads``' two library calls, one gradient each."""
    def one(mask):
        return torch.ops.aten.convolution_backward(g, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)
    return one([True, False, False])[0], one([False, True, False])[1]


def _block(gen, B=4, H=12, W=10):
    x = torch.randn(B, 16, H, W, device="cuda", generator=gen)
    w = torch.randn(32, 16, 3, 3, device="cuda", generator=gen) * 0.08
    b = torch.randn(32, device="cuda", generator=gen) * 0.3
    return x, w, b


def test_the_switch_routes_both_backwards_through_the_narrow_builds(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    calls, real_d, real_w = _counted(monkeypatch)
    monkeypatch.setattr(H, "NARROW_MIN_PIXELS", 1)
    monkeypatch.setenv("AURPPO_NARROW_GRADS", "1")
    gen = _gen(4)
    x, w, b = _block(gen)
    # conv3x3
    g = torch.randn(4, 32, 12, 10, device="cuda", generator=gen)
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    H.conv3x3(xa, wa, 1).backward(g)
    assert calls == dict(K11n=1, K12n=1)
    assert torch.equal(xa.grad, real_d(g, w, 1)) and torch.equal(wa.grad, real_w(g, x, 32, 1))
    # conv3x3_pool: K9's backward rebuilds dz from the mask, the narrow builds take it from there
    gy = torch.randn(4, 32, 6, 5, device="cuda", generator=gen)
    xb, wb, bb = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    H.conv3x3_pool(xb, wb, bb, 1).backward(gy)
    assert calls == dict(K11n=2, K12n=2)
    z = H.conv3x3(x, w, 1).detach().requires_grad_(True)
    H.bias_relu_pool2(z, b).backward(gy)
    dz = z.grad.contiguous()
    assert torch.equal(xb.grad, real_d(dz, w, 1)) and torch.equal(wb.grad, real_w(dz, x, 32, 1))
    # ... and the values are the gradient's
    ref_dx, ref_dw = _library_grads(g, x, w, 1)
    torch.testing.assert_close(xa.grad, ref_dx, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(wa.grad, ref_dw, rtol=2e-5, atol=2e-5 * float(ref_dw.abs().max()))


@pytest.mark.parametrize("env,lifted", [(None, True), ("0", True), ("1", False)], ids=["unset", "zero", "set-under-the-size-rule"])
def test_without_the_switch_or_under_the_size_rule_the_backward_is_todays(monkeypatch, env, lifted):
    from aur_ppo_amd import hip_ops as H
    calls, _, _ = _counted(monkeypatch)
    if lifted:
        monkeypatch.setattr(H, "NARROW_MIN_PIXELS", 1)
    else:
        assert H.NARROW_MIN_PIXELS > 4 * 12 * 10
    if env is None:
        monkeypatch.delenv("AURPPO_NARROW_GRADS", raising=False)
    else:
        monkeypatch.setenv("AURPPO_NARROW_GRADS", env)
    gen = _gen(4)
    x, w, _ = _block(gen)
    g = torch.randn(4, 32, 12, 10, device="cuda", generator=gen)
    # the library's weight gradient is not reproducible from call to call (its kernel adds with atomics), so "today's route" is pinned
    # by what it is: _conv3x3_grads' two aten.convolution_backward calls, one gradient each, whose results ARE the gradients
    made, real_aten = [], torch.ops.aten.convolution_backward

    def recording(*a):
        out = real_aten(*a)
        made.append((a, out))
        return out
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", recording)
    xa, wa = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    H.conv3x3(xa, wa, 1).backward(g)
    monkeypatch.setattr(torch.ops.aten, "convolution_backward", real_aten)
    assert not calls
    assert [a[10] for a, _ in made] == [[True, False, False], [False, True, False]]
    for a, _ in made:
        assert a[0].data_ptr() == g.data_ptr() and torch.equal(a[1], x) and torch.equal(a[2], w) and a[3] is None
        assert list(a[4:10]) == [[1, 1], [1, 1], [1, 1], False, [0, 0], 1]
    assert torch.equal(xa.grad, made[0][1][0]) and torch.equal(wa.grad, made[1][1][1])
    ref_dx, ref_dw = _library_grads(g, x, w, 1)
    assert torch.equal(xa.grad, ref_dx)
    torch.testing.assert_close(wa.grad, ref_dw, rtol=1e-4, atol=1e-5 * float(ref_dw.abs().max()))


# =================================================================================================================== the encoder
@pytest.mark.parametrize("obs_shape,batch", [((2, 128, 128), 6), ((3, 84, 84), 3)], ids=["2x128x128", "3x84x84"])
def test_encoder_with_the_narrow_builds_matches_the_stock_encoder(monkeypatch, obs_shape, batch):
    """tests/test_conv_gpu.py::test_encoder_with_k11_matches_the_stock_encoder with the switch on and the size rules lifted, at its tolerances."""
    from aur_ppo_amd import hip_ops as H
    from aur_ppo_amd.base_cnns import base_encoder
    calls, _, _ = _counted(monkeypatch)
    for name in ("CONV3X3_MIN_PIXELS", "K12_MIN_PIXELS", "NARROW_MIN_PIXELS"):
        monkeypatch.setattr(H, name, 1)
    monkeypatch.setenv("AURPPO_NARROW_GRADS", "1")
    torch.manual_seed(0)
    enc = base_encoder(obs_shape=obs_shape, out_dim=128).cuda()
    obs = torch.rand(batch, obs_shape[0] - 1, *obs_shape[1:], device="cuda")
    state = (torch.rand(batch, device="cuda") < 0.5).float()
    outs = []
    for fused in (True, False):
        enc.fused_conv = fused
        enc.zero_grad()
        y = enc.forward_split(obs, state)
        y.square().sum().backward()
        outs.append((y.detach().clone(), [p.grad.detach().clone() for p in enc.parameters()]))
    assert calls == dict(K11n=1, K12n=1), calls          # the 16 -> 32 block, once, on the fused pass
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=2e-5, atol=2e-5)
    for a, b in zip(outs[0][1], outs[1][1]):
        torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5 * float(b.abs().max()) + 1e-7)


# =================================================================================================================== the policy against fp64
@pytest.mark.parametrize("C,S", [(1, 128), (3, 84)], ids=["128x128x1", "84x84x3"])
def test_policy_gradients_with_the_narrow_builds_meet_the_fp64_bars(C, S, monkeypatch):
    """The hand_written_convolutions path of tests/ref64_robot.py with the 16 -> 32 block's gradients on K11n / K12n: ``R.check`` with its own
    bars (gradients 8, forward 4, scalars 16 x Y).  Both narrow functions run twice per backward pass, once per encoder,
    and ``_conv3x3_grads`` never reaches aten.convolution_backward."""
    from oracle import ppo_oracle as O
    from tests import ref64_robot as R
    from aur_ppo_amd import hip_ops as H
    assert (C, S) in R.SHAPES
    sd, case = R.make_case(C, S)
    pol = R.gpu_policy(sd, C, S)
    R.select_path("hand_written_convolutions", pol, monkeypatch.setattr, monkeypatch.setenv)
    calls, _, _ = _counted(monkeypatch)
    monkeypatch.setattr(H, "NARROW_MIN_PIXELS", 1)
    monkeypatch.setenv("AURPPO_NARROW_GRADS", "1")
    real_grads, reached = H._conv3x3_grads, []

    def guarded_grads(*a, **k):
        real_aten = torch.ops.aten.convolution_backward
        with monkeypatch.context() as m:
            m.setattr(torch.ops.aten, "convolution_backward", lambda *aa, **kk: (reached.append(1), real_aten(*aa, **kk))[1])
            return real_grads(*a, **k)
    monkeypatch.setattr(H, "_conv3x3_grads", guarded_grads)
    lp, ent, v, routing, counts = R.path_evaluate(pol, case)
    n_backward = 0
    for vmode, packed in ((O.VLOSS_CLIPPED, True), (O.VLOSS_RETURNS, False)):
        ref = R.reference((C, S, 2), sd, case, routing, vmode)
        Y = R.gpu_yardstick((C, S, 2), sd, case, ref, vmode)
        got = R.path_step(pol, case, lp, ent, v, vmode, packed)
        n_backward += 1
        R.check(got, ref, Y, f"narrow {C}x{S}x{S} {'clip_vloss' if vmode == O.VLOSS_CLIPPED else 'returns'} {'packed' if packed else 'unpacked'}")
    assert calls == dict(K11n=2 * n_backward, K12n=2 * n_backward), calls
    assert not reached, "aten.convolution_backward was reached from _conv3x3_grads"


# =================================================================================================================== 2^31 and 2^32 bytes
@pytest.fixture
def _free_after():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _need(gib):
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * gib * (1 << 30):
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free on the device, the case needs {gib:.1f} GiB and asks for twice that")


def test_k11n_at_config_3_every_image_meets_its_base_image(lib, _free_after):
    """dy is exactly 2^32 bytes, dx 2^31: a tile of P = 7 base images, every image of dx against the fp64 gradient of its base image."""
    shape = NC.CONFIG3
    B, Ci, Co, H, W, pad = shape
    assert B * Co * H * W * 4 == 1 << 32 and B * Ci * H * W * 4 == 1 << 31
    _need(7.0)
    g = _gen(*shape, 1)
    base = torch.randn(P, Co, H, W, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * (2.0 / (9 * Co)) ** 0.5
    ref, mag = E.dgrad64(base, w, pad), E.dgrad64(base.abs(), w.abs(), pad)
    dy = E.tile_images(base, B)
    dx = torch.full((B, Ci, H, W), float("nan"), device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_dgrad_narrow_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_dgrad_narrow_f32(E.ptr(dy), E.ptr(w), E.ptr(dx), *shape, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert ws.guards_intact()
    del dy
    err = E.compare_periodic(dx, ref, mag, images_per_chunk=max(P, (256 << 20) // (dx[0].numel() * 12)))
    print(f"\nK11n {shape}: worst of {B} images {err:.3e} of sum|ab|")
    assert err <= BOUND        # (NaN -- an element never written -- fails this too)


def test_k12n_at_config_3_meets_the_weighted_sum_of_base_gradients(lib, _free_after):
    """The masked-sum construction of tests/test_encoder_large_gpu.py: dy[b] = s_b * G[b mod 7], the reference sum_r n_r dW_r."""
    shape = NC.CONFIG3
    B, Ci, Co, H, W, pad = shape
    nbytes = lib.aurppo_conv3x3_wgrad_narrow_ws_bytes(*shape)
    plan = NC.wgrad_plan(*shape)
    S = NC.wgrad_slices_from_ws(nbytes, Ci, Co)
    assert S == plan["S"] and S > 1
    # the last slice begins beyond byte 2^31 of dy: its buffer is re-based there and not capped; the first slice's is capped at 2^31
    b_last = ((S - 1) * plan["pps"]) // (H * W)
    assert b_last * Co * H * W * 4 > (1 << 31) and (B - b_last) * Co * H * W * 4 < (1 << 31) and B * Co * H * W * 4 == 1 << 32
    _need(7.0)
    g = _gen(*shape, 2)
    base_x = torch.randn(P, Ci, H, W, device="cuda", generator=g)
    base_g = torch.randn(P, Co, H, W, device="cuda", generator=g)
    s = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
    ref, mag = E.structured_wgrad64(base_x, base_g, s, Co, pad)
    x = E.tile_images(base_x, B)
    dy = E.tile_images(base_g, B)
    dy.mul_(s.view(-1, 1, 1, 1))
    dw = E.Guarded(Co, Ci, 3, 3)
    ws = E.Workspace(nbytes)
    rc = lib.aurppo_conv3x3_wgrad_narrow_f32(E.ptr(dy), E.ptr(x), E.ptr(dw.view), *shape, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert dw.guards_intact() and ws.guards_intact() and dw.written()
    err = E.rel_err(dw.view, ref, mag)
    print(f"\nK12n {shape}: S = {S}, {plan['pps']} pixels per slice, {err:.3e} of sum|ab|")
    assert err <= BOUND
