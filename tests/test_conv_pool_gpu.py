"""GPU: K11p (csrc/conv.hip, the POOL builds of k_conv3x3 behind aurppo_conv3x3_pool_f32) -- a hidden encoder block's 3x3
convolution, bias, ReLU and 2 x 2 max-pool in one launch -- through the C ABI between guards, at the smallest shapes that take each of
its branches (tests/conv_pool_cases.py).

1. Bit identity: y as int32 and mask as bytes equal what the two launches K11 -> K9 leave on the same inputs, with and without a bias;
   guards intact, every output element written, a second call gives the same bits.
2. fp64: y within 1e-6 * max over the window of (sum |a b| + |bias|) of the fp64 conv -> + bias -> relu -> max_pool, K11's own bound
   (tests/test_conv_gpu.py), which ReLU and max -- both 1-Lipschitz -- carry through.  Nothing is excluded.  (The mask is held by 1.:
   an fp32 and an fp64 argmax may differ on a near-tie.)
3. Non-finite inputs: one NaN, then one +Inf, at the first, an interior and the last element of x: still K9's bits.
Then the autograd function, the two encoders and one robot_ppo.update, switch on against switch off."""
import numpy as np
import pytest
import torch

from tests import conv_pool_cases as CP
from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

BOUND = 1e-6        # of the sum of |products| (+ |bias|) behind an element (tests/test_conv_gpu.py)


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


def _pair(lib, shape, x, w, bias):
    """The two-launch reference: aurppo_conv3x3_f32 (mode 0) into z, aurppo_bias_relu_pool2_fwd_f32 on z.  Returns y, mask."""
    B, Ci, Co, H, W, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    z = torch.full((B, Co, Ho, Wo), float("nan"), device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_f32(E.ptr(x), E.ptr(w), E.ptr(z), B, Ci, Co, H, W, pad, 0, E.ptr(ws.view), E.stream())
    assert rc == 0, lib.aurppo_last_error()
    y = torch.full((B, Co, Ho // 2, Wo // 2), float("nan"), device="cuda")
    mask = torch.full((B, Co, Ho // 2, Wo // 2), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.aurppo_bias_relu_pool2_fwd_f32(E.ptr(z), E.ptr(bias) if bias is not None else None, None, None, E.ptr(y), E.ptr(mask),
                                            B, Co, Ho, Wo, E.stream())
    assert rc == 0, lib.aurppo_last_error()
    torch.cuda.synchronize()
    return y, mask


def _fused(lib, shape, x, w, bias, aligned):
    """aurppo_conv3x3_pool_f32 between guards: inputs exact-size views of NaN-filled buffers, outputs NaN / 0xA5-filled guarded views, the
    operand workspace exactly aurppo_conv3x3_wop_bytes long and 0xFF-filled.  Returns rc and the guarded objects."""
    B, Ci, Co, H, W, pad = shape
    hp, wp = CP.pooled(H, W, pad)
    gx, gw = E.Guarded(*x.shape, aligned=True, like=x), E.Guarded(*w.shape, aligned=True, like=w)
    gb = E.Guarded(Co, aligned=False, like=bias) if bias is not None else None
    y = E.Guarded(B, Co, max(hp, 1), max(wp, 1), aligned=aligned)
    mask = E.Guarded(B, Co, max(hp, 1), max(wp, 1), dtype=torch.uint8, aligned=aligned)
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_pool_f32(E.ptr(gx.view), E.ptr(gw.view), E.ptr(gb.view) if gb is not None else None, E.ptr(y.view),
                                     E.ptr(mask.view), B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    return rc, y, mask, ws, (gx, gw, gb)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_ref_cache = {}


def _inputs_and_pair(lib, shape):
    """x, w, bias on the device and the two-launch results with and without the bias: computed once per shape, read by every test."""
    if shape not in _ref_cache:
        x, w, b = CP.inputs(shape, device="cuda")
        _ref_cache[shape] = (x, w, b, _pair(lib, shape, x, w, b), _pair(lib, shape, x, w, None))
    return _ref_cache[shape]


# ------------------------------------------------------------------------------------------------------------- 1. bit identity
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "shifted"])
@pytest.mark.parametrize("shape", CP.SHAPES, ids=CP.IDS)
def test_fused_block_is_bit_for_bit_the_two_launches(lib, shape, aligned):
    x, w, b, with_bias, without = _inputs_and_pair(lib, shape)
    for bias, (ry, rmask) in ((b, with_bias), (None, without)):
        rc, y, mask, ws, ins = _fused(lib, shape, x, w, bias, aligned)
        assert rc == 0, lib.aurppo_last_error()
        assert y.guards_intact() and mask.guards_intact() and ws.guards_intact()
        assert all(g.guards_intact() for g in ins if g is not None)
        assert y.written() and mask.written()
        assert not bool(torch.isnan(ry).any()) and int(rmask.max()) <= 4
        assert _same_bits(y.view, ry), f"y differs in {int((y.view.view(torch.int32) != ry.view(torch.int32)).sum())} of {ry.numel()} elements"
        assert torch.equal(mask.view, rmask)
        rc2, y2, mask2, _, _ = _fused(lib, shape, x, w, bias, aligned)
        assert rc2 == 0 and _same_bits(y2.view, y.view) and torch.equal(mask2.view, mask.view)
    # the windows are not all dead and not all alive, and every window position is taken somewhere: the comparison saw K9's rules at work
    if with_bias[1].numel() >= 64:
        assert set(with_bias[1].unique().tolist()) == {0, 1, 2, 3, 4}


def test_a_map_without_a_whole_window_is_refused_before_any_launch(lib):
    shape = CP.REFUSED
    x, w, b = CP.inputs(shape, device="cuda")
    rc, y, mask, ws, ins = _fused(lib, shape, x, w, b, True)
    assert rc == CP.AURPPO_ESHAPE
    assert "window" in lib.aurppo_last_error().decode()
    assert bool(torch.isnan(y.buf).all()) and bool((mask.buf == E.GUARD_BYTE).all())
    assert bool((ws.buf == 0xFF).all())          # the operand copy was not begun either


def test_what_mode_0_refuses_is_refused(lib):
    shape = (2, 16, 32, 8, 8, 1)
    x, w, b = CP.inputs(shape, device="cuda")
    y, mask = torch.empty(2, 32, 4, 4, device="cuda"), torch.empty(2, 32, 4, 4, dtype=torch.uint8, device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(16, 32))
    ok = [E.ptr(x), E.ptr(w), E.ptr(b), E.ptr(y), E.ptr(mask), 2, 16, 32, 8, 8, 1, E.ptr(ws.view), E.stream()]
    for i in (0, 1, 3, 4, 11):                     # x, w, y, mask, wop_ws may not be NULL
        bad = list(ok)
        bad[i] = None
        assert lib.aurppo_conv3x3_pool_f32(*bad) == -1
    for i, v in ((5, 0), (6, 24), (6, 0), (7, 0), (8, 0), (9, -1), (10, 3), (10, -1)):
        bad = list(ok)
        bad[i] = v
        assert lib.aurppo_conv3x3_pool_f32(*bad) == CP.AURPPO_ESHAPE, (i, v)
    bad = list(ok)
    bad[11] = E.ptr(ws.view[4:])                   # a workspace off its 16-byte boundary
    assert lib.aurppo_conv3x3_pool_f32(*bad) == CP.AURPPO_ESHAPE
    torch.cuda.synchronize()
    assert bool((ws.buf == 0xFF).all())


# ------------------------------------------------------------------------------------------------------------- 2. against fp64
@pytest.mark.parametrize("shape", CP.SHAPES, ids=CP.IDS)
def test_fused_block_meets_the_fp64_block(lib, shape):
    x, w, b, _, _ = _inputs_and_pair(lib, shape)
    for bias in (b, None):
        rc, y, _, _, _ = _fused(lib, shape, x, w, bias, True)
        assert rc == 0, lib.aurppo_last_error()
        ref, mag = CP.block64(x, w, bias, shape[5])
        assert ref.shape == y.view.shape and float(ref.max()) > 0.0
        err = E.rel_err(y.view, ref, mag)
        print(f"\nK11p {shape} bias={bias is not None}: {err:.3e} of max_u(sum|ab| + |bias|)")
        assert err <= BOUND


# ------------------------------------------------------------------------------------------------------------- 3. non-finite values
@pytest.mark.parametrize("shape", CP.SHAPES, ids=CP.IDS)
def test_a_nan_or_an_inf_in_x_leaves_k9_s_bits(lib, shape):
    x, w, b, _, _ = _inputs_and_pair(lib, shape)
    n = x.numel()
    for value in (float("nan"), float("inf")):
        for at in (0, n // 2 + 1 if n > 2 else 1, n - 1):
            xv = x.clone()
            xv.view(-1)[at] = value
            ry, rmask = _pair(lib, shape, xv, w, b)
            rc, y, mask, ws, _ = _fused(lib, shape, xv, w, b, False)
            assert rc == 0, lib.aurppo_last_error()
            assert y.guards_intact() and mask.guards_intact() and ws.guards_intact() and mask.written()
            assert _same_bits(y.view, ry) and torch.equal(mask.view, rmask), (value, at)
            # the value reached a window: a NaN window is alive (its byte names the NaN), none is left as a dead 0
            nan = torch.isnan(ry)
            assert bool(nan.any()) or value == float("inf")
            assert bool((rmask[nan] < 4).all())


# ------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("shape", [(3, 48, 160, 10, 10, 1), (2, 16, 80, 7, 9, 1), (2, 16, 32, 8, 8, 0)], ids=lambda s: "x".join(map(str, s)))
def test_autograd_function_equals_the_two_functions_bit_for_bit(shape, monkeypatch):
    """``conv3x3_pool`` against ``bias_relu_pool2(conv3x3(...))`` with K11's mode 1 and K12 carrying every gradient (no library kernel on
    the path): y, dx, dw and db, all bit-equal."""
    from aur_ppo_amd import hip_ops as H
    monkeypatch.setenv("AURPPO_K11_DGRAD16", "1")
    monkeypatch.setenv("AURPPO_K12_ALL", "1")
    x0, w0, b0 = CP.inputs(shape, device="cuda")
    hp, wp = CP.pooled(shape[3], shape[4], shape[5])
    dy = torch.randn(shape[0], shape[2], hp, wp, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    assert H.conv3x3_wgrad_ok(x0, shape[1], shape[2], shape[5])
    outs = []
    for fused in (True, False):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        y = H.conv3x3_pool(x, w, b, shape[5]) if fused else H.bias_relu_pool2(H.conv3x3(x, w, shape[5]), b)
        y.backward(dy)
        outs.append((y.detach(), x.grad, w.grad, b.grad))
    for name, a, r in zip(("y", "dx", "dw", "db"), *outs):
        assert a.shape == r.shape and _same_bits(a, r), name
    assert float(outs[0][1].abs().max()) > 0 and float(outs[0][2].abs().max()) > 0 and float(outs[0][3].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- the encoders
def _lift_size_rules(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 0)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 0)
    monkeypatch.setenv("AURPPO_K11_DGRAD16", "1")
    monkeypatch.setenv("AURPPO_K12_ALL", "1")
    calls = []
    real = H.conv3x3_pool
    monkeypatch.setattr(H, "conv3x3_pool", lambda x, w, b, p: (calls.append(tuple(x.shape)), real(x, w, b, p))[1])
    return calls


def _on_against_off(holder, run, params, calls, n_fused):
    outs = []
    for on in (True, False):
        holder.fused_block = on
        for p in params:
            p.grad = None
        calls.clear()
        y = run()
        y.square().sum().backward()
        assert len(calls) == (n_fused if on else 0)
        outs.append((y.detach().clone(), [p.grad.detach().clone() for p in params]))
    return outs


@pytest.mark.parametrize("size,n_fused", [(84, 3), (128, 4)])
def test_base_encoder_switch_on_equals_switch_off(size, n_fused, monkeypatch):
    """Features bit-equal; the gradients of the hidden layers -- K11's mode 1 and K12 under the two switches -- bit-equal; the first
    block's (K10, fed the same bits) at the tolerance tests/test_conv_gpu.py holds the encoder to against the stock encoder."""
    from aur_ppo_amd.base_cnns import base_encoder
    calls = _lift_size_rules(monkeypatch)
    torch.manual_seed(0)
    enc = base_encoder(obs_shape=(2, size, size), out_dim=128).cuda()
    obs = torch.rand(8, 1, size, size, device="cuda")
    state = (torch.rand(8, device="cuda") < 0.5).float()
    named = list(enc.named_parameters())
    monkeypatch.setattr(base_encoder, "fused_block", False)
    outs = _on_against_off(base_encoder, lambda: enc.forward_split(obs, state), [p for _, p in named], calls, n_fused)
    assert _same_bits(outs[0][0], outs[1][0])
    for (name, _), a, b in zip(named, outs[0][1], outs[1][1]):
        if name.startswith("conv.0."):
            torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5 * float(b.abs().max()) + 1e-7)
        else:
            assert _same_bits(a, b), name
        assert float(b.abs().max()) > 0, name


def test_equivariant_encoder_switch_on_equals_switch_off(monkeypatch):
    from aur_ppo_amd.equiv import EquivariantEncoder, _Block
    calls = _lift_size_rules(monkeypatch)
    torch.manual_seed(0)
    enc = EquivariantEncoder(2, 32, 128).cuda()      # (the image channel and the tiled state: K10 takes the first block)
    obs = torch.rand(8, 1, 128, 128, device="cuda")
    state = (torch.rand(8, device="cuda") < 0.5).float()
    named = list(enc.named_parameters())
    monkeypatch.setattr(_Block, "fused_block", False)
    outs = _on_against_off(_Block, lambda: enc(obs, state), [p for _, p in named], calls, 4)
    assert _same_bits(outs[0][0], outs[1][0])
    for (name, _), a, b in zip(named, outs[0][1], outs[1][1]):
        if name.startswith("conv.0."):
            torch.testing.assert_close(a, b, rtol=2e-4, atol=2e-5 * float(b.abs().max()) + 1e-7)
        else:
            assert _same_bits(a, b), name


# ------------------------------------------------------------------------------------------------------------- one update
def _one_update(fused, monkeypatch):
    from aur_ppo_amd.base_cnns import base_encoder
    from aur_ppo_amd.robot_ppo import robot_ppo
    from aur_ppo_amd.robot_run import build_parser, params_from_args
    C_, S, T, N = 1, 128, 8, 8
    monkeypatch.setattr(base_encoder, "fused_block", fused)
    p = params_from_args(build_parser().parse_args([]))
    p.update(gym_id="Synthetic-arm", num_envs=N, num_steps=T, total_timesteps=128, num_update_epochs=2, num_minibatches=2,
             do_pretraining=False, log=False, clip_vloss=True, entropy_coeff=0.01, obs_size=S, obs_channels=C_)
    torch.manual_seed(2)
    agent = robot_ppo(p)
    g = torch.Generator().manual_seed(9)
    buf = dict(states=(torch.rand(T, N, generator=g) < 0.5).float(), observations=torch.rand(T, N, C_, S, S, generator=g),
               actions=0.3 * torch.randn(T, N, 5, generator=g), true_actions=torch.zeros(T, N, 5),
               rewards=(torch.rand(T, N, generator=g) < 0.3).float(), terminals=(torch.rand(T, N, generator=g) < 0.1).float())
    base_encoder.fused_block = False               # the behaviour policy's numbers: the same bits for both runs
    with torch.no_grad():
        _, _, lp, _, v = agent.policy.evaluate(buf["states"].view(-1).cuda(), buf["observations"].view(-1, C_, S, S).cuda(),
                                               buf["actions"].view(-1, 5).cuda())
    base_encoder.fused_block = fused
    buf["log_probs"] = lp.view(T, N).cpu() + 0.05 * torch.randn(T, N, generator=g)
    buf["values"] = v.view(T, N).cpu().clone()
    for k, t in buf.items():
        getattr(agent.buffer, k).copy_(t)
    next_state, next_obs = (torch.rand(N, generator=g) < 0.5).float(), torch.rand(N, C_, S, S, generator=g)
    agent.seed_all(1)
    ret, adv = agent.advantages(next_state.cuda(), next_obs.cuda(), torch.zeros(N).cuda(), agent.buffer, T)
    agent.update(agent.buffer.flatten(ret, adv), 2, agent.batch_size, agent.minibatch_size, [])
    return agent._last_scalars.copy()


def test_one_robot_update_switch_on_against_off(monkeypatch):
    """tests/test_robot_gpu.py's smallest update (8 envs x 8 steps of 128 x 128 x 1) with the size rule lifted so that the hidden blocks
    are K11's: the six loss scalars of optimizer step 1 -- identical weights on both sides -- at that file's 1e-5."""
    calls = _lift_size_rules(monkeypatch)
    off = _one_update(False, monkeypatch)
    assert not calls
    on = _one_update(True, monkeypatch)
    assert len(calls) >= 2 * 4 * 4, "K11p did not run"           # two encoders x 4 optimizer steps x 4 eligible blocks
    assert off.shape[0] == on.shape[0] == 4
    np.testing.assert_allclose(on[0, :6], off[0, :6], rtol=1e-5, atol=1e-6)
