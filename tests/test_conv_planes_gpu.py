"""GPU: K11x -- hidden activations kept as bf16 planes (include/aurppo.h: the layout).  The split is a function of a value alone, so a
convolution that reads planes multiplies the very bits the fp32 kernel would have split, and EVERY comparison here is bit for bit: no
tolerance is set anywhere in this file.

1. aurppo_split_planes_f32 against the numpy restatement of the split (tests/conv_planes_cases.py), wide-range values, +-0 and +-inf.
2. K11 on planes (aurppo_conv3x3_planes_f32) against aurppo_conv3x3_f32 mode 0 on the same x, pad 0, 1 and 2, and with a NaN, a +inf and a
   -0.0 planted at the first, the last and a border pixel.
3. K11p with planes in, planes out, and both (aurppo_conv3x3_pool_planes_f32) against aurppo_conv3x3_pool_f32; yp == split_planes(y).
4. K10 with planes out against aurppo_first_block_fwd_f32.
5. Refusals: the code, and nothing written.
6. The autograd functions, the two plain encoders and one robot_ppo.update: AURPPO_K11_PLANES against AURPPO_K11_POOL.
Outputs are views into sentinel-filled buffers with guards either side; a second launch leaves the same bits."""
import numpy as np
import pytest
import torch

from tests import conv_planes_cases as XP
from tests import conv_pool_cases as CP
from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

PLAIN = XP.with_pads(XP.SHAPES, pooled=False)
POOLED = XP.with_pads(XP.SHAPES, pooled=True)


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _split(lib, x):
    """aurppo_split_planes_f32 into guarded planes."""
    B, C, H, W = x.shape
    gp = XP.GuardedPlanes(B, C, H, W)
    rc = lib.aurppo_split_planes_f32(E.ptr(x.contiguous()), E.ptr(gp.view), B, C, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert gp.guards_intact()
    return gp


_cache = {}


def _inputs(lib, shape):
    """x, w, bias of a shape and x's planes: made once, read by every test."""
    key = shape[:5]
    if key not in _cache:
        x, w, b = CP.inputs(shape[:5] + (1,), device="cuda")
        _cache[key] = (x, w, b, _split(lib, x))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------- 1. the split
@pytest.mark.parametrize("shape", XP.SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_planes_is_the_restated_split(lib, shape):
    B, C, H, W = shape
    n = B * C * H * W
    v = XP.wide_range(n, seed=n)
    special = np.array([0.0, -0.0, np.inf, -np.inf], dtype=np.float32)
    v[:min(n, 4)] = special[:min(n, 4)]
    if n > 8:
        v[-4:] = special[::-1]
    x = torch.from_numpy(v.reshape(shape)).cuda()
    gp = _split(lib, x)
    got = gp.view.cpu().numpy().view(np.uint16)
    want = XP.planes_np(v.reshape(shape))
    assert got.shape == want.shape
    assert np.array_equal(XP.canonical(got), XP.canonical(want))
    finite = np.isfinite(v.reshape(shape))
    # the planes of every finite value are compared as they are: no NaN pattern among them, nothing canonicalised
    fin = np.broadcast_to(finite.reshape(B, C // 8, 8, H * W).transpose(0, 1, 3, 2)[:, :, None], got.shape)
    assert np.array_equal(got[fin], want[fin])
    gp2 = _split(lib, x)
    assert torch.equal(gp2.view, gp.view)


# ------------------------------------------------------------------------------------------------------------- 2. K11 on planes
def _conv_f32(lib, shape, x, w):
    B, Ci, Co, H, W, pad = shape
    z = torch.full((B, Co, H + 2 * pad - 2, W + 2 * pad - 2), float("nan"), device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_f32(E.ptr(x), E.ptr(w), E.ptr(z), B, Ci, Co, H, W, pad, 0, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    return z


def _conv_planes(lib, shape, xp, w, aligned):
    B, Ci, Co, H, W, pad = shape
    z = E.Guarded(B, Co, H + 2 * pad - 2, W + 2 * pad - 2, aligned=aligned)
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_planes_f32(E.ptr(xp.view), E.ptr(w), E.ptr(z.view), B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert z.guards_intact() and ws.guards_intact() and xp.guards_intact()
    return z


@pytest.mark.parametrize("shape", PLAIN, ids=XP.ids(PLAIN))
def test_conv_on_planes_is_bit_for_bit_the_fp32_convolution(lib, shape):
    x, w, _, xp = _inputs(lib, shape)
    ref = _conv_f32(lib, shape, x, w)
    assert not bool(torch.isnan(ref).any())
    for aligned in (True, False):
        z = _conv_planes(lib, shape, xp, w, aligned)
        assert z.written()
        assert torch.equal(_bits(z.view), _bits(ref)), f"{int((_bits(z.view) != _bits(ref)).sum())} of {ref.numel()} elements differ"
    z2 = _conv_planes(lib, shape, xp, w, True)
    assert torch.equal(_bits(z2.view), _bits(ref))


def _planted(x):
    """Three copies of x with a NaN, a +inf and a -0.0 at the first pixel, the last pixel and a border pixel (the last column of the first
    row of the last image's first channel), each value visiting each place once."""
    B, C, H, W = x.shape
    flat = [0, x.numel() - 1, ((B - 1) * C * H) * W + (W - 1)]
    values = [float("nan"), float("inf"), -0.0]
    out = []
    for r in range(3):
        xv = x.clone()
        for k, at in enumerate(flat):
            xv.view(-1)[at] = values[(k + r) % 3]
        out.append(xv)
    return out


@pytest.mark.parametrize("shape", XP.SHAPES, ids=XP.ids(XP.SHAPES))
def test_conv_on_planes_with_nan_inf_and_negative_zero_planted(lib, shape):
    x, w, _, _ = _inputs(lib, shape)
    for xv in _planted(x):
        ref = _conv_f32(lib, shape, xv, w)
        z = _conv_planes(lib, shape, _split(lib, xv), w, True)
        assert torch.equal(_bits(z.view), _bits(ref))
        assert bool(torch.isnan(ref).any())


# ------------------------------------------------------------------------------------------------------------- 3. K11p on planes
def _pool_f32(lib, shape, x, w, bias):
    B, Ci, Co, H, W, pad = shape
    hp, wp = CP.pooled(H, W, pad)
    y = torch.full((B, Co, hp, wp), float("nan"), device="cuda")
    mask = torch.full((B, Co, hp, wp), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    rc = lib.aurppo_conv3x3_pool_f32(E.ptr(x), E.ptr(w), E.ptr(bias), E.ptr(y), E.ptr(mask), B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    return y, mask


def _pool_planes(lib, shape, x, xp, w, bias, want, aligned=True, yp_aligned=True):
    """aurppo_conv3x3_pool_planes_f32 between guards; ``xp`` None: fp32 input.  Returns rc, y, mask, yp (or None), ws."""
    B, Ci, Co, H, W, pad = shape
    hp, wp = CP.pooled(H, W, pad)
    y = E.Guarded(B, Co, max(hp, 1), max(wp, 1), aligned=aligned)
    mask = E.Guarded(B, Co, max(hp, 1), max(wp, 1), dtype=torch.uint8, aligned=aligned)
    yp = XP.GuardedPlanes(B, (Co + 7) // 8 * 8, max(hp, 1), max(wp, 1), aligned=yp_aligned) if want else None
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    src = E.ptr(xp.view) if xp is not None else E.ptr(x)
    rc = lib.aurppo_conv3x3_pool_planes_f32(src, int(xp is not None), E.ptr(w), E.ptr(bias), E.ptr(y.view), E.ptr(mask.view),
                                            E.ptr(yp.view) if want else None, B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    return rc, y, mask, yp, ws


@pytest.mark.parametrize("shape", POOLED, ids=XP.ids(POOLED))
def test_pooled_block_with_planes_in_out_and_both(lib, shape):
    x, w, b, xp = _inputs(lib, shape)
    Co = shape[2]
    ry, rmask = _pool_f32(lib, shape, x, w, b)
    ryp = _split(lib, ry) if Co % 8 == 0 else None
    for planes_in, want in ((True, False), (False, True), (True, True)):
        if want and ryp is None:
            continue
        for aligned in (True, False):
            rc, y, mask, yp, ws = _pool_planes(lib, shape, x, xp if planes_in else None, w, b, want, aligned)
            assert rc == 0, lib.aurppo_last_error()
            assert y.guards_intact() and mask.guards_intact() and ws.guards_intact() and xp.guards_intact()
            assert y.written() and mask.written()
            assert torch.equal(_bits(y.view), _bits(ry)), (planes_in, want)
            assert torch.equal(mask.view, rmask), (planes_in, want)
            if want:
                assert yp.guards_intact()
                assert torch.equal(yp.view, ryp.view), (planes_in, want)      # dead windows included: the planes of 0.0f
        rc2, y2, mask2, yp2, _ = _pool_planes(lib, shape, x, xp if planes_in else None, w, b, want)
        assert rc2 == 0 and torch.equal(_bits(y2.view), _bits(ry)) and torch.equal(mask2.view, rmask)
        assert not want or torch.equal(yp2.view, ryp.view)
    if rmask.numel() >= 64 and shape[5] == 1:
        assert 4 in rmask.unique().tolist()          # dead windows were among them


def test_neither_planes_in_nor_out_is_the_fp32_block(lib):
    shape = (4, 16, 48, 8, 8, 1)
    x, w, b, _ = _inputs(lib, shape)
    ry, rmask = _pool_f32(lib, shape, x, w, b)
    rc, y, mask, _, _ = _pool_planes(lib, shape, x, None, w, b, False)
    assert rc == 0 and torch.equal(_bits(y.view), _bits(ry)) and torch.equal(mask.view, rmask)


# ------------------------------------------------------------------------------------------------------------- 4. K10 with planes out
@pytest.mark.parametrize("shape", XP.K10_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_first_block_with_planes_out(lib, shape):
    B, Ci, Co, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    obs = torch.rand(B, Ci, H, W, generator=g).cuda()
    w = (torch.randn(Co, Ci + 1, 3, 3, generator=g) * 0.3).cuda()
    bias = (torch.randn(Co, generator=g) * 0.2).cuda()
    state = (torch.rand(B, generator=g) < 0.5).float().cuda()
    ry = torch.full((B, Co, H // 2, W // 2), float("nan"), device="cuda")
    rmask = torch.full((B, Co, H // 2, W // 2), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    assert lib.aurppo_first_block_fwd_f32(E.ptr(obs), E.ptr(w), E.ptr(bias), E.ptr(state), E.ptr(ry), E.ptr(rmask), B, Ci, Co, H, W,
                                          E.stream()) == 0
    torch.cuda.synchronize()
    ryp = _split(lib, ry)
    for _ in range(2):
        y, mask = E.Guarded(B, Co, H // 2, W // 2, aligned=False), E.Guarded(B, Co, H // 2, W // 2, dtype=torch.uint8, aligned=False)
        yp = XP.GuardedPlanes(B, Co, H // 2, W // 2)
        rc = lib.aurppo_first_block_planes_fwd_f32(E.ptr(obs), E.ptr(w), E.ptr(bias), E.ptr(state), E.ptr(y.view), E.ptr(mask.view),
                                                   E.ptr(yp.view), B, Ci, Co, H, W, E.stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.aurppo_last_error()
        assert y.guards_intact() and mask.guards_intact() and yp.guards_intact() and y.written() and mask.written()
        assert torch.equal(_bits(y.view), _bits(ry)) and torch.equal(mask.view, rmask)
        assert torch.equal(yp.view, ryp.view)
    assert 4 in rmask.unique().tolist() and int(rmask.min()) < 4


# ------------------------------------------------------------------------------------------------------------- 5. refusals
def _nothing_written(*gs):
    for g in gs:
        if isinstance(g, XP.GuardedPlanes):
            assert g.untouched()
        elif isinstance(g, E.Workspace):
            assert bool((g.buf == 0xFF).all())
        else:
            assert bool((torch.isnan(g.buf) if g.buf.dtype == torch.float32 else g.buf == E.GUARD_BYTE).all())


def test_planes_out_of_a_channel_count_that_is_no_multiple_of_8_is_refused(lib):
    shape = (2, 16, 20, 8, 8, 1)
    x, w, b = CP.inputs(shape, device="cuda")
    rc, y, mask, yp, ws = _pool_planes(lib, shape, x, None, w, b, True)
    assert rc == XP.AURPPO_ESHAPE, lib.aurppo_last_error()
    _nothing_written(y, mask, yp, ws)


def test_input_channels_that_are_no_multiple_of_16_are_refused(lib):
    shape = (2, 24, 32, 8, 8, 1)
    x, w, b = CP.inputs(shape, device="cuda")
    xp = _split(lib, x)
    rc, y, mask, yp, ws = _pool_planes(lib, shape, x, xp, w, b, True)
    assert rc == XP.AURPPO_ESHAPE
    _nothing_written(y, mask, yp, ws)
    z = E.Guarded(2, 32, 8, 8)
    assert lib.aurppo_conv3x3_planes_f32(E.ptr(xp.view), E.ptr(w), E.ptr(z.view), 2, 24, 32, 8, 8, 1, E.ptr(ws.view), E.stream()) == XP.AURPPO_ESHAPE
    torch.cuda.synchronize()
    _nothing_written(z, ws)
    # the split itself asks for whole groups of eight
    bad = XP.GuardedPlanes(2, 16, 8, 8)
    assert lib.aurppo_split_planes_f32(E.ptr(x), E.ptr(bad.view), 2, 12, 8, 8, E.stream()) == XP.AURPPO_ESHAPE
    torch.cuda.synchronize()
    _nothing_written(bad)


def test_an_unaligned_or_null_planes_pointer_is_refused(lib):
    shape = (2, 16, 32, 8, 8, 1)
    x, w, b = CP.inputs(shape, device="cuda")
    off = XP.GuardedPlanes(2, 16, 8, 8, aligned=False)
    assert lib.aurppo_split_planes_f32(E.ptr(x), E.ptr(off.view), 2, 16, 8, 8, E.stream()) == XP.AURPPO_EINVAL
    assert lib.aurppo_split_planes_f32(E.ptr(x), None, 2, 16, 8, 8, E.stream()) == XP.AURPPO_EINVAL
    torch.cuda.synchronize()
    _nothing_written(off)
    off.view.copy_(_split(lib, x).view)
    z, ws = E.Guarded(2, 32, 8, 8), E.Workspace(lib.aurppo_conv3x3_wop_bytes(16, 32))
    assert lib.aurppo_conv3x3_planes_f32(E.ptr(off.view), E.ptr(w), E.ptr(z.view), 2, 16, 32, 8, 8, 1, E.ptr(ws.view), E.stream()) == XP.AURPPO_EINVAL
    assert lib.aurppo_conv3x3_planes_f32(None, E.ptr(w), E.ptr(z.view), 2, 16, 32, 8, 8, 1, E.ptr(ws.view), E.stream()) == XP.AURPPO_EINVAL
    torch.cuda.synchronize()
    _nothing_written(z, ws)
    rc, y, mask, yp, ws = _pool_planes(lib, shape, x, off, w, b, True)                       # planes in off their boundary
    assert rc == XP.AURPPO_EINVAL
    _nothing_written(y, mask, yp, ws)
    rc, y, mask, yp, ws = _pool_planes(lib, shape, x, None, w, b, True, yp_aligned=False)    # planes out off theirs
    assert rc == XP.AURPPO_EINVAL
    _nothing_written(y, mask, yp, ws)
    # K10
    obs, st = torch.rand(2, 1, 8, 8, device="cuda"), torch.ones(2, device="cuda")
    w10, b10 = torch.randn(16, 2, 3, 3, device="cuda"), torch.zeros(16, device="cuda")
    y, mask = E.Guarded(2, 16, 4, 4), E.Guarded(2, 16, 4, 4, dtype=torch.uint8)
    yp = XP.GuardedPlanes(2, 16, 4, 4, aligned=False)
    args = [E.ptr(obs), E.ptr(w10), E.ptr(b10), E.ptr(st), E.ptr(y.view), E.ptr(mask.view)]
    assert lib.aurppo_first_block_planes_fwd_f32(*args, E.ptr(yp.view), 2, 1, 16, 8, 8, E.stream()) == XP.AURPPO_EINVAL
    assert lib.aurppo_first_block_planes_fwd_f32(*args, None, 2, 1, 16, 8, 8, E.stream()) == XP.AURPPO_EINVAL
    torch.cuda.synchronize()
    _nothing_written(y, mask, yp)


def test_a_map_without_a_whole_window_is_refused(lib):
    shape = CP.REFUSED[:2] + (16,) + CP.REFUSED[3:]
    x, w, b = CP.inputs(shape, device="cuda")
    xp = _split(lib, x)
    for planes_in, want in ((True, False), (False, True), (True, True)):
        rc, y, mask, yp, ws = _pool_planes(lib, shape, x, xp if planes_in else None, w, b, want)
        assert rc == XP.AURPPO_ESHAPE and "window" in lib.aurppo_last_error().decode()
        _nothing_written(y, mask, ws, *([yp] if want else []))


# ------------------------------------------------------------------------------------------------------------- 6. autograd and callers
@pytest.mark.parametrize("shape", [(3, 48, 160, 10, 10, 1), (2, 16, 80, 7, 9, 1), (2, 16, 32, 8, 8, 0)], ids=lambda s: "x".join(map(str, s)))
def test_autograd_functions_equal_the_fp32_functions_bit_for_bit(shape, monkeypatch):
    from aur_ppo_amd import hip_ops as H
    monkeypatch.setenv("AURPPO_K11_DGRAD16", "1")
    monkeypatch.setenv("AURPPO_K12_ALL", "1")
    x0, w0, b0 = CP.inputs(shape, device="cuda")
    pad = shape[5]
    hp, wp = CP.pooled(shape[3], shape[4], pad)
    gen = torch.Generator(device="cuda").manual_seed(5)
    dy = torch.randn(shape[0], shape[2], hp, wp, device="cuda", generator=gen)
    dz = torch.randn(shape[0], shape[2], shape[3] + 2 * pad - 2, shape[4] + 2 * pad - 2, device="cuda", generator=gen)
    xp = H.split_planes(x0)
    assert xp.dtype == torch.int16 and tuple(xp.shape) == (shape[0], shape[1] // 8, 3, shape[3] * shape[4], 8)
    # the pooled block: planes in and out against conv3x3_pool
    outs = []
    for planes in (True, False):
        x, w, b = (t.clone().requires_grad_(True) for t in (x0, w0, b0))
        if planes:
            y, yp = H.conv3x3_pool_planes(x, xp, w, b, pad, want_planes=True)
            assert not yp.requires_grad and torch.equal(yp, H.split_planes(y))
            assert [tuple(t.shape) for t in y.grad_fn.saved_tensors] == [tuple(x.shape), tuple(w.shape), tuple(y.shape)]
        else:
            y = H.conv3x3_pool(x, w, b, pad)
        y.backward(dy)
        outs.append((y.detach(), x.grad, w.grad, b.grad))
    for name, a, r in zip(("y", "dx", "dw", "db"), *outs):
        assert a.shape == r.shape and torch.equal(_bits(a), _bits(r)), name
    assert all(float(t.abs().max()) > 0 for t in outs[0][1:])
    # the plain convolution
    outs = []
    for planes in (True, False):
        x, w = (t.clone().requires_grad_(True) for t in (x0, w0))
        z = H.conv3x3_planes(x, xp, w, pad) if planes else H.conv3x3(x, w, pad)
        z.backward(dz)
        outs.append((z.detach(), x.grad, w.grad))
    for name, a, r in zip(("z", "dx", "dw"), *outs):
        assert a.shape == r.shape and torch.equal(_bits(a), _bits(r)), name


def test_first_block_function_with_planes(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    g = torch.Generator().manual_seed(3)
    obs, state = torch.rand(2, 1, 12, 12, generator=g).cuda(), (torch.rand(2, generator=g) < 0.5).float().cuda()
    w0, b0 = (torch.randn(16, 2, 3, 3, generator=g) * 0.3).cuda(), (torch.randn(16, generator=g) * 0.2).cuda()
    dy = torch.randn(2, 16, 6, 6, generator=g).cuda()
    outs = []
    for planes in (True, False):
        w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = H.first_block(obs, state, w, b, want_planes=planes)
        if planes:
            y, yp = y
            assert not yp.requires_grad and torch.equal(yp, H.split_planes(y))
        y.backward(dy)
        outs.append((y.detach(), w.grad, b.grad))
    for a, r in zip(*outs):
        assert torch.equal(_bits(a), _bits(r))


def _lift_size_rules(monkeypatch):
    from aur_ppo_amd import hip_ops as H
    monkeypatch.setattr(H, "CONV3X3_MIN_PIXELS", 0)
    monkeypatch.setattr(H, "CONV3X3_MIN_WGS", 0)
    monkeypatch.setenv("AURPPO_K11_DGRAD16", "1")
    monkeypatch.setenv("AURPPO_K12_ALL", "1")
    calls = []
    real_pool, real_conv, real_first = H.conv3x3_pool_planes, H.conv3x3_planes, H.first_block

    def pool(x, xp, w, b, p, want=False):
        calls.append(("pool", xp is not None, bool(want)))
        return real_pool(x, xp, w, b, p, want)

    def conv(x, xp, w, p):
        calls.append(("conv", True, False))
        return real_conv(x, xp, w, p)

    def first(obs, state, w, b, want_planes=False):
        calls.append(("first", False, bool(want_planes)))
        return real_first(obs, state, w, b, want_planes)

    monkeypatch.setattr(H, "conv3x3_pool_planes", pool)
    monkeypatch.setattr(H, "conv3x3_planes", conv)
    monkeypatch.setattr(H, "first_block", first)
    return calls


@pytest.mark.parametrize("size", [84, 128])
def test_base_encoder_planes_equal_the_fused_blocks_bit_for_bit(size, monkeypatch):
    from aur_ppo_amd.base_cnns import base_encoder
    calls = _lift_size_rules(monkeypatch)
    torch.manual_seed(0)
    enc = base_encoder(obs_shape=(2, size, size), out_dim=128).cuda()
    obs = torch.rand(2, 1, size, size, device="cuda")
    state = (torch.rand(2, device="cuda") < 0.5).float()
    named = list(enc.named_parameters())
    monkeypatch.setattr(base_encoder, "fused_block", True)
    outs = []
    for planes in (True, False):
        monkeypatch.setattr(base_encoder, "fused_planes", planes)
        for _, p in named:
            p.grad = None
        calls.clear()
        y = enc.forward_split(obs, state)
        y.square().sum().backward()
        if planes:
            # K10 writes planes; every pooled block reads its predecessor's and writes its own; the chain ends in a plain K11 on planes.
            # (With the size rule lifted the 128 encoder's 256 -> 256 block and its last convolution are K11's too: a second, short chain.)
            want = [("first", False, True)] + [("pool", True, True)] * 3 + [("conv", True, False)]
            assert calls == want + ([("pool", False, True), ("conv", True, False)] if size == 128 else [])
        else:
            assert calls == [("first", False, False)]
        outs.append((y.detach().clone(), [p.grad.detach().clone() for _, p in named]))
    assert torch.equal(_bits(outs[0][0]), _bits(outs[1][0]))
    for (name, _), a, b in zip(named, outs[0][1], outs[1][1]):
        assert torch.equal(_bits(a), _bits(b)), name
        assert float(b.abs().max()) > 0, name


def test_one_robot_update_planes_against_the_fused_blocks(monkeypatch):
    """tests/test_conv_pool_gpu.py's smallest update with AURPPO_K11_POOL's blocks on both sides: the six loss scalars of every optimizer
    step, identical in every bit."""
    from aur_ppo_amd.base_cnns import base_encoder
    from tests.test_conv_pool_gpu import _one_update
    calls = _lift_size_rules(monkeypatch)
    monkeypatch.setattr(base_encoder, "fused_planes", False)
    off = _one_update(True, monkeypatch)
    assert not [c for c in calls if c[0] != "first"]
    monkeypatch.setattr(base_encoder, "fused_planes", True)
    on = _one_update(True, monkeypatch)
    assert len([c for c in calls if c[0] == "pool" and c[1] and c[2]]) >= 2 * 4 * 3, "K11x did not run"
    assert off.shape == on.shape and off.shape[0] == 4
    assert np.ascontiguousarray(on[:, :6]).tobytes() == np.ascontiguousarray(off[:, :6]).tobytes()
