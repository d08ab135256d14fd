"""GPU: the encoder kernels at the tensor sizes the robot benchmark gives them -- 2^31 bytes and more, where K11 takes an addressing
case per size range (32-bit byte offsets through a buffer resource that may wrap; 64-bit addresses from 4 GB on) and K12 caps its
buffer sizes at 2^31 and re-bases every slice on its first image.  An addressing error that begins at byte 2^31 shows at no smaller size.

The reference stays small by structure, not by sampling: every tensor is a tile of P = 7 base images (7 divides no power of two, so the
image 2^31 or 2^32 bytes away has another residue), and
* K11, K9, K10 (forward) work per image: EVERY output image is compared with the reference of its base image;
* K12 and the K9 / K10 gradient sums add over images: dy[b] = s_b * G[b mod P] with a random 0/1 mask s, so the products are exact and
  the reference is sum_r n_r dW_r with n_r the mask's count over residue r (tests/test_encoder_cases_host.py checks the construction
  against the direct fp64 result); an image read from elsewhere carries another mask bit and another residue.
Outputs are NaN-filled before the call and no NaN may be left.  A case skips only when the device has less than twice its memory free."""
import gc

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

P = 7
BOUND = 1e-6        # of the sum of |products| behind an element (tests/test_conv_gpu.py)


@pytest.fixture(scope="module")
def lib():
    from aur_ppo_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _free_between_cases():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _need(gib):
    gc.collect()
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 2 * gib * (1 << 30):
        pytest.skip(f"{free / 2 ** 30:.1f} GiB free on the device, the case needs {gib:.1f} GiB and asks for twice that")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# =================================================================================================================== K11
# (B, cin, cout, H, W, p, mode) as tests/encoder_cases.py names a product
K11_LARGE = [
    pytest.param((12288, 16, 32, 64, 64, 1, 0), 10.0, True, id="buf-3GiB-forward"),        # x 3 GiB, z 6 GiB: the 16 -> 32 block
    pytest.param((6144, 32, 16, 64, 64, 1, 1), 5.0, True, id="buf-3GiB-input-gradient"),    # x = dY of that block, 3 GiB; z 1.5 GiB
    pytest.param((4194304 + 4099, 16, 16, 4, 4, 0, 0), 5.5, False, id="64bit-4GiB-forward"),  # x 4 GiB + 4 MB, z a quarter of it
]


@pytest.mark.parametrize("case,gib,buf", K11_LARGE)
def test_k11_every_image_of_a_tiled_batch_meets_its_base_image(lib, case, gib, buf):
    B, cin, cout, H, W, p, mode = case
    assert E.k11_plan(B, cin, cout, H, W)[1] == buf
    x_bytes = B * cin * H * W * 4
    assert x_bytes > (1 << 31) and (buf or x_bytes > (1 << 32))
    _need(gib)
    g = _gen(B + mode)
    base = torch.randn(P, cin, H, W, device="cuda", generator=g)
    if mode == 0:
        w = torch.randn(cout, cin, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
        args = (B, cin, cout, H, W, p, 0)
        ref, mag = E.conv64(base, w, p), E.conv64(base.abs(), w.abs(), p)
    else:
        w = torch.randn(cin, cout, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5
        args = (B, cout, cin, H, W, 2 - p, 1)
        ref, mag = E.dgrad64(base, w, 2 - p), E.dgrad64(base.abs(), w.abs(), 2 - p)
    x = E.tile_images(base, B)
    z = torch.full((B, cout, H + 2 * p - 2, W + 2 * p - 2), float("nan"), device="cuda")
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(cin, cout))
    rc = lib.aurppo_conv3x3_f32(E.ptr(x), E.ptr(w), E.ptr(z), *args, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert ws.guards_intact()
    del x
    per_image = z[0].numel() * 12
    err = E.compare_periodic(z, ref, mag, images_per_chunk=max(P, (256 << 20) // per_image))
    print(f"\nK11 {case}: worst of {B} images {err:.3e} of sum|ab|")
    assert err <= BOUND        # (NaN -- an element never written, or one computed from a guard -- fails this too)


# =================================================================================================================== K12
# (B, Ci, Co, H, W, pad): dy over 2^31 bytes (the 32 -> 64 block: 8192 images of dy are exactly 2^31 bytes; with 8800 the first slices'
# buffer of dy is capped at 2^31 and the later ones' is not); then both x and dy over 2^31 bytes
K12_LARGE = [
    pytest.param((8800, 32, 64, 32, 32, 1), 4.0, id="dy-over-2GiB"),
    pytest.param((8800, 64, 64, 32, 32, 1), 5.0, id="x-and-dy-over-2GiB"),
]


@pytest.mark.parametrize("shape,gib", K12_LARGE)
def test_k12_masked_tiled_batch_meets_the_weighted_sum_of_base_gradients(lib, shape, gib):
    B, Ci, Co, H, W, pad = shape
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    nbytes = lib.aurppo_conv3x3_wgrad_ws_bytes(*shape)
    S = E.k12_slices_from_ws(nbytes, Ci, Co)
    plan = E.k12_plan(*shape)
    assert S > 1 and S == plan["S"]
    # some slice begins beyond byte 2^31 of every tensor that is that large; an early slice's buffer is capped, the last one's is not
    b_last = ((S - 1) * plan["pps"]) // (Ho * Wo)
    img_dy, img_x = Co * Ho * Wo * 4, Ci * H * W * 4
    assert B * img_dy > (1 << 31) and b_last * img_dy > (1 << 31) and (B - b_last) * img_dy < (1 << 31)
    if B * img_x > (1 << 31):
        assert b_last * img_x > (1 << 31) and (B - b_last) * img_x < (1 << 31)
    else:
        assert shape[1] == 32
    _need(gib)
    g = _gen(B + Ci)
    base_x = torch.randn(P, Ci, H, W, device="cuda", generator=g)
    base_g = torch.randn(P, Co, Ho, Wo, device="cuda", generator=g)
    s = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
    ref, mag = E.structured_wgrad64(base_x, base_g, s, Co, pad)
    x = E.tile_images(base_x, B)
    dy = E.tile_images(base_g, B)
    dy.mul_(s.view(-1, 1, 1, 1))
    dw = E.Guarded(Co, Ci, 3, 3)
    ws = E.Workspace(nbytes)
    rc = lib.aurppo_conv3x3_wgrad_f32(E.ptr(dy), E.ptr(x), E.ptr(dw.view), *shape, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert dw.guards_intact() and ws.guards_intact() and dw.written()
    err = E.rel_err(dw.view, ref, mag)
    print(f"\nK12 {shape}: S = {S}, {plan['pps']} pixels per slice, {err:.3e} of sum|ab|")
    assert err <= BOUND


# =================================================================================================================== K9
def test_k9_at_8192_images_equals_torch_on_the_base_images(lib):
    """The 32-channel block of the 128 x 128 encoder at the benchmark's minibatch: x is 2^32 bytes, dx too.  y and dx of EVERY image are
    bit-equal to torch's op chain on its base image; the bias sums meet the n_r-weighted fp64 sums of torch's per-image bias gradients
    at the tolerance of tests/test_hip_parity.py."""
    B, C_, H, W = 8192, 32, 64, 64
    Ho, Wo = H // 2, W // 2
    _need(7.0)
    g = _gen(9)
    base = torch.randn(P, C_, H, W, device="cuda", generator=g)
    base[0, 0].fill_(0.25)
    bias = torch.randn(C_, device="cuda", generator=g)
    base_g = torch.randn(P, C_, Ho, Wo, device="cuda", generator=g)
    s = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
    xr = base.clone().requires_grad_(True)
    yr = F.max_pool2d(F.relu(xr + bias.view(1, -1, 1, 1)), 2)
    yr.backward(base_g)
    ry, rdx = yr.detach(), xr.grad
    rdb_images = rdx.double().sum((2, 3))                       # (P, C): an image's bias gradient is the sum of its routed gradients
    x = E.tile_images(base, B)
    assert x.numel() * 4 == 1 << 32
    y = torch.full((B, C_, Ho, Wo), float("nan"), device="cuda")
    mask = torch.full((B, C_, Ho, Wo), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.aurppo_bias_relu_pool2_fwd_f32(E.ptr(x), E.ptr(bias), None, None, E.ptr(y), E.ptr(mask), B, C_, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    del x
    idx = torch.arange(B, device="cuda") % P

    def every_image_equals(t, ref, chunk=448):
        for b0 in range(0, B, chunk):
            if not torch.equal(t[b0:b0 + chunk], ref[idx[b0:b0 + chunk]]):
                return False
        return True
    assert every_image_equals(y, ry)
    dy = E.tile_images(base_g, B)
    dy.mul_(s.view(-1, 1, 1, 1))
    del y
    dx = torch.full((B, C_, H, W), float("nan"), device="cuda")
    part = E.Guarded(B, C_)
    rc = lib.aurppo_bias_relu_pool2_bwd_f32(E.ptr(dy), E.ptr(mask), E.ptr(dx), E.ptr(part.view), B, C_, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert part.guards_intact() and part.written()
    for b0 in range(0, B, 448):
        sl = slice(b0, b0 + 448)
        assert torch.equal(dx[sl], rdx[idx[sl]] * s[sl].view(-1, 1, 1, 1)), f"dx of images {b0}.."
    n = E.residue_counts(s, P)
    want = (n.view(P, 1) * rdb_images).sum(0)
    n_terms = B * Ho * Wo
    torch.testing.assert_close(part.view.double().sum(0), want, rtol=1e-5, atol=2e-7 * n_terms ** 0.5 * float(base_g.abs().max()) + 1e-6)


# =================================================================================================================== K10
def test_k10_at_8192_images_meets_torch_on_the_base_images(lib):
    """The first block at the benchmark's minibatch (8192 x 1 x 128 x 128 -> 16 channels): every image of y against the MIOpen-free
    torch block of its base image at the tolerance of tests/test_hip_parity.py, and the per-image partial sums, added in fp64, against
    the n_r-weighted sums of torch's per-image gradients at that test's gradient tolerance."""
    B, Ci, Co, H, W = 8192, 1, 16, 128, 128
    Ho, Wo, NT = H // 2, W // 2, (Ci + 1) * 9
    _need(6.0)
    g = _gen(10)
    base = torch.rand(P, Ci, H, W, device="cuda", generator=g)
    base_state = torch.tensor([1., 0., 1., 1., 0., 0., 1.], device="cuda")
    w = 0.3 * torch.randn(Co, Ci + 1, 3, 3, device="cuda", generator=g)
    b = 0.1 * torch.randn(Co, device="cuda", generator=g)
    base_g = torch.randn(P, Co, Ho, Wo, device="cuda", generator=g)
    s = (torch.rand(B, device="cuda", generator=g) < 0.5).float()
    ry, rdw, rdb = [], [], []
    for r in range(P):                                          # per base image: its own weight and bias gradient
        w1, b1 = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        xin = torch.cat([base[r:r + 1], base_state[r].view(1, 1, 1, 1).expand(1, 1, H, W)], 1)
        with torch.backends.cudnn.flags(enabled=False):
            yr = F.max_pool2d(F.relu(F.conv2d(xin, w1, b1, padding=1)), 2)
            yr.backward(base_g[r:r + 1])
        ry.append(yr.detach()[0]); rdw.append(w1.grad.double()); rdb.append(b1.grad.double())
    ry = torch.stack(ry)
    n = E.residue_counts(s, P)
    want_w = sum(n[r] * rdw[r] for r in range(P))
    want_b = sum(n[r] * rdb[r] for r in range(P))
    idx = torch.arange(B, device="cuda") % P
    obs, state = E.tile_images(base, B), base_state[idx].contiguous()
    y = torch.full((B, Co, Ho, Wo), float("nan"), device="cuda")
    mask = torch.full((B, Co, Ho, Wo), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.aurppo_first_block_fwd_f32(E.ptr(obs), E.ptr(w), E.ptr(b), E.ptr(state), E.ptr(y), E.ptr(mask), B, Ci, Co, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    for b0 in range(0, B, 896):
        sl = slice(b0, b0 + 896)
        torch.testing.assert_close(y[sl], ry[idx[sl]], rtol=1e-5, atol=2e-6)
    dy = E.tile_images(base_g, B)
    dy.mul_(s.view(-1, 1, 1, 1))
    del y
    dwp, dbp = E.Guarded(B * (Co // 16), 16, NT), E.Guarded(B * (Co // 16), 16)
    rc = lib.aurppo_first_block_bwd_f32(E.ptr(dy), E.ptr(mask), E.ptr(obs), E.ptr(state), E.ptr(dwp.view), E.ptr(dbp.view),
                                        B, Ci, Co, H, W, E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert dwp.guards_intact() and dbp.guards_intact() and dwp.written() and dbp.written()
    dw = dwp.view.double().view(B, Co // 16, 16, NT).sum(0).reshape(Co, Ci + 1, 3, 3)
    db = dbp.view.double().view(B, Co // 16, 16).sum(0).reshape(Co)
    sw, sb = float(want_w.abs().max()), float(want_b.abs().max())
    ew, eb = float((dw - want_w).abs().max()), float((db - want_b).abs().max())
    print(f"\nK10 at {B} images: weight sums off by {ew:.3e} of a largest {sw:.3e}, bias sums by {eb:.3e} of {sb:.3e}")
    assert ew <= 2e-5 * sw + 1e-6
    assert eb <= 2e-5 * sb + 1e-6
