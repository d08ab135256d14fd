"""GPU: K11p (aurppo_conv3x3_pool_f32) at the tensor sizes the robot benchmark gives it, where K11 takes an addressing case per size
range: 32-bit byte offsets through a buffer resource up to 4 GB (the BUF builds; the 16 -> 32 block's input of 8,192 images is exactly
2^31 bytes), 64-bit addresses from there on.  An addressing error that begins at byte 2^31 or 2^32 shows at no smaller size.

The periodic construction of tests/test_encoder_large_gpu.py keeps the reference small: the batch is a tile of P = 7 base images (7
divides no power of two, so the image 2^31 or 2^32 bytes away has another residue) and EVERY output image is compared, bit for bit,
with the two-launch result K11 -> K9 of its base image.  Outputs are NaN / 0xA5-filled before the call and none of either may be left.
A case skips only when the device has less than twice its memory free."""
import gc

import pytest
import torch

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

P = 7


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


LARGE = [
    pytest.param((8192, 16, 32, 64, 64, 1), 4.0, True, id="buf-2GiB-the-16-to-32-block"),       # x 2^31 bytes, y 1 GiB
    pytest.param((4194304 + 4099, 16, 16, 4, 4, 1), 6.0, False, id="64bit-4GiB"),              # x 4 GiB + 4 MB, y 1 GiB
]


@pytest.mark.parametrize("shape,gib,buf", LARGE)
def test_every_image_of_a_tiled_batch_equals_the_two_launches_on_its_base_image(lib, shape, gib, buf):
    B, Ci, Co, H, W, pad = shape
    assert E.k11_plan(B, Ci, Co, H, W)[1] == buf
    x_bytes = B * Ci * H * W * 4
    assert x_bytes == (1 << 31) if buf else x_bytes > (1 << 32)
    _need(gib)
    g = torch.Generator(device="cuda").manual_seed(B)
    base = torch.randn(P, Ci, H, W, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * (2.0 / (9 * Ci)) ** 0.5
    bias = torch.randn(Co, device="cuda", generator=g) * 0.5
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    Hp, Wp = Ho // 2, Wo // 2
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    # the base images through the two launches
    z = torch.empty(P, Co, Ho, Wo, device="cuda")
    ry = torch.empty(P, Co, Hp, Wp, device="cuda")
    rmask = torch.empty(P, Co, Hp, Wp, dtype=torch.uint8, device="cuda")
    assert lib.aurppo_conv3x3_f32(E.ptr(base), E.ptr(w), E.ptr(z), P, Ci, Co, H, W, pad, 0, E.ptr(ws.view), E.stream()) == 0
    assert lib.aurppo_bias_relu_pool2_fwd_f32(E.ptr(z), E.ptr(bias), None, None, E.ptr(ry), E.ptr(rmask), P, Co, Ho, Wo, E.stream()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ry).any()) and set(rmask.unique().tolist()) == {0, 1, 2, 3, 4}
    x = E.tile_images(base, B)
    assert x.numel() * 4 == x_bytes
    y = torch.full((B, Co, Hp, Wp), float("nan"), device="cuda")
    mask = torch.full((B, Co, Hp, Wp), E.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    rc = lib.aurppo_conv3x3_pool_f32(E.ptr(x), E.ptr(w), E.ptr(bias), E.ptr(y), E.ptr(mask), B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert ws.guards_intact()
    del x
    idx = torch.arange(B, device="cuda") % P
    ry_bits = ry.view(torch.int32)
    chunk = max(P, (128 << 20) // (ry[0].numel() * 4))
    for b0 in range(0, B, chunk):
        sl = slice(b0, b0 + chunk)
        assert torch.equal(y[sl].view(torch.int32), ry_bits[idx[sl]]), f"y of images {b0}.."        # (a NaN left behind has other bits)
        assert torch.equal(mask[sl], rmask[idx[sl]]), f"mask of images {b0}.."
