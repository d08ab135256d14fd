"""GPU: K11 on planes (aurppo_conv3x3_planes_f32) at the two sizes where its addressing changes: a planes tensor just under the buffer
builds' limit (4 GiB - 1 MiB of planes: 32-bit byte offsets, the largest they get) and one just over 2^32 bytes (64-bit addresses with a
zero select).  An offset that wraps or a limit taken in the wrong unit shows at no smaller size.  Planes hold 6 bytes an element, so
both sizes come 1.5 x sooner than for fp32 -- at both, the fp32 kernel it is compared with still runs its buffer build.

Each case follows tests/test_conv_pool_large_gpu.py: the batch is a tile of P = 7 base images, and a strided sample of output images --
both ends of the batch, and the images either side of byte 2^31 and byte 2^32 of the planes -- is compared, bit for bit, with the fp32
kernel's result on the base images.  A case skips only when the device has less than twice its memory free."""
import gc

import pytest
import torch

from tests import encoder_cases as E

pytestmark = pytest.mark.gpu

P = 7
BUF_LIMIT = (1 << 32) - (1 << 20)


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


# (B, Ci, Co, H, W, pad): an image's planes are 6 * 16 * 16 * 16 = 24 576 bytes
LARGE = [
    pytest.param((174719, 16, 16, 16, 16, 1), 8.0, True, id="buf-just-under-4GiB-of-planes"),       # the limit less one image: 174 720 images are the limit itself
    pytest.param((174763, 16, 16, 16, 16, 1), 8.0, False, id="64bit-just-over-4GiB-of-planes"),     # 2^32 + 8 192 bytes
]


@pytest.mark.parametrize("shape,gib,buf", LARGE)
def test_a_sample_of_a_tiled_batch_equals_the_fp32_kernel_on_its_base_image(lib, shape, gib, buf):
    B, Ci, Co, H, W, pad = shape
    img = 6 * Ci * H * W
    assert (B * img < BUF_LIMIT) == buf
    assert (BUF_LIMIT - img <= B * img) if buf else (1 << 32) < B * img < (1 << 32) + (1 << 20)
    assert E.k11_plan(B, Ci, Co, H, W)[1]            # the fp32 tensor, two thirds the size, is under its own limit
    _need(gib)
    g = torch.Generator(device="cuda").manual_seed(B)
    base = torch.randn(P, Ci, H, W, device="cuda", generator=g)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=g) * (2.0 / (9 * Ci)) ** 0.5
    ws = E.Workspace(lib.aurppo_conv3x3_wop_bytes(Ci, Co))
    ref = torch.empty(P, Co, H, W, device="cuda")
    assert lib.aurppo_conv3x3_f32(E.ptr(base), E.ptr(w), E.ptr(ref), P, Ci, Co, H, W, pad, 0, E.ptr(ws.view), E.stream()) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ref).any())
    # the planes of the tiled batch: the base images' planes, tiled (the split is a function of the value alone)
    bp = torch.empty(P, Ci // 8, 3, H * W, 8, dtype=torch.int16, device="cuda")
    assert lib.aurppo_split_planes_f32(E.ptr(base), E.ptr(bp), P, Ci, H, W, E.stream()) == 0
    xp = E.tile_images(bp, B)
    assert xp.is_contiguous() and xp.numel() * 2 == B * img and xp.data_ptr() % 16 == 0
    del bp
    z = torch.full((B, Co, H, W), float("nan"), device="cuda")
    rc = lib.aurppo_conv3x3_planes_f32(E.ptr(xp), E.ptr(w), E.ptr(z), B, Ci, Co, H, W, pad, E.ptr(ws.view), E.stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.aurppo_last_error()
    assert ws.guards_intact()
    del xp
    # both ends, both crossings (the images that hold byte 2^31 and byte 2^32 - 1 of the planes, with their neighbours), and every 997th
    picks = set(range(0, B, 997)) | set(range(8)) | set(range(B - 8, B))
    for byte in ((1 << 31), (1 << 32) - 1):
        b = min(byte // img, B - 1)
        picks |= set(range(max(b - 3, 0), min(b + 4, B)))
    idx = torch.tensor(sorted(picks), device="cuda")
    got = z[idx].view(torch.int32)
    assert torch.equal(got, ref.view(torch.int32)[idx % P]), "a sampled image differs"        # (a NaN left behind has other bits)
