"""What the K11p suites share (tests/test_conv_pool_host.py, tests/test_conv_pool_gpu.py, tests/test_conv_pool_large_gpu.py): the shapes
of aurppo_conv3x3_pool_f32, a restatement of its host-side plan, and the two references -- the two-launch pair K11 -> K9 through the C
ABI (bit for bit) and the fp64 ``conv -> + bias -> relu -> max_pool`` with the sum of |products| behind every window.

Shapes are (B, Ci, Co, H, W, pad) as in tests/encoder_cases.py.  A "window" is one pooled element: Hp x Wp = ((H + 2 pad - 2) >> 1, ...)
per image and channel; a 32-lane block of the kernel holds 8 consecutive windows of the flattened (b, ho, wo), a workgroup 64."""
import torch

from tests.encoder_cases import conv64

SHAPES = [
    (1, 16, 16, 2, 2, 1),        # 1 window; half a channel block
    (4, 16, 48, 8, 8, 1),        # 64 windows: exactly one workgroup; NB 2 with a half-empty block
    (1, 16, 32, 2, 130, 1),      # 65 windows: one workgroup plus one window
    (3, 48, 160, 10, 10, 1),     # 75 windows; image boundaries at 25 and 50 fall inside 8-window blocks; NB 4 in two groups, the second
                                 # with one block of four
    (2, 16, 80, 7, 9, 1),        # odd H and W: the last row and column are in no window
    (2, 16, 32, 8, 8, 0),        # pad 0, the 256 -> 256 valid block's 6 x 6 -> 3 x 3 geometry
    (2, 16, 80, 3, 4, 2),        # pad 2
    (1, 32, 64, 21, 21, 1),      # config 5's odd map; two channel groups per tap
    (1, 48, 48, 2, 2, 2),        # most taps outside the image
]
REFUSED = (5, 48, 16, 1, 1, 1)   # Hp = 0: AURPPO_ESHAPE with nothing written
IDS = ["x".join(map(str, s)) for s in SHAPES]

# shape -> (windows, workgroups along the windows, NB, channel groups)
CLAIMS = {
    (1, 16, 16, 2, 2, 1): (1, 1, 1, 1),
    (4, 16, 48, 8, 8, 1): (64, 1, 2, 1),
    (1, 16, 32, 2, 130, 1): (65, 2, 1, 1),
    (3, 48, 160, 10, 10, 1): (75, 2, 4, 2),
    (2, 16, 80, 7, 9, 1): (24, 1, 2, 2),
    (2, 16, 32, 8, 8, 0): (18, 1, 1, 1),
    (2, 16, 80, 3, 4, 2): (12, 1, 2, 2),
    (1, 32, 64, 21, 21, 1): (100, 2, 2, 1),
    (1, 48, 48, 2, 2, 2): (4, 1, 2, 1),
}

AURPPO_ESHAPE = -2     # include/aurppo.h


def pooled(H, W, pad):
    return (H + 2 * pad - 2) >> 1, (W + 2 * pad - 2) >> 1


def plan(B, Ci, Co, H, W, pad):
    """(windows, workgroups along the windows, NB, channel groups) of aurppo_conv3x3_pool_f32, restated from csrc/conv.hip."""
    hp, wp = pooled(H, W, pad)
    q = B * hp * wp
    nblk = (Co + 31) // 32
    nb = 4 if nblk >= 4 else (2 if nblk >= 2 else 1)
    return q, (4 * q + 255) // 256, nb, (nblk + nb - 1) // nb


def inputs(shape, seed=0, device="cpu"):
    """x, w, bias of a shape: unit-normal activations, a filter of He scale, a bias large enough to move windows across zero."""
    B, Ci, Co, H, W, pad = shape
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (9 * Ci)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.5
    return x.to(device), w.to(device), b.to(device)


def block64(x, w, bias, pad):
    """fp64 ``max_pool2d(relu(conv2d(x, w) + bias), 2)`` and, per pooled element, the largest sum of |products| + |bias| among its
    window's four pixels: ReLU and max are 1-Lipschitz, so K11's bound on a pre-activation carries through to the window."""
    z = conv64(x, w, pad)
    mag = conv64(x.abs(), w.abs(), pad)
    if bias is not None:
        z = z + bias.double().reshape(1, -1, 1, 1)
        mag = mag + bias.double().abs().reshape(1, -1, 1, 1)
    y = torch.nn.functional.max_pool2d(torch.relu(z), 2)
    return y, torch.nn.functional.max_pool2d(mag, 2)
