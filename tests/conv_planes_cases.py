"""What the K11x suites share (tests/test_conv_planes_host.py, tests/test_conv_planes_gpu.py, tests/test_conv_planes_large_gpu.py): a
numpy restatement of the bf16x3 split (csrc/bf16x3.h::split3) and of the planes layout of include/aurppo.h, the shapes, and guarded
planes buffers.

The planes of an fp32 NCHW tensor x (B, C, H, W), C a multiple of 8: uint16 [B][C / 8][3][H * W][8]; plane 0 = bf16(a) rounded to
nearest even, plane 1 = bf16(a - plane 0), plane 2 = bf16(a - plane 0 - plane 1), every subtraction in fp32 (and exact).

NaN planes: the split of +-inf has NaN residuals (inf - inf), and IEEE 754 leaves a NaN's sign and payload to the implementation, so
``canonical`` maps every NaN bf16 pattern to 0x7fc0 before two sets of planes are compared; every other pattern is compared as it is."""
import numpy as np
import torch

from tests import conv_pool_cases as CP
from tests.encoder_cases import GUARD_BYTE, Guarded

AURPPO_EINVAL, AURPPO_ESHAPE = -1, -2     # include/aurppo.h

# (B, Ci, Co, H, W, pad): K11p's list, a 1 x 1 map, and a wide map whose 32-pixel blocks straddle rows and images (5 * 300 = 1500 pixels
# an image: no multiple of 32)
SHAPES = CP.SHAPES + [(1, 16, 32, 1, 1, 1), (2, 32, 64, 5, 300, 1)]
PADS = (0, 1, 2)
SPLIT_SHAPES = [(1, 8, 1, 1), (2, 16, 3, 5), (3, 48, 10, 10)]
K10_SHAPES = [(2, ci, 16, h, w) for ci in (1, 3) for (h, w) in ((8, 8), (6, 10))]


def with_pads(shapes, pooled):
    """Every shape under pad 0, 1 and 2 where the output is not empty (``pooled``: holds one whole 2 x 2 window)."""
    out = []
    for (B, Ci, Co, H, W, _) in shapes:
        for pad in PADS:
            ho, wo = H + 2 * pad - 2, W + 2 * pad - 2
            if (ho >= 2 and wo >= 2) if pooled else (ho >= 1 and wo >= 1):
                out.append((B, Ci, Co, H, W, pad))
    return out


def ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


# ------------------------------------------------------------------------------------------------------------- the split, restated
def bf16_rne(x):
    """float32 array -> (bf16 bits as uint16, the bf16 values as float32): round to nearest, ties to even; a NaN becomes 0x7fc0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    bits = np.where(np.isnan(x), 0x7FC0, bits).astype(np.uint16)
    return bits, (bits.astype(np.uint32) << 16).view(np.float32)


def split3(x):
    """The three planes (uint16 bits) of every element of the float32 array ``x``."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        p0, v0 = bf16_rne(x)
        r1 = (x - v0).astype(np.float32)
        p1, v1 = bf16_rne(r1)
        p2, _ = bf16_rne((r1 - v1).astype(np.float32))
    return p0, p1, p2


def join3(p0, p1, p2):
    f = lambda p: (p.astype(np.uint32) << 16).view(np.float32)
    return ((f(p0) + f(p1)).astype(np.float32) + f(p2)).astype(np.float32)


def canonical(planes):
    """uint16 planes with every NaN pattern mapped to 0x7fc0 (module docstring)."""
    p = np.asarray(planes).view(np.uint16)
    nan = ((p & 0x7F80) == 0x7F80) & ((p & 0x007F) != 0)
    return np.where(nan, np.uint16(0x7FC0), p)


def planes_np(x):
    """The planes tensor of a float32 (B, C, H, W) array: uint16 (B, C / 8, 3, H * W, 8)."""
    B, C, H, W = x.shape
    assert C % 8 == 0
    p = np.stack(split3(x), 0).reshape(3, B, C // 8, 8, H * W)          # [plane][b][g][j][pixel]
    return np.ascontiguousarray(p.transpose(1, 2, 0, 4, 3))              # [b][g][plane][pixel][j]


def wide_range(n, seed):
    """n float32 draws with |x| log-uniform over [2^-100, 2^100] and a random sign."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-100.0, 100.0, n))
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- guarded planes
class GuardedPlanes:
    """The planes of a (B, C, H, W) tensor as an int16 view (B, C / 8, 3, H * W, 8) into a 0xA5-filled byte buffer with guards either
    side; ``aligned=False`` starts it 2 bytes past a 16-byte boundary (a pointer the library must refuse)."""

    def __init__(self, B, C, H, W, aligned=True, like=None):
        n = 6 * B * C * H * W
        self.g = Guarded(n + 16, dtype=torch.uint8, aligned=True)
        off = 0 if aligned else 2
        self.view = self.g.view[off:off + n].view(torch.int16).view(B, C // 8, 3, H * W, 8)
        assert (self.view.data_ptr() % 16 == 0) == aligned
        self.slack = self.g.view[off + n:]
        self.head = self.g.view[:off]
        if like is not None:
            self.view.copy_(like)

    def guards_intact(self):
        return self.g.guards_intact() and bool((self.slack == GUARD_BYTE).all()) and bool((self.head == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.g.buf == GUARD_BYTE).all())


def same_planes(a, b):
    """Two int16 planes tensors hold the same bits (NaN patterns compared as one)."""
    return np.array_equal(canonical(a.detach().cpu().numpy()), canonical(b.detach().cpu().numpy()))
