"""What the encoder suites share (tests/test_encoder_edges_gpu.py, tests/test_encoder_large_gpu.py, tests/test_encoder_cases_host.py):
the shapes, guarded views, the fp64 references of K11 / K12, the periodic and masked constructions of the large cases, and a restatement
of the host-side plans of csrc/conv.hip (which kernel build a call takes, how K12 cuts its pixels into slices).

Shapes are (B, Ci, Co, H, W, pad): the filter is (Co, Ci, 3, 3), ``pad`` the FORWARD padding, H x W the map K11's mode 0 and K12 read.
For K11's mode 1 (the input gradient) the same tuple names the product: Ci channels in, Co out, ``pad`` the product's own padding; the
filter handed to the entry point is then (Ci, Co, 3, 3) and its ``pad`` argument 2 - pad."""
import ctypes as C

import numpy as np
import torch

GUARD = 64          # elements of guard either side of a view
SHIFT = 3           # a shifted view starts 3 elements past a 16-byte boundary
GUARD_BYTE = 0xA5   # the uint8 guard (pool masks hold 0..4)


class Guarded:
    """A tensor of ``shape`` as a view into a guard-filled buffer: GUARD elements, the view, GUARD elements.  float32: NaN guards and a
    NaN-filled view; uint8: GUARD_BYTE.  ``aligned``: the view starts at a 16-byte boundary, otherwise SHIFT elements past one (float32:
    4-byte aligned and not 16; uint8: odd).  ``like``: the view's contents (an input of exactly its size); without it the view is an
    output that the kernel must fill."""

    def __init__(self, *shape, dtype=torch.float32, aligned=False, like=None, device="cuda"):
        n = int(np.prod(shape))
        item = 4 if dtype == torch.float32 else 1
        assert dtype in (torch.float32, torch.uint8)
        self.fill = float("nan") if dtype == torch.float32 else GUARD_BYTE
        self.buf = torch.full((GUARD + 16 + SHIFT + n + GUARD,), self.fill, dtype=dtype, device=device)
        base = (-self.buf.data_ptr() % 16) // item           # elements to the next 16-byte boundary
        self.lo = base + GUARD + (0 if aligned else SHIFT)   # (GUARD elements are a multiple of 16 bytes)
        self.n = n
        self.view = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.view.is_contiguous() and (self.view.data_ptr() % 16 == 0) == bool(aligned)
        assert self.lo >= GUARD and self.buf.numel() - (self.lo + n) >= GUARD
        if like is not None:
            self.view.copy_(like)

    def _is_guard(self, t):
        return bool(torch.isnan(t).all()) if self.buf.dtype == torch.float32 else bool((t == GUARD_BYTE).all())

    def guards_intact(self):
        return self._is_guard(self.buf[:self.lo]) and self._is_guard(self.buf[self.lo + self.n:])

    def written(self):
        """No element of the view still holds the fill (outputs of finite inputs: every element was stored)."""
        v = self.view
        return not bool((torch.isnan(v) if v.dtype == torch.float32 else v == GUARD_BYTE).any())


class Workspace:
    """Exactly ``nbytes`` bytes at a 16-byte boundary, every byte 0xFF (a float NaN, a bf16 NaN), 256 guard bytes of 0xFF behind them."""
    TAIL = 256

    def __init__(self, nbytes, device="cuda"):
        self.buf = torch.full((16 + nbytes + self.TAIL,), 0xFF, dtype=torch.uint8, device=device)
        self.lo = -self.buf.data_ptr() % 16
        self.n = int(nbytes)
        self.view = self.buf[self.lo:self.lo + self.n]
        assert self.view.data_ptr() % 16 == 0

    def guards_intact(self):
        return bool((self.buf[:self.lo] == 0xFF).all()) and bool((self.buf[self.lo + self.n:] == 0xFF).all())


def ptr(t):
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------- shapes
# K11 (both modes).  B * Ho * Wo in the comment; NB from the output channels: 16 -> 1; 48 -> 2 (second block half empty); 80 -> 2 (two
# groups, the last one half absent: its slack group of the operand copy is never written); 160 -> 4 (two groups, 3 of 4 blocks absent)
K11_SHAPES = [
    (1, 16, 16, 5, 7, 1),        # 35 pixels: one partial pixel block, the wave's second block and three waves idle
    (4, 16, 48, 8, 8, 1),        # 256: exactly one workgroup; four images, boundaries at 64 = inside no block
    (1, 48, 80, 1, 257, 1),      # 257: one workgroup plus one pixel; a one-row image (rows -1 and 1 are outside for every pixel)
    (3, 48, 160, 10, 10, 1),     # 300: image boundaries at 100, 200 fall inside 32-pixel blocks
    (2, 16, 160, 7, 6, 0),       # pad 0; 40 pixels, boundary at 20
    (2, 16, 80, 3, 4, 2),        # pad 2; 60 pixels, boundary at 30
    (5, 48, 16, 1, 1, 1),        # a 1 x 1 image with pad 1: every tap but the centre is outside
    (1, 48, 48, 2, 2, 2),        # pad 2 on a 2 x 2 image: 16 pixels, most taps outside
]

# K12.  M = B * Ho * Wo; S, pixels per slice, the last slice's pixels and the chunk counts are asserted in test_encoder_cases_host.py
# against ``K12_CLAIMS`` below.
K12_SHAPES = [
    (2, 16, 48, 4, 4, 1),        # M 32: one chunk; QUAD, W = 4 with pad 1 (every quad touches both row ends); Co 48 < one tile
    (3, 16, 64, 4, 4, 1),        # M 48: two chunks (prologue only, no steady state); QUAD; Co 64 = WM 1 full
    (5, 16, 65, 4, 4, 1),        # M 80: three chunks (odd last step); QUAD; Co 65 = WM 2 with one row in the second half
    (2, 16, 160, 5, 5, 1),       # M 50: non-QUAD (Wo 5), WM 2, a ragged second tile along Co (32 of 128 rows)
    (3, 16, 64, 2, 6, 2),        # M 96: three full chunks; non-QUAD because of pad 2 (Wo 8 is a multiple of 4), WM 1
    (2, 16, 48, 6, 6, 0),        # M 32: QUAD with pad 0
    (1, 16, 160, 3, 4, 2),       # M 30: non-QUAD, WM 2, pad 2, a chunk that is not full
    (37, 16, 64, 12, 12, 1),     # M 5328: S 11 slices of 512 pixels, the last 208 (6.5 chunks); slices begin inside images; QUAD
    (23, 16, 65, 17, 17, 0),     # M 5175: S 6 slices of 864, the last 855 (26 chunks + 23 pixels); non-QUAD (Wo 15); WM 2
]
# shape -> (S, pixels per slice, pixels of the last slice, chunks of a full slice, chunks of the last slice, QUAD, WM)
K12_CLAIMS = {
    (2, 16, 48, 4, 4, 1): (1, 32, 32, 1, 1, True, 1),
    (3, 16, 64, 4, 4, 1): (1, 64, 48, 2, 2, True, 1),
    (5, 16, 65, 4, 4, 1): (1, 96, 80, 3, 3, True, 2),
    (2, 16, 160, 5, 5, 1): (1, 64, 50, 2, 2, False, 2),
    (3, 16, 64, 2, 6, 2): (1, 96, 96, 3, 3, False, 1),
    (2, 16, 48, 6, 6, 0): (1, 32, 32, 1, 1, True, 1),
    (1, 16, 160, 3, 4, 2): (1, 32, 30, 1, 1, False, 2),
    (37, 16, 64, 12, 12, 1): (11, 512, 208, 16, 7, True, 1),
    (23, 16, 65, 17, 17, 0): (6, 864, 855, 27, 27, False, 2),
}

# K9: (B, C, H, W, with_plane).  H * W <= 1024 takes the wave-per-plane build (four planes per workgroup), above it a workgroup per plane.
K9_SHAPES = [
    (3, 3, 6, 6, False),         # 9 planes: the last workgroup of the wave-per-plane build has one live wave
    (1, 5, 32, 32, True),        # H * W = 1024: the last size of the wave-per-plane build; 5 planes; B = 1
    (3, 3, 257, 4, True),        # H * W = 1028: the first size of the workgroup-per-plane build; odd H; B = 3
    (4, 2, 8, 12, True),         # W a multiple of 4, B = 4 (k_weighted_batch_sum: one full group of four)
    (5, 3, 7, 9, True),          # odd H and odd W (scalar path whatever the alignment), B = 5 (a group of four and one)
    (2, 5, 33, 36, False),       # odd H with a vector-width W on the large build
    (1, 1, 2, 2, False),         # the smallest plane
]

# K10: (B, Ci, Co, H, W)
K10_HW = [(2, 3), (3, 3), (7, 9), (12, 12), (2, 514)]      # the last: Ho * Wo = 257, a second workgroup along x with one live thread
K10_SHAPES = [(2, ci, co, h, w) for ci in (1, 2, 3) for co in (16, 48) for (h, w) in K10_HW]


# ------------------------------------------------------------------------------------------------------------- host-side plans
def k11_plan(B, cin, cout, H, W):
    """(NB, BUF) of aurppo_conv3x3_f32, restated: NB from the 32-channel blocks of the output, BUF while the input is under 4 GB - 1 MB."""
    nblk = (cout + 31) // 32
    nb = 4 if nblk >= 4 else (2 if nblk >= 2 else 1)
    buf = B * cin * H * W * 4 < (1 << 32) - (1 << 20)
    return nb, buf


def _slices_for(tiles, most):
    most = min(max(most, 1), 4096)
    best, best_util, S = 1, 0.0, 1
    while S <= most and tiles * S <= 4 * 512:
        wgs = tiles * S
        rounds = (wgs + 511) // 512
        util = wgs / (rounds * 512)
        if util > best_util + 0.02:
            best_util, best = util, S
        S += 1
    return best


def k12_plan(B, Ci, Co, H, W, pad):
    """conv_wgrad_plan of csrc/conv.hip, restated: dict(WM, tiles, S, pps, last, chunks, chunks_last, quad).  The library's own slice count
    is (aurppo_conv3x3_wgrad_ws_bytes - 64) / (Co * Ci * 36); test_encoder_cases_host.py holds the two together."""
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    M, HoWo, HW = B * Ho * Wo, Ho * Wo, H * W
    WM = 2 if Co > 64 else 1
    tiles = ((Co + 64 * WM - 1) // (64 * WM)) * ((Ci * 9 + 64 * (4 // WM) - 1) // (64 * (4 // WM)))
    S = _slices_for(tiles, (M + 511) // 512)
    pps = ((M + S - 1) // S + 31) // 32 * 32
    per_img = 4 * max(HoWo * Co, HW * Ci)
    while pps > 32 and ((pps // HoWo + 2) * per_img >= (1 << 31) or pps + HoWo >= (1 << 23)):
        pps = (pps // 2 + 31) // 32 * 32
    S = (M + pps - 1) // pps
    last = M - (S - 1) * pps
    return dict(WM=WM, tiles=tiles, S=S, pps=pps, last=last, chunks=(min(pps, M) + 31) // 32, chunks_last=(last + 31) // 32,
                quad=Wo % 4 == 0 and W >= 4 and pad <= 1, M=M, HoWo=HoWo)


def k12_slices_from_ws(ws_bytes, Ci, Co):
    assert ws_bytes > 64 and (ws_bytes - 64) % (Co * Ci * 36) == 0
    return (ws_bytes - 64) // (Co * Ci * 36)


# ------------------------------------------------------------------------------------------------------------- fp64 references
def conv64(x, w, pad):
    return torch.nn.functional.conv2d(x.double(), w.double(), None, stride=1, padding=pad)


def dgrad64(g, w, pad_fwd):
    """d conv2d(., w, padding = pad_fwd) / d input applied to g: what K11's mode 1 computes."""
    return torch.nn.functional.conv_transpose2d(g.double(), w.double(), None, stride=1, padding=pad_fwd)


def wgrad64(x, g, Co, pad):
    """The fp64 weight gradient of conv2d(x, w, padding = pad) under the output gradient g."""
    wd = torch.zeros(Co, x.shape[1], 3, 3, device=x.device, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double(), wd, None, padding=pad).backward(g.double())
    return wd.grad


def rel_err(got, ref, mag):
    """Worst |got - ref| over the sum of |products| behind the element (``mag``), every element counted."""
    return float(((got.double() - ref).abs() / mag.clamp_min(1e-30)).max())


# ------------------------------------------------------------------------------------------------------------- periodic tensors
def tile_images(base, B):
    """(B, ...) whose image b is base[b mod P]."""
    P = base.shape[0]
    return base[torch.arange(B, device=base.device) % P]


def residue_counts(s, P):
    """n_r = sum of s_b over the images b = r mod P, as float64 (P,)."""
    B = s.numel()
    r = torch.arange(B, device=s.device) % P
    return torch.zeros(P, dtype=torch.float64, device=s.device).index_add_(0, r, s.double())


def structured_wgrad64(base_x, base_g, s, Co, pad):
    """The fp64 weight gradient of x = tile_images(base_x, B), dy[b] = s_b * base_g[b mod P], and its sum of |products|, from P
    single-image gradients: sum_r n_r dW_r."""
    P = base_x.shape[0]
    n = residue_counts(s, P)
    ref = sum(n[r] * wgrad64(base_x[r:r + 1], base_g[r:r + 1], Co, pad) for r in range(P))
    mag = sum(n[r] * wgrad64(base_x[r:r + 1].abs(), base_g[r:r + 1].abs(), Co, pad) for r in range(P))
    return ref, mag


def compare_periodic(z, ref, mag, images_per_chunk=64):
    """Worst relative error of every image z[b] against ref[b mod P] (fp64, (P, ...)), over mag[b mod P]; walks z in chunks of whole
    periods so that the fp64 copies stay small.  A NaN left anywhere in z makes the result NaN."""
    P, B = ref.shape[0], z.shape[0]
    step = P * max(1, images_per_chunk // P)
    worst = torch.zeros((), dtype=torch.float64, device=z.device)
    inv = 1.0 / mag.clamp_min(1e-30)
    for b0 in range(0, B, step):
        zc = z[b0:b0 + step]
        n = zc.shape[0]
        full, rem = divmod(n, P)
        if full:
            e = ((zc[:full * P].view(full, P, *z.shape[1:]).double() - ref).abs() * inv).amax()
            worst = torch.maximum(worst, e)          # (amax and maximum both propagate NaN)
        if rem:
            e = ((zc[full * P:].double() - ref[:rem]).abs() * inv[:rem]).amax()
            worst = torch.maximum(worst, e)          # (amax and maximum both propagate NaN)
    return float(worst)
